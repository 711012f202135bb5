/*
 * test_parquet_plan.cpp - the host arithmetic of
 * libdeflate_amd_parquet_decode_batch (csrc/parquet_plan.h) on the CPU: every
 * refusal with its row and reason, and the plan against a serial model - the
 * class of every row, the rooms on 16-byte boundaries and disjoint, the decode
 * batch's columns, the data pages' columns, the run lists disjoint and large
 * enough for the worst stream, the slot prefix and the tile count at its edges,
 * the verdict words.  Stand-alone: tests/test_parquet_plan.py builds it with
 * the host compiler under the address and undefined-behaviour sanitizers and
 * runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parquet_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<uint64_t> Rows;

static uint64_t fields(uint64_t kind, uint64_t enc, uint64_t packed, uint64_t max_def, uint64_t width)
{
	return kind | enc << 4 | packed << 12 | max_def << 13 | (width - 1) << 16;
}

static void row(Rows &r, uint64_t off, uint64_t csize, uint64_t usize, uint64_t f, uint64_t count,
		uint64_t def_len = 0, uint64_t out = 0, uint64_t valid = 0, uint64_t dict = 0)
{
	const uint64_t x[PQ_WORDS] = { off, csize, usize, f, count | def_len << 32, out, valid, dict };
	r.insert(r.end(), x, x + PQ_WORDS);
}

static bool refused(const Rows &r, uint64_t in_n, uint64_t out_n, uint64_t valid_n, bool have_valid,
		    const char *word, long long at_row, int format = 2)
{
	std::string err;
	if (pq_check(format, r.size() / PQ_WORDS, r.data(), in_n, out_n, valid_n, have_valid, err))
		return false;
	char want[40];
	snprintf(want, sizeof(want), "row %lld:", at_row);
	return err.find(word) != std::string::npos && (at_row < 0 || err.find(want) != std::string::npos);
}

/* in_nbytes 100, out_avail 400, valid_avail 50 */
static Rows good(void)
{
	Rows ok;
	row(ok, 0, 20, 40, fields(PQ_DICT, PQ_PLAIN, 1, 0, 4), 10);			/* 10 entries of 4 */
	row(ok, 20, 30, 90, fields(PQ_DATA_V1, PQ_RLE_DICTIONARY, 1, 1, 4), 50, 0, 0, 0, 0);	/* slots 0 .. 200 */
	row(ok, 50, 40, 40, fields(PQ_DATA_V2, PQ_PLAIN, 0, 1, 8), 20, 3, 200, 30);	/* slots 200 .. 360, valid 30 .. 50 */
	row(ok, 90, 10, 10, fields(PQ_DATA_V1, PQ_PLAIN, 0, 0, 5), 2, 0, 390, 99, 99);	/* slots 390 .. 400 */
	return ok;
}

static void refusals(void)
{
	std::string err;
	const Rows ok = good();
	CHECK(pq_check(2, 4, ok.data(), 100, 400, 50, true, err));
	CHECK(pq_check(0, 4, ok.data(), 100, 400, 50, true, err) && pq_check(1, 4, ok.data(), 100, 400, 50, true, err));
	CHECK(pq_check(2, 0, NULL, 0, 0, 0, false, err));
	CHECK(refused(ok, 100, 400, 50, true, "format", -1, 3) && refused(ok, 100, 400, 50, true, "format", -1, -1));
	CHECK(!pq_check(2, PQ_MAX_PAGES + 1, ok.data(), 100, 400, 50, true, err) &&
	      err.find("n_pages") != std::string::npos);
	CHECK(refused(ok, 99, 400, 50, true, "in_nbytes", 3));
	CHECK(refused(ok, 100, 399, 50, true, "out_avail", 3));
	CHECK(refused(ok, 100, 359, 50, true, "out_avail", 2));
	CHECK(refused(ok, 100, 400, 49, true, "valid_avail", 1));
	CHECK(refused(ok, 100, 400, 50, false, "d_valid is NULL", 1));
	struct { size_t r, word; uint64_t value; const char *why; } bad[] = {
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 4) | (uint64_t)1 << 24, "unknown bits" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 4) | (uint64_t)1 << 14, "unknown bits" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 4) | (uint64_t)1 << 15, "unknown bits" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 4) | (uint64_t)1 << 63, "unknown bits" },
		{ 3, PQ_W_FIELDS, fields(1, 0, 0, 0, 5), "a kind" },
		{ 3, PQ_W_FIELDS, fields(4, 0, 0, 0, 5), "a kind" },
		{ 3, PQ_W_FIELDS, fields(15, 0, 0, 0, 5), "a kind" },
		{ 3, PQ_W_FIELDS, fields(PQ_DATA_V1, 1, 0, 0, 5), "an encoding" },
		{ 3, PQ_W_FIELDS, fields(PQ_DATA_V1, 3, 0, 0, 5), "an encoding" },
		{ 3, PQ_W_FIELDS, fields(PQ_DATA_V1, 255, 0, 0, 5), "an encoding" },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, PQ_RLE_DICTIONARY, 1, 0, 4), "dictionary encoding on a dictionary page" },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, PQ_PLAIN_DICTIONARY, 1, 0, 4), "dictionary encoding on a dictionary page" },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, PQ_PLAIN, 1, 1, 4), "max_def on a dictionary page" },
		{ 0, PQ_W_USIZE, (uint64_t)1 << 31, "2^31" },
		{ 0, PQ_W_CSIZE, (uint64_t)1 << 31, "2^31" },
		{ 0, PQ_W_COUNT, (uint64_t)1 << 31, "2^31" },
		{ 1, PQ_W_COUNT, 50 | (uint64_t)1 << 32, "level bytes on a row" },	/* a V1 page */
		{ 0, PQ_W_COUNT, 10 | (uint64_t)1 << 32, "level bytes on a row" },	/* a dictionary page */
		{ 2, PQ_W_COUNT, 20 | (uint64_t)41 << 32, "level bytes beyond" },
		{ 2, PQ_W_COUNT, 20 | (uint64_t)0xFFFFFFFF << 32, "level bytes beyond" },
		{ 2, PQ_W_USIZE, 41, "two sizes differ" },
		{ 3, PQ_W_CSIZE, 9, "two sizes differ" },
		{ 3, PQ_W_OFF, 91, "in_nbytes" },
		{ 3, PQ_W_OFF, ~(uint64_t)0, "in_nbytes" },
		{ 1, PQ_W_CSIZE, 81, "in_nbytes" },
		{ 1, PQ_W_DICT, 1, "not an earlier row" },
		{ 1, PQ_W_DICT, 2, "not an earlier row" },
		{ 1, PQ_W_DICT, ~(uint64_t)0, "not an earlier row" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, PQ_RLE_DICTIONARY, 1, 1, 8), "another width" },
		{ 1, PQ_W_OUT, 201, "out_avail" },
		{ 1, PQ_W_OUT, ~(uint64_t)0 - 3, "out_avail" },
		{ 2, PQ_W_VALID, 31, "valid_avail" },
		{ 2, PQ_W_VALID, ~(uint64_t)0, "valid_avail" },
	};
	for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); k++) {
		Rows r = ok;
		r[PQ_WORDS * bad[k].r + bad[k].word] = bad[k].value;
		if (!refused(r, 100, 400, 50, true, bad[k].why, (long long)bad[k].r)) {
			pq_check(2, 4, r.data(), 100, 400, 50, true, err);
			printf("FAILED: case %zu (%s) gave: %s\n", k, bad[k].why, err.c_str());
			failures++;
		}
	}
	/* a dictionary reference that is a data page */
	Rows r = ok;
	row(r, 0, 0, 0, fields(PQ_DATA_V2, PQ_PLAIN_DICTIONARY, 0, 0, 4), 0, 0, 0, 0, 3);
	CHECK(refused(r, 100, 400, 50, true, "not a dictionary page", 4));
	r[PQ_WORDS * 4 + PQ_W_DICT] = 0;
	CHECK(pq_check(2, 5, r.data(), 100, 400, 50, true, err));
	/* words a row ignores may hold anything; d_valid may be missing while no row has max_def */
	Rows q;
	row(q, 0, 20, 40, fields(PQ_DICT, PQ_PLAIN, 1, 0, 4), 10, 0, ~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0);
	row(q, 90, 10, 10, fields(PQ_DATA_V1, PQ_PLAIN, 0, 0, 5), 2, 0, 390, ~(uint64_t)0, ~(uint64_t)0);
	CHECK(pq_check(2, 2, q.data(), 100, 400, 0, false, err));
}

/* the plan against a serial restatement */
static void check_plan(const Rows &rows)
{
	const uint64_t n = rows.size() / PQ_WORDS;
	pq_plan p;
	pq_plan_build(n, rows.data(), p);
	uint64_t z = 0, u = 0, rooms = 0, slots = 0, recs = 0;
	std::vector<uint64_t> sec(n);

	CHECK(p.n == n);
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows.data() + PQ_WORDS * r;
		const uint64_t kind = w[3] & 15, enc = w[3] >> 4 & 255, packed = w[3] >> 12 & 1;
		const uint64_t max_def = w[3] >> 13 & 1, width = (w[3] >> 16 & 255) + 1;
		const uint64_t count = w[4] & 0xFFFFFFFF, def_len = w[4] >> 32, sec_n = w[2] - def_len;
		const uint64_t *v = p.cols.data() + p.v_at;
		if (packed) {
			const uint64_t *d = p.cols.data();
			CHECK(z < p.n_z);
			CHECK(d[CHUNK_D_IN_OFF * p.n_z + z] == w[0] + def_len && d[CHUNK_D_IN_N * p.n_z + z] == w[1] - def_len);
			CHECK(d[CHUNK_D_OUT_OFF * p.n_z + z] == rooms && rooms % 16 == 0);
			CHECK(d[CHUNK_D_OUT_N * p.n_z + z] == sec_n);
			sec[r] = rooms;
			rooms += (sec_n + 15) / 16 * 16;
			z++;
			CHECK(v[PQ_V_Z * n + r] == z);
		} else {
			sec[r] = PQ_IN_PLACE | (w[0] + def_len);
			CHECK(v[PQ_V_Z * n + r] == 0);
		}
		if (kind == PQ_DICT) {
			CHECK(v[PQ_V_OWN * n + r] == (PQ_V_IS_DICT | (count * width > w[2] ? 1 : 0)));
			CHECK(v[PQ_V_DICT * n + r] == 0);
			continue;
		}
		const uint64_t *c = p.cols.data() + p.u_at;
		CHECK(u < p.n_u);
		CHECK(v[PQ_V_OWN * n + r] == u);
		CHECK(v[PQ_V_DICT * n + r] == (enc ? w[7] + 1 : 0));
		slots += count;
		CHECK(c[PQ_U_SLOT_END * p.n_u + u] == slots);
		CHECK(c[PQ_U_SEC * p.n_u + u] == sec[r] && c[PQ_U_SEC_N * p.n_u + u] == sec_n);
		CHECK(c[PQ_U_LEV * p.n_u + u] == w[0] && c[PQ_U_LEV_N * p.n_u + u] == def_len);
		CHECK(c[PQ_U_COUNT * p.n_u + u] == count && c[PQ_U_OUT * p.n_u + u] == w[5] &&
		      c[PQ_U_VALID * p.n_u + u] == w[6]);
		uint64_t f = (w[3] & 0xFFFFFF) | (packed ? z : 0) << 32;
		if (enc) {
			const uint64_t *dw = rows.data() + PQ_WORDS * w[7];
			const uint64_t entries = dw[4] & 0xFFFFFFFF;
			CHECK(c[PQ_U_DICT * p.n_u + u] == sec[w[7]] && c[PQ_U_DICT_N * p.n_u + u] == entries);
			if (entries * width > dw[2])
				f |= PQ_F_SKIP;
		}
		CHECK(c[PQ_U_FIELDS * p.n_u + u] == f);
		/* the run lists: disjoint, in order, and no smaller than the most runs
		 * a stream of that many bytes can hold for that many values - a run
		 * takes a byte at least and gives a value at least -, plus the pieces */
		const uint64_t lbytes = kind == PQ_DATA_V2 ? def_len : w[2];
		const uint64_t lcap = c[PQ_U_LCAP * p.n_u + u], icap = c[PQ_U_ICAP * p.n_u + u];
		CHECK(c[PQ_U_LRUNS * p.n_u + u] == recs);
		if (max_def)
			CHECK(lcap >= (count < lbytes ? count : lbytes) + count / PQ_LEVEL_PIECE);
		else
			CHECK(lcap == 0);
		recs += lcap;
		CHECK(c[PQ_U_IRUNS * p.n_u + u] == recs);
		if (enc)
			CHECK(icap >= (count < sec_n ? count : sec_n));
		else
			CHECK(icap == 0);
		recs += icap;
		u++;
	}
	CHECK(z == p.n_z && u == p.n_u && rooms == p.room_bytes && slots == p.slots && recs == p.run_records);
	CHECK(p.tiles == (slots + PQ_TILE - 1) / PQ_TILE);
	CHECK(p.u_at == CHUNK_DCOLS * p.n_z && p.v_at == p.u_at + PQ_UCOLS * p.n_u &&
	      p.cols.size() == p.v_at + PQ_VCOLS * n);
}

static void plans(void)
{
	check_plan(good());
	check_plan(Rows());
	/* the tile table at its edges: the slots of all pages laid end to end */
	const uint64_t counts[] = { 0, 1, PQ_TILE - 1, PQ_TILE, PQ_TILE + 1, 2 * PQ_TILE + 3 };
	for (uint64_t a : counts)
		for (uint64_t b : counts) {
			Rows r;
			row(r, 0, 8, 8, fields(PQ_DICT, PQ_PLAIN, 0, 0, 4), 3);		/* too short for 3 entries */
			row(r, 8, 9, a * 4 + 100, fields(PQ_DATA_V1, PQ_PLAIN, 1, 1, 4), a, 0, 0, 0);
			row(r, 20, 30, b + 7, fields(PQ_DATA_V2, PQ_RLE_DICTIONARY, 1, 1, 4), b, 7, a * 4, a, 0);
			row(r, 50, 5, 5, fields(PQ_DATA_V2, PQ_PLAIN_DICTIONARY, 0, 0, 4), 1, 0, (a + b) * 4, 0, 0);
			std::string err;
			CHECK(pq_check(2, 4, r.data(), 100, (a + b + 1) * 4, a + b, true, err));
			check_plan(r);
			pq_plan p;
			pq_plan_build(4, r.data(), p);
			CHECK(p.slots == a + b + 1 && p.tiles == (a + b + 1 + PQ_TILE - 1) / PQ_TILE);
			CHECK(p.cols[p.u_at + PQ_U_FIELDS * 3 + 1] & PQ_F_SKIP);
			CHECK(!(p.cols[p.u_at + PQ_U_FIELDS * 3 + 0] & PQ_F_SKIP));
		}
	/* many small pages */
	Rows many;
	row(many, 0, 4, 40, fields(PQ_DICT, PQ_PLAIN, 1, 0, 8), 5);
	for (uint64_t k = 0; k < 3000; k++)
		row(many, 4 + k % 50, 20, 20 + k % 7, fields(k % 2 ? PQ_DATA_V1 : PQ_DATA_V2, k % 3 ? PQ_PLAIN : 8,
							     k % 5 != 0, k % 2, 8), k % 11, 0, 8 * k, k, 0);
	for (uint64_t k = 0; k < 3000; k++)	/* an uncompressed body has one size */
		if (!(many[PQ_WORDS * (k + 1) + 3] >> 12 & 1))
			many[PQ_WORDS * (k + 1) + 2] = 20;
	std::string err;
	CHECK(pq_check(2, 3001, many.data(), 200, 8 * 3000 + 100, 3100, true, err));
	check_plan(many);
}

int main(void)
{
	refusals();
	plans();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("parquet plan ok\n");
	return 0;
}
