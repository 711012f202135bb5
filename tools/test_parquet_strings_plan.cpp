/*
 * test_parquet_strings_plan.cpp - the host arithmetic that
 * libdeflate_amd_parquet_decode_batch_ex adds (csrc/parquet_strings_plan.h) on
 * the CPU: its refusals with row and reason, rows without the BYTE_ARRAY bit
 * planned exactly as pq_plan_build() plans them, and over random mixes of rows
 * the plan against a serial model - which sections are walked, the start lists
 * disjoint and of min(count, bytes / 4) + 1 words, the two slot prefixes, the
 * tile counts at their edges, the tile-sum area and the verdict columns.
 * Stand-alone: tests/test_parquet_strings_plan.py builds it with the host
 * compiler under the address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parquet_strings_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<uint64_t> Rows;

static uint64_t fields(uint64_t kind, uint64_t enc, uint64_t packed, uint64_t max_def, uint64_t width,
		       uint64_t str = 0)
{
	return kind | enc << 4 | packed << 12 | max_def << 13 | (width - 1) << 16 | (str ? PQ_BYTE_ARRAY : 0);
}

static void row(Rows &r, uint64_t off, uint64_t csize, uint64_t usize, uint64_t f, uint64_t count,
		uint64_t def_len = 0, uint64_t out = 0, uint64_t valid = 0, uint64_t dict = 0)
{
	const uint64_t x[PQ_WORDS] = { off, csize, usize, f, count | def_len << 32, out, valid, dict };
	r.insert(r.end(), x, x + PQ_WORDS);
}

struct Call {
	uint64_t in_n = 100, out_n = 400, valid_n = 50, bytes_avail = 10, flags = 0;
	bool have_valid = true, have_bytes = true, have_total = true;
	int format = 2;
};

static bool check(const Rows &r, const Call &c, std::string &err, Rows &masked)
{
	return pqs_check(c.format, r.size() / PQ_WORDS, r.data(), c.in_n, c.out_n, c.valid_n, c.have_valid,
			 c.have_bytes, c.bytes_avail, c.have_total, c.flags, masked, err);
}

static bool refused(const Rows &r, const Call &c, const char *word, long long at_row)
{
	std::string err;
	Rows masked;
	if (check(r, c, err, masked))
		return false;
	char want[40];
	snprintf(want, sizeof(want), "row %lld:", at_row);
	const bool ok = err.find(word) != std::string::npos &&
			(at_row < 0 || err.find(want) != std::string::npos);
	if (!ok)
		printf("got: %s\n", err.c_str());
	return ok;
}

/* in_nbytes 100, out_avail 400, valid_avail 50: a string dictionary, a string
 * page coded with it, a PLAIN string page, a fixed-width page */
static Rows good(void)
{
	Rows ok;
	row(ok, 0, 20, 40, fields(PQ_DICT, PQ_PLAIN, 1, 0, 1, 1), 5);
	row(ok, 20, 30, 90, fields(PQ_DATA_V1, PQ_RLE_DICTIONARY, 1, 1, 1, 1), 20, 0, 0, 0, 0);	/* entries 0 .. 168 */
	row(ok, 50, 40, 40, fields(PQ_DATA_V2, PQ_PLAIN, 0, 1, 1, 1), 6, 3, 168, 30);		/* entries 168 .. 224 */
	row(ok, 90, 10, 10, fields(PQ_DATA_V1, PQ_PLAIN, 0, 0, 5), 2, 0, 390, 99, 99);		/* slots 390 .. 400 */
	return ok;
}

static void refusals(void)
{
	std::string err;
	Rows masked;
	const Rows ok = good();
	const Call c;
	CHECK(check(ok, c, err, masked));
	CHECK(masked.size() == ok.size());
	for (size_t r = 0; r < 4; r++)
		for (size_t w = 0; w < PQ_WORDS; w++)
			CHECK(masked[PQ_WORDS * r + w] == (w == PQ_W_FIELDS ? ok[PQ_WORDS * r + w] & ~PQ_BYTE_ARRAY
									     : ok[PQ_WORDS * r + w]));
	CHECK(check(Rows(), c, err, masked));
	/* the old call refuses the bit */
	CHECK(!pq_check(2, 4, ok.data(), 100, 400, 50, true, err) && err.find("unknown bits") != std::string::npos);
	Call k = c;
	k.flags = 1;
	CHECK(refused(ok, k, "flags", -1));
	k = c, k.have_bytes = false;
	CHECK(refused(ok, k, "d_bytes is NULL", -1));
	k.bytes_avail = 0;
	CHECK(check(ok, k, err, masked));		/* the sizing call */
	k = c, k.have_total = false;
	CHECK(refused(ok, k, "d_bytes_total is NULL", 0));
	k = c, k.format = 3;
	CHECK(refused(ok, k, "format", -1));
	k = c, k.out_n = 399;
	CHECK(refused(ok, k, "out_avail", 3));
	k = c, k.have_valid = false;
	CHECK(refused(ok, k, "d_valid is NULL", 1));
	{	/* without a string row d_bytes_total may be NULL */
		Rows one;
		row(one, 90, 10, 10, fields(PQ_DATA_V1, PQ_PLAIN, 0, 0, 5), 2, 0, 390);
		k = c, k.have_total = false;
		CHECK(check(one, k, err, masked));
	}
	/* (at: the row the refusal names, where that is not r) */
	struct { size_t r, word; uint64_t value; const char *why; long long at; } bad[] = {
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 2, 1), "non-zero width field" },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, 0, 1, 0, 256, 1), "non-zero width field" },
		{ 1, PQ_W_OUT, 4, "not a multiple of 8" },
		{ 2, PQ_W_OUT, 169, "not a multiple of 8" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 1, 0), "BYTE_ARRAY on one side only" },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, 0, 1, 0, 1, 0), "BYTE_ARRAY on one side only", 1 },
		{ 0, PQ_W_FIELDS, fields(PQ_DICT, 0, 1, 0, 4, 0), "BYTE_ARRAY on one side only", 1 },
		{ 1, PQ_W_OUT, 240, "offsets do not lie inside out_avail" },	/* 240 + 21 * 8 > 400 */
		{ 2, PQ_W_OUT, 392, "offsets do not lie inside out_avail" },	/* (6 slots of width 1 would fit) */
		{ 1, PQ_W_OUT, ~(uint64_t)0 - 7, "out_avail" },
		{ 1, PQ_W_FIELDS, fields(PQ_DATA_V1, 8, 1, 1, 1, 1) | (uint64_t)1 << 15, "unknown bits" },
		{ 2, PQ_W_FIELDS, fields(PQ_DATA_V2, 3, 0, 1, 1, 1), "an encoding" },
		{ 1, PQ_W_DICT, 1, "not an earlier row" },
		{ 2, PQ_W_VALID, 45, "valid_avail" },
		{ 2, PQ_W_OFF, 61, "in_nbytes" },
	};
	for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) {
		Rows r = ok;
		r[PQ_WORDS * bad[i].r + bad[i].word] = bad[i].value;
		if (!refused(r, c, bad[i].why, bad[i].at ? bad[i].at : (long long)bad[i].r)) {
			printf("FAILED refusal %zu (%s)\n", i, bad[i].why);
			failures++;
		}
	}
	{	/* count + 1 entries: 23 * 8 + 216 = 400 fits, 24 do not */
		Rows r = ok;
		r[PQ_WORDS * 1 + PQ_W_OUT] = 216;
		r[PQ_WORDS * 1 + PQ_W_COUNT] = 22;
		r[PQ_WORDS * 2 + PQ_W_OUT] = 0;
		CHECK(check(r, c, err, masked));
		r[PQ_WORDS * 1 + PQ_W_COUNT] = 23;
		CHECK(refused(r, c, "offsets do not lie inside out_avail", 1));
	}
}

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd(uint64_t n)
{
	rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
	return rnd_state % n;
}

/* rows without the bit: pq_plan_build()'s plan, and nothing for the strings */
static void fixed_rows_are_planned_as_before(void)
{
	Rows r;
	std::string err;
	Rows masked;
	row(r, 0, 20, 40, fields(PQ_DICT, PQ_PLAIN, 1, 0, 4), 10);
	row(r, 20, 30, 90, fields(PQ_DATA_V1, PQ_RLE_DICTIONARY, 1, 1, 4), 50, 0, 0, 0, 0);
	row(r, 50, 40, 40, fields(PQ_DATA_V2, PQ_PLAIN, 0, 1, 8), 20, 3, 200, 30);
	row(r, 90, 10, 10, fields(PQ_DATA_V1, PQ_PLAIN, 0, 0, 5), 2, 0, 390, 99, 99);
	Call c;
	c.have_total = c.have_bytes = false, c.bytes_avail = 0;
	CHECK(check(r, c, err, masked) && masked == r);
	pq_plan old;
	pqs_plan p;
	pq_plan_build(4, r.data(), old);
	pqs_plan_build(4, r.data(), masked.data(), p);
	CHECK(p.n_w == 0 && p.n_s == 0 && p.slots == 0 && p.tiles == 0 && p.walk_words == 0);
	CHECK(p.sum_words == 1);
	CHECK(p.base.slots == old.slots && p.base.tiles == old.tiles && p.base.n_u == old.n_u &&
	      p.base.n_z == old.n_z && p.base.room_bytes == old.room_bytes &&
	      p.base.run_records == old.run_records && p.base.u_at == old.u_at && p.base.v_at == old.v_at);
	CHECK(p.base.cols.size() == old.cols.size() + PQS_VCOLS * 4);
	CHECK(std::equal(old.cols.begin(), old.cols.end(), p.base.cols.begin()));
	for (size_t k = old.cols.size(); k < p.base.cols.size(); k++)
		CHECK(p.base.cols[k] == 0);
}

/* random mixes against a serial model */
static void plans(void)
{
	const uint64_t counts[] = { 0, 1, 3, 4, 1023, 1024, 1025, 2048, 5000 };
	for (int round = 0; round < 300; round++) {
		const uint64_t n = 1 + rnd(40);
		Rows r;
		std::vector<long long> dict_of_type[2] = { { -1 }, { -1 } };	/* the latest dictionary row */
		uint64_t off = 0, out = 0, valid = 0;
		for (uint64_t k = 0; k < n; k++) {
			const uint64_t str = rnd(3) != 0, packed = rnd(2), count = counts[rnd(9)];
			const uint64_t usize = rnd(4) ? 4 * count + rnd(64) : rnd(4 * count + 1);
			const uint64_t csize = packed ? 1 + rnd(50) : usize;
			const uint64_t what = rnd(4);
			if (what == 0) {
				row(r, off, csize, usize, fields(PQ_DICT, PQ_PLAIN, packed, 0, str ? 1 : 4, str), count);
				dict_of_type[str][0] = (long long)k;
			} else {
				const bool coded = what == 1 && dict_of_type[str][0] >= 0;
				const uint64_t v2 = rnd(2), max_def = rnd(2);
				const uint64_t def_len = v2 && max_def ? rnd((usize < csize ? usize : csize) + 1) : 0;
				out = (out + 7) & ~(uint64_t)7;
				row(r, off, csize, usize,
				    fields(v2 ? PQ_DATA_V2 : PQ_DATA_V1, coded ? PQ_RLE_DICTIONARY : PQ_PLAIN, packed,
					   max_def, str ? 1 : 4, str),
				    count, def_len, out, valid, coded ? (uint64_t)dict_of_type[str][0] : 0);
				out += str ? (count + 1) * 8 : count * 4;
				valid += max_def ? count : 0;
			}
			off += csize;
		}
		std::string err;
		Rows masked;
		Call c;
		c.in_n = off, c.out_n = out, c.valid_n = valid;
		if (!check(r, c, err, masked)) {
			printf("FAILED round %d: %s\n", round, err.c_str());
			failures++;
			continue;
		}
		pqs_plan p;
		pq_plan all;
		pqs_plan_build(n, r.data(), masked.data(), p);
		pq_plan_build(n, masked.data(), all);
		const pq_plan &b = p.base;
		const uint64_t *w = b.cols.data() + p.w_at, *s = b.cols.data() + p.s_at, *v = b.cols.data() + p.v_at;
		const uint64_t *u = b.cols.data() + b.u_at, *au = all.cols.data() + all.u_at;
		/* the base plan is the masked rows' but for the expand kernel's prefix */
		CHECK(b.n_u == all.n_u && b.n_z == all.n_z && b.u_at == all.u_at && b.v_at == all.v_at);
		CHECK(std::equal(all.cols.begin() + all.u_at + all.n_u, all.cols.end(), b.cols.begin() + b.u_at + b.n_u));
		CHECK(std::equal(all.cols.begin(), all.cols.begin() + all.u_at, b.cols.begin()));
		uint64_t n_w = 0, n_s = 0, n_u = 0, fixed = 0, strs = 0, starts = 0;
		std::vector<uint64_t> walk_of(n, ~(uint64_t)0);
		for (uint64_t k = 0; k < n; k++) {
			const uint64_t *x = r.data() + PQ_WORDS * k;
			const pq_page t = pq_page_of(masked.data() + PQ_WORDS * k);
			const bool str = x[PQ_W_FIELDS] & PQ_BYTE_ARRAY;
			const bool walked = str && (!t.data || !t.dict_coded);
			if (walked) {
				const uint64_t bytes = t.usize - t.def_len;
				const uint64_t cap = (t.count < bytes / 4 ? t.count : bytes / 4) + 1;
				CHECK(n_w < p.n_w);
				CHECK(w[PQS_W_SEC_N * p.n_w + n_w] == bytes && w[PQS_W_COUNT * p.n_w + n_w] == t.count);
				CHECK(w[PQS_W_STARTS * p.n_w + n_w] == 2 * p.n_w + starts && w[PQS_W_CAP * p.n_w + n_w] == cap);
				CHECK(w[PQS_W_Z * p.n_w + n_w] == b.cols[b.v_at + PQ_V_Z * n + k]);
				CHECK(w[PQS_W_U * p.n_w + n_w] == (t.data ? n_u + 1 : 0));
				if (t.data)
					CHECK(w[PQS_W_SEC * p.n_w + n_w] == au[PQ_U_SEC * all.n_u + n_u]);
				else if (!t.compressed)
					CHECK(w[PQS_W_SEC * p.n_w + n_w] == (PQ_IN_PLACE | t.off));
				starts += cap;
				walk_of[k] = n_w++;
			}
			CHECK(v[PQS_V_WALK * n + k] == (walked ? walk_of[k] + 1 : 0));
			if (!t.data) {
				CHECK(v[PQS_V_S * n + k] == 0 && v[PQS_V_DWALK * n + k] == 0);
				continue;
			}
			if (str) {
				strs += t.count;
				CHECK(n_s < p.n_s);
				CHECK(s[PQS_S_SLOT_END * p.n_s + n_s] == strs && s[PQS_S_U * p.n_s + n_s] == n_u);
				const uint64_t from = t.dict_coded ? x[PQ_W_DICT] : k;
				CHECK(walk_of[from] != ~(uint64_t)0 && s[PQS_S_WALK * p.n_s + n_s] == walk_of[from]);
				CHECK(s[PQS_S_STARTS * p.n_s + n_s] == w[PQS_W_STARTS * p.n_w + walk_of[from]]);
				if (t.dict_coded)	/* the dictionary's section is the one the data page names */
					CHECK(w[PQS_W_SEC * p.n_w + walk_of[from]] == au[PQ_U_DICT * all.n_u + n_u]);
				CHECK(v[PQS_V_DWALK * n + k] == (t.dict_coded ? walk_of[from] + 1 : 0));
				n_s++;
			} else {
				fixed += t.count;
				CHECK(v[PQS_V_DWALK * n + k] == 0);
			}
			CHECK(v[PQS_V_S * n + k] == (str ? n_s : 0));
			CHECK(u[PQ_U_SLOT_END * b.n_u + n_u] == fixed);
			n_u++;
		}
		CHECK(n_w == p.n_w && n_s == p.n_s && n_u == b.n_u && starts == p.start_words);
		CHECK(p.walk_words == 2 * p.n_w + starts);
		CHECK(p.slots == strs && b.slots == fixed && strs + fixed == all.slots);
		CHECK(p.tiles * PQ_TILE >= strs && (p.tiles == 0 || (p.tiles - 1) * PQ_TILE < strs));
		CHECK(b.tiles * PQ_TILE >= fixed && (b.tiles == 0 || (b.tiles - 1) * PQ_TILE < fixed));
		CHECK(p.sum_words == 2 * p.tiles + (p.tiles + PQS_SCAN_BLOCK - 1) / PQS_SCAN_BLOCK + 1);
		CHECK(p.v_at + PQS_VCOLS * n == b.cols.size());
	}
}

int main(void)
{
	refusals();
	fixed_rows_are_planned_as_before();
	plans();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("parquet strings plan ok\n");
	return 0;
}
