/*
 * test_zip_large_plan.cpp - the host arithmetic of libdeflate_amd_zip_read_large
 * (csrc/zip_large_plan.h) on the CPU, against a plain serial model: which
 * entries go to the many-wave decoder, which are cut into pieces and how, what
 * is left of the sibling's columns, the runs of rows that stay with the
 * sibling's final kernel, and every refusal.  Stand-alone:
 * tests/test_zip_large_plan.py builds it with the host compiler under the
 * address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zip_large_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Row { uint64_t w[8]; };

static Row row(uint64_t rec, uint64_t name, uint64_t method, uint64_t flags, uint64_t crc,
	       uint64_t data_off, uint64_t csize, uint64_t usize)
{
	return Row{ { rec, name, method | flags << 16, crc, data_off, csize, usize, 12345 } };
}

static bool plan(const std::vector<Row> &rows, const std::vector<uint64_t> &sel, uint64_t n,
		 uint64_t avail, uint64_t align, uint64_t large_min, uint64_t piece, ZipLargePlan &p,
		 std::vector<uint64_t> &offs, uint64_t *total, std::string &err)
{
	offs.assign(sel.size() + 1, ~0ull);
	return zip_plan_read_large(rows.empty() ? NULL : rows[0].w, rows.size(), sel.size(),
				   sel.empty() ? NULL : sel.data(), n, avail, align - 1, large_min,
				   piece, p, offs.data(), total, err);
}

/* the rows of a file of n bytes for one piece size: deflated and stored
 * entries at piece - 1, piece, piece + 1, 3 * piece and 0 bytes, csizes on
 * both sides of every large_min, and the three kinds of refused row */
static std::vector<Row> make_rows(uint64_t piece, uint64_t n)
{
	std::vector<Row> rows;
	uint64_t rec = n - 4000, at = 0, k = 0;
	const uint64_t usizes[] = { piece - 1, piece, piece + 1, 3 * piece, 0 };
	const uint64_t csizes[] = { 0, 1, 99, 100, 101, 5000 };

	for (uint64_t us : usizes) {
		for (uint64_t cs : csizes) {	/* deflated: csize is free */
			rows.push_back(row(rec, 1, 8, 0, 0x1000 + k, at, cs, us));
			rec += 47, at += cs, k++;
		}
		rows.push_back(row(rec, 1, 0, 0, 0x2000 + k, at, us, us));	/* stored */
		rec += 47, at += us, k++;
	}
	rows.push_back(row(rec, 1, 12, 0, 1, at, 3 * piece, 3 * piece));	/* method 12 */
	rows.push_back(row(rec + 47, 1, 8, 1, 2, at, 4999, 3 * piece));	/* encrypted */
	rows.push_back(row(rec + 94, 1, 0, 0, 3, at, 3 * piece, 3 * piece + 1));	/* stored, sizes differ */
	return rows;
}

static void check_selection(const std::vector<Row> &rows, const std::vector<uint64_t> &sel,
			    uint64_t n, uint64_t align, uint64_t large_min, uint64_t piece)
{
	const size_t S = sel.size();
	ZipLargePlan p;
	std::vector<uint64_t> offs, offs0, cols0;
	std::string err;
	uint64_t total = ~0ull, total0 = ~0ull;

	CHECK(plan(rows, sel, n, ~0ull, align, large_min, piece, p, offs, &total, err));
	/* the sibling's plan of the same selection */
	offs0.assign(S + 1, ~0ull);
	CHECK(zip_plan_read(rows[0].w, rows.size(), S, S ? sel.data() : NULL, n, ~0ull, align - 1,
			    cols0, offs0.data(), &total0, err));
	CHECK(offs == offs0 && total == total0);
	CHECK(p.cols.size() == ZIP_COLS * S && p.own.size() == ZIPL_COLS * p.n_own &&
	      p.pieces.size() == ZIPP_COLS * p.n_pieces);

	/* the serial model */
	const uint64_t L = p.n_own, P = p.n_pieces;
	uint64_t j = 0, pc = 0, many = 0;
	std::vector<uint64_t> runs;
	for (size_t r = 0; r < S; r++) {
		const uint64_t *w = rows[sel[r]].w;
		const bool live = zip_row_result(w) == 0, defl = live && (w[2] & 0xFFFF) == 8;
		const bool mw = defl && w[5] >= large_min, pcd = live && w[6] > piece;
		const bool owned = mw || pcd;
#define COL(a) p.cols[(a) * S + r]
#define COL0(a) cols0[(a) * S + r]
		CHECK(COL(ZIP_COL_OUT_OFF) == COL0(ZIP_COL_OUT_OFF));
		CHECK(COL(ZIP_COL_META) == (COL0(ZIP_COL_META) | (uint64_t)owned << ZIPL_OWNED));
		CHECK(COL(ZIP_COL_IN_OFF) == (mw ? 0 : COL0(ZIP_COL_IN_OFF)));
		CHECK(COL(ZIP_COL_IN_N) == (mw ? 0 : COL0(ZIP_COL_IN_N)));
		CHECK(COL(ZIP_COL_OUT_AV) == (mw ? 0 : COL0(ZIP_COL_OUT_AV)));
		CHECK(COL(ZIP_COL_CP_SRC) == (pcd ? 0 : COL0(ZIP_COL_CP_SRC)));
		CHECK(COL(ZIP_COL_CP_LEN) == (pcd ? 0 : COL0(ZIP_COL_CP_LEN)));
		CHECK(COL(ZIP_COL_CRC_N) == (pcd ? 0 : COL0(ZIP_COL_CRC_N)));
		if (!owned) {
			if (runs.empty() || runs[runs.size() - 2] + runs.back() != r) {
				runs.push_back(r);
				runs.push_back(0);
			}
			runs.back()++;
			continue;
		}
		CHECK(j < L);
		if (j >= L)
			break;
#define OWN(a) p.own[(a) * L + j]
		CHECK(OWN(ZIPL_COL_SEL) == r);
		CHECK(OWN(ZIPL_COL_FLAGS) == ((mw ? ZIPL_MANY_WAVE : 0u) | (pcd ? ZIPL_PIECED : 0u)));
		CHECK(OWN(ZIPL_COL_IN_OFF) == w[4] && OWN(ZIPL_COL_IN_N) == w[5]);
		CHECK(OWN(ZIPL_COL_OUT_OFF) == offs[r] && OWN(ZIPL_COL_USIZE) == w[6]);
		CHECK(OWN(ZIPL_COL_RES) == 0 && OWN(ZIPL_COL_AIN) == 0);
		many += mw;
		if (!pcd) {
			CHECK(OWN(ZIPL_COL_FIRST) == 0 && OWN(ZIPL_COL_COUNT) == 0);
		} else {
			/* its pieces tile [0, usize) in order: full ones, then at most
			 * one shorter, never an empty one */
			const uint64_t cnt = OWN(ZIPL_COL_COUNT);
			CHECK(OWN(ZIPL_COL_FIRST) == pc);
			CHECK(cnt == w[6] / piece + (w[6] % piece != 0) && cnt >= 2);
			CHECK(pc + cnt <= P);
			uint64_t at = 0;
			for (uint64_t i = 0; i < cnt && pc + i < P; i++) {
				const uint64_t q = pc + i;
				const uint64_t len = p.pieces[ZIPP_COL_LEN * P + q];
				CHECK(len >= 1 && len <= piece);
				CHECK(len == piece || i == cnt - 1);
				CHECK(p.pieces[ZIPP_COL_DST * P + q] == offs[r] + at);
				CHECK(p.pieces[ZIPP_COL_SRC * P + q] == (defl ? 0 : w[4] + at));
				CHECK(p.pieces[ZIPP_COL_CP * P + q] == (defl ? 0 : len));
				at += len;
			}
			CHECK(at == w[6]);
			if (w[6] % piece == 0)
				CHECK(p.pieces[ZIPP_COL_LEN * P + pc + cnt - 1] == piece);
			pc += cnt;
		}
		j++;
	}
	CHECK(j == L && pc == P && many == p.n_many);
	CHECK(p.runs == runs);
	/* exactly that much room is enough, one byte less is not */
	CHECK(plan(rows, sel, n, total, align, large_min, piece, p, offs, NULL, err));
	if (total) {
		CHECK(!plan(rows, sel, n, total - 1, align, large_min, piece, p, offs, NULL, err));
		CHECK(err.find("out_avail") != std::string::npos);
	}
}

int main(void)
{
	const uint64_t n = 1000000;
	ZipLargePlan p;
	std::vector<uint64_t> offs;
	std::string err;

	for (uint64_t piece : { 1ull, 7ull, 4096ull }) {
		const std::vector<Row> rows = make_rows(piece, n);
		const size_t m = rows.size();
		for (size_t k = 0; k < m; k++)
			CHECK(zip_row_check(rows[k].w, n) == NULL);
		std::vector<uint64_t> all, rev, twice, stored3, big3;
		for (size_t k = 0; k < m; k++) {
			all.push_back(k);
			rev.push_back(m - 1 - k);
			/* 3 * piece, deflated with csize 5000 and stored */
			if (rows[k].w[6] == 3 * piece && rows[k].w[5] == 5000 && (rows[k].w[2] & 0xFFFF) == 8)
				big3.push_back(k);
			if (rows[k].w[6] == 3 * piece && rows[k].w[2] == 0 && rows[k].w[5] == rows[k].w[6])
				stored3.push_back(k);
		}
		CHECK(big3.size() == 1 && stored3.size() == 1);
		/* duplicates: the same large entry twice, side by side and apart */
		twice = { big3[0], big3[0], 0, stored3[0], big3[0], stored3[0], stored3[0] };
		const std::vector<std::vector<uint64_t>> sels = {
			{}, all, rev, twice, { big3[0] }, { stored3[0] }, { 0 }, { m - 1, m - 2, m - 3 },
		};
		for (uint64_t large_min : { 1ull, 100ull, 1ull << 40 })
			for (uint64_t align = 1; align <= 256; align *= 2)
				for (const auto &sel : sels)
					check_selection(rows, sel, n, align, large_min, piece);
		/* two independent sets of pieces at two places */
		CHECK(plan(rows, { big3[0], big3[0] }, n, ~0ull, 16, 100, piece, p, offs, NULL, err));
		CHECK(p.n_own == 2 && p.n_many == 2 && p.n_pieces == 6 && p.runs.empty());
		CHECK(p.own[ZIPL_COL_FIRST * 2 + 0] == 0 && p.own[ZIPL_COL_FIRST * 2 + 1] == 3);
		CHECK(p.pieces[ZIPP_COL_DST * 6 + 0] == 0);
		CHECK(p.pieces[ZIPP_COL_DST * 6 + 3] == offs[1] && offs[1] == (3 * piece + 15) / 16 * 16);
		/* nothing large: the sibling's columns, one run, no tables */
		CHECK(plan(rows, { 0, 1, 2 }, n, ~0ull, 1, 1ull << 40, piece, p, offs, NULL, err));
		CHECK(p.n_own == 0 && p.n_pieces == 0 && p.n_many == 0);
		CHECK(p.runs == (std::vector<uint64_t>{ 0, 3 }));
	}

	/* every refusal: the sibling's, through this plan */
	{
		std::vector<Row> rows = make_rows(7, n);
		const uint64_t m = rows.size();
		CHECK(!plan(rows, { 0, m }, n, 1 << 20, 1, 100, 7, p, offs, NULL, err));
		CHECK(err.find("sel[1] = ") != std::string::npos);
		CHECK(!plan(rows, { m - 1 }, rows[m - 1].w[0] + 46, 1 << 20, 1, 100, 7, p, offs, NULL, err));
		CHECK(err.find("in_nbytes") != std::string::npos);
		CHECK(!plan(rows, { 3 }, rows[3].w[4] + rows[3].w[5] - 1, 1 << 20, 1, 100, 7, p, offs, NULL,
			    err));
		CHECK(err.find("in_nbytes") != std::string::npos);
		rows[1].w[6] = 1ull << 32;
		CHECK(!plan(rows, { 1 }, n, ~0ull, 1, 100, 7, p, offs, NULL, err));
		CHECK(err.find("4 GiB") != std::string::npos);
		rows[1].w[6] = 5;
		rows[1].w[3] = 1ull << 32;
		CHECK(!plan(rows, { 1 }, n, ~0ull, 1, 100, 7, p, offs, NULL, err));
		CHECK(err.find("32-bit") != std::string::npos);
		rows[1].w[3] = 0;
		rows[1].w[1] = 0x10000;
		CHECK(!plan(rows, { 1 }, n, ~0ull, 1, 100, 7, p, offs, NULL, err));
		CHECK(err.find("central record") != std::string::npos);
		rows[1].w[1] = 1;
		CHECK(plan(rows, { 1 }, n, ~0ull, 1, 100, 7, p, offs, NULL, err));
		/* a piece of 0 bytes tiles nothing */
		CHECK(!plan(rows, { 1 }, n, ~0ull, 1, 100, 0, p, offs, NULL, err));
		CHECK(err.find("piece") != std::string::npos);
		/* a refused plan leaves no table behind */
		CHECK(!plan(rows, { 4, m }, n, ~0ull, 1, 1, 7, p, offs, NULL, err));
		CHECK(p.n_own == 0 && p.own.empty() && p.pieces.empty() && p.runs.empty());
	}
	/* the largest entry there is at the real piece size: 4096 pieces, the last
	 * one a byte short; offsets near 2^64 do not wrap */
	{
		std::vector<Row> rows = { row(0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF) };
		CHECK(plan(rows, { 0, 0, 0 }, 1ull << 36, ~0ull, 256, 1 << 20, 1 << 20, p, offs, NULL, err));
		CHECK(offs[3] == 3 * (1ull << 32) && p.n_own == 3 && p.n_pieces == 3 * 4096);
		CHECK(p.pieces[ZIPP_COL_LEN * p.n_pieces + 4095] == (1 << 20) - 1);
		CHECK(p.pieces[ZIPP_COL_DST * p.n_pieces + 4096] == 1ull << 32);
		CHECK(!plan(rows, { 0, 0, 0 }, 1ull << 36, 3 * (1ull << 32) - 1, 256, 1 << 20, 1 << 20, p,
			    offs, NULL, err));
	}

	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("zip large plan ok\n");
	return 0;
}
