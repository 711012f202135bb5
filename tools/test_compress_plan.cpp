/*
 * test_compress_plan.cpp - the arithmetic of a compress batch call
 * (csrc/compress_plan.h) on the CPU, against a plain serial model: the layout
 * of the kernels' scratch as it was before a slice had a tail, the rule that
 * says which slices have one, and the regions the tail adds.  Stand-alone:
 * tests/test_compress_plan.py builds it with the host compiler under the
 * address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "compress_plan.h"

using namespace lda;

static int failures;
static long checked;
#define CHECK(c) do { checked++; if (!(c)) { if (failures < 40) printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); failures++; } } while (0)
static char g_case[256];

/* the serial schedule's plan, stated plainly: one kernel state per workgroup,
 * four counters per slice, the sums, then the dictionary block or one slice's
 * token lists and block descriptors */
struct Model {
	bool small, split;
	size_t grid, per_slice, nslices, tok_stride, blk_stride;
	size_t cnt_at, sums_at, tok_at, blk_at, dict_at, total;
};

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static Model model(const compress_plan_env &e, size_t n, size_t max_in, int level, bool seg, bool dict)
{
	Model m = {};
	const size_t scratch = (size_t)1280 << 20, words = 8 + 320;

	m.small = max_in <= e.small_max && level <= 9 && !seg && !dict && !e.no_small;
	m.tok_stride = up(max_in, 16);
	m.blk_stride = std::max<size_t>(1, (m.tok_stride + e.tile - 1) / e.tile);
	const size_t per_buf = m.tok_stride * 4 + m.blk_stride * words * 4 + 4;
	m.split = !m.small && level <= 9 && !dict && max_in != SIZE_MAX && n >= 4 * e.num_cus &&
		  per_buf <= scratch && m.tok_stride <= 0xFFFFFFF0u;
	m.per_slice = std::max<size_t>(m.split ? std::min(n, scratch / per_buf) : n, 1);
	m.nslices = (n + m.per_slice - 1) / m.per_slice;
	m.grid = std::min(m.per_slice, e.num_cus * (m.small ? e.small_wgs : 1));
	m.cnt_at = m.grid * e.seq_words * 8;
	m.sums_at = m.cnt_at + 16 * m.nslices;
	m.dict_at = m.tok_at = up(m.sums_at + n * 4, 64);
	m.total = m.sums_at + n * 4;
	if (dict)
		m.total = m.dict_at + e.dict_bytes;
	if (m.split) {
		m.blk_at = up(m.tok_at + m.per_slice * m.tok_stride * 4, 64);
		const size_t list = (m.per_slice + 15) / 16 * 16;
		m.total = m.blk_at + (2 * list + m.per_slice * m.blk_stride * words) * 4;
	} else {
		m.tok_stride = m.blk_stride = 0;
	}
	return m;
}

struct Region { size_t lo, hi; const char *name; };

static void check_one(const compress_plan_env &e, size_t n, size_t max_in, int level, bool seg, bool dict)
{
	snprintf(g_case, sizeof(g_case), "n %zu max_in %zu level %d seg %d dict %d cus %zu R %zu", n,
		 max_in, level, (int)seg, (int)dict, e.num_cus, e.tail_rounds);
	const Model m = model(e, n, max_in, level, seg, dict);
	const batch_plan p = plan_batch(e, n, max_in, level, seg, dict);
	const size_t R = e.tail_rounds, cus = e.num_cus;

	/* which kernel, and the slices: never moved by the tail */
	CHECK(p.small == m.small && p.split == m.split);
	CHECK(p.grid == m.grid && p.per_slice == m.per_slice && p.nslices == m.nslices);
	CHECK(p.tok_stride == m.tok_stride && p.blk_stride == m.blk_stride);
	/* the rule: the first slice is the largest, so the call overlaps exactly
	 * where that one leaves its head LDA_SPLIT_MIN_PER_CU buffers per CU */
	const bool rule = m.split && R && m.per_slice >= (4 + R) * cus;
	CHECK(p.overlap == rule);
	CHECK(p.tail_max == (rule ? R * cus : 0));
	CHECK(p.grid2 == (rule ? std::min(R * cus, cus) : 0));
	if (!p.overlap) {
		/* the serial layout, value for value */
		CHECK(p.cnt_at == m.cnt_at && p.sums_at == m.sums_at && p.tok_at == m.tok_at &&
		      p.dict_at == m.dict_at && p.total == m.total);
		CHECK(!m.split || p.blk_at == m.blk_at);
		CHECK(p.seq2_at == p.cnt_at && p.cnt2_at == p.sums_at);
		CHECK(!m.split || p.blk2_at == p.total);
	}
	/* head + tail = the slice, slice after slice */
	size_t seen = 0, tails = 0;
	for (size_t k = 0; k < p.nslices; k++) {
		const size_t lo = k * p.per_slice, nk = std::min(p.per_slice, n - lo);
		const size_t tail = plan_tail_of(nk, cus, p.tail_rounds), head = nk - tail;
		const bool has = m.split && R && nk >= (4 + R) * cus;
		CHECK(tail == (has ? R * cus : 0));
		CHECK(tail <= nk && head + tail == nk);
		CHECK(!tail || head >= 4 * cus);
		CHECK(tail <= p.tail_max);
		/* the tail's token lists end inside the slice's */
		CHECK((head + tail) * (size_t)p.tok_stride <= p.per_slice * (size_t)p.tok_stride);
		if (tail && p.split) {
			const size_t need = (LDA_PLAN_BLK_HDR_WORDS(tail) + tail * p.blk_stride * LDA_PLAN_BLK_WORDS) * 4;
			CHECK(p.blk2_at + need <= p.total);
			const size_t need1 = (LDA_PLAN_BLK_HDR_WORDS(head) + head * p.blk_stride * LDA_PLAN_BLK_WORDS) * 4;
			CHECK(p.blk_at + need1 <= p.blk2_at);
			CHECK(std::min(tail, p.grid2) * e.seq_words * 8 <= p.cnt_at - p.seq2_at);
		}
		seen += nk;
		tails += tail;
	}
	CHECK(seen == n);
	CHECK((tails != 0) == (p.overlap && n != 0));
	/* the regions, in order, apart, inside total */
	std::vector<Region> r;
	r.push_back({ 0, p.grid * e.seq_words * 8, "state" });
	if (p.overlap)
		r.push_back({ p.seq2_at, p.seq2_at + p.grid2 * e.seq_words * 8, "tail state" });
	r.push_back({ p.cnt_at, p.cnt_at + 16 * p.nslices, "counters" });
	if (p.overlap)
		r.push_back({ p.cnt2_at, p.cnt2_at + 16 * p.nslices, "tail counters" });
	r.push_back({ p.sums_at, p.sums_at + 4 * n, "sums" });
	if (dict)
		r.push_back({ p.dict_at, p.dict_at + e.dict_bytes, "dictionary" });
	if (p.split) {
		r.push_back({ p.tok_at, p.tok_at + p.per_slice * (size_t)p.tok_stride * 4, "tokens" });
		r.push_back({ p.blk_at, p.blk_at + (LDA_PLAN_BLK_HDR_WORDS(p.per_slice) +
						    p.per_slice * p.blk_stride * LDA_PLAN_BLK_WORDS) * 4, "blocks" });
		if (p.overlap)
			r.push_back({ p.blk2_at, p.blk2_at + (LDA_PLAN_BLK_HDR_WORDS(p.tail_max) +
							      p.tail_max * p.blk_stride * LDA_PLAN_BLK_WORDS) * 4,
				      "tail blocks" });
	}
	for (size_t i = 0; i < r.size(); i++) {
		CHECK(r[i].lo <= r[i].hi && r[i].hi <= p.total);
		CHECK(i == 0 || r[i - 1].hi <= r[i].lo);
		CHECK(r[i].lo % 4 == 0);
	}
	CHECK(p.tok_at % 64 == 0 && (!p.split || (p.blk_at % 64 == 0 && p.blk2_at % 4 == 0)));
	/* what an overlapped call reserves covers the serial call that a failed
	 * side stream falls back to */
	CHECK(p.total >= m.total);
}

int main()
{
	const size_t cus_v[] = { 1, 8, 256, 304 };
	const size_t R_v[] = { 0, 1, 2, 4 };
	const size_t max_in_v[] = { 4096, 4097, 65536, (size_t)1 << 20, SIZE_MAX };
	const int level_v[] = { 0, 1, 6, 9, 10 };

	for (size_t cus : cus_v)
	for (size_t R : R_v)
	for (size_t max_in : max_in_v)
	for (int level : level_v)
	for (int sd = 0; sd < 3; sd++)
	for (int no_small = 0; no_small < 2; no_small++) {
		compress_plan_env e;
		e.num_cus = cus;
		e.small_max = 4096;
		e.small_wgs = 3;
		e.no_small = no_small != 0;
		e.tile = 4096;
		e.seq_words = 5321;
		e.dict_bytes = 64 + 20480;
		e.tail_rounds = R;
		const bool seg = sd == 1, dict = sd == 2;
		/* the scratch slice of this bound, from the model */
		const size_t slice = model(e, (size_t)1 << 40, max_in, level, seg, dict).per_slice;
		std::vector<size_t> ns = { 0, 1, 2 };
		const size_t marks[] = { 4 * cus, (4 + R) * cus, (4 + R) * cus + R * cus, 16 * cus, slice,
					 2 * slice, slice + 4 * cus, slice + (4 + R) * cus, 3 * slice + 1 };
		for (size_t m : marks) {
			if (m > ((size_t)1 << 30))
				continue;	/* (a non-split plan's one slice: any n) */
			for (size_t d = 0; d <= 6; d++)
				if (m + d >= 3)
					ns.push_back(m + d - 3);
		}
		for (size_t n : ns)
			check_one(e, n, max_in, level, seg, dict);
	}
	if (failures) {
		printf("%d of %ld checks FAILED\n", failures, checked);
		return 1;
	}
	printf("compress plan ok (%ld checks)\n", checked);
	return 0;
}
