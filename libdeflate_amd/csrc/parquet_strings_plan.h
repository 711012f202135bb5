/*
 * parquet_strings_plan.h - the host arithmetic that
 * libdeflate_amd_parquet_decode_batch_ex adds to parquet_plan.h for BYTE_ARRAY
 * pages (host_parquet.hip, parquet_strings_kernels.hip): its refusals, the
 * sections that carry length-prefixed values, their start lists, the slot
 * prefix over the string data pages and the tile-sum area.  Free of HIP:
 * tools/test_parquet_strings_plan.cpp runs it on the CPU.
 *
 * The call takes the rows of the old call plus bit PQ_BYTE_ARRAY of word 3.
 * pqs_check() clears that bit in a copy of the rows - a BYTE_ARRAY row has the
 * width field 0, so the copy reads as a column of width 1 - and puts the copy
 * through pq_row_why(), then pq_plan_build() plans it: one inflate batch, one
 * level and index walk (lda_pq_runs_kernel) and one verdict merge for all rows.
 * A width of 1 asks nothing of a string page that its values do not ask
 * anyway: every value takes 4 bytes at least.  pqs_plan_build() then takes the
 * string data pages out of the expand kernel's slot prefix, so that
 * lda_pq_expand_kernel writes the fixed-width pages alone, exactly as in the
 * old call, and appends three groups of columns:
 *
 *   PQS_WCOLS x n_w  the *walk sections*: every BYTE_ARRAY dictionary page and
 *                    every PLAIN BYTE_ARRAY data page.  lda_pqs_walk_kernel
 *                    lists where each of the values owed starts, and where the
 *                    last one ends, as uint32_t in the walk area - [two words
 *                    per section: failed, the values owed][the start lists] -:
 *                    PQS_W_STARTS is where the section's list begins there and
 *                    PQS_W_CAP what it holds, min(count, section bytes / 4) + 1
 *                    words
 *   PQS_SCOLS x n_s  the string data pages: PQS_S_SLOT_END is the prefix of
 *                    their slots, over which the sum and offsets kernels are
 *                    tiled PQ_TILE slots a workgroup
 *   PQS_VCOLS x n    per row, for the verdicts
 */
#ifndef LDA_PARQUET_STRINGS_PLAN_H
#define LDA_PARQUET_STRINGS_PLAN_H

#include "parquet_plan.h"

namespace lda {

enum {
	PQS_SCAN_BLOCK = 2048,	/* LDA_SCAN_BLOCK: sizes per workgroup of the project's scan */
	/* the walk sections' columns, n_w words each */
	PQS_W_SEC = 0,		/* as PQ_U_SEC */
	PQS_W_SEC_N,
	PQS_W_Z,		/* 1 + its place in the decode batch, or 0 */
	PQS_W_U,		/* a data page: 1 + its place among the data pages; a dictionary: 0 */
	PQS_W_COUNT,		/* a dictionary: its entries; a data page: its slots */
	PQS_W_STARTS, PQS_W_CAP,	/* its start list in the walk area, in words, and the list's words */
	PQS_WCOLS,
	/* the string data pages' columns, n_s words each */
	PQS_S_SLOT_END = 0,	/* the slots of this string page and all before it */
	PQS_S_U,		/* its place among the data pages */
	PQS_S_WALK,		/* the walk section its lengths come from: its own, or its dictionary's */
	PQS_S_STARTS,		/* and that section's PQS_W_STARTS */
	PQS_SCOLS,
	/* the verdict columns, n words each */
	PQS_V_S = 0,		/* a string data page: 1 + its place among them, else 0 */
	PQS_V_WALK,		/* 1 + the row's own walk section, or 0 */
	PQS_V_DWALK,		/* a dictionary-coded string page: 1 + its dictionary's walk section */
	PQS_VCOLS
};
#define PQ_BYTE_ARRAY ((uint64_t)1 << 14)	/* LIBDEFLATE_AMD_PARQUET_BYTE_ARRAY */

/* what the call refuses in row r beyond pq_row_why(), or NULL; masked holds
 * the rows 0 .. r with PQ_BYTE_ARRAY cleared */
static inline const char *
pqs_row_why(const uint64_t *rows, const uint64_t *masked, uint64_t r, uint64_t in_nbytes,
	    uint64_t out_avail, uint64_t valid_avail, bool have_valid, bool have_total)
{
	const uint64_t *row = rows + PQ_WORDS * r;
	const bool str = row[PQ_W_FIELDS] & PQ_BYTE_ARRAY;
	const pq_page s = pq_page_of(masked + PQ_WORDS * r);

	if (str && s.width != 1)
		return "BYTE_ARRAY with a non-zero width field";
	if (str && s.data && row[PQ_W_OUT] % 8)
		return "BYTE_ARRAY offsets (word 5) that are not a multiple of 8";
	if (str && !have_total)
		return "BYTE_ARRAY and d_bytes_total is NULL";
	if (s.dict_coded && row[PQ_W_DICT] < r) {
		const uint64_t *t = rows + PQ_WORDS * row[PQ_W_DICT];
		if ((t[PQ_W_FIELDS] & 15) == PQ_DICT && str != (bool)(t[PQ_W_FIELDS] & PQ_BYTE_ARRAY))
			return "its dictionary is of another type (BYTE_ARRAY on one side only)";
	}
	const char *why = pq_row_why(masked, r, in_nbytes, out_avail, valid_avail, have_valid);
	if (why)
		return why;
	/* (count + 1) * 8 < 2^35 */
	if (str && s.data && out_avail - row[PQ_W_OUT] < (s.count + 1) * 8)
		return "its offsets do not lie inside out_avail";
	return NULL;
}

/* true, with the rows less PQ_BYTE_ARRAY in masked, or false with the reason in
 * err: pointers apart, what the call refuses before any device work */
static inline bool
pqs_check(int format, uint64_t n, const uint64_t *rows, uint64_t in_nbytes, uint64_t out_avail,
	  uint64_t valid_avail, bool have_valid, bool have_bytes, uint64_t bytes_avail, bool have_total,
	  uint64_t flags, std::vector<uint64_t> &masked, std::string &err)
{
	if (format < 0 || format > 2) {
		err = "format " + std::to_string(format) + " is not DEFLATE, ZLIB or GZIP";
		return false;
	}
	if (flags) {
		err = "flags " + std::to_string(flags) + " is not 0";
		return false;
	}
	if (!have_bytes && bytes_avail) {
		err = "d_bytes is NULL and bytes_avail is not 0";
		return false;
	}
	masked.clear();
	if (n <= PQ_MAX_PAGES)
		masked.reserve((size_t)(PQ_WORDS * n));
	return chunk_check("n_pages", n, PQ_MAX_PAGES, [&](uint64_t r) {
		masked.insert(masked.end(), rows + PQ_WORDS * r, rows + PQ_WORDS * (r + 1));
		masked[(size_t)(PQ_WORDS * r + PQ_W_FIELDS)] &= ~PQ_BYTE_ARRAY;
		return pqs_row_why(rows, masked.data(), r, in_nbytes, out_avail, valid_avail, have_valid,
				   have_total);
	}, err);
}

/* the most words of the start list of a section of `bytes` that owes at most
 * `count` values: a value takes 4 bytes at least, and the end is listed too */
static inline uint64_t pqs_start_cap(uint64_t count, uint64_t bytes)
{
	return (count < bytes / 4 ? count : bytes / 4) + 1;
}

struct pqs_plan {
	pq_plan base;		/* of the masked rows; its slots and tiles: the fixed-width pages' */
	uint64_t n_w;		/* walk sections */
	uint64_t n_s;		/* string data pages */
	uint64_t slots, tiles;	/* of the string data pages */
	uint64_t start_words;	/* the start lists */
	uint64_t walk_words;	/* the walk area: 2 * n_w words and the start lists */
	uint64_t sum_words;	/* the tile-sum area: the tile sums, their places, the scan's block sums */
	/* in base.cols: [PQS_WCOLS x n_w] at w_at, [PQS_SCOLS x n_s] at s_at, [PQS_VCOLS x n]
	 * at v_at */
	uint64_t w_at, s_at, v_at;
};

/* the rows have passed pqs_check(), which made masked */
static inline void
pqs_plan_build(uint64_t n, const uint64_t *rows, const uint64_t *masked, pqs_plan &p)
{
	std::vector<uint64_t> w[PQS_WCOLS], s[PQS_SCOLS], v[PQS_VCOLS];
	std::vector<uint64_t> walk_of((size_t)n);
	chunk_rooms rooms;	/* as pq_plan_build() lays them */
	pq_plan &b = p.base;

	pq_plan_build(n, masked, b);
	uint64_t *slot_end = b.cols.data() + b.u_at + PQ_U_SLOT_END * b.n_u;
	const uint64_t *vz = b.cols.data() + b.v_at + PQ_V_Z * n;
	uint64_t u = 0, fixed = 0;
	p.slots = p.start_words = 0;
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *row = rows + PQ_WORDS * r;
		const pq_page t = pq_page_of(masked + PQ_WORDS * r);
		const bool str = row[PQ_W_FIELDS] & PQ_BYTE_ARRAY;
		const uint64_t sec_n = t.usize - t.def_len;
		const uint64_t sec = t.compressed ? rooms.take(sec_n) : PQ_IN_PLACE | (t.off + t.def_len);
		uint64_t own = 0;

		if (str && (!t.data || !t.dict_coded)) {
			const uint64_t cap = pqs_start_cap(t.count, sec_n);
			walk_of[(size_t)r] = w[0].size();
			own = w[0].size() + 1;
			w[PQS_W_SEC].push_back(sec);
			w[PQS_W_SEC_N].push_back(sec_n);
			w[PQS_W_Z].push_back(vz[r]);
			w[PQS_W_U].push_back(t.data ? u + 1 : 0);
			w[PQS_W_COUNT].push_back(t.count);
			w[PQS_W_STARTS].push_back(p.start_words);
			w[PQS_W_CAP].push_back(cap);
			p.start_words += cap;
		}
		v[PQS_V_WALK].push_back(own);
		if (!t.data) {
			v[PQS_V_S].push_back(0);
			v[PQS_V_DWALK].push_back(0);
			continue;
		}
		if (str) {
			p.slots += t.count;
			s[PQS_S_SLOT_END].push_back(p.slots);
			s[PQS_S_U].push_back(u);
			s[PQS_S_WALK].push_back(walk_of[(size_t)(t.dict_coded ? row[PQ_W_DICT] : r)]);
			s[PQS_S_STARTS].push_back(w[PQS_W_STARTS][(size_t)s[PQS_S_WALK].back()]);
		} else {
			fixed += t.count;
		}
		v[PQS_V_S].push_back(str ? s[0].size() : 0);
		v[PQS_V_DWALK].push_back(str && t.dict_coded ? walk_of[(size_t)row[PQ_W_DICT]] + 1 : 0);
		slot_end[u++] = fixed;
	}
	b.slots = fixed;
	b.tiles = (fixed + PQ_TILE - 1) / PQ_TILE;
	p.n_w = w[0].size();
	p.n_s = s[0].size();
	p.walk_words = 2 * p.n_w + p.start_words;
	for (uint64_t &at : w[PQS_W_STARTS])	/* the lists stand behind the sections' words */
		at += 2 * p.n_w;
	for (uint64_t &at : s[PQS_S_STARTS])
		at += 2 * p.n_w;
	p.tiles = (p.slots + PQ_TILE - 1) / PQ_TILE;
	p.sum_words = 2 * p.tiles + (p.tiles + PQS_SCAN_BLOCK - 1) / PQS_SCAN_BLOCK + 1;
	p.w_at = chunk_append(b.cols, w, PQS_WCOLS);
	p.s_at = chunk_append(b.cols, s, PQS_SCOLS);
	p.v_at = chunk_append(b.cols, v, PQS_VCOLS);
}

} /* namespace lda */

#endif /* LDA_PARQUET_STRINGS_PLAN_H */
