/*
 * tar_plan.h - the host arithmetic of libdeflate_amd_tar_read_batch and
 * libdeflate_amd_tar_ranges (host_tar.hip): the index rows of a selection
 * checked, and from them every selected entry's place in the output, the
 * columns of the gather copy, or the (offset, length) pairs a ranged read of
 * the archive takes.  Free of HIP: tools/test_tar_plan.cpp runs it on the CPU.
 *
 * A row is what libdeflate_amd_tar_index_batch wrote (include/libdeflate_amd.h):
 * { header, name_off, name_len | prefix_len << 32, typeflag | name source << 8,
 * data_off, usize, mtime, out_off }.  out_off is not read: a selection has
 * offsets of its own.
 */
#ifndef LDA_TAR_PLAN_H
#define LDA_TAR_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace lda {

enum {
	TAR_ROW_WORDS = 8,
	TAR_BLOCK = 512,
	TAR_UNSUPPORTED = 18,	/* LIBDEFLATE_AMD_TAR_UNSUPPORTED */
	TAR_COPY_TILE = 65536,	/* LDA_TAR_COPY_TILE */
	/* the columns of a plan, n_sel words each, in the order they go up; one
	 * word with the number of tiles follows them */
	TAR_COL_SRC = 0,
	TAR_COL_DST,
	TAR_COL_LEN,
	TAR_COL_TILE,
	TAR_COLS
};
static const uint64_t TAR_MAX_FILE = (uint64_t)1 << 36;

/* the entry's result as the row alone tells it: sparse, multi-volume and
 * dumpdir entries are UNSUPPORTED */
static inline int tar_row_result(const uint64_t *row)
{
	const uint64_t t = row[3] & 0xFF;
	return t == 'S' || t == 'M' || t == 'D' ? TAR_UNSUPPORTED : 0;
}

/* NULL, or why the row cannot be one of a file of in_nbytes bytes */
static inline const char *tar_row_check(const uint64_t *row, uint64_t in_nbytes)
{
	const uint64_t name_len = row[2] & 0xFFFFFFFFull, prefix_len = row[2] >> 32;

	if (row[0] % TAR_BLOCK || row[0] > in_nbytes || in_nbytes - row[0] < TAR_BLOCK)
		return "its header is no block inside in_nbytes";
	if (row[1] > in_nbytes || in_nbytes - row[1] < name_len || prefix_len > 155)
		return "its name does not lie inside in_nbytes";
	if (row[3] > 0xFFFF)
		return "its typeflag and name source are no 16-bit word";
	if (row[5] >= TAR_MAX_FILE)
		return "a size of 2^36 or more";
	if (row[4] != row[0] + TAR_BLOCK || in_nbytes - row[4] < row[5])
		return "its data does not lie inside in_nbytes";
	return NULL;
}

static inline bool
tar_sel_row(const uint64_t *index, uint64_t entries, const uint64_t *sel, uint64_t r,
	    uint64_t in_nbytes, const uint64_t **row_ret, std::string &err)
{
	char msg[160];

	if (sel[r] >= entries) {
		snprintf(msg, sizeof(msg), "sel[%llu] = %llu of %llu entries", (unsigned long long)r,
			 (unsigned long long)sel[r], (unsigned long long)entries);
		err = msg;
		return false;
	}
	const uint64_t *row = index + TAR_ROW_WORDS * sel[r];
	const char *why = tar_row_check(row, in_nbytes);
	if (why) {
		snprintf(msg, sizeof(msg), "row %llu: %s", (unsigned long long)sel[r], why);
		err = msg;
		return false;
	}
	*row_ret = row;
	return true;
}

/*
 * cols: TAR_COLS columns of n_sel words and the tile count; results: n_sel
 * per-selection results; out_offsets: NULL or n_sel + 1 words, where selection
 * r starts and where the last one ends.  false with a reason in err: a sel at
 * or above entries, a row that fails tar_row_check(), a selection that needs
 * more than out_avail.  align_mask: out_align - 1.
 */
static inline bool
tar_plan_read(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
	      uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask,
	      std::vector<uint64_t> &cols, std::vector<int32_t> &results, uint64_t *out_offsets,
	      uint64_t *total_ret, std::string &err)
{
	uint64_t at = 0, tiles = 0;

	cols.assign((size_t)(TAR_COLS * n_sel + 1), 0);
	results.assign((size_t)n_sel, 0);
	for (uint64_t r = 0; r < n_sel; r++) {
		const uint64_t *row;
		if (!tar_sel_row(index, entries, sel, r, in_nbytes, &row, err))
			return false;
		const int pre = tar_row_result(row);
		results[(size_t)r] = pre;
		if (out_offsets)
			out_offsets[r] = at;
		cols[TAR_COL_TILE * n_sel + r] = tiles;
		if (pre == 0) {
			const uint64_t room = (row[5] + align_mask) & ~align_mask;
			if (at > out_avail || room > out_avail - at) {
				err = "the selection needs more than out_avail";
				return false;
			}
			cols[TAR_COL_SRC * n_sel + r] = row[4];
			cols[TAR_COL_DST * n_sel + r] = at;
			cols[TAR_COL_LEN * n_sel + r] = row[5];
			tiles += (row[5] + TAR_COPY_TILE - 1) / TAR_COPY_TILE;
			at += room;
		}
	}
	cols[TAR_COLS * n_sel] = tiles;
	if (out_offsets)
		out_offsets[n_sel] = at;
	if (total_ret)
		*total_ret = at;
	return true;
}

/*
 * ranges: 2 n_sel words, (data_off, usize) of every selection - what
 * libdeflate_amd_seek_read_batch takes for the uncompressed archive; an
 * UNSUPPORTED row gives (data_off, 0).  The rows are checked as above against
 * the largest file there is.
 */
static inline bool
tar_plan_ranges(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		uint64_t *ranges, uint64_t *total_ret, std::string &err)
{
	uint64_t total = 0;

	for (uint64_t r = 0; r < n_sel; r++) {
		const uint64_t *row;
		if (!tar_sel_row(index, entries, sel, r, TAR_MAX_FILE, &row, err))
			return false;
		ranges[2 * r] = row[4];
		ranges[2 * r + 1] = tar_row_result(row) == 0 ? row[5] : 0;
		total += ranges[2 * r + 1];
	}
	if (total_ret)
		*total_ret = total;
	return true;
}

} /* namespace lda */

#endif /* LDA_TAR_PLAN_H */
