/*
 * zip_plan.h - the host arithmetic of libdeflate_amd_zip_read_batch
 * (host_zip.hip): the index rows of a selection checked against the file, and
 * from them every selected entry's place in the output and the descriptors of
 * the decode batch, the copy of the stored entries and the CRC batch.  Free of
 * HIP: tools/test_zip_plan.cpp runs it on the CPU.
 *
 * A row is what libdeflate_amd_zip_index_batch wrote (include/libdeflate_amd.h):
 * { central record, name_len, method | flags << 16, CRC-32, data_off, csize,
 * usize, out_off }.  out_off is not read: a selection has offsets of its own.
 */
#ifndef LDA_ZIP_PLAN_H
#define LDA_ZIP_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace lda {

enum {
	ZIP_ROW_WORDS = 8,
	ZIP_CEN_BYTES = 46,
	ZIP_BAD_DATA = 1,	/* LIBDEFLATE_BAD_DATA */
	ZIP_UNSUPPORTED = 18,	/* LIBDEFLATE_AMD_ZIP_UNSUPPORTED */
	ZIP_FLAGS_REFUSED = 0x2061,	/* flag bits 0, 5, 6, 13 */
	/* meta >> 40: what the kernels do for the entry */
	ZIP_KIND_NONE = 0,
	ZIP_KIND_STORED = 1,
	ZIP_KIND_DEFLATE = 2,
	/* the columns of a plan, n_sel words each, in the order they go up */
	ZIP_COL_IN_OFF = 0,
	ZIP_COL_IN_N,
	ZIP_COL_OUT_OFF,
	ZIP_COL_OUT_AV,
	ZIP_COL_CP_SRC,
	ZIP_COL_CP_LEN,
	ZIP_COL_CRC_N,
	ZIP_COL_META,
	ZIP_COLS
};

/* the entry's pre-decode result as the row alone tells it: 0, UNSUPPORTED
 * (method, flags), BAD_DATA (a stored entry whose sizes differ) */
static inline int zip_row_result(const uint64_t *row)
{
	const uint64_t method = row[2] & 0xFFFF, flags = row[2] >> 16;

	if ((flags & ZIP_FLAGS_REFUSED) || (method != 0 && method != 8))
		return ZIP_UNSUPPORTED;
	if (method == 0 && row[5] != row[6])
		return ZIP_BAD_DATA;
	return 0;
}

/* NULL, or why the row cannot be one of a file of in_nbytes bytes */
static inline const char *zip_row_check(const uint64_t *row, uint64_t in_nbytes)
{
	if (row[1] > 0xFFFF || row[0] > in_nbytes || in_nbytes - row[0] < ZIP_CEN_BYTES + row[1])
		return "its central record does not lie inside in_nbytes";
	if (row[2] > 0xFFFFFFFFull || row[3] > 0xFFFFFFFFull)
		return "its method, flags or CRC-32 are no 32-bit words";
	if (row[5] > 0xFFFFFFFFull || row[6] > 0xFFFFFFFFull)
		return "a size of 4 GiB or more";
	if (row[4] > in_nbytes || in_nbytes - row[4] < row[5])
		return "its data does not lie inside in_nbytes";
	return NULL;
}

/*
 * cols: ZIP_COLS columns of n_sel words; out_offsets: NULL or n_sel + 1 words,
 * where selection r starts and where the last one ends.  false with a reason
 * in err: a sel at or above entries, a row that fails zip_row_check(), a
 * selection that needs more than out_avail.  align_mask: out_align - 1.
 */
static inline bool
zip_plan_read(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
	      uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask,
	      std::vector<uint64_t> &cols, uint64_t *out_offsets, uint64_t *total_ret,
	      std::string &err)
{
	char msg[160];
	uint64_t at = 0;

	cols.assign((size_t)(ZIP_COLS * n_sel), 0);
	for (uint64_t r = 0; r < n_sel; r++) {
		if (sel[r] >= entries) {
			snprintf(msg, sizeof(msg), "sel[%llu] = %llu of %llu entries",
				 (unsigned long long)r, (unsigned long long)sel[r],
				 (unsigned long long)entries);
			err = msg;
			return false;
		}
		const uint64_t *row = index + ZIP_ROW_WORDS * sel[r];
		const char *why = zip_row_check(row, in_nbytes);
		if (why) {
			snprintf(msg, sizeof(msg), "row %llu: %s", (unsigned long long)sel[r], why);
			err = msg;
			return false;
		}
		const int pre = zip_row_result(row);
		uint64_t meta = row[3] | (uint64_t)pre << 32;
		if (out_offsets)
			out_offsets[r] = at;
		if (pre == 0) {
			const uint64_t room = (row[6] + align_mask) & ~align_mask;
			if (at > out_avail || room > out_avail - at) {
				err = "the selection needs more than out_avail";
				return false;
			}
			cols[ZIP_COL_OUT_OFF * n_sel + r] = at;
			cols[ZIP_COL_CRC_N * n_sel + r] = row[6];
			if ((row[2] & 0xFFFF) == 8) {
				meta |= (uint64_t)ZIP_KIND_DEFLATE << 40;
				cols[ZIP_COL_IN_OFF * n_sel + r] = row[4];
				cols[ZIP_COL_IN_N * n_sel + r] = row[5];
				cols[ZIP_COL_OUT_AV * n_sel + r] = row[6];
			} else {
				meta |= (uint64_t)ZIP_KIND_STORED << 40;
				cols[ZIP_COL_CP_SRC * n_sel + r] = row[4];
				cols[ZIP_COL_CP_LEN * n_sel + r] = row[6];
			}
			at += room;
		}
		cols[ZIP_COL_META * n_sel + r] = meta;
	}
	if (out_offsets)
		out_offsets[n_sel] = at;
	if (total_ret)
		*total_ret = at;
	return true;
}

} /* namespace lda */

#endif /* LDA_ZIP_PLAN_H */
