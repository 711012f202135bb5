/*
 * zip_large_plan.h - the host arithmetic of libdeflate_amd_zip_read_large
 * (host_zip_large.hip): zip_plan_read()'s plan of a selection (zip_plan.h),
 * and on top of it which entries leave the one-wave batch.  Free of HIP:
 * tools/test_zip_large_plan.cpp runs it on the CPU.
 *
 * Two rules, each from the index row alone:
 *
 *   MANY-WAVE  a method-8 entry with csize >= large_min is decoded by
 *              libdeflate_amd_decompress_large, one call per entry;
 *   PIECED     an entry of either method with usize > piece is copied (if
 *              stored) and checksummed in pieces of `piece` bytes, the last
 *              one ragged, and its CRC-32 is combined from the pieces'.
 *
 * An entry under either rule is OWNED by lda_zip_lfinal_kernel
 * (zip_large_kernels.hip), which writes its result; bit ZIPL_OWNED of its meta
 * word says so, and lda_zip_rfinal_kernel is launched over the runs of rows
 * in between (runs).  What the rule takes over is zeroed in the sibling's
 * columns, so that the batch kernels see an empty chunk there: the decode
 * descriptor (in_off, in_n, out_av) of a many-wave entry, the copy and CRC
 * descriptors (cp_src, cp_len, crc_n) of a pieced one.  A pieced entry whose
 * csize is below large_min keeps its decode descriptor - the batch decodes
 * it, and the final kernel reads the batch's verdict for it; a many-wave entry
 * of at most `piece` bytes keeps its CRC descriptor likewise.
 */
#ifndef LDA_ZIP_LARGE_PLAN_H
#define LDA_ZIP_LARGE_PLAN_H

#include "zip_plan.h"

namespace lda {

enum {
	ZIPL_OWNED = 48,	/* meta bit: lda_zip_lfinal_kernel writes the row's result */
	/* flags of an owned entry */
	ZIPL_MANY_WAVE = 1,
	ZIPL_PIECED = 2,
	/* the columns of the owned entries, n_own words each, in the order they go up */
	ZIPL_COL_SEL = 0,	/* the selection number r */
	ZIPL_COL_FLAGS,
	ZIPL_COL_IN_OFF,	/* data_off */
	ZIPL_COL_IN_N,		/* csize */
	ZIPL_COL_OUT_OFF,
	ZIPL_COL_USIZE,
	ZIPL_COL_FIRST,		/* its first piece, its piece count (0 unless pieced) */
	ZIPL_COL_COUNT,
	ZIPL_COL_RES,		/* the many-wave decode's result and actual_in: the host */
	ZIPL_COL_AIN,		/* fills them in after the decode (0 here) */
	ZIPL_COLS,
	/* the columns of the pieces, n_pieces words each */
	ZIPP_COL_SRC = 0,	/* into the file (a stored entry's pieces; else 0) */
	ZIPP_COL_DST,		/* into the output */
	ZIPP_COL_LEN,
	ZIPP_COL_CP,		/* bytes to copy: LEN for a stored entry's piece, else 0 */
	ZIPP_COLS
};

struct ZipLargePlan {
	std::vector<uint64_t> cols;	/* ZIP_COLS x n_sel: the sibling's, owned rows emptied */
	std::vector<uint64_t> own;	/* ZIPL_COLS x n_own, in sel order */
	std::vector<uint64_t> pieces;	/* ZIPP_COLS x n_pieces, in sel order */
	/* maximal runs { first row, rows } of rows that are not owned */
	std::vector<uint64_t> runs;
	uint64_t n_own = 0, n_pieces = 0, n_many = 0;
};

/*
 * zip_plan_read()'s arguments, refusals, out_offsets and total; large_min and
 * piece as above (piece != 0).  p is rebuilt from nothing.
 */
static inline bool
zip_plan_read_large(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		    uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask,
		    uint64_t large_min, uint64_t piece, ZipLargePlan &p, uint64_t *out_offsets,
		    uint64_t *total_ret, std::string &err)
{
	struct Own { uint64_t w[ZIPL_COLS]; };
	struct Piece { uint64_t w[ZIPP_COLS]; };
	std::vector<Own> own;
	std::vector<Piece> pcs;

	p = ZipLargePlan();
	if (piece == 0) {
		err = "piece 0";
		return false;
	}
	if (!zip_plan_read(index, entries, n_sel, sel, in_nbytes, out_avail, align_mask, p.cols,
			   out_offsets, total_ret, err))
		return false;
	uint64_t *c = p.cols.data();
	uint64_t run0 = 0;	/* where the run of rows that are not owned began */
	for (uint64_t r = 0; r < n_sel; r++) {
		const uint64_t kind = (c[ZIP_COL_META * n_sel + r] >> 40) & 3;
		if (kind == ZIP_KIND_NONE)
			continue;
		const uint64_t *row = index + ZIP_ROW_WORDS * sel[r];
		const uint64_t csize = row[5], usize = row[6];
		const bool many = kind == ZIP_KIND_DEFLATE && csize >= large_min;
		const bool pieced = usize > piece;
		if (!many && !pieced)
			continue;
		Own o = {};
		o.w[ZIPL_COL_SEL] = r;
		o.w[ZIPL_COL_FLAGS] = (many ? ZIPL_MANY_WAVE : 0) | (pieced ? ZIPL_PIECED : 0);
		o.w[ZIPL_COL_IN_OFF] = row[4];
		o.w[ZIPL_COL_IN_N] = csize;
		o.w[ZIPL_COL_OUT_OFF] = c[ZIP_COL_OUT_OFF * n_sel + r];
		o.w[ZIPL_COL_USIZE] = usize;
		if (many) {
			c[ZIP_COL_IN_OFF * n_sel + r] = 0;
			c[ZIP_COL_IN_N * n_sel + r] = 0;
			c[ZIP_COL_OUT_AV * n_sel + r] = 0;
			p.n_many++;
		}
		if (pieced) {
			const bool stored = kind == ZIP_KIND_STORED;
			o.w[ZIPL_COL_FIRST] = pcs.size();
			o.w[ZIPL_COL_COUNT] = (usize + piece - 1) / piece;
			for (uint64_t at = 0; at < usize; at += piece) {
				const uint64_t len = usize - at < piece ? usize - at : piece;
				pcs.push_back(Piece{ { stored ? row[4] + at : 0,
						       o.w[ZIPL_COL_OUT_OFF] + at, len, stored ? len : 0 } });
			}
			c[ZIP_COL_CP_SRC * n_sel + r] = 0;
			c[ZIP_COL_CP_LEN * n_sel + r] = 0;
			c[ZIP_COL_CRC_N * n_sel + r] = 0;
		}
		c[ZIP_COL_META * n_sel + r] |= (uint64_t)1 << ZIPL_OWNED;
		own.push_back(o);
		if (r > run0) {
			p.runs.push_back(run0);
			p.runs.push_back(r - run0);
		}
		run0 = r + 1;
	}
	if (n_sel > run0) {
		p.runs.push_back(run0);
		p.runs.push_back(n_sel - run0);
	}
	/* rows -> columns */
	p.n_own = own.size();
	p.n_pieces = pcs.size();
	p.own.resize((size_t)(ZIPL_COLS * p.n_own));
	for (uint64_t j = 0; j < p.n_own; j++)
		for (uint64_t a = 0; a < ZIPL_COLS; a++)
			p.own[(size_t)(a * p.n_own + j)] = own[(size_t)j].w[a];
	p.pieces.resize((size_t)(ZIPP_COLS * p.n_pieces));
	for (uint64_t i = 0; i < p.n_pieces; i++)
		for (uint64_t a = 0; a < ZIPP_COLS; a++)
			p.pieces[(size_t)(a * p.n_pieces + i)] = pcs[(size_t)i].w[a];
	return true;
}

} /* namespace lda */

#endif /* LDA_ZIP_LARGE_PLAN_H */
