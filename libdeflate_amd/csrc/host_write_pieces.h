/*
 * host_write_pieces.h - what the enqueue functions of the ZIP, gzip-members and
 * PNG writers share (host_write_pieces.hip): the plan's parameters, the common
 * regions of c->zipw, the reserve step, the upload, the compress stage and the
 * copy kernel's launch.  A writer calls them in that order, its own regions and
 * kernels between them.
 */
#ifndef LDA_HOST_WRITE_PIECES_H
#define LDA_HOST_WRITE_PIECES_H

#include "host_read_plan.h"	/* the grids: wave_grid(), tile_grid() */
#include "write_pieces_plan.h"

namespace lda {

/* what zipw_cut_pieces() takes of the object and the environment */
zipw_params pieces_params(const struct libdeflate_compressor *c, bool store);

/* the regions of c->zipw every writer has; a writer's struct derives from it */
struct PiecesScratch {
	/* what goes up, behind the writer's columns */
	uint64_t *pcols;
	uint32_t *seg;
	uint8_t *behind;	/* the writer's names or work list */
	size_t up_bytes;
	/* what the kernels leave */
	uint64_t *out_n, *cp_src, *cp_dst, *cp_len, *sizes, *offs, *bsum;
	uint8_t *slots;
	const uint64_t *pcol[ZIPW_PCOLS];	/* the columns of pcols */
};

/* [pcols][seg][behind] - where what goes up ends - [out_n][cp_src cp_dst
 * cp_len][sizes][offs][bsum][slots] out of c, which holds the writer's columns
 * and gets its results behind the slots.  n: entries */
void pieces_carve(Carve &c, const zipw_pieces &p, size_t n, size_t behind_bytes, PiecesScratch &s);

/* begins the upload and reserves c->zipw (bytes), the pinned block (up_bytes)
 * and the kernels' scratch of the largest launch: OK, OOM or NO_DEVICE */
int pieces_reserve(struct libdeflate_compressor *c, const std::vector<zipw_launch> &launches,
		   size_t bytes, size_t up_bytes, uint8_t **ws, uint8_t **pinned);

/* the piece columns and seg_info into the pinned block's regions hs - the writer
 * has copied its own -, and the block up to ws; up_bytes 0: nothing is sent */
int pieces_upload(struct libdeflate_compressor *c, const PiecesScratch &hs, const zipw_pieces &p,
		  uint8_t *ws, hipStream_t st);

/* every launch of the list: the pieces, read at src + their offsets, into their slots */
int pieces_compress(struct libdeflate_compressor *c, const PiecesScratch &s,
		    const std::vector<zipw_launch> &launches, const uint8_t *src, hipStream_t st);

/* lda_zipw_copy_kernel over the np pieces the writer's place kernel has listed;
 * tail: bytes the writer puts behind the pieces' total (the ZIP directory) */
void pieces_copy(const DeviceCtx *ctx, const PiecesScratch &s, size_t np, const uint64_t *total_at,
		 uint64_t out_avail, uint64_t tail, const uint8_t *d_in, uint8_t *d_out,
		 hipStream_t st);

} /* namespace lda */

#endif /* LDA_HOST_WRITE_PIECES_H */
