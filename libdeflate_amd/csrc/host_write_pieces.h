/*
 * host_write_pieces.h - what the enqueue functions of the ZIP, gzip-members,
 * PNG, shuffle, TIFF and OpenEXR writers share (host_write_pieces.hip): the
 * plan's parameters, the common regions of c->zipw, the reserve step, the
 * upload, the compress stage and the copy kernel's launch.  A writer calls
 * them in that order, its own regions and kernels between them; the last
 * three, the chunk codecs, through the steps at the end of this file.
 */
#ifndef LDA_HOST_WRITE_PIECES_H
#define LDA_HOST_WRITE_PIECES_H

#include "host_read_plan.h"	/* the grids: wave_grid(), tile_grid(); chunk_plan.h */
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

/*
 * ---- the chunk codecs' writers (chunk_plan.h: host_shuffle_write.hip,
 * host_tiff_write.hip, host_exr_write.hip) ----
 * A plan gives every row a room; the format's kernels fill the rooms; then, in
 * this order: chunkw_begin(), [the format's kernels], chunkw_compress(),
 * chunkw_sizes(), chunkw_scan(), [the format's place kernel, or
 * chunkw_place()], chunkw_finish().
 */

/* c->zipw: [ecols][the pieces' regions, pieces_carve()][csize][dsize][sum][sums]
 * [raw][rooms]; dsize and raw only where the writer has two areas */
struct ChunkwScratch : PiecesScratch {
	uint64_t *ecols, *csize, *dsize;
	uint32_t *sum, *sums;
	uint8_t *raw, *rooms;	/* p.rooms_bytes each, and 64 to spare */
	size_t bytes;
};

/* the size pass, pieces_reserve(), the carves of c->zipw and of the pinned
 * block, the copy of ecols and pieces_upload().  two_areas: OpenEXR's second
 * size per row and second area of rooms, for the chunks stored raw */
int chunkw_begin(struct libdeflate_compressor *c, const chunk_write_plan &p,
		 const std::vector<zipw_launch> &launches, hipStream_t st, ChunkwScratch &s,
		 bool two_areas = false);

/* ONE checksum batch over the pieces in src - Adler-32 for zlib, CRC-32 for
 * gzip, none for raw deflate - into sums, then pieces_compress() from src */
int chunkw_compress(struct libdeflate_compressor *c, int format, const chunk_write_plan &p,
		    const ChunkwScratch &s, const std::vector<zipw_launch> &launches, const uint8_t *src,
		    hipStream_t st);

/* lda_shufw_chunk_kernel sizes the streams; then, behind what a format does to
 * the sizes (OpenEXR's choose kernel), chunkw_scan() -> where the total is */
void chunkw_sizes(const DeviceCtx *ctx, int format, const chunk_write_plan &p, const ChunkwScratch &s,
		  hipStream_t st);
const uint64_t *chunkw_scan(const chunk_write_plan &p, const ChunkwScratch &s, hipStream_t st);

/* lda_shufw_place_kernel: headers, footers, the copy list and, where d_index is
 * not NULL, the shuffle reader's rows */
void chunkw_place(const DeviceCtx *ctx, int format, int level, const chunk_write_plan &p,
		  const ChunkwScratch &s, uint64_t out_avail, uint8_t *d_out, uint64_t *d_index,
		  hipStream_t st);

/* pieces_copy() - copy_src: where the pieces that are not copied from the
 * slots are read - and lda_shufw_final_kernel into d_result */
int chunkw_finish(const DeviceCtx *ctx, const chunk_write_plan &p, const ChunkwScratch &s,
		  const uint64_t *total_at, uint64_t out_avail, const uint8_t *copy_src, uint8_t *d_out,
		  uint64_t *d_result, hipStream_t st);

/* a *_bound entry: bound() behind the pointer it refuses */
template <typename Bound>
static inline size_t chunkw_bound_call(const char *what, size_t n, const uint64_t *rows, Bound bound)
{
	if (n && !rows) {
		set_error("%s: NULL argument", what);
		return 0;
	}
	return (size_t)bound();
}

/* the envelope of a writer's call with a plan of type P, the mirror of
 * read_call(): check(err) -> bool is the plan's check, its refusal the call's
 * BAD_ARG under the call's name; of no rows, where empty_returns, nothing is
 * done; build(pr, p) fills the plan and run(p) queues it on the object's device */
template <typename P, typename Check, typename Build, typename Run>
static inline int
chunkw_call(const char *what, struct libdeflate_compressor *c, size_t n, const uint64_t *rows,
	    const void *d_in, size_t in_avail, const void *d_out, const uint64_t *d_result,
	    bool empty_returns, Check check, Build build, Run run)
{
	if (!c || !d_out || !d_result || (!d_in && in_avail) || (n && !rows)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!check(err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (empty_returns && n == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (store false at level 0 too: its stored blocks are the compress kernel's) */
		const zipw_params pr = pieces_params(c, false);
		P p;
		build(pr, p);
		return run(p);
	});
}

} /* namespace lda */

#endif /* LDA_HOST_WRITE_PIECES_H */
