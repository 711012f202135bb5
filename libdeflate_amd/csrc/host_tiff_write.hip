/*
 * host_tiff_write.hip - C-ABI of writing predictor-coded deflate strips and
 * tiles (TIFF, GeoTIFF) in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_tiff_encode_batch).
 *
 * tiff_plan.h checks the rows, gives every segment a room for its predicted
 * bytes in the object's scratch and cuts the rooms into pieces; its columns go
 * up; lda_tiff_predict_kernel (tiff_kernels.hip) fills the rooms from the raw
 * pixels in d_in - the kept rectangle, zero samples up to the coded size -;
 * ONE Adler-32 batch runs over the pieces in the rooms, the pieces are
 * compressed into slots (the shared piece pipeline, host_write_pieces.hip),
 * and the shuffle writer's kernels (shuffle_kernels.hip, format zlib) size the
 * streams and place headers and footers; lda_tiffw_index_kernel writes the
 * reader's rows.
 * c->zipw: [segment columns][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize][sum]
 * [sums][rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "tiff_plan.h"

using namespace lda;

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_tiff_encode_bound(struct libdeflate_compressor *c, size_t n_segments,
				 const uint64_t *rows)
{
	(void)c;	/* (no level has another bound: libdeflate_zlib_compress_bound()) */
	return chunkw_bound_call("tiff_encode_bound", n_segments, rows,
				 [&] { return tiff_bound(n_segments, rows); });
}

/* (p.n is not 0: the call has returned for no segments) */
static int tiffw_enqueue(struct libdeflate_compressor *c, const tiff_write_plan &p, const uint8_t *d_in,
			 uint8_t *d_out, uint64_t out_avail, uint64_t *d_result, uint64_t *d_index,
			 hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n;
	const std::vector<zipw_launch> launches = zipw_launches(p);
	ChunkwScratch s;

	LDA_OK_TRY(chunkw_begin(c, p, launches, st, s));
	if (p.tiles)
		hipLaunchKernelGGL(lda_tiff_predict_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n, p.tiles, (const uint64_t *)s.ecols, d_in, s.rooms);
	LDA_OK_TRY(chunkw_compress(c, LIBDEFLATE_AMD_ZLIB, p, s, launches, s.rooms, st));
	chunkw_sizes(ctx, LIBDEFLATE_AMD_ZLIB, p, s, st);
	const uint64_t *total_at = chunkw_scan(p, s, st);
	/* d_index NULL: the place kernel's index rows are the shuffle calls'; ours
	 * come from lda_tiffw_index_kernel */
	chunkw_place(ctx, LIBDEFLATE_AMD_ZLIB, c->level, p, s, out_avail, d_out, NULL, st);
	if (d_index)
		hipLaunchKernelGGL(lda_tiffw_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
				   st, (uint64_t)n, out_avail, (const uint64_t *)s.ecols,
				   (const uint64_t *)s.csize, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_index);
	/* (copy_src is d_in, as the shuffle writer's) */
	return chunkw_finish(ctx, p, s, total_at, out_avail, d_in, d_out, d_result, st);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tiff_encode_batch(struct libdeflate_compressor *c, size_t n_segments,
				 const uint64_t *rows, const void *d_in, size_t in_avail, void *d_out,
				 size_t out_avail, uint64_t *d_result, uint64_t *d_index, void *stream)
{
	/* empty_returns true: of no segments nothing is queued, and d_result is not
	 * written either */
	return chunkw_call<tiff_write_plan>("tiff_encode_batch", c, n_segments, rows, d_in, in_avail, d_out,
					    d_result, true, [&](std::string &err) {
		return tiff_check(n_segments, rows, false, 0, in_avail, c->level, err);
	}, [&](const zipw_params &pr, tiff_write_plan &p) {
		tiff_write_plan_build(pr, n_segments, rows, p);
	}, [&](const tiff_write_plan &p) {
		return tiffw_enqueue(c, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result,
				     d_index, (hipStream_t)stream);
	});
}
