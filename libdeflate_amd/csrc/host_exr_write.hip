/*
 * host_exr_write.hip - C-ABI of writing OpenEXR ZIP and ZIPS chunks, scanline
 * blocks and tiles, in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_exr_encode_batch).
 *
 * exr_plan.h checks the rows, gives every chunk a room in each of two areas of
 * the object's scratch - raw and coded, at the same offset - and cuts the
 * coded rooms into pieces; its columns go up; lda_exr_gather_kernel
 * (exr_kernels.hip) collects every chunk's lines or pixels from d_in into its
 * raw room and lda_exr_code_kernel codes the raw room into the coded room; ONE
 * Adler-32 batch runs over the pieces in the coded rooms, the pieces are
 * compressed into slots (the shared piece pipeline, host_write_pieces.hip) and
 * the shuffle writer's lda_shufw_chunk_kernel (format zlib) sizes the streams;
 * lda_exrw_choose_kernel keeps a stream where it is shorter than its raw
 * chunk, the sizes are scanned, and lda_exrw_place_kernel writes heads, zlib
 * headers and footers and the reader's rows and lists the copies: of a kept
 * stream from the slots, of a raw chunk the same ranges of the raw area, which
 * is what lda_zipw_copy_kernel reads as its source.
 * c->zipw: [chunk and layout columns][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize]
 * [dsize][sum][sums][raw rooms][coded rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "exr_plan.h"

using namespace lda;

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_exr_encode_bound(struct libdeflate_compressor *c, size_t n_chunks, const uint64_t *rows)
{
	(void)c;	/* (no level has another bound: a chunk is never written longer than raw) */
	return chunkw_bound_call("exr_encode_bound", n_chunks, rows, [&] { return exr_bound(n_chunks, rows); });
}

/* (p.n is not 0: the call has returned for no chunks) */
static int exrw_enqueue(struct libdeflate_compressor *c, const exr_write_plan &p, const uint8_t *d_in,
			uint8_t *d_out, uint64_t out_avail, uint64_t *d_result, uint64_t *d_index,
			hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n;
	const std::vector<zipw_launch> launches = zipw_launches(p);
	ChunkwScratch s;	/* two areas: s.raw, and s.rooms the coded rooms */

	LDA_OK_TRY(chunkw_begin(c, p, launches, st, s, true));
	const uint64_t *const *pcol = s.pcol;

	hipLaunchKernelGGL(lda_exr_gather_kernel, dim3(tile_grid(ctx, p.ltiles)), dim3(256), 0, st,
			   (uint64_t)n, p.ltiles, (const uint64_t *)(s.ecols + p.l_at), d_in, s.raw);
	hipLaunchKernelGGL(lda_exr_code_kernel, dim3(tile_grid(ctx, p.ctiles)), dim3(256), 0, st,
			   (uint64_t)n, p.ctiles, (const uint64_t *)s.ecols, (const uint8_t *)s.raw, s.rooms);
	LDA_OK_TRY(chunkw_compress(c, LIBDEFLATE_AMD_ZLIB, p, s, launches, s.rooms, st));
	chunkw_sizes(ctx, LIBDEFLATE_AMD_ZLIB, p, s, st);
	/* between the sizes and their scan: a stream that is no shorter than its
	 * raw chunk gives way to it */
	hipLaunchKernelGGL(lda_exrw_choose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, (const uint64_t *)s.ecols, s.dsize, s.sizes);
	const uint64_t *total_at = chunkw_scan(p, s, st);
	hipLaunchKernelGGL(lda_exrw_place_kernel, dim3(wave_grid(ctx, n)), dim3(256), 0, st, (uint64_t)n,
			   c->level, out_avail, (const uint64_t *)s.ecols, pcol[ZIPW_P_PC_OFF],
			   pcol[ZIPW_P_PC_N], pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n,
			   (const uint64_t *)s.csize, (const uint32_t *)s.sum, (const uint64_t *)s.dsize,
			   (const uint64_t *)s.offs, (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst,
			   s.cp_len, d_index);
	/* copy_src is the raw area, not d_in as in the shuffle and TIFF writers: a
	 * raw chunk's pieces are the same ranges of it */
	return chunkw_finish(ctx, p, s, total_at, out_avail, s.raw, d_out, d_result, st);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_exr_encode_batch(struct libdeflate_compressor *c, size_t n_chunks, const uint64_t *rows,
				const void *d_in, size_t in_avail, void *d_out, size_t out_avail,
				uint64_t *d_result, uint64_t *d_index, void *stream)
{
	/* empty_returns true: of no chunks nothing is queued, and d_result is not
	 * written either.  (At level 0 the stored blocks are longer than raw, so
	 * every chunk goes raw) */
	return chunkw_call<exr_write_plan>("exr_encode_batch", c, n_chunks, rows, d_in, in_avail, d_out,
					   d_result, true, [&](std::string &err) {
		return exr_check(n_chunks, rows, false, 0, in_avail, c->level, err);
	}, [&](const zipw_params &pr, exr_write_plan &p) {
		exr_write_plan_build(pr, n_chunks, rows, p);
	}, [&](const exr_write_plan &p) {
		return exrw_enqueue(c, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result,
				    d_index, (hipStream_t)stream);
	});
}
