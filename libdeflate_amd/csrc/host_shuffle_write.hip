/*
 * host_shuffle_write.hip - C-ABI of writing byte-shuffled deflate chunks (HDF5,
 * NetCDF-4, Zarr) in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_shuffle_compress_batch).
 *
 * shuffle_plan.h checks the rows, gives every chunk a room for its shuffled
 * bytes in the object's scratch and cuts the rooms into pieces; its columns go
 * up; lda_shuffle_kernel (shuffle_kernels.hip) fills the rooms from the raw
 * bytes in d_in - identity and NO_SHUFFLE chunks are copied there as element
 * size 1, because the piece pipeline compresses from one source base -; ONE
 * Adler-32 (zlib) or CRC-32 (gzip) batch runs over the pieces in the rooms, the
 * pieces are compressed into slots (the shared piece pipeline,
 * host_write_pieces.hip), and the kernels of shuffle_kernels.hip size the
 * streams and place headers and footers.
 * c->zipw: [chunk columns, kernel rows][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize][sum]
 * [sums][rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "shuffle_plan.h"

using namespace lda;

/* the stages of a call; the benchmark times each alone (lda_shuffle_write_stages) */
enum { SHUFW_STAGE_SHUFFLE = 1, SHUFW_STAGE_COMPRESS = 2, SHUFW_STAGE_ASSEMBLE = 4, SHUFW_STAGE_ALL = 7 };

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_shuffle_compress_bound(struct libdeflate_compressor *c, int format, size_t n_chunks,
				      const uint64_t *chunks)
{
	(void)c;	/* (no level has another bound: libdeflate_<format>_compress_bound()) */
	return chunkw_bound_call("shuffle_compress_bound", n_chunks, chunks,
				 [&] { return shuf_bound(format, n_chunks, chunks); });
}

static int shufw_enqueue(struct libdeflate_compressor *c, int format, const shuf_write_plan &p,
			 const uint8_t *d_in, uint8_t *d_out, uint64_t out_avail, uint64_t *d_result,
			 uint64_t *d_index, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n, n_u = (size_t)p.n_u;
	const std::vector<zipw_launch> launches = zipw_launches(p);
	ChunkwScratch s;

	LDA_OK_TRY(chunkw_begin(c, p, launches, st, s));
	const uint64_t *ucol[SHUF_UCOLS];
	for (size_t a = 0; a < SHUF_UCOLS; a++)
		ucol[a] = s.ecols + SHUFW_ECOLS * n + a * n_u;

	/* the stages are gated here and nowhere else: lda_shuffle_write_stages
	 * times each alone, and without ASSEMBLE the call ends behind the compress */
	if (p.tiles && (stages & SHUFW_STAGE_SHUFFLE)) {
		hipLaunchKernelGGL(lda_shuffle_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n_u, p.tiles, ucol[SHUF_U_TILE_END], ucol[SHUF_U_SRC], ucol[SHUF_U_DST],
				   ucol[SHUF_U_GEOM], d_in, s.rooms);
	}
	if (stages & SHUFW_STAGE_COMPRESS)
		LDA_OK_TRY(chunkw_compress(c, format, p, s, launches, s.rooms, st));
	if (!(stages & SHUFW_STAGE_ASSEMBLE)) {
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	chunkw_sizes(ctx, format, p, s, st);
	const uint64_t *total_at = chunkw_scan(p, s, st);
	chunkw_place(ctx, format, c->level, p, s, out_avail, d_out, d_index, st);
	/* (copy_src is d_in, as the TIFF writer's; the OpenEXR writer's is its raw area) */
	return chunkw_finish(ctx, p, s, total_at, out_avail, d_in, d_out, d_result, st);
}

static int shufw_call(const char *what, struct libdeflate_compressor *c, int format, size_t n_chunks,
		      const uint64_t *chunks, const void *d_in, size_t in_avail, void *d_out,
		      size_t out_avail, uint64_t *d_result, uint64_t *d_index, unsigned stages,
		      void *stream)
{
	/* empty_returns false: of no chunks the scan of nothing and the final
	 * kernel are still queued, and d_result is written */
	return chunkw_call<shuf_write_plan>(what, c, n_chunks, chunks, d_in, in_avail, d_out, d_result, false,
					    [&](std::string &err) {
		return shuf_check(format, n_chunks, chunks, false, 0, in_avail, c->level, err);
	}, [&](const zipw_params &pr, shuf_write_plan &p) {
		shuf_write_plan_build(pr, n_chunks, chunks, p);
	}, [&](const shuf_write_plan &p) {
		return shufw_enqueue(c, format, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail,
				     d_result, d_index, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_shuffle_compress_batch(struct libdeflate_compressor *c, int format, size_t n_chunks,
				      const uint64_t *chunks, const void *d_in, size_t in_avail,
				      void *d_out, size_t out_avail, uint64_t *d_result,
				      uint64_t *d_index, void *stream)
{
	return shufw_call("shuffle_compress_batch", c, format, n_chunks, chunks, d_in, in_avail, d_out,
			  out_avail, d_result, d_index, SHUFW_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 the shuffle kernel, 2 checksums and compress, 4 the assembly), so
 * that tools/bench_shuffle.py can time each alone on scratch an earlier full
 * call has filled */
extern "C" LIBDEFLATEAPI int
lda_shuffle_write_stages(struct libdeflate_compressor *c, int format, size_t n_chunks,
			 const uint64_t *chunks, const void *d_in, size_t in_avail, void *d_out,
			 size_t out_avail, uint64_t *d_result, uint64_t *d_index, unsigned stages,
			 void *stream)
{
	return shufw_call("shuffle_write_stages", c, format, n_chunks, chunks, d_in, in_avail, d_out,
			  out_avail, d_result, d_index, stages & SHUFW_STAGE_ALL, stream);
}
