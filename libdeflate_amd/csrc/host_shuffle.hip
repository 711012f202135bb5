/*
 * host_shuffle.hip - C-ABI of reading byte-shuffled deflate chunks (HDF5,
 * NetCDF-4, Zarr) from device memory (include/libdeflate_amd.h:
 * libdeflate_amd_shuffle_decompress_batch).
 *
 * shuffle_plan.h checks the rows and classifies them; its columns go up through
 * the object's pinned block in ONE copy.  The deflated, shuffled rows are
 * decoded into rooms of the object's scratch and the deflated rows whose
 * transform is the identity straight into their rooms of d_out: one decompress
 * batch per output base, each left out when it has no row.  Then
 * lda_unshuffle_kernel (shuffle_kernels.hip) writes the rooms of the shuffled
 * rows - the NO_DEFLATE ones from their stored bytes in d_in -, and the
 * verdicts are merged.  A batch that is identity throughout queues what
 * libdeflate_amd_decompress_batch queues, and the verdict kernel.  Nothing
 * waits for the device and nothing is read back.
 * d->bgzf: [the scratch rooms][the plan's columns][the decoder's results].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "shuffle_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_SHUF_WORDS == SHUF_WORDS &&
	      LIBDEFLATE_AMD_SHUF_ELEM_MAX == SHUF_ELEM_MAX &&
	      LIBDEFLATE_AMD_SHUF_NO_DEFLATE == SHUF_NO_DEFLATE &&
	      LIBDEFLATE_AMD_SHUF_NO_SHUFFLE == SHUF_NO_SHUFFLE &&
	      LIBDEFLATE_AMD_SHUFW_RESULT_WORDS == SHUF_RESULT_WORDS &&
	      LDA_SHUF_TILE == SHUF_TILE && LDA_SHUF_GEN_BYTES == SHUF_GEN_BYTES &&
	      LDA_SHUF_SRC_ALT == SHUF_SRC_ALT && LDA_SHUF_VERD_OWN == SHUF_VERD_OWN &&
	      LIBDEFLATE_AMD_DEFLATE == 0 && LIBDEFLATE_AMD_ZLIB == 1 && LIBDEFLATE_AMD_GZIP == 2,
	      "shuffle_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_shuffle_stages) */
enum { SHUF_STAGE_INFLATE = 1, SHUF_STAGE_UNSHUFFLE = 2, SHUF_STAGE_ALL = 3 };

static int shuf_decode(struct libdeflate_decompressor *d, int format, const shuf_read_plan &p,
		       const uint8_t *d_in, uint8_t *d_out, int32_t *d_results, unsigned stages,
		       hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n_u = (size_t)p.n_u;
	uint8_t *g_area = NULL;
	ChunkStage g;
	LDA_OK_TRY(chunk_stage(d, p.cols, (size_t)(p.n_sd + p.n_id), d_in, d_out, st, g, [&](Carve &cv) {
		g_area = cv.take<uint8_t>((size_t)p.scratch + 16, 256);
	}));
	const uint64_t *ucol[SHUF_UCOLS];
	for (size_t a = 0; a < SHUF_UCOLS; a++)
		ucol[a] = g.cols + p.u_at + a * n_u;

	if (stages & SHUF_STAGE_INFLATE)
		LDA_OK_TRY(chunk_inflate(d, format, g, (size_t)p.n_sd, g_area, (size_t)p.n_id, st));
	if (p.tiles && (stages & SHUF_STAGE_UNSHUFFLE)) {
		hipLaunchKernelGGL(lda_unshuffle_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n_u, p.tiles, ucol[SHUF_U_TILE_END], ucol[SHUF_U_SRC],
				   ucol[SHUF_U_DST], ucol[SHUF_U_GEOM], (const uint8_t *)g_area, g.in, g.out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	return chunk_verdicts(g, (size_t)p.n, p.verd_at, d_results, st);
}

static int shuf_call(const char *what, struct libdeflate_decompressor *d, int format, size_t n_chunks,
		     const uint64_t *chunks, const void *d_in, size_t in_nbytes, void *d_out,
		     size_t out_avail, int32_t *d_results, unsigned stages, void *stream)
{
	return chunk_read_call<shuf_read_plan>(what, d, n_chunks, chunks, d_in, in_nbytes, d_out, out_avail,
					       d_results, [&](shuf_read_plan &p, std::string &err) {
		if (!shuf_check(format, n_chunks, chunks, true, in_nbytes, out_avail, -1, err))
			return false;
		shuf_read_plan_build(n_chunks, chunks, p);
		return true;
	}, [&](const shuf_read_plan &p) {
		return shuf_decode(d, format, p, (const uint8_t *)d_in, (uint8_t *)d_out, d_results,
				   stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_shuffle_decompress_batch(struct libdeflate_decompressor *d, int format,
					size_t n_chunks, const uint64_t *chunks, const void *d_in,
					size_t in_nbytes, void *d_out, size_t out_avail,
					int32_t *d_results, void *stream)
{
	return shuf_call("shuffle_decompress_batch", d, format, n_chunks, chunks, d_in, in_nbytes,
			 d_out, out_avail, d_results, SHUF_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 inflate, 2 unshuffle; 0: the upload and the verdict kernel alone),
 * so that tools/bench_shuffle.py can time the unshuffle stage alone on scratch
 * an earlier full call has filled */
extern "C" LIBDEFLATEAPI int
lda_shuffle_stages(struct libdeflate_decompressor *d, int format, size_t n_chunks,
		   const uint64_t *chunks, const void *d_in, size_t in_nbytes, void *d_out,
		   size_t out_avail, int32_t *d_results, unsigned stages, void *stream)
{
	return shuf_call("shuffle_stages", d, format, n_chunks, chunks, d_in, in_nbytes, d_out,
			 out_avail, d_results, stages & SHUF_STAGE_ALL, stream);
}
