/*
 * host_tiff.hip - C-ABI of reading predictor-coded deflate strips and tiles
 * (TIFF, GeoTIFF) from device memory (include/libdeflate_amd.h:
 * libdeflate_amd_tiff_decode_batch).
 *
 * tiff_plan.h checks the rows and classifies them; its columns go up through
 * the object's pinned block in ONE copy.  The direct rows - predictor 1, kept
 * whole at their own pitch - are decoded straight into d_out and every other
 * row into a room of the object's scratch: one decompress batch per output
 * base, each left out when it has no row.  Then lda_tiff_unpredict_kernel
 * (tiff_kernels.hip) scans the kept rows - predictors 1 and 2 from the rooms
 * into the kept rectangles of d_out, predictor 3 the byte planes in place -,
 * lda_tiff_gather_kernel collects the kept pixels of the predictor-3 rows, and
 * the verdicts are merged (lda_shuf_final_kernel).  A batch that is direct
 * throughout queues what libdeflate_amd_decompress_batch queues, and the
 * verdict kernel.  Nothing waits for the device and nothing is read back.
 * d->bgzf: [the scratch rooms][the plan's columns][the decoder's results].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "tiff_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_TIFF_WORDS == TIFF_WORDS && LDA_TIFF_WORDS == TIFF_WORDS &&
	      LIBDEFLATE_AMD_TIFF_SPP_MAX == TIFF_SPP_MAX && LDA_TIFF_SPP_MAX == TIFF_SPP_MAX &&
	      LIBDEFLATE_AMD_TIFFW_RESULT_WORDS == TIFF_RESULT_WORDS &&
	      LDA_TIFF_PTILE == TIFF_PTILE && LDA_TIFF_DST_WS == TIFF_DST_WS &&
	      LIBDEFLATE_AMD_ZLIB == 1,
	      "tiff_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_tiff_stages) */
enum { TIFF_STAGE_INFLATE = 1, TIFF_STAGE_UNPREDICT = 2, TIFF_STAGE_ALL = 3 };

static int tiff_decode(struct libdeflate_decompressor *d, const tiff_read_plan &p, const uint8_t *d_in,
		       uint8_t *d_out, int32_t *d_results, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n, n_k = (size_t)p.n_k, n_g = (size_t)p.n_g;
	uint8_t *g_area = NULL;
	ChunkStage g;
	LDA_OK_TRY(chunk_stage(d, p.cols, n, d_in, d_out, st, g, [&](Carve &cv) {
		/* (128 to spare: the scan reads a row's tail as a whole piece of up to 64 bytes) */
		g_area = cv.take<uint8_t>((size_t)p.scratch + 128, 256);
	}));
	const uint64_t *gcol[TIFF_GCOLS];
	for (size_t a = 0; a < TIFF_GCOLS; a++)
		gcol[a] = g.cols + p.g_at + a * n_g;

	/* (every row has pixels inside out_avail: d_out is not NULL here, and g.out is d_out) */
	if (stages & TIFF_STAGE_INFLATE)
		LDA_OK_TRY(chunk_inflate(d, LIBDEFLATE_AMD_ZLIB, g, (size_t)p.n_ws, g_area,
					 (size_t)p.n_direct, st));
	if (p.quads && (stages & TIFF_STAGE_UNPREDICT)) {
		hipLaunchKernelGGL(lda_tiff_unpredict_kernel, dim3(tile_grid(ctx, (p.quads + 63) / 64)),
				   dim3(256), 0, st, (uint64_t)n_k, p.quads,
				   (const uint64_t *)(g.cols + p.k_at), g_area, g.out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (p.gtiles && (stages & TIFF_STAGE_UNPREDICT)) {
		hipLaunchKernelGGL(lda_tiff_gather_kernel, dim3(tile_grid(ctx, p.gtiles)),
				   dim3(256), 0, st, (uint64_t)n_g, p.gtiles, gcol[TIFF_G_TILE_END],
				   gcol[TIFF_G_SRC], gcol[TIFF_G_DST], gcol[TIFF_G_DPITCH],
				   gcol[TIFF_G_GEOM], gcol[TIFF_G_PLANE], (const uint8_t *)g_area, g.out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	return chunk_verdicts(g, n, p.verd_at, d_results, st);
}

static int tiff_call(const char *what, struct libdeflate_decompressor *d, size_t n_segments,
		     const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		     size_t out_avail, int32_t *d_results, unsigned stages, void *stream)
{
	return chunk_read_call<tiff_read_plan>(what, d, n_segments, rows, d_in, in_nbytes, d_out, out_avail,
					       d_results, [&](tiff_read_plan &p, std::string &err) {
		if (!tiff_check(n_segments, rows, true, in_nbytes, out_avail, -1, err))
			return false;
		tiff_read_plan_build(n_segments, rows, p);
		return true;
	}, [&](const tiff_read_plan &p) {
		return tiff_decode(d, p, (const uint8_t *)d_in, (uint8_t *)d_out, d_results, stages,
				   (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tiff_decode_batch(struct libdeflate_decompressor *d, size_t n_segments,
				 const uint64_t *rows, const void *d_in, size_t in_nbytes,
				 void *d_out, size_t out_avail, int32_t *d_results, void *stream)
{
	return tiff_call("tiff_decode_batch", d, n_segments, rows, d_in, in_nbytes, d_out, out_avail,
			 d_results, TIFF_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 inflate, 2 unpredict and gather; 0: the upload and the verdict
 * kernel alone), so that tools/bench_tiff.py can time the unpredict stage alone
 * on scratch an earlier full call has filled.  (A predictor-3 row's scan runs
 * in place: a second pass over the same scratch sums sums - the time is the
 * same, the pixels are not) */
extern "C" LIBDEFLATEAPI int
lda_tiff_stages(struct libdeflate_decompressor *d, size_t n_segments, const uint64_t *rows,
		const void *d_in, size_t in_nbytes, void *d_out, size_t out_avail,
		int32_t *d_results, unsigned stages, void *stream)
{
	return tiff_call("tiff_stages", d, n_segments, rows, d_in, in_nbytes, d_out, out_avail,
			 d_results, stages & TIFF_STAGE_ALL, stream);
}
