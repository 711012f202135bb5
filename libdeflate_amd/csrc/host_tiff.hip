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
	uint64_t *g_cols = NULL;
	int32_t *g_decode = NULL;
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		/* (128 to spare: the scan reads a row's tail as a whole piece of up to 64 bytes) */
		g_area = cv.take<uint8_t>((size_t)p.scratch + 128, 256);
		g_cols = cv.take<uint64_t>(p.cols.size());
		g_decode = cv.take<int32_t>(n + 1);
		return ReadUp{ g_cols, p.cols.size() * sizeof(uint64_t) };
	}, s));
	memcpy(s.h, p.cols.data(), s.up.bytes);
	LDA_OK_TRY(read_send(d, s, st));
	uint8_t *ws = s.ws;
	const uint64_t *dcol[TIFF_DCOLS], *gcol[TIFF_GCOLS];
	for (size_t a = 0; a < TIFF_DCOLS; a++)
		dcol[a] = g_cols + a * n;
	for (size_t a = 0; a < TIFF_GCOLS; a++)
		gcol[a] = g_cols + p.g_at + a * n_g;
	/* (NULL d_in: in_nbytes is 0, and so is every stored size) */
	const uint8_t *in = d_in ? d_in : ws;

	/* the scratch rows stand first in the columns, the d_out rows behind them */
	for (int k = 0; k < 2 && (stages & TIFF_STAGE_INFLATE); k++) {
		const size_t lo = k ? (size_t)p.n_ws : 0, cnt = (size_t)(k ? p.n_direct : p.n_ws);
		if (!cnt)
			continue;
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_ZLIB, cnt, in,
							 dcol[TIFF_D_IN_OFF] + lo, dcol[TIFF_D_IN_N] + lo,
							 k ? d_out : g_area, dcol[TIFF_D_OUT_OFF] + lo,
							 dcol[TIFF_D_OUT_N] + lo, g_decode + lo, NULL,
							 NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (p.quads && (stages & TIFF_STAGE_UNPREDICT)) {
		hipLaunchKernelGGL(lda_tiff_unpredict_kernel, dim3(tile_grid(ctx, (p.quads + 63) / 64)),
				   dim3(256), 0, st, (uint64_t)n_k, p.quads,
				   (const uint64_t *)(g_cols + p.k_at), g_area, d_out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (p.gtiles && (stages & TIFF_STAGE_UNPREDICT)) {
		hipLaunchKernelGGL(lda_tiff_gather_kernel, dim3(tile_grid(ctx, p.gtiles)),
				   dim3(256), 0, st, (uint64_t)n_g, p.gtiles, gcol[TIFF_G_TILE_END],
				   gcol[TIFF_G_SRC], gcol[TIFF_G_DST], gcol[TIFF_G_DPITCH],
				   gcol[TIFF_G_GEOM], gcol[TIFF_G_PLANE], (const uint8_t *)g_area, d_out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_shuf_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, (const uint64_t *)(g_cols + p.verd_at),
			   (const int32_t *)g_decode, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int tiff_call(const char *what, struct libdeflate_decompressor *d, size_t n_segments,
		     const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		     size_t out_avail, int32_t *d_results, unsigned stages, void *stream)
{
	if (!d || (n_segments && (!rows || !d_results)) || (!d_in && in_nbytes) ||
	    (!d_out && out_avail)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return read_call<tiff_read_plan>(what, d, n_segments, [&](tiff_read_plan &p, std::string &err) {
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
