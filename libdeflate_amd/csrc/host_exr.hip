/*
 * host_exr.hip - C-ABI of reading OpenEXR ZIP and ZIPS chunks, scanline blocks
 * and tiles, from device memory (include/libdeflate_amd.h:
 * libdeflate_amd_exr_decode_batch).
 *
 * exr_plan.h checks the rows and puts each in its class; its columns go up
 * through the object's pinned block in ONE copy.  The zlib rows are decoded
 * into rooms of the object's scratch in ONE decompress batch; the raw rows
 * that are direct are spans of lda_zip_copy_kernel.  Then the three launches
 * that undo the coding (exr_kernels.hip: lda_exr_sums_kernel,
 * lda_exr_carry_kernel, lda_exr_undo_kernel) turn every room into the raw
 * chunk - of a direct row straight in d_out, of any other in a second room -,
 * lda_exr_layout_kernel lays the remaining raw chunks out, those of raw rows
 * straight from d_in, and the verdicts are merged (lda_shuf_final_kernel).  A
 * batch of direct raw rows queues the copy kernel and the verdict kernel.
 * Nothing waits for the device and nothing is read back.
 * d->bgzf: [the coded rooms][the raw rooms][the slots][the plan's columns]
 * [the decoder's results].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "exr_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_EXR_WORDS == EXR_WORDS && LDA_EXR_WORDS == EXR_WORDS &&
	      LIBDEFLATE_AMD_EXR_CHANNELS_MAX == EXR_CHANNELS_MAX &&
	      LIBDEFLATE_AMD_EXRW_RESULT_WORDS == EXR_RESULT_WORDS &&
	      LIBDEFLATE_AMD_EXR_LINES == EXR_LINES && LIBDEFLATE_AMD_EXR_PIXELS == EXR_PIXELS &&
	      LDA_EXR_LAYOUT_LINES == EXR_LINES && LDA_EXR_LANE == EXR_LANE &&
	      LDA_EXR_TILE == EXR_TILE && EXR_TILE == 64 * EXR_LANE &&
	      LDA_EXR_WG_TILES == EXR_WG_TILES && LDA_EXR_LTILE == EXR_LTILE &&
	      LDA_EXR_CTILE == EXR_CTILE && LDA_EXRW_E_WORDS == EXRW_E_WORDS &&
	      LDA_EXR_DST_OUT == EXR_DST_OUT && LDA_EXR_RAW_IN == EXR_RAW_IN &&
	      LDA_SHUF_VERD_OWN == EXR_VERD_OWN && LIBDEFLATE_AMD_ZLIB == 1,
	      "exr_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_exr_stages) */
enum { EXR_STAGE_INFLATE = 1, EXR_STAGE_UNDO = 2, EXR_STAGE_ALL = 3 };

static int exr_decode(struct libdeflate_decompressor *d, const exr_read_plan &p, const uint8_t *d_in,
		      uint8_t *d_out, int32_t *d_results, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n, n_z = (size_t)p.n_z, n_c = (size_t)p.n_copy, n_l = (size_t)p.n_l;
	uint8_t *g_coded = NULL, *g_raw = NULL;
	uint32_t *g_slots = NULL;
	ChunkStage g;
	LDA_OK_TRY(chunk_stage(d, p.cols, n_z, d_in, d_out, st, g, [&](Carve &cv) {
		g_coded = cv.take<uint8_t>((size_t)p.coded_bytes + 16, 256);
		g_raw = cv.take<uint8_t>((size_t)p.raw_bytes + 16, 256);
		g_slots = cv.take<uint32_t>((size_t)(2 * p.utiles) + 1);
	}));
	const uint64_t *pcol[EXR_PCOLS];
	for (size_t a = 0; a < EXR_PCOLS; a++)
		pcol[a] = g.cols + p.p_at + a * n_c;
	const uint64_t *ucols = g.cols + p.u_at, *lcols = g.cols + p.l_at;
	const uint8_t *in = g.in;
	uint8_t *out = g.out;

	if (stages & EXR_STAGE_INFLATE)
		LDA_OK_TRY(chunk_inflate(d, LIBDEFLATE_AMD_ZLIB, g, n_z, g_coded, 0, st));
	if (n_c && (stages & EXR_STAGE_UNDO))
		hipLaunchKernelGGL(lda_zip_copy_kernel, dim3(copy_grid(ctx, n_c)), dim3(256), 0, st,
				   (uint64_t)n_c, pcol[EXR_P_SRC], pcol[EXR_P_DST], pcol[EXR_P_LEN], in,
				   out);
	if (p.utiles && (stages & EXR_STAGE_UNDO)) {
		const unsigned grid = tile_grid(ctx, (p.utiles + EXR_WG_TILES - 1) / EXR_WG_TILES);
		hipLaunchKernelGGL(lda_exr_sums_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n_z,
				   p.utiles, ucols, (const uint8_t *)g_coded, g_slots);
		hipLaunchKernelGGL(lda_exr_carry_kernel, dim3(wave_grid(ctx, n_z)), dim3(256), 0, st,
				   (uint64_t)n_z, ucols + EXR_U_TILE_END * n_z, g_slots);
		hipLaunchKernelGGL(lda_exr_undo_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n_z,
				   p.utiles, ucols, (const uint8_t *)g_coded, (const uint32_t *)g_slots,
				   g_raw, out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (p.ltiles && (stages & EXR_STAGE_UNDO)) {
		hipLaunchKernelGGL(lda_exr_layout_kernel, dim3(tile_grid(ctx, p.ltiles)), dim3(256), 0, st,
				   (uint64_t)n_l, p.ltiles, lcols, in, (const uint8_t *)g_raw, out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	return chunk_verdicts(g, n, p.verd_at, d_results, st);
}

static int exr_call(const char *what, struct libdeflate_decompressor *d, size_t n_chunks,
		    const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		    size_t out_avail, int32_t *d_results, unsigned stages, void *stream)
{
	return chunk_read_call<exr_read_plan>(what, d, n_chunks, rows, d_in, in_nbytes, d_out, out_avail,
					      d_results, [&](exr_read_plan &p, std::string &err) {
		if (!exr_check(n_chunks, rows, true, in_nbytes, out_avail, -1, err))
			return false;
		exr_read_plan_build(n_chunks, rows, p);
		return true;
	}, [&](const exr_read_plan &p) {
		return exr_decode(d, p, (const uint8_t *)d_in, (uint8_t *)d_out, d_results, stages,
				  (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_exr_decode_batch(struct libdeflate_decompressor *d, size_t n_chunks,
				const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
				size_t out_avail, int32_t *d_results, void *stream)
{
	return exr_call("exr_decode_batch", d, n_chunks, rows, d_in, in_nbytes, d_out, out_avail,
			d_results, EXR_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 inflate, 2 the copy, undo and layout kernels; 0: the upload and the
 * verdict kernel alone), so that tools/bench_exr.py can time the transform
 * kernels alone on scratch an earlier full call has filled */
extern "C" LIBDEFLATEAPI int
lda_exr_stages(struct libdeflate_decompressor *d, size_t n_chunks, const uint64_t *rows,
	       const void *d_in, size_t in_nbytes, void *d_out, size_t out_avail, int32_t *d_results,
	       unsigned stages, void *stream)
{
	return exr_call("exr_stages", d, n_chunks, rows, d_in, in_nbytes, d_out, out_avail, d_results,
			stages & EXR_STAGE_ALL, stream);
}
