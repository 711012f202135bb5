/*
 * host_png.hip - C-ABI of reading PNG files from device memory
 * (include/libdeflate_amd.h), and the decode pipeline of all three decode
 * calls (host_png.h).
 *
 * The index call is one kernel, a lane per file (png_kernels.hip).  A decode
 * takes the index rows and the selection from the host: its plan - png_plan.h
 * here, png_pixels_plan.h and png_adam7_plan.h in the sibling files - checks
 * them and gives every selection its room in the output and in the scratch
 * areas of the object, and the descriptor columns go up in one copy.  Then
 * png_decode_run() queues the steps: the IDAT payloads of every selection
 * gathered into its zlib stream, ONE zlib decompress batch of n_sel chunks over
 * those streams (exact fill of height * (1 + rowbytes) bytes, the
 * wave-per-stream kernel as every other caller launches it), the scanline
 * filters undone - into d_out, or into the scratch where a later step follows -,
 * the deinterlace and the convert of the plans that have them, and the
 * verdicts merged into d_results.  Nothing waits for the device and nothing is
 * read back; every size and launch shape is the plan's.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_png.h"
#include "png_adam7_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNG_UNSUPPORTED == LDA_PNG_UNSUPPORTED &&
	      LIBDEFLATE_AMD_PNG_UNSUPPORTED == LIBDEFLATE_AMD_ZIP_UNSUPPORTED &&
	      LIBDEFLATE_AMD_PNG_UNSUPPORTED == LIBDEFLATE_AMD_TAR_UNSUPPORTED &&
	      LIBDEFLATE_AMD_PNG_WORDS == LDA_PNG_WORDS &&
	      LIBDEFLATE_AMD_PNG_LE16 << 8 == LDA_PNG_META_LE16,
	      "kernels.h holds copies of the header's constants");
static_assert(PNG_UNSUPPORTED == LDA_PNG_UNSUPPORTED && PNG_BAD_DATA == LIBDEFLATE_BAD_DATA &&
	      PNG_ROW_WORDS == LDA_PNG_WORDS && PNG_LE16 == LIBDEFLATE_AMD_PNG_LE16,
	      "png_plan.h holds copies of them too");

static_assert(PNG7_U_RAW_OFF == 0 && PNG7_U_RAW_N == PNG_COL_RAW_N - PNG_COL_RAW_OFF &&
	      PNG7_U_OUT_OFF == PNG_COL_OUT_OFF - PNG_COL_RAW_OFF &&
	      PNG7_U_GEOM == PNG_COL_GEOM - PNG_COL_RAW_OFF &&
	      PNG7_U_META == PNG_COL_META - PNG_COL_RAW_OFF && PNG7_UCOLS == 5,
	      "the unfilter's five columns stand in one order in a selection and in a unit");

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_index_batch(struct libdeflate_decompressor *d, size_t n_files, const void *d_in,
			       const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
			       uint64_t *d_index, int32_t *d_results, void *stream)
{
	const char *what = "png_index_batch";
	if (!d || (n_files && (!d_in || !d_in_offsets || !d_in_nbytes || !d_index || !d_results))) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (n_files > LDA_FINDER_MAX_RECORDS) {
		set_error("%s: n_files %zu (at most 2^28)", what, n_files);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (n_files == 0)
		return LIBDEFLATE_AMD_OK;
	DeviceGuard on(d->device);
	if (!on.ok() || !device_ctx())
		return LIBDEFLATE_AMD_NO_DEVICE;
	hipLaunchKernelGGL(lda_png_index_kernel, dim3((unsigned)((n_files + 255) / 256)), dim3(256), 0,
			   (hipStream_t)stream, (uint64_t)n_files, (uint32_t)0, (const uint8_t *)d_in,
			   d_in_offsets, d_in_nbytes, d_index, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
			     const uint64_t *sel, size_t out_align, uint64_t *out_offsets,
			     uint64_t *total_ret)
{
	const char *what = "png_out_sizes";
	if (!read_sel_args_ok(what, index, entries, n_sel, sel))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!out_offsets) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!read_align_ok(what, out_align))
		return LIBDEFLATE_AMD_BAD_ARG;
	return read_plan_call(what, [&](std::string &err) {
		return png_plan_out_sizes(index, entries, n_sel, sel, out_align - 1, out_offsets,
					  total_ret, err);
	});
}

bool lda::png_decode_args_ok(const char *what, const struct libdeflate_decompressor *d,
			     const void *d_in, size_t in_nbytes, const uint64_t *index, size_t entries,
			     size_t n_sel, const uint64_t *sel, const void *d_out, size_t out_avail,
			     size_t out_align, unsigned flags, unsigned known, const int32_t *d_results)
{
	if (!read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			  out_align, d_results))
		return false;
	if (flags & ~known) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return false;
	}
	return true;
}

int lda::png_decode_run(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
			const PngRun &r, uint8_t *d_out, int32_t *d_results, unsigned stages,
			hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const bool conv_verdicts = r.final != PNG_FINAL_PLAIN;
	/* device: [the areas][the plan's columns][the verdicts: the gather's, the
	 * decoder's and the convert's per selection, the unfilter's per image] */
	uint8_t *g_area = NULL;
	uint64_t *g_cols = NULL;
	int32_t *g_gather = NULL, *g_decode = NULL, *g_unf = NULL, *g_conv = NULL;
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		g_area = cv.take<uint8_t>(r.scratch + 16);
		g_cols = cv.take<uint64_t>(r.cols.size());
		g_gather = cv.take<int32_t>(n_sel);
		g_decode = cv.take<int32_t>(n_sel);
		if (r.final != PNG_FINAL_ADAM7)
			g_unf = cv.take<int32_t>(r.n_verd);
		if (conv_verdicts)
			g_conv = cv.take<int32_t>(n_sel);
		if (r.final == PNG_FINAL_ADAM7)
			g_unf = cv.take<int32_t>(r.n_verd);
		return ReadUp{ g_cols, r.cols.size() * sizeof(uint64_t) };
	}, s));
	memcpy(s.h, r.cols.data(), s.up.bytes);
	LDA_OK_TRY(read_send(d, s, st));
	const auto col = [&](size_t a) { return (const uint64_t *)g_cols + a * n_sel; };
	const auto ucol = [&](size_t a) { return (const uint64_t *)g_cols + r.unf_at + a * r.n_unf; };
	const auto dcol = [&](size_t a) { return (const uint64_t *)g_cols + r.il_at + a * r.n_il; };
	const auto ccol = [&](size_t a) { return (const uint64_t *)g_cols + r.conv_at + a * r.n_conv; };
	/* (a NULL d_out has out_avail 0: every selection is a zero row, nothing is
	 * written and nothing is read) */
	uint8_t *out = d_out ? d_out : s.ws;

	if (stages & PNG_STAGE_GATHER) {
		hipLaunchKernelGGL(lda_png_gather_kernel, dim3(copy_grid(ctx, n_sel)), dim3(256), 0, st,
				   (uint64_t)n_sel, col(PNG_COL_IDAT), col(PNG_COL_END), col(PNG_COL_ZSUM),
				   col(PNG_COL_Z_OFF), d_in, g_area, g_gather);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (stages & PNG_STAGE_INFLATE)
		LDA_OK_TRY(libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_ZLIB, n_sel, g_area,
							   col(PNG_COL_Z_OFF), col(PNG_COL_ZSUM), g_area,
							   col(PNG_COL_RAW_OFF), col(PNG_COL_RAW_N),
							   g_decode, NULL, NULL, st));
	if (r.n_unf && (stages & PNG_STAGE_UNFILTER)) {
		/* an image to the kernel: a selection, or one pass of an interlaced one;
		 * its META says which of the two bases its OUT_OFF counts from */
		hipLaunchKernelGGL(lda_png_unfilter_kernel, dim3(wave_grid(ctx, r.n_unf)), dim3(256), 0,
				   st, (uint64_t)r.n_unf, ucol(PNG7_U_RAW_OFF), ucol(PNG7_U_RAW_N),
				   ucol(PNG7_U_OUT_OFF), ucol(PNG7_U_GEOM), ucol(PNG7_U_META),
				   (const uint8_t *)g_area, out, r.alt ? g_area : out, g_unf);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (r.n_il && (stages & PNG_STAGE_DEINTERLACE)) {
		hipLaunchKernelGGL(lda_png7_deinterlace_kernel, dim3(tile_grid(ctx, r.il_tiles)),
				   dim3(256), 0, st, (uint64_t)r.n_il, r.il_tiles, dcol(PNG7_D_TILE_END),
				   dcol(PNG7_D_PASS), dcol(PNG7_D_SHAPE), dcol(PNG7_D_KIND),
				   dcol(PNG7_D_DST), g_area, out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (conv_verdicts)
		LDA_HIP_TRY(hipMemsetAsync(g_conv, 0, n_sel * sizeof(int32_t), st),
			    LIBDEFLATE_AMD_NO_DEVICE);
	if (r.n_conv && (stages & PNG_STAGE_CONVERT)) {
		hipLaunchKernelGGL(lda_pngx_convert_kernel, dim3(tile_grid(ctx, r.conv_tiles)), dim3(256),
				   0, st, (uint64_t)r.n_conv, r.conv_tiles, (uint32_t)r.format,
				   (uint32_t)r.le16, ccol(PNGX_C_TILE_END), ccol(PNGX_C_SEL),
				   col(PNG_COL_OUT_OFF), ccol(PNGX_C_DST), ccol(PNGX_C_SHAPE),
				   ccol(PNGX_C_KIND), ccol(PNGX_C_PLTE), ccol(PNGX_C_TRNS), d_in,
				   (const uint8_t *)g_area, out, g_conv);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	const dim3 per256((unsigned)((n_sel + 255) / 256));
	if (r.final == PNG_FINAL_PLAIN)
		hipLaunchKernelGGL(lda_png_final_kernel, per256, dim3(256), 0, st, (uint64_t)n_sel,
				   col(PNG_COL_META), (const int32_t *)g_gather, (const int32_t *)g_decode,
				   (const int32_t *)g_unf, d_results);
	else if (r.final == PNG_FINAL_PIXELS)
		hipLaunchKernelGGL(lda_pngx_final_kernel, per256, dim3(256), 0, st, (uint64_t)n_sel,
				   col(PNG_COL_META), (const int32_t *)g_gather, (const int32_t *)g_decode,
				   (const int32_t *)g_unf, (const int32_t *)g_conv, d_results);
	else
		hipLaunchKernelGGL(lda_png7_final_kernel, per256, dim3(256), 0, st, (uint64_t)n_sel,
				   col(PNG_COL_META), col(PNG7_COL_UNITS), (const int32_t *)g_gather,
				   (const int32_t *)g_decode, (const int32_t *)g_unf,
				   (const int32_t *)g_conv, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int png_decode_call(const char *what, struct libdeflate_decompressor *d, const void *d_in,
			   size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			   const uint64_t *sel, void *d_out, size_t out_avail, size_t out_align,
			   unsigned flags, uint64_t *out_offsets, int32_t *d_results,
			   unsigned stages, void *stream)
{
	if (!png_decode_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
				out_align, flags, LIBDEFLATE_AMD_PNG_LE16, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	return read_call<PngRun>(what, d, n_sel, [&](PngRun &r, std::string &err) {
		/* the selections are the images, unfiltered into d_out */
		r.n_unf = r.n_verd = n_sel;
		r.unf_at = PNG_COL_RAW_OFF * n_sel;
		r.final = PNG_FINAL_PLAIN;
		return png_plan_decode(index, entries, n_sel, sel, in_nbytes, out_avail, out_align - 1,
				       flags, r.cols, out_offsets, &r.scratch, err);
	}, [&](const PngRun &r) {
		return png_decode_run(d, (const uint8_t *)d_in, n_sel, r, (uint8_t *)d_out, d_results,
				      stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_decode_batch(struct libdeflate_decompressor *d, const void *d_in,
				size_t in_nbytes, const uint64_t *index, size_t entries,
				size_t n_sel, const uint64_t *sel, void *d_out, size_t out_avail,
				size_t out_align, unsigned flags, uint64_t *out_offsets,
				int32_t *d_results, void *stream)
{
	return png_decode_call("png_decode_batch", d, d_in, in_nbytes, index, entries, n_sel, sel,
			       d_out, out_avail, out_align, flags, out_offsets, d_results,
			       PNG_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 gather, 2 inflate, 4 unfilter), so that tools/bench_png.py can time
 * each alone on scratch an earlier full call has filled; d_results then mixes
 * verdicts of this call and of that one */
extern "C" LIBDEFLATEAPI int
lda_png_decode_stages(struct libdeflate_decompressor *d, const void *d_in, size_t in_nbytes,
		      const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel,
		      void *d_out, size_t out_avail, size_t out_align, unsigned flags,
		      uint64_t *out_offsets, int32_t *d_results, unsigned stages, void *stream)
{
	return png_decode_call("png_decode_stages", d, d_in, in_nbytes, index, entries, n_sel, sel,
			       d_out, out_avail, out_align, flags, out_offsets, d_results,
			       stages & (PNG_STAGE_GATHER | PNG_STAGE_INFLATE | PNG_STAGE_UNFILTER),
			       stream);
}
