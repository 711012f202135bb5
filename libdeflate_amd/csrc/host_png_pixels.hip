/*
 * host_png_pixels.hip - C-ABI of decoding PNG files from device memory to one
 * pixel format (include/libdeflate_amd.h): libdeflate_amd_png_decode_batch's
 * steps (host_png.hip) with the plan of png_pixels_plan.h.  The gather and the
 * ONE zlib decompress batch run over all selections as they do there, and so
 * does the unfilter, in one launch: a selection that already is the format is
 * written into its room of d_out, the others into the scratch (the kernel's
 * second base, LDA_PNG_META_ALT).  Then the convert kernel writes the rooms of
 * the second kind (png_pixels_kernels.hip), and the verdicts are merged.  A
 * batch that is direct throughout uploads and launches what
 * libdeflate_amd_png_decode_batch does, and one memset and a verdict kernel of
 * one more input.  Nothing waits for the device and nothing is read back.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_zip_args.h"
#include "png_pixels_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNG_GRAY == PNGX_GRAY && LIBDEFLATE_AMD_PNG_GRAY_ALPHA == PNGX_GRAY_ALPHA &&
	      LIBDEFLATE_AMD_PNG_RGB == PNGX_RGB && LIBDEFLATE_AMD_PNG_RGBA == PNGX_RGBA &&
	      LIBDEFLATE_AMD_PNG_OUT16 == PNGX_OUT16 && LDA_PNGX_OUT16 == PNGX_OUT16 &&
	      LDA_PNGX_TILE == PNGX_TILE && LDA_PNGX_KIND_KEY == PNGX_KIND_KEY &&
	      LDA_PNG_META_ALT == PNGX_META_ALT,
	      "png_pixels_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a decode; the benchmark times each alone (lda_png_pixels_stages) */
enum {
	PNGX_STAGE_GATHER = 1, PNGX_STAGE_INFLATE = 2, PNGX_STAGE_UNFILTER = 4,
	PNGX_STAGE_CONVERT = 8, PNGX_STAGE_ALL = 15
};

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_pixels_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
				    const uint64_t *sel, unsigned format, size_t out_align,
				    uint64_t *out_offsets, uint64_t *total_ret)
{
	const char *what = "png_pixels_out_sizes";
	if ((!index && entries) || (n_sel && !sel) || !out_offsets) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (entries > LDA_FINDER_MAX_RECORDS || n_sel > LDA_FINDER_MAX_RECORDS) {
		set_error("%s: entries %zu, n_sel %zu (at most 2^28)", what, entries, n_sel);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!zip_align_ok(what, out_align))
		return LIBDEFLATE_AMD_BAD_ARG;
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!png_pixels_plan_out_sizes(index, entries, n_sel, sel, format, out_align - 1,
					       out_offsets, total_ret, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		return LIBDEFLATE_AMD_OK;
	});
}

/* as host_png.hip's: four waves to a workgroup, sixteen workgroups to a CU */
static unsigned unfilter_grid(const DeviceCtx *ctx, size_t n_sel)
{
	return (unsigned)std::max((size_t)1, std::min((n_sel + 3) / 4, (size_t)ctx->num_cus * 16));
}

/* the convert kernel's workgroups stride over the tiles: eight to a CU fill
 * its wave slots */
static unsigned convert_grid(const DeviceCtx *ctx, uint64_t tiles)
{
	return (unsigned)std::min(tiles, (uint64_t)ctx->num_cus * 8);
}

static int pngx_decode(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		       const std::vector<uint64_t> &cols, const PngxPlan &plan, unsigned format,
		       unsigned flags, uint8_t *d_out, int32_t *d_results, unsigned stages,
		       hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n_conv = (size_t)plan.n_conv;
	/* device: [the three areas][the plan's columns][the four verdicts] */
	uint8_t *g_area = NULL;
	uint64_t *g_cols = NULL;
	int32_t *g_gather = NULL, *g_decode = NULL, *g_unf = NULL, *g_conv = NULL;
	const size_t up_words = cols.size(), up_bytes = up_words * sizeof(uint64_t);
	auto lay = [&](Carve *cv) {
		g_area = cv->take<uint8_t>(plan.scratch + 16);
		g_cols = cv->take<uint64_t>(up_words);
		g_gather = cv->take<int32_t>(n_sel);
		g_decode = cv->take<int32_t>(n_sel);
		g_unf = cv->take<int32_t>(n_sel);
		g_conv = cv->take<int32_t>(n_sel);
	};
	Carve sizes(NULL);
	lay(&sizes);
	LDA_OK_TRY(d->bgzf_up.begin());
	uint8_t *ws = (uint8_t *)d->bgzf.reserve(sizes.at + 16);
	void *h = d->bgzf_up.pinned(up_bytes);
	if (!ws || !h)
		return LIBDEFLATE_AMD_OOM;
	Carve real(ws);
	lay(&real);
	memcpy(h, cols.data(), up_bytes);
	LDA_OK_TRY(d->bgzf_up.send(g_cols, up_bytes, st));
	const uint64_t *col[PNG_COLS], *ccol[PNGX_CCOLS];
	for (size_t a = 0; a < PNG_COLS; a++)
		col[a] = g_cols + a * n_sel;
	for (size_t a = 0; a < PNGX_CCOLS; a++)
		ccol[a] = g_cols + plan.conv_at + a * n_conv;
	/* (a NULL d_out has out_avail 0: every selection is a zero row) */
	uint8_t *out = d_out ? d_out : ws;

	if (stages & PNGX_STAGE_GATHER) {
		hipLaunchKernelGGL(lda_png_gather_kernel, dim3(zip_copy_grid(ctx, n_sel)), dim3(256), 0,
				   st, (uint64_t)n_sel, col[PNG_COL_IDAT], col[PNG_COL_END],
				   col[PNG_COL_ZSUM], col[PNG_COL_Z_OFF], d_in, g_area, g_gather);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (stages & PNGX_STAGE_INFLATE) {
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_ZLIB, n_sel, g_area,
						     col[PNG_COL_Z_OFF], col[PNG_COL_ZSUM], g_area,
						     col[PNG_COL_RAW_OFF], col[PNG_COL_RAW_N], g_decode,
						     NULL, NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (stages & PNGX_STAGE_UNFILTER) {
		/* the direct selections into d_out, the others into the scratch */
		hipLaunchKernelGGL(lda_png_unfilter_kernel, dim3(unfilter_grid(ctx, n_sel)), dim3(256),
				   0, st, (uint64_t)n_sel, col[PNG_COL_RAW_OFF], col[PNG_COL_RAW_N],
				   col[PNG_COL_OUT_OFF], col[PNG_COL_GEOM], col[PNG_COL_META],
				   (const uint8_t *)g_area, out, g_area, g_unf);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	LDA_HIP_TRY(hipMemsetAsync(g_conv, 0, n_sel * sizeof(int32_t), st), LIBDEFLATE_AMD_NO_DEVICE);
	if (n_conv && (stages & PNGX_STAGE_CONVERT)) {
		hipLaunchKernelGGL(lda_pngx_convert_kernel, dim3(convert_grid(ctx, plan.tiles)),
				   dim3(256), 0, st, (uint64_t)n_conv, plan.tiles, (uint32_t)format,
				   (uint32_t)(flags & PNG_LE16), ccol[PNGX_C_TILE_END], ccol[PNGX_C_SEL],
				   col[PNG_COL_OUT_OFF], ccol[PNGX_C_DST], ccol[PNGX_C_SHAPE],
				   ccol[PNGX_C_KIND], ccol[PNGX_C_PLTE], ccol[PNGX_C_TRNS], d_in,
				   (const uint8_t *)g_area, out, g_conv);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_pngx_final_kernel, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0,
			   st, (uint64_t)n_sel, col[PNG_COL_META], (const int32_t *)g_gather,
			   (const int32_t *)g_decode, (const int32_t *)g_unf,
			   (const int32_t *)g_conv, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int pngx_call(const char *what, struct libdeflate_decompressor *d, const void *d_in,
		     size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
		     const uint64_t *sel, unsigned format, void *d_out, size_t out_avail,
		     size_t out_align, unsigned flags, uint64_t *out_offsets, int32_t *d_results,
		     unsigned stages, void *stream)
{
	if (!zip_read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			      out_align, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (flags & ~(unsigned)LIBDEFLATE_AMD_PNG_LE16) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::vector<uint64_t> cols;
		std::string err;
		PngxPlan plan;
		if (!png_pixels_plan(index, entries, n_sel, sel, format, in_nbytes, out_avail,
				     out_align - 1, flags, cols, out_offsets, &plan, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_sel == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return pngx_decode(d, (const uint8_t *)d_in, n_sel, cols, plan, format, flags,
				   (uint8_t *)d_out, d_results, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_decode_pixels_batch(struct libdeflate_decompressor *d, const void *d_in,
				       size_t in_nbytes, const uint64_t *index, size_t entries,
				       size_t n_sel, const uint64_t *sel, unsigned format, void *d_out,
				       size_t out_avail, size_t out_align, unsigned flags,
				       uint64_t *out_offsets, int32_t *d_results, void *stream)
{
	return pngx_call("png_decode_pixels_batch", d, d_in, in_nbytes, index, entries, n_sel, sel,
			 format, d_out, out_avail, out_align, flags, out_offsets, d_results,
			 PNGX_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 gather, 2 inflate, 4 unfilter, 8 convert), so that
 * tools/bench_png_pixels.py can time the convert stage alone on scratch an
 * earlier full call has filled; d_results then mixes verdicts of both calls */
extern "C" LIBDEFLATEAPI int
lda_png_pixels_stages(struct libdeflate_decompressor *d, const void *d_in, size_t in_nbytes,
		      const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel,
		      unsigned format, void *d_out, size_t out_avail, size_t out_align,
		      unsigned flags, uint64_t *out_offsets, int32_t *d_results, unsigned stages,
		      void *stream)
{
	return pngx_call("png_pixels_stages", d, d_in, in_nbytes, index, entries, n_sel, sel, format,
			 d_out, out_avail, out_align, flags, out_offsets, d_results,
			 stages & PNGX_STAGE_ALL, stream);
}
