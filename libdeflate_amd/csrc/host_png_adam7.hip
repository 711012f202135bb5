/*
 * host_png_adam7.hip - C-ABI of the PNG reader's calls that take
 * Adam7-interlaced files (include/libdeflate_amd.h): the index call with a
 * flags argument, and one decode call for both output layouts - format 0 is
 * libdeflate_amd_png_decode_batch's, any other that of
 * libdeflate_amd_png_decode_pixels_batch.
 *
 * A selection without an interlaced row is handed to those two calls as it
 * is: it queues what they queue and writes what they write.  With one, the
 * plan of png_adam7_plan.h goes up in one copy and the steps of
 * host_png_pixels.hip are queued with two changes: the unfilter runs once over
 * the plan's units - a plain selection is one, an interlaced one is one per
 * present pass, an ordinary filtered image each, written into a pass-image room
 * of the scratch - and behind it the deinterlace kernel weaves the pass images
 * of every interlaced selection into its room of d_out, or into the convert
 * scratch where the convert kernel follows.  The gather and the ONE zlib
 * decompress batch run over the selections as before (exact fill of raw7 bytes
 * for an interlaced one), and a verdict kernel merges per selection, over its
 * units.  Nothing waits for the device and nothing is read back.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_zip_args.h"
#include "png_adam7_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNG_ADAM7 == PNG_ADAM7 && LDA_PNG_ADAM7 == PNG_ADAM7 &&
	      LDA_PNG7_TILE == PNG7_TILE && LDA_PNG7_KIND_ALT == PNG7_KIND_ALT &&
	      LDA_PNG_META_ALT == PNGX_META_ALT && LDA_PNG_META_LE16 == PNG_LE16 << 8,
	      "png_adam7_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a decode; the benchmark times each alone (lda_png_adam7_stages) */
enum {
	PNG7_STAGE_GATHER = 1, PNG7_STAGE_INFLATE = 2, PNG7_STAGE_UNFILTER = 4,
	PNG7_STAGE_DEINTERLACE = 8, PNG7_STAGE_CONVERT = 16, PNG7_STAGE_ALL = 31
};

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_index_batch_ex(struct libdeflate_decompressor *d, size_t n_files, const void *d_in,
				  const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
				  unsigned flags, uint64_t *d_index, int32_t *d_results, void *stream)
{
	const char *what = "png_index_batch_ex";
	if (!d || (n_files && (!d_in || !d_in_offsets || !d_in_nbytes || !d_index || !d_results))) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (flags & ~(unsigned)LIBDEFLATE_AMD_PNG_ADAM7) {
		set_error("%s: unknown flags 0x%x", what, flags);
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
			   (hipStream_t)stream, (uint64_t)n_files, (uint32_t)flags, (const uint8_t *)d_in,
			   d_in_offsets, d_in_nbytes, d_index, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_out_sizes_ex(const uint64_t *index, size_t entries, size_t n_sel,
				const uint64_t *sel, unsigned format, size_t out_align, unsigned flags,
				uint64_t *out_offsets, uint64_t *total_ret)
{
	const char *what = "png_out_sizes_ex";
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
	if (flags & ~(unsigned)LIBDEFLATE_AMD_PNG_ADAM7) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!png7_plan_out_sizes(index, entries, n_sel, sel, format, out_align - 1, flags,
					 out_offsets, total_ret, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		return LIBDEFLATE_AMD_OK;
	});
}

/* as host_png.hip's: four waves to a workgroup, sixteen workgroups to a CU */
static unsigned unfilter_grid(const DeviceCtx *ctx, size_t n_units)
{
	return (unsigned)std::max((size_t)1, std::min((n_units + 3) / 4, (size_t)ctx->num_cus * 16));
}

/* the deinterlace and the convert kernel's workgroups stride over the tiles:
 * eight to a CU fill its wave slots */
static unsigned tile_grid(const DeviceCtx *ctx, uint64_t tiles)
{
	return (unsigned)std::min(tiles, (uint64_t)ctx->num_cus * 8);
}

static int png7_decode(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		       const std::vector<uint64_t> &cols, const Png7Plan &plan, unsigned format,
		       unsigned flags, uint8_t *d_out, int32_t *d_results, unsigned stages,
		       hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n_units = (size_t)plan.n_units, n_conv = (size_t)plan.n_conv,
		     n_il = (size_t)plan.n_il;
	/* device: [the four areas][the plan's columns][the verdicts: the gather's,
	 * the decoder's and the convert's per selection, the unfilter's per unit] */
	uint8_t *g_area = NULL;
	uint64_t *g_cols = NULL;
	int32_t *g_gather = NULL, *g_decode = NULL, *g_unf = NULL, *g_conv = NULL;
	const size_t up_words = cols.size(), up_bytes = up_words * sizeof(uint64_t);
	auto lay = [&](Carve *cv) {
		g_area = cv->take<uint8_t>(plan.scratch + 16);
		g_cols = cv->take<uint64_t>(up_words);
		g_gather = cv->take<int32_t>(n_sel);
		g_decode = cv->take<int32_t>(n_sel);
		g_conv = cv->take<int32_t>(n_sel);
		g_unf = cv->take<int32_t>(n_units + 1);
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
	const uint64_t *col[PNG7_SCOLS], *ucol[PNG7_UCOLS], *ccol[PNGX_CCOLS], *dcol[PNG7_DCOLS];
	for (size_t a = 0; a < PNG7_SCOLS; a++)
		col[a] = g_cols + a * n_sel;
	for (size_t a = 0; a < PNG7_UCOLS; a++)
		ucol[a] = g_cols + plan.units_at + a * n_units;
	for (size_t a = 0; a < PNGX_CCOLS; a++)
		ccol[a] = g_cols + plan.conv_at + a * n_conv;
	for (size_t a = 0; a < PNG7_DCOLS; a++)
		dcol[a] = g_cols + plan.il_at + a * n_il;
	/* (a NULL d_out has out_avail 0: every selection is a zero row) */
	uint8_t *out = d_out ? d_out : ws;

	if (stages & PNG7_STAGE_GATHER) {
		hipLaunchKernelGGL(lda_png_gather_kernel, dim3(zip_copy_grid(ctx, n_sel)), dim3(256), 0,
				   st, (uint64_t)n_sel, col[PNG_COL_IDAT], col[PNG_COL_END],
				   col[PNG_COL_ZSUM], col[PNG_COL_Z_OFF], d_in, g_area, g_gather);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (stages & PNG7_STAGE_INFLATE) {
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_ZLIB, n_sel, g_area,
						     col[PNG_COL_Z_OFF], col[PNG_COL_ZSUM], g_area,
						     col[PNG_COL_RAW_OFF], col[PNG_COL_RAW_N], g_decode,
						     NULL, NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (n_units && (stages & PNG7_STAGE_UNFILTER)) {
		/* a unit is an image to the kernel: a plain selection, or one pass */
		hipLaunchKernelGGL(lda_png_unfilter_kernel, dim3(unfilter_grid(ctx, n_units)), dim3(256),
				   0, st, (uint64_t)n_units, ucol[PNG7_U_RAW_OFF], ucol[PNG7_U_RAW_N],
				   ucol[PNG7_U_OUT_OFF], ucol[PNG7_U_GEOM], ucol[PNG7_U_META],
				   (const uint8_t *)g_area, out, g_area, g_unf);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (n_il && (stages & PNG7_STAGE_DEINTERLACE)) {
		hipLaunchKernelGGL(lda_png7_deinterlace_kernel, dim3(tile_grid(ctx, plan.il_tiles)),
				   dim3(256), 0, st, (uint64_t)n_il, plan.il_tiles, dcol[PNG7_D_TILE_END],
				   dcol[PNG7_D_PASS], dcol[PNG7_D_SHAPE], dcol[PNG7_D_KIND],
				   dcol[PNG7_D_DST], g_area, out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	LDA_HIP_TRY(hipMemsetAsync(g_conv, 0, n_sel * sizeof(int32_t), st), LIBDEFLATE_AMD_NO_DEVICE);
	if (n_conv && (stages & PNG7_STAGE_CONVERT)) {
		hipLaunchKernelGGL(lda_pngx_convert_kernel, dim3(tile_grid(ctx, plan.conv_tiles)),
				   dim3(256), 0, st, (uint64_t)n_conv, plan.conv_tiles, (uint32_t)format,
				   (uint32_t)(flags & PNG_LE16), ccol[PNGX_C_TILE_END], ccol[PNGX_C_SEL],
				   col[PNG_COL_OUT_OFF], ccol[PNGX_C_DST], ccol[PNGX_C_SHAPE],
				   ccol[PNGX_C_KIND], ccol[PNGX_C_PLTE], ccol[PNGX_C_TRNS], d_in,
				   (const uint8_t *)g_area, out, g_conv);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_png7_final_kernel, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0,
			   st, (uint64_t)n_sel, col[PNG_COL_META], col[PNG7_COL_UNITS],
			   (const int32_t *)g_gather, (const int32_t *)g_decode, (const int32_t *)g_unf,
			   (const int32_t *)g_conv, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

/* whether a selection the older calls would not refuse for its sel alone has
 * an interlaced row in it (a sel at or above entries: they say so) */
static bool any_interlaced(const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel)
{
	for (size_t r = 0; r < n_sel; r++) {
		if (sel[r] >= entries)
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		if (!png_row_is_zero(row) && png7_row_interlaced(row))
			return true;
	}
	return false;
}

static int png7_call(const char *what, struct libdeflate_decompressor *d, const void *d_in,
		     size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
		     const uint64_t *sel, unsigned format, void *d_out, size_t out_avail,
		     size_t out_align, unsigned flags, uint64_t *out_offsets, int32_t *d_results,
		     unsigned stages, bool hand_on, void *stream)
{
	if (!zip_read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			      out_align, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (flags & ~(unsigned)(LIBDEFLATE_AMD_PNG_LE16 | LIBDEFLATE_AMD_PNG_ADAM7)) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!png7_format_ok(format)) {
		std::string err;
		png7_format_error(format, err);
		set_error("%s: %s", what, err.c_str());
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	/* nothing interlaced: the older call's launches, bytes and verdicts */
	if (hand_on && !any_interlaced(index, entries, n_sel, sel)) {
		const unsigned f = flags & LIBDEFLATE_AMD_PNG_LE16;
		return format == 0 ?
			libdeflate_amd_png_decode_batch(d, d_in, in_nbytes, index, entries, n_sel, sel,
							d_out, out_avail, out_align, f, out_offsets,
							d_results, stream) :
			libdeflate_amd_png_decode_pixels_batch(d, d_in, in_nbytes, index, entries,
							       n_sel, sel, format, d_out, out_avail,
							       out_align, f, out_offsets, d_results,
							       stream);
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::vector<uint64_t> cols;
		std::string err;
		Png7Plan plan;
		if (!png7_plan(index, entries, n_sel, sel, format, in_nbytes, out_avail, out_align - 1,
			       flags, cols, out_offsets, &plan, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_sel == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return png7_decode(d, (const uint8_t *)d_in, n_sel, cols, plan, format, flags,
				   (uint8_t *)d_out, d_results, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_decode_batch_ex(struct libdeflate_decompressor *d, const void *d_in,
				   size_t in_nbytes, const uint64_t *index, size_t entries,
				   size_t n_sel, const uint64_t *sel, unsigned format, void *d_out,
				   size_t out_avail, size_t out_align, unsigned flags,
				   uint64_t *out_offsets, int32_t *d_results, void *stream)
{
	return png7_call("png_decode_batch_ex", d, d_in, in_nbytes, index, entries, n_sel, sel, format,
			 d_out, out_avail, out_align, flags, out_offsets, d_results, PNG7_STAGE_ALL,
			 true, stream);
}

/* not part of the interface: the call's own path, also where nothing is
 * interlaced, with only the stages of `stages` queued (1 gather, 2 inflate, 4
 * unfilter, 8 deinterlace, 16 convert), so that tools/bench_png_adam7.py can
 * time each alone on scratch an earlier full call has filled; d_results then
 * mixes verdicts of both calls */
extern "C" LIBDEFLATEAPI int
lda_png_adam7_stages(struct libdeflate_decompressor *d, const void *d_in, size_t in_nbytes,
		     const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel,
		     unsigned format, void *d_out, size_t out_avail, size_t out_align, unsigned flags,
		     uint64_t *out_offsets, int32_t *d_results, unsigned stages, void *stream)
{
	return png7_call("png_adam7_stages", d, d_in, in_nbytes, index, entries, n_sel, sel, format,
			 d_out, out_avail, out_align, flags, out_offsets, d_results,
			 stages & PNG7_STAGE_ALL, false, stream);
}
