/*
 * host_png.hip - C-ABI of reading PNG files from device memory
 * (include/libdeflate_amd.h).
 *
 * The index call is one kernel, a lane per file (png_kernels.hip).  A decode
 * takes the index rows and the selection from the host: png_plan.h checks them
 * and gives every selection its room in the output and in two scratch areas of
 * the object, and the descriptor columns go up in one copy.  Then four steps
 * are queued: the IDAT payloads of every selection gathered into its zlib
 * stream, ONE zlib decompress batch of n_sel chunks over those streams (exact
 * fill of height * (1 + rowbytes) bytes, the wave-per-stream kernel as every
 * other caller launches it), the scanline filters undone into d_out, and the
 * three verdicts merged into d_results.  Nothing waits for the device and
 * nothing is read back; every size and launch shape is the plan's.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_zip_args.h"
#include "png_plan.h"

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

/* the stages of a decode; the benchmark times each alone (lda_png_decode_stages) */
enum { PNG_STAGE_GATHER = 1, PNG_STAGE_INFLATE = 2, PNG_STAGE_UNFILTER = 4, PNG_STAGE_ALL = 7 };

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

static bool png_sel_args_ok(const char *what, const uint64_t *index, size_t entries, size_t n_sel,
			    const uint64_t *sel)
{
	if ((!index && entries) || (n_sel && !sel)) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (entries > LDA_FINDER_MAX_RECORDS || n_sel > LDA_FINDER_MAX_RECORDS) {
		set_error("%s: entries %zu, n_sel %zu (at most 2^28)", what, entries, n_sel);
		return false;
	}
	return true;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
			     const uint64_t *sel, size_t out_align, uint64_t *out_offsets,
			     uint64_t *total_ret)
{
	const char *what = "png_out_sizes";
	if (!png_sel_args_ok(what, index, entries, n_sel, sel))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!out_offsets) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!zip_align_ok(what, out_align))
		return LIBDEFLATE_AMD_BAD_ARG;
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!png_plan_out_sizes(index, entries, n_sel, sel, out_align - 1, out_offsets,
					total_ret, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		return LIBDEFLATE_AMD_OK;
	});
}

/* the waves of the unfilter, four to a workgroup: sixteen workgroups fill a
 * CU's wave slots, and the grid strides over what is beyond */
static unsigned unfilter_grid(const DeviceCtx *ctx, size_t n_sel)
{
	return (unsigned)std::max((size_t)1, std::min((n_sel + 3) / 4, (size_t)ctx->num_cus * 16));
}

static int png_decode(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		      const std::vector<uint64_t> &cols, uint64_t scratch, uint8_t *d_out,
		      int32_t *d_results, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	/* device: [the two areas][the plan's columns][gather, decode, unfilter verdicts] */
	uint8_t *g_area = NULL;
	uint64_t *g_cols = NULL;
	int32_t *g_gather = NULL, *g_decode = NULL, *g_unf = NULL;
	size_t up_bytes = 0;
	auto lay = [&](Carve *cv) {
		g_area = cv->take<uint8_t>(scratch + 16);
		g_cols = cv->take<uint64_t>(PNG_COLS * n_sel);
		up_bytes = PNG_COLS * n_sel * sizeof(uint64_t);
		g_gather = cv->take<int32_t>(n_sel);
		g_decode = cv->take<int32_t>(n_sel);
		g_unf = cv->take<int32_t>(n_sel);
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
	const uint64_t *col[PNG_COLS];
	for (size_t a = 0; a < PNG_COLS; a++)
		col[a] = g_cols + a * n_sel;
	/* (a NULL d_out has out_avail 0: every selection is a zero row, nothing is
	 * written and nothing is read) */
	uint8_t *out = d_out ? d_out : ws;

	if (stages & PNG_STAGE_GATHER) {
		hipLaunchKernelGGL(lda_png_gather_kernel, dim3(zip_copy_grid(ctx, n_sel)), dim3(256), 0,
				   st, (uint64_t)n_sel, col[PNG_COL_IDAT], col[PNG_COL_END],
				   col[PNG_COL_ZSUM], col[PNG_COL_Z_OFF], d_in, g_area, g_gather);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	if (stages & PNG_STAGE_INFLATE) {
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_ZLIB, n_sel, g_area,
						     col[PNG_COL_Z_OFF], col[PNG_COL_ZSUM], g_area,
						     col[PNG_COL_RAW_OFF], col[PNG_COL_RAW_N], g_decode,
						     NULL, NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (stages & PNG_STAGE_UNFILTER) {
		hipLaunchKernelGGL(lda_png_unfilter_kernel, dim3(unfilter_grid(ctx, n_sel)), dim3(256),
				   0, st, (uint64_t)n_sel, col[PNG_COL_RAW_OFF], col[PNG_COL_RAW_N],
				   col[PNG_COL_OUT_OFF], col[PNG_COL_GEOM], col[PNG_COL_META],
				   (const uint8_t *)g_area, out, out, g_unf);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_png_final_kernel, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0,
			   st, (uint64_t)n_sel, col[PNG_COL_META], (const int32_t *)g_gather,
			   (const int32_t *)g_decode, (const int32_t *)g_unf, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int png_decode_call(const char *what, struct libdeflate_decompressor *d, const void *d_in,
			   size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			   const uint64_t *sel, void *d_out, size_t out_avail, size_t out_align,
			   unsigned flags, uint64_t *out_offsets, int32_t *d_results,
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
		uint64_t scratch = 0;
		if (!png_plan_decode(index, entries, n_sel, sel, in_nbytes, out_avail, out_align - 1,
				     flags, cols, out_offsets, &scratch, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_sel == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return png_decode(d, (const uint8_t *)d_in, n_sel, cols, scratch, (uint8_t *)d_out,
				  d_results, stages, (hipStream_t)stream);
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
			       stages & PNG_STAGE_ALL, stream);
}
