/*
 * host_png_pixels.hip - C-ABI of decoding PNG files from device memory to one
 * pixel format (include/libdeflate_amd.h): the decode pipeline of host_png.hip
 * (png_decode_run()) with the plan of png_pixels_plan.h.  The gather and the
 * ONE zlib decompress batch run over all selections, and so does the unfilter,
 * in one launch: a selection that already is the format is written into its
 * room of d_out, the others into the scratch (the kernel's second base,
 * LDA_PNG_META_ALT).  Then the convert kernel writes the rooms of the second
 * kind (png_pixels_kernels.hip), and the verdicts are merged.  A batch that is
 * direct throughout uploads and launches what libdeflate_amd_png_decode_batch
 * does, and one memset and a verdict kernel of one more input.  Nothing waits
 * for the device and nothing is read back.
 */
#include <string>
#include <vector>

#include "host_png.h"
#include "png_pixels_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNG_GRAY == PNGX_GRAY && LIBDEFLATE_AMD_PNG_GRAY_ALPHA == PNGX_GRAY_ALPHA &&
	      LIBDEFLATE_AMD_PNG_RGB == PNGX_RGB && LIBDEFLATE_AMD_PNG_RGBA == PNGX_RGBA &&
	      LIBDEFLATE_AMD_PNG_OUT16 == PNGX_OUT16 && LDA_PNGX_OUT16 == PNGX_OUT16 &&
	      LDA_PNGX_TILE == PNGX_TILE && LDA_PNGX_KIND_KEY == PNGX_KIND_KEY &&
	      LDA_PNG_META_ALT == PNGX_META_ALT,
	      "png_pixels_plan.h and kernels.h hold copies of the header's constants");

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_pixels_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
				    const uint64_t *sel, unsigned format, size_t out_align,
				    uint64_t *out_offsets, uint64_t *total_ret)
{
	const char *what = "png_pixels_out_sizes";
	if (!out_offsets) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!read_sel_args_ok(what, index, entries, n_sel, sel) || !read_align_ok(what, out_align))
		return LIBDEFLATE_AMD_BAD_ARG;
	return read_plan_call(what, [&](std::string &err) {
		return png_pixels_plan_out_sizes(index, entries, n_sel, sel, format, out_align - 1,
						 out_offsets, total_ret, err);
	});
}

/* png_pixels_plan.h's plan: the selections are the images, the direct ones
 * unfiltered into d_out and the others into the scratch, where the convert
 * reads them */
static void pngx_run(const PngxPlan &plan, size_t n_sel, unsigned format, unsigned flags, PngRun &r)
{
	r.scratch = plan.scratch;
	r.n_unf = r.n_verd = n_sel;
	r.unf_at = PNG_COL_RAW_OFF * n_sel;
	r.alt = true;
	r.n_conv = (size_t)plan.n_conv;
	r.conv_at = (size_t)plan.conv_at;
	r.conv_tiles = plan.tiles;
	r.format = format;
	r.le16 = flags & PNG_LE16;
	r.final = PNG_FINAL_PIXELS;
}

static int pngx_call(const char *what, struct libdeflate_decompressor *d, const void *d_in,
		     size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
		     const uint64_t *sel, unsigned format, void *d_out, size_t out_avail,
		     size_t out_align, unsigned flags, uint64_t *out_offsets, int32_t *d_results,
		     unsigned stages, void *stream)
{
	if (!png_decode_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
				out_align, flags, LIBDEFLATE_AMD_PNG_LE16, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	return read_call<PngRun>(what, d, n_sel, [&](PngRun &r, std::string &err) {
		PngxPlan plan;
		if (!png_pixels_plan(index, entries, n_sel, sel, format, in_nbytes, out_avail,
				     out_align - 1, flags, r.cols, out_offsets, &plan, err))
			return false;
		pngx_run(plan, n_sel, format, flags, r);
		return true;
	}, [&](const PngRun &r) {
		return png_decode_run(d, (const uint8_t *)d_in, n_sel, r, (uint8_t *)d_out, d_results,
				      stages, (hipStream_t)stream);
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
			 PNG_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 gather, 2 inflate, 4 unfilter, 8 convert - the pipeline's bit for
 * the convert lies one higher), so that tools/bench_png_pixels.py can time the
 * convert stage alone on scratch an earlier full call has filled; d_results
 * then mixes verdicts of both calls */
extern "C" LIBDEFLATEAPI int
lda_png_pixels_stages(struct libdeflate_decompressor *d, const void *d_in, size_t in_nbytes,
		      const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel,
		      unsigned format, void *d_out, size_t out_avail, size_t out_align,
		      unsigned flags, uint64_t *out_offsets, int32_t *d_results, unsigned stages,
		      void *stream)
{
	return pngx_call("png_pixels_stages", d, d_in, in_nbytes, index, entries, n_sel, sel, format,
			 d_out, out_avail, out_align, flags, out_offsets, d_results,
			 (stages & 7) | (stages & 8 ? PNG_STAGE_CONVERT : 0), stream);
}
