/*
 * host_png_adam7.hip - C-ABI of the PNG reader's calls that take
 * Adam7-interlaced files (include/libdeflate_amd.h): the index call with a
 * flags argument, and one decode call for both output layouts - format 0 is
 * libdeflate_amd_png_decode_batch's, any other that of
 * libdeflate_amd_png_decode_pixels_batch.
 *
 * A selection without an interlaced row is handed to those two calls as it
 * is: it queues what they queue and writes what they write.  With one, the
 * plan of png_adam7_plan.h goes through the decode pipeline of host_png.hip
 * (png_decode_run()), with two changes from the sibling calls' plans: the
 * unfilter runs once over the plan's units - a plain selection is one, an interlaced one is one per
 * present pass, an ordinary filtered image each, written into a pass-image room
 * of the scratch - and behind it the deinterlace kernel weaves the pass images
 * of every interlaced selection into its room of d_out, or into the convert
 * scratch where the convert kernel follows.  The gather and the ONE zlib
 * decompress batch run over the selections as before (exact fill of raw7 bytes
 * for an interlaced one), and a verdict kernel merges per selection, over its
 * units.  Nothing waits for the device and nothing is read back.
 */
#include <string>
#include <vector>

#include "host_png.h"
#include "png_adam7_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNG_ADAM7 == PNG_ADAM7 && LDA_PNG_ADAM7 == PNG_ADAM7 &&
	      LDA_PNG7_TILE == PNG7_TILE && LDA_PNG7_KIND_ALT == PNG7_KIND_ALT &&
	      LDA_PNG_META_ALT == PNGX_META_ALT && LDA_PNG_META_LE16 == PNG_LE16 << 8,
	      "png_adam7_plan.h and kernels.h hold copies of the header's constants");

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
	if (!out_offsets) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!read_sel_args_ok(what, index, entries, n_sel, sel) || !read_align_ok(what, out_align))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (flags & ~(unsigned)LIBDEFLATE_AMD_PNG_ADAM7) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return read_plan_call(what, [&](std::string &err) {
		return png7_plan_out_sizes(index, entries, n_sel, sel, format, out_align - 1, flags,
					   out_offsets, total_ret, err);
	});
}

/* png_adam7_plan.h's plan: the units are the images, all unfiltered into the
 * scratch or d_out as their META says; the deinterlace and the convert follow
 * where the plan has rows for them */
static void png7_run(const Png7Plan &plan, unsigned format, unsigned flags, PngRun &r)
{
	r.scratch = plan.scratch;
	r.n_unf = (size_t)plan.n_units;
	r.unf_at = (size_t)plan.units_at;
	r.n_verd = r.n_unf + 1;
	r.alt = true;
	r.n_il = (size_t)plan.n_il;
	r.il_at = (size_t)plan.il_at;
	r.il_tiles = plan.il_tiles;
	r.n_conv = (size_t)plan.n_conv;
	r.conv_at = (size_t)plan.conv_at;
	r.conv_tiles = plan.conv_tiles;
	r.format = format;
	r.le16 = flags & PNG_LE16;
	r.final = PNG_FINAL_ADAM7;
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
	if (!png_decode_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
				out_align, flags, LIBDEFLATE_AMD_PNG_LE16 | LIBDEFLATE_AMD_PNG_ADAM7,
				d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
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
	return read_call<PngRun>(what, d, n_sel, [&](PngRun &r, std::string &err) {
		Png7Plan plan;
		if (!png7_plan(index, entries, n_sel, sel, format, in_nbytes, out_avail, out_align - 1,
			       flags, r.cols, out_offsets, &plan, err))
			return false;
		png7_run(plan, format, flags, r);
		return true;
	}, [&](const PngRun &r) {
		return png_decode_run(d, (const uint8_t *)d_in, n_sel, r, (uint8_t *)d_out, d_results,
				      stages, (hipStream_t)stream);
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
			 d_out, out_avail, out_align, flags, out_offsets, d_results, PNG_STAGE_ALL,
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
			 stages & PNG_STAGE_ALL, false, stream);
}
