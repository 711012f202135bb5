/*
 * host_png.h - the one decode pipeline of the PNG reader (png_decode_run(),
 * host_png.hip) and what its three callers tell it of their plans: the plain
 * decode (host_png.hip), the decode to one pixel format (host_png_pixels.hip)
 * and the decode that takes Adam7-interlaced files (host_png_adam7.hip).
 */
#ifndef LDA_HOST_PNG_H
#define LDA_HOST_PNG_H

#include <vector>

#include "host_read_plan.h"

namespace lda {

/* the stages of a decode; the lda_png_*_stages hooks translate their own bits */
enum {
	PNG_STAGE_GATHER = 1, PNG_STAGE_INFLATE = 2, PNG_STAGE_UNFILTER = 4,
	PNG_STAGE_DEINTERLACE = 8, PNG_STAGE_CONVERT = 16, PNG_STAGE_ALL = 31
};

/* the kernel that merges the verdicts, and with it which verdicts there are */
enum PngFinal {
	PNG_FINAL_PLAIN,	/* lda_png_final_kernel: no convert verdicts */
	PNG_FINAL_PIXELS,	/* lda_pngx_final_kernel */
	PNG_FINAL_ADAM7		/* lda_png7_final_kernel: the unfilter's verdicts per unit, carved last */
};

/* a plan as png_decode_run() sees it.  `at`s are words into cols; a count of
 * 0 leaves the stage out */
struct PngRun {
	std::vector<uint64_t> cols;	/* what goes up; the selections' columns first */
	uint64_t scratch = 0;	/* bytes of the areas together */
	/* the unfilter: n_unf images, five columns from PNG_COL_RAW_OFF's on, and
	 * n_verd verdicts; alt: its second base is the scratch, not d_out */
	size_t n_unf = 0, unf_at = 0, n_verd = 0;
	bool alt = false;
	/* the deinterlace: PNG7_DCOLS columns */
	size_t n_il = 0, il_at = 0;
	uint64_t il_tiles = 0;
	/* the convert: PNGX_CCOLS columns */
	size_t n_conv = 0, conv_at = 0;
	uint64_t conv_tiles = 0;
	unsigned format = 0, le16 = 0;
	PngFinal final = PNG_FINAL_PLAIN;
};

/* the gather, ONE zlib decompress batch, the unfilter, the deinterlace, the
 * convert - those of `stages` - and the merge of the verdicts into d_results */
int png_decode_run(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		   const PngRun &r, uint8_t *d_out, int32_t *d_results, unsigned stages,
		   hipStream_t st);

/* what the three decode calls refuse before their plans: read_args_ok() and
 * flag bits outside `known` */
bool png_decode_args_ok(const char *what, const struct libdeflate_decompressor *d, const void *d_in,
			size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			const uint64_t *sel, const void *d_out, size_t out_avail, size_t out_align,
			unsigned flags, unsigned known, const int32_t *d_results);

} /* namespace lda */

#endif /* LDA_HOST_PNG_H */
