/*
 * png_pixels_plan.h - the host arithmetic of the PNG reader's decode to one
 * pixel format (host_png_pixels.hip), on top of png_plan.h: the rows are
 * checked by png_row_check() and the first PNG_COLS columns are those of
 * png_plan_decode(), so the gather, the zlib batch and the unfilter run as they
 * do there.  What is added: the format, every selection's room of height *
 * width * channels * (1 or 2) bytes, the sorting of the selections into two
 * kinds, and the columns of the convert kernel.
 *
 *   direct:    the file already stores the format - colour type 0, 2, 4 or 6,
 *              its depth the output's, its channels the format's (a tRNS
 *              changes nothing: with equal channels the format has no alpha
 *              to put it in).  The unfilter writes the room in d_out.
 *   converted: everything else.  The unfilter writes height * rowbytes bytes
 *              in PNG order into a third scratch area behind the streams' and
 *              the raw scanlines', and the convert kernel writes the room.
 *
 * The unfilter runs once over all selections: PNG_COL_OUT_OFF is the offset in
 * d_out for a direct selection and in the scratch for a converted one, whose
 * PNG_COL_META has PNGX_META_ALT, the bit that makes the kernel count from its
 * second base.
 *
 * The columns, in the order they go up: png_plan.h's PNG_COLS of n_sel words,
 * then the convert kernel's PNGX_CCOLS of n_conv words, one per converted
 * selection - a batch that is direct throughout uploads what
 * png_plan_decode() uploads.
 * Free of HIP: tools/test_png_pixels_plan.cpp runs it on the CPU.
 */
#ifndef LDA_PNG_PIXELS_PLAN_H
#define LDA_PNG_PIXELS_PLAN_H

#include <algorithm>

#include "png_plan.h"

namespace lda {

enum {
	PNGX_GRAY = 1,		/* LIBDEFLATE_AMD_PNG_GRAY .. _RGBA: the channels */
	PNGX_GRAY_ALPHA = 2,
	PNGX_RGB = 3,
	PNGX_RGBA = 4,
	PNGX_OUT16 = 0x10,	/* LIBDEFLATE_AMD_PNG_OUT16 */
	PNGX_TILE = 4096,	/* pixels of a tile of the convert kernel */
	PNGX_KIND_KEY = 0x10000,	/* kind: the tRNS is a colour key */
	PNGX_META_ALT = 0x200,	/* PNG_COL_META: the unfilter writes into the scratch */
	/* the columns of the converted selections, n_conv words each */
	PNGX_C_SEL = 0,		/* which selection */
	PNGX_C_DST,		/* the room, offset in d_out */
	PNGX_C_SHAPE,		/* width | height << 32 */
	PNGX_C_KIND,		/* depth | colour << 8 | PNGX_KIND_KEY | alphas of the palette << 32 */
	PNGX_C_PLTE,		/* the row's word 6 for colour type 3, else 0 */
	PNGX_C_TRNS,		/* the row's word 7 where the kernel reads it, else 0 */
	PNGX_C_TILE_END,	/* tiles of the converted selections up to and with this one */
	PNGX_CCOLS
};

/* what a plan found, and where its parts lie in cols */
struct PngxPlan {
	uint64_t scratch;	/* bytes of the three scratch areas together */
	uint64_t tiles;		/* tiles of the convert kernel */
	uint64_t n_conv;	/* converted selections */
	uint64_t conv_at;	/* first word of the PNGX_C_* columns */
};

/* false: the low four bits are not 1 .. 4, or other bits than OUT16 are set */
static inline bool pngx_format_ok(unsigned format)
{
	const unsigned ch = format & 0xF;
	return ch >= 1 && ch <= 4 && !(format & ~(0xFu | PNGX_OUT16));
}

static inline unsigned pngx_channels(unsigned format) { return format & 0xF; }
static inline unsigned pngx_depth(unsigned format) { return format & PNGX_OUT16 ? 16 : 8; }

/* the file already stores the format */
static inline bool pngx_direct(unsigned depth, unsigned colour, unsigned format)
{
	return colour != 3 && depth == pngx_depth(format) &&
	       png_channels(colour) == pngx_channels(format);
}

/* bytes of an image in the format: height * rowbytes < 2^32 and a row byte
 * holds 8 pixels at most, so below 2^35 pixels of 8 bytes at most: no overflow */
static inline uint64_t pngx_out_bytes(const PngShape &s, unsigned format)
{
	return s.height * s.width * pngx_channels(format) * (pngx_depth(format) / 8);
}

/* the tRNS is a colour key (PNG 11.3.2.1): grey with one word, RGB with three */
static inline bool pngx_has_key(const uint64_t *row, unsigned colour)
{
	const uint64_t n = row[7] >> 48;
	return row[7] && ((colour == 0 && n == 2) || (colour == 2 && n == 6));
}

static inline bool pngx_format_error(unsigned format, std::string &err)
{
	char msg[96];

	snprintf(msg, sizeof(msg), "format 0x%x is not 1 .. 4, alone or with OUT16 (0x10)", format);
	err = msg;
	return false;
}

/* at + room, false where that passes 2^64 (2^28 selections of up to 2^38 bytes) */
static inline bool pngx_advance(uint64_t *at, uint64_t room, std::string &err)
{
	if (room > ~(uint64_t)0 - *at) {
		err = "the selection needs more than 2^64 bytes";
		return false;
	}
	*at += room;
	return true;
}

/* png_plan_out_sizes() for the format: every image takes pngx_out_bytes()
 * rounded up to the alignment, a zero row none */
static inline bool
png_pixels_plan_out_sizes(const uint64_t *index, uint64_t entries, uint64_t n_sel,
			  const uint64_t *sel, unsigned format, uint64_t align_mask,
			  uint64_t *out_offsets, uint64_t *total_ret, std::string &err)
{
	uint64_t at = 0;

	if (!pngx_format_ok(format))
		return pngx_format_error(format, err);
	for (uint64_t r = 0; r < n_sel; r++) {
		if (!png_sel_ok(entries, sel, r, err))
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		out_offsets[r] = at;
		if (png_row_is_zero(row))
			continue;
		PngShape s;
		const char *why = png_row_shape(row, &s);
		if (why) {
			png_row_error(sel[r], why, err);
			return false;
		}
		if (!pngx_advance(&at, (pngx_out_bytes(s, format) + align_mask) & ~align_mask, err))
			return false;
	}
	out_offsets[n_sel] = at;
	if (total_ret)
		*total_ret = at;
	return true;
}

/*
 * cols: the columns as laid out above; out_offsets: NULL or n_sel + 1 words;
 * plan->scratch: the bytes of the three scratch areas together - the streams'
 * rooms, the raw scanlines', the converted selections' pixels in PNG order -
 * every room on PNG_ROOM_ALIGN.  false with a reason in err: a format that is
 * none, and what png_plan_decode() refuses.
 */
static inline bool
png_pixels_plan(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		unsigned format, uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask,
		unsigned flags, std::vector<uint64_t> &cols, uint64_t *out_offsets,
		PngxPlan *plan, std::string &err)
{
	const uint64_t ra = PNG_ROOM_ALIGN - 1;
	uint64_t at = 0, z_at = 0, raw_at = 0, pix_at = 0, tiles = 0;
	std::vector<uint64_t> conv;	/* PNGX_CCOLS words per converted selection */

	cols.clear();
	*plan = PngxPlan();
	if (!pngx_format_ok(format))
		return pngx_format_error(format, err);
	cols.assign((size_t)(PNG_COLS * n_sel), 0);
	auto col = [&](unsigned c, uint64_t r) -> uint64_t & { return cols[(size_t)(c * n_sel + r)]; };
	for (uint64_t r = 0; r < n_sel; r++) {
		if (!png_sel_ok(entries, sel, r, err))
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		if (out_offsets)
			out_offsets[r] = at;
		if (png_row_is_zero(row)) {
			col(PNG_COL_OUT_OFF, r) = at;
			col(PNG_COL_META, r) = (uint64_t)PNG_UNSUPPORTED << 16;
			continue;
		}
		PngShape s;
		const char *why = png_row_check(row, in_nbytes, &s);
		if (why) {
			png_row_error(sel[r], why, err);
			return false;
		}
		const uint64_t pixels = s.height * s.rowbytes;
		const uint64_t room = (pngx_out_bytes(s, format) + align_mask) & ~align_mask;
		if (at > out_avail || room > out_avail - at) {
			err = "the selection needs more than out_avail";
			return false;
		}
		col(PNG_COL_IDAT, r) = row[4];
		col(PNG_COL_END, r) = row[0] + row[1];
		col(PNG_COL_ZSUM, r) = row[5];
		col(PNG_COL_Z_OFF, r) = z_at;
		col(PNG_COL_RAW_OFF, r) = raw_at;	/* (the areas' order: below) */
		col(PNG_COL_RAW_N, r) = pixels + s.height;
		col(PNG_COL_GEOM, r) = s.height | s.rowbytes << 32;
		if (pngx_direct(s.depth, s.colour, format)) {
			col(PNG_COL_OUT_OFF, r) = at;
			col(PNG_COL_META, r) =
				s.bpp | (uint64_t)((flags & PNG_LE16) && s.depth == 16) << 8;
		} else {
			const bool key = pngx_has_key(row, s.colour);
			uint64_t alphas = 0;
			if (s.colour == 3 && row[7])
				alphas = std::min(row[7] >> 48, row[6] >> 48);
			col(PNG_COL_OUT_OFF, r) = pix_at;
			col(PNG_COL_META, r) = s.bpp | PNGX_META_ALT;	/* PNG order: the convert kernel swaps */
			pix_at += (pixels + ra) & ~ra;
			tiles += (s.width * s.height + PNGX_TILE - 1) / PNGX_TILE;
			const uint64_t c[PNGX_CCOLS] = {
				r, at, s.width | s.height << 32,
				s.depth | s.colour << 8 | (key ? PNGX_KIND_KEY : 0) | alphas << 32,
				s.colour == 3 ? row[6] : 0, key || alphas ? row[7] : 0, tiles,
			};
			conv.insert(conv.end(), c, c + PNGX_CCOLS);
		}
		at += room;
		z_at += (row[5] + ra) & ~ra;
		raw_at += (pixels + s.height + ra) & ~ra;
		if (z_at > PNG_MAX_SCRATCH || raw_at > PNG_MAX_SCRATCH || pix_at > PNG_MAX_SCRATCH) {
			err = "the selection needs more than 2^48 bytes of scratch";
			return false;
		}
	}
	const uint64_t n_conv = conv.size() / PNGX_CCOLS;
	plan->scratch = z_at + raw_at + pix_at;
	plan->tiles = tiles;
	plan->n_conv = n_conv;
	plan->conv_at = PNG_COLS * n_sel;
	cols.resize((size_t)(plan->conv_at + PNGX_CCOLS * n_conv), 0);
	for (uint64_t c = 0; c < n_conv; c++) {
		for (unsigned a = 0; a < PNGX_CCOLS; a++)
			cols[(size_t)(plan->conv_at + a * n_conv + c)] = conv[PNGX_CCOLS * c + a];
		/* the pixels' area lies behind the streams' and the raw scanlines' */
		cols[(size_t)(PNG_COL_OUT_OFF * n_sel + conv[PNGX_CCOLS * c + PNGX_C_SEL])] +=
			z_at + raw_at;
	}
	/* the raw area lies behind the streams' */
	for (uint64_t r = 0; r < n_sel; r++)
		if (cols[(size_t)(PNG_COL_RAW_N * n_sel + r)])
			cols[(size_t)(PNG_COL_RAW_OFF * n_sel + r)] += z_at;
	if (out_offsets)
		out_offsets[n_sel] = at;
	return true;
}

} /* namespace lda */

#endif /* LDA_PNG_PIXELS_PLAN_H */
