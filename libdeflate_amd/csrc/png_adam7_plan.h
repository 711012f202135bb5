/*
 * png_adam7_plan.h - the host arithmetic of the PNG reader's calls that take
 * Adam7-interlaced files (host_png_adam7.hip), on top of png_plan.h and
 * png_pixels_plan.h: the geometry of the seven passes, the rows checked with
 * or without the interlace bit, and a plan in which the unfilter's work is no
 * longer the selections but a set of units.
 *
 * An interlaced image's zlib stream holds its passes back to back, every
 * present pass an ordinary filtered image of h_p scanlines of 1 + rb_p bytes:
 * raw7 bytes in all.  A plain selection is one unit, as before.  An interlaced
 * one is one unit per present pass: the unfilter kernel sees an image of h_p
 * rows of rb_p bytes at the pass's offset in the selection's raw room and
 * writes it into a pass-image room of the scratch (PNGX_META_ALT).  The
 * deinterlace kernel then weaves the pass images into the finished image of
 * height rows of rowbytes bytes - in the selection's room of d_out where the
 * file already is what the call returns, or in the convert scratch where a
 * pixel format needs the convert kernel of png_pixels_plan.h, which then runs
 * unchanged.
 *
 * format 0 is libdeflate_amd_png_decode_batch's layout (height * rowbytes,
 * everything direct), any other that of libdeflate_amd_png_decode_pixels_batch.
 *
 * The columns in cols, in the order they go up:
 *   PNG7_SCOLS of n_sel words   png_plan.h's PNG_COLS and PNG7_COL_UNITS
 *   PNG7_UCOLS of n_units words the five the unfilter kernel takes
 *   PNGX_CCOLS of n_conv words  png_pixels_plan.h's, per converted selection
 *   PNG7_DCOLS of n_il words    per interlaced selection, the deinterlace's;
 *                               its seven pass offsets lie together, selection
 *                               by selection, in front of the other columns
 * The scratch: the streams' rooms, the raw scanlines', the pass images', the
 * converted selections' pixels in PNG order, every room on PNG_ROOM_ALIGN.
 * Free of HIP: tools/test_png_adam7_plan.cpp runs it on the CPU.
 */
#ifndef LDA_PNG_ADAM7_PLAN_H
#define LDA_PNG_ADAM7_PLAN_H

#include "png_pixels_plan.h"

namespace lda {

enum {
	PNG_ADAM7 = 2,		/* LIBDEFLATE_AMD_PNG_ADAM7 */
	PNG7_PASSES = 7,
	PNG7_TILE = 1024,	/* 16-byte pieces of a tile of the deinterlace kernel */
	/* the selections' columns: png_plan.h's, and */
	PNG7_COL_UNITS = PNG_COLS,	/* first unit | units << 32 */
	PNG7_SCOLS,
	/* the units' columns */
	PNG7_U_RAW_OFF = 0,	/* the filtered rows, offset in the scratch */
	PNG7_U_RAW_N,		/* rows * (1 + rowbytes) */
	PNG7_U_OUT_OFF,		/* in d_out, or in the scratch with PNGX_META_ALT */
	PNG7_U_GEOM,		/* rows | rowbytes << 32 */
	PNG7_U_META,		/* bpp | PNG_LE16 << 8 | PNGX_META_ALT */
	PNG7_UCOLS,
	/* the interlaced selections' columns */
	PNG7_D_PASS = 0,	/* seven words a selection: the pass images, offsets in the scratch */
	PNG7_D_SHAPE = 7,	/* width | height << 32 */
	PNG7_D_KIND,		/* bits per pixel | PNG7_KIND_ALT | rowbytes << 16 */
	PNG7_D_DST,		/* the finished image: offset in d_out, or in the scratch */
	PNG7_D_TILE_END,	/* tiles of the interlaced selections up to and with this one */
	PNG7_DCOLS,
	PNG7_KIND_ALT = 0x100	/* kind: PNG7_D_DST counts from the scratch */
};

struct Png7Pass {
	uint64_t w, h, rb;	/* pixels a row, rows, bytes a row: all 0 for an absent pass */
};

static const unsigned char PNG7_X0[7] = { 0, 4, 0, 2, 0, 1, 0 };
static const unsigned char PNG7_Y0[7] = { 0, 0, 4, 0, 2, 0, 1 };
static const unsigned char PNG7_DX[7] = { 8, 8, 4, 4, 2, 2, 1 };
static const unsigned char PNG7_DY[7] = { 8, 8, 8, 4, 4, 2, 2 };
static const unsigned char PNG7_LOG_DX[7] = { 3, 3, 2, 2, 1, 1, 0 };	/* (shifts, not divisions: */
static const unsigned char PNG7_LOG_DY[7] = { 3, 3, 3, 2, 2, 1, 1 };	/* a plan has 2^28 rows) */

/* the seven reduced images of a width x height image (PNG 8.2) */
static inline void
png7_passes(uint64_t width, uint64_t height, unsigned depth, unsigned colour, Png7Pass pass[7])
{
	for (unsigned p = 0; p < PNG7_PASSES; p++) {
		const uint64_t w = width > PNG7_X0[p] ?
			(width - PNG7_X0[p] + PNG7_DX[p] - 1) >> PNG7_LOG_DX[p] : 0;
		const uint64_t h = height > PNG7_Y0[p] ?
			(height - PNG7_Y0[p] + PNG7_DY[p] - 1) >> PNG7_LOG_DY[p] : 0;
		if (w && h)
			pass[p] = Png7Pass{ w, h, png_rowbytes(w, depth, colour) };
		else
			pass[p] = Png7Pass{ 0, 0, 0 };
	}
}

/* the bytes the stream inflates to; false where that is 2^32 or more (a pass
 * has fewer than 2^31 rows, so with its row bytes below 2^32 the product stays
 * below 2^63, and seven terms below 2^32 do not pass 2^64 either) */
static inline bool png7_raw_bytes(const Png7Pass pass[7], uint64_t *raw7)
{
	uint64_t sum = 0;

	for (unsigned p = 0; p < PNG7_PASSES; p++) {
		if (!pass[p].h)
			continue;
		if (pass[p].rb > 0xFFFFFFFFull || pass[p].h * (1 + pass[p].rb) > 0xFFFFFFFFull)
			return false;
		sum += pass[p].h * (1 + pass[p].rb);
	}
	*raw7 = sum;
	return sum <= 0xFFFFFFFFull;
}

/* the row with its interlace byte cleared */
static inline void png7_plain_twin(const uint64_t *row, uint64_t *twin)
{
	for (unsigned w = 0; w < PNG_ROW_WORDS; w++)
		twin[w] = row[w];
	twin[3] &= ~((uint64_t)0xFF << 16);
}

static inline bool png7_row_interlaced(const uint64_t *row) { return (row[3] >> 16 & 0xFF) != 0; }

/*
 * png_row_shape() for the calls that take PNG_ADAM7: without the flag, and for
 * a row that is not interlaced, its verdict word for word; with it, interlace
 * 1 is an image of its twin's shape whose raw7 must stay below 2^32 as well.
 */
static inline const char *
png7_row_shape(const uint64_t *row, unsigned flags, PngShape *s, bool *interlaced, Png7Pass pass[7],
	       uint64_t *raw7)
{
	*interlaced = false;
	if (!(flags & PNG_ADAM7) || !png7_row_interlaced(row))
		return png_row_shape(row, s);
	uint64_t twin[PNG_ROW_WORDS];
	png7_plain_twin(row, twin);
	const char *why = png_row_shape(twin, s);
	if (why)
		return why;
	if ((row[3] >> 16 & 0xFF) != 1)
		return "its interlace method is neither 0 nor 1";
	png7_passes(s->width, s->height, s->depth, s->colour, pass);
	if (!png7_raw_bytes(pass, raw7))
		return "an image of 2^32 raw bytes or more";
	*interlaced = true;
	return NULL;
}

/* png_row_check() likewise */
static inline const char *
png7_row_check(const uint64_t *row, uint64_t in_nbytes, unsigned flags, PngShape *s, bool *interlaced,
	       Png7Pass pass[7], uint64_t *raw7)
{
	*interlaced = false;
	if (!(flags & PNG_ADAM7) || !png7_row_interlaced(row))
		return png_row_check(row, in_nbytes, s);
	if (row[0] > in_nbytes || row[1] > in_nbytes - row[0])
		return "its file does not lie inside in_nbytes";
	const char *why = png7_row_shape(row, flags, s, interlaced, pass, raw7);
	if (why)
		return why;
	uint64_t twin[PNG_ROW_WORDS];
	png7_plain_twin(row, twin);
	return png_row_check(twin, in_nbytes, s);
}

static inline bool png7_format_ok(unsigned format) { return format == 0 || pngx_format_ok(format); }

static inline bool png7_format_error(unsigned format, std::string &err)
{
	char msg[112];

	snprintf(msg, sizeof(msg), "format 0x%x is not 0 or 1 .. 4, alone or with OUT16 (0x10)", format);
	err = msg;
	return false;
}

/* the room of an image: format 0 the bytes as PNG stores them */
static inline uint64_t png7_out_bytes(const PngShape &s, unsigned format)
{
	return format ? pngx_out_bytes(s, format) : s.height * s.rowbytes;
}

/* the rooms of png_plan_out_sizes() (format 0) or png_pixels_plan_out_sizes();
 * an interlaced image takes the room of its twin */
static inline bool
png7_plan_out_sizes(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		    unsigned format, uint64_t align_mask, unsigned flags, uint64_t *out_offsets,
		    uint64_t *total_ret, std::string &err)
{
	uint64_t at = 0;

	if (!png7_format_ok(format))
		return png7_format_error(format, err);
	for (uint64_t r = 0; r < n_sel; r++) {
		if (!png_sel_ok(entries, sel, r, err))
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		out_offsets[r] = at;
		if (png_row_is_zero(row))
			continue;
		PngShape s;
		Png7Pass pass[7];
		uint64_t raw7;
		bool il;
		const char *why = png7_row_shape(row, flags, &s, &il, pass, &raw7);
		if (why) {
			png_row_error(sel[r], why, err);
			return false;
		}
		if (!pngx_advance(&at, (png7_out_bytes(s, format) + align_mask) & ~align_mask, err))
			return false;
	}
	out_offsets[n_sel] = at;
	if (total_ret)
		*total_ret = at;
	return true;
}

/* what a plan found, and where its parts lie in cols */
struct Png7Plan {
	uint64_t scratch;	/* bytes of the four scratch areas together */
	uint64_t n_units, units_at;
	uint64_t n_conv, conv_at, conv_tiles;
	uint64_t n_il, il_at, il_tiles;
};

/* the 16-byte pieces of a finished image: every row on its own */
static inline uint64_t png7_pieces(const PngShape &s)
{
	return s.height * ((s.rowbytes + 15) / 16);	/* below 2^32, as height * rowbytes */
}

/* what png7_plan() knows of one selection in both of its passes */
struct Png7Sel {
	PngShape s;
	Png7Pass pass[7];
	uint64_t raw_n, room;
	bool interlaced, direct;
};

/* false with a reason in err: the row is refused, or needs more than out_avail
 * behind the `at` bytes of the selections in front of it */
static inline bool
png7_plan_sel(const uint64_t *row, uint64_t k, unsigned format, uint64_t in_nbytes,
	      uint64_t out_avail, uint64_t align_mask, unsigned flags, uint64_t at, Png7Sel *q,
	      std::string &err)
{
	uint64_t raw7 = 0;
	const char *why = png7_row_check(row, in_nbytes, flags, &q->s, &q->interlaced, q->pass, &raw7);
	if (why) {
		png_row_error(k, why, err);
		return false;
	}
	q->raw_n = q->interlaced ? raw7 : q->s.height * (q->s.rowbytes + 1);
	q->room = (png7_out_bytes(q->s, format) + align_mask) & ~align_mask;
	q->direct = !format || pngx_direct(q->s.depth, q->s.colour, format);
	if (at > out_avail || q->room > out_avail - at) {
		err = "the selection needs more than out_avail";
		return false;
	}
	return true;
}

/*
 * cols: the columns as laid out above; out_offsets: NULL or n_sel + 1 words.
 * false with a reason in err: a format that is none, a sel at or above
 * entries, a row png7_row_check() refuses, a selection that needs more than
 * out_avail or more than 2^48 bytes of scratch.  A first pass over the
 * selections checks them, counts the units and sizes the areas; then every
 * column is written where it goes up from.
 */
static inline bool
png7_plan(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
	  unsigned format, uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask,
	  unsigned flags, std::vector<uint64_t> &cols, uint64_t *out_offsets, Png7Plan *plan,
	  std::string &err)
{
	const uint64_t ra = PNG_ROOM_ALIGN - 1;
	uint64_t at = 0, z_at = 0, raw_at = 0, pass_at = 0, pix_at = 0;
	uint64_t n_units = 0, n_conv = 0, n_il = 0;
	Png7Sel q;

	cols.clear();
	*plan = Png7Plan();
	if (!png7_format_ok(format))
		return png7_format_error(format, err);
	for (uint64_t r = 0; r < n_sel; r++) {
		if (!png_sel_ok(entries, sel, r, err))
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		if (out_offsets)
			out_offsets[r] = at;
		if (png_row_is_zero(row))
			continue;
		if (!png7_plan_sel(row, sel[r], format, in_nbytes, out_avail, align_mask, flags, at, &q, err))
			return false;
		if (q.interlaced) {
			n_il++;
			for (unsigned p = 0; p < PNG7_PASSES; p++) {
				n_units += q.pass[p].h != 0;
				pass_at += (q.pass[p].h * q.pass[p].rb + ra) & ~ra;
			}
		} else {
			n_units++;
		}
		if (!q.direct) {
			n_conv++;
			pix_at += (q.s.height * q.s.rowbytes + ra) & ~ra;
		}
		at += q.room;
		z_at += (row[5] + ra) & ~ra;
		raw_at += (q.raw_n + ra) & ~ra;
		if (z_at > PNG_MAX_SCRATCH || raw_at > PNG_MAX_SCRATCH || pass_at > PNG_MAX_SCRATCH ||
		    pix_at > PNG_MAX_SCRATCH) {
			err = "the selection needs more than 2^48 bytes of scratch";
			return false;
		}
	}
	if (out_offsets)
		out_offsets[n_sel] = at;
	/* the areas one behind the other */
	const uint64_t raw_base = z_at, pass_base = z_at + raw_at, pix_base = pass_base + pass_at;
	plan->scratch = pix_base + pix_at;
	plan->n_units = n_units;
	plan->units_at = PNG7_SCOLS * n_sel;
	plan->n_conv = n_conv;
	plan->conv_at = plan->units_at + PNG7_UCOLS * n_units;
	plan->n_il = n_il;
	plan->il_at = plan->conv_at + PNGX_CCOLS * n_conv;
	cols.assign((size_t)(plan->il_at + PNG7_DCOLS * n_il), 0);

	/* Three sweeps, one per group of columns, so that a sweep writes ten
	 * columns at most side by side and not all 26: the columns of a group lie
	 * n_sel (n_units, ...) words apart, which for a batch of 2^16 images is a
	 * multiple of every cache's way size (on the host this was measured on,
	 * 11.9 ms against 13.7 for 65 536 interlaced selections in one sweep) */
	uint64_t *scol = cols.data(), *ucol = scol + plan->units_at, *ccol = scol + plan->conv_at,
		 *dcol = scol + plan->il_at;
	uint64_t c_tiles = 0, d_tiles = 0;
	enum { SELECTIONS, UNITS, REST, SWEEPS };
	for (int sweep = 0; sweep < SWEEPS; sweep++) {
		uint64_t u = 0, c = 0, i = 0;
		at = z_at = raw_at = pass_at = pix_at = c_tiles = d_tiles = 0;
		auto unit = [&](uint64_t raw, uint64_t raw_n, uint64_t out, uint64_t geom, uint64_t meta) {
			if (sweep == UNITS) {
				ucol[PNG7_U_RAW_OFF * n_units + u] = raw;
				ucol[PNG7_U_RAW_N * n_units + u] = raw_n;
				ucol[PNG7_U_OUT_OFF * n_units + u] = out;
				ucol[PNG7_U_GEOM * n_units + u] = geom;
				ucol[PNG7_U_META * n_units + u] = meta;
			}
			u++;
		};
		for (uint64_t r = 0; r < n_sel; r++) {
			const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
			const uint64_t unit0 = u;
			if (png_row_is_zero(row)) {
				if (sweep == SELECTIONS) {
					scol[PNG7_COL_UNITS * n_sel + r] = unit0;
					scol[PNG_COL_OUT_OFF * n_sel + r] = at;
					scol[PNG_COL_META * n_sel + r] = (uint64_t)PNG_UNSUPPORTED << 16;
				}
				continue;
			}
			(void)png7_plan_sel(row, sel[r], format, in_nbytes, out_avail, align_mask, flags, at, &q,
					    err);
			const PngShape &s = q.s;
			const uint64_t pixels = s.height * s.rowbytes;
			/* the finished image: in d_out, or in the pixels' area for the convert kernel */
			const uint64_t image = q.direct ? at : pix_base + pix_at;
			/* the filters see PNG's byte order; a direct 16-bit image is swapped
			 * where the unfilter wrote it, a converted one by the convert kernel */
			const uint64_t le16 = (uint64_t)(q.direct && (flags & PNG_LE16) && s.depth == 16) << 8;
			const uint64_t meta = s.bpp | le16 | (q.direct ? 0 : PNGX_META_ALT);
			if (!q.interlaced) {
				unit(raw_base + raw_at, q.raw_n, image, s.height | s.rowbytes << 32, meta);
			} else {
				uint64_t in_raw = 0;
				for (unsigned p = 0; p < PNG7_PASSES; p++) {
					const Png7Pass &ps = q.pass[p];
					if (sweep == REST)
						dcol[PNG7_PASSES * i + p] = pass_base + pass_at;
					if (!ps.h)
						continue;
					unit(raw_base + raw_at + in_raw, ps.h * (1 + ps.rb), pass_base + pass_at,
					     ps.h | ps.rb << 32, s.bpp | le16 | PNGX_META_ALT);
					in_raw += ps.h * (1 + ps.rb);
					pass_at += (ps.h * ps.rb + ra) & ~ra;
				}
				d_tiles += (png7_pieces(s) + PNG7_TILE - 1) / PNG7_TILE;
				if (sweep == REST) {
					dcol[PNG7_D_SHAPE * n_il + i] = s.width | s.height << 32;
					dcol[PNG7_D_KIND * n_il + i] = (uint64_t)(s.depth * s.channels) |
								       (q.direct ? 0 : PNG7_KIND_ALT) |
								       s.rowbytes << 16;
					dcol[PNG7_D_DST * n_il + i] = image;
					dcol[PNG7_D_TILE_END * n_il + i] = d_tiles;
				}
				i++;
			}
			if (sweep == SELECTIONS) {
				scol[PNG_COL_IDAT * n_sel + r] = row[4];
				scol[PNG_COL_END * n_sel + r] = row[0] + row[1];
				scol[PNG_COL_ZSUM * n_sel + r] = row[5];
				scol[PNG_COL_Z_OFF * n_sel + r] = z_at;
				scol[PNG_COL_RAW_OFF * n_sel + r] = raw_base + raw_at;
				scol[PNG_COL_RAW_N * n_sel + r] = q.raw_n;
				scol[PNG_COL_OUT_OFF * n_sel + r] = image;
				scol[PNG_COL_GEOM * n_sel + r] = s.height | s.rowbytes << 32;
				scol[PNG_COL_META * n_sel + r] = meta;
				scol[PNG7_COL_UNITS * n_sel + r] = unit0 | (u - unit0) << 32;
			}
			if (!q.direct) {
				c_tiles += (s.width * s.height + PNGX_TILE - 1) / PNGX_TILE;
				if (sweep == REST) {
					const bool key = pngx_has_key(row, s.colour);
					uint64_t alphas = 0;
					if (s.colour == 3 && row[7])
						alphas = std::min(row[7] >> 48, row[6] >> 48);
					ccol[PNGX_C_SEL * n_conv + c] = r;
					ccol[PNGX_C_DST * n_conv + c] = at;
					ccol[PNGX_C_SHAPE * n_conv + c] = s.width | s.height << 32;
					ccol[PNGX_C_KIND * n_conv + c] =
						s.depth | s.colour << 8 | (key ? PNGX_KIND_KEY : 0) | alphas << 32;
					ccol[PNGX_C_PLTE * n_conv + c] = s.colour == 3 ? row[6] : 0;
					ccol[PNGX_C_TRNS * n_conv + c] = key || alphas ? row[7] : 0;
					ccol[PNGX_C_TILE_END * n_conv + c] = c_tiles;
				}
				c++;
				pix_at += (pixels + ra) & ~ra;
			}
			at += q.room;
			z_at += (row[5] + ra) & ~ra;
			raw_at += (q.raw_n + ra) & ~ra;
		}
	}
	plan->conv_tiles = c_tiles;
	plan->il_tiles = d_tiles;
	return true;
}

} /* namespace lda */

#endif /* LDA_PNG_ADAM7_PLAN_H */
