/*
 * png_plan.h - the host arithmetic of the PNG reader (host_png.hip): what an
 * IHDR means (bytes per row, the filter unit, the channels), the index rows of
 * a selection checked against the input, and from them every selection's room
 * in the three areas - the zlib stream gathered out of the IDAT chunks, the
 * raw scanlines height * (1 + rowbytes), the output height * rowbytes - and
 * the descriptor columns of the kernels.  Free of HIP:
 * tools/test_png_plan.cpp runs it on the CPU.
 *
 * A row is what libdeflate_amd_png_index_batch wrote (include/libdeflate_amd.h):
 * { file offset, file nbytes, width | height << 32,
 *   depth | colour << 8 | interlace << 16 | bpp << 24 | channels << 32,
 *   first IDAT, sum of the IDAT lengths, PLTE offset | entries << 48,
 *   tRNS offset | length << 48 }; words 2 .. 7 are zero for a refused file.
 */
#ifndef LDA_PNG_PLAN_H
#define LDA_PNG_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace lda {

enum {
	PNG_ROW_WORDS = 8,
	PNG_BAD_DATA = 1,	/* LIBDEFLATE_BAD_DATA */
	PNG_UNSUPPORTED = 18,	/* LIBDEFLATE_AMD_PNG_UNSUPPORTED */
	PNG_LE16 = 1,		/* LIBDEFLATE_AMD_PNG_LE16 */
	PNG_FIRST_CHUNK = 33,	/* the signature and the IHDR chunk */
	PNG_ROOM_ALIGN = 16,	/* the rooms of the two scratch areas start on it */
	/* the columns of a plan, n_sel words each, in the order they go up */
	PNG_COL_IDAT = 0,	/* first IDAT's length field, offset in d_in */
	PNG_COL_END,		/* where the file ends in d_in */
	PNG_COL_ZSUM,		/* bytes of the zlib stream (0: nothing to do) */
	PNG_COL_Z_OFF,		/* its room, offset in the scratch */
	PNG_COL_RAW_OFF,	/* the raw scanlines' room, offset in the scratch */
	PNG_COL_RAW_N,		/* height * (1 + rowbytes) */
	PNG_COL_OUT_OFF,	/* the pixels, offset in d_out */
	PNG_COL_GEOM,		/* height | rowbytes << 32 */
	PNG_COL_META,		/* bpp | flags << 8 | the row's own result << 16 */
	PNG_COLS
};

static const uint64_t PNG_MAX_DIM = 0x7FFFFFFFull;
static const uint64_t PNG_MAX_SCRATCH = (uint64_t)1 << 48;

/* channels of a colour type, 0 for a type there is not */
static inline unsigned png_channels(unsigned colour)
{
	switch (colour) {
	case 0: return 1;
	case 2: return 3;
	case 3: return 1;
	case 4: return 2;
	case 6: return 4;
	}
	return 0;
}

/* the table of the specification (PNG 11.2.2) */
static inline bool png_depth_ok(unsigned depth, unsigned colour)
{
	switch (colour) {
	case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
	case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
	case 2: case 4: case 6: return depth == 8 || depth == 16;
	}
	return false;
}

/* the filter unit: bytes per complete pixel, 1 below 8 bits */
static inline unsigned png_bpp(unsigned depth, unsigned colour)
{
	const unsigned bits = png_channels(colour) * depth;
	return bits < 8 ? 1 : bits / 8;
}

/* bytes of a scanline without its filter byte; width <= 2^31 - 1, so below 2^34 */
static inline uint64_t png_rowbytes(uint64_t width, unsigned depth, unsigned colour)
{
	return (width * png_channels(colour) * depth + 7) / 8;
}

/* height * (1 + rowbytes) is 2^32 or more: such an image is not decoded */
static inline bool png_too_large(uint64_t height, uint64_t rowbytes)
{
	return rowbytes + 1 > 0xFFFFFFFFull / height;	/* (both below 2^35) */
}

struct PngShape {
	uint64_t width, height, rowbytes;
	unsigned depth, colour, bpp, channels;
};

static inline bool png_row_is_zero(const uint64_t *row)
{
	return !(row[2] | row[3] | row[4] | row[5] | row[6] | row[7]);
}

/* NULL, or why words 2 and 3 are not those of an image this reader decodes */
static inline const char *png_row_shape(const uint64_t *row, PngShape *s)
{
	s->width = row[2] & 0xFFFFFFFFull;
	s->height = row[2] >> 32;
	s->depth = (unsigned)(row[3] & 0xFF);
	s->colour = (unsigned)(row[3] >> 8 & 0xFF);
	s->bpp = (unsigned)(row[3] >> 24 & 0xFF);
	s->channels = (unsigned)(row[3] >> 32);
	if (!s->width || !s->height || s->width > PNG_MAX_DIM || s->height > PNG_MAX_DIM)
		return "its width or height is 0 or above 2^31 - 1";
	if (!png_depth_ok(s->depth, s->colour))
		return "its bit depth and colour type are no pair of the specification";
	if ((row[3] >> 16 & 0xFF) != 0)
		return "it is interlaced";
	if (s->bpp != png_bpp(s->depth, s->colour) || row[3] >> 32 != png_channels(s->colour))
		return "its filter unit or channel count is not the IHDR's";
	s->rowbytes = png_rowbytes(s->width, s->depth, s->colour);
	if (png_too_large(s->height, s->rowbytes))
		return "an image of 2^32 raw bytes or more";
	return NULL;
}

/* NULL, or why the row cannot be one of a file inside in_nbytes bytes */
static inline const char *png_row_check(const uint64_t *row, uint64_t in_nbytes, PngShape *s)
{
	if (row[0] > in_nbytes || row[1] > in_nbytes - row[0])
		return "its file does not lie inside in_nbytes";
	const char *why = png_row_shape(row, s);
	if (why)
		return why;
	const uint64_t lo = row[0] + PNG_FIRST_CHUNK, end = row[0] + row[1];
	if (row[1] < PNG_FIRST_CHUNK + 12 || row[4] < lo || row[4] > end - 12 ||
	    row[5] > end - 12 - row[4])
		return "its IDAT chunks do not lie inside the file";
	const uint64_t mask = ((uint64_t)1 << 48) - 1;
	if (row[6]) {
		const uint64_t off = row[6] & mask, n = row[6] >> 48;
		if (n > 256 || off < lo + 8 || off > end || 3 * n + 4 > end - off)
			return "its PLTE does not lie inside the file";
	} else if (s->colour == 3) {
		return "a palette image without a PLTE";
	}
	if (row[7]) {
		const uint64_t off = row[7] & mask, n = row[7] >> 48;
		if (off < lo + 8 || off > end || n + 4 > end - off)
			return "its tRNS does not lie inside the file";
	}
	return NULL;
}

static inline bool png_sel_ok(uint64_t entries, const uint64_t *sel, uint64_t r, std::string &err)
{
	char msg[160];

	if (sel[r] < entries)
		return true;
	snprintf(msg, sizeof(msg), "sel[%llu] = %llu of %llu entries", (unsigned long long)r,
		 (unsigned long long)sel[r], (unsigned long long)entries);
	err = msg;
	return false;
}

static inline void png_row_error(uint64_t k, const char *why, std::string &err)
{
	char msg[160];

	snprintf(msg, sizeof(msg), "row %llu: %s", (unsigned long long)k, why);
	err = msg;
}

/*
 * out_offsets: n_sel + 1 words, where selection r starts and where the last
 * one ends: every image takes height * rowbytes bytes rounded up to the
 * alignment, a zero row takes none.  false with a reason in err: a sel at or
 * above entries, words 2 and 3 that are no image.  align_mask: out_align - 1.
 */
static inline bool
png_plan_out_sizes(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		   uint64_t align_mask, uint64_t *out_offsets, uint64_t *total_ret,
		   std::string &err)
{
	uint64_t at = 0;

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
		/* below 2^32 each and n_sel at most 2^28: no overflow */
		at += (s.height * s.rowbytes + align_mask) & ~align_mask;
	}
	out_offsets[n_sel] = at;
	if (total_ret)
		*total_ret = at;
	return true;
}

/*
 * cols: PNG_COLS columns of n_sel words; out_offsets: NULL or n_sel + 1 words;
 * *scratch_ret: the bytes of the two scratch areas together, the streams' rooms
 * first, the raw scanlines' behind them, every room on PNG_ROOM_ALIGN.  false
 * with a reason in err: a sel at or above entries, a row that fails
 * png_row_check(), a selection that needs more than out_avail (or more scratch
 * than 2^48 bytes).
 */
static inline bool
png_plan_decode(const uint64_t *index, uint64_t entries, uint64_t n_sel, const uint64_t *sel,
		uint64_t in_nbytes, uint64_t out_avail, uint64_t align_mask, unsigned flags,
		std::vector<uint64_t> &cols, uint64_t *out_offsets, uint64_t *scratch_ret,
		std::string &err)
{
	const uint64_t ra = PNG_ROOM_ALIGN - 1;
	uint64_t at = 0, z_at = 0, raw_at = 0;

	cols.assign((size_t)(PNG_COLS * n_sel), 0);
	for (uint64_t r = 0; r < n_sel; r++) {
		if (!png_sel_ok(entries, sel, r, err))
			return false;
		const uint64_t *row = index + PNG_ROW_WORDS * sel[r];
		if (out_offsets)
			out_offsets[r] = at;
		cols[PNG_COL_OUT_OFF * n_sel + r] = at;
		if (png_row_is_zero(row)) {
			cols[PNG_COL_META * n_sel + r] = (uint64_t)PNG_UNSUPPORTED << 16;
			continue;
		}
		PngShape s;
		const char *why = png_row_check(row, in_nbytes, &s);
		if (why) {
			png_row_error(sel[r], why, err);
			return false;
		}
		const uint64_t pixels = s.height * s.rowbytes;
		const uint64_t room = (pixels + align_mask) & ~align_mask;
		if (at > out_avail || room > out_avail - at) {
			err = "the selection needs more than out_avail";
			return false;
		}
		cols[PNG_COL_IDAT * n_sel + r] = row[4];
		cols[PNG_COL_END * n_sel + r] = row[0] + row[1];
		cols[PNG_COL_ZSUM * n_sel + r] = row[5];
		cols[PNG_COL_Z_OFF * n_sel + r] = z_at;
		cols[PNG_COL_RAW_OFF * n_sel + r] = raw_at;	/* (the areas' order: below) */
		cols[PNG_COL_RAW_N * n_sel + r] = pixels + s.height;
		cols[PNG_COL_GEOM * n_sel + r] = s.height | s.rowbytes << 32;
		cols[PNG_COL_META * n_sel + r] =
			s.bpp | (uint64_t)((flags & PNG_LE16) && s.depth == 16) << 8;
		at += room;
		z_at += (row[5] + ra) & ~ra;
		raw_at += (pixels + s.height + ra) & ~ra;
		if (z_at > PNG_MAX_SCRATCH || raw_at > PNG_MAX_SCRATCH) {
			err = "the selection needs more than 2^48 bytes of scratch";
			return false;
		}
	}
	/* the raw area lies behind the streams' */
	for (uint64_t r = 0; r < n_sel; r++)
		if (cols[PNG_COL_RAW_N * n_sel + r])
			cols[PNG_COL_RAW_OFF * n_sel + r] += z_at;
	if (out_offsets)
		out_offsets[n_sel] = at;
	if (scratch_ret)
		*scratch_ret = z_at + raw_at;
	return true;
}

} /* namespace lda */

#endif /* LDA_PNG_PLAN_H */
