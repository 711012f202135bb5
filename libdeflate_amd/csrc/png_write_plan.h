/*
 * png_write_plan.h - the host arithmetic of libdeflate_amd_png_encode_batch
 * (host_png_write.hip): the refusals, the bound, and the plan over many images
 * - every image's room for its filtered scanlines in the object's scratch,
 * those rooms cut into the pieces the compress, Adler-32 and CRC-32 batches run
 * on (write_pieces_plan.h: zipw_cut_pieces(), store false), the fixed
 * part of every file, the per-image columns the kernels of
 * png_write_kernels.hip read and the filter kernel's work list.  Free of HIP:
 * tools/test_png_write_plan.cpp runs it on the CPU.
 *
 * An image row is the reader's index row (png_plan.h) read the other way:
 * { pixels' offset in d_in, their size, width | height << 32,
 *   depth | colour << 8 (bits 16..23 zero, the rest ignored), -, -,
 *   PLTE data offset | entries << 48, tRNS data offset | length << 48 }.
 */
#ifndef LDA_PNG_WRITE_PLAN_H
#define LDA_PNG_WRITE_PLAN_H

#include "png_plan.h"
#include "write_pieces_plan.h"

namespace lda {

enum {
	PNGW_RESULT_WORDS = 4,		/* LIBDEFLATE_AMD_PNGW_RESULT_WORDS */
	PNGW_FILTER_ADAPTIVE = 5,	/* LIBDEFLATE_AMD_PNG_FILTER_ADAPTIVE */
	PNGW_CHUNK = 12,		/* length, type and CRC-32 of a chunk */
	PNGW_ZLIB_EXTRA = 6,		/* the zlib header and the Adler-32 */
	/* the per-image columns, n words each, in the order they go up */
	PNGW_I_FIRST = 0,	/* first piece */
	PNGW_I_COUNT,		/* pieces */
	PNGW_I_PIX,		/* the pixels, offset in d_in */
	PNGW_I_ROOM,		/* the scanlines' room, offset in the scanline area */
	PNGW_I_SCAN,		/* height * (1 + rowbytes) */
	PNGW_I_GEOM,		/* height | rowbytes << 32 */
	PNGW_I_DIMS,		/* width | height << 32: the index row's word 2 */
	PNGW_I_META,		/* the index row's word 3; PNGW_META_LE16: swap on load */
	PNGW_I_PLTE,		/* the row's word 6 */
	PNGW_I_TRNS,		/* the row's word 7 */
	PNGW_I_HEAD,		/* bytes of the file in front of the IDAT payload */
	PNGW_ICOLS,
	PNGW_WORK_WORDS = 2,	/* a work item: image, first row | rows << 32 */
	PNGW_CLASSES = 3	/* G = 4, 16, 64 */
};
#define PNGW_MAX_IMAGES ((uint64_t)1 << 28)
#define PNGW_META_LE16 ((uint64_t)1 << 40)
#define PNGW_IDAT_MAX 0x7FFFFFFFull	/* what a chunk's length field holds */
#define PNGW_OFF_MASK (((uint64_t)1 << 48) - 1)

/* libdeflate_zlib_compress_bound() */
static inline uint64_t pngw_zlib_bound(uint64_t len)
{
	uint64_t blocks = (len + 4999) / 5000;
	if (blocks < 1)
		blocks = 1;
	return PNGW_ZLIB_EXTRA + 5 * blocks + len;
}

/* the CRC-32 of "IDAT" and the two bytes of the zlib header at a level: the
 * part of every IDAT chunk's CRC that is the same for all images */
static inline uint32_t pngw_idat_head_crc(int level)
{
	const uint32_t hw = lda_zlib_header(level);
	const uint8_t b[6] = { 'I', 'D', 'A', 'T', (uint8_t)(hw >> 8), (uint8_t)hw };
	uint32_t crc = ~(uint32_t)0;

	for (unsigned i = 0; i < 6; i++) {
		crc ^= b[i];
		for (unsigned k = 0; k < 8; k++)
			crc = (crc >> 1) ^ (0xEDB88320u & (0 - (crc & 1)));
	}
	return ~crc;
}

/* the lanes of a row: the smallest of 4, 16, 64 whose 16 bytes each cover it */
static inline unsigned pngw_group_class(uint64_t rowbytes)
{
	return rowbytes <= 64 ? 0 : rowbytes <= 256 ? 1 : 2;
}

static inline unsigned pngw_group_lanes(unsigned cls)
{
	return cls == 0 ? 4 : cls == 1 ? 16 : 64;
}

/* rows of one work item: four passes of a 256-thread workgroup's groups, more
 * where an image has so many rows that it would make above 1024 items */
static inline uint64_t pngw_item_rows(uint64_t height, unsigned cls)
{
	const uint64_t groups = 256 / pngw_group_lanes(cls);
	const uint64_t by_height = ((height + 1023) / 1024 + groups - 1) / groups * groups;
	return by_height > 4 * groups ? by_height : 4 * groups;
}

struct PngwShape {
	PngShape s;
	uint64_t pixels, scan, head, plte_n, trns_n;
};

/* NULL, or why the call refuses the row.  in_avail: ~0 where only the bound is
 * asked for */
static inline const char *
pngw_row_check(const uint64_t *row, uint64_t in_avail, int level, PngwShape *w)
{
	/* the reader's rule on words 2 and 3, with the two fields it derives */
	const unsigned depth = (unsigned)(row[3] & 0xFF), colour = (unsigned)(row[3] >> 8 & 0xFF);
	const uint64_t full[PNG_ROW_WORDS] = {
		0, 0, row[2],
		(row[3] & 0xFFFFFF) | (uint64_t)(png_channels(colour) ? png_bpp(depth, colour) : 0) << 24 |
			(uint64_t)png_channels(colour) << 32,
		0, 0, 0, 0 };
	const char *why = png_row_shape(full, &w->s);
	if (why)
		return why;
	w->pixels = w->s.height * w->s.rowbytes;
	w->scan = w->pixels + w->s.height;
	if (row[1] != w->pixels)
		return "word 1 is not height * rowbytes";
	if (level == 0 && w->scan > 0xFFFFFF00ull)
		return "a level-0 image above 0xFFFFFF00 scanline bytes, which no compress call takes";
	if (pngw_zlib_bound(w->scan) > PNGW_IDAT_MAX)
		return "its zlib bound is above 2^31 - 1, more than one IDAT holds";
	if (row[0] > in_avail || in_avail - row[0] < w->pixels)
		return "its pixels do not lie inside in_avail";
	w->plte_n = w->trns_n = 0;
	if (row[6]) {
		const uint64_t off = row[6] & PNGW_OFF_MASK, e = row[6] >> 48;
		if (colour == 0 || colour == 4)
			return "a PLTE with a grey colour type";
		if (e < 1 || e > 256 || (colour == 3 && e > (uint64_t)1 << depth))
			return "its PLTE has no entry, above 256 or above 1 << depth";
		if (off > in_avail || in_avail - off < 3 * e)
			return "its PLTE does not lie inside in_avail";
		w->plte_n = e;
	} else if (colour == 3) {
		return "a palette image without a PLTE";
	}
	if (row[7]) {
		const uint64_t off = row[7] & PNGW_OFF_MASK, t = row[7] >> 48;
		if (colour == 4 || colour == 6)
			return "a tRNS with an alpha colour type";
		if ((colour == 0 && t != 2) || (colour == 2 && t != 6) ||
		    (colour == 3 && (t < 1 || t > w->plte_n)))
			return "its tRNS length is not 2 (grey), 6 (RGB) or 1 .. PLTE entries";
		if (off > in_avail || in_avail - off < t)
			return "its tRNS does not lie inside in_avail";
		w->trns_n = t;
	}
	w->head = 8 + 25 + (w->plte_n ? PNGW_CHUNK + 3 * w->plte_n : 0) +
		  (w->trns_n ? PNGW_CHUNK + w->trns_n : 0) + 8;
	return NULL;
}

/* the most bytes the image's file can have */
static inline uint64_t pngw_image_bound(const PngwShape &w)
{
	return w.head + pngw_zlib_bound(w.scan) + 4 + PNGW_CHUNK;
}

/* true, or false with the reason in err: what the call refuses before any
 * device work, pointers apart (images is there when n != 0) */
static inline bool
pngw_check(uint64_t n, const uint64_t *images, uint64_t in_avail, unsigned filter, unsigned flags,
	   int level, std::string &err)
{
	char msg[200];

	if (filter > PNGW_FILTER_ADAPTIVE) {
		snprintf(msg, sizeof(msg), "filter %u above 5", filter);
		err = msg;
		return false;
	}
	if (flags & ~(unsigned)PNG_LE16) {
		snprintf(msg, sizeof(msg), "unknown flags 0x%x", flags);
		err = msg;
		return false;
	}
	if (n > PNGW_MAX_IMAGES) {
		snprintf(msg, sizeof(msg), "n_images %llu above 2^28", (unsigned long long)n);
		err = msg;
		return false;
	}
	for (uint64_t k = 0; k < n; k++) {
		PngwShape w;
		const char *why = pngw_row_check(images + PNG_ROW_WORDS * k, in_avail, level, &w);
		if (why) {
			snprintf(msg, sizeof(msg), "image %llu: %s", (unsigned long long)k, why);
			err = msg;
			return false;
		}
	}
	return true;
}

/* the sum of the images' bounds; 0 where a row is one the call refuses (in_avail
 * apart) or n is above 2^28 */
static inline uint64_t pngw_bound(uint64_t n, const uint64_t *images, int level)
{
	uint64_t sum = 0;

	if (n > PNGW_MAX_IMAGES)
		return 0;
	for (uint64_t k = 0; k < n; k++) {
		PngwShape w;
		if (pngw_row_check(images + PNG_ROW_WORDS * k, ~(uint64_t)0, level, &w))
			return 0;
		sum += pngw_image_bound(w);	/* below 2^32 each: no overflow */
	}
	return sum;
}

struct pngw_plan : zipw_pieces {
	uint64_t n, bound, pixels_total, scan_bytes;
	std::vector<uint64_t> icols;	/* PNGW_ICOLS x n */
	std::vector<uint64_t> work;	/* PNGW_WORK_WORDS per item, class by class */
	uint64_t items[PNGW_CLASSES + 1];	/* class c: items [items[c], items[c + 1]) */
};

/* the arguments have passed pngw_check(); pr.store is false whatever the level */
static inline void
pngw_plan_build(const zipw_params &pr, uint64_t n, const uint64_t *images, unsigned flags,
		pngw_plan &p)
{
	const uint64_t ra = PNG_ROOM_ALIGN - 1;
	std::vector<uint64_t> rooms((size_t)n), scans((size_t)n);
	uint64_t at = 0;

	p.n = n;
	p.bound = p.pixels_total = 0;
	p.icols.assign((size_t)(PNGW_ICOLS * n), 0);
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *row = images + PNG_ROW_WORDS * k;
		PngwShape w;
		pngw_row_check(row, ~(uint64_t)0, pr.level, &w);
		rooms[(size_t)k] = at;
		scans[(size_t)k] = w.scan;
		p.icols[PNGW_I_PIX * n + k] = row[0];
		p.icols[PNGW_I_ROOM * n + k] = at;
		p.icols[PNGW_I_SCAN * n + k] = w.scan;
		p.icols[PNGW_I_GEOM * n + k] = w.s.height | w.s.rowbytes << 32;
		p.icols[PNGW_I_DIMS * n + k] = row[2];
		p.icols[PNGW_I_META * n + k] =
			w.s.depth | (uint64_t)w.s.colour << 8 | (uint64_t)w.s.bpp << 24 |
			(uint64_t)w.s.channels << 32 |
			((flags & PNG_LE16) && w.s.depth == 16 ? PNGW_META_LE16 : 0);
		p.icols[PNGW_I_PLTE * n + k] = row[6];
		p.icols[PNGW_I_TRNS * n + k] = row[7];
		p.icols[PNGW_I_HEAD * n + k] = w.head;
		p.bound += pngw_image_bound(w);
		p.pixels_total += w.pixels;
		at += (w.scan + ra) & ~ra;	/* below 2^32 each, n at most 2^28 */
	}
	p.scan_bytes = at;
	/* the work list, class by class, the images in the caller's order */
	p.work.clear();
	for (unsigned c = 0; c < PNGW_CLASSES; c++) {
		p.items[c] = p.work.size() / PNGW_WORK_WORDS;
		for (uint64_t k = 0; k < n; k++) {
			const uint64_t geom = p.icols[PNGW_I_GEOM * n + k];
			const uint64_t height = geom & 0xFFFFFFFFull;
			if (pngw_group_class(geom >> 32) != c)
				continue;
			const uint64_t per = pngw_item_rows(height, c);
			for (uint64_t y = 0; y < height; y += per) {
				p.work.push_back(k);
				p.work.push_back(y | (height - y < per ? height - y : per) << 32);
			}
		}
	}
	p.items[PNGW_CLASSES] = p.work.size() / PNGW_WORK_WORDS;
	zipw_cut_pieces(pr, n, rooms.data(), scans.data(), p.icols.data() + PNGW_I_FIRST * n,
			p.icols.data() + PNGW_I_COUNT * n, p);
}

} /* namespace lda */

#endif /* LDA_PNG_WRITE_PLAN_H */
