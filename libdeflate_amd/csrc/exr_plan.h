/*
 * exr_plan.h - the host arithmetic of OpenEXR's ZIP and ZIPS chunks, scanline
 * blocks and tiles (include/libdeflate_amd.h: libdeflate_amd_exr_decode_batch,
 * host_exr.hip, and libdeflate_amd_exr_encode_batch, host_exr_write.hip): the
 * refusals made before any device work, the bound, and the two plans.  Free of
 * HIP: tools/test_exr_plan.cpp runs it on the CPU.
 *
 * A chunk holds `lines` lines of `width` pixels channel-planar: for every line
 * in turn, for every channel in the file's order, the line's samples of that
 * channel (2 or 4 bytes each); px the sum of the sample sizes, lb = width * px
 * a line's bytes, n = lines * lb the raw chunk.  Its coding, with h = (n + 1) /
 * 2: t = the even bytes of raw, then the odd ones; p[0] = t[0], p[i] = t[i] -
 * t[i - 1] + 128; the stored data is the zlib stream of p where that is
 * shorter than n, else raw itself.
 *
 * The reader's plan puts every row in a class by its dataSize: above n it is
 * BAD_DATA on the spot; equal to n it is raw - a *direct* row (LINES at a pitch
 * of lb, or one line) is one span of lda_zip_copy_kernel, any other goes
 * through the layout kernel straight from d_in -; below n it is a zlib stream,
 * decoded into a room for p in the object's scratch.
 *
 * lda_exr_undo_kernel turns p into raw in tiles of EXR_TILE raw bytes, a wave
 * a tile.  Tile j of a chunk needs two stretches of p, EXR_TILE / 2 bytes
 * each: A_j = p[j S, ...) of the first half and B_j = p[h + j S, ...) of the
 * second.  The running sum in front of a stretch is its *carry*: the chunk's
 * stretches in the order A_0 .. A_{nt-1}, B_0 .. B_{nt-1} partition p (a B
 * stretch may be empty), so slot s of a chunk carries from the slots 0 .. s -
 * 1 of the same chunk and from no other.  lda_exr_sums_kernel leaves every
 * stretch's byte sum in its slot - chunk k's slots start at 2 * (the tiles in
 * front of chunk k), A_j at + j, B_j at + nt + j -, lda_exr_carry_kernel
 * replaces them by the exclusive sums, restarted at every chunk, and the undo
 * kernel adds the slot's carry.  A direct row's tiles are written straight into
 * d_out, any other's into a second room, for raw, which the layout kernel
 * reads.
 *
 * The layout kernel's rows (EXR_LCOLS) describe one chunk each, its raw side
 * and its pixel side; the work is counted in *items* - LINES: 16 bytes of a
 * line; PIXELS with samples of one size and up to four channels: the 16 / size
 * pixels whose planes' pieces fill one 16-byte load each; PIXELS otherwise: one
 * pixel - and a tile is EXR_LTILE items.  The writer's gather kernel runs the
 * same rows the other way.
 *
 * The writer's plan gives every chunk two rooms at the same offset of two
 * areas, raw and coded, and cuts the coded rooms into the writers' shared
 * pieces (write_pieces_plan.h); a chunk that is stored raw copies the same
 * ranges of the raw area.
 */
#ifndef LDA_EXR_PLAN_H
#define LDA_EXR_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "chunk_plan.h"

namespace lda {

enum {
	EXR_WORDS = 10,		/* LIBDEFLATE_AMD_EXR_WORDS */
	EXR_CHANNELS_MAX = 16,	/* LIBDEFLATE_AMD_EXR_CHANNELS_MAX */
	EXR_RESULT_WORDS = 4,	/* LIBDEFLATE_AMD_EXRW_RESULT_WORDS */
	EXR_LINES = 0, EXR_PIXELS = 1,	/* LIBDEFLATE_AMD_EXR_LINES, _PIXELS */
	EXR_LANE = 32,		/* LDA_EXR_LANE: raw bytes a lane undoes */
	EXR_TILE = 2048,	/* LDA_EXR_TILE: raw bytes a wave undoes, 64 lanes */
	EXR_WG_TILES = 4,	/* LDA_EXR_WG_TILES: the waves, and tiles, of a workgroup */
	EXR_LTILE = 256,	/* LDA_EXR_LTILE: items of a layout tile */
	EXR_CTILE = 4096,	/* LDA_EXR_CTILE: bytes of a coded room one workgroup makes */
	/* a row's words */
	EXR_W_DATA_OFF = 0, EXR_W_DATA_N, EXR_W_PIX_OFF, EXR_W_PITCH, EXR_W_GEOM, EXR_W_FMT,
	EXR_W_SLOTS, EXR_W_HEAD, EXR_W_H0, EXR_W_H1,
	/* the row classes */
	EXR_C_BAD = 0, EXR_C_RAW_DIRECT, EXR_C_RAW_LAYOUT, EXR_C_ZLIB,
	/* the copy kernel's columns, n_copy words each */
	EXR_P_SRC = 0, EXR_P_DST, EXR_P_LEN, EXR_PCOLS,
	/* the undo kernels' columns, n_z words each */
	EXR_U_TILE_END = 0,	/* the tiles of this chunk and all before it */
	EXR_U_SRC,		/* the room of p, in the coded area */
	EXR_U_N,
	EXR_U_DST,		/* EXR_DST_OUT: in d_out, else in the raw area */
	EXR_UCOLS,
	/* the layout kernel's and the gather kernel's columns, n_l words each */
	EXR_L_TILE_END = 0,
	EXR_L_RAW,		/* the raw chunk; the reader: EXR_RAW_IN: in d_in, else in the raw area */
	EXR_L_PIX,		/* line 0, pixel 0 on the pixel side */
	EXR_L_PITCH,
	EXR_L_GEOM,		/* word 4 */
	EXR_L_FMT,		/* word 5 */
	EXR_L_DOFF0,		/* PIXELS: 8 bits per channel, where channel k stands in the pixel */
	EXR_L_DOFF1,		/* channels 8 .. 15 */
	EXR_LCOLS,
	/* the writer's per-chunk columns, n words each, behind CHUNKW_E_USIZE */
	EXRW_E_ROOM = CHUNKW_E_USIZE + 1, EXRW_E_CTILE_END, EXRW_E_WORDS,
	EXRW_ECOLS = EXRW_E_WORDS + 8	/* words 2 .. 9 of the row */
};
#define EXR_MAX_CHUNKS ((uint64_t)1 << 28)
#define EXR_DST_OUT ((uint64_t)1 << 63)	/* LDA_EXR_DST_OUT */
#define EXR_RAW_IN ((uint64_t)1 << 63)	/* LDA_EXR_RAW_IN */
#define EXR_VERD_OWN ((uint64_t)1 << 63)	/* LDA_SHUF_VERD_OWN */
#define EXR_PIECE_MAX 0xFFFFFF00ull	/* as SHUF_PIECE_MAX */

/* a row taken apart; sizes as 64-bit numbers */
struct exr_chunk {
	uint64_t w, lines, c, mask, layout, px, lb, n;
	bool uniform;	/* samples of one size and at most four channels: the register path */
	uint64_t sz;	/* that size */
};

static inline exr_chunk exr_chunk_of(const uint64_t *r)
{
	exr_chunk s;
	s.w = r[EXR_W_GEOM] & 0xFFFFFFFFull;
	s.lines = r[EXR_W_GEOM] >> 32;
	s.c = r[EXR_W_FMT] & 0xFF;
	s.mask = (r[EXR_W_FMT] >> 8) & 0xFFFF;
	s.layout = r[EXR_W_FMT] >> 32;
	s.px = 0;
	for (uint64_t k = 0; k < s.c && k < EXR_CHANNELS_MAX; k++)
		s.px += (s.mask >> k & 1) ? 4 : 2;
	s.lb = s.w * s.px;
	s.n = s.lb * s.lines;	/* (meaningful only after the checks; see exr_row_why) */
	const uint64_t all = s.c <= EXR_CHANNELS_MAX ? ((uint64_t)1 << s.c) - 1 : 0;
	s.uniform = s.c >= 1 && s.c <= 4 && (s.mask == 0 || s.mask == all);
	s.sz = s.mask ? 4 : 2;
	return s;
}

/* the size of channel k's samples */
static inline uint64_t exr_size_of(const exr_chunk &s, uint64_t k) { return (s.mask >> k & 1) ? 4 : 2; }

/* what either call refuses in row r, or NULL.  reader: the stored range;
 * pix_avail: out_avail of the reader, in_avail of the writer; level: the
 * writer's */
static inline const char *
exr_row_why(const uint64_t *row, bool reader, uint64_t stored_avail, uint64_t pix_avail, int level)
{
	const exr_chunk s = exr_chunk_of(row);

	if ((row[EXR_W_FMT] >> 24 & 0xFF) || (row[EXR_W_FMT] >> 33))
		return "unknown bits in word 5";
	if (s.c == 0 || s.c > EXR_CHANNELS_MAX)
		return "channels outside 1 .. 16";
	if (s.mask >> s.c)
		return "a wide-mask bit at or above the channel count";
	if (s.w == 0 || s.lines == 0)
		return "a zero width or zero lines";
	if (s.layout == EXR_LINES) {
		if (row[EXR_W_SLOTS])
			return "word 6 is not 0 for the LINES layout";
	} else {
		uint64_t seen = 0;
		if (s.c < 16 && (row[EXR_W_SLOTS] >> (4 * s.c)))
			return "the slots are not a permutation of the channels";
		for (uint64_t k = 0; k < s.c; k++) {
			const uint64_t slot = row[EXR_W_SLOTS] >> (4 * k) & 15;
			if (slot >= s.c || (seen >> slot & 1))
				return "the slots are not a permutation of the channels";
			seen |= (uint64_t)1 << slot;
		}
	}
	if (row[EXR_W_HEAD] != 0 && row[EXR_W_HEAD] != 8 && row[EXR_W_HEAD] != 20)
		return "a head length that is not 0, 8 or 20";
	/* w * px < 2^38 and lines < 2^32: the product could pass 2^64 */
	if (s.lb > 0xFFFFFFFFull || s.lb * s.lines > 0xFFFFFFFFull)
		return "a raw size of 2^32 bytes or more";
	if (reader && (row[EXR_W_DATA_OFF] > stored_avail ||
		       stored_avail - row[EXR_W_DATA_OFF] < row[EXR_W_DATA_N]))
		return "its stored bytes do not lie inside in_nbytes";
	if (s.lines > 1 && row[EXR_W_PITCH] < s.lb)
		return "a pitch below the line's bytes";
	{
		/* word 2 + (lines - 1) * pitch + line bytes <= pix_avail, without overflow */
		const char *outside = reader ? "its lines do not lie inside out_avail" :
					       "its lines do not lie inside in_avail";
		const uint64_t off = row[EXR_W_PIX_OFF], pitch = s.lines > 1 ? row[EXR_W_PITCH] : 0;
		if (off > pix_avail || pix_avail - off < s.lb)
			return outside;
		const uint64_t room = pix_avail - off - s.lb;
		if (pitch && (s.lines - 1) > room / pitch)
			return outside;
	}
	if (!reader && level == 0 && s.n > EXR_PIECE_MAX)
		return "a level-0 chunk above 0xFFFFFF00 bytes, which no compress call takes";
	return NULL;
}

/* true, or false with the reason in err: pointers apart, what a call refuses
 * before any device work */
static inline bool
exr_check(uint64_t n, const uint64_t *rows, bool reader, uint64_t stored_avail, uint64_t pix_avail,
	  int level, std::string &err)
{
	return chunk_check("n_chunks", n, EXR_MAX_CHUNKS, [&](uint64_t r) {
		return exr_row_why(rows + EXR_WORDS * r, reader, stored_avail, pix_avail, level);
	}, err);
}

/* the sum of head + n: no chunk is written longer than raw; 0 for rows the
 * writer refuses */
static inline uint64_t exr_bound(uint64_t n, const uint64_t *rows)
{
	return chunk_bound(n, EXR_MAX_CHUNKS, [&](uint64_t r) {
		return exr_row_why(rows + EXR_WORDS * r, false, 0, ~(uint64_t)0, -1);
	}, [&](uint64_t r) { return rows[EXR_WORDS * r + EXR_W_HEAD] + exr_chunk_of(rows + EXR_WORDS * r).n; });
}

/* is the pixel side of the row the raw chunk itself, in one span? */
static inline bool exr_direct(const uint64_t *row)
{
	const exr_chunk s = exr_chunk_of(row);
	return s.layout == EXR_LINES && (s.lines == 1 || row[EXR_W_PITCH] == s.lb);
}

static inline int exr_class(const uint64_t *row)
{
	const exr_chunk s = exr_chunk_of(row);
	if (row[EXR_W_DATA_N] > s.n)
		return EXR_C_BAD;
	if (row[EXR_W_DATA_N] == s.n)
		return exr_direct(row) ? EXR_C_RAW_DIRECT : EXR_C_RAW_LAYOUT;
	return EXR_C_ZLIB;
}

/* ---- the undo kernels' tiles ---- */

static inline uint64_t exr_tiles(uint64_t n) { return (n + EXR_TILE - 1) / EXR_TILE; }

/* the bytes of stretch A_j (second false) or B_j of a chunk of n bytes, and
 * where it starts in p */
static inline uint64_t exr_stretch(uint64_t n, uint64_t j, bool second, uint64_t *start)
{
	const uint64_t h = (n + 1) / 2, S = EXR_TILE / 2;
	const uint64_t len = second ? n - h : h;
	*start = (second ? h : 0) + j * S;
	if (j * S >= len)
		return 0;
	return len - j * S < S ? len - j * S : S;
}

/* ---- the layout rows ---- */

/* the items of a line of the chunk: see the top of the file */
static inline uint64_t exr_line_items(const exr_chunk &s)
{
	if (s.layout == EXR_LINES)
		return (s.lb + 15) / 16;
	if (s.uniform)
		return (s.w + 16 / s.sz - 1) / (16 / s.sz);
	return s.w;
}

struct exr_layout_rows {
	std::vector<uint64_t> col[EXR_LCOLS];
	uint64_t tiles = 0;

	void add(const uint64_t *row, uint64_t raw)
	{
		const exr_chunk s = exr_chunk_of(row);
		uint64_t slot_off[EXR_CHANNELS_MAX] = { 0 }, doff[2] = { 0, 0 };
		const uint64_t items = s.lines * exr_line_items(s);	/* (below 2^32: n is) */

		tiles += (items + EXR_LTILE - 1) / EXR_LTILE;
		if (s.layout == EXR_PIXELS) {
			/* the bytes in front of every slot, then every channel's place */
			uint64_t size_of_slot[EXR_CHANNELS_MAX] = { 0 }, at = 0;
			for (uint64_t k = 0; k < s.c; k++)
				size_of_slot[row[EXR_W_SLOTS] >> (4 * k) & 15] = exr_size_of(s, k);
			for (uint64_t q = 0; q < s.c; q++) {
				slot_off[q] = at;
				at += size_of_slot[q];
			}
			for (uint64_t k = 0; k < s.c; k++)
				doff[k >> 3] |= slot_off[row[EXR_W_SLOTS] >> (4 * k) & 15] << (8 * (k & 7));
		}
		col[EXR_L_TILE_END].push_back(tiles);
		col[EXR_L_RAW].push_back(raw);
		col[EXR_L_PIX].push_back(row[EXR_W_PIX_OFF]);
		col[EXR_L_PITCH].push_back(s.lines > 1 ? row[EXR_W_PITCH] : 0);
		col[EXR_L_GEOM].push_back(row[EXR_W_GEOM]);
		col[EXR_L_FMT].push_back(row[EXR_W_FMT]);
		col[EXR_L_DOFF0].push_back(doff[0]);
		col[EXR_L_DOFF1].push_back(doff[1]);
	}
};

struct exr_read_plan {
	uint64_t n;
	uint64_t n_z;		/* zlib rows */
	uint64_t n_copy;	/* raw-direct rows */
	uint64_t n_l, ltiles;	/* the layout kernel's rows and tiles */
	uint64_t utiles;	/* the undo kernels' tiles; twice as many slots */
	uint64_t coded_bytes;	/* the area of the rooms of p */
	uint64_t raw_bytes;	/* the area of the rooms of raw */
	/* what goes up: [CHUNK_DCOLS x n_z] at 0, [EXR_UCOLS x n_z] at u_at, [EXR_PCOLS
	 * x n_copy] at p_at, [EXR_LCOLS x n_l] at l_at, [n verdict words] at verd_at */
	uint64_t u_at, p_at, l_at, verd_at;
	std::vector<uint64_t> cols;
};

/* the rows have passed exr_check() */
static inline void exr_read_plan_build(uint64_t n, const uint64_t *rows, exr_read_plan &p)
{
	std::vector<uint64_t> u[EXR_UCOLS], c[EXR_PCOLS], verd((size_t)n);
	chunk_rooms coded, raw;
	exr_layout_rows l;

	p.n = n;
	p.n_z = p.utiles = 0;
	std::vector<uint8_t> cls((size_t)n);
	for (uint64_t r = 0; r < n; r++)
		p.n_z += (cls[(size_t)r] = (uint8_t)exr_class(rows + EXR_WORDS * r)) == EXR_C_ZLIB;
	chunk_decode_cols d(p.cols, p.n_z);
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows + EXR_WORDS * r;
		const exr_chunk s = exr_chunk_of(w);
		switch (cls[(size_t)r]) {
		case EXR_C_BAD:
			verd[(size_t)r] = EXR_VERD_OWN | 1;	/* LIBDEFLATE_BAD_DATA */
			break;
		case EXR_C_RAW_DIRECT:
			verd[(size_t)r] = EXR_VERD_OWN | 0;
			c[EXR_P_SRC].push_back(w[EXR_W_DATA_OFF]);
			c[EXR_P_DST].push_back(w[EXR_W_PIX_OFF]);
			c[EXR_P_LEN].push_back(s.n);
			break;
		case EXR_C_RAW_LAYOUT:
			verd[(size_t)r] = EXR_VERD_OWN | 0;
			l.add(w, w[EXR_W_DATA_OFF] | EXR_RAW_IN);
			break;
		default: {
			const uint64_t room = coded.take(s.n);
			verd[(size_t)r] = d.add(false, w[EXR_W_DATA_OFF], w[EXR_W_DATA_N], room, s.n);
			p.utiles += exr_tiles(s.n);
			u[EXR_U_TILE_END].push_back(p.utiles);
			u[EXR_U_SRC].push_back(room);
			u[EXR_U_N].push_back(s.n);
			if (exr_direct(w)) {
				u[EXR_U_DST].push_back(w[EXR_W_PIX_OFF] | EXR_DST_OUT);
			} else {
				u[EXR_U_DST].push_back(raw.take(s.n));
				l.add(w, u[EXR_U_DST].back());
			}
			break;
		}
		}
	}
	p.n_copy = c[0].size();
	p.n_l = l.col[0].size();
	p.ltiles = l.tiles;
	p.coded_bytes = coded.bytes;
	p.raw_bytes = raw.bytes;
	p.u_at = chunk_append(p.cols, u, EXR_UCOLS);
	p.p_at = chunk_append(p.cols, c, EXR_PCOLS);
	p.l_at = chunk_append(p.cols, l.col, EXR_LCOLS);
	p.verd_at = chunk_append(p.cols, &verd);
}

struct exr_write_plan : chunk_write_plan {	/* rooms_bytes: of either area */
	uint64_t ctiles;	/* the coding kernel's tiles */
	uint64_t ltiles;	/* the gather kernel's */
	uint64_t l_at;		/* ecols: [EXRW_ECOLS x n] at 0, [EXR_LCOLS x n] at l_at */
};

/* the rows have passed exr_check(); pr.store is false whatever the level */
static inline void
exr_write_plan_build(const zipw_params &pr, uint64_t n, const uint64_t *rows, exr_write_plan &p)
{
	chunk_write_rows e(p, n, EXRW_ECOLS);
	exr_layout_rows l;

	p.ctiles = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = rows + EXR_WORDS * k;
		const exr_chunk s = exr_chunk_of(w);
		const uint64_t room = e.add(s.n, s.n);
		p.ctiles += (s.n + EXR_CTILE - 1) / EXR_CTILE;
		p.ecols[(size_t)(EXRW_E_ROOM * n + k)] = room;
		p.ecols[(size_t)(EXRW_E_CTILE_END * n + k)] = p.ctiles;
		for (uint64_t a = 0; a < 8; a++)
			p.ecols[(size_t)((EXRW_E_WORDS + a) * n + k)] = w[2 + a];
		l.add(w, room);
	}
	p.ltiles = l.tiles;
	e.cut(pr);
	p.l_at = chunk_append(p.ecols, l.col, EXR_LCOLS);
}

} /* namespace lda */

#endif /* LDA_EXR_PLAN_H */
