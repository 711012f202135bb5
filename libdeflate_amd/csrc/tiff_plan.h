/*
 * tiff_plan.h - the host arithmetic of the predictor-coded deflate strips and
 * tiles of TIFF and GeoTIFF (include/libdeflate_amd.h:
 * libdeflate_amd_tiff_decode_batch, host_tiff.hip, and
 * libdeflate_amd_tiff_encode_batch, host_tiff_write.hip): the refusals made
 * before any device work, the bound, and the two plans.  Free of HIP:
 * tools/test_tiff_plan.cpp runs it on the CPU.
 *
 * A segment - a strip or a tile - is one zlib stream of coded_rows rows of
 * coded_width pixels, a pixel spp samples of bps bytes, px = spp * bps.
 * Predictor 2: every sample is stored minus the sample px bytes earlier in its
 * row, modulo 2^(8 bps).  Predictor 3: the row's samples are split into bps
 * byte planes, the most significant first, and the planes' bytes - the whole
 * row of them - are stored minus the byte spp places earlier.
 *
 * The reader's plan classifies every row: a *direct* row - predictor 1, kept
 * equal to coded, a pitch equal to the row's bytes or a single row - is decoded
 * straight into d_out; every other row is decoded into a room of the object's
 * scratch (16-byte boundaries) and moved by lda_tiff_unpredict_kernel.  The
 * decode batch's columns hold the scratch rows first, then the d_out rows: two
 * decompress batches, one per output base, and either is left out when it has
 * no row.
 *
 * The unpredict kernel's rows (TIFF_KCOLS) are *scans*: `rows` rows of `rb`
 * bytes, samples of sb bytes, each added to the sample st bytes earlier (st 0:
 * a copy).  Predictors 1 and 2 scan the kept rectangle from the room into
 * d_out (sb = bps, st = px); predictor 3 scans the whole coded row of every
 * kept row in place in the room (sb = 1, st = spp), and lda_tiff_gather_kernel
 * (TIFF_GCOLS) then collects the kept pixels from the planes.  A scan is
 * walked by groups of G = 4, 16 or 64 lanes, one group a row; the kernel's
 * work is counted in quads of 4 lanes, and the rows are ordered by G - 64,
 * 16, 4 - so that every group lies inside one wave.
 *
 * The writer's plan gives every segment a room for its predicted bytes in the
 * object's scratch and cuts the rooms into the writers' shared pieces
 * (write_pieces_plan.h).  lda_tiff_predict_kernel fills the rooms in tiles of
 * TIFF_PTILE bytes.
 */
#ifndef LDA_TIFF_PLAN_H
#define LDA_TIFF_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "chunk_plan.h"

namespace lda {

enum {
	TIFF_WORDS = 8,		/* LIBDEFLATE_AMD_TIFF_WORDS */
	TIFF_SPP_MAX = 16,	/* LIBDEFLATE_AMD_TIFF_SPP_MAX */
	TIFF_RESULT_WORDS = 4,	/* LIBDEFLATE_AMD_TIFFW_RESULT_WORDS */
	TIFF_PTILE = 4096,	/* LDA_TIFF_PTILE: bytes of a room one workgroup predicts */
	/* a row's words */
	TIFF_W_STORED_OFF = 0, TIFF_W_STORED_N, TIFF_W_RAW_OFF, TIFF_W_PITCH, TIFF_W_CODED,
	TIFF_W_KEPT, TIFF_W_FMT, TIFF_W_RESERVED,
	/* the unpredict kernel's columns, n_k words each */
	TIFF_K_QUAD_END = 0,	/* the quads of this scan and all before it */
	TIFF_K_SRC,		/* where the first row is read, in the scratch */
	TIFF_K_DST,		/* where it is written, TIFF_DST_WS: in the scratch */
	TIFF_K_DPITCH,		/* between written rows */
	TIFF_K_GEOM,		/* rb | sb << 32 | st << 40 | G << 48 */
	TIFF_K_SPITCH,		/* between read rows */
	TIFF_KCOLS,
	/* the gather kernel's columns, n_g words each */
	TIFF_G_TILE_END = 0,	/* tiles of 256 items, running; an item is four samples of a kept row */
	TIFF_G_SRC,		/* the scanned room */
	TIFF_G_DST,
	TIFF_G_DPITCH,
	TIFF_G_GEOM,		/* kept samples of a row | bps << 32 */
	TIFF_G_PLANE,		/* coded samples of a row - the planes' distance; the rows' is bps
				 * times it - | the items << 32: kept_rows * ceil(kept samples / 4) */
	TIFF_GCOLS,
	/* the writer's per-segment columns, n words each, behind CHUNKW_E_USIZE */
	TIFFW_E_RAW_OFF = CHUNKW_E_USIZE + 1, TIFFW_E_PITCH, TIFFW_E_CODED, TIFFW_E_KEPT, TIFFW_E_FMT,
	TIFFW_E_ROOM, TIFFW_E_TILE_END,
	TIFFW_ECOLS
};
#define TIFF_MAX_SEGMENTS ((uint64_t)1 << 28)
#define TIFF_DST_WS ((uint64_t)1 << 63)	/* LDA_TIFF_DST_WS */
#define TIFF_PIECE_MAX 0xFFFFFF00ull	/* as SHUF_PIECE_MAX */

/* a row taken apart; sizes as 64-bit numbers */
struct tiff_seg {
	uint64_t cw, cr, kw, kr, spp, bps, pred, px;
	uint64_t coded_rb, kept_rb, coded;	/* bytes of a coded row, a kept row, the segment */
};

static inline tiff_seg tiff_seg_of(const uint64_t *w)
{
	tiff_seg s;
	s.cw = w[TIFF_W_CODED] & 0xFFFFFFFFull;
	s.cr = w[TIFF_W_CODED] >> 32;
	s.kw = w[TIFF_W_KEPT] & 0xFFFFFFFFull;
	s.kr = w[TIFF_W_KEPT] >> 32;
	s.spp = w[TIFF_W_FMT] & 0xFF;
	s.bps = (w[TIFF_W_FMT] >> 8) & 0xFF;
	s.pred = (w[TIFF_W_FMT] >> 16) & 0xFF;
	s.px = s.spp * s.bps;
	s.coded_rb = s.cw * s.px;
	s.kept_rb = s.kw * s.px;
	s.coded = s.coded_rb * s.cr;	/* (below 2^40 * 2^32 only after the checks; see tiff_row_why) */
	return s;
}

/* what either call refuses in row r, or NULL.  reader: the stored range;
 * raw_avail: out_avail of the reader, in_avail of the writer; level: the
 * writer's */
static inline const char *
tiff_row_why(const uint64_t *row, bool reader, uint64_t stored_avail, uint64_t raw_avail, int level)
{
	const tiff_seg s = tiff_seg_of(row);

	if (row[TIFF_W_FMT] >> 24)
		return "unknown bits in word 6";
	if (row[TIFF_W_RESERVED])
		return "word 7 is reserved and not 0";
	if (s.spp == 0 || s.spp > TIFF_SPP_MAX)
		return "samples per pixel outside 1 .. 16";
	if (s.bps != 1 && s.bps != 2 && s.bps != 4 && s.bps != 8)
		return "bytes per sample not 1, 2, 4 or 8";
	if (s.pred < 1 || s.pred > 3)
		return "a predictor that is not 1, 2 or 3";
	if (s.pred == 3 && s.bps == 1)
		return "the floating-point predictor with bytes per sample 1";
	if (s.cw == 0 || s.cr == 0 || s.kw == 0 || s.kr == 0)
		return "a zero width or zero rows";
	if (s.kw > s.cw || s.kr > s.cr)
		return "kept above coded";
	/* cw * px < 2^39 and cr < 2^32: the product could pass 2^64 */
	if (s.coded_rb > 0xFFFFFFFFull || s.coded_rb * s.cr > 0xFFFFFFFFull)
		return "a coded size of 2^32 bytes or more";
	if (reader && (row[TIFF_W_STORED_OFF] > stored_avail ||
		       stored_avail - row[TIFF_W_STORED_OFF] < row[TIFF_W_STORED_N]))
		return "its stored bytes do not lie inside in_nbytes";
	if (s.kr > 1 && row[TIFF_W_PITCH] < s.kept_rb)
		return "a pitch below the kept row's bytes";
	{
		/* word2 + (kept_rows - 1) * pitch + kept row bytes <= raw_avail, without overflow */
		const char *outside = reader ? "its kept rectangle does not lie inside out_avail" :
					       "its kept rectangle does not lie inside in_avail";
		const uint64_t off = row[TIFF_W_RAW_OFF], pitch = s.kr > 1 ? row[TIFF_W_PITCH] : 0;
		if (off > raw_avail || raw_avail - off < s.kept_rb)
			return outside;
		const uint64_t room = raw_avail - off - s.kept_rb;
		if (pitch && (s.kr - 1) > room / pitch)
			return outside;
	}
	if (!reader && level == 0 && s.coded > TIFF_PIECE_MAX)
		return "a level-0 segment above 0xFFFFFF00 bytes, which no compress call takes";
	return NULL;
}

/* true, or false with the reason in err: pointers apart, what a call refuses
 * before any device work */
static inline bool
tiff_check(uint64_t n, const uint64_t *rows, bool reader, uint64_t stored_avail, uint64_t raw_avail,
	   int level, std::string &err)
{
	return chunk_check("n_segments", n, TIFF_MAX_SEGMENTS, [&](uint64_t r) {
		return tiff_row_why(rows + TIFF_WORDS * r, reader, stored_avail, raw_avail, level);
	}, err);
}

/* the sum of the zlib streams' bounds; 0 for rows the writer refuses */
static inline uint64_t tiff_bound(uint64_t n, const uint64_t *rows)
{
	return chunk_bound(n, TIFF_MAX_SEGMENTS, [&](uint64_t r) {
		return tiff_row_why(rows + TIFF_WORDS * r, false, 0, ~(uint64_t)0, -1);
	}, [&](uint64_t r) { return chunk_stream_bound(1, tiff_seg_of(rows + TIFF_WORDS * r).coded); });
}

/* is the row decoded straight into d_out? */
static inline bool tiff_direct(const uint64_t *row)
{
	const tiff_seg s = tiff_seg_of(row);
	return s.pred == 1 && s.kw == s.cw && s.kr == s.cr && (s.cr == 1 || row[TIFF_W_PITCH] == s.coded_rb);
}

/* ---- the scans ---- */

/* does the kernel keep a stride of st bytes in registers?  A lane then owns
 * tiff_lane_bytes(st) bytes of a row: whole pixels */
static inline bool tiff_reg_stride(uint64_t st)
{
	return st == 0 || st == 1 || st == 2 || st == 4 || st == 8 || st == 16 || st == 3 || st == 6 ||
	       st == 12 || st == 24 || st == 48;
}

static inline uint64_t tiff_lane_bytes(uint64_t st)
{
	if (!tiff_reg_stride(st))
		return st;	/* the generic path: one pixel a lane */
	if (st == 0)
		return 16;	/* the copy */
	return st == 3 || st == 6 || st == 12 || st == 24 || st == 48 ? 48 : 64;
}

/* the lanes of a group by the row's bytes: one pass where 4 or 16 lanes do */
static inline uint64_t tiff_group(uint64_t rb, uint64_t st)
{
	const uint64_t L = tiff_lane_bytes(st);
	return rb <= 4 * L ? 4 : rb <= 16 * L ? 16 : 64;
}

struct tiff_scan {
	uint64_t src, dst, spitch, dpitch, rows, rb, sb, st, G;
};

/* the unpredict kernel's rows: scans added in any order, laid out by G */
struct tiff_kernel_rows {
	std::vector<tiff_scan> scans;

	void add(uint64_t src, uint64_t dst, uint64_t spitch, uint64_t dpitch, uint64_t rows,
		 uint64_t rb, uint64_t sb, uint64_t st)
	{
		const tiff_scan s = { src, dst, spitch, dpitch, rows, rb, sb, st, tiff_group(rb, st) };
		scans.push_back(s);
	}
	/* TIFF_KCOLS x n_k words behind what cols holds; -> the quads */
	uint64_t append_to(std::vector<uint64_t> &cols) const
	{
		const size_t n_k = scans.size(), at = cols.size();
		uint64_t quads = 0;
		size_t k = 0;
		cols.resize(at + TIFF_KCOLS * n_k);
		for (uint64_t G : { (uint64_t)64, (uint64_t)16, (uint64_t)4 })
			for (const tiff_scan &s : scans) {
				if (s.G != G)
					continue;
				quads += s.rows * (G / 4);
				cols[at + TIFF_K_QUAD_END * n_k + k] = quads;
				cols[at + TIFF_K_SRC * n_k + k] = s.src;
				cols[at + TIFF_K_DST * n_k + k] = s.dst;
				cols[at + TIFF_K_DPITCH * n_k + k] = s.dpitch;
				cols[at + TIFF_K_GEOM * n_k + k] = s.rb | s.sb << 32 | s.st << 40 | G << 48;
				cols[at + TIFF_K_SPITCH * n_k + k] = s.spitch;
				k++;
			}
		return quads;
	}
};

struct tiff_read_plan {
	uint64_t n;
	uint64_t n_ws;		/* decoded into the scratch */
	uint64_t n_direct;	/* decoded into d_out */
	uint64_t n_k, quads;	/* the unpredict kernel's rows and quads */
	uint64_t n_g, gtiles;	/* the gather kernel's rows and tiles */
	uint64_t scratch;	/* bytes of the scratch rooms */
	/* what goes up: [CHUNK_DCOLS x (n_ws + n_direct)] at 0, [TIFF_KCOLS x n_k]
	 * at k_at, [TIFF_GCOLS x n_g] at g_at, [n verdict words] at verd_at */
	uint64_t k_at, g_at, verd_at;
	std::vector<uint64_t> cols;
};

/* the rows have passed tiff_check() */
static inline void tiff_read_plan_build(uint64_t n, const uint64_t *rows, tiff_read_plan &p)
{
	p.n = n;
	p.n_ws = p.n_direct = 0;
	for (uint64_t r = 0; r < n; r++) {
		if (tiff_direct(rows + TIFF_WORDS * r))
			p.n_direct++;
		else
			p.n_ws++;
	}
	std::vector<uint64_t> verd((size_t)n);
	std::vector<uint64_t> g[TIFF_GCOLS];
	chunk_decode_cols d(p.cols, p.n_ws, p.n_direct);
	chunk_rooms rooms;
	tiff_kernel_rows k;
	uint64_t gtiles = 0;
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows + TIFF_WORDS * r;
		const tiff_seg s = tiff_seg_of(w);
		const bool direct = tiff_direct(w);
		const uint64_t room = direct ? 0 : rooms.take(s.coded);
		const uint64_t pitch = s.kr > 1 ? w[TIFF_W_PITCH] : 0;
		verd[(size_t)r] = d.add(direct, w[TIFF_W_STORED_OFF], w[TIFF_W_STORED_N],
					direct ? w[TIFF_W_RAW_OFF] : room, s.coded);
		if (direct)
			continue;
		if (s.pred == 3) {
			/* the whole coded row of every kept row, in place; then the gather */
			k.add(room, room | TIFF_DST_WS, s.coded_rb, s.coded_rb, s.kr, s.coded_rb, 1, s.spp);
			const uint64_t ns = s.kw * s.spp;
			const uint64_t items = s.kr * ((ns + 3) / 4);	/* (below 2^32: the coded size is) */
			gtiles += (items + 255) / 256;
			g[TIFF_G_TILE_END].push_back(gtiles);
			g[TIFF_G_SRC].push_back(room);
			g[TIFF_G_DST].push_back(w[TIFF_W_RAW_OFF]);
			g[TIFF_G_DPITCH].push_back(pitch);
			g[TIFF_G_GEOM].push_back(ns | s.bps << 32);
			g[TIFF_G_PLANE].push_back(s.cw * s.spp | items << 32);
		} else {
			k.add(room, w[TIFF_W_RAW_OFF], s.coded_rb, pitch, s.kr, s.kept_rb, s.bps,
			      s.pred == 2 ? s.px : 0);
		}
	}
	p.scratch = rooms.bytes;
	p.n_k = k.scans.size();
	p.k_at = p.cols.size();
	p.quads = k.append_to(p.cols);
	p.n_g = g[0].size();
	p.gtiles = gtiles;
	p.g_at = chunk_append(p.cols, g, TIFF_GCOLS);
	p.verd_at = chunk_append(p.cols, &verd);
}

struct tiff_write_plan : chunk_write_plan {	/* raw_total: the kept rectangles' bytes */
	uint64_t tiles;		/* the predict kernel's */
	/* ecols: [TIFFW_ECOLS x n] */
};

/* the rows have passed tiff_check(); pr.store is false whatever the level */
static inline void
tiff_write_plan_build(const zipw_params &pr, uint64_t n, const uint64_t *rows, tiff_write_plan &p)
{
	chunk_write_rows e(p, n, TIFFW_ECOLS);

	p.tiles = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = rows + TIFF_WORDS * k;
		const tiff_seg s = tiff_seg_of(w);
		p.tiles += (s.coded + TIFF_PTILE - 1) / TIFF_PTILE;
		p.ecols[(size_t)(TIFFW_E_RAW_OFF * n + k)] = w[TIFF_W_RAW_OFF];
		p.ecols[(size_t)(TIFFW_E_PITCH * n + k)] = w[TIFF_W_PITCH];
		p.ecols[(size_t)(TIFFW_E_CODED * n + k)] = w[TIFF_W_CODED];
		p.ecols[(size_t)(TIFFW_E_KEPT * n + k)] = w[TIFF_W_KEPT];
		p.ecols[(size_t)(TIFFW_E_FMT * n + k)] = w[TIFF_W_FMT];
		p.ecols[(size_t)(TIFFW_E_ROOM * n + k)] = e.add(s.coded, s.kept_rb * s.kr);
		p.ecols[(size_t)(TIFFW_E_TILE_END * n + k)] = p.tiles;
	}
	e.cut(pr);
}

} /* namespace lda */

#endif /* LDA_TIFF_PLAN_H */
