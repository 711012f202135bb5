/*
 * shuffle_plan.h - the host arithmetic of the byte-shuffled deflate chunks of
 * HDF5, NetCDF-4 and Zarr (include/libdeflate_amd.h:
 * libdeflate_amd_shuffle_decompress_batch, host_shuffle.hip, and
 * libdeflate_amd_shuffle_compress_batch, host_shuffle_write.hip): the refusals
 * made before any device work, the bound, and the two plans.  Free of HIP:
 * tools/test_shuffle_plan.cpp runs it on the CPU.
 *
 * The transform.  A chunk of n bytes and element size es has ne = n / es
 * elements and left = n % es bytes behind them:
 *     shuffled[j * ne + k]  = raw[k * es + j]     0 <= j < es, 0 <= k < ne
 *     shuffled[es * ne + t] = raw[es * ne + t]    0 <= t < left
 * (H5Z_FILTER_SHUFFLE), the identity when es == 1 or ne <= 1.
 *
 * The reader's plan classifies every row: a deflated row whose transform is the
 * identity is decoded straight into its room of d_out; a deflated, shuffled row
 * is decoded into a room of the object's scratch (16-byte boundaries) and
 * unshuffled from there; a NO_DEFLATE row is unshuffled - or, the identity,
 * copied as element size 1 - from its stored bytes in d_in (SHUF_SRC_ALT); a
 * NO_DEFLATE row whose two sizes differ is BAD_DATA and meets no kernel.  The
 * decode batch's columns hold the scratch rows first, then the d_out rows: two
 * decompress batches, one per output base, and either is left out when it has
 * no row.  The kernels' rows (SHUF_UCOLS) are the same for lda_unshuffle_kernel
 * and lda_shuffle_kernel: the running tile count, the two offsets, the size and
 * the element size.  A tile is shuf_tile_elems(es) consecutive elements.
 *
 * The writer's plan gives every chunk a room for its shuffled bytes in the
 * object's scratch - identity and NO_SHUFFLE chunks too, copied there as element
 * size 1: the piece pipeline compresses from ONE source base - and cuts the
 * rooms into the writers' shared pieces (write_pieces_plan.h).
 */
#ifndef LDA_SHUFFLE_PLAN_H
#define LDA_SHUFFLE_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "chunk_plan.h"

namespace lda {

enum {
	SHUF_WORDS = 6,		/* LIBDEFLATE_AMD_SHUF_WORDS */
	SHUF_ELEM_MAX = 256,	/* LIBDEFLATE_AMD_SHUF_ELEM_MAX */
	SHUF_NO_DEFLATE = 1,	/* LIBDEFLATE_AMD_SHUF_NO_DEFLATE */
	SHUF_NO_SHUFFLE = 2,	/* LIBDEFLATE_AMD_SHUF_NO_SHUFFLE */
	SHUF_RESULT_WORDS = 4,	/* LIBDEFLATE_AMD_SHUFW_RESULT_WORDS */
	SHUF_TILE = 4096,	/* LDA_SHUF_TILE: elements of a tile, es 1, 2, 4, 8 */
	SHUF_GEN_BYTES = 16384,	/* LDA_SHUF_GEN_BYTES: about the bytes of a tile, any other es */
	/* a row's words */
	SHUF_W_STORED_OFF = 0, SHUF_W_STORED_N, SHUF_W_RAW_OFF, SHUF_W_RAW_N, SHUF_W_ES, SHUF_W_MASK,
	/* the transpose kernels' columns, n_u words each */
	SHUF_U_TILE_END = 0,	/* the tiles of this row and all before it */
	SHUF_U_SRC,		/* where the kernel reads, SHUF_SRC_ALT: from the second base */
	SHUF_U_DST,
	SHUF_U_GEOM,		/* the raw size | es << 32 */
	SHUF_UCOLS,
	/* the writer's per-chunk columns, n words each, behind CHUNKW_E_USIZE */
	SHUFW_E_ES = CHUNKW_E_USIZE + 1, SHUFW_E_MASK, SHUFW_E_RAW_OFF,
	SHUFW_ECOLS
};
#define SHUF_MAX_CHUNKS ((uint64_t)1 << 28)
#define SHUF_SRC_ALT ((uint64_t)1 << 63)	/* LDA_SHUF_SRC_ALT */
#define SHUF_VERD_OWN ((uint64_t)1 << 63)	/* LDA_SHUF_VERD_OWN: the low bits are the verdict */

/* is es one of the sizes the kernels transpose in registers? */
static inline bool shuf_reg_es(uint64_t es) { return es == 1 || es == 2 || es == 4 || es == 8; }

/* the elements of a tile: a multiple of 16, at least 64 */
static inline uint64_t shuf_tile_elems(uint64_t es)
{
	return shuf_reg_es(es) ? SHUF_TILE : (SHUF_GEN_BYTES / es) & ~(uint64_t)15;
}

/* is the transform of n bytes the identity? */
static inline bool shuf_identity(uint64_t n, uint64_t es, uint64_t mask)
{
	return es == 1 || n / es <= 1 || (mask & SHUF_NO_SHUFFLE) != 0;
}

/* the tiles of n bytes the kernels take as elements of es bytes */
static inline uint64_t shuf_tiles(uint64_t n, uint64_t es)
{
	const uint64_t T = shuf_tile_elems(es);
	return (n / es + T - 1) / T;
}

/* the most bytes one piece of a compress launch may have (the kernels'
 * positions are 32 bits wide); only a level-0 chunk is ever that long in one
 * piece, and libdeflate_<format>_compress() returns 0 for it */
#define SHUF_PIECE_MAX 0xFFFFFF00ull

/* what either call refuses in row r, or NULL.  reader: the stored range and
 * NO_DEFLATE count; raw_avail: out_avail of the reader, in_avail of the writer;
 * level: the writer's */
static inline const char *
shuf_row_why(const uint64_t *row, bool reader, uint64_t stored_avail, uint64_t raw_avail, int level)
{
	if (row[SHUF_W_ES] == 0 || row[SHUF_W_ES] > SHUF_ELEM_MAX)
		return "an element size outside 1 .. 256";
	if (row[SHUF_W_MASK] & ~(uint64_t)(reader ? SHUF_NO_DEFLATE | SHUF_NO_SHUFFLE : SHUF_NO_SHUFFLE))
		return "unknown mask bits";
	if (row[SHUF_W_RAW_N] > 0xFFFFFFFFull)
		return "a raw size of 2^32 bytes or more";
	if (reader && (row[SHUF_W_STORED_OFF] > stored_avail ||
		       stored_avail - row[SHUF_W_STORED_OFF] < row[SHUF_W_STORED_N]))
		return "its stored bytes do not lie inside in_nbytes";
	if (row[SHUF_W_RAW_OFF] > raw_avail || raw_avail - row[SHUF_W_RAW_OFF] < row[SHUF_W_RAW_N])
		return reader ? "its room does not lie inside out_avail" :
				"its raw bytes do not lie inside in_avail";
	if (!reader && level == 0 && row[SHUF_W_RAW_N] > SHUF_PIECE_MAX)
		return "a level-0 chunk above 0xFFFFFF00 bytes, which no compress call takes";
	return NULL;
}

/* true, or false with the reason in err: pointers apart, what a call refuses
 * before any device work */
static inline bool
shuf_check(int format, uint64_t n, const uint64_t *rows, bool reader, uint64_t stored_avail,
	   uint64_t raw_avail, int level, std::string &err)
{
	if (format < 0 || format > 2) {
		err = "unknown format " + std::to_string(format);
		return false;
	}
	return chunk_check("n_chunks", n, SHUF_MAX_CHUNKS, [&](uint64_t r) {
		return shuf_row_why(rows + SHUF_WORDS * r, reader, stored_avail, raw_avail, level);
	}, err);
}

/* the sum of the streams' bounds; 0 for rows the writer refuses */
static inline uint64_t shuf_bound(int format, uint64_t n, const uint64_t *rows)
{
	if (format < 0 || format > 2)
		return 0;
	return chunk_bound(n, SHUF_MAX_CHUNKS, [&](uint64_t r) {
		return shuf_row_why(rows + SHUF_WORDS * r, false, 0, ~(uint64_t)0, -1);
	}, [&](uint64_t r) { return chunk_stream_bound(format, rows[SHUF_WORDS * r + SHUF_W_RAW_N]); });
}

/* the kernels' rows: one call per row in order, then chunk_append() */
struct shuf_kernel_rows {
	uint64_t n_u = 0, tiles = 0;
	std::vector<uint64_t> col[SHUF_UCOLS];

	void add(uint64_t s, uint64_t d, uint64_t n, uint64_t es)
	{
		tiles += shuf_tiles(n, es);
		col[SHUF_U_TILE_END].push_back(tiles);
		col[SHUF_U_SRC].push_back(s);
		col[SHUF_U_DST].push_back(d);
		col[SHUF_U_GEOM].push_back(n | es << 32);
		n_u++;
	}
};

struct shuf_read_plan {
	uint64_t n;
	uint64_t n_sd;		/* deflated, shuffled: decoded into the scratch */
	uint64_t n_id;		/* deflated, identity: decoded into d_out */
	uint64_t n_u, tiles;	/* the unshuffle kernel's rows and tiles */
	uint64_t scratch;	/* bytes of the scratch rooms */
	/* what goes up: [CHUNK_DCOLS x (n_sd + n_id)] at 0, [SHUF_UCOLS x n_u] at
	 * u_at, [n verdict words] at verd_at */
	uint64_t u_at, verd_at;
	std::vector<uint64_t> cols;
};

/* the rows have passed shuf_check() */
static inline void shuf_read_plan_build(uint64_t n, const uint64_t *rows, shuf_read_plan &p)
{
	p.n = n;
	p.n_sd = p.n_id = 0;
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows + SHUF_WORDS * r;
		if (w[SHUF_W_MASK] & SHUF_NO_DEFLATE)
			continue;
		if (shuf_identity(w[SHUF_W_RAW_N], w[SHUF_W_ES], w[SHUF_W_MASK]))
			p.n_id++;
		else
			p.n_sd++;
	}
	std::vector<uint64_t> verd((size_t)n);
	chunk_decode_cols d(p.cols, p.n_sd, p.n_id);
	chunk_rooms rooms;
	shuf_kernel_rows u;
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows + SHUF_WORDS * r;
		const uint64_t raw = w[SHUF_W_RAW_N], es = w[SHUF_W_ES];
		const bool ident = shuf_identity(raw, es, w[SHUF_W_MASK]);
		if (w[SHUF_W_MASK] & SHUF_NO_DEFLATE) {
			/* the stored bytes are the shuffled bytes: 0 SUCCESS, 1 BAD_DATA */
			verd[(size_t)r] = SHUF_VERD_OWN | (w[SHUF_W_STORED_N] != raw);
			if (w[SHUF_W_STORED_N] == raw && raw)
				u.add(w[SHUF_W_STORED_OFF] | SHUF_SRC_ALT, w[SHUF_W_RAW_OFF], raw,
				      ident ? 1 : es);
		} else if (ident) {
			verd[(size_t)r] = d.add(true, w[SHUF_W_STORED_OFF], w[SHUF_W_STORED_N],
						w[SHUF_W_RAW_OFF], raw);
		} else {
			const uint64_t room = rooms.take(raw);
			verd[(size_t)r] = d.add(false, w[SHUF_W_STORED_OFF], w[SHUF_W_STORED_N], room, raw);
			u.add(room, w[SHUF_W_RAW_OFF], raw, es);
		}
	}
	p.n_u = u.n_u;
	p.tiles = u.tiles;
	p.scratch = rooms.bytes;
	p.u_at = chunk_append(p.cols, u.col, SHUF_UCOLS);
	p.verd_at = chunk_append(p.cols, &verd);
}

struct shuf_write_plan : chunk_write_plan {
	uint64_t n_u, tiles;	/* the shuffle kernel's rows and tiles */
	/* ecols: [SHUFW_ECOLS x n][SHUF_UCOLS x n_u] */
};

/* the rows have passed shuf_check(); pr.store is false whatever the level */
static inline void
shuf_write_plan_build(const zipw_params &pr, uint64_t n, const uint64_t *rows, shuf_write_plan &p)
{
	chunk_write_rows e(p, n, SHUFW_ECOLS);
	shuf_kernel_rows u;

	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = rows + SHUF_WORDS * k;
		const uint64_t raw = w[SHUF_W_RAW_N], es = w[SHUF_W_ES];
		const uint64_t room = e.add(raw, raw);
		if (raw)
			u.add(w[SHUF_W_RAW_OFF], room, raw, shuf_identity(raw, es, w[SHUF_W_MASK]) ? 1 : es);
		p.ecols[(size_t)(SHUFW_E_ES * n + k)] = es;
		p.ecols[(size_t)(SHUFW_E_MASK * n + k)] = w[SHUF_W_MASK];
		p.ecols[(size_t)(SHUFW_E_RAW_OFF * n + k)] = w[SHUF_W_RAW_OFF];
	}
	p.n_u = u.n_u;
	p.tiles = u.tiles;
	e.cut(pr);
	chunk_append(p.ecols, u.col, SHUF_UCOLS);
}

} /* namespace lda */

#endif /* LDA_SHUFFLE_PLAN_H */
