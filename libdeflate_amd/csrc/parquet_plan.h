/*
 * parquet_plan.h - the host arithmetic of reading the pages of flat Parquet
 * column chunks (include/libdeflate_amd.h: libdeflate_amd_parquet_decode_batch,
 * host_parquet.hip): the refusals made before any device work, the class of
 * every row, the rooms, the decode batch's columns, the run-list capacities and
 * the expand kernel's tile table.  Free of HIP: tools/test_parquet_plan.cpp runs
 * it on the CPU.
 *
 * A row is a page.  Its *section* is what may be a gzip member: the whole body
 * of a V1 data page or a dictionary page, the values behind the levels of a V2
 * data page.  A compressed section is inflated into a room of the object's
 * scratch (16-byte aligned, its uncompressed size); an uncompressed one, and
 * the levels of a V2 page, are read where they lie in d_in.
 *
 * Every data page becomes a row of the PQ_UCOLS columns, in the order of the
 * call.  lda_pq_runs_kernel walks its hybrid streams - definition levels, then
 * dictionary indices - a wave a page, and lists the runs as records of 16 bytes
 * in the run area: PQ_U_LRUNS / PQ_U_IRUNS are where the page's two lists start
 * (in records) and PQ_U_LCAP / PQ_U_ICAP what they hold at most.  A run of R
 * values takes at least one byte, so a stream of b bytes that owes N values has
 * at most min(N, b) runs; a bit-packed run of levels is recorded in pieces of
 * PQ_LEVEL_PIECE values, each with the count of valid slots in front, which
 * adds at most N / PQ_LEVEL_PIECE records.
 *
 * lda_pq_expand_kernel is tiled over the slots of all data pages laid end to
 * end: tile t holds the slots [t * PQ_TILE, (t + 1) * PQ_TILE) of that
 * sequence, PQ_U_SLOT_END is its prefix column, and a tile may span any number
 * of pages.
 */
#ifndef LDA_PARQUET_PLAN_H
#define LDA_PARQUET_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "chunk_plan.h"

namespace lda {

enum {
	PQ_WORDS = 8,		/* LIBDEFLATE_AMD_PARQUET_WORDS */
	PQ_TILE = 1024,		/* LDA_PQ_TILE: slots of an expand tile, 256 threads x 4 */
	PQ_LEVEL_PIECE = 512,	/* LDA_PQ_LEVEL_PIECE: values of a piece of a bit-packed level run */
	PQ_RUN_WORDS = 4,	/* LDA_PQ_RUN_WORDS: uint32_t of a run record */
	PQ_INFO_WORDS = 8,	/* LDA_PQ_INFO_WORDS: uint32_t the walk leaves per data page */
	PQ_WIDTH_MAX = 256,
	/* a row's words */
	PQ_W_OFF = 0, PQ_W_CSIZE, PQ_W_USIZE, PQ_W_FIELDS, PQ_W_COUNT, PQ_W_OUT, PQ_W_VALID, PQ_W_DICT,
	/* the kinds and encodings */
	PQ_DATA_V1 = 0, PQ_DICT = 2, PQ_DATA_V2 = 3,
	PQ_PLAIN = 0, PQ_PLAIN_DICTIONARY = 2, PQ_RLE_DICTIONARY = 8,
	/* the data pages' columns, n_u words each */
	PQ_U_SLOT_END = 0,	/* the slots of this page and all before it */
	PQ_U_SEC,		/* the section: in the rooms, or PQ_IN_PLACE | its offset in d_in */
	PQ_U_SEC_N,		/* its uncompressed bytes */
	PQ_U_LEV,		/* V2: the definition levels in d_in */
	PQ_U_LEV_N,
	PQ_U_FIELDS,		/* word 3 | PQ_F_SKIP | (1 + its place in the decode batch, or 0) << 32 */
	PQ_U_COUNT,		/* the slots */
	PQ_U_OUT, PQ_U_VALID,	/* words 5 and 6 */
	PQ_U_DICT,		/* the dictionary's section, as PQ_U_SEC */
	PQ_U_DICT_N,		/* its entries */
	PQ_U_LRUNS, PQ_U_LCAP, PQ_U_IRUNS, PQ_U_ICAP,
	PQ_UCOLS,
	/* the verdict columns, n words each */
	PQ_V_Z = 0,		/* 1 + the row's place in the decode batch, or 0 */
	PQ_V_OWN,		/* a dictionary page: PQ_V_IS_DICT | its own verdict; a data page: its place among the data pages */
	PQ_V_DICT,		/* a dictionary-coded data page: 1 + its dictionary's row, else 0 */
	PQ_VCOLS
};
#define PQ_MAX_PAGES ((uint64_t)1 << 28)
#define PQ_IN_PLACE ((uint64_t)1 << 63)	/* LDA_PQ_IN_PLACE */
#define PQ_F_SKIP ((uint64_t)1 << 31)		/* LDA_PQ_F_SKIP: the dictionary is too short for its entries */
#define PQ_V_IS_DICT ((uint64_t)1 << 63)	/* LDA_PQ_V_IS_DICT */
#define PQ_SIZE_MAX 0x7FFFFFFFull		/* Parquet's sizes and counts are int32 */

/* a row taken apart */
struct pq_page {
	uint64_t off, csize, usize, kind, enc, compressed, max_def, width, count, def_len;
	bool data, dict_coded;
};

static inline pq_page pq_page_of(const uint64_t *r)
{
	pq_page s;
	s.off = r[PQ_W_OFF], s.csize = r[PQ_W_CSIZE], s.usize = r[PQ_W_USIZE];
	s.kind = r[PQ_W_FIELDS] & 15;
	s.enc = r[PQ_W_FIELDS] >> 4 & 255;
	s.compressed = r[PQ_W_FIELDS] >> 12 & 1;
	s.max_def = r[PQ_W_FIELDS] >> 13 & 1;
	s.width = (r[PQ_W_FIELDS] >> 16 & 255) + 1;
	s.count = r[PQ_W_COUNT] & 0xFFFFFFFFull;
	s.def_len = r[PQ_W_COUNT] >> 32;
	s.data = s.kind != PQ_DICT;
	s.dict_coded = s.data && s.enc != PQ_PLAIN;
	return s;
}

/* what the call refuses in row r of rows, or NULL */
static inline const char *
pq_row_why(const uint64_t *rows, uint64_t r, uint64_t in_nbytes, uint64_t out_avail,
	   uint64_t valid_avail, bool have_valid)
{
	const uint64_t *row = rows + PQ_WORDS * r;
	const pq_page s = pq_page_of(row);

	if (row[PQ_W_FIELDS] >> 24 || (row[PQ_W_FIELDS] >> 14 & 3))
		return "unknown bits in word 3";
	if (s.kind != PQ_DATA_V1 && s.kind != PQ_DICT && s.kind != PQ_DATA_V2)
		return "a kind that is not 0, 2 or 3";
	if (s.enc != PQ_PLAIN && s.enc != PQ_PLAIN_DICTIONARY && s.enc != PQ_RLE_DICTIONARY)
		return "an encoding that is not 0, 2 or 8";
	if (!s.data && s.enc != PQ_PLAIN)
		return "a dictionary encoding on a dictionary page";
	if (!s.data && s.max_def)
		return "max_def on a dictionary page";
	if (s.csize > PQ_SIZE_MAX || s.usize > PQ_SIZE_MAX || s.count > PQ_SIZE_MAX)
		return "a size or count of 2^31 or more";
	if (s.def_len && (s.kind != PQ_DATA_V2 || !s.max_def))
		return "level bytes on a row that is not a V2 data page with max_def 1";
	if (s.def_len > s.csize || s.def_len > s.usize)
		return "V2 level bytes beyond the page's sizes";
	if (!s.compressed && s.csize != s.usize)
		return "an uncompressed body whose two sizes differ";
	if (s.off > in_nbytes || in_nbytes - s.off < s.csize)
		return "its body does not lie inside in_nbytes";
	if (!s.data)
		return NULL;
	if (s.dict_coded) {
		const uint64_t d = row[PQ_W_DICT];
		if (d >= r)
			return "its dictionary is not an earlier row";
		const pq_page t = pq_page_of(rows + PQ_WORDS * d);
		if (t.data)
			return "its dictionary row is not a dictionary page";
		if (t.width != s.width)
			return "its dictionary has another width";
	}
	/* count * width < 2^39 */
	if (row[PQ_W_OUT] > out_avail || out_avail - row[PQ_W_OUT] < s.count * s.width)
		return "its slots do not lie inside out_avail";
	if (s.max_def) {
		if (!have_valid)
			return "max_def 1 and d_valid is NULL";
		if (row[PQ_W_VALID] > valid_avail || valid_avail - row[PQ_W_VALID] < s.count)
			return "its validity bytes do not lie inside valid_avail";
	}
	return NULL;
}

/* true, or false with the reason in err: pointers apart, what the call refuses
 * before any device work */
static inline bool
pq_check(int format, uint64_t n, const uint64_t *rows, uint64_t in_nbytes, uint64_t out_avail,
	 uint64_t valid_avail, bool have_valid, std::string &err)
{
	if (format < 0 || format > 2) {
		err = "format " + std::to_string(format) + " is not DEFLATE, ZLIB or GZIP";
		return false;
	}
	return chunk_check("n_pages", n, PQ_MAX_PAGES, [&](uint64_t r) {
		return pq_row_why(rows, r, in_nbytes, out_avail, valid_avail, have_valid);
	}, err);
}

/* the most records of the two run lists of a data page */
static inline uint64_t pq_level_cap(const pq_page &s)
{
	if (!s.max_def)
		return 0;
	const uint64_t bytes = s.kind == PQ_DATA_V2 ? s.def_len : s.usize;
	return (s.count < bytes ? s.count : bytes) + s.count / PQ_LEVEL_PIECE + 1;
}

static inline uint64_t pq_index_cap(const pq_page &s)
{
	if (!s.dict_coded)
		return 0;
	const uint64_t bytes = s.usize - s.def_len;
	return (s.count < bytes ? s.count : bytes) + 1;
}

struct pq_plan {
	uint64_t n;
	uint64_t n_z;		/* compressed sections */
	uint64_t n_u;		/* data pages */
	uint64_t slots, tiles;	/* of all data pages */
	uint64_t room_bytes;	/* the area of the rooms */
	uint64_t run_records;	/* the run area */
	/* what goes up: [CHUNK_DCOLS x n_z] at 0, [PQ_UCOLS x n_u] at u_at, [PQ_VCOLS x n]
	 * at v_at */
	uint64_t u_at, v_at;
	std::vector<uint64_t> cols;
};

/* the rows have passed pq_check() */
static inline void pq_plan_build(uint64_t n, const uint64_t *rows, pq_plan &p)
{
	std::vector<uint64_t> u[PQ_UCOLS], v[PQ_VCOLS];
	std::vector<uint64_t> sec((size_t)n);	/* every row's section, as PQ_U_SEC */
	chunk_rooms rooms;

	p.n = n;
	p.n_z = p.slots = p.run_records = 0;
	for (uint64_t r = 0; r < n; r++)
		p.n_z += pq_page_of(rows + PQ_WORDS * r).compressed;
	chunk_decode_cols d(p.cols, p.n_z);
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t *w = rows + PQ_WORDS * r;
		const pq_page s = pq_page_of(w);
		uint64_t z = 0;

		if (s.compressed) {
			sec[(size_t)r] = rooms.take(s.usize - s.def_len);
			z = 1 + d.add(false, s.off + s.def_len, s.csize - s.def_len, sec[(size_t)r],
				      s.usize - s.def_len);
		} else {
			sec[(size_t)r] = PQ_IN_PLACE | (s.off + s.def_len);
		}
		v[PQ_V_Z].push_back(z);
		if (!s.data) {
			v[PQ_V_OWN].push_back(PQ_V_IS_DICT | (s.count * s.width > s.usize ? 1 : 0));
			v[PQ_V_DICT].push_back(0);
			continue;
		}
		v[PQ_V_OWN].push_back(u[0].size());
		v[PQ_V_DICT].push_back(s.dict_coded ? w[PQ_W_DICT] + 1 : 0);
		uint64_t fields = (w[PQ_W_FIELDS] & 0xFFFFFF) | z << 32, dict = 0, dict_n = 0;
		if (s.dict_coded) {
			const pq_page t = pq_page_of(rows + PQ_WORDS * w[PQ_W_DICT]);
			dict = sec[(size_t)w[PQ_W_DICT]];
			dict_n = t.count;
			if (t.count * t.width > t.usize)
				fields |= PQ_F_SKIP;
		}
		p.slots += s.count;
		u[PQ_U_SLOT_END].push_back(p.slots);
		u[PQ_U_SEC].push_back(sec[(size_t)r]);
		u[PQ_U_SEC_N].push_back(s.usize - s.def_len);
		u[PQ_U_LEV].push_back(s.off);
		u[PQ_U_LEV_N].push_back(s.def_len);
		u[PQ_U_FIELDS].push_back(fields);
		u[PQ_U_COUNT].push_back(s.count);
		u[PQ_U_OUT].push_back(w[PQ_W_OUT]);
		u[PQ_U_VALID].push_back(w[PQ_W_VALID]);
		u[PQ_U_DICT].push_back(dict);
		u[PQ_U_DICT_N].push_back(dict_n);
		u[PQ_U_LRUNS].push_back(p.run_records);
		u[PQ_U_LCAP].push_back(pq_level_cap(s));
		p.run_records += pq_level_cap(s);
		u[PQ_U_IRUNS].push_back(p.run_records);
		u[PQ_U_ICAP].push_back(pq_index_cap(s));
		p.run_records += pq_index_cap(s);
	}
	p.n_u = u[0].size();
	p.tiles = (p.slots + PQ_TILE - 1) / PQ_TILE;
	p.room_bytes = rooms.bytes;
	p.u_at = chunk_append(p.cols, u, PQ_UCOLS);
	p.v_at = chunk_append(p.cols, v, PQ_VCOLS);
}

} /* namespace lda */

#endif /* LDA_PARQUET_PLAN_H */
