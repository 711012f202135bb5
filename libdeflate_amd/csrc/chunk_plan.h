/*
 * chunk_plan.h - what the plans of the chunk codecs share: the byte-shuffled
 * chunks, TIFF strips and tiles, OpenEXR chunks and Parquet pages
 * (shuffle_plan.h, tiff_plan.h, exr_plan.h, parquet_plan.h).  A reader checks
 * host rows, classifies them into columns that go up in one copy, inflates the
 * compressed rows into rooms of the object's scratch or straight into d_out,
 * runs the format's kernels and leaves one verdict word per row; a writer gives
 * every row a room, which the format's kernels fill, and cuts the rooms into the
 * writers' shared pieces (write_pieces_plan.h).  A format adds its row's reason
 * (`*_row_why`), its classes and its kernels' columns.  Free of HIP.
 */
#ifndef LDA_CHUNK_PLAN_H
#define LDA_CHUNK_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "write_pieces_plan.h"

namespace lda {

enum {
	/* the decode batches' columns, n_dec words each */
	CHUNK_D_IN_OFF = 0, CHUNK_D_IN_N, CHUNK_D_OUT_OFF, CHUNK_D_OUT_N, CHUNK_DCOLS,
	/* the first of a writer's per-row columns, n words each: what
	 * lda_shufw_chunk_kernel and lda_shufw_place_kernel read */
	CHUNKW_E_FIRST = 0, CHUNKW_E_COUNT, CHUNKW_E_USIZE
};

static inline uint64_t chunk_align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

/* libdeflate_<format>_compress_bound(len): 5 bytes per 5000-byte block, and
 * what stands around a zlib (1) or gzip (2) stream */
static inline uint64_t chunk_stream_bound(int format, uint64_t len)
{
	uint64_t blocks = (len + 4999) / 5000;
	if (blocks < 1)
		blocks = 1;
	return 5 * blocks + len + (format == 1 ? 6 : format == 2 ? 18 : 0);
}

/* true, or false with the reason in err: the count of rows (`noun` names it)
 * against max, then row_why(r) -> the reason row r is refused for, or NULL */
template <typename RowWhy>
static inline bool
chunk_check(const char *noun, uint64_t n, uint64_t max, RowWhy row_why, std::string &err)
{
	char msg[200];

	if (n > max) {
		snprintf(msg, sizeof(msg), "%s %llu above 2^28", noun, (unsigned long long)n);
		err = msg;
		return false;
	}
	for (uint64_t r = 0; r < n; r++) {
		const char *why = row_why(r);
		if (why) {
			snprintf(msg, sizeof(msg), "row %llu: %s", (unsigned long long)r, why);
			err = msg;
			return false;
		}
	}
	return true;
}

/* the sum of bound(r) over the rows; 0 for more rows than max and for rows the
 * writer refuses (row_why as above) */
template <typename RowWhy, typename RowBound>
static inline uint64_t chunk_bound(uint64_t n, uint64_t max, RowWhy row_why, RowBound bound)
{
	uint64_t sum = 0;
	if (n > max)
		return 0;
	for (uint64_t r = 0; r < n; r++) {
		if (row_why(r))
			return 0;
		sum += bound(r);
	}
	return sum;
}

/* rooms back to back in an area of the object's scratch, at 16-byte boundaries */
struct chunk_rooms {
	uint64_t bytes = 0;	/* the area so far */

	uint64_t take(uint64_t n)
	{
		const uint64_t at = bytes;
		bytes += chunk_align16(n);
		return at;
	}
};

/* n_cols columns of one length, as they stand in col[], behind what cols
 * holds; -> where the group starts */
static inline uint64_t
chunk_append(std::vector<uint64_t> &cols, const std::vector<uint64_t> *col, size_t n_cols = 1)
{
	const uint64_t at = cols.size();
	for (size_t a = 0; a < n_cols; a++)
		cols.insert(cols.end(), col[a].begin(), col[a].end());
	return at;
}

/*
 * The decode batches' columns: [CHUNK_DCOLS x n_dec], the rows decoded into the
 * scratch first, the rows decoded into d_out behind them - one decompress batch
 * per output base.  They begin cols, in one allocation: the plan has counted
 * its n_ws scratch rows and n_out d_out rows (a plan that decodes into the
 * scratch alone: 0), and appends its other groups once every row is added.
 */
struct chunk_decode_cols {
	std::vector<uint64_t> &cols;
	const uint64_t n_dec;
	uint64_t ws = 0, out;	/* the next place of either kind */

	chunk_decode_cols(std::vector<uint64_t> &cols, uint64_t n_ws, uint64_t n_out = 0)
		: cols(cols), n_dec(n_ws + n_out), out(n_ws)
	{
		cols.assign((size_t)(CHUNK_DCOLS * n_dec), 0);
	}
	/* -> the row's place in the columns and in the decoder's results: its
	 * verdict word */
	uint64_t add(bool to_out, uint64_t in_off, uint64_t in_n, uint64_t out_off, uint64_t out_n)
	{
		const uint64_t at = to_out ? out++ : ws++;
		cols[(size_t)(CHUNK_D_IN_OFF * n_dec + at)] = in_off;
		cols[(size_t)(CHUNK_D_IN_N * n_dec + at)] = in_n;
		cols[(size_t)(CHUNK_D_OUT_OFF * n_dec + at)] = out_off;
		cols[(size_t)(CHUNK_D_OUT_N * n_dec + at)] = out_n;
		return at;
	}
};

/* a writer's plan: the pieces, and in front of them what goes up, [ECOLS x n]
 * per-row columns and the format's kernel rows behind them */
struct chunk_write_plan : zipw_pieces {
	uint64_t n, raw_total;	/* the bytes the call reads of d_in */
	uint64_t rooms_bytes;	/* the area of the rooms */
	std::vector<uint64_t> ecols;
};

/* the rows of a writer's plan, one add() per row in order, then cut() */
struct chunk_write_rows {
	chunk_write_plan &p;
	chunk_rooms rooms;
	std::vector<uint64_t> room, size;
	uint64_t k = 0;

	chunk_write_rows(chunk_write_plan &p, uint64_t n, size_t ecols) : p(p), room((size_t)n), size((size_t)n)
	{
		p.n = n;
		p.raw_total = 0;
		p.ecols.assign(ecols * (size_t)n, 0);
	}
	/* row k: a room of `bytes` that the pieces are cut from, `raw` bytes read;
	 * -> the room */
	uint64_t add(uint64_t bytes, uint64_t raw)
	{
		room[(size_t)k] = rooms.take(bytes);
		size[(size_t)k] = bytes;
		p.ecols[(size_t)(CHUNKW_E_USIZE * p.n + k)] = bytes;
		p.raw_total += raw;
		return room[(size_t)k++];
	}
	/* the rooms into pieces: columns CHUNKW_E_FIRST and CHUNKW_E_COUNT */
	void cut(const zipw_params &pr)
	{
		p.rooms_bytes = rooms.bytes;
		zipw_cut_pieces(pr, p.n, room.data(), size.data(), p.ecols.data() + CHUNKW_E_FIRST * p.n,
				p.ecols.data() + CHUNKW_E_COUNT * p.n, p);
	}
};

} /* namespace lda */

#endif /* LDA_CHUNK_PLAN_H */
