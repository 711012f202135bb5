/*
 * seek_plan.h - the host arithmetic of the seek index over ONE plain DEFLATE /
 * zlib / gzip stream (host_seek.hip): which chunks of the many-wave decoder's
 * accepted chain become points, the index's rows and their checks, and the
 * tables of a ranged read (range -> interval -> piece -> slot).  No HIP in
 * here: tools/test_seek_plan.cpp compiles it with the host compiler alone.
 *
 * THE INDEX: rows of LIBDEFLATE_AMD_SEEK_WORDS (4) u64 on the host.
 *   row 0        { LDA_SEEK_MAGIC, format, byte offset of the raw DEFLATE
 *                  stream in d_in, n = number of points }
 *   rows 1 .. n  { out_off, start_bit, hdr_bit, kind }: what a
 *                  struct lda_stream_chunk needs to decode from that point on;
 *                  bits relative to the raw stream, kind LDA_CHUNK_HEADER (0)
 *                  or LDA_CHUNK_EXACT (2)
 *   row n + 1    { total output bytes, bytes of the raw stream (up to the end
 *                  of its final block), footer bytes, LDA_SEEK_END }
 * Interval k is point k up to point k + 1 (the last: up to the total).
 */
#ifndef LDA_SEEK_PLAN_H
#define LDA_SEEK_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>

#include "stream_types.h"

namespace lda {

#define LDA_SEEK_MAGIC 0x314B45455341444Cull	/* "LDASEEK1" */
#define LDA_SEEK_END 0x21444E454B454553ull	/* "SEEKEND!" */
#define LDA_SEEK_ROW 4u				/* = LIBDEFLATE_AMD_SEEK_WORDS */
#define LDA_SEEK_WIN 32768u			/* = LIBDEFLATE_AMD_SEEK_WINDOW */
/* the first slot of the symbol scratch: copy_syms::in_front() takes absolute
 * positions below 65536 for the start of a stream, far_base() reads 32768
 * symbols in front of a position */
#define LDA_SEEK_SLOT0 65536u
#define LDA_SEEK_MAX_POINTS ((uint64_t)1 << 26)

/* one chunk of the accepted chain, in stream order, starts exact */
struct seek_link {
	uint64_t out_off, start_bit, hdr_bit;
	uint32_t kind;
};

/* what the decode leaves for the index */
struct seek_export {
	bool parallel = false;	/* the many-wave path answered: chain[] is its chain */
	bool known = false;	/* raw_off .. total are set */
	uint64_t raw_off = 0, raw_nbytes = 0, ftr = 0, total = 0;
	std::vector<seek_link> chain;
};

/* A chunk planned under the static codes without a header stops at its
 * block's end whatever its limit (chunk_run()): it cannot stand for an
 * interval that goes on behind that block. */
static inline bool seek_eligible(const seek_link &c)
{
	return !(c.hdr_bit == LDA_HDR_STATIC && c.kind != LDA_CHUNK_HEADER);
}

static inline size_t seek_capacity(size_t index_avail, size_t windows_avail)
{
	const size_t rows = index_avail / LDA_SEEK_ROW;
	const size_t a = rows >= 2 ? rows - 2 : 0, b = windows_avail / LDA_SEEK_WIN;
	return a < b ? a : b;
}

/*
 * The points: chain[0] always (the stream's first bit, output offset 0), then
 * greedily the first eligible chunk at least `spacing` bytes of output behind
 * the last point (and in front of the end: an empty interval reads nothing).
 * More than `capacity` points: the spacing is doubled until they fit.  Returns
 * indices into chain[]; *spacing_ret = the spacing that was used.
 */
static inline std::vector<size_t>
seek_thin(const std::vector<seek_link> &chain, uint64_t total, uint64_t spacing, size_t capacity,
	  uint64_t *spacing_ret)
{
	std::vector<size_t> pts;
	if (chain.empty() || capacity < 1 || spacing == 0)
		return pts;
	for (;;) {
		pts.clear();
		pts.push_back(0);
		uint64_t last = chain[0].out_off, last_bit = chain[0].start_bit;
		for (size_t i = 1; i < chain.size(); i++) {
			const seek_link &c = chain[i];
			if (!seek_eligible(c) || c.out_off >= total || c.out_off - last < spacing ||
			    c.out_off < last || c.start_bit <= last_bit)
				continue;
			pts.push_back(i);
			last = c.out_off;
			last_bit = c.start_bit;
			if (pts.size() > capacity)
				break;
		}
		if (pts.size() <= capacity || spacing > total)
			break;
		spacing = spacing > (~(uint64_t)0) / 2 ? ~(uint64_t)0 : spacing * 2;
	}
	if (pts.size() > capacity)
		pts.resize(capacity);	/* (spacing > total leaves point 0 alone: not reached) */
	if (spacing_ret)
		*spacing_ret = spacing;
	return pts;
}

/*
 * Points whose interval did not verify leave (failed[k] != 0: interval k):
 * point k is dropped and its interval merges into its predecessor's; point 0
 * stays, so there its successor goes.  recount[] of the survivors: the
 * intervals that changed.  Returns how many points were dropped.
 */
static inline size_t
seek_drop_failed(std::vector<seek_link> &pts, const std::vector<uint8_t> &failed,
		 std::vector<uint8_t> &recount)
{
	const size_t n = pts.size();
	std::vector<uint8_t> drop(n, 0);
	for (size_t k = 0; k < n; k++) {
		if (!failed[k])
			continue;
		if (k > 0)
			drop[k] = 1;
		else if (n > 1)
			drop[1] = 1;
	}
	std::vector<seek_link> keep;
	recount.clear();
	size_t dropped = 0;
	for (size_t k = 0; k < n; k++) {
		if (drop[k]) {
			dropped++;
			recount.back() = 1;	/* (k >= 1: point 0 is never dropped) */
			continue;
		}
		keep.push_back(pts[k]);
		recount.push_back(0);
	}
	pts.swap(keep);
	return dropped;
}

/* the rows from the points; index has room for 4 (n + 2) words */
static inline void
seek_write_index(uint64_t *index, int format, const seek_export &x, const std::vector<seek_link> &pts)
{
	const size_t n = pts.size();
	index[0] = LDA_SEEK_MAGIC;
	index[1] = (uint64_t)format;
	index[2] = x.raw_off;
	index[3] = n;
	for (size_t k = 0; k < n; k++) {
		uint64_t *r = index + LDA_SEEK_ROW * (k + 1);
		r[0] = pts[k].out_off;
		r[1] = pts[k].start_bit;
		r[2] = pts[k].hdr_bit;
		r[3] = pts[k].kind;
	}
	uint64_t *e = index + LDA_SEEK_ROW * (n + 1);
	e[0] = x.total;
	e[1] = x.raw_nbytes;
	e[2] = x.ftr;
	e[3] = LDA_SEEK_END;
}

/* a view of a checked index */
struct seek_view {
	const uint64_t *rows = nullptr;	/* row 1 */
	size_t n = 0;
	uint64_t raw_off = 0, raw_nbytes = 0, ftr = 0, total = 0;
	int format = 0;
	uint64_t out_off(size_t k) const { return k < n ? rows[LDA_SEEK_ROW * k] : total; }
	uint64_t start_bit(size_t k) const { return rows[LDA_SEEK_ROW * k + 1]; }
	uint64_t hdr_bit(size_t k) const { return rows[LDA_SEEK_ROW * k + 2]; }
	uint32_t kind(size_t k) const { return (uint32_t)rows[LDA_SEEK_ROW * k + 3]; }
};

/* "" and *v, or what is wrong with the index */
static inline std::string
seek_check_index(const uint64_t *index, size_t index_words, size_t in_nbytes, seek_view *v)
{
	char b[160];
	if (index_words < 3 * LDA_SEEK_ROW)
		return "index_words is less than the three rows of the smallest index";
	if (index[0] != LDA_SEEK_MAGIC)
		return "the index does not begin with the magic word";
	if (index[1] > 2)
		return "the index names a format that is not DEFLATE, zlib or gzip";
	const uint64_t n = index[3];
	if (n < 1 || n > LDA_SEEK_MAX_POINTS || (n + 2) * LDA_SEEK_ROW > index_words) {
		snprintf(b, sizeof(b), "the index says %llu points, index_words %zu holds %zu",
			 (unsigned long long)n, index_words, index_words / LDA_SEEK_ROW - 2);
		return b;
	}
	const uint64_t *rows = index + LDA_SEEK_ROW, *e = rows + LDA_SEEK_ROW * n;
	if (e[3] != LDA_SEEK_END)
		return "the index's closing row does not carry the end marker";
	const uint64_t raw_off = index[2], total = e[0], raw_n = e[1], ftr = e[2];
	if (ftr > 8 || raw_off > in_nbytes || raw_n > in_nbytes - raw_off ||
	    ftr > in_nbytes - raw_off - raw_n) {
		snprintf(b, sizeof(b), "the index's closing row needs %llu + %llu + %llu bytes of input, "
			 "in_nbytes is %zu", (unsigned long long)raw_off, (unsigned long long)raw_n,
			 (unsigned long long)ftr, in_nbytes);
		return b;
	}
	if (raw_n >= ((uint64_t)1 << 60))
		return "the index's raw stream is too long";
	if (rows[0] != 0 || rows[1] != 0 || rows[2] != 0 || rows[3] != LDA_CHUNK_HEADER)
		return "point 0 is not the stream's first bit at output offset 0";
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *r = rows + LDA_SEEK_ROW * k;
		const bool hdr = r[3] == LDA_CHUNK_HEADER;
		const bool state_ok = hdr ? r[2] == r[1] :
				      r[3] == LDA_CHUNK_EXACT && r[2] < r[1] && r[2] != LDA_HDR_STATIC;
		const bool rising = k == 0 || (r[0] > r[0 - (ptrdiff_t)LDA_SEEK_ROW] &&
					       r[1] > r[1 - (ptrdiff_t)LDA_SEEK_ROW]);
		if (!state_ok || !rising || r[1] >= 8 * raw_n + (k == 0) || r[0] > total ||
		    (k > 0 && r[0] >= total)) {
			snprintf(b, sizeof(b), "row %llu of the index is not a point behind row %llu "
				 "(out_off and start_bit must rise strictly, inside the stream)",
				 (unsigned long long)k + 1, (unsigned long long)k);
			return b;
		}
	}
	if (v) {
		v->rows = rows;
		v->n = (size_t)n;
		v->raw_off = raw_off;
		v->raw_nbytes = raw_n;
		v->ftr = ftr;
		v->total = total;
		v->format = (int)index[1];
	}
	return "";
}

/* a touched interval: point k, its bytes, its slot in the symbol scratch */
struct seek_interval {
	size_t k;
	uint64_t out_off, nbytes;
	uint64_t slot;		/* in 16-bit symbols from the scratch's start */
};
/* one range's share of one interval */
struct seek_piece {
	uint32_t interval;	/* index into seek_read_plan::iv */
	uint32_t range;
	uint64_t src;		/* first byte, from the interval's start */
	uint64_t dst;		/* from d_out */
	uint64_t len;
};
struct seek_read_plan {
	std::vector<seek_interval> iv;		/* ascending k, each once */
	std::vector<seek_piece> pieces;		/* range by range, in stream order */
	std::vector<uint64_t> first;		/* n_ranges + 1: pieces of range r */
	uint64_t sym_words = 0;			/* 16-bit symbols of scratch */
	uint64_t out_bytes = 0;
};

static inline uint64_t seek_slot_words(uint64_t nbytes)
{
	return (nbytes + 63) / 64 * 64 + 64;
}

/* "" and *p, or what is wrong with the ranges */
static inline std::string
seek_plan_ranges(const seek_view &v, size_t n_ranges, const uint64_t *ranges, size_t out_avail,
		 seek_read_plan *p)
{
	char b[160];
	uint64_t need = 0;
	for (size_t r = 0; r < n_ranges; r++) {
		const uint64_t at = ranges[2 * r], len = ranges[2 * r + 1];
		if (at > v.total || len > v.total - at) {
			snprintf(b, sizeof(b), "range %zu lies past the end of the data (%llu bytes)", r,
				 (unsigned long long)v.total);
			return b;
		}
		need += len;
		if (need > out_avail) {
			snprintf(b, sizeof(b), "the ranges need more than out_avail %zu bytes", out_avail);
			return b;
		}
	}
	p->iv.clear();
	p->pieces.clear();
	p->first.assign(n_ranges + 1, 0);
	p->out_bytes = need;
	/* interval of byte `at` (< total): the last point at or in front of it */
	auto interval_of = [&](uint64_t at) -> size_t {
		size_t lo = 0, hi = v.n;	/* out_off(lo) <= at < out_off(hi) */
		while (hi - lo > 1) {
			const size_t mid = lo + (hi - lo) / 2;
			if (v.out_off(mid) <= at)
				lo = mid;
			else
				hi = mid;
		}
		return lo;
	};
	std::vector<size_t> touched;
	for (size_t r = 0; r < n_ranges; r++) {
		const uint64_t at = ranges[2 * r], len = ranges[2 * r + 1];
		if (!len)
			continue;
		for (size_t k = interval_of(at); k < v.n && v.out_off(k) < at + len; k++)
			touched.push_back(k);
	}
	std::sort(touched.begin(), touched.end());
	touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
	uint64_t slot = LDA_SEEK_SLOT0;
	for (size_t k : touched) {
		seek_interval iv = { k, v.out_off(k), v.out_off(k + 1) - v.out_off(k), slot };
		slot += seek_slot_words(iv.nbytes);
		p->iv.push_back(iv);
	}
	p->sym_words = slot;
	if (p->iv.size() >= 0xFFFFFFFFull || n_ranges >= 0xFFFFFFFFull)
		return "more than 2^32 intervals or ranges";
	uint64_t outpos = 0;
	for (size_t r = 0; r < n_ranges; r++) {
		const uint64_t at = ranges[2 * r], len = ranges[2 * r + 1];
		p->first[r] = p->pieces.size();
		if (len) {
			for (size_t k = interval_of(at); k < v.n && v.out_off(k) < at + len; k++) {
				const uint64_t from = std::max(at, v.out_off(k));
				const uint64_t to = std::min(at + len, v.out_off(k + 1));
				const size_t j = (size_t)(std::lower_bound(touched.begin(), touched.end(), k) -
							  touched.begin());
				seek_piece pc = { (uint32_t)j, (uint32_t)r, from - v.out_off(k),
						  outpos + (from - at), to - from };
				p->pieces.push_back(pc);
			}
		}
		outpos += len;
	}
	p->first[n_ranges] = p->pieces.size();
	return "";
}

} /* namespace lda */

#endif /* LDA_SEEK_PLAN_H */
