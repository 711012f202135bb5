/*
 * stored_rows.h - the walk over a RUN OF STORED BLOCKS (host_stream.hip,
 * walk_stored()), written once for the two things it can read: the stream's
 * bytes in host memory, or the rows lda_stream_find_stored_kernel made of a
 * stream that lies in device memory (stream_probe_kernels.hip).
 *
 * Host only and free of HIP: tools/test_stored_rows.cpp compiles it with the
 * host compiler under the sanitizers.
 */
#ifndef LDA_STORED_ROWS_H
#define LDA_STORED_ROWS_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

/*
 * One byte offset bp of the raw stream at which LEN == ~NLEN, where
 * LEN = bytes bp, bp + 1 and NLEN = bytes bp + 2, bp + 3 (little-endian) and
 * bp + 4 is not past the bytes searched.  `front` holds the two bytes in front
 * of bp (byte bp - 2 in its bits 0..7, byte bp - 1 in bits 8..15; zero where
 * they lie before the stream): the three header bits of a stored block whose
 * LEN is at bp start at bit q with (q + 10) >> 3 == bp, that is in
 * [8 bp - 10, 8 bp - 3], which is bit q - 8 bp + 16 of `front`.
 */
struct lda_stored_row {
	uint64_t bp;
	uint32_t len;
	uint32_t front;
};

namespace lda {

/*
 * Is there a stored block whose header starts at bit q?  bp = (q + 10) >> 3 is
 * where its LEN lies.  Both probes say yes only when the block type is 0,
 * bp + 4 is inside the stream and LEN == ~NLEN; then *h gets the three header
 * bits and *len LEN (lib/decompress_template.h:247-285).
 */
struct stored_probe_bytes {
	const uint8_t *raw;
	uint64_t raw_n;

	uint32_t peek(uint64_t bit, unsigned n) const	/* n <= 24; zeros past the end */
	{
		uint32_t v = 0;
		const uint64_t b0 = bit >> 3;
		if (b0 + 4 <= raw_n)
			memcpy(&v, raw + b0, 4);	/* (little-endian host, as the HIP runtime's) */
		else
			for (unsigned k = 0; k < 4; k++)
				if (b0 + k < raw_n)
					v |= (uint32_t)raw[b0 + k] << (8 * k);
		return (v >> (bit & 7)) & ((1u << n) - 1);
	}
	bool operator()(uint64_t q, uint64_t bp, uint32_t *h, uint32_t *len) const
	{
		*h = peek(q, 3);
		if ((*h >> 1) != 0)
			return false;
		if (bp + 4 > raw_n)
			return false;
		*len = raw[bp] | ((uint32_t)raw[bp + 1] << 8);
		const uint32_t nlen = raw[bp + 2] | ((uint32_t)raw[bp + 3] << 8);
		return *len == (nlen ^ 0xFFFFu);
	}
};

/* rows sorted by bp (sort_stored_rows()).  A missing row means "not a stored
 * block here": rows a full queue lost only end a walk early. */
struct stored_probe_rows {
	const lda_stored_row *rows;
	size_t n;

	bool operator()(uint64_t q, uint64_t bp, uint32_t *h, uint32_t *len) const
	{
		const lda_stored_row *e = rows + n;
		const lda_stored_row *r = std::lower_bound(
			rows, e, bp, [](const lda_stored_row &a, uint64_t v) { return a.bp < v; });
		if (r == e || r->bp != bp)
			return false;
		*h = (r->front >> (q + 16 - 8 * bp)) & 7;
		if ((*h >> 1) != 0)
			return false;
		*len = r->len;
		return true;
	}
};

static inline void sort_stored_rows(lda_stored_row *rows, size_t n)
{
	std::sort(rows, rows + n,
		  [](const lda_stored_row &a, const lda_stored_row &b) { return a.bp < b.bp; });
}

/*
 * The run of stored blocks from the block boundary `p` (a bit offset) on.
 * Every stored block - several small ones together, up to `group` bits of
 * input - is handed to emit(first bit, bit behind the last block, bytes of
 * output, the last block was BFINAL).  Stops in front of the first block that
 * is not stored, is not wholly inside the first `dev_bytes` bytes of the
 * stream (or inside its raw_n bytes), or is invalid.  Returns the bit it
 * stopped at; *fin_ret: that was the end of the stream's final block.
 */
template <typename Probe, typename Emit>
static inline uint64_t walk_stored_run(uint64_t p, uint64_t raw_n, uint64_t dev_bytes,
				       uint64_t group, const Probe &probe, Emit emit,
				       bool *fin_ret)
{
	const uint64_t raw_bits = 8 * raw_n;
	*fin_ret = false;
	for (;;) {
		uint64_t q = p, nout = 0;
		bool fin = false;
		while (q + 3 <= raw_bits && !fin && q - p < group) {
			const uint64_t bp = (q + 3 + 7) >> 3;
			uint32_t h = 0, len = 0;
			if (!probe(q, bp, &h, &len))
				break;
			if (bp + 4 + len > raw_n || bp + 4 + len > dev_bytes)
				break;
			nout += len;
			q = 8 * (bp + 4 + len);
			fin = h & 1;
		}
		if (q == p)
			return p;
		emit(p, q, nout, fin);
		p = q;
		if (fin) {
			*fin_ret = true;
			return p;
		}
	}
}

} /* namespace lda */

#endif /* LDA_STORED_ROWS_H */
