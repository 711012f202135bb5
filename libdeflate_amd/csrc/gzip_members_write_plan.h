/*
 * gzip_members_write_plan.h - the host arithmetic of
 * libdeflate_amd_gzip_members_compress_batch (host_gzip_members_write.hip):
 * the argument checks, the bound, and the plan over many records - every record
 * cut into the pieces the compress and CRC-32 batches run on, the pieces'
 * slots, the per-record columns the assembly kernels
 * (gzip_members_write_kernels.hip) read.  Free of HIP:
 * tools/test_gzip_members_write_plan.cpp runs it on the CPU.
 *
 * The pieces are the writers' shared ones (write_pieces_plan.h:
 * zipw_cut_pieces(), the segment rule of large_plan.h, slots of zipw_slot(), the
 * launch groups small / whole / per segment size), so every record meets the
 * kernel, the seg_info and the size bound that libdeflate_gzip_compress() on its
 * bytes would give it.  Two things differ from the ZIP writer's use of them.
 * Nothing is ever stored in place of the compressor's
 * stream: level 0 goes through the compress kernel like every other level (its
 * stored blocks are the stream), and the slot of
 * libdeflate_deflate_compress_bound() always holds it.  And a record of 0
 * bytes, which has no piece, still has a stream - the kernels' one empty final
 * stored block, GZMW_EMPTY_STREAM bytes - that the place kernel writes.
 */
#ifndef LDA_GZIP_MEMBERS_WRITE_PLAN_H
#define LDA_GZIP_MEMBERS_WRITE_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "write_pieces_plan.h"

namespace lda {

enum {
	GZMW_RESULT_WORDS = 4,	/* LIBDEFLATE_AMD_GZMW_RESULT_WORDS */
	GZMW_HEADER_BYTES = 10,
	GZMW_FOOTER_BYTES = 8,
	GZMW_EMPTY_STREAM = 5,	/* 01 00 00 ff ff: what the compress kernels make of 0 bytes */
	GZMW_NAME_MAX = 65534,	/* with its terminator: the reader's LIBDEFLATE_AMD_GZM_NAME_MAX */
	/* the per-record columns, n words each, in the order they go up */
	GZMW_E_FIRST = 0,	/* first piece */
	GZMW_E_COUNT,		/* pieces */
	GZMW_E_NAME_OFF,	/* the name in the names' bytes */
	GZMW_E_NAME_LEN,	/* its length, 0: no FNAME field */
	GZMW_E_USIZE,
	GZMW_E_UOFF,		/* exclusive prefix sum of the usizes: the index pair's second word */
	GZMW_ECOLS
};
#define GZMW_MAX_RECORDS ((uint64_t)1 << 28)
/* the most bytes one piece of the compress launch may have (the kernels'
 * positions are 32 bits wide); only a level-0 record is ever that long in one
 * piece, and libdeflate_gzip_compress() returns 0 for it */
#define GZMW_PIECE_MAX 0xFFFFFF00ull

/* libdeflate_deflate_compress_bound() */
static inline uint64_t gzmw_deflate_bound(uint64_t len)
{
	uint64_t blocks = (len + 4999) / 5000;
	if (blocks < 1)
		blocks = 1;
	return 5 * blocks + len;
}

/* Sum(libdeflate_gzip_compress_bound(in_nbytes[k]) + (name ? name + 1 : 0));
 * name_offsets NULL: no record has a name */
static inline uint64_t
gzmw_bound(uint64_t n, const uint64_t *name_offsets, const uint64_t *in_nbytes)
{
	uint64_t sum = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t nl = name_offsets ? name_offsets[k + 1] - name_offsets[k] : 0;
		sum += GZMW_HEADER_BYTES + GZMW_FOOTER_BYTES + gzmw_deflate_bound(in_nbytes[k]) +
		       (nl ? nl + 1 : 0);
	}
	return sum;
}

/* true, or false with the reason in err: what the call refuses before any
 * device work, pointers apart (the arrays are there when n != 0; names and
 * name_offsets both or neither) */
static inline bool
gzmw_check(uint64_t n, const uint8_t *names, const uint64_t *name_offsets,
	   const uint64_t *in_offsets, const uint64_t *in_nbytes, uint64_t in_avail, unsigned flags,
	   int level, std::string &err)
{
	char msg[200];

	if (flags) {
		snprintf(msg, sizeof(msg), "unknown flags 0x%x", flags);
		err = msg;
		return false;
	}
	if (n > GZMW_MAX_RECORDS) {
		snprintf(msg, sizeof(msg), "n_records %llu above 2^28", (unsigned long long)n);
		err = msg;
		return false;
	}
	for (uint64_t k = 0; k < n; k++) {
		const char *why = NULL;
		if (name_offsets && name_offsets[k + 1] < name_offsets[k])
			why = "name_offsets decrease";
		else if (name_offsets && name_offsets[k + 1] - name_offsets[k] > GZMW_NAME_MAX)
			why = "a name of more than 65534 bytes";
		else if (in_nbytes[k] > 0xFFFFFFFFull)
			why = "a record of 4 GiB or more";
		else if (in_offsets[k] > in_avail || in_avail - in_offsets[k] < in_nbytes[k])
			why = "its bytes do not lie inside in_avail";
		else if (level == 0 && in_nbytes[k] > GZMW_PIECE_MAX)
			why = "a level-0 record above 0xFFFFFF00 bytes, which no compress call takes";
		if (!why && name_offsets)
			for (uint64_t b = name_offsets[k]; b < name_offsets[k + 1]; b++)
				if (names[b] == 0)
					why = "a name that holds a 0 byte";
		if (why) {
			snprintf(msg, sizeof(msg), "record %llu: %s", (unsigned long long)k, why);
			err = msg;
			return false;
		}
	}
	return true;
}

struct gzmw_plan : zipw_pieces {
	uint64_t n, bound, usize_total, names_bytes;
	std::vector<uint64_t> ecols;	/* GZMW_ECOLS x n */
};

/* the arguments have passed gzmw_check(); pr.store is false whatever the level */
static inline void
gzmw_plan_build(const zipw_params &pr, uint64_t n, const uint64_t *name_offsets,
		const uint64_t *in_offsets, const uint64_t *in_nbytes, gzmw_plan &p)
{
	p.n = n;
	p.bound = gzmw_bound(n, name_offsets, in_nbytes);
	p.names_bytes = n && name_offsets ? name_offsets[n] - name_offsets[0] : 0;
	p.ecols.assign((size_t)(GZMW_ECOLS * n), 0);
	uint64_t uoff = 0;
	for (uint64_t k = 0; k < n; k++) {
		if (name_offsets) {
			p.ecols[GZMW_E_NAME_OFF * n + k] = name_offsets[k] - name_offsets[0];
			p.ecols[GZMW_E_NAME_LEN * n + k] = name_offsets[k + 1] - name_offsets[k];
		}
		p.ecols[GZMW_E_USIZE * n + k] = in_nbytes[k];
		p.ecols[GZMW_E_UOFF * n + k] = uoff;
		uoff += in_nbytes[k];
	}
	p.usize_total = uoff;
	zipw_cut_pieces(pr, n, in_offsets, in_nbytes, p.ecols.data() + GZMW_E_FIRST * n,
			p.ecols.data() + GZMW_E_COUNT * n, p);
}

} /* namespace lda */

#endif /* LDA_GZIP_MEMBERS_WRITE_PLAN_H */
