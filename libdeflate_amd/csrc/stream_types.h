/*
 * stream_types.h - the chunk descriptor and the chunk result of the kernels
 * that decode ONE large stream on many waves (inflate_stream.hip), as plain
 * data: what the kernels (stream_kernels.h), the host that plans and chains
 * them (stream_plan.h, host_stream.hip) and the seek index (seek_plan.h) share.
 * No HIP in here: the stand-alone CPU tests under tools/ include it.
 */
#ifndef LDA_STREAM_TYPES_H
#define LDA_STREAM_TYPES_H

#include <stdint.h>

/* how a chunk starts */
#define LDA_CHUNK_HEADER 0u	/* at the block header at hdr_bit */
#define LDA_CHUNK_WARM 1u	/* inside the block of hdr_bit: parse from start_bit (a guess),
				 * the first token boundary >= target_bit is the start */
#define LDA_CHUNK_EXACT 2u	/* inside the block of hdr_bit, at the token boundary start_bit */

/* hdr_bit of a chunk that starts inside a STATIC block: the static codes need
 * no header, so such a chunk can be planned without knowing where its block
 * began (a stream of static blocks has no header the finder could find).  It
 * does not know either whether its block is the stream's last: it stops at
 * the block's end-of-block symbol, a boundary like any other, and the host -
 * which follows the chain from a chunk that did read the header - knows
 * whether the stream ends there. */
#define LDA_HDR_STATIC (~(uint64_t)1)

/* All positions are bit offsets into the raw DEFLATE stream.  A chunk ends at
 * the first token boundary (the end of a block counts) at or after limit_bit,
 * or with the stream's final block. */
struct lda_stream_chunk {
	uint64_t hdr_bit;
	uint64_t start_bit;
	uint64_t target_bit;
	uint64_t limit_bit;
	uint64_t out_off;	/* decode pass: absolute output position of the chunk's first byte */
	uint32_t kind;
	uint32_t phases;	/* count pass: 0, or K on the first of K EXACT chunks at consecutive
				 * bits with one limit that are counted together, ~0 on the others */
	uint32_t hdr_cache;	/* 0, or 1 + the slot of lda_stream_hdr_cache_kernel that holds the
				 * code lengths of the header at hdr_bit */
	uint32_t hint;		/* decode pass: 0, or 1 + the row of token boundaries the count pass
				 * left for this chunk (phase_count(): starts for the lanes' parses) */
};

#define LDA_STREAM_OK 0u	/* stopped at the limit */
#define LDA_STREAM_FINAL 1u	/* the final block ended */
#define LDA_STREAM_ERR 2u	/* not decodable from here (or a garbage start) */
#define LDA_RES_BOUNDARY 1u	/* end_bit is the first bit of a block header */
#define LDA_RES_BAD_DIST 2u	/* a distance reaches back before the stream */
#define LDA_RES_GOV_FINAL 4u	/* end_bit lies inside the stream's final block (as far as the
				 * chunk knows: it read that block's header) */

struct lda_stream_res {
	uint64_t start_bit;	/* where the chunk really started (WARM: found) */
	uint64_t end_bit;
	uint64_t end_hdr_bit;	/* header of the block end_bit lies in (= end_bit at a boundary;
				 * LDA_HDR_STATIC inside a static block, wherever it began) */
	uint64_t nout;		/* bytes the chunk produces */
	uint32_t status;
	uint32_t flags;
};

#endif /* LDA_STREAM_TYPES_H */
