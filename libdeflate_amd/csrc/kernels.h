/*
 * kernels.h - device entry points shared between the .hip translation units
 * and the host side of the C-ABI (host_*.hip).
 */
#ifndef LDA_KERNELS_H
#define LDA_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "large_plan.h"

/* checksum_kernels.hip */
extern "C" __global__ void
lda_crc32_batch_kernel(uint64_t n_chunks, const uint8_t *base,
		       const uint64_t *offsets, const uint64_t *nbytes,
		       const uint32_t *init, uint32_t *out,
		       const uint32_t *g_tables, const uint32_t *xpow8);
extern "C" __global__ void
lda_adler32_batch_kernel(uint64_t n_chunks, const uint8_t *base,
			 const uint64_t *offsets, const uint64_t *nbytes,
			 const uint32_t *init, uint32_t *out);
/* a preset dictionary's per-batch block (layout in checksum_kernels.hip) */
#define LDA_DICT_BLK_HDR 64
extern "C" __global__ void
lda_dict_prep_kernel(const uint8_t *dict, uint64_t dict_nbytes, uint32_t tail,
		     uint32_t pre_len, uint32_t sinfo, uint8_t *blk);

/* inflate_kernel.hip */
extern "C" __global__ void
lda_inflate_batch_kernel(uint64_t n_chunks, int format, uint32_t lpw,
			 const uint8_t *in_base,
			 const uint64_t *in_offsets, const uint64_t *in_nbytes,
			 uint8_t *out_base, const uint64_t *out_offsets,
			 const uint64_t *out_avail, int32_t *results,
			 uint64_t *actual_in, uint64_t *actual_out,
			 const uint8_t *dict, uint32_t dict_len,
			 const uint32_t *dict_id);
extern "C" __global__ void
lda_inflate_wave_kernel(uint64_t n_chunks, int format, uint32_t *tokscratch,
			uint32_t *next_stream, const uint32_t *order,
			const uint8_t *in_base,
			const uint64_t *in_offsets, const uint64_t *in_nbytes,
			uint8_t *out_base, const uint64_t *out_offsets,
			const uint64_t *out_avail, int32_t *results,
			uint64_t *actual_in, uint64_t *actual_out,
			const uint8_t *dict, uint32_t dict_len,
			const uint32_t *dict_id);
extern "C" __global__ void
lda_inflate_order_kernel(uint64_t n, const uint64_t *in_nbytes, const uint64_t *out_avail,
			 uint32_t *order);
/* inflate_sizes.hip: the size query and the descriptors of the packed decode */
extern "C" __global__ void
lda_inflate_sizes_kernel(uint64_t n_chunks, int format, uint32_t par, uint32_t *next_stream,
			 const uint32_t *order, const uint8_t *in_base,
			 const uint64_t *in_offsets, const uint64_t *in_nbytes,
			 const uint64_t *limits, int32_t *results, uint64_t *actual_in,
			 uint64_t *out_nbytes, uint32_t dict_len, const uint32_t *dict_id);
extern "C" size_t lda_inflate_sizes_lds_bytes(void);
extern "C" __global__ void
lda_packed_round_kernel(uint64_t n, uint64_t align_mask, const uint64_t *sizes,
			uint64_t *rounded);
extern "C" __global__ void
lda_packed_desc_kernel(uint64_t n, uint64_t capacity, const uint64_t *in_nbytes,
		       const uint64_t *sizes, const uint64_t *block_sums, uint64_t *offsets,
		       int32_t *verdict, uint64_t *dec_in_nbytes, uint64_t *dec_avail);
extern "C" __global__ void
lda_packed_merge_kernel(uint64_t n, const int32_t *verdict, int32_t *results,
			uint64_t *actual_in, uint64_t *actual_out);
/* inflate_prefix.hip: the decode cut at every stream's limit */
extern "C" __global__ void
lda_inflate_prefix_kernel(uint64_t n_chunks, int format, uint32_t par, uint32_t *tokscratch,
			  uint32_t *next_stream, const uint32_t *order, const uint8_t *in_base,
			  const uint64_t *in_offsets, const uint64_t *in_nbytes,
			  uint8_t *out_base, const uint64_t *out_offsets, const uint64_t *limits,
			  int32_t *results, uint64_t *actual_in, uint64_t *actual_out,
			  const uint8_t *dict, uint32_t dict_len, const uint32_t *dict_id);
/* ... and the descriptors of the heads of an indexed gzip-members file */
extern "C" __global__ void
lda_gzm_peek_desc_kernel(uint64_t max_members, uint64_t n, uint64_t head, const uint64_t *result,
			 const uint64_t *index, uint64_t *in_off, uint64_t *in_n, uint64_t *out_off,
			 uint64_t *limits, int32_t *results, uint64_t *head_nbytes);
extern "C" size_t lda_inflate_tokcap(void);
extern "C" size_t lda_inflate_window_bytes(void);
extern "C" __global__ void
lda_inflate_finalize_kernel(uint64_t n_chunks, int format, int exact_fill,
			    const uint8_t *in_base, const uint64_t *in_offsets,
			    const uint64_t *out_avail, const uint32_t *sums,
			    int32_t *results, uint64_t *actual_in,
			    uint64_t *actual_out);

/* deflate_kernel.hip */
#define LDA_DEFLATE_THREADS 1024	/* one workgroup (16 waves) per buffer */
/*
 * Levels 0-9 of a batch with a size bound run in two kernels: the LZ77 stage
 * (lda_deflate_batch_kernel) leaves every buffer's tokens in a list of its own
 * (tok_buf + c * tok_stride, u32 each, TOK_MATCH of deflate_kernel.hip) and
 * one descriptor per block; lda_deflate_entropy_kernel (deflate_entropy.hip)
 * writes the streams from them.  blk_buf: [count of buffer c: u32 x n, padded
 * to 16 words][list of the LDA_BLK_FUSED buffers: u32 x n, padded][blk_stride
 * descriptors of LDA_BLK_WORDS u32 per buffer]; the count is LDA_BLK_OVERFLOW
 * where the stream cannot fit (its size becomes 0), LDA_BLK_FUSED where the
 * buffer is larger than the bound: the LZ77 stage lists it (*fused_cnt, zero
 * before the launch, counts the list), the entropy kernel skips it and
 * lda_deflate_fused_kernel, launched behind it with the same blk_buf and
 * fused_cnt, compresses it.
 */
#define LDA_BLK_TOK0 0		/* first token: index in the buffer's list */
#define LDA_BLK_NTOK 1		/* tokens */
#define LDA_BLK_START 2		/* bytes [start, end) of the buffer */
#define LDA_BLK_END 3
#define LDA_BLK_FLAGS 4		/* BFINAL | LDA_BLK_STORED */
#define LDA_BLK_STORED 2u	/* level 0 and tiny inputs: stored only */
#define LDA_BLK_FREQ 8		/* [320] litlen 0..287, offset 288..319 (no end-of-block) */
#define LDA_BLK_WORDS (LDA_BLK_FREQ + 320)
#define LDA_BLK_OVERFLOW 0xFFFFFFFFu
#define LDA_BLK_FUSED 0xFFFFFFFEu
#define LDA_BLK_LIST(n) (((n) + 15) / 16 * 16)
#define LDA_BLK_HDR_WORDS(n) (2 * LDA_BLK_LIST(n))
extern "C" __global__ void
lda_deflate_batch_kernel(uint64_t n_chunks, int format, int level,
			 uint32_t depth, uint32_t nice, uint32_t mode,
			 const uint8_t *in_base, const uint64_t *in_offsets,
			 const uint64_t *in_nbytes, uint8_t *out_base,
			 const uint64_t *out_offsets, const uint64_t *out_avail,
			 uint64_t *out_nbytes, const uint32_t *sums,
			 uint64_t *seq_scratch, const uint32_t *seg_info,
			 uint32_t *next_chunk, const uint8_t *dict_pre,
			 uint32_t *tok_buf, uint32_t *blk_buf, uint32_t tok_stride,
			 uint32_t blk_stride, uint32_t *fused_cnt);
/* the same stage built for one level, 1-9, with that level's depth, nice length
 * and mode as constants (deflate_l<N>.hip): the same arguments, of which level,
 * depth, nice and mode are not read */
typedef void (*lda_lz77_kernel_t)(uint64_t, int, int, uint32_t, uint32_t, uint32_t,
				  const uint8_t *, const uint64_t *, const uint64_t *, uint8_t *,
				  const uint64_t *, const uint64_t *, uint64_t *, const uint32_t *,
				  uint64_t *, const uint32_t *, uint32_t *, const uint8_t *,
				  uint32_t *, uint32_t *, uint32_t, uint32_t, uint32_t *);
#define LDA_LZ77_INSTANCE(N)                                                   \
	extern "C" __global__ void                                             \
	lda_deflate_batch_kernel_l##N(uint64_t n_chunks, int format, int level, \
		uint32_t depth, uint32_t nice, uint32_t mode,                  \
		const uint8_t *in_base, const uint64_t *in_offsets,            \
		const uint64_t *in_nbytes, uint8_t *out_base,                  \
		const uint64_t *out_offsets, const uint64_t *out_avail,        \
		uint64_t *out_nbytes, const uint32_t *sums,                    \
		uint64_t *seq_scratch, const uint32_t *seg_info,               \
		uint32_t *next_chunk, const uint8_t *dict_pre,                 \
		uint32_t *tok_buf, uint32_t *blk_buf, uint32_t tok_stride,     \
		uint32_t blk_stride, uint32_t *fused_cnt);
LDA_LZ77_INSTANCE(1) LDA_LZ77_INSTANCE(2) LDA_LZ77_INSTANCE(3)
LDA_LZ77_INSTANCE(4) LDA_LZ77_INSTANCE(5) LDA_LZ77_INSTANCE(6)
LDA_LZ77_INSTANCE(7) LDA_LZ77_INSTANCE(8) LDA_LZ77_INSTANCE(9)
#undef LDA_LZ77_INSTANCE
/* the same body with the block end inside the tile loop (no bound: unbounded
 * batches, a preset dictionary; blk_buf NULL), or behind a split launch for
 * the buffers it marked LDA_BLK_FUSED (blk_buf of that launch) */
extern "C" __global__ void
lda_deflate_fused_kernel(uint64_t n_chunks, int format, int level,
			 uint32_t depth, uint32_t nice, uint32_t mode,
			 const uint8_t *in_base, const uint64_t *in_offsets,
			 const uint64_t *in_nbytes, uint8_t *out_base,
			 const uint64_t *out_offsets, const uint64_t *out_avail,
			 uint64_t *out_nbytes, const uint32_t *sums,
			 uint64_t *seq_scratch, const uint32_t *seg_info,
			 uint32_t *next_chunk, const uint8_t *dict_pre,
			 const uint32_t *blk_buf, const uint32_t *fused_cnt);
/* deflate_entropy.hip: one workgroup per buffer of the launch before it;
 * *next_chunk (zero before the launch) hands the buffers out */
#define LDA_DEFLATE_ENTROPY_THREADS 256
extern "C" __global__ void
lda_deflate_entropy_kernel(uint64_t n_chunks, int format, int level,
			   const uint8_t *in_base, const uint64_t *in_offsets,
			   const uint64_t *in_nbytes, uint8_t *out_base,
			   const uint64_t *out_offsets, const uint64_t *out_avail,
			   uint64_t *out_nbytes, const uint32_t *sums,
			   const uint32_t *seg_info, const uint32_t *tok_buf,
			   const uint32_t *blk_buf, uint32_t tok_stride,
			   uint32_t blk_stride, uint32_t *next_chunk);
extern "C" size_t lda_deflate_entropy_lds_bytes(void);
/* same body with the min-cost parse compiled in: levels 10-12 */
extern "C" __global__ void
lda_deflate_opt_kernel(uint64_t n_chunks, int format, int level,
		       uint32_t depth, uint32_t nice, uint32_t mode,
		       const uint8_t *in_base, const uint64_t *in_offsets,
		       const uint64_t *in_nbytes, uint8_t *out_base,
		       const uint64_t *out_offsets, const uint64_t *out_avail,
		       uint64_t *out_nbytes, const uint32_t *sums,
		       uint64_t *seq_scratch, const uint32_t *seg_info,
		       uint32_t *next_chunk, const uint8_t *dict_pre);
/* deflate_small.hip: buffers of at most lda_deflate_small_max() bytes */
#define LDA_DEFLATE_SMALL_THREADS 256
extern "C" __global__ void
lda_deflate_small_kernel(uint64_t n_chunks, int format, int level,
			 uint32_t depth, uint32_t nice, uint32_t mode,
			 const uint8_t *in_base, const uint64_t *in_offsets,
			 const uint64_t *in_nbytes, uint8_t *out_base,
			 const uint64_t *out_offsets, const uint64_t *out_avail,
			 uint64_t *out_nbytes, const uint32_t *sums,
			 uint64_t *seq_scratch, const uint32_t *seg_info,
			 uint32_t *next_chunk, const uint8_t *dict_pre);
extern "C" size_t lda_deflate_small_lds_bytes(void);
extern "C" size_t lda_deflate_small_max(void);
extern "C" size_t lda_deflate_small_wgs(void);	/* workgroups per CU it is built for */
extern "C" size_t lda_deflate_tile(void);	/* positions per tile (dictionary granularity) */
extern "C" size_t lda_deflate_lds_bytes(void);
extern "C" size_t lda_deflate_seq_words(void);	/* u64 words of HBM scratch per workgroup (token list, saved histograms) */

extern "C" size_t lda_inflate_lds_per_stream(void);
extern "C" size_t lda_inflate_lds_shared(void);

/* compact_kernels.hip */
#define LDA_SCAN_BLOCK 2048	/* compact_kernels.hip: SCAN_BLOCK, sizes per lda_scan_local_kernel workgroup */
extern "C" __global__ void
lda_scan_local_kernel(uint64_t n, const uint64_t *sizes, uint64_t *offsets,
		      uint64_t *block_sums);
extern "C" __global__ void
lda_scan_blocks_kernel(uint64_t nblocks, uint64_t *block_sums);
extern "C" __global__ void
lda_compact_copy_kernel(uint64_t n, const uint8_t *in_base,
			const uint64_t *in_offsets, const uint64_t *sizes,
			uint8_t *out_base, uint64_t *offsets,
			const uint64_t *block_sums);
/* compact_kernels.hip: a BGZF file from one device buffer (host_bgzf.hip) */
extern "C" __global__ void
lda_bgzf_desc_kernel(uint64_t m, uint64_t n, uint64_t *in_off, uint64_t *in_n,
		     uint64_t *slot_off, uint64_t *slot_avail);
extern "C" __global__ void
lda_bgzf_copy_kernel(uint64_t m, const uint8_t *slots, const uint64_t *sizes,
		     const uint64_t *offsets, const uint64_t *block_sums, uint8_t *out,
		     uint64_t out_avail, uint32_t eof_bytes, uint64_t *index);
extern "C" __global__ void
lda_bgzf_finalize_kernel(uint64_t m, uint64_t n, const uint64_t *sizes,
			 const uint64_t *total_at, uint8_t *out, uint64_t out_avail,
			 uint32_t eof_bytes, uint64_t *out_nbytes, uint64_t *index);

/* large_kernels.hip: one raw DEFLATE / zlib / gzip stream from one device
 * buffer (host_compress.hip, large_plan.h) */
extern "C" __global__ void
lda_large_desc_kernel(struct lda_large_shape g, uint64_t *rows, uint32_t *seg_info);
extern "C" __global__ void
lda_large_one_desc_kernel(uint64_t n, uint64_t out_avail, uint64_t *rows);
extern "C" __global__ void
lda_large_copy_kernel(uint64_t nseg, const uint8_t *slots, uint64_t slot, const uint64_t *sizes,
		      const uint64_t *offsets, const uint64_t *block_sums, uint8_t *out,
		      uint32_t hdr, uint32_t ftr, uint64_t out_avail);
extern "C" __global__ void
lda_large_finalize_kernel(uint64_t nseg, uint64_t n, uint64_t S, int format, int level,
			  const uint64_t *sizes, const uint32_t *sums, const uint64_t *total_at,
			  uint32_t xS, uint32_t xL, uint8_t *out, uint64_t out_avail,
			  uint64_t *out_nbytes);

/* bgzf_read_kernels.hip: a BGZF file read from device memory (host_bgzf_read.hip) */
#define LDA_BR_TILE 4096	/* bytes per step of the candidate scan: 256 threads x 16 */
#define LDA_BR_SCAN_WG 16384	/* bytes per workgroup of it */
#define LDA_BR_JUMP 1024	/* candidates per block of the chain validation */
#define LDA_BR_LOG 10
#define LDA_BR_END 0xFFFFFFFFu	/* a candidate's successor: the end of the file */
#define LDA_BR_NONE 0xFFFFFFFEu	/* no candidate starts where it ends */
/* the finder's state (u32 words, zero before the first launch) */
#define LDA_BR_CHAIN 0		/* 1: the chain from offset 0 ends exactly at n */
#define LDA_BR_MEMBERS 1	/* its length */
#define LDA_BR_BADISIZE 2	/* a member's ISIZE is above 64 KiB */
#define LDA_BR_STATE_WORDS 4
#define LDA_BR_MORE 16		/* LIBDEFLATE_AMD_BGZF_MORE_MEMBERS */
#define LDA_BR_HAS_EOF 1	/* LIBDEFLATE_AMD_BGZF_HAS_EOF */
#define LDA_BR_RESULT_WORDS 5
extern "C" __global__ void
lda_bgzf_scan_kernel(const uint8_t *in, uint64_t n, uint64_t *counts, const uint64_t *offsets,
		     const uint64_t *block_sums, uint64_t cap, uint64_t *cand_pos,
		     uint32_t *cand_size);
extern "C" __global__ void
lda_bgzf_jump_kernel(uint64_t n, const uint64_t *k_at, uint64_t cap, const uint64_t *cand_pos,
		     const uint32_t *cand_size, uint32_t *next, uint32_t *exit_at, uint32_t *hops,
		     uint32_t *entry);
extern "C" __global__ void
lda_bgzf_top_kernel(const uint64_t *k_at, uint64_t cap, const uint64_t *cand_pos,
		    const uint32_t *exit_at, const uint32_t *hops, uint32_t *entry,
		    uint32_t *base, uint32_t *state);
extern "C" __global__ void
lda_bgzf_members_kernel(const uint64_t *k_at, uint64_t cap, uint64_t max_members,
			const uint64_t *cand_pos, const uint32_t *cand_size,
			const uint32_t *next, const uint32_t *hops, const uint32_t *entry,
			const uint32_t *base, const uint32_t *state, uint64_t *in_off,
			uint64_t *in_n);
extern "C" __global__ void
lda_bgzf_walk_kernel(const uint8_t *in, uint64_t n, uint64_t max_members, const uint64_t *k_at,
		     uint64_t cap, int force, uint64_t *in_off, uint64_t *in_n, uint32_t *state);
extern "C" __global__ void
lda_bgzf_isize_kernel(const uint8_t *in, uint64_t n, uint64_t max_members,
		      const uint64_t *in_off, const uint64_t *in_n, uint32_t *state,
		      uint64_t *isize);
extern "C" __global__ void
lda_bgzf_rdesc_kernel(uint64_t max_members, uint64_t out_avail, const uint32_t *state,
		      const uint64_t *isize, const uint64_t *block_sums, uint64_t *in_off,
		      uint64_t *in_n, uint64_t *out_off, uint64_t *out_av, uint64_t *index);
extern "C" __global__ void
lda_bgzf_rfinal_kernel(const uint8_t *in, uint64_t n, uint64_t max_members, uint64_t out_avail,
		       const uint32_t *state, const uint64_t *total_at, const uint64_t *in_off,
		       const uint64_t *in_n, const int32_t *results, const uint64_t *actual_in,
		       uint64_t *result, uint64_t *index);
extern "C" __global__ void
lda_bgzf_trim_kernel(uint64_t n_trims, const uint64_t *trims, const uint8_t *slots,
		     uint8_t *out);
extern "C" __global__ void
lda_bgzf_range_kernel(uint64_t n_ranges, const uint64_t *first, const uint64_t *in_n,
		      const int32_t *results, const uint64_t *actual_in, int32_t *range_results);

/* gzip_members_kernels.hip: a file of concatenated gzip members read from
 * device memory (host_gzip_members.hip); the chain among the candidates is
 * found by lda_bgzf_jump_kernel / _top_ / _members_ above, whose state words
 * LDA_BR_CHAIN and LDA_BR_MEMBERS it shares */
#define LDA_GZM_BREAK 3		/* state word: the verdict of a broken chain */
#define LDA_GZM_MORE_CANDIDATES 17	/* LIBDEFLATE_AMD_GZM_MORE_CANDIDATES */
#define LDA_GZM_RESULT_WORDS 5
#define LDA_GZM_NAME_MAX 65536u	/* LIBDEFLATE_AMD_GZM_NAME_MAX */
extern "C" __global__ void
lda_gzm_scan_kernel(const uint8_t *in, uint64_t n, uint64_t *counts, const uint64_t *offsets,
		    const uint64_t *block_sums, uint64_t cap, uint64_t *cand_pos);
extern "C" __global__ void
lda_gzm_slots_kernel(const uint8_t *in, uint64_t n, const uint64_t *k_at, uint64_t cap, const uint64_t *cand_pos,
		     uint64_t *in_off, uint64_t *in_n);
extern "C" __global__ void
lda_gzm_size32_kernel(const uint64_t *k_at, uint64_t cap, int32_t *results,
		      const uint64_t *actual_in, uint32_t *cand_size);
extern "C" __global__ void
lda_gzm_break_kernel(const uint64_t *k_at, uint64_t cap, const uint64_t *cand_pos,
		     const uint32_t *next, const uint32_t *exit_at, const int32_t *results,
		     uint32_t *state);
extern "C" __global__ void
lda_gzm_msize_kernel(uint64_t max_members, const uint64_t *k_at, uint64_t cap,
		     const uint64_t *cand_pos, const uint64_t *cand_out, const uint32_t *state,
		     const uint64_t *in_off, uint64_t *msize);
extern "C" __global__ void
lda_gzm_desc_kernel(uint64_t max_members, uint64_t out_avail, const uint64_t *k_at, uint64_t cap,
		    const uint32_t *state, const uint64_t *msize, const uint64_t *block_sums,
		    uint64_t *in_off, uint64_t *in_n, uint64_t *out_off, uint64_t *out_av,
		    uint64_t *index);
extern "C" __global__ void
lda_gzm_final_kernel(uint64_t n, uint64_t max_members, uint64_t out_avail, const uint64_t *k_at,
		     uint64_t cap, const uint32_t *state, const uint64_t *total_at,
		     const uint64_t *in_n, const int32_t *results, const uint64_t *actual_in,
		     uint64_t *result, uint64_t *index);

/* zip_kernels.hip: a ZIP archive read from device memory (host_zip.hip); the
 * chain among the directory's candidates is found by lda_bgzf_jump_kernel /
 * _top_ / _members_ above, whose state words LDA_BR_CHAIN and LDA_BR_MEMBERS it
 * shares.  Copies of the header's constants (static_assert in host_zip.hip) */
#define LDA_ZIP_MORE_ENTRIES 16		/* LIBDEFLATE_AMD_ZIP_MORE_ENTRIES */
#define LDA_ZIP_MORE_CANDIDATES 17	/* LIBDEFLATE_AMD_ZIP_MORE_CANDIDATES */
#define LDA_ZIP_UNSUPPORTED 18		/* LIBDEFLATE_AMD_ZIP_UNSUPPORTED */
#define LDA_ZIP_RESULT_WORDS 5
#define LDA_ZIP_WORDS 8
#define LDA_ZIP_ZIP64 1
#define LDA_ZIP_WINDOW 65557u	/* an end record and the longest comment */
/* the chain's end as the chain kernels are told it: cd_size is below 2^32 */
#define LDA_ZIP_CHAIN_END 0xFFFFFFFFull
/* what the end record says (u64 words) */
#define LDA_ZS_BAD 0		/* 1: no end record, an inconsistent one, a directory out of bounds */
#define LDA_ZS_ENTRIES 1
#define LDA_ZS_CD_OFF 2
#define LDA_ZS_CD_SIZE 3
#define LDA_ZS_FLAGS 4
#define LDA_ZS_WORDS 8
/* meta[k] >> 40 (zip_plan.h builds the same words for a selection) */
#define LDA_ZIP_KIND_NONE 0
#define LDA_ZIP_KIND_STORED 1
#define LDA_ZIP_KIND_DEFLATE 2
extern "C" __global__ void
lda_zip_end_kernel(const uint8_t *in, uint64_t n, uint64_t *zs);
extern "C" __global__ void
lda_zip_scan_kernel(const uint8_t *in, const uint64_t *zs, uint64_t *counts,
		    const uint64_t *offsets, const uint64_t *block_sums, uint64_t cap,
		    uint64_t *cand_pos);
extern "C" __global__ void
lda_zip_size_kernel(const uint8_t *in, const uint64_t *zs, const uint64_t *k_at, uint64_t cap,
		    const uint64_t *cand_pos, uint32_t *cand_size);
extern "C" __global__ void
lda_zip_resolve_kernel(const uint8_t *in, uint64_t max_entries, uint64_t align_mask,
		       const uint64_t *zs, const uint32_t *state, const uint64_t *k_at,
		       uint64_t cap, const uint64_t *rel, uint64_t *rows, int32_t *results,
		       uint64_t *sizes);
extern "C" __global__ void
lda_zip_desc_kernel(uint64_t max_entries, uint64_t out_avail, const uint64_t *zs,
		    const uint32_t *state, const uint64_t *k_at, uint64_t cap,
		    const uint64_t *block_sums, uint64_t *rows, const int32_t *results,
		    uint64_t *in_off, uint64_t *in_n, uint64_t *out_off, uint64_t *out_av,
		    uint64_t *cp_src, uint64_t *cp_len, uint64_t *crc_n, uint64_t *meta);
extern "C" __global__ void
lda_zip_copy_kernel(uint64_t n_chunks, const uint64_t *src, const uint64_t *dst,
		    const uint64_t *len, const uint8_t *in, uint8_t *out);
extern "C" __global__ void
lda_zip_final_kernel(uint64_t max_entries, uint64_t out_avail, const uint64_t *zs,
		     const uint32_t *state, const uint64_t *k_at, uint64_t cap,
		     const uint64_t *total_at, const uint64_t *meta, const uint64_t *in_n,
		     const int32_t *batch_res, const uint64_t *actual_in, const uint32_t *crcs,
		     int32_t *results, uint64_t *result);
extern "C" __global__ void
lda_zip_rfinal_kernel(uint64_t n_sel, const uint64_t *meta, const uint64_t *in_n,
		      const int32_t *batch_res, const uint64_t *actual_in, const uint32_t *crcs,
		      int32_t *results);

/* zip_large_kernels.hip: the entries of a selection that left the one-wave
 * batch (host_zip_large.hip; zip_large_plan.h builds the tables and holds
 * copies of these constants) */
#define LDA_ZIP_PIECE (1u << 20)	/* LIBDEFLATE_AMD_ZIP_PIECE */
#define LDA_ZIPL_OWNED 48		/* meta bit: the row's result is lda_zip_lfinal_kernel's */
#define LDA_ZIPL_MANY_WAVE 1		/* flags of an owned entry */
#define LDA_ZIPL_PIECED 2
extern "C" __global__ void
lda_zip_lfinal_kernel(uint64_t n_own, uint64_t n_sel, uint64_t n_pieces, const uint64_t *l_sel,
		      const uint64_t *l_flags, const uint64_t *l_in_n, const uint64_t *l_usize,
		      const uint64_t *l_first, const uint64_t *l_count, const uint64_t *l_res,
		      const uint64_t *l_ain, const uint64_t *meta, const int32_t *batch_res,
		      const uint64_t *batch_ain, const uint32_t *batch_crcs, const uint64_t *p_dst,
		      const uint64_t *p_len, const uint32_t *p_crcs, int32_t *results);

/* tar_kernels.hip: a tar archive read from device memory (host_tar.hip).  The
 * candidates are (position, size) in blocks of 512 bytes, and the chain among
 * them is found by lda_bgzf_jump_kernel / _top_ / _members_ above, launched
 * with the block count as the end; the state words LDA_BR_CHAIN and
 * LDA_BR_MEMBERS are theirs, the other two this reader's.  Copies of the
 * header's constants (static_assert in host_tar.hip) */
#define LDA_TAR_MORE_RECORDS 16		/* LIBDEFLATE_AMD_TAR_MORE_RECORDS */
#define LDA_TAR_MORE_CANDIDATES 17	/* LIBDEFLATE_AMD_TAR_MORE_CANDIDATES */
#define LDA_TAR_UNSUPPORTED 18		/* LIBDEFLATE_AMD_TAR_UNSUPPORTED */
#define LDA_TAR_RESULT_WORDS 5
#define LDA_TAR_WORDS 8
#define LDA_TAR_EOF 1
#define LDA_TAR_HAS_L 2
#define LDA_TAR_HAS_PAX 4
#define LDA_TAR_NAME_HEADER 0	/* row word 3 >> 8: where the name stands */
#define LDA_TAR_NAME_L 1
#define LDA_TAR_NAME_PAX 2
#define LDA_TAR_EXT_MAX 8	/* extension records in front of one entry */
#define LDA_TAR_EXT_BYTES 1048576	/* the largest L or x record that is read */
#define LDA_TAR_SCAN_BLOCKS 32	/* blocks per scan workgroup: LDA_BR_SCAN_WG / 512 */
#define LDA_TAR_COPY_TILE 65536	/* bytes per tile of the gather copy */
#define LDA_TAR_FLAGS 2		/* state word: LDA_TAR_HAS_L | LDA_TAR_HAS_PAX */
#define LDA_TAR_ZERO0 3		/* state word: block 0 is all zero, an empty archive */
#define LDA_TS_END 0		/* ts[]: where the last record ends by its own size, in blocks */
#define LDA_TS_WORDS 2
extern "C" __global__ void
lda_tar_scan_kernel(const uint8_t *in, uint64_t nb, uint64_t *counts, const uint64_t *offsets,
		    const uint64_t *block_sums, uint64_t cap, uint64_t *cand_pos,
		    uint32_t *cand_size, uint32_t *state);
extern "C" __global__ void
lda_tar_walk_kernel(const uint8_t *in, uint64_t nb, uint64_t max_records, uint64_t *rec_pos,
		    uint64_t *rec_n, uint32_t *state, uint64_t *k_out);
extern "C" __global__ void
lda_tar_resolve_kernel(const uint8_t *in, uint64_t nb, uint64_t max_records, uint64_t align_mask,
		       uint32_t *state, const uint64_t *k_at, uint64_t cap,
		       const uint64_t *rec_pos, uint64_t *ts, uint64_t *tmp, int32_t *res,
		       uint64_t *flag, uint64_t *room);
extern "C" __global__ void
lda_tar_desc_kernel(uint64_t max_records, uint64_t out_avail, const uint32_t *state,
		    const uint64_t *k_at, uint64_t cap, const uint64_t *tmp, const int32_t *res,
		    const uint64_t *flag, const uint64_t *f_off, const uint64_t *f_sums,
		    const uint64_t *r_off, const uint64_t *r_sums, uint64_t *rows,
		    int32_t *results, uint64_t *cp_src, uint64_t *cp_dst, uint64_t *cp_len,
		    uint64_t *tiles);
extern "C" __global__ void
lda_tar_copy_kernel(uint64_t n_chunks, const uint64_t *t_off, const uint64_t *t_sums,
		    const uint64_t *total_at, const uint64_t *src, const uint64_t *dst,
		    const uint64_t *len, const uint8_t *in, uint8_t *out);
extern "C" __global__ void
lda_tar_final_kernel(uint64_t nb, uint64_t max_records, uint64_t out_avail,
		     const uint32_t *state, const uint64_t *k_at, uint64_t cap,
		     const uint64_t *ts, const uint64_t *entries_at, const uint64_t *total_at,
		     const int32_t *results, uint64_t *result);

/* zip_write_kernels.hip: a ZIP archive assembled in device memory
 * (host_zip_write.hip, zip_write_plan.h) */
extern "C" __global__ void
lda_zipw_entry_kernel(uint64_t n, const uint64_t *first, const uint64_t *count,
		      const uint64_t *name_len, const uint64_t *usize, const uint64_t *pc_off,
		      const uint64_t *pc_n, const uint64_t *out_n, const uint32_t *crcs,
		      uint64_t *e_info, uint64_t *sizes);
extern "C" __global__ void
lda_zipw_place_kernel(uint64_t n, uint32_t zip64, uint32_t dos_datetime, uint64_t out_avail,
		      uint64_t tail, const uint64_t *first, const uint64_t *count,
		      const uint64_t *name_off, const uint64_t *name_len, const uint64_t *cen,
		      const uint64_t *usize, const uint64_t *uoff, const uint8_t *names,
		      const uint64_t *pc_off, const uint64_t *pc_n, const uint64_t *slot_off,
		      const uint64_t *out_n, const uint64_t *e_info, const uint64_t *offsets,
		      const uint64_t *block_sums, uint8_t *out, uint64_t *cp_src, uint64_t *cp_dst,
		      uint64_t *cp_len, uint64_t *index);
extern "C" __global__ void
lda_zipw_copy_kernel(uint64_t np, const uint64_t *total_at, uint64_t out_avail, uint64_t tail,
		     const uint64_t *cp_src, const uint64_t *cp_dst, const uint64_t *cp_len,
		     const uint8_t *in, const uint8_t *slots, uint8_t *out);
extern "C" __global__ void
lda_zipw_final_kernel(uint64_t n, uint32_t zip64, uint64_t out_avail, uint64_t cd_size,
		      uint64_t tail, const uint64_t *usize, const uint64_t *e_info,
		      const uint64_t *total_at, uint8_t *out, uint64_t *result);

/* gzip_members_write_kernels.hip: a file of gzip members assembled in device
 * memory (host_gzip_members_write.hip, gzip_members_write_plan.h); the pieces
 * are copied by lda_zipw_copy_kernel */
extern "C" __global__ void
lda_gzmw_member_kernel(uint64_t n, const uint64_t *first, const uint64_t *count,
		       const uint64_t *name_len, const uint64_t *usize, const uint64_t *pc_off,
		       const uint64_t *pc_n, const uint64_t *out_n, const uint32_t *crcs,
		       uint64_t *csize, uint32_t *crc, uint64_t *sizes);
extern "C" __global__ void
lda_gzmw_place_kernel(uint64_t n, int level, uint32_t mtime, uint64_t out_avail,
		      const uint64_t *first, const uint64_t *count, const uint64_t *name_off,
		      const uint64_t *name_len, const uint64_t *usize, const uint64_t *uoff,
		      const uint8_t *names, const uint64_t *pc_off, const uint64_t *pc_n,
		      const uint64_t *slot_off, const uint64_t *out_n, const uint64_t *csize,
		      const uint32_t *crc, const uint64_t *offsets, const uint64_t *block_sums,
		      uint8_t *out, uint64_t *cp_src, uint64_t *cp_dst, uint64_t *cp_len,
		      uint64_t *index);
extern "C" __global__ void
lda_gzmw_final_kernel(uint64_t n, uint64_t usize_total, uint64_t out_avail,
		      const uint64_t *total_at, uint64_t *result, uint64_t *index);

/* tar_write_kernels.hip: a tar archive written into device memory from the
 * rows of tar_write_plan.h (host_tar_write.hip), one workgroup per tile */
#define LDA_TARW_TILE 65536	/* bytes of the archive per tile */
#define LDA_TARW_E_OFF 0	/* the words of an entry's row: TARW_E_* of tar_write_plan.h */
#define LDA_TARW_E_PAX 1
#define LDA_TARW_E_NAME_OFF 2
#define LDA_TARW_E_NAME_LEN 3
#define LDA_TARW_E_SRC 4
#define LDA_TARW_E_SIZE 5
#define LDA_TARW_ECOLS 6
extern "C" __global__ void
lda_tarw_pack_kernel(uint64_t n, uint64_t end, uint64_t total, uint64_t mtime,
		     const uint64_t *rows, const uint8_t *names, const uint8_t *in,
		     uint8_t *out);

/* png_kernels.hip: PNG files read from device memory (host_png.hip): the chunk
 * walk, one lane per file; the IDAT payloads of a selection gathered into one
 * zlib stream, one workgroup per selection; the scanline filters undone behind
 * the zlib batch decode, one wave per selection; the verdicts merged.  The
 * c_* columns are those of png_plan.h.  Copies of the header's constants
 * (static_assert in host_png.hip) */
#define LDA_PNG_UNSUPPORTED 18		/* LIBDEFLATE_AMD_PNG_UNSUPPORTED */
#define LDA_PNG_WORDS 8
#define LDA_PNG_META_LE16 0x100		/* meta: LIBDEFLATE_AMD_PNG_LE16 << 8, 16-bit images */
#define LDA_PNG_META_ALT 0x200		/* meta: the unfilter writes at alt_base + c_out_off */
#define LDA_PNG_ADAM7 2			/* LIBDEFLATE_AMD_PNG_ADAM7: the index takes interlace 1 */
extern "C" __global__ void
lda_png_index_kernel(uint64_t n_files, uint32_t flags, const uint8_t *in, const uint64_t *in_off,
		     const uint64_t *in_n, uint64_t *rows, int32_t *results);
extern "C" __global__ void
lda_png_gather_kernel(uint64_t n_sel, const uint64_t *c_idat, const uint64_t *c_end,
		      const uint64_t *c_zsum, const uint64_t *c_zoff, const uint8_t *in,
		      uint8_t *ws, int32_t *flags);
extern "C" __global__ void
lda_png_unfilter_kernel(uint64_t n_sel, const uint64_t *c_raw_off, const uint64_t *c_raw_n,
			const uint64_t *c_out_off, const uint64_t *c_geom, const uint64_t *c_meta,
			const uint8_t *ws, uint8_t *out_base, uint8_t *alt_base, int32_t *flags);
extern "C" __global__ void
lda_png_final_kernel(uint64_t n_sel, const uint64_t *c_meta, const int32_t *gather,
		     const int32_t *decode, const int32_t *unfilter, int32_t *results);

/* png_pixels_kernels.hip: the selections of a PNG decode that are not yet the
 * target pixel format converted from the scratch into their rooms
 * (host_png_pixels.hip): tiles of LDA_PNGX_TILE pixels, the grid strides over
 * them; the verdicts merged.  The x_* columns are png_pixels_plan.h's of the
 * converted selections, c_src is PNG_COL_OUT_OFF of all selections */
#define LDA_PNGX_TILE 4096		/* pixels: 256 threads x 16 */
#define LDA_PNGX_OUT16 0x10		/* LIBDEFLATE_AMD_PNG_OUT16 */
#define LDA_PNGX_KIND_KEY 0x10000	/* kind: the tRNS is a colour key */
extern "C" __global__ void
lda_pngx_convert_kernel(uint64_t n_conv, uint64_t n_tiles, uint32_t format, uint32_t le16,
			const uint64_t *x_tile_end, const uint64_t *x_sel, const uint64_t *c_src,
			const uint64_t *x_dst, const uint64_t *x_shape, const uint64_t *x_kind,
			const uint64_t *x_plte, const uint64_t *x_trns, const uint8_t *in,
			const uint8_t *ws, uint8_t *out_base, int32_t *flags);
extern "C" __global__ void
lda_pngx_final_kernel(uint64_t n_sel, const uint64_t *c_meta, const int32_t *gather,
		      const int32_t *decode, const int32_t *unfilter, const int32_t *convert,
		      int32_t *results);

/* png_adam7_kernels.hip: Adam7-interlaced selections of a PNG decode
 * (host_png_adam7.hip): the pass images the unfilter left in the scratch woven
 * into the finished images, tiles of LDA_PNG7_TILE 16-byte pieces, the grid
 * strides over them; the verdicts merged over every selection's units.  The
 * d_* columns are png_adam7_plan.h's of the interlaced selections (d_pass:
 * seven words a selection), c_units its PNG7_COL_UNITS */
#define LDA_PNG7_TILE 1024		/* pieces: 256 threads x 4 */
#define LDA_PNG7_KIND_ALT 0x100		/* kind: d_dst counts from the scratch */
extern "C" __global__ void
lda_png7_deinterlace_kernel(uint64_t n_il, uint64_t n_tiles, const uint64_t *d_tile_end,
			    const uint64_t *d_pass, const uint64_t *d_shape, const uint64_t *d_kind,
			    const uint64_t *d_dst, uint8_t *ws, uint8_t *out_base);
extern "C" __global__ void
lda_png7_final_kernel(uint64_t n_sel, const uint64_t *c_meta, const uint64_t *c_units,
		      const int32_t *gather, const int32_t *decode, const int32_t *unit_flags,
		      const int32_t *convert, int32_t *results);

/* png_write_kernels.hip: PNG files written into device memory
 * (host_png_write.hip, png_write_plan.h): the scanlines filtered into the
 * scratch, 4, 16 or 64 lanes per row; behind the checksum and compress
 * batches the files sized and placed, a wave per image; the pieces are copied
 * by lda_zipw_copy_kernel */
extern "C" __global__ void
lda_pngw_filter4_kernel(uint64_t n, uint64_t n_items, uint32_t filter, const uint64_t *work,
			const uint64_t *icols, const uint8_t *in, uint8_t *scan);
extern "C" __global__ void
lda_pngw_filter16_kernel(uint64_t n, uint64_t n_items, uint32_t filter, const uint64_t *work,
			 const uint64_t *icols, const uint8_t *in, uint8_t *scan);
extern "C" __global__ void
lda_pngw_filter64_kernel(uint64_t n, uint64_t n_items, uint32_t filter, const uint64_t *work,
			 const uint64_t *icols, const uint8_t *in, uint8_t *scan);
extern "C" __global__ void
lda_pngw_image_kernel(uint64_t n, uint64_t np, uint32_t crc_head, const uint64_t *icols,
		      const uint64_t *pcols, const uint64_t *out_n, const uint32_t *adlers,
		      const uint32_t *crcs, uint64_t *csize, uint32_t *adler, uint32_t *crc,
		      uint64_t *sizes);
extern "C" __global__ void
lda_pngw_place_kernel(uint64_t n, uint64_t np, int level, uint64_t out_avail,
		      const uint64_t *icols, const uint64_t *pcols, const uint64_t *out_n,
		      const uint64_t *csize, const uint32_t *adler, const uint32_t *crc,
		      const uint64_t *offsets, const uint64_t *block_sums, const uint8_t *in,
		      uint8_t *out, uint64_t *cp_src, uint64_t *cp_dst, uint64_t *cp_len,
		      uint64_t *index);
extern "C" __global__ void
lda_pngw_final_kernel(uint64_t n, uint64_t pixels_total, uint64_t out_avail,
		      const uint64_t *total_at, uint64_t *result);

/* shuffle_kernels.hip: byte-shuffled deflate chunks (HDF5, NetCDF-4, Zarr;
 * host_shuffle.hip, host_shuffle_write.hip): the byte transpose over many ragged
 * chunks and its inverse, tiles of consecutive elements of one chunk, the grid
 * strides over them; the reader's verdicts merged; the writer's streams sized
 * and placed, a wave per chunk, their pieces copied by lda_zipw_copy_kernel.
 * The u_* columns are shuffle_plan.h's SHUF_UCOLS.  Copies of the header's and
 * the plan's constants (static_assert in host_shuffle.hip) */
#define LDA_SHUF_TILE 4096		/* elements of a tile, es 1, 2, 4, 8: 256 threads x 16 */
#define LDA_SHUF_GEN_BYTES 16384	/* any other es: a tile is (this / es) & ~15 elements */
#define LDA_SHUF_SRC_ALT ((uint64_t)1 << 63)	/* u_src counts from the second base */
#define LDA_SHUF_VERD_OWN ((uint64_t)1 << 63)	/* verd: the row's own verdict in the low bits */
extern "C" __global__ void
lda_unshuffle_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *u_tile_end,
		     const uint64_t *u_src, const uint64_t *u_dst, const uint64_t *u_geom,
		     const uint8_t *ws, const uint8_t *alt, uint8_t *out);
extern "C" __global__ void
lda_shuf_final_kernel(uint64_t n, const uint64_t *verd, const int32_t *decode, int32_t *results);
extern "C" __global__ void
lda_shuffle_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *u_tile_end,
		   const uint64_t *u_src, const uint64_t *u_dst, const uint64_t *u_geom,
		   const uint8_t *in, uint8_t *rooms);
/* first, count, usize: columns 0 - 2 of every chunk writer's ecols, CHUNKW_E_FIRST, _COUNT and
 * _USIZE of chunk_plan.h - what the comments in shuffle_kernels.hip and exr_kernels.hip still
 * call SHUFW_E_FIRST, _COUNT, _USIZE and EXRW_E_USIZE */
extern "C" __global__ void
lda_shufw_chunk_kernel(uint64_t n, int format, const uint64_t *first, const uint64_t *count,
		       const uint64_t *usize, const uint64_t *pc_off, const uint64_t *pc_n,
		       const uint64_t *out_n, const uint32_t *sums, uint64_t *csize, uint32_t *sum,
		       uint64_t *sizes);
extern "C" __global__ void
lda_shufw_place_kernel(uint64_t n, int format, int level, uint64_t out_avail,
		       const uint64_t *ecols, const uint64_t *pc_off, const uint64_t *pc_n,
		       const uint64_t *slot_off, const uint64_t *out_n, const uint64_t *csize,
		       const uint32_t *sum, const uint64_t *offsets, const uint64_t *block_sums,
		       uint8_t *out, uint64_t *cp_src, uint64_t *cp_dst, uint64_t *cp_len,
		       uint64_t *index);
extern "C" __global__ void
lda_shufw_final_kernel(uint64_t n, uint64_t raw_total, uint64_t out_avail,
		       const uint64_t *total_at, uint64_t *result);

/* tiff_kernels.hip: predictor-coded deflate strips and tiles (TIFF, GeoTIFF;
 * host_tiff.hip, host_tiff_write.hip): the per-row, per-channel prefix sums
 * over the kept rows of many segments, groups of 4, 16 or 64 lanes a row, the
 * grid strides over quads of lanes; the floating-point predictor's gather from
 * the byte planes; the forward differences into the writer's rooms, tiles of
 * LDA_TIFF_PTILE bytes; the writer's index rows.  The k_* and g_* columns are
 * tiff_plan.h's TIFF_KCOLS and TIFF_GCOLS, ecols its TIFFW_ECOLS; the reader's
 * verdicts and the writer's assembly are shuffle_kernels.hip's.  Copies of the
 * header's and the plan's constants (static_assert in host_tiff.hip) */
#define LDA_TIFF_WORDS 8
#define LDA_TIFF_SPP_MAX 16
#define LDA_TIFF_PTILE 4096		/* bytes of a room a workgroup predicts: 256 threads x 16 */
#define LDA_TIFF_DST_WS ((uint64_t)1 << 63)	/* k_dst counts from the scratch: a scan in place */
extern "C" __global__ void
lda_tiff_unpredict_kernel(uint64_t n_k, uint64_t n_quads, const uint64_t *kcols, uint8_t *ws,
			  uint8_t *out);
extern "C" __global__ void
lda_tiff_gather_kernel(uint64_t n_g, uint64_t n_tiles, const uint64_t *g_tile_end,
		       const uint64_t *g_src, const uint64_t *g_dst, const uint64_t *g_dpitch,
		       const uint64_t *g_geom, const uint64_t *g_plane, const uint8_t *ws,
		       uint8_t *out);
extern "C" __global__ void
lda_tiff_predict_kernel(uint64_t n, uint64_t n_tiles, const uint64_t *ecols, const uint8_t *in,
			uint8_t *rooms);
extern "C" __global__ void
lda_tiffw_index_kernel(uint64_t n, uint64_t out_avail, const uint64_t *ecols,
		       const uint64_t *csize, const uint64_t *offsets, const uint64_t *block_sums,
		       uint64_t *index);

/* exr_kernels.hip: OpenEXR's ZIP and ZIPS chunks (host_exr.hip,
 * host_exr_write.hip): the byte-wise running sum over a whole chunk and the
 * interleave of its halves undone in three launches - stretch sums, their
 * carries per chunk, the tiles -, a wave a tile of LDA_EXR_TILE raw bytes; the
 * raw chunk laid out as lines at a pitch or as interleaved pixels, and
 * gathered back, in tiles of LDA_EXR_LTILE items; the forward coding in tiles
 * of LDA_EXR_CTILE bytes; the writer's choice between stream and raw and its
 * placement.  ucols, lcols and ecols are exr_plan.h's EXR_UCOLS, EXR_LCOLS and
 * EXRW_ECOLS; the reader's verdicts and the writer's sizes and result are
 * shuffle_kernels.hip's.  Copies of the header's and the plan's constants
 * (static_assert in host_exr.hip) */
#define LDA_EXR_WORDS 10
#define LDA_EXR_LAYOUT_LINES 0
#define LDA_EXR_LANE 32			/* raw bytes a lane undoes */
#define LDA_EXR_TILE 2048		/* raw bytes a wave undoes */
#define LDA_EXR_WG_TILES 4		/* tiles of a workgroup of 256 */
#define LDA_EXR_LTILE 256		/* items of a layout tile */
#define LDA_EXR_CTILE 4096		/* bytes of a coded room a workgroup makes: 256 threads x 16 */
#define LDA_EXRW_E_WORDS 5		/* the column of a row's word 2 in ecols */
#define LDA_EXR_DST_OUT ((uint64_t)1 << 63)	/* u_dst counts from d_out, not from the raw area */
#define LDA_EXR_RAW_IN ((uint64_t)1 << 63)	/* l_raw counts from d_in, not from the raw area */
extern "C" __global__ void
lda_exr_sums_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *ucols, const uint8_t *coded,
		    uint32_t *slots);
extern "C" __global__ void
lda_exr_carry_kernel(uint64_t n_u, const uint64_t *u_tile_end, uint32_t *slots);
extern "C" __global__ void
lda_exr_undo_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *ucols, const uint8_t *coded,
		    const uint32_t *slots, uint8_t *raw, uint8_t *out);
extern "C" __global__ void
lda_exr_layout_kernel(uint64_t n_l, uint64_t n_tiles, const uint64_t *lcols, const uint8_t *in,
		      const uint8_t *raw, uint8_t *out);
extern "C" __global__ void
lda_exr_gather_kernel(uint64_t n_l, uint64_t n_tiles, const uint64_t *lcols, const uint8_t *in,
		      uint8_t *raw);
extern "C" __global__ void
lda_exr_code_kernel(uint64_t n, uint64_t n_tiles, const uint64_t *ecols, const uint8_t *raw_area,
		    uint8_t *coded_area);
extern "C" __global__ void
lda_exrw_choose_kernel(uint64_t n, const uint64_t *ecols, uint64_t *dsize, uint64_t *sizes);
extern "C" __global__ void
lda_exrw_place_kernel(uint64_t n, int level, uint64_t out_avail, const uint64_t *ecols,
		      const uint64_t *pc_off, const uint64_t *pc_n, const uint64_t *slot_off,
		      const uint64_t *out_n, const uint64_t *csize, const uint32_t *sum,
		      const uint64_t *dsize, const uint64_t *offsets, const uint64_t *block_sums,
		      uint8_t *out, uint64_t *cp_src, uint64_t *cp_dst, uint64_t *cp_len,
		      uint64_t *index);

/* parquet_kernels.hip: the pages of flat Parquet column chunks
 * (host_parquet.hip): the runs of every data page's hybrid streams listed, a
 * wave a page; the slots of all pages expanded in tiles of LDA_PQ_TILE; the
 * verdicts merged.  ucols and vcols are parquet_plan.h's PQ_UCOLS and PQ_VCOLS;
 * `runs` holds records of LDA_PQ_RUN_WORDS words, `info` LDA_PQ_INFO_WORDS
 * words per data page.  Copies of the header's and the plan's constants
 * (static_assert in host_parquet.hip) */
#define LDA_PQ_TILE 1024		/* slots of an expand tile: 256 threads x 4 */
#define LDA_PQ_LEVEL_PIECE 512		/* values of a piece of a bit-packed level run */
#define LDA_PQ_RUN_WORDS 4
#define LDA_PQ_INFO_WORDS 8
#define LDA_PQ_DATA_V2 3
#define LDA_PQ_PLAIN 0
#define LDA_PQ_IN_PLACE ((uint64_t)1 << 63)	/* a section counts from d_in, not from the rooms */
#define LDA_PQ_F_SKIP ((uint64_t)1 << 31)	/* u_fields: the page's dictionary is too short */
#define LDA_PQ_V_IS_DICT ((uint64_t)1 << 63)	/* v_own: a dictionary page's own verdict */
enum {
	LDA_PQ_U_SLOT_END = 0, LDA_PQ_U_SEC, LDA_PQ_U_SEC_N, LDA_PQ_U_LEV, LDA_PQ_U_LEV_N,
	LDA_PQ_U_FIELDS, LDA_PQ_U_COUNT, LDA_PQ_U_OUT, LDA_PQ_U_VALID, LDA_PQ_U_DICT,
	LDA_PQ_U_DICT_N, LDA_PQ_U_LRUNS, LDA_PQ_U_LCAP, LDA_PQ_U_IRUNS, LDA_PQ_U_ICAP, LDA_PQ_UCOLS,
	LDA_PQ_V_Z = 0, LDA_PQ_V_OWN, LDA_PQ_V_DICT
};
extern "C" __global__ void
lda_pq_runs_kernel(uint64_t n_u, const uint64_t *ucols, const int32_t *decode, const uint8_t *in,
		   const uint8_t *rooms, uint4 *runs, uint32_t *info);
extern "C" __global__ void
lda_pq_expand_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *ucols, const uint8_t *in,
		     const uint8_t *rooms, const uint4 *runs, uint32_t *info, uint8_t *out,
		     uint8_t *valid);
extern "C" __global__ void
lda_pq_final_kernel(uint64_t n, const uint64_t *vcols, const int32_t *decode, const uint32_t *info,
		    int32_t *results);

/* parquet_strings_kernels.hip: the BYTE_ARRAY pages of
 * libdeflate_amd_parquet_decode_batch_ex - the starts of the length-prefixed
 * values of every walk section listed, a wave a section; the lengths of the
 * string slots summed per tile of LDA_PQ_TILE, placed by the scan and written
 * as int64 entries; the bytes gathered; the verdicts added.  wcols, scols and
 * svcols are parquet_strings_plan.h's PQS_WCOLS, PQS_SCOLS and PQS_VCOLS;
 * `walks` holds two words per walk section (failed, the
 * values owed) and behind them the start lists; `sums` the tile sums, their
 * places and the scan's block sums; `places` per string slot its length and
 * then its place in d_bytes, the total behind the last, and then per slot where
 * its bytes lie.
 * Copies of the plan's constants (static_assert in host_parquet.hip) */
enum {
	LDA_PQS_W_SEC = 0, LDA_PQS_W_SEC_N, LDA_PQS_W_Z, LDA_PQS_W_U, LDA_PQS_W_COUNT, LDA_PQS_W_STARTS,
	LDA_PQS_W_CAP, LDA_PQS_WCOLS,
	LDA_PQS_S_SLOT_END = 0, LDA_PQS_S_U, LDA_PQS_S_WALK, LDA_PQS_S_STARTS, LDA_PQS_SCOLS,
	LDA_PQS_V_S = 0, LDA_PQS_V_WALK, LDA_PQS_V_DWALK, LDA_PQS_VCOLS
};
extern "C" __global__ void
lda_pqs_walk_kernel(uint64_t n_w, const uint64_t *wcols, const int32_t *decode, const uint32_t *info,
		    const uint8_t *in, const uint8_t *rooms, uint32_t *walks);
extern "C" __global__ void
lda_pqs_sum_kernel(uint64_t n_u, uint64_t n_s, uint64_t n_tiles, const uint64_t *ucols,
		   const uint64_t *scols, const uint8_t *in, const uint8_t *rooms, const uint4 *runs,
		   uint32_t *info, const uint32_t *walks, uint64_t *sums, uint8_t *valid,
		   uint64_t *places);
extern "C" __global__ void
lda_pqs_offsets_kernel(uint64_t n_u, uint64_t n_s, uint64_t n_tiles, const uint64_t *ucols,
		       const uint64_t *scols, const uint64_t *sums, uint8_t *out, uint64_t *places);
extern "C" __global__ void
lda_pqs_copy_kernel(uint64_t n_s, const uint64_t *scols, const uint64_t *places, const uint8_t *in,
		    const uint8_t *rooms, uint8_t *bytes, uint64_t bytes_avail);
extern "C" __global__ void
lda_pqs_final_kernel(uint64_t n, uint64_t n_u, uint64_t n_s, const uint64_t *svcols,
		     const uint64_t *ucols, const uint64_t *scols, const uint32_t *winfo,
		     const uint64_t *ent, const uint64_t *total, uint64_t bytes_avail, uint8_t *out,
		     uint64_t *bytes_total, int32_t *results);

/* selfcheck_kernels.hip: the hardware behaviours the kernels rely on, checked
 * per device (counters: [0] lanes, [1] order mismatches, [2] same-instruction
 * conflicts seen, [3] loads, [4] stale loads) */
extern "C" __global__ void
lda_selfcheck_lds_order_kernel(uint64_t *counters);
extern "C" __global__ void
lda_selfcheck_visibility_kernel(uint8_t *buf, uint64_t *counters);
extern "C" size_t lda_selfcheck_region_bytes(void);

/* CRC constant tables, generated on the host at first use (host_context.hip) */
#define LDA_CRC_TABLE_WORDS (17 * 256)
#define LDA_CRC_XPOW_WORDS 1024

#endif /* LDA_KERNELS_H */
