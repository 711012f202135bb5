/*
 * deflate_entropy.hip - the entropy stage of the 64 KiB compress kernel: the
 * streams of a batch whose LZ77 stage (lda_deflate_batch_kernel) has left the
 * tokens of every buffer and one descriptor per block in HBM (kernels.h,
 * LDA_BLK_*).  One workgroup of 256 threads per buffer (claimed from a counter
 * as the workgroup starts) writes its container
 * header, its blocks in order (a block's bit offset - so its stored padding
 * and its cost - depends on the block before it), the empty stored block of a
 * segment other than the last, and the trailer.  Each block goes through
 * block_emit() of deflate_blockend.h, the code the fused kernels run inside
 * their tile loop: rank sort, make_code() for both alphabets, the precode,
 * the exact dynamic / static / stored cost, the header, the token encode.
 *
 * Why a kernel of its own: the block end needs none of the LZ77 window state
 * that fills a CU's LDS (the input ring, the chains) and most of it is
 * latency-bound work on one or two waves (the tree merges are one lane) while
 * the others wait at barriers.  Inside the tile loop it held a 1024-thread
 * workgroup that owned the whole CU.  Here it needs 20 KiB of LDS and few
 * registers, so several buffers' block ends share a CU and one buffer's
 * serial tree build runs beside another's token encode - the arrangement of
 * deflate_small.hip, for the same reason.
 */
#include <stddef.h>
#include "device_common.h"
#include "kernels.h"

#define LDA_ENTROPY 1
#define NT LDA_DEFLATE_ENTROPY_THREADS
#define VPT (1024 / NT)
#define NWAVES (NT / 64)
/* __launch_bounds__' second argument: the waves per EU (SIMD) the registers
 * are held for - with one wave per SIMD per workgroup (NT 256) the workgroups
 * per CU, which the LDS is checked against below */
#ifndef ENTROPY_WGS
#define ENTROPY_WGS 4
#endif
static_assert(NT == 256, "ENTROPY_WGS waves per EU are ENTROPY_WGS workgroups per CU");
#define TOK_MATCH 0x80000000u
/* bit staging: a window of 4 * NT tokens is at most 48 * 4 * NT bits (6 KiB,
 * held by a static_assert next to the encode loop in deflate_blockend.h); a
 * stored piece goes through in 2 KiB steps */
#define STG_WORDS 2044

struct deflate_lds {
	u32 M[1776];		/* keys, run starts; the litlen tree's scratch from M + 512; S6: the encode tables (deflate_blockend.h) */
	u32 freq[320];		/* litlen 0..287, offset 288..319 */
	u8 lens[320];
	u16 codes[320];		/* bit-reversed codewords */
	u16 sorted[288];
	u32 hw[288];		/* the offset tree's scratch */
	u16 pre_items[320 + 8];	/* precode symbol | extra << 5 */
	u32 pre_freq[19];
	u8 pre_lens[20];
	u16 pre_codes[20];
	u32 nxtA[STG_WORDS + 8] __attribute__((aligned(16)));	/* bit staging (the fused kernels' name) */
	u32 scan[2][NWAVES + 1];
	u32 carry[6];		/* staging bytes kept between blocks */
	u32 vars[4];
};
static_assert(sizeof(struct deflate_lds) * ENTROPY_WGS <= 163840, "ENTROPY_WGS workgroups per CU");

#ifdef __HIP_DEVICE_COMPILE__
#define AS3 __attribute__((address_space(3)))
#else
#define AS3
#endif
typedef AS3 struct deflate_lds lds_t;

enum { V_TMP1 = 0, V_TMP2, V_TMP3, V_NPRE, V_COUNT };
static_assert(V_COUNT <= sizeof(((struct deflate_lds *)0)->vars) / sizeof(u32), "vars[] holds them all");

#include "deflate_huffman.h"
#include "deflate_blockend.h"

extern "C" __global__ void __launch_bounds__(NT, ENTROPY_WGS)
lda_deflate_entropy_kernel(u64 n_chunks, int format, int level,
			   const u8 *__restrict__ in_base, const u64 *__restrict__ in_offsets,
			   const u64 *__restrict__ in_nbytes, u8 *__restrict__ out_base,
			   const u64 *__restrict__ out_offsets,
			   const u64 *__restrict__ out_avail_arr, u64 *__restrict__ out_nbytes,
			   const u32 *__restrict__ sums, const u32 *__restrict__ seg_info,
			   const u32 *__restrict__ tok_buf, const u32 *__restrict__ blk_buf,
			   u32 tok_stride, u32 blk_stride, u32 *__restrict__ next_chunk)
{
	extern __shared__ __attribute__((aligned(16))) u8 lds_raw[];
	lds_t *L = (lds_t *)(uintptr_t)0;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if ((u32)(uintptr_t)(__attribute__((address_space(3))) u8 *)lds_raw != 0)
		__builtin_trap();	/* the LDS block is addressed from 0, as in the fused kernels */
	/* Buffers are claimed in the order the workgroups start, not by
	 * blockIdx: consecutive workgroup ids go round the XCDs, so with
	 * c = blockIdx.x every eighth buffer of the batch runs on the same
	 * XCD, and a batch whose buffers differ with that period (one stored
	 * 64 KiB buffer in eight takes twice a text buffer's time) leaves one
	 * XCD working when seven are done.  *next_chunk is zero before the
	 * launch; nobody waits for anybody. */
	if (tid == 0)
		L->vars[V_TMP1] = atomicAdd(next_chunk, 1u);
	__syncthreads();
	const u64 c = (u32)__builtin_amdgcn_readfirstlane((int)L->vars[V_TMP1]);
	if (c >= n_chunks)
		return;
	const u32 nb = blk_buf[c];
	if (nb == LDA_BLK_FUSED)
		return;		/* above the bound: the fused kernel behind this one writes it */
	const u32 *__restrict__ desc = blk_buf + LDA_BLK_HDR_WORDS(n_chunks) +
				       c * blk_stride * LDA_BLK_WORDS;
	const u32 *__restrict__ tokg = tok_buf + c * tok_stride;
	const u8 *__restrict__ inp = in_base + in_offsets[c];
	const u32 n = (u32)in_nbytes[c];	/* (checked by the LZ77 stage) */
	const bool seg_last = seg_info ? seg_info[c] >> 31 : true;
	const u32 hdr_bytes = format == LDA_FMT_GZIP ? 10 : format == LDA_FMT_BGZF ? 18 :
			      format == LDA_FMT_ZLIB ? 2 : 0;
	const u32 ftr_bytes = format == LDA_FMT_GZIP || format == LDA_FMT_BGZF ? 8 :
			      format == LDA_FMT_ZLIB ? 4 : 0;
	bool overflow = nb == LDA_BLK_OVERFLOW;
	struct outstate os;
	os.out = out_base + out_offsets[c];
	os.avail = out_avail_arr[c];
	if (format == LDA_FMT_BGZF && os.avail > LDA_BGZF_MEMBER_MAX)
		os.avail = LDA_BGZF_MEMBER_MAX;	/* (the LZ77 stage refused a larger block) */
	os.sg = (u64)(0 - ((uintptr_t)os.out & 15));
	os.bits = 0;
	u32 tog = 0;

	for (u32 i = tid; i < STG_WORDS + 8; i += NT)
		stg_of(L)[i] = 0;
	__syncthreads();
	if (!overflow && hdr_bytes)
		put_container_header(L, &os, format, level, NULL, hdr_bytes, tid);
	__syncthreads();
	stg_save(L, &os);

	for (u32 b = 0; b < nb && !overflow; b++) {
		const u32 *__restrict__ d = desc + (size_t)b * LDA_BLK_WORDS;
		for (u32 i = tid; i < 320; i += NT)
			L->freq[i] = d[LDA_BLK_FREQ + i];
		const u32 tok0 = d[LDA_BLK_TOK0], ntok = d[LDA_BLK_NTOK];
		const u32 bstart = d[LDA_BLK_START], bend = d[LDA_BLK_END];
		const u32 flags = d[LDA_BLK_FLAGS];
		__syncthreads();
		if (!block_emit(L, &os, tokg + tok0, ntok, inp, bstart, bend - bstart, flags & 1,
				(flags & LDA_BLK_STORED) != 0, ftr_bytes, &tog, tid, lane, wave))
			overflow = true;
	}
	finish_stream(L, &os, overflow, seg_last, format, ftr_bytes, sums, c, n, out_nbytes, tid);
}

extern "C" size_t lda_deflate_entropy_lds_bytes(void)
{
	return sizeof(struct deflate_lds);
}

LDA_PROF_DEFINE_READER(libdeflate_amd_profile_read_deflate_entropy)
