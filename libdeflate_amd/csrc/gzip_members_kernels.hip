/*
 * gzip_members_kernels.hip - reading a file of concatenated gzip members
 * (`cat a.gz b.gz`, WARC, mgzip / pgzip output) that lies in device memory:
 * where its members are, the descriptors of ONE decompress batch that puts
 * every member at its final place, the file's result words and index
 * (host_gzip_members.hip; tools/models/gzip_chain.py is the CPU model of the
 * finder, and the tests run it on the same files).
 *
 * Unlike a BGZF member (bgzf_read_kernels.hip) a plain gzip member does not
 * say how long it is: its end is known once its DEFLATE stream has been
 * parsed.  So the finder speculates:
 *
 *   lda_gzm_scan_kernel     every byte offset p against the candidate rule -
 *                           1f 8b 08, FLG & 0xE0 == 0, p + 18 <= n -: counted
 *                           per 16 KiB of file, then - after the scan kernels
 *                           of compact_kernels.hip - written in file order
 *                           (host_finder.h launches the passes).
 *                           Candidates are not members: a stored block, a
 *                           FNAME or plain chance carries the three bytes.
 *   lda_gzm_slots_kernel    one size query (lda_inflate_sizes_kernel, GZIP)
 *                           over ALL candidates: slot i is [p_i, n), the rest
 *                           of the file - the count mode of the decoder stops
 *                           at the member's footer and reports actual_in and
 *                           the size, with nothing written.  A candidate whose
 *                           FNAME + FCOMMENT run past LDA_GZM_NAME_MAX bytes
 *                           gets no input: that bounds what one lane walks
 *                           for a header, whatever the file holds.
 *   lda_gzm_size32_kernel   a candidate's size as the chain kernels want it:
 *                           actual_in as u32, 0 where the count failed.
 *   lda_bgzf_jump_kernel / lda_bgzf_top_kernel / lda_bgzf_members_kernel
 *                           (bgzf_read_kernels.hip, launched by host_finder.h)
 *                           keep the candidates that the chain from offset 0
 *                           reaches.
 *   lda_gzm_break_kernel    where a broken chain stopped, and so its verdict.
 *   lda_gzm_msize_kernel    the counted size of every member.
 *   lda_gzm_desc_kernel     behind the scan of the sizes: the batch's
 *                           descriptors and the index.
 *   lda_gzm_final_kernel    one workgroup: the five result words, the closing
 *                           index pair.
 * (The heads of the members, libdeflate_amd_gzip_members_peek_batch, are a
 * prefix batch over the index this reader wrote: lda_gzm_peek_desc_kernel in
 * inflate_prefix.hip.)
 *
 * The input is hostile by definition: every load is checked against n, every
 * index against the candidate count, and no loop of these kernels takes its
 * bound from the file.  The worst case of the speculation is in the count:
 * per candidate a header of at most 64 KiB + LDA_GZM_NAME_MAX bytes walked
 * by one lane (header_bounded() below is what bounds it), and a DEFLATE parse
 * that runs until the candidate's stream breaks or ends.
 */
#include "device_common.h"
#include "kernels.h"

#define SIG24 0x00088b1fu	/* 1f 8b 08, and a FLG without reserved bits */
#define SIG_MASK 0xE0FFFFFFu
#define MIN_MEMBER 18u

/* pre-decode verdict from the finder's state, the sum of the counted sizes and
 * the caller's limits; precedence as include/libdeflate_amd.h states it */
static __device__ __forceinline__ u32
pre_status(const u32 *__restrict__ state, u64 K, u64 cap, u64 total, u64 out_avail,
	   u64 max_members)
{
	if (K > cap)
		return LDA_GZM_MORE_CANDIDATES;
	if (!state[LDA_BR_CHAIN])
		return state[LDA_GZM_BREAK];
	if (state[LDA_BR_MEMBERS] > max_members)
		return LDA_BR_MORE;
	if (total > out_avail)
		return LDA_INSUFFICIENT_SPACE;
	return LDA_SUCCESS;
}

/*
 * One workgroup per LDA_BR_SCAN_WG bytes of file, in steps of 4 KiB: 16
 * bytes per thread into LDS (and 16 more behind the tile; the next step's are
 * on their way while this step's are tested), every offset's four bytes
 * against the rule.  Candidates can stand 3 bytes apart, so a thread holds up
 * to 6 of them (a 16-bit mask) and a step up to 1366.
 * offsets == NULL: counts[wg] = candidates of the workgroup's range.
 * Otherwise offsets / block_sums are the scan of the counts, and the
 * candidates below index cap are written in file order.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_scan_kernel(const u8 *__restrict__ in, u64 n, u64 *__restrict__ counts,
		    const u64 *__restrict__ offsets, const u64 *__restrict__ block_sums,
		    u64 cap, u64 *__restrict__ cand_pos)
{
	__shared__ __attribute__((aligned(16))) u32 tile[LDA_BR_TILE / 4 + 4];
	__shared__ u32 wsum[4];
	const u32 tid = threadIdx.x;
	const u64 wg0 = (u64)blockIdx.x * LDA_BR_SCAN_WG;
	u64 at = 0;	/* candidates of this workgroup so far / where they go */

	if (offsets) {
		if (counts[blockIdx.x] == 0)
			return;
		at = offsets[blockIdx.x] + block_sums[blockIdx.x / LDA_SCAN_BLOCK];
	}
	uint4 mine = load16_guard(in, wg0 + 16 * (u64)tid, n);
	uint4 behind = { 0, 0, 0, 0 };
	if (tid == 0)
		behind = load16_guard(in, wg0 + LDA_BR_TILE, n);
	for (u32 s = 0; s < LDA_BR_SCAN_WG / LDA_BR_TILE; s++) {
		const u64 base = wg0 + (u64)s * LDA_BR_TILE;
		if (base >= n)
			break;	/* (uniform) */
		*(uint4 *)&tile[4 * tid] = mine;
		if (tid == 0)
			*(uint4 *)&tile[LDA_BR_TILE / 4] = behind;
		__syncthreads();
		if (s + 1 < LDA_BR_SCAN_WG / LDA_BR_TILE) {
			mine = load16_guard(in, base + LDA_BR_TILE + 16 * (u64)tid, n);
			if (tid == 0)
				behind = load16_guard(in, base + 2 * LDA_BR_TILE, n);
		}
		const uint4 q = *(const uint4 *)&tile[4 * tid];
		const u32 w[5] = { q.x, q.y, q.z, q.w, tile[4 * tid + 4] };
		u32 mask = 0;
#pragma unroll
		for (u32 j = 0; j < 16; j++) {
			const u32 win = j & 3 ? (w[j >> 2] >> (8 * (j & 3))) |
						(w[(j >> 2) + 1] << (32 - 8 * (j & 3))) : w[j >> 2];
			mask |= (u32)((win & SIG_MASK) == SIG24) << j;
		}
		/* p + 18 <= n: only the file's last 17 offsets can fail it */
		const u64 p0 = base + 16 * (u64)tid;
		if (mask && p0 + 15 + MIN_MEMBER > n) {
#pragma unroll
			for (u32 j = 0; j < 16; j++)
				if (p0 + j + MIN_MEMBER > n)
					mask &= ~(1u << j);
		}
		u32 tot;
		const u32 pre = wg_count_excl((u32)__builtin_popcount(mask), wsum, &tot);
		if (offsets) {
			u64 dst = at + pre;
			for (u32 m = mask; m && dst < cap; m &= m - 1, dst++)
				cand_pos[dst] = p0 + (u32)__builtin_ctz(m);
		}
		at += tot;
		__syncthreads();	/* the tile and wsum are free again */
	}
	if (!offsets && tid == 0)
		counts[blockIdx.x] = at;
}

/*
 * The gzip header at h (left >= 18 bytes of file from there on; signature and
 * FLG checked by the scan) by the decoder's rules (inflate_kernel.hip, the
 * GZIP container header), with one more: FNAME and FCOMMENT together are
 * LDA_GZM_NAME_MAX bytes at most.  The decoder looks for their ends with one
 * lane, byte after byte, as far as its input goes - and a candidate's input is
 * the rest of the file.  Without the limit every false candidate with FNAME
 * set in front of bytes without a zero would be walked to the end of the
 * file, candidates x file size dependent loads before the chain says which
 * candidates matter.  true: the count may parse this header, and reads at
 * most 65 549 + LDA_GZM_NAME_MAX bytes doing so.
 */
static __device__ __forceinline__ bool header_bounded(const u8 *__restrict__ h, u64 left)
{
	const u32 flg = h[3];
	u64 q = 10;
	u32 budget = LDA_GZM_NAME_MAX;

	if (flg & 0x04) {
		const u32 xlen = h[10] | ((u32)h[11] << 8);
		q = 12;
		if (left - q < (u64)xlen + 8)
			return false;
		q += xlen;
	}
	/* (left - q >= 8 here and behind every field: every load is inside) */
	for (u32 bit = 0x08; bit <= 0x10; bit <<= 1) {
		if (!(flg & bit))
			continue;
		bool ended = false;
		while (budget) {
			budget--;
			const u8 c = h[q++];
			if (c == 0 || q == left) {
				ended = true;
				break;
			}
		}
		if (!ended || left - q < 8)
			return false;
	}
	if (flg & 0x02) {
		q += 2;
		if (left - q < 8)
			return false;
	}
	return true;
}

/* the size query's descriptors: slot i < K is the file from candidate i on,
 * when its header is one the count may parse (header_bounded()); the other
 * candidates, the slots behind the last candidate - and all of them when the
 * candidates overflowed their room - have no input and fail in the header
 * check before anything is read */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_slots_kernel(const u8 *__restrict__ in, u64 n, const u64 *__restrict__ k_at, u64 cap,
		     const u64 *__restrict__ cand_pos, u64 *__restrict__ in_off,
		     u64 *__restrict__ in_n)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= cap)
		return;
	const u64 K = *k_at;
	const u64 p = K <= cap && i < K ? cand_pos[i] : n;
	/* (p + 18 <= n holds for every candidate written) */
	const bool live = p < n && n - p >= MIN_MEMBER && header_bounded(in + p, n - p);
	in_off[i] = live ? p : 0;
	in_n[i] = live ? n - p : 0;
}

/* what the chain kernels take for a candidate's size: its counted actual_in,
 * 0 - no successor - where the count failed or does not fit 32 bits.  The
 * count's verdict of such a long member becomes INSUFFICIENT_SPACE, the
 * verdict of the members the size query cannot count */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_size32_kernel(const u64 *__restrict__ k_at, u64 cap, s32 *__restrict__ results,
		      const u64 *__restrict__ actual_in, u32 *__restrict__ cand_size)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 K = *k_at;
	if (i >= cap || K > cap || i >= K)
		return;
	u32 size = 0;
	if (results[i] == LDA_SUCCESS) {
		if (actual_in[i] <= 0xFFFFFFFFull)
			size = (u32)actual_in[i];
		else
			results[i] = LDA_INSUFFICIENT_SPACE;
	}
	cand_size[i] = size;
}

/* one lane, behind lda_bgzf_top_kernel and only for a broken chain: the chain
 * from offset 0 again, block by block and then hop by hop inside the block
 * where it ends, to the position q that starts no counted member.
 * state[LDA_GZM_BREAK] = the count's verdict of the candidate at q, BAD_DATA
 * when none stands there */
extern "C" __global__ void __launch_bounds__(64)
lda_gzm_break_kernel(const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ cand_pos,
		     const u32 *__restrict__ next, const u32 *__restrict__ exit_at,
		     const s32 *__restrict__ results, u32 *__restrict__ state)
{
	const u64 K = *k_at;

	if (threadIdx.x || K > cap || state[LDA_BR_CHAIN])
		return;
	u32 verdict = LDA_BAD_DATA;
	if (K && cand_pos[0] == 0) {
		const u64 nblocks = (K + LDA_BR_JUMP - 1) / LDA_BR_JUMP;
		u32 cur = 0;
		/* (exit_at[] of a block lies in a later one: at most nblocks steps) */
		for (u64 step = 0; step < nblocks; step++) {
			const u32 e = exit_at[cur];
			if (e >= K)
				break;
			cur = e;
		}
		/* (a successor stands behind its candidate and inside the block here) */
		for (u32 hop = 0; hop < LDA_BR_JUMP; hop++) {
			const u32 nx = next[cur];
			if (nx >= K || nx <= cur)
				break;
			cur = nx;
		}
		if (results[cur] != LDA_SUCCESS)
			verdict = (u32)results[cur];
	}
	state[LDA_GZM_BREAK] = verdict;
}

/* msize[k] = the counted size of member k (0 for the rest of the max_members
 * chunks, and for all of them when there is no chain): the member's candidate
 * is found again by its position */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_msize_kernel(u64 max_members, const u64 *__restrict__ k_at, u64 cap,
		     const u64 *__restrict__ cand_pos, const u64 *__restrict__ cand_out,
		     const u32 *__restrict__ state, const u64 *__restrict__ in_off,
		     u64 *__restrict__ msize)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_members)
		return;
	const u64 K = *k_at;
	u64 v = 0;
	if (K <= cap && state[LDA_BR_CHAIN] && k < state[LDA_BR_MEMBERS]) {
		const u64 p = in_off[k];
		u64 lo = 0, hi = K;
		for (u32 s = 0; s < 64 && lo < hi; s++) {
			const u64 mid = lo + (hi - lo) / 2;
			if (cand_pos[mid] < p)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo < K && cand_pos[lo] == p)	/* (holds for every member found) */
			v = cand_out[lo];
	}
	msize[k] = v;
}

/* behind the scan of msize[] (out_off holds the local prefix): the batch's
 * descriptors - exact input length, exact fill - and the index pairs of the
 * members.  A file refused before the decode leaves max_members empty chunks */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_desc_kernel(u64 max_members, u64 out_avail, const u64 *__restrict__ k_at, u64 cap,
		    const u32 *__restrict__ state, const u64 *__restrict__ msize,
		    const u64 *__restrict__ block_sums, u64 *__restrict__ in_off,
		    u64 *__restrict__ in_n, u64 *__restrict__ out_off, u64 *__restrict__ out_av,
		    u64 *__restrict__ index)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_members)
		return;
	const u64 total = block_sums[(max_members + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];
	const u32 pre = pre_status(state, *k_at, cap, total, out_avail, max_members);
	const bool known = pre == LDA_SUCCESS ||
			   (pre == LDA_INSUFFICIENT_SPACE && state[LDA_BR_CHAIN]);
	const bool member = known && k < state[LDA_BR_MEMBERS];
	const u64 uoff = out_off[k] + block_sums[k / LDA_SCAN_BLOCK];

	if (index && member) {
		index[2 * k] = in_off[k];
		index[2 * k + 1] = uoff;
	}
	const bool live = member && pre == LDA_SUCCESS;
	if (!live) {
		in_off[k] = 0;
		in_n[k] = 0;
	}
	out_off[k] = live ? uoff : 0;
	out_av[k] = live ? msize[k] : 0;
}

/*
 * One workgroup behind the decode (results NULL: nothing was decoded - the
 * index call): result[0] the verdict - the pre-decode one, else the first
 * member in file order that failed -, [1] members (candidates under
 * MORE_CANDIDATES), [2] compressed bytes, [3] uncompressed bytes, [4] 0; the
 * closing index pair.  state NULL: the file is empty, which is BAD_DATA.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_final_kernel(u64 n, u64 max_members, u64 out_avail, const u64 *__restrict__ k_at,
		     u64 cap, const u32 *__restrict__ state, const u64 *__restrict__ total_at,
		     const u64 *__restrict__ in_n, const s32 *__restrict__ results,
		     const u64 *__restrict__ actual_in, u64 *__restrict__ result,
		     u64 *__restrict__ index)
{
	__shared__ u32 first;
	const u32 tid = threadIdx.x;

	if (!state) {
		if (tid < LDA_GZM_RESULT_WORDS)
			result[tid] = tid == 0 ? LDA_BAD_DATA : 0;
		return;
	}
	const u64 K = *k_at, total = *total_at;
	const u32 members = state[LDA_BR_MEMBERS];
	const u32 pre = pre_status(state, K, cap, total, out_avail, max_members);
	u32 verdict = pre;

	if (tid == 0)
		first = 0xFFFFFFFFu;
	__syncthreads();
	if (pre == LDA_SUCCESS && results)
		for (u32 k = tid; k < members; k += 256)
			if (results[k] != LDA_SUCCESS || actual_in[k] != in_n[k])
				atomicMin(&first, k);
	__syncthreads();
	if (pre == LDA_SUCCESS && first != 0xFFFFFFFFu)
		verdict = results[first] != LDA_SUCCESS ? (u32)results[first] : LDA_BAD_DATA;
	if (tid == 0) {
		const bool chain = K <= cap && state[LDA_BR_CHAIN];
		const bool known = pre == LDA_SUCCESS || (pre == LDA_INSUFFICIENT_SPACE && chain);
		result[0] = verdict;
		result[1] = K > cap ? K : chain ? members : 0;
		result[2] = known ? n : 0;
		result[3] = known ? total : 0;
		result[4] = 0;
		if (index && known) {
			index[2 * (u64)members] = n;
			index[2 * (u64)members + 1] = total;
		}
	}
}
