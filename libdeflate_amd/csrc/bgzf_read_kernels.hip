/*
 * bgzf_read_kernels.hip - reading a BGZF file (SAM/BAM spec 4.1) that lies in
 * device memory: where its members are, the descriptors of ONE decompress
 * batch that puts every member at its final place, the file's result words
 * and index (host_bgzf_read.hip; tools/models/bgzf_chain.py is the CPU model
 * of the finder, and the tests run it on the same files).
 *
 * The members form a linked list (next = pos + BSIZE + 1).  Walked by one
 * lane that is a dependent load per member, so the list is found in parallel
 * (host_finder.h launches the finder, for this reader and for those of
 * concatenated gzip members and ZIP directories, whose candidates the chain
 * kernels below link as well):
 *
 *   lda_bgzf_scan_kernel     every byte offset against htslib's header rule
 *                            (1f 8b 08 04, XLEN 6, "BC" 2 0) with a size that
 *                            stays inside the file: counted per 16 KiB of
 *                            file, then - after the scan kernels of
 *                            compact_kernels.hip - written in file order as
 *                            (position, size).  Candidates are not members:
 *                            a stored block carries the signature verbatim.
 *   lda_bgzf_jump_kernel     per candidate the candidate that starts where
 *                            it ends (binary search); per block of 1024
 *                            candidates jump tables of 2^k hops inside the
 *                            block, from which every candidate learns where
 *                            its path leaves the block and after how many
 *                            hops.  A candidate's successor stands behind
 *                            it, so every path ends.
 *   lda_bgzf_top_kernel      one lane from candidate 0 block by block (K /
 *                            1024 steps): the block's entry on the true
 *                            chain and the members before it.
 *   lda_bgzf_members_kernel  per block, rank r of the path from the entry is
 *                            member base + r (r in binary through the tables).
 *   lda_bgzf_walk_kernel     the serial walk from offset 0: what runs when
 *                            the scan found more candidates than the host
 *                            made room for, or when LDA_BGZF_SERIAL asks.
 *
 * and then, whichever found the members,
 *
 *   lda_bgzf_isize_kernel    ISIZE of every member (4 bytes at any alignment)
 *   lda_bgzf_rdesc_kernel    behind the scan of the ISIZEs: the batch's
 *                            descriptors and the index; every chunk is
 *                            emptied when the file is refused before the
 *                            decode
 *   lda_bgzf_rfinal_kernel   one workgroup: the five result words, the
 *                            closing index pair
 *   lda_bgzf_trim_kernel / lda_bgzf_range_kernel   ranged reads
 *
 * The input is hostile by definition: every load is checked against n, every
 * index against the candidate count, and no loop takes its bound from the file.
 */
#include "device_common.h"
#include "kernels.h"

#define SIG32 0x04088b1fu	/* 1f 8b 08 04 */
#define MIN_MEMBER 28u
#define OUT16 0xFFFFu

/* pre-decode verdict from the finder's state, the sum of the ISIZEs and the
 * caller's limits; precedence as include/libdeflate_amd.h states it */
static __device__ __forceinline__ u32
pre_status(const u32 *__restrict__ state, u64 total, u64 out_avail, u64 max_members)
{
	if (!state[LDA_BR_CHAIN] || state[LDA_BR_BADISIZE])
		return LDA_BAD_DATA;
	if (state[LDA_BR_MEMBERS] > max_members)
		return LDA_BR_MORE;
	if (total > out_avail)
		return LDA_INSUFFICIENT_SPACE;
	return LDA_SUCCESS;
}

/* member size by the header rule from 18 header bytes, 0 = no member: bytes
 * 4..9 (MTIME, XFL, OS) are free.  left = bytes of the file from this offset */
static __device__ __forceinline__ u32 header_size(const u8 *h, u64 left)
{
	if (h[10] != 6 || h[11] != 0 || h[12] != 0x42 || h[13] != 0x43 || h[14] != 2 || h[15] != 0)
		return 0;
	const u32 size = ((u32)h[16] | (u32)h[17] << 8) + 1;
	return size >= MIN_MEMBER && size <= left ? size : 0;
}

/*
 * One workgroup per LDA_BR_SCAN_WG bytes of file, in steps of 4 KiB: 16
 * bytes per thread into LDS (and 32 more behind the tile), every offset's
 * four bytes against the signature, the rest of the rule for the survivors.
 * offsets == NULL: counts[wg] = candidates of the workgroup's range.
 * Otherwise offsets / block_sums are the scan of the counts, and the
 * candidates below index cap are written in file order.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_scan_kernel(const u8 *__restrict__ in, u64 n, u64 *__restrict__ counts,
		     const u64 *__restrict__ offsets, const u64 *__restrict__ block_sums,
		     u64 cap, u64 *__restrict__ cand_pos, u32 *__restrict__ cand_size)
{
	__shared__ __attribute__((aligned(16))) u32 tile[LDA_BR_TILE / 4 + 8];
	__shared__ u32 wsum[4];
	const u32 tid = threadIdx.x;
	const u64 wg0 = (u64)blockIdx.x * LDA_BR_SCAN_WG;
	u64 at = 0;	/* candidates of this workgroup so far / where they go */

	if (offsets) {
		if (counts[blockIdx.x] == 0)
			return;
		at = offsets[blockIdx.x] + block_sums[blockIdx.x / LDA_SCAN_BLOCK];
	}
	for (u32 s = 0; s < LDA_BR_SCAN_WG / LDA_BR_TILE; s++) {
		const u64 base = wg0 + (u64)s * LDA_BR_TILE;
		if (base >= n)
			break;	/* (uniform) */
		*(uint4 *)&tile[4 * tid] = load16_guard(in, base + 16 * (u64)tid, n);
		if (tid < 2)
			*(uint4 *)&tile[LDA_BR_TILE / 4 + 4 * tid] =
				load16_guard(in, base + LDA_BR_TILE + 16 * (u64)tid, n);
		__syncthreads();
		const uint4 q = *(const uint4 *)&tile[4 * tid];
		const u32 w[5] = { q.x, q.y, q.z, q.w, tile[4 * tid + 4] };
		u32 mask = 0, size = 0;
#pragma unroll
		for (u32 j = 0; j < 16; j++) {
			const u32 win = j & 3 ? (w[j >> 2] >> (8 * (j & 3))) |
						(w[(j >> 2) + 1] << (32 - 8 * (j & 3))) : w[j >> 2];
			mask |= (u32)(win == SIG32) << j;
		}
		/* the rest of the rule for the survivors (rare).  Two members cannot
		 * start within 16 bytes of each other - the fixed bytes 10..15 of
		 * the first would have to be signature or fixed bytes of the second,
		 * or its BSIZE says 7 bytes - so a thread keeps one at most */
		if (mask) {
			const u8 *tb = (const u8 *)tile;
			u32 keep = 0;
			for (u32 m = mask; m && !keep; m &= m - 1) {
				const u32 j = (u32)__builtin_ctz(m), o = 16 * tid + j;
				size = header_size(tb + o, n - (base + o));
				if (size)
					keep = 1u << j;
			}
			mask = keep;
		}
		u32 tot;
		const u32 pre = wg_count_excl((u32)__builtin_popcount(mask), wsum, &tot);
		if (offsets && mask && at + pre < cap) {
			cand_pos[at + pre] = base + 16 * tid + (u32)__builtin_ctz(mask);
			cand_size[at + pre] = size;
		}
		at += tot;
		__syncthreads();	/* the tile and wsum are free again */
	}
	if (!offsets && tid == 0)
		counts[blockIdx.x] = at;
}

/* J[k][t]: the candidate 2^k hops behind candidate blk0 + t as an index inside
 * the block of LDA_BR_JUMP candidates, OUT16 once the path has left it.
 * nx: the thread's own successor (candidate index, LDA_BR_END, LDA_BR_NONE) */
static __device__ __forceinline__ void
build_tables(u16 (*J)[LDA_BR_JUMP], u32 nx, u64 blk0, u64 K)
{
	const u32 t = threadIdx.x;
	const u64 hi = blk0 + LDA_BR_JUMP < K ? blk0 + LDA_BR_JUMP : K;

	/* (a successor stands behind its candidate: nx > blk0 + t) */
	J[0][t] = nx < hi && nx > blk0 + t ? (u16)(nx - blk0) : OUT16;
	__syncthreads();
	for (u32 k = 1; k < LDA_BR_LOG; k++) {
		const u32 a = J[k - 1][t];
		J[k][t] = a == OUT16 ? OUT16 : J[k - 1][a];
		__syncthreads();
	}
}

/*
 * One workgroup of LDA_BR_JUMP threads per block of candidates: next[] (kept
 * for lda_bgzf_members_kernel), exit[i] = the first candidate outside the
 * block on i's path (or END / NONE), hops[i] = candidates of the block on
 * that path, i included.  k_at: the candidate count the scan found; above
 * cap nothing is done (the serial walk runs instead).
 */
extern "C" __global__ void __launch_bounds__(LDA_BR_JUMP)
lda_bgzf_jump_kernel(u64 n, const u64 *__restrict__ k_at, u64 cap,
		     const u64 *__restrict__ cand_pos, const u32 *__restrict__ cand_size,
		     u32 *__restrict__ next, u32 *__restrict__ exit_at, u32 *__restrict__ hops,
		     u32 *__restrict__ entry)
{
	__shared__ u16 J[LDA_BR_LOG][LDA_BR_JUMP];
	__shared__ u32 nx_s[LDA_BR_JUMP];
	const u64 K = *k_at;
	const u32 t = threadIdx.x;
	const u64 blk0 = (u64)blockIdx.x * LDA_BR_JUMP, i = blk0 + t;

	if (K > cap || blk0 >= K)
		return;
	if (t == 0)
		entry[blockIdx.x] = LDA_BR_NONE;
	u32 nx = LDA_BR_NONE;
	if (i < K) {
		const u64 end = cand_pos[i] + cand_size[i];
		if (end == n) {
			nx = LDA_BR_END;
		} else {
			u64 lo = i + 1, hi = K;
			for (u32 s = 0; s < 64 && lo < hi; s++) {
				const u64 mid = lo + (hi - lo) / 2;
				if (cand_pos[mid] < end)
					lo = mid + 1;
				else
					hi = mid;
			}
			if (lo < K && cand_pos[lo] == end)
				nx = (u32)lo;
		}
		next[i] = nx;
	}
	nx_s[t] = nx;
	build_tables(J, nx, blk0, K);
	if (i >= K)
		return;
	u32 cur = t, cnt = 1;
#pragma unroll
	for (int k = LDA_BR_LOG - 1; k >= 0; k--) {
		const u32 a = J[k][cur];
		if (a != OUT16) {
			cur = a;
			cnt += 1u << k;
		}
	}
	exit_at[i] = nx_s[cur];
	hops[i] = cnt;
}

/* one lane: the true chain block by block.  state[CHAIN] = it starts at offset
 * 0 and ends exactly at n; state[MEMBERS] = its length */
extern "C" __global__ void __launch_bounds__(64)
lda_bgzf_top_kernel(const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ cand_pos,
		    const u32 *__restrict__ exit_at, const u32 *__restrict__ hops,
		    u32 *__restrict__ entry, u32 *__restrict__ base, u32 *__restrict__ state)
{
	const u64 K = *k_at;

	if (threadIdx.x || K > cap)
		return;
	const u64 nblocks = (K + LDA_BR_JUMP - 1) / LDA_BR_JUMP;
	u32 cur = LDA_BR_NONE, count = 0;
	if (K && cand_pos[0] == 0) {
		cur = 0;
		/* (exit_at[] of a block lies in a later one: at most nblocks steps) */
		for (u64 step = 0; step < nblocks; step++) {
			const u32 b = cur / LDA_BR_JUMP;
			entry[b] = cur;
			base[b] = count;
			count += hops[cur];
			cur = exit_at[cur];
			if (cur >= K)
				break;
		}
	}
	state[LDA_BR_CHAIN] = cur == LDA_BR_END;
	state[LDA_BR_MEMBERS] = count;
}

/* the members of every block on the chain into in_off / in_n (the first
 * max_members of them) */
extern "C" __global__ void __launch_bounds__(LDA_BR_JUMP)
lda_bgzf_members_kernel(const u64 *__restrict__ k_at, u64 cap, u64 max_members,
			const u64 *__restrict__ cand_pos, const u32 *__restrict__ cand_size,
			const u32 *__restrict__ next, const u32 *__restrict__ hops,
			const u32 *__restrict__ entry, const u32 *__restrict__ base,
			const u32 *__restrict__ state, u64 *__restrict__ in_off,
			u64 *__restrict__ in_n)
{
	__shared__ u16 J[LDA_BR_LOG][LDA_BR_JUMP];
	const u64 K = *k_at;
	const u32 t = threadIdx.x;
	const u64 blk0 = (u64)blockIdx.x * LDA_BR_JUMP;

	if (K > cap || blk0 >= K || !state[LDA_BR_CHAIN])
		return;
	const u32 e = entry[blockIdx.x];
	if (e < blk0 || e >= blk0 + LDA_BR_JUMP || e >= K)	/* LDA_BR_NONE: not on the chain */
		return;
	build_tables(J, blk0 + t < K ? next[blk0 + t] : LDA_BR_NONE, blk0, K);
	if (t >= hops[e])
		return;
	u32 cur = e - (u32)blk0;
#pragma unroll
	for (u32 k = 0; k < LDA_BR_LOG; k++)
		if (t >> k & 1) {
			cur = J[k][cur];
			if (cur == OUT16)
				return;	/* (cannot happen: t < hops[e]) */
		}
	const u64 mi = (u64)base[blockIdx.x] + t;
	if (mi < max_members) {
		in_off[mi] = cand_pos[blk0 + cur];
		in_n[mi] = cand_size[blk0 + cur];
	}
}

/* the serial walk, one lane: a dependent load per member.  Runs when forced or
 * when the scan found more than cap candidates (k_at NULL: no scan ran) */
extern "C" __global__ void __launch_bounds__(64)
lda_bgzf_walk_kernel(const u8 *__restrict__ in, u64 n, u64 max_members,
		     const u64 *__restrict__ k_at, u64 cap, int force, u64 *__restrict__ in_off,
		     u64 *__restrict__ in_n, u32 *__restrict__ state)
{
	if (threadIdx.x || !(force || (k_at && *k_at > cap)))
		return;
	u64 pos = 0;
	u32 count = 0, ok = 1;
	/* (a member is 28 bytes at least: n / 28 steps at most) */
	while (pos < n) {
		u32 size = 0;
		if (n - pos >= MIN_MEMBER) {
			u32 h[5];
			__builtin_memcpy(h, in + pos, 16);
			h[4] = (u32)in[pos + 16] | (u32)in[pos + 17] << 8;
			if (h[0] == SIG32)
				size = header_size((const u8 *)h, n - pos);
		}
		if (!size) {
			ok = 0;
			break;
		}
		if (count < max_members) {
			in_off[count] = pos;
			in_n[count] = size;
		}
		count++;
		pos += size;
	}
	state[LDA_BR_CHAIN] = ok;
	state[LDA_BR_MEMBERS] = count;
}

/* isize[k] of the members found (0 for the rest of the max_members chunks, and
 * for all of them when the chain is bad); an ISIZE above 64 KiB is flagged */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_isize_kernel(const u8 *__restrict__ in, u64 n, u64 max_members,
		      const u64 *__restrict__ in_off, const u64 *__restrict__ in_n,
		      u32 *__restrict__ state, u64 *__restrict__ isize)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_members)
		return;
	u64 v = 0;
	if (state[LDA_BR_CHAIN] && k < state[LDA_BR_MEMBERS]) {
		const u64 end = in_off[k] + in_n[k];
		if (end >= 4 && end <= n) {	/* (holds for every member found) */
			const u8 *p = in + end - 4;
			v = (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24;
		}
		if (v > LDA_BGZF_MEMBER_MAX) {
			atomicOr(&state[LDA_BR_BADISIZE], 1u);
			v = 0;
		}
	}
	isize[k] = v;
}

/* behind the scan of isize[] (out_off holds the local prefix): the batch's
 * descriptors, the index pairs of the members.  A file refused before the
 * decode leaves max_members empty chunks */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_rdesc_kernel(u64 max_members, u64 out_avail, const u32 *__restrict__ state,
		      const u64 *__restrict__ isize, const u64 *__restrict__ block_sums,
		      u64 *__restrict__ in_off, u64 *__restrict__ in_n, u64 *__restrict__ out_off,
		      u64 *__restrict__ out_av, u64 *__restrict__ index)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_members)
		return;
	const u64 total = block_sums[(max_members + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];
	const u32 pre = pre_status(state, total, out_avail, max_members);
	const bool member = k < state[LDA_BR_MEMBERS];
	const u64 uoff = out_off[k] + block_sums[k / LDA_SCAN_BLOCK];

	if (index && member && (pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE)) {
		index[2 * k] = in_off[k];
		index[2 * k + 1] = uoff;
	}
	const bool live = member && pre == LDA_SUCCESS;
	if (!live) {
		in_off[k] = 0;
		in_n[k] = 0;
	}
	out_off[k] = live ? uoff : 0;
	out_av[k] = live ? isize[k] : 0;
}

static __device__ const u8 k_eof_member[28] = {
	0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
	0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
};

/*
 * One workgroup behind the decode (results NULL: nothing was decoded - the
 * index call): result[0] the verdict - the pre-decode one, else the first
 * member in file order that failed or that ended before its size says
 * (BAD_DATA) -, [1] members, [2] compressed bytes, [3] uncompressed bytes, [4]
 * flags; the closing index pair.  state NULL: the file is empty.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_rfinal_kernel(const u8 *__restrict__ in, u64 n, u64 max_members, u64 out_avail,
		       const u32 *__restrict__ state, const u64 *__restrict__ total_at,
		       const u64 *__restrict__ in_off, const u64 *__restrict__ in_n,
		       const s32 *__restrict__ results, const u64 *__restrict__ actual_in,
		       u64 *__restrict__ result, u64 *__restrict__ index)
{
	__shared__ u32 first;
	const u32 tid = threadIdx.x;

	if (!state) {
		if (tid < LDA_BR_RESULT_WORDS)
			result[tid] = 0;
		if (index && tid < 2)
			index[tid] = 0;
		return;
	}
	const u64 total = *total_at;
	const u32 members = state[LDA_BR_MEMBERS];
	const u32 pre = pre_status(state, total, out_avail, max_members);
	u32 verdict = pre;
	int differs = 1;	/* the last member from the 28 bytes of the EOF member */

	if (tid == 0)
		first = 0xFFFFFFFFu;
	__syncthreads();
	if (pre == LDA_SUCCESS) {
		if (results)
			for (u32 k = tid; k < members; k += 256)
				if (results[k] != LDA_SUCCESS || actual_in[k] != in_n[k])
					atomicMin(&first, k);
		/* (members <= max_members here: the last member's descriptor is there) */
		if (members && in_n[members - 1] == 28)
			differs = tid < 28 && in[in_off[members - 1] + tid] != k_eof_member[tid];
	}
	const int eof = !__syncthreads_or(differs);
	if (pre == LDA_SUCCESS && first != 0xFFFFFFFFu)
		verdict = results[first] != LDA_SUCCESS ? (u32)results[first] : LDA_BAD_DATA;
	if (tid == 0) {
		const bool known = pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE;
		result[0] = verdict;
		result[1] = pre == LDA_BAD_DATA ? 0 : members;
		result[2] = known ? n : 0;
		result[3] = known ? total : 0;
		result[4] = pre == LDA_SUCCESS && eof ? LDA_BR_HAS_EOF : 0;
		if (index && known) {
			index[2 * (u64)members] = n;
			index[2 * (u64)members + 1] = total;
		}
	}
}

/* ranged reads: trim t copies len bytes from offset src of the slot area to
 * offset dst of the output (trims: src, dst, len as u64 triples) */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_trim_kernel(u64 n_trims, const u64 *__restrict__ trims, const u8 *__restrict__ slots,
		     u8 *__restrict__ out)
{
	for (u64 t = blockIdx.x; t < n_trims; t += gridDim.x)
		copy_span(slots + trims[3 * t], out + trims[3 * t + 1], trims[3 * t + 2],
			  threadIdx.x);
}

/* ranged reads: range r owns the chunks [first[r], first[r + 1]) of the batch;
 * its result is that of its first chunk that failed or ended early */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_range_kernel(u64 n_ranges, const u64 *__restrict__ first, const u64 *__restrict__ in_n,
		      const s32 *__restrict__ results, const u64 *__restrict__ actual_in,
		      s32 *__restrict__ range_results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n_ranges)
		return;
	s32 v = LDA_SUCCESS;
	for (u64 c = first[r]; c < first[r + 1]; c++) {
		if (results[c] != LDA_SUCCESS)
			v = results[c];
		else if (actual_in[c] != in_n[c])
			v = LDA_BAD_DATA;
		if (v != LDA_SUCCESS)
			break;
	}
	range_results[r] = v;
}
