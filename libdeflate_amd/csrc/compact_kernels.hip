/*
 * compact_kernels.hip - device-side compaction of a batch's ragged outputs.
 *
 * A compress batch leaves stream i in a slot sized by compress_bound; callers
 * that ship the bytes on (the multi-GPU payload gather, the host-pointer
 * batch entry points, a file writer) want them back to back, the way the
 * reference's callers concatenate the return values of
 * libdeflate_*_compress (lib/deflate_compress.c:4064-4068 returns the size
 * that makes that possible; programs/gzip.c:149-185 writes exactly that many
 * bytes).  Three launches, all HBM-bound:
 *
 *   lda_scan_local_kernel    exclusive prefix sum of the sizes inside blocks
 *                            of 2048 chunks + the block totals
 *   lda_scan_blocks_kernel   exclusive prefix sum of the block totals (one
 *                            workgroup), grand total
 *   lda_compact_copy_kernel  one 256-thread workgroup per chunk: final offset
 *                            = local prefix + block prefix, then a copy with
 *                            16-byte stores to the aligned part of the
 *                            destination
 *
 * and the BGZF file assembly behind a compress batch (lda_bgzf_*).
 */
#include "device_common.h"
#include "kernels.h"

#define SCAN_THREADS 256
#define SCAN_PER_THREAD 8
#define SCAN_BLOCK (SCAN_THREADS * SCAN_PER_THREAD)

extern "C" __global__ void __launch_bounds__(SCAN_THREADS)
lda_scan_local_kernel(u64 n, const u64 *__restrict__ sizes,
		      u64 *__restrict__ offsets, u64 *__restrict__ block_sums)
{
	__shared__ u64 wsum[SCAN_THREADS / 64];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const u64 base = (u64)blockIdx.x * SCAN_BLOCK + (u64)tid * SCAN_PER_THREAD;
	u64 v[SCAN_PER_THREAD], mine = 0;

#pragma unroll
	for (int k = 0; k < SCAN_PER_THREAD; k++) {
		v[k] = base + k < n ? sizes[base + k] : 0;
		mine += v[k];
	}
	u64 incl = wave_scan_incl64(mine);
	if (lane == 63)
		wsum[wave] = incl;
	__syncthreads();
	u64 pre = incl - mine, tot = 0;
#pragma unroll
	for (u32 w = 0; w < SCAN_THREADS / 64; w++) {
		u64 s = wsum[w];
		if (w < wave)
			pre += s;
		tot += s;
	}
#pragma unroll
	for (int k = 0; k < SCAN_PER_THREAD; k++) {
		if (base + k < n)
			offsets[base + k] = pre;
		pre += v[k];
	}
	if (tid == 0)
		block_sums[blockIdx.x] = tot;
}

/* in place: block_sums[b] := sum of the totals before block b;
 * block_sums[nblocks] := grand total.  One workgroup. */
extern "C" __global__ void __launch_bounds__(1024)
lda_scan_blocks_kernel(u64 nblocks, u64 *__restrict__ block_sums)
{
	__shared__ u64 wsum[16];
	__shared__ u64 carry_s;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

	if (tid == 0)
		carry_s = 0;
	__syncthreads();
	for (u64 b0 = 0; b0 < nblocks; b0 += 1024) {
		u64 mine = b0 + tid < nblocks ? block_sums[b0 + tid] : 0;
		u64 incl = wave_scan_incl64(mine);
		if (lane == 63)
			wsum[wave] = incl;
		__syncthreads();
		u64 pre = carry_s + incl - mine, tot = 0;
#pragma unroll
		for (u32 w = 0; w < 16; w++) {
			u64 s = wsum[w];
			if (w < wave)
				pre += s;
			tot += s;
		}
		if (b0 + tid < nblocks)
			block_sums[b0 + tid] = pre;
		__syncthreads();
		if (tid == 0)
			carry_s += tot;
		__syncthreads();
	}
	if (tid == 0)
		block_sums[nblocks] = carry_s;
}

extern "C" __global__ void __launch_bounds__(256)
lda_compact_copy_kernel(u64 n, const u8 *__restrict__ in_base,
			const u64 *__restrict__ in_offsets,
			const u64 *__restrict__ sizes, u8 *__restrict__ out_base,
			u64 *__restrict__ offsets,
			const u64 *__restrict__ block_sums)
{
	const u32 tid = threadIdx.x;

	for (u64 c = blockIdx.x; c < n; c += gridDim.x) {
		const u64 start = offsets[c] + block_sums[c / SCAN_BLOCK];
		const u64 len = sizes[c];
		const u8 *src = in_base + in_offsets[c];
		u8 *dst = out_base + start;

		__syncthreads();	/* every thread has read offsets[c] */
		if (tid == 0) {
			offsets[c] = start;
			if (c == n - 1)
				offsets[n] = block_sums[(n + SCAN_BLOCK - 1) / SCAN_BLOCK];
		}
		copy_span(src, dst, len, tid);
	}
}

/*
 * A BGZF file (SAM/BAM spec 4.1) from one device buffer of n bytes: block k
 * is bytes [LDA_BGZF_BLOCK k, +LDA_BGZF_BLOCK) - the last one shorter - and
 * becomes member k, compressed into slot k (LDA_BGZF_MEMBER_MAX bytes) of a
 * scratch area by the compress kernels (format LDA_FMT_BGZF).  The scan
 * kernels above turn the member sizes into offsets; these three do the rest.
 */

/* the batch descriptors of the m blocks: input offset and size, slot offset
 * and size; nothing is uploaded from the host */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_desc_kernel(u64 m, u64 n, u64 *__restrict__ in_off, u64 *__restrict__ in_n,
		     u64 *__restrict__ slot_off, u64 *__restrict__ slot_avail)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= m)
		return;
	const u64 a = k * LDA_BGZF_BLOCK;
	in_off[k] = a;
	in_n[k] = n - a < LDA_BGZF_BLOCK ? n - a : LDA_BGZF_BLOCK;
	slot_off[k] = k * LDA_BGZF_MEMBER_MAX;
	slot_avail[k] = LDA_BGZF_MEMBER_MAX;
}

/* the members back to back at out, when all of them and eof_bytes more fit
 * out_avail (otherwise nothing is written: the finalize kernel reports 0);
 * index[2k], index[2k + 1] = the compressed and uncompressed offsets of
 * member k.  offsets / block_sums: the scan kernels' output */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_copy_kernel(u64 m, const u8 *__restrict__ slots, const u64 *__restrict__ sizes,
		     const u64 *__restrict__ offsets, const u64 *__restrict__ block_sums,
		     u8 *__restrict__ out, u64 out_avail, u32 eof_bytes, u64 *__restrict__ index)
{
	const u32 tid = threadIdx.x;
	const u64 total = block_sums[(m + SCAN_BLOCK - 1) / SCAN_BLOCK];

	if (total > out_avail || out_avail - total < eof_bytes)
		return;
	for (u64 c = blockIdx.x; c < m; c += gridDim.x) {
		const u64 start = offsets[c] + block_sums[c / SCAN_BLOCK];
		if (tid == 0 && index) {
			index[2 * c] = start;
			index[2 * c + 1] = c * LDA_BGZF_BLOCK;
		}
		copy_span(slots + c * LDA_BGZF_MEMBER_MAX, out + start, sizes[c], tid);
	}
}

/* the empty member that ends a BGZF file (SAM/BAM spec 4.1.2) */
static __device__ const u8 k_bgzf_eof[28] = {
	0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
	0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
};

/* one workgroup behind the copy: the EOF member (eof_bytes 28 or 0), the
 * file's size into *out_nbytes - 0 when a member did not fit its slot or the
 * file does not fit out_avail - and the index's last pair (EOF member, n).
 * total_at: the scan's grand total, NULL for m == 0 */
extern "C" __global__ void __launch_bounds__(256)
lda_bgzf_finalize_kernel(u64 m, u64 n, const u64 *__restrict__ sizes,
			 const u64 *__restrict__ total_at, u8 *__restrict__ out, u64 out_avail,
			 u32 eof_bytes, u64 *__restrict__ out_nbytes, u64 *__restrict__ index)
{
	const u32 tid = threadIdx.x;
	int missing = 0;

	for (u64 k = tid; k < m; k += 256)
		missing |= sizes[k] == 0;
	missing = __syncthreads_or(missing);
	const u64 total = total_at ? *total_at : 0;
	const bool ok = !missing && total <= out_avail && out_avail - total >= eof_bytes;
	if (ok && tid < eof_bytes)
		out[total + tid] = k_bgzf_eof[tid];
	if (tid == 0) {
		*out_nbytes = ok ? total + eof_bytes : 0;
		if (ok && index) {
			index[2 * m] = total;
			index[2 * m + 1] = n;
		}
	}
}
