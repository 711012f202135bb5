/*
 * large_kernels.hip - ONE raw DEFLATE / zlib / gzip stream from one device
 * buffer (host_compress.hip: libdeflate_amd_compress_large_batch).
 *
 * The buffer is cut into segments that the compress kernels turn into
 * byte-aligned pieces of one raw stream, each in a slot of a scratch area
 * (large_plan.h).  These kernels do what the host-memory form does on the
 * host: the batch descriptors, the pieces back to back behind the container
 * header, and the header, the footer - the checksum of the whole buffer
 * combined from the pieces' checksums - and the size.  Nothing is uploaded
 * and nothing is read back.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "large_plan.h"

/* the batch descriptors of the nseg segments: rows of nseg u64 each - input
 * offset and size (the prime in front), slot offset and size, [sizes out: the
 * compress kernels write that row], piece offset and size - and seg_info */
extern "C" __global__ void __launch_bounds__(256)
lda_large_desc_kernel(lda_large_shape g, u64 *__restrict__ rows, u32 *__restrict__ seg_info)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= g.nseg)
		return;
	const lda_large_seg s = lda_large_seg_of(g, i);
	rows[i] = s.in_off;
	rows[g.nseg + i] = s.in_n;
	rows[2 * g.nseg + i] = s.out_off;
	rows[3 * g.nseg + i] = s.out_av;
	rows[5 * g.nseg + i] = s.pc_off;
	rows[6 * g.nseg + i] = s.pc_n;
	seg_info[i] = s.info;
}

/* an input that is ONE chunk of the ordinary batch: its four descriptors */
extern "C" __global__ void
lda_large_one_desc_kernel(u64 n, u64 out_avail, u64 *__restrict__ rows)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		rows[0] = 0;
		rows[1] = n;
		rows[2] = 0;
		rows[3] = out_avail;
	}
}

/* does hdr + total + ftr fit out_avail?  (no sum that could wrap) */
static __device__ __forceinline__ bool large_fits(u64 total, u32 hdr_ftr, u64 out_avail)
{
	return total <= out_avail && out_avail - total >= hdr_ftr;
}

/* the pieces back to back at out + hdr, when header, pieces and footer fit
 * out_avail (otherwise nothing is written: the finalize kernel reports 0).
 * offsets / block_sums: the scan kernels' output over the sizes */
extern "C" __global__ void __launch_bounds__(256)
lda_large_copy_kernel(u64 nseg, const u8 *__restrict__ slots, u64 slot,
		      const u64 *__restrict__ sizes, const u64 *__restrict__ offsets,
		      const u64 *__restrict__ block_sums, u8 *__restrict__ out, u32 hdr, u32 ftr,
		      u64 out_avail)
{
	const u32 tid = threadIdx.x;
	const u64 total = block_sums[(nseg + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (!large_fits(total, hdr + ftr, out_avail))
		return;
	for (u64 c = blockIdx.x; c < nseg; c += gridDim.x) {
		const u64 start = offsets[c] + block_sums[c / LDA_SCAN_BLOCK];
		copy_span(slots + c * slot, out + hdr + start, sizes[c], tid);
	}
}

#define LARGE_FIN_THREADS 1024

/* XOR / sum over the workgroup, the result in every thread */
static __device__ __forceinline__ u32 block_xor(u32 v, u32 *sh, u32 tid)
{
	v = wave_xor(v);
	__syncthreads();
	if ((tid & 63) == 0)
		sh[tid >> 6] = v;
	__syncthreads();
	u32 r = 0;
	for (u32 w = 0; w < LARGE_FIN_THREADS / 64; w++)
		r ^= sh[w];
	return r;
}

static __device__ __forceinline__ u64 block_sum64(u64 v, u64 *sh, u32 tid)
{
	v = wave_sum64(v);
	__syncthreads();
	if ((tid & 63) == 0)
		sh[tid >> 6] = v;
	__syncthreads();
	u64 r = 0;
	for (u32 w = 0; w < LARGE_FIN_THREADS / 64; w++)
		r += sh[w];
	return r;
}

/*
 * One workgroup behind the copy: the container header, the footer and the
 * stream's size into *out_nbytes - 0 when a segment did not fit its slot or
 * the stream does not fit out_avail (then nothing is written).
 *
 * The checksum of the whole buffer from the pieces' (sums[i] of piece i,
 * t_i = the bytes behind piece i), every thread over a contiguous run [a, b)
 * of the pieces:
 *   CRC-32   crc = XOR_i sums[i] * x^(8 t_i) mod P.  Horner over the run - a
 *            multiply by x^(8 len_i) per piece, xS = x^(8 S) for every piece
 *            but the last, xL for that one - then one multiply by
 *            x^(8 t_(b-1)) = xS^(nseg - 1 - b) * xL, and XOR over the threads.
 *   Adler-32 (M = 65521) a = 1 + SUM_i (a_i - 1), b = SUM_i (b_i + (t_i mod M)
 *            (a_i - 1)), both mod M: lda::adler32_concat() applied nseg - 1
 *            times and multiplied out.
 * total_at: the scan's grand total of the sizes.
 */
extern "C" __global__ void __launch_bounds__(LARGE_FIN_THREADS)
lda_large_finalize_kernel(u64 nseg, u64 n, u64 S, int format, int level,
			  const u64 *__restrict__ sizes, const u32 *__restrict__ sums,
			  const u64 *__restrict__ total_at, u32 xS, u32 xL,
			  u8 *__restrict__ out, u64 out_avail, u64 *__restrict__ out_nbytes)
{
	__shared__ u64 sh[LARGE_FIN_THREADS / 64];
	const u32 tid = threadIdx.x;
	const u32 M = 65521;
	const u64 run = (nseg + LARGE_FIN_THREADS - 1) / LARGE_FIN_THREADS;
	const u64 a = (u64)tid * run < nseg ? (u64)tid * run : nseg;
	const u64 b = a + run < nseg ? a + run : nseg;
	const u32 hdr = format == LDA_FMT_GZIP ? 10 : format == LDA_FMT_ZLIB ? 2 : 0;
	const u32 ftr = format == LDA_FMT_GZIP ? 8 : format == LDA_FMT_ZLIB ? 4 : 0;
	int missing = 0;

	for (u64 i = a; i < b; i++)
		missing |= sizes[i] == 0;
	missing = __syncthreads_or(missing);
	const u64 total = *total_at;
	const bool ok = !missing && large_fits(total, hdr + ftr, out_avail);
	u32 sum = 0;
	if (format == LDA_FMT_GZIP) {
		u32 acc = 0;
		for (u64 i = a; i < b; i++)
			acc = lda_crc_mulmod(acc, i + 1 == nseg ? xL : xS) ^ sums[i];
		if (a < b && b < nseg)
			acc = lda_crc_mulmod(acc, lda_crc_mulmod(lda_crc_powmod(xS, nseg - 1 - b), xL));
		sum = block_xor(acc, (u32 *)sh, tid);
	} else if (format == LDA_FMT_ZLIB) {
		u64 sa = 0, sb = 0;
		for (u64 i = a; i < b; i++) {
			const u32 ai = ((sums[i] & 0xFFFF) + M - 1) % M, bi = (sums[i] >> 16) % M;
			const u64 t = i + 1 < nseg ? n - (i + 1) * S : 0;
			sa = (sa + ai) % M;
			sb = (sb + bi + (t % M) * ai) % M;
		}
		sa = block_sum64(sa, sh, tid);
		sb = block_sum64(sb, sh, tid);
		sum = (u32)(sb % M) << 16 | (u32)((1 + sa) % M);
	}
	if (ok && format == LDA_FMT_GZIP) {
		/* lib/gzip_compress.c:44-79: MTIME 0, OS 0xFF; CRC-32 and ISIZE, LE */
		if (tid < 8)	/* 1F 8B, CM 8, FLG 0, MTIME */
			out[tid] = (u8)(0x00088B1Full >> (8 * tid));
		else if (tid < 10)
			out[tid] = tid == 8 ? lda_gzip_xfl(level) : 0xFF;
		else if (tid < 14)
			out[10 + total + (tid - 10)] = (u8)(sum >> (8 * (tid - 10)));
		else if (tid < 18)
			out[14 + total + (tid - 14)] = (u8)((u32)n >> (8 * (tid - 14)));
	} else if (ok && format == LDA_FMT_ZLIB) {
		/* lib/zlib_compress.c:45-72: Adler-32, big endian */
		const u32 hw = lda_zlib_header(level);
		if (tid < 2)
			out[tid] = (u8)(hw >> (8 * (1 - tid)));
		else if (tid < 6)
			out[2 + total + (tid - 2)] = (u8)(sum >> (8 * (5 - tid)));
	}
	if (tid == 0)
		*out_nbytes = ok ? hdr + total + ftr : 0;
}
