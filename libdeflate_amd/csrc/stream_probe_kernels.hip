/*
 * stream_probe_kernels.hip - what the host of the many-wave decoder
 * (host_stream.hip) used to read out of the stream itself, for a stream that
 * lies in device memory (libdeflate_amd_decompress_large):
 *
 *   lda_stream_find_stored_kernel  every byte offset at which a stored block's
 *                                  LEN / NLEN pair could lie, as 16-byte rows
 *                                  (stored_rows.h) - what walk_stored() reads
 *   lda_stream_hdr_class_kernel    the rule of one_length_code() on the headers
 *                                  lda_stream_hdr_cache_kernel has parsed
 */
#include "device_common.h"
#include "stream_kernels.h"

/* the bytes of the aligned dword at address B that lie in [a, end) */
static __device__ __forceinline__ u32 clip4(u32 v, uintptr_t B, uintptr_t a, uintptr_t end)
{
	u32 m = 0;
#pragma unroll
	for (u32 k = 0; k < 4; k++)
		if (B + k >= a && B + k < end)
			m |= 0xFFu << (8 * k);
	return v & m;
}

/*
 * Every bp in [bp0, in_n - 4] with LEN == (NLEN ^ 0xFFFF) appends a row
 * { bp, LEN, the two bytes in front of bp } to rows[] through *count (which may
 * pass cap: the rows past it are lost).  A lane takes the 16 offsets of one
 * ALIGNED 16-byte word of memory - `inp` itself has any alignment -, so that a
 * wave reads 1 KiB in one instruction.  Only aligned words that hold at least
 * one byte of [inp, inp + in_n) are loaded, the rule of load_in()
 * (inflate_kernel.hip); what they hold outside that range is cleared.  The two
 * bytes in front of a lane's word and the three behind it come from the lanes
 * next to it (ds_bpermute), at the wave's two edges from a load of their own.
 * Bound by the read of the window: on arbitrary bytes one offset in 65536
 * passes, and a wave without a hit leaves after one ballot.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_stream_find_stored_kernel(const u8 *__restrict__ inp, u64 in_n, u64 bp0,
			      uint4 *__restrict__ rows, u32 *__restrict__ count, u32 cap)
{
	if (in_n < 4 || bp0 + 4 > in_n)
		return;
	const uintptr_t a = (uintptr_t)inp, end = a + in_n;
	const uintptr_t first = a + bp0;		/* the first and the last offset tested */
	const uintptr_t last = end - 4;
	const u64 w_first = first >> 4, w_last = last >> 4;
	const u32 lane = threadIdx.x & 63;
	for (u64 w0 = w_first + (u64)blockIdx.x * 256; w0 <= w_last; w0 += 256ull * gridDim.x) {
		const uintptr_t A = (uintptr_t)(w0 + threadIdx.x) << 4;
		const bool have = A < end;	/* (A + 15 >= a: w_first's word holds `first`) */
		uint4 x = make_uint4(0, 0, 0, 0);
		if (have)
			x = *(const uint4 *)A;
		if (A < a || A + 16 > end) {
			x.x = clip4(x.x, A, a, end);
			x.y = clip4(x.y, A + 4, a, end);
			x.z = clip4(x.z, A + 8, a, end);
			x.w = clip4(x.w, A + 12, a, end);
		}
		u32 W[6];
		W[0] = __shfl_up(x.w, 1, 64);
		W[5] = __shfl_down(x.x, 1, 64);
		if (lane == 0)
			W[0] = have && A > a ? clip4(*(const u32 *)(A - 4), A - 4, a, end) : 0;
		if (lane == 63)
			W[5] = A + 16 < end ? clip4(*(const u32 *)(A + 16), A + 16, a, end) : 0;
		W[1] = x.x;
		W[2] = x.y;
		W[3] = x.z;
		W[4] = x.w;
		/* byte j of the word is byte j + 4 of W[] */
		u32 hits = 0;
#pragma unroll
		for (u32 j = 0; j < 16; j++) {
			const u32 v = __builtin_amdgcn_alignbyte(W[(j + 4) / 4 + 1], W[(j + 4) / 4], j & 3);
			const bool hit = ((v ^ (v >> 16)) & 0xFFFFu) == 0xFFFFu && A + j >= first &&
					 A + j <= last;
			hits |= (u32)hit << j;
		}
		if (__ballot(hits != 0) == 0)
			continue;
		/* the wave's rows: lane after lane, one atomic for all of them */
		const u32 mine = __popc(hits);
		u32 incl = mine;
#pragma unroll
		for (u32 off = 1; off < 64; off *= 2) {
			const u32 t = __shfl_up(incl, off, 64);
			if (lane >= off)
				incl += t;
		}
		const u32 total = bcast_lane(incl, 63);
		u32 base = 0;
		if (lane == 0)
			base = atomicAdd(count, total);
		u32 at = bcast_first(base) + incl - mine;
#pragma unroll
		for (u32 j = 0; j < 16; j++) {
			if (!((hits >> j) & 1))
				continue;
			if (at < cap) {
				const u32 v = __builtin_amdgcn_alignbyte(W[(j + 4) / 4 + 1], W[(j + 4) / 4], j & 3);
				const u32 f = __builtin_amdgcn_alignbyte(W[(j + 2) / 4 + 1], W[(j + 2) / 4], (j + 2) & 3);
				const u64 bp = (u64)(A + j - a);
				rows[at] = make_uint4((u32)bp, (u32)(bp >> 32), v & 0xFFFFu, f & 0xFFFFu);
			}
			at++;
		}
	}
}

/*
 * Is the dynamic block of slot i one of literal codewords of (nearly) ONE
 * length?  The final rule of one_length_code() (host_stream.hip) on the code
 * lengths lda_stream_hdr_cache_kernel left in the slot: of the first
 * min(HLIT + 257, 256) lengths, `hi` is the longest in use and `top` the most
 * frequent, and the block is such a one when the codewords of length `top` are
 * at least 32, fill 98 % of the code space and hi <= 11.  cls[i] = { hi or 0,
 * bits from the header to the block's first token }; a slot whose header did
 * not parse gives { 0, 0 }.  A lane per slot; the histogram is four 64-bit
 * registers of four 16-bit counters each (no indexed array: no scratch).
 */
extern "C" __global__ void __launch_bounds__(64)
lda_stream_hdr_class_kernel(const u32 *__restrict__ ncand, u32 nslots,
			    const u8 *__restrict__ hdr_lens, const u32 *__restrict__ hdr_info,
			    uint2 *__restrict__ cls)
{
	u32 nc = *ncand;
	nc = nc < nslots ? nc : nslots;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= nc)
		return;
	const u32 nlit = hdr_info[4 * (size_t)i], used = hdr_info[4 * (size_t)i + 2];
	u32 res = 0;
	if (nlit) {
		const u32 want = nlit < 256 ? nlit : 256;
		const u32 *lens = (const u32 *)(hdr_lens + (size_t)i * 320);
		u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0;	/* lengths 0-3, 4-7, 8-11, 12-15 */
		for (u32 w = 0; 4 * w < want; w++) {
			const u32 four = lens[w];
#pragma unroll
			for (u32 k = 0; k < 4; k++) {
				const u32 len = (four >> (8 * k)) & 15;
				const u64 one = 4 * w + k < want ? 1ull << (16 * (len & 3)) : 0;
				h0 += (len >> 2) == 0 ? one : 0;
				h1 += (len >> 2) == 1 ? one : 0;
				h2 += (len >> 2) == 2 ? one : 0;
				h3 += (len >> 2) == 3 ? one : 0;
			}
		}
		u32 hi = 0, top = 1, ntop = (u32)(h0 >> 16) & 0xFFFF;
#pragma unroll
		for (u32 len = 1; len < 16; len++) {
			const u64 h = len < 4 ? h0 : len < 8 ? h1 : len < 12 ? h2 : h3;
			const u32 c = (u32)(h >> (16 * (len & 3))) & 0xFFFF;
			if (c)
				hi = len;
			if (c > ntop) {
				top = len;
				ntop = c;
			}
		}
		if (ntop >= 32 && hi <= 11 && 50 * ntop >= 49 * (1u << top))
			res = hi;
	}
	cls[i] = make_uint2(res, nlit ? used : 0);
}
