/*
 * seek_kernels.hip - the kernels of the seek index (host_seek.hip) that need
 * nothing of the decoder:
 *
 *   lda_seek_window_kernel    behind a decode: the 32 KiB of output in front
 *                             of every point (zeros in front of the stream)
 *                             into the caller's window array.
 *   lda_seek_resolve_kernel   one PIECE - one range's share of one interval -
 *                             from the 16-bit symbols lda_seek_decode_kernel
 *                             left in the interval's slot to bytes at the
 *                             piece's place in the output: a marker 0x8000 | i
 *                             is byte i of the interval's stored window.
 *   lda_seek_verdict_kernel   a range's result from its pieces' intervals.
 *
 * The window is gathered from global memory (it is 32 KiB per interval, read
 * by a few thousand lanes that mostly hit the same lines), as
 * lda_stream_resolve_kernel does; no LDS staging until a measurement asks.
 */
#include "device_common.h"
#include "stream_kernels.h"

#define SEEK_WIN 32768u

extern "C" __global__ void __launch_bounds__(256)
lda_seek_window_kernel(u32 npoints, const u64 *__restrict__ out_off,
		       const u8 *__restrict__ out, u8 *__restrict__ windows)
{
	const u32 k = blockIdx.x;
	if (k >= npoints)
		return;
	const u64 at = out_off[k];
	u8 *w = windows + (size_t)k * SEEK_WIN;
	for (u32 i = 8 * threadIdx.x; i < SEEK_WIN; i += 8 * 256) {
		/* byte i of the window is output byte at + i - 32768 */
		u64 v = 0;
		if (at + i >= SEEK_WIN) {
			__builtin_memcpy(&v, out + (at + i - SEEK_WIN), 8);
		} else {
			for (u32 b = 0; b < 8; b++)
				if (at + i + b >= SEEK_WIN)
					v |= (u64)out[at + i + b - SEEK_WIN] << (8 * b);
		}
		__builtin_memcpy(w + i, &v, 8);
	}
}

static __device__ __forceinline__ u32
seek_byte(u32 s, const u8 *__restrict__ win, u32 lowest, bool *bad)
{
	if (s & 0x8000) {
		const u32 i = s & 0x7FFF;
		if (i < lowest) {	/* in front of the stream's first byte */
			*bad = true;
			return 0;
		}
		return win[i];
	}
	return s & 0xFF;
}

/* grid.y: the pieces piece0 .. (the host launches batches: grid.y <= 65535);
 * grid.x: the piece's words of 8 bytes, strided */
extern "C" __global__ void __launch_bounds__(256)
lda_seek_resolve_kernel(u32 npieces, u32 piece0, const u64 *__restrict__ pieces,
			const u64 *__restrict__ win_of, const u32 *__restrict__ lowest,
			const u16 *__restrict__ sym, const u8 *__restrict__ windows,
			u8 *__restrict__ out, u32 *__restrict__ fail)
{
	const u32 p = piece0 + blockIdx.y;
	if (p >= npieces)
		return;
	const u32 j = (u32)pieces[4 * (size_t)p];
	const u16 *s = sym + pieces[4 * (size_t)p + 1];
	u8 *dst = out + pieces[4 * (size_t)p + 2];
	const u64 len = pieces[4 * (size_t)p + 3];
	if (fail[j] == 1)
		return;		/* (the gate wrote no symbols: nothing of this interval lands) */
	const u8 *win = windows + (size_t)win_of[j] * SEEK_WIN;
	const u32 low = lowest[j];
	/* bytes up to the first 8-byte boundary of the destination, whole words,
	 * the bytes behind them */
	u64 head = (8 - ((uintptr_t)dst & 7)) & 7;
	head = head < len ? head : len;
	const u64 nbody = (len - head) / 8, tail = len - head - 8 * nbody;
	bool bad = false;
	for (u64 q = (u64)blockIdx.x * 256 + threadIdx.x; q < nbody; q += 256ull * gridDim.x) {
		uint4 v;
		__builtin_memcpy(&v, s + head + 8 * q, 16);
		const u32 w[4] = { v.x, v.y, v.z, v.w };
		u64 r = 0;
#pragma unroll
		for (u32 t = 0; t < 4; t++) {
			r |= (u64)seek_byte(w[t] & 0xFFFF, win, low, &bad) << (16 * t);
			r |= (u64)seek_byte(w[t] >> 16, win, low, &bad) << (16 * t + 8);
		}
		*(u64 *)(dst + head + 8 * q) = r;
	}
	if (blockIdx.x == 0 && threadIdx.x < 16) {
		const u32 t = threadIdx.x;
		u64 at = len;
		if (t < 8 && t < head)
			at = t;
		else if (t >= 8 && t - 8 < tail)
			at = head + 8 * nbody + (t - 8);
		if (at < len)
			dst[at] = (u8)seek_byte(s[at], win, low, &bad);
	}
	if (bad)
		fail[j] = 2;
}

extern "C" __global__ void __launch_bounds__(256)
lda_seek_verdict_kernel(u32 nranges, const u64 *__restrict__ first,
			const u64 *__restrict__ pieces, const u32 *__restrict__ fail,
			int32_t *__restrict__ results)
{
	const u32 r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nranges)
		return;
	u32 bad = 0;
	for (u64 p = first[r]; p < first[r + 1]; p++)
		bad |= fail[(u32)pieces[4 * p]];
	results[r] = bad ? 1 : 0;	/* LIBDEFLATE_BAD_DATA */
}
