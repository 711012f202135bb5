/*
 * large_plan.h - the arithmetic of ONE large buffer compressed as segments
 * (host_compress.hip: compress_large() from host memory,
 * libdeflate_amd_compress_large_batch() from device memory), in the one place
 * both forms take it from: the host loop and the descriptor kernel
 * (large_kernels.hip) compile the same functions, so the two streams cannot
 * drift apart.
 */
#ifndef LDA_LARGE_PLAN_H
#define LDA_LARGE_PLAN_H

/* (a host compiler takes the arithmetic alone: tools/test_zip_write_plan.cpp) */
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <stdint.h>

#define LDA_SEG_BYTES 65536u
#define LDA_LARGE_MIN (2 * LDA_SEG_BYTES)
/* input bytes of one compress launch of the segmented forms */
#define LDA_LARGE_SLICE_BYTES ((uint64_t)32 << 20)

/* does a single-buffer call of n bytes run as segments?  (inputs of 4 GiB and
 * more always do: the kernels index a chunk with 32 bits) */
static __host__ __device__ inline bool
lda_large_segmented(uint64_t n, int level, bool no_segments)
{
	return n >= LDA_LARGE_MIN && level > 0 && (!no_segments || n >= 0xFFFF0000u);
}

/* sub-ranges of 64 KiB; an input that would not fill the CUs with those is cut
 * finer (more blocks and sync markers: ~1 % larger at 16 KiB).  env_seg:
 * LDA_SEG_BYTES, 0 = by size */
static __host__ __device__ inline uint64_t
lda_large_seg_bytes(uint64_t n, uint64_t env_seg)
{
	if (env_seg)
		return env_seg;
	if (n <= ((uint64_t)4 << 20))
		return 16384;
	if (n <= ((uint64_t)8 << 20))
		return 32768;
	return LDA_SEG_BYTES;
}

/* segments per compress launch */
static __host__ __device__ inline uint64_t
lda_large_per_slice(uint64_t S)
{
	const uint64_t k = LDA_LARGE_SLICE_BYTES / S;
	return k ? k : 1;
}

/*
 * n bytes at offset in_at of the input base, cut into nseg sub-ranges of S
 * (the last one shorter), segment i compressed into the slot at out_at +
 * i * slot of the output base.  D: the most bytes of its predecessors that
 * prime a segment (dict_window()), tile: the granularity they come in.
 */
struct lda_large_shape {
	uint64_t n, S, D, tile, nseg, slot, in_at, out_at;
};

/* a segment's rows of the batch descriptors, and its seg_info word: the prime
 * in whole tiles, bit 31 on the last segment */
struct lda_large_seg {
	uint64_t in_off, in_n;		/* what the compress kernel reads: the prime in front */
	uint64_t out_off, out_av;	/* its slot */
	uint64_t pc_off, pc_n;		/* the piece itself: what the checksum covers */
	uint32_t info;
};

static __host__ __device__ inline lda_large_seg
lda_large_seg_of(const lda_large_shape &g, uint64_t i)
{
	const uint64_t before = i * g.S;
	const uint64_t prime = i ? (g.D < before ? g.D : before) / g.tile * g.tile : 0;
	const uint64_t len = i + 1 < g.nseg ? g.S : g.n - before;
	lda_large_seg s;
	s.in_off = g.in_at + before - prime;
	s.in_n = prime + len;
	s.out_off = g.out_at + i * g.slot;
	s.out_av = g.slot;
	s.pc_off = g.in_at + before;
	s.pc_n = len;
	s.info = (uint32_t)prime | (i + 1 == g.nseg ? 0x80000000u : 0);
	return s;
}

/* multiply two reflected polynomials mod the CRC-32 polynomial (bit 31 = x^0);
 * bit by bit: CDNA4 has no carry-less multiply */
static __host__ __device__ inline uint32_t lda_crc_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m; m >>= 1) {
		if (a & m)
			p ^= b;
		b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}

/* base^k mod P */
static __host__ __device__ inline uint32_t lda_crc_powmod(uint32_t base, uint64_t k)
{
	uint32_t xp = 0x80000000u;	/* 1 */
	for (; k; k >>= 1) {
		if (k & 1)
			xp = lda_crc_mulmod(xp, base);
		base = lda_crc_mulmod(base, base);
	}
	return xp;
}

/* the container around the raw stream (lib/gzip_compress.c:44-79,
 * lib/zlib_compress.c:45-72): gzip's XFL and zlib's first two bytes by level */
static __host__ __device__ inline uint8_t lda_gzip_xfl(int level)
{
	return level < 2 ? 4 : level >= 8 ? 2 : 0;
}

static __host__ __device__ inline uint32_t lda_zlib_header(int level)
{
	const uint32_t fl = level < 2 ? 0 : level < 6 ? 1 : level < 8 ? 2 : 3;
	uint32_t hw = (0x78u << 8) | (fl << 6);
	hw |= 31 - (hw % 31);
	return hw;
}

#endif /* LDA_LARGE_PLAN_H */
