/*
 * png_write_kernels.hip - PNG files written in device memory
 * (host_png_write.hip: libdeflate_amd_png_encode_batch; the columns are those
 * of png_write_plan.h).
 *
 *   lda_pngw_filter{4,16,64}_kernel
 *                           the scanlines of every image, filtered, into the
 *                           image's room in the scratch: a group of 4, 16 or 64
 *                           lanes per row, 16 bytes per lane and step
 *   (the Adler-32 batch over the pieces of the rooms, the compress batches into
 *    the slots, the CRC-32 batch over the compressed pieces)
 *   lda_pngw_image_kernel   a wave per image: the pieces' compressed sizes
 *                           summed, the image's Adler-32 and the IDAT chunk's
 *                           CRC-32 combined from the pieces', the file's size
 *   (the scan kernels of compact_kernels.hip over those sizes)
 *   lda_pngw_place_kernel   a wave per image: signature, IHDR, PLTE, tRNS, the
 *                           IDAT chunk's frame, IEND, every piece's source and
 *                           destination, the index row
 *   lda_zipw_copy_kernel    (zip_write_kernels.hip) the pieces
 *   lda_pngw_final_kernel   d_result
 *
 * The last three write nothing into the files or the index unless all of the
 * files fit out_avail.  Plain C++, vector stores only; no loop bound is a byte
 * of an image.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"
#include "png_write_plan.h"

#define PW_ADAPTIVE lda::PNGW_FILTER_ADAPTIVE
#define PW_LE16 PNGW_META_LE16
#define PW_OFF_MASK PNGW_OFF_MASK
/* column a of the n images' / the np pieces' */
#define PW_ICOL(a) (icols + (u64)lda::PNGW_I_##a * n)
#define PW_PCOL(a) (pcols + (u64)lda::ZIPW_P_##a * np)
#define PW_H 0x80808080u
#define PW_X32 0xEDB88320u	/* x^32 mod P: what appending four bytes multiplies a CRC by */

/* ---- the filter kernel ---- */

/* byte-wise a - b */
static __device__ __forceinline__ u32 pw_sub8(u32 a, u32 b)
{
	return ((a | PW_H) - (b & ~PW_H)) ^ ((a ^ ~b) & PW_H);
}

/* byte-wise (a + b) >> 1 of the 9-bit sums */
static __device__ __forceinline__ u32 pw_avg8(u32 a, u32 b)
{
	return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1);
}

/* byte-wise Paeth predictor: a left, b above, c above left; ties a, b, c */
static __device__ __forceinline__ u32 pw_paeth8(u32 a, u32 b, u32 c)
{
	u32 r = 0;
#pragma unroll
	for (u32 k = 0; k < 32; k += 8) {
		const s32 A = (a >> k) & 0xFF, B = (b >> k) & 0xFF, C = (c >> k) & 0xFF;
		const s32 pa = B > C ? B - C : C - B, pb = A > C ? A - C : C - A;
		const s32 t = A + B - 2 * C, pc = t < 0 ? -t : t;
		const s32 pred = pa <= pb && pa <= pc ? A : pb <= pc ? B : C;
		r |= (u32)pred << k;
	}
	return r;
}

/* the sum of the bytes of x & mask read as signed, in absolute value */
static __device__ __forceinline__ u32 pw_abs_sum(u32 x, u32 mask, u32 acc)
{
	const u32 neg = ((x & PW_H) >> 7) * 0xFFu;	/* 0xFF in every negative byte */
	const u32 mag = (x & ~neg) | (pw_sub8(0, x) & neg);
	return __builtin_amdgcn_sad_u8(mag & mask, 0, acc);
}

static __device__ __forceinline__ uint4 pw_swap16(uint4 v)
{
	v.x = ((v.x & 0x00FF00FFu) << 8) | ((v.x >> 8) & 0x00FF00FFu);
	v.y = ((v.y & 0x00FF00FFu) << 8) | ((v.y >> 8) & 0x00FF00FFu);
	v.z = ((v.z & 0x00FF00FFu) << 8) | ((v.z >> 8) & 0x00FF00FFu);
	v.w = ((v.w & 0x00FF00FFu) << 8) | ((v.w >> 8) & 0x00FF00FFu);
	return v;
}

/* the 16 bytes `unit` (1 .. 8) bytes in front of v's, zeros in front of v */
static __device__ __forceinline__ uint4 pw_shift_in(uint4 v, u32 unit)
{
	const u64 lo = (u64)v.y << 32 | v.x, hi = (u64)v.w << 32 | v.z;
	const u32 s = 8 * unit;		/* 8 .. 64 */
	const u64 nlo = s < 64 ? lo << s : 0;
	const u64 nhi = s < 64 ? hi << s | lo >> (64 - s) : lo;
	return make_uint4((u32)nlo, (u32)(nlo >> 32), (u32)nhi, (u32)(nhi >> 32));
}

/* the 16 bytes at in + off; bytes at or past n read as 0.  (load16_guard() with
 * its ragged end rolled up: twelve copies of it stand in every filter kernel) */
static __device__ __forceinline__ uint4 pw_load16(const u8 *__restrict__ in, u64 off, u64 n)
{
	uint4 v = { 0, 0, 0, 0 };
	if (off + 16 <= n) {
		__builtin_memcpy(&v, in + off, 16);
	} else {
		u64 lo = 0, hi = 0;
#pragma nounroll
		for (u32 k = 0; k < 8; k++) {
			lo |= (u64)(off + k < n ? in[off + k] : 0) << (8 * k);
			hi |= (u64)(off + 8 + k < n ? in[off + 8 + k] : 0) << (8 * k);
		}
		v = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
	}
	return v;
}

/* what a piece's filters read: the row's bytes, the row above's, and the bytes
 * one filter unit in front of each */
struct pw_piece {
	uint4 cur, left, up, upleft;
};

/*
 * Piece x0 / 16 of the row at pix + row_at (pix_n: the image's pixel bytes, so
 * no load reads past them): bytes in front of the row and above the first row
 * are zero, bytes past the row's end are whatever follows (the caller masks
 * them).
 */
static __device__ __forceinline__ pw_piece
pw_load(const u8 *__restrict__ pix, u64 pix_n, u64 row_at, u64 rb, u32 x0, u32 unit, bool top,
	bool le16)
{
	pw_piece p;
	const uint4 zero = { 0, 0, 0, 0 };

	p.cur = pw_load16(pix, row_at + x0, pix_n);
	p.up = top ? zero : pw_load16(pix, row_at - rb + x0, pix_n);
	if (x0) {
		p.left = pw_load16(pix, row_at + x0 - unit, pix_n);
		p.upleft = top ? zero : pw_load16(pix, row_at - rb + x0 - unit, pix_n);
	}
	if (le16) {
		p.cur = pw_swap16(p.cur);
		p.up = pw_swap16(p.up);
		if (x0) {
			p.left = pw_swap16(p.left);
			p.upleft = pw_swap16(p.upleft);
		}
	}
	if (!x0) {
		p.left = pw_shift_in(p.cur, unit);
		p.upleft = pw_shift_in(p.up, unit);
	}
	return p;
}

/* the piece filtered with type t (PNG 9.2) */
static __device__ __forceinline__ uint4 pw_filter(const pw_piece &p, u32 t)
{
	uint4 r = p.cur;

	if (t == 1) {
		r = make_uint4(pw_sub8(p.cur.x, p.left.x), pw_sub8(p.cur.y, p.left.y),
			       pw_sub8(p.cur.z, p.left.z), pw_sub8(p.cur.w, p.left.w));
	} else if (t == 2) {
		r = make_uint4(pw_sub8(p.cur.x, p.up.x), pw_sub8(p.cur.y, p.up.y),
			       pw_sub8(p.cur.z, p.up.z), pw_sub8(p.cur.w, p.up.w));
	} else if (t == 3) {
		r = make_uint4(pw_sub8(p.cur.x, pw_avg8(p.left.x, p.up.x)),
			       pw_sub8(p.cur.y, pw_avg8(p.left.y, p.up.y)),
			       pw_sub8(p.cur.z, pw_avg8(p.left.z, p.up.z)),
			       pw_sub8(p.cur.w, pw_avg8(p.left.w, p.up.w)));
	} else if (t == 4) {
		r = make_uint4(pw_sub8(p.cur.x, pw_paeth8(p.left.x, p.up.x, p.upleft.x)),
			       pw_sub8(p.cur.y, pw_paeth8(p.left.y, p.up.y, p.upleft.y)),
			       pw_sub8(p.cur.z, pw_paeth8(p.left.z, p.up.z, p.upleft.z)),
			       pw_sub8(p.cur.w, pw_paeth8(p.left.w, p.up.w, p.upleft.w)));
	}
	return r;
}

/* the first nvalid (0 .. 16) bytes of v read as signed, their absolute sum */
static __device__ __forceinline__ u32 pw_piece_sum(uint4 v, u32 nvalid)
{
	const u32 w[4] = { v.x, v.y, v.z, v.w };
	u32 acc = 0;
#pragma unroll
	for (u32 i = 0; i < 4; i++) {
		const u32 have = nvalid > 4 * i ? nvalid - 4 * i : 0;
		const u32 mask = have >= 4 ? ~0u : (1u << (8 * have)) - 1;
		acc = pw_abs_sum(w[i], mask, acc);
	}
	return acc;
}

/* 16 bytes where the row has them, its ragged end byte by byte; dst is at no
 * particular alignment */
static __device__ __forceinline__ void pw_store(u8 *__restrict__ dst, uint4 v, u32 nvalid)
{
	if (nvalid >= 16) {
		__builtin_memcpy(dst, &v, 16);
	} else {
		u64 lo = (u64)v.y << 32 | v.x, hi = (u64)v.w << 32 | v.z;
#pragma nounroll
		for (u32 k = 0; k < nvalid; k++) {
			dst[k] = (u8)lo;
			lo = lo >> 8 | hi << 56;
			hi >>= 8;
		}
	}
}

/* the least of five sums, the lowest type on ties */
template <typename T> static __device__ __forceinline__ u32 pw_argmin(const T *s)
{
	u32 best = 0;
#pragma unroll
	for (u32 t = 1; t < 5; t++)
		if (s[t] < s[best])
			best = t;
	return best;
}

/*
 * Work item it: rows [first, first + rows) of image k.  Group g of the
 * workgroup's 256 / G takes the rows first + g, first + g + 256 / G, ...; lane
 * j of the group the pieces j, j + G, ... of its row.
 */
template <u32 G>
static __device__ __forceinline__ void
pw_filter_items(u64 n, u64 n_items, u32 filter, const u64 *__restrict__ work,
		const u64 *__restrict__ icols, const u8 *__restrict__ in, u8 *__restrict__ scan)
{
	const u32 GROUPS = 256 / G;
	const u32 grp = threadIdx.x / G, j = threadIdx.x % G;

	for (u64 it = blockIdx.x; it < n_items; it += gridDim.x) {
		const u64 k = work[2 * it], span = work[2 * it + 1];
		const u32 first = (u32)span, rows = (u32)(span >> 32);
		const u64 geom = PW_ICOL(GEOM)[k], meta = PW_ICOL(META)[k];
		const u64 height = geom & 0xFFFFFFFFu, rb = geom >> 32;
		const u32 unit = (u32)(meta >> 24) & 0xFF;
		const bool le16 = (meta & PW_LE16) != 0;
		const u8 *pix = in + PW_ICOL(PIX)[k];
		u8 *room = scan + PW_ICOL(ROOM)[k];
		const u64 pix_n = height * rb;
		const u32 np = (u32)((rb + 15) / 16);

		for (u32 r = grp; r < rows; r += GROUPS) {
			const u64 y = (u64)first + r, row_at = y * rb;
			u8 *dst = room + y * (rb + 1);
			u32 type = filter;

			if (filter == PW_ADAPTIVE && np <= G) {
				/* one pass: the five pieces stay in registers */
				const u32 x0 = 16 * j;
				const u32 nvalid = j >= np ? 0 : rb - x0 < 16 ? (u32)(rb - x0) : 16;
				uint4 f[5];
				u32 s[5];
				pw_piece p = { };
				if (nvalid)
					p = pw_load(pix, pix_n, row_at, rb, x0, unit, y == 0, le16);
#pragma unroll
				for (u32 t = 0; t < 5; t++) {
					f[t] = pw_filter(p, t);
					s[t] = pw_piece_sum(f[t], nvalid);
				}
#pragma unroll
				for (u32 off = G / 2; off; off >>= 1)
#pragma unroll
					for (u32 t = 0; t < 5; t++)
						s[t] += __shfl_xor(s[t], off, 64);
				type = pw_argmin(s);
				uint4 v = f[0];
#pragma unroll
				for (u32 t = 1; t < 5; t++)
					if (type == t)
						v = f[t];
				pw_store(dst + 1 + x0, v, nvalid);
				if (j == 0)
					dst[0] = (u8)type;
				continue;
			}
			if (filter == PW_ADAPTIVE) {
				/* a lane has at most 2^26 bytes of 128 each: 64 bits */
				u64 s[5] = { 0, 0, 0, 0, 0 };
				for (u32 pc = j; pc < np; pc += G) {
					const u64 x0 = 16 * (u64)pc;
					const u32 nvalid = rb - x0 < 16 ? (u32)(rb - x0) : 16;
					const pw_piece p = pw_load(pix, pix_n, row_at, rb, (u32)x0, unit,
								   y == 0, le16);
#pragma unroll
					for (u32 t = 0; t < 5; t++)
						s[t] += pw_piece_sum(pw_filter(p, t), nvalid);
				}
#pragma unroll
				for (u32 off = G / 2; off; off >>= 1)
#pragma unroll
					for (u32 t = 0; t < 5; t++) {
						const u32 lo = __shfl_xor((u32)s[t], off, 64);
						const u32 hi = __shfl_xor((u32)(s[t] >> 32), off, 64);
						s[t] += (u64)hi << 32 | lo;
					}
				type = pw_argmin(s);
			}
			/* the chosen type alone (of a long row the second read: L2) */
			for (u32 pc = j; pc < np; pc += G) {
				const u64 x0 = 16 * (u64)pc;
				const u32 nvalid = rb - x0 < 16 ? (u32)(rb - x0) : 16;
				const pw_piece p = pw_load(pix, pix_n, row_at, rb, (u32)x0, unit,
							   y == 0, le16);
				pw_store(dst + 1 + x0, pw_filter(p, type), nvalid);
			}
			if (j == 0)
				dst[0] = (u8)type;
		}
	}
}

/* n: the images of the batch, whose columns icols holds; one launch per class
 * of rows with the class's items */
#define PW_FILTER_KERNEL(G)                                                                     \
	extern "C" __global__ void __launch_bounds__(256)                                       \
	lda_pngw_filter##G##_kernel(u64 n, u64 n_items, u32 filter, const u64 *__restrict__ work, \
				    const u64 *__restrict__ icols, const u8 *__restrict__ in,   \
				    u8 *__restrict__ scan)                                      \
	{                                                                                       \
		pw_filter_items<G>(n, n_items, filter, work, icols, in, scan);                  \
	}
PW_FILTER_KERNEL(4)
PW_FILTER_KERNEL(16)
PW_FILTER_KERNEL(64)

/* ---- the assembly kernels ---- */

/* pw_mulmod() and lda_crc_powmod() (large_plan.h) with the 32 steps of the
 * multiply rolled up: these kernels multiply in many places and a wave per
 * image has time, unrolled they cost scalar registers the kernels do not have */
static __device__ __forceinline__ u32 pw_mulmod(u32 a, u32 b)
{
	u32 p = 0;
#pragma nounroll
	for (u32 m = 0x80000000u; m; m >>= 1) {
		p ^= a & m ? b : 0;
		b = (b >> 1) ^ (0xEDB88320u & (0 - (b & 1)));
	}
	return p;
}

/* x^(8 k) mod P */
static __device__ __forceinline__ u32 pw_xpow8(u64 k)
{
	u32 xp = 0x80000000u, base = ZW_X8;
#pragma nounroll
	for (; k; k >>= 1) {
		if (k & 1)
			xp = pw_mulmod(xp, base);
		base = pw_mulmod(base, base);
	}
	return xp;
}

/*
 * One wave: the CRC-32 of the n (at most 64 * 13) bytes byte_at(0 .. n - 1),
 * in every lane.  Every lane takes a contiguous run bit by bit; the runs are
 * combined as zw_combine() combines pieces.
 */
template <typename F> static __device__ __forceinline__ u32 pw_wave_crc(u32 lane, u32 n, F byte_at)
{
	const u32 run = (n + 63) / 64;
	const u32 a = lane * run < n ? lane * run : n;
	const u32 b = a + run < n ? a + run : n;
	u32 crc = ~0u;

	for (u32 i = a; i < b; i++) {
		crc ^= byte_at(i);
#pragma unroll
		for (u32 k = 0; k < 8; k++)
			crc = (crc >> 1) ^ (0xEDB88320u & (0 - (crc & 1)));
	}
	crc = a < b ? ~crc : 0;
	if (a < b && b < n)
		crc = pw_mulmod(crc, pw_xpow8(n - b));
	return wave_xor(crc);
}

/* v's NBYTES low bytes, big endian, at any alignment */
template <u32 NBYTES> static __device__ __forceinline__ void pw_put_be(u8 *p, u64 v)
{
#pragma unroll
	for (u32 i = 0; i < NBYTES; i++)
		p[i] = (u8)(v >> (8 * (NBYTES - 1 - i)));
}

/* byte i of the 13 of an IHDR */
static __device__ __forceinline__ u32 pw_ihdr_byte(u32 i, u64 dims, u64 meta)
{
	if (i < 4)
		return ((u32)dims >> (8 * (3 - i))) & 0xFF;
	if (i < 8)
		return ((u32)(dims >> 32) >> (8 * (7 - i))) & 0xFF;
	if (i == 8)
		return (u32)meta & 0xFF;
	if (i == 9)
		return (u32)(meta >> 8) & 0xFF;
	return 0;	/* compression, filter method, interlace */
}

/* the size of a chunk of n data bytes that is there when n != 0 */
static __device__ __forceinline__ u64 pw_opt_chunk(u64 n)
{
	return n ? 12 + n : 0;
}

/*
 * Image k, pieces first[k] .. + count[k] of its scanlines: csize[k] the bytes
 * of its DEFLATE stream, adler[k] the Adler-32 of the scanlines (combined as
 * lda_large_finalize_kernel combines it), crc[k] the CRC-32 of the IDAT chunk -
 * "IDAT" and the two bytes of the zlib header (crc_head: the host's), the
 * pieces' COMPRESSED bytes, the Adler-32 - and sizes[k] the file: head, zlib stream, the chunk's CRC, IEND.
 * zw_combine()'s sibling: the multipliers are powers of the compressed lengths.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pngw_image_kernel(u64 n, u64 np, u32 crc_head, const u64 *__restrict__ icols,
		      const u64 *__restrict__ pcols, const u64 *__restrict__ out_n,
		      const u32 *__restrict__ adlers, const u32 *__restrict__ crcs,
		      u64 *__restrict__ csize, u32 *__restrict__ adler, u32 *__restrict__ crc,
		      u64 *__restrict__ sizes)
{
	const u64 *pc_off = PW_PCOL(PC_OFF), *pc_n = PW_PCOL(PC_N);
	const u32 lane = threadIdx.x & 63;
	const u32 M = 65521;

	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 f = PW_ICOL(FIRST)[k], cnt = PW_ICOL(COUNT)[k], us = PW_ICOL(SCAN)[k];
		const u64 run = (cnt + 63) / 64;
		const u64 a = lane * run < cnt ? lane * run : cnt;
		const u64 b = a + run < cnt ? a + run : cnt;
		u64 mine = 0, sa = 0, sb = 0;
		u32 acc = 0;

		for (u64 i = a; i < b; i++) {
			const u64 len = out_n[f + i];
			const u32 ad = adlers[f + i];
			const u32 ai = ((ad & 0xFFFF) + M - 1) % M, bi = (ad >> 16) % M;
			const u64 t = us - (pc_off[f + i] + pc_n[f + i] - pc_off[f]);
			acc = pw_mulmod(acc, pw_xpow8(len)) ^ crcs[f + i];
			mine += len;
			sa = (sa + ai) % M;
			sb = (sb + bi + (t % M) * ai) % M;
		}
		const u64 upto = wave_scan_incl64(mine);
		const u64 cs = wave_sum64(mine);
		if (a < b && cs - upto)
			acc = pw_mulmod(acc, pw_xpow8(cs - upto));
		const u32 pieces = wave_xor(acc);
		sa = wave_sum64(sa);
		sb = wave_sum64(sb);
		const u32 sum = (u32)(sb % M) << 16 | (u32)((1 + sa) % M);
		if (lane == 0) {
			/* the chunk's CRC-32: crc_head over "IDAT" and the zlib header,
			 * the pieces, the Adler-32's four bytes */
			u32 tail = ~0u ^ __builtin_bswap32(sum);
#pragma nounroll
			for (u32 i = 0; i < 32; i++)
				tail = (tail >> 1) ^ (0xEDB88320u & (0 - (tail & 1)));
			csize[k] = cs;
			adler[k] = sum;
			crc[k] = pw_mulmod(crc_head, pw_xpow8(cs + 4)) ^
				 pw_mulmod(pieces, PW_X32) ^ ~tail;
			sizes[k] = PW_ICOL(HEAD)[k] + 2 + cs + 4 + 4 + 12;
		}
	}
}

/*
 * offsets / block_sums: the scan kernels' output over sizes[], so image k's
 * file stands at offsets[k] + block_sums[k / LDA_SCAN_BLOCK] and all files
 * together take the grand total.  Writes the file's fixed parts (PLTE and tRNS
 * from `in`), piece j's copy (cp_src with ZW_FROM_SLOT into the slots; cp_dst
 * into the file; cp_len) and, index not NULL, the row
 * libdeflate_amd_png_index_batch returns for the file.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pngw_place_kernel(u64 n, u64 np, int level, u64 out_avail, const u64 *__restrict__ icols,
		      const u64 *__restrict__ pcols, const u64 *__restrict__ out_n,
		      const u64 *__restrict__ csize, const u32 *__restrict__ adler,
		      const u32 *__restrict__ crc, const u64 *__restrict__ offsets,
		      const u64 *__restrict__ block_sums, const u8 *__restrict__ in,
		      u8 *__restrict__ out, u64 *__restrict__ cp_src, u64 *__restrict__ cp_dst,
		      u64 *__restrict__ cp_len, u64 *__restrict__ index)
{
	const u32 lane = threadIdx.x & 63;
	const u64 total = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (total > out_avail)
		return;
	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 at = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
		const u64 dm = PW_ICOL(DIMS)[k], meta = PW_ICOL(META)[k], cs = csize[k];
		const u64 hd = PW_ICOL(HEAD)[k], plte = PW_ICOL(PLTE)[k], trns = PW_ICOL(TRNS)[k];
		const u64 pl_n = plte >> 48, tr_n = trns >> 48;
		const u8 *pl = in + (plte & PW_OFF_MASK), *tr = in + (trns & PW_OFF_MASK);
		u8 *file = out + at;
		u8 *pchunk = file + 33, *tchunk = pchunk + pw_opt_chunk(3 * pl_n);
		u8 *idat = file + hd - 8, *z = file + hd;

		if (lane < 8)
			file[lane] = (u8)(0x0A1A0A0D474E5089ull >> (8 * lane));
		/* IHDR, PLTE, tRNS: one body for the three, so one copy of the CRC */
#pragma nounroll
		for (u32 c = 0; c < 3; c++) {
			const u32 len = c == 0 ? 13 : c == 1 ? (u32)(3 * pl_n) : (u32)tr_n;
			const u32 tag = c == 0 ? 0x49484452u : c == 1 ? 0x504C5445u : 0x74524E53u;
			const u8 *src = c == 1 ? pl : tr;
			u8 *chunk = c == 0 ? file + 8 : c == 1 ? pchunk : tchunk;
			if (!len)
				continue;
			const u32 sum = pw_wave_crc(lane, 4 + len, [=](u32 i) {
				return i < 4 ? (tag >> (8 * (3 - i))) & 0xFF :
				       c == 0 ? pw_ihdr_byte(i - 4, dm, meta) : (u32)src[i - 4];
			});
			for (u32 i = lane; i < len; i += 64)
				chunk[8 + i] = c == 0 ? (u8)pw_ihdr_byte(i, dm, meta) : src[i];
			if (lane == 0) {
				pw_put_be<4>(chunk, len);
				pw_put_be<4>(chunk + 4, tag);
				pw_put_be<4>(chunk + 8 + len, sum);
			}
		}
		if (lane == 32) {
			pw_put_be<4>(idat, 2 + cs + 4);
			pw_put_be<4>(idat + 4, 0x49444154u);
			pw_put_be<2>(z, lda_zlib_header(level));
		} else if (lane == 33) {
			pw_put_be<4>(z + 2 + cs, adler[k]);
			pw_put_be<4>(z + 2 + cs + 4, crc[k]);
		} else if (lane == 34) {
			u8 *iend = z + 2 + cs + 8;
			pw_put_be<4>(iend, 0);
			pw_put_be<4>(iend + 4, 0x49454E44u);
			pw_put_be<4>(iend + 8, 0xAE426082u);	/* the CRC-32 of "IEND" */
		} else if (lane == 35 && index) {
			u64 *row = index + LDA_PNG_WORDS * k;
			row[0] = at;
			row[1] = hd + 2 + cs + 4 + 4 + 12;
			row[2] = dm;
			row[3] = meta & ~PW_LE16;
			row[4] = at + hd - 8;
			row[5] = 2 + cs + 4;
			row[6] = pl_n ? (at + 33 + 8) | pl_n << 48 : 0;
			row[7] = tr_n ? (at + 33 + pw_opt_chunk(3 * pl_n) + 8) | tr_n << 48 : 0;
		}
		zw_place_pieces(lane, PW_ICOL(FIRST)[k], PW_ICOL(COUNT)[k], at + hd + 2, true,
				PW_PCOL(PC_OFF), PW_PCOL(PC_N), PW_PCOL(SLOT_OFF), out_n, cp_src, cp_dst,
				cp_len);
	}
}

/* result[0] = 0 or LIBDEFLATE_INSUFFICIENT_SPACE, [1] the files' bytes in all,
 * [2] the pixels' bytes, [3] the images */
extern "C" __global__ void __launch_bounds__(64)
lda_pngw_final_kernel(u64 n, u64 pixels_total, u64 out_avail, const u64 *__restrict__ total_at,
		      u64 *__restrict__ result)
{
	if (threadIdx.x != 0)
		return;
	const u64 total = *total_at;
	result[0] = total <= out_avail ? LDA_SUCCESS : LDA_INSUFFICIENT_SPACE;
	result[1] = total;
	result[2] = pixels_total;
	result[3] = n;
}
