/*
 * exr_kernels.hip - the coding of OpenEXR's ZIP and ZIPS chunks undone and
 * applied in device memory (host_exr.hip: libdeflate_amd_exr_decode_batch;
 * host_exr_write.hip: libdeflate_amd_exr_encode_batch).  exr_plan.h states the
 * transforms and builds the rows; tools/models/exr_model.py restates them on
 * the CPU.
 *
 * Undoing a chunk of n bytes is one byte-wise running sum over all of p, minus
 * 128 per place - an XOR of 0x80 at every odd place -, and then the interleave
 * of the sum's two halves.  The work is the bytes, not the chunks: a tile is
 * LDA_EXR_TILE raw bytes of one chunk and belongs to one wave, a workgroup of
 * four waves takes four tiles, and the workgroups stride over the tiles of all
 * chunks; a wave finds its chunk by a binary search in the prefix column
 * u_tile_end.  Tile j reads two stretches of p, 1024 bytes each, 16 bytes a
 * lane: A_j from the first half and B_j from the second (exr_plan.h).  Three
 * launches, and no workgroup waits for another of its own launch:
 *
 *   lda_exr_sums_kernel   every stretch's byte sum (v_sad_u8, a wave reduce)
 *                         into its slot
 *   lda_exr_carry_kernel  a wave per chunk: the slots' exclusive sums, in place
 *   lda_exr_undo_kernel   a lane sums its 16 bytes of either stretch as packed
 *                         bytes in four dwords (padd8: no carry leaves a byte),
 *                         the lanes' totals are scanned across the wave with DPP
 *                         shifts, the slot's carry is added, the odd places are
 *                         flipped, and v_perm_b32 interleaves the 16 + 16 bytes
 *                         into the 32 the lane stores
 *
 * The bytes behind a stretch's end are read as zeros (load16_guard), so a tile
 * never depends on what lies behind its chunk's n bytes, and only bytes in
 * front of n are stored.
 *
 * lda_exr_layout_kernel moves raw chunks to their lines at a pitch (LINES) or
 * to interleaved pixels (PIXELS); lda_exr_gather_kernel is its inverse, for
 * the writer.  Both walk exr_plan.h's layout rows in tiles of LDA_EXR_LTILE
 * items, a thread an item.  With samples of one size and up to four channels
 * an item is 16 bytes of every channel's plane on the raw side and c * 16
 * contiguous bytes on the pixel side, transposed in registers; the last pixels
 * of a line, and every other mix of channels, go sample by sample.
 *
 * lda_exr_code_kernel is the forward coding: every coded byte depends on two
 * raw bytes, so a thread makes 16 bytes of p from 32 raw bytes (v_perm_b32
 * picks the even or the odd ones) and the one in front, with one packed
 * subtraction.  lda_exrw_choose_kernel takes the zlib stream where it is
 * shorter than raw, and lda_exrw_place_kernel, a wave per chunk, writes the
 * head, dataSize, the zlib header and footer, lists the copies of the pieces -
 * from the slots or from the raw room - and writes the reader's row.
 *
 * The undo and layout kernels also run over chunks whose inflate failed: the
 * scratch is then anything.  Every address and loop bound comes from the
 * plan's rows, never from a byte, so they stay inside the rooms and the lines.
 * Nothing spins.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"

#define EXR_H 0x80808080u
#define EXR_STRETCH (LDA_EXR_TILE / 2)

static __device__ __forceinline__ void ex_load16(const u8 *p, u32 *w)
{
	uint4 v;
	__builtin_memcpy(&v, p, 16);	/* (may be unaligned) */
	w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

static __device__ __forceinline__ void ex_store16(u8 *p, const u32 *w)
{
	const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
	__builtin_memcpy(p, &v, 16);	/* (may be unaligned) */
}

/* a + b and a - b per byte: the top bits apart, so that nothing crosses a byte */
static __device__ __forceinline__ u32 padd8(u32 a, u32 b)
{
	return ((a & ~EXR_H) + (b & ~EXR_H)) ^ ((a ^ b) & EXR_H);
}

static __device__ __forceinline__ u32 psub8(u32 a, u32 b)
{
	return ((a | EXR_H) - (b & ~EXR_H)) ^ ((a ^ ~b) & EXR_H);
}

/* the row of tile t: the first whose tile_end is above t (n >= 1) */
static __device__ __forceinline__ u64 ex_find(const u64 *__restrict__ tile_end, u64 n, u64 t)
{
	u64 lo = 0, hi = n - 1;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (tile_end[mid] > t)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

/* a wave's tile: its chunk, the stretches' places in p and their slots */
struct ex_tile {
	const u8 *p;	/* the chunk's room */
	u64 dst;
	u32 n, h, j;
	u64 slot_a, slot_b;
};

static __device__ __forceinline__ ex_tile
ex_tile_of(u64 n_u, u64 t, const u64 *__restrict__ ucols, const u8 *__restrict__ coded)
{
	const u64 *tile_end = ucols, *src = ucols + n_u, *un = ucols + 2 * n_u, *dst = ucols + 3 * n_u;
	const u64 k = ex_find(tile_end, n_u, t);
	const u64 t0 = k ? tile_end[k - 1] : 0;
	ex_tile x;
	x.p = coded + src[k];
	x.dst = dst[k];
	x.n = (u32)un[k];
	x.h = (u32)(((u64)x.n + 1) >> 1);
	x.j = (u32)(t - t0);
	x.slot_a = 2 * t0 + x.j;
	x.slot_b = 2 * t0 + (tile_end[k] - t0) + x.j;
	return x;
}

/* the lane's 16 bytes of stretch A and of stretch B; zeros behind their ends */
static __device__ __forceinline__ void ex_load_pair(const ex_tile &x, u32 lane, u32 *a, u32 *b)
{
	const u64 at = (u64)x.j * EXR_STRETCH + 16 * lane;
	const uint4 va = load16_guard(x.p, at, x.h);
	const uint4 vb = load16_guard(x.p, (u64)x.h + at, x.n);
	a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
	b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
}

/* the wave of this thread and the waves of the grid: tiles are dealt to waves */
static __device__ __forceinline__ u64 ex_first_tile(void)
{
	return (u64)blockIdx.x * LDA_EXR_WG_TILES +
	       (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

extern "C" __global__ void __launch_bounds__(256)
lda_exr_sums_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *__restrict__ ucols,
		    const uint8_t *__restrict__ coded, uint32_t *__restrict__ slots)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 t = ex_first_tile(); t < n_tiles; t += (u64)gridDim.x * LDA_EXR_WG_TILES) {
		const ex_tile x = ex_tile_of(n_u, t, ucols, coded);
		u32 a[4], b[4], sa = 0, sb = 0;
		ex_load_pair(x, lane, a, b);
#pragma unroll
		for (u32 k = 0; k < 4; k++) {
			sa = __builtin_amdgcn_sad_u8(a[k], 0, sa);
			sb = __builtin_amdgcn_sad_u8(b[k], 0, sb);
		}
		sa = wave_sum(sa);
		sb = wave_sum(sb);
		if (lane == 0) {
			slots[x.slot_a] = sa & 0xFF;
			slots[x.slot_b] = sb & 0xFF;
		}
	}
}

/* chunk k's slots 2 * (tiles in front) .. + 2 * (its tiles): every slot becomes
 * the sum, modulo 256, of the slots in front of it in its chunk */
extern "C" __global__ void __launch_bounds__(256)
lda_exr_carry_kernel(uint64_t n_u, const uint64_t *__restrict__ u_tile_end,
		     uint32_t *__restrict__ slots)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 k = (u64)blockIdx.x * 4 + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	     k < n_u; k += (u64)gridDim.x * 4) {
		const u64 t0 = k ? u_tile_end[k - 1] : 0;
		const u64 cnt = 2 * (u_tile_end[k] - t0);
		u32 *s = slots + 2 * t0;
		u32 run = 0;
		for (u64 base = 0; base < cnt; base += 64) {
			const bool live = base + lane < cnt;
			const u32 v = live ? s[base + lane] : 0;
			const u32 incl = wave_scan_incl(v);
			if (live)
				s[base + lane] = (run + incl - v) & 0xFF;
			run += (u32)__builtin_amdgcn_readlane((int)incl, 63);
		}
	}
}

/* the running sum of the lane's 16 bytes, packed; -> the last byte's sum in
 * every byte */
static __device__ __forceinline__ u32 ex_scan16(u32 *w)
{
	u32 carry = 0;
#pragma unroll
	for (u32 k = 0; k < 4; k++) {
		u32 v = w[k];
		v = padd8(v, v << 8);
		v = padd8(v, v << 16);
		v = padd8(v, carry);
		w[k] = v;
		carry = (v >> 24) * 0x01010101u;
	}
	return carry;
}

/* the lanes' sums made the wave's: every byte of w plus the bytes of all lanes
 * below and `carry`; then the odd places flipped.  odd0: w's byte 0 stands at an
 * odd place of p */
static __device__ __forceinline__ void ex_finish(u32 *w, u32 total, u32 carry, bool odd0)
{
	const u32 t = total & 0xFF;
	const u32 base = ((wave_scan_incl(t) - t + carry) & 0xFF) * 0x01010101u;
	const u32 flip = odd0 ? 0x00800080u : 0x80008000u;
#pragma unroll
	for (u32 k = 0; k < 4; k++)
		w[k] = padd8(w[k], base) ^ flip;
}

extern "C" __global__ void __launch_bounds__(256)
lda_exr_undo_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *__restrict__ ucols,
		    const uint8_t *__restrict__ coded, const uint32_t *__restrict__ slots,
		    uint8_t *__restrict__ raw, uint8_t *__restrict__ out)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 t = ex_first_tile(); t < n_tiles; t += (u64)gridDim.x * LDA_EXR_WG_TILES) {
		const ex_tile x = ex_tile_of(n_u, t, ucols, coded);
		u32 a[4], b[4], o[8];
		ex_load_pair(x, lane, a, b);
		const u32 ta = ex_scan16(a), tb = ex_scan16(b);
		/* (a stretch starts at an even place of its half: j * 1024 + 16 * lane) */
		ex_finish(a, ta, slots[x.slot_a], false);
		ex_finish(b, tb, slots[x.slot_b], (x.h & 1) != 0);
#pragma unroll
		for (u32 m = 0; m < 4; m++) {
			/* v_perm_b32: selector bytes 0 .. 3 take the second operand's bytes, 4 .. 7 the first's */
			o[2 * m] = __builtin_amdgcn_perm(b[m], a[m], 0x05010400u);
			o[2 * m + 1] = __builtin_amdgcn_perm(b[m], a[m], 0x07030602u);
		}
		const u64 at = (u64)x.j * LDA_EXR_TILE + LDA_EXR_LANE * lane;
		if (at >= x.n)
			continue;
		u8 *dst = (x.dst & LDA_EXR_DST_OUT ? out + (x.dst & ~LDA_EXR_DST_OUT) : raw + x.dst) + at;
		if (at + LDA_EXR_LANE <= x.n) {
			ex_store16(dst, o);
			ex_store16(dst + 16, o + 4);
		} else {
			const u32 left = (u32)(x.n - at);
#pragma unroll
			for (u32 i = 0; i < LDA_EXR_LANE; i++)
				if (i < left)
					dst[i] = (u8)(o[i >> 2] >> (8 * (i & 3)));
		}
	}
}

/* ---- the layouts ---- */

struct ex_lrow {
	u64 raw, pix, pitch;
	u32 w, lines, c, mask, layout;
	u64 doff0, doff1;
};

static __device__ __forceinline__ u32 ex_doff(const ex_lrow &r, u32 k)
{
	return (u32)((k < 8 ? r.doff0 >> (8 * k) : r.doff1 >> (8 * (k - 8))) & 0xFF);
}

/* n bytes (2 or 4) from src to dst, at any alignment */
static __device__ __forceinline__ void ex_sample(const u8 *src, u8 *dst, u32 n)
{
	if (n == 4) {
		u32 v;
		__builtin_memcpy(&v, src, 4);
		__builtin_memcpy(dst, &v, 4);
	} else {
		u16 v;
		__builtin_memcpy(&v, src, 2);
		__builtin_memcpy(dst, &v, 2);
	}
}

/* pixels x0 .. x1 - 1 of a line, sample by sample.  rawl, pixl: the line on
 * either side */
template <bool TO_PIXELS>
static __device__ __forceinline__ void
ex_pixels_slow(const ex_lrow &r, u32 px, const u8 *rawl, const u8 *pixl, u8 *raww, u8 *pixw, u32 x0,
	       u32 x1)
{
	u32 plane = 0;
	for (u32 k = 0; k < r.c; k++) {
		const u32 sz = (r.mask >> k & 1) ? 4 : 2, d = ex_doff(r, k);
		for (u32 x = x0; x < x1; x++) {
			const u64 ro = (u64)plane + (u64)x * sz, po = (u64)x * px + d;
			if (TO_PIXELS)
				ex_sample(rawl + ro, pixw + po, sz);
			else
				ex_sample(pixl + po, raww + ro, sz);
		}
		plane += sz * r.w;
	}
}

/* 16 / SZ pixels of C channels of SZ bytes through the registers: P[q] the 16
 * bytes of the plane that fills slot q, O the C * 16 bytes of the pixels */
template <u32 SZ, u32 C, bool TO_PIXELS>
static __device__ __forceinline__ void ex_transpose(u32 (&P)[C][4], u32 (&O)[4 * C])
{
	if (TO_PIXELS) {
#pragma unroll
		for (u32 i = 0; i < 4 * C; i++)
			O[i] = 0;
	} else {
#pragma unroll
		for (u32 q = 0; q < C; q++)
			P[q][0] = P[q][1] = P[q][2] = P[q][3] = 0;
	}
#pragma unroll
	for (u32 x = 0; x < 16 / SZ; x++) {
#pragma unroll
		for (u32 q = 0; q < C; q++) {
			const u32 e = x * C + q;	/* the sample's place among the pixels' */
			if (SZ == 4) {
				if (TO_PIXELS)
					O[e] = P[q][x];
				else
					P[q][x] = O[e];
			} else if (TO_PIXELS) {
				O[e >> 1] |= ((P[q][x >> 1] >> (16 * (x & 1))) & 0xFFFFu) << (16 * (e & 1));
			} else {
				P[q][x >> 1] |= ((O[e >> 1] >> (16 * (e & 1))) & 0xFFFFu) << (16 * (x & 1));
			}
		}
	}
}

template <u32 SZ, u32 C, bool TO_PIXELS>
static __device__ __forceinline__ void
ex_pixels_fast(const ex_lrow &r, const u8 *rawl, const u8 *pixl, u8 *raww, u8 *pixw, u32 x0)
{
	u32 P[C][4], O[4 * C];
	u32 plane_of[C] = { 0 };	/* the plane that fills slot q */

#pragma unroll
	for (u32 k = 0; k < C; k++) {
		const u32 q = ex_doff(r, k) / SZ;
#pragma unroll
		for (u32 qq = 0; qq < C; qq++)
			if (qq == q)
				plane_of[qq] = k * SZ * r.w;
	}
	const u64 po = (u64)x0 * (SZ * C);
	if (TO_PIXELS) {
#pragma unroll
		for (u32 q = 0; q < C; q++)
			ex_load16(rawl + plane_of[q] + (u64)x0 * SZ, P[q]);
		ex_transpose<SZ, C, true>(P, O);
#pragma unroll
		for (u32 q = 0; q < C; q++)
			ex_store16(pixw + po + 16 * q, O + 4 * q);
	} else {
#pragma unroll
		for (u32 q = 0; q < C; q++)
			ex_load16(pixl + po + 16 * q, O + 4 * q);
		ex_transpose<SZ, C, false>(P, O);
#pragma unroll
		for (u32 q = 0; q < C; q++)
			ex_store16(raww + plane_of[q] + (u64)x0 * SZ, P[q]);
	}
}

/* item `it` of row r.  raw_r / pix_r: what is read on either side, raw_w / pix_w:
 * what is written (one of each pair is used) */
template <bool TO_PIXELS>
static __device__ __forceinline__ void
ex_item(const ex_lrow &r, u64 it, const u8 *raw_r, const u8 *pix_r, u8 *raw_w, u8 *pix_w)
{
	const u32 c = r.c;
	u32 px = 0;
	for (u32 k = 0; k < c; k++)
		px += (r.mask >> k & 1) ? 4 : 2;
	const u32 lb = r.w * px;
	const bool uniform = c <= 4 && (r.mask == 0 || r.mask == (1u << c) - 1);
	const u32 sz = r.mask ? 4 : 2;
	const u32 G = r.layout == LDA_EXR_LAYOUT_LINES ? 16 : uniform ? 16 / sz : 1;
	const u32 per_line = r.layout == LDA_EXR_LAYOUT_LINES ? (lb + 15) / 16 : (r.w + G - 1) / G;
	/* (the items of a row are fewer than its bytes: below 2^32) */
	const u32 y = (u32)it / per_line, g = (u32)it - y * per_line;

	if (y >= r.lines)
		return;
	const u64 ro = r.raw + (u64)y * lb, po = r.pix + (u64)y * r.pitch;
	const u8 *rawl = raw_r + ro, *pixl = pix_r + po;
	u8 *raww = raw_w + ro, *pixw = pix_w + po;

	if (r.layout == LDA_EXR_LAYOUT_LINES) {
		const u32 off = 16 * g, len = lb - off < 16 ? lb - off : 16;
		const u8 *src = TO_PIXELS ? rawl + off : pixl + off;
		u8 *dst = TO_PIXELS ? pixw + off : raww + off;
		if (len == 16) {
			u32 v[4];
			ex_load16(src, v);
			ex_store16(dst, v);
		} else {
			for (u32 i = 0; i < len; i++)
				dst[i] = src[i];
		}
		return;
	}
	const u32 x0 = g * G;
	if (!uniform || x0 + G > r.w) {
		ex_pixels_slow<TO_PIXELS>(r, px, rawl, pixl, raww, pixw, x0, x0 + G < r.w ? x0 + G : r.w);
		return;
	}
	switch (sz * 8 + c) {
	case 2 * 8 + 1: ex_pixels_fast<2, 1, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 2 * 8 + 2: ex_pixels_fast<2, 2, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 2 * 8 + 3: ex_pixels_fast<2, 3, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 2 * 8 + 4: ex_pixels_fast<2, 4, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 4 * 8 + 1: ex_pixels_fast<4, 1, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 4 * 8 + 2: ex_pixels_fast<4, 2, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	case 4 * 8 + 3: ex_pixels_fast<4, 3, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	default: ex_pixels_fast<4, 4, TO_PIXELS>(r, rawl, pixl, raww, pixw, x0); break;
	}
}

/* tile t of all rows: its row and the thread's item in it */
static __device__ __forceinline__ u64
ex_lrow_of(u64 n_l, u64 t, const u64 *__restrict__ lcols, ex_lrow &r)
{
	const u64 k = ex_find(lcols, n_l, t);
	r.raw = lcols[1 * n_l + k];
	r.pix = lcols[2 * n_l + k];
	r.pitch = lcols[3 * n_l + k];
	r.w = (u32)lcols[4 * n_l + k];
	r.lines = (u32)(lcols[4 * n_l + k] >> 32);
	const u64 fmt = lcols[5 * n_l + k];
	r.c = (u32)(fmt & 0xFF);
	r.mask = (u32)(fmt >> 8) & 0xFFFF;
	r.layout = (u32)(fmt >> 32);
	r.doff0 = lcols[6 * n_l + k];
	r.doff1 = lcols[7 * n_l + k];
	return (t - (k ? lcols[k - 1] : 0)) * LDA_EXR_LTILE + threadIdx.x;
}

/* raw chunks -> lines or pixels in out.  A row's raw chunk lies in d_in
 * (LDA_EXR_RAW_IN) or in the raw area */
extern "C" __global__ void __launch_bounds__(256)
lda_exr_layout_kernel(uint64_t n_l, uint64_t n_tiles, const uint64_t *__restrict__ lcols,
		      const uint8_t *__restrict__ in, const uint8_t *__restrict__ raw,
		      uint8_t *__restrict__ out)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		ex_lrow r;
		const u64 it = ex_lrow_of(n_l, t, lcols, r);
		const u8 *base = r.raw & LDA_EXR_RAW_IN ? in : raw;
		r.raw &= ~LDA_EXR_RAW_IN;
		ex_item<true>(r, it, base, NULL, NULL, out);
	}
}

/* the inverse: lines or pixels in `in` -> raw chunks in the raw area */
extern "C" __global__ void __launch_bounds__(256)
lda_exr_gather_kernel(uint64_t n_l, uint64_t n_tiles, const uint64_t *__restrict__ lcols,
		      const uint8_t *__restrict__ in, uint8_t *__restrict__ raw)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		ex_lrow r;
		const u64 it = ex_lrow_of(n_l, t, lcols, r);
		ex_item<false>(r, it, NULL, in, raw, NULL);
	}
}

/* ---- the writer ---- */

/* byte k of t: the even bytes of raw, then the odd ones */
static __device__ __forceinline__ u32 ex_t(const u8 *raw, u32 h, u32 k)
{
	return raw[k < h ? 2 * (u64)k : 2 * (u64)(k - h) + 1];
}

/* tile t of all chunks: LDA_EXR_CTILE bytes of one chunk's coded room from its
 * raw room, 16 a thread; the two rooms stand at the same offset of their areas */
extern "C" __global__ void __launch_bounds__(256)
lda_exr_code_kernel(uint64_t n, uint64_t n_tiles, const uint64_t *__restrict__ ecols,
		    const uint8_t *__restrict__ raw_area, uint8_t *__restrict__ coded_area)
{
	/* exr_plan.h: EXRW_E_USIZE 2, _ROOM, _CTILE_END */
	const u64 *usize = ecols + 2 * n, *room = ecols + 3 * n, *tile_end = ecols + 4 * n;

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 k = ex_find(tile_end, n, t);
		const u64 at64 = (t - (k ? tile_end[k - 1] : 0)) * LDA_EXR_CTILE + 16 * threadIdx.x;
		const u32 nb = (u32)usize[k], h = (u32)(((u64)nb + 1) >> 1);
		if (at64 >= nb)	/* (the room ends on a 16-byte boundary behind nb) */
			continue;
		const u32 at = (u32)at64;
		const u8 *raw = raw_area + room[k];
		u32 T[4], P[4];

		const bool first = at >= 16 && (u64)at + 16 <= h;
		const bool second = at > h && (u64)at + 16 <= nb;
		if (first || second) {
			/* t[at .. at + 15] are every other byte of 32 raw bytes; t[at - 1] two in front */
			const u8 *src = first ? raw + 2 * (u64)at : raw + 2 * (u64)(at - h);
			const u32 sel = first ? 0x06040200u : 0x07050301u;
			const u32 prev = first ? src[-2] : src[-1];
			u32 R[8];
			ex_load16(src, R);
			ex_load16(src + 16, R + 4);
#pragma unroll
			for (u32 m = 0; m < 4; m++)
				T[m] = __builtin_amdgcn_perm(R[2 * m + 1], R[2 * m], sel);
			P[0] = psub8(T[0], T[0] << 8 | prev) ^ EXR_H;
#pragma unroll
			for (u32 m = 1; m < 4; m++)
				P[m] = psub8(T[m], T[m] << 8 | T[m - 1] >> 24) ^ EXR_H;
		} else {
			P[0] = P[1] = P[2] = P[3] = 0;
			for (u32 i = 0; i < 16 && (u64)at + i < nb; i++) {
				const u32 q = at + i;
				const u32 v = q ? ex_t(raw, h, q) - ex_t(raw, h, q - 1) + 128 : ex_t(raw, h, 0);
				P[i >> 2] |= (v & 0xFF) << (8 * (i & 3));
			}
		}
		*(uint4 *)(coded_area + room[k] + at) = make_uint4(P[0], P[1], P[2], P[3]);
	}
}

/* the decision of the format: chunk k's data is its zlib stream - sizes[k] as
 * lda_shufw_chunk_kernel left it: header, stream, footer - where that is
 * shorter than raw, else raw.  dsize[k] the data's bytes, sizes[k] the chunk's
 * with its head */
extern "C" __global__ void __launch_bounds__(256)
lda_exrw_choose_kernel(uint64_t n, const uint64_t *__restrict__ ecols, uint64_t *__restrict__ dsize,
		       uint64_t *__restrict__ sizes)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= n)
		return;
	const u64 raw = ecols[2 * n + k], stream = sizes[k];
	const u64 head = ecols[(LDA_EXRW_E_WORDS + 5) * n + k];
	const u64 data = stream < raw ? stream : raw;
	dsize[k] = data;
	sizes[k] = head + data;
}

/*
 * offsets / block_sums: the scan kernels' output over sizes[].  Writes chunk
 * k's head - the ints of words 8 and 9, then dataSize -, of a zlib chunk the
 * stream's header and Adler-32, every piece's copy (from its slot, or of a raw
 * chunk from the raw area, where the pieces' ranges are the coded area's) and,
 * index not NULL, the reader's row.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_exrw_place_kernel(uint64_t n, int level, uint64_t out_avail, const uint64_t *__restrict__ ecols,
		      const uint64_t *__restrict__ pc_off, const uint64_t *__restrict__ pc_n,
		      const uint64_t *__restrict__ slot_off, const uint64_t *__restrict__ out_n,
		      const uint64_t *__restrict__ csize, const uint32_t *__restrict__ sum,
		      const uint64_t *__restrict__ dsize, const uint64_t *__restrict__ offsets,
		      const uint64_t *__restrict__ block_sums, uint8_t *__restrict__ out,
		      uint64_t *__restrict__ cp_src, uint64_t *__restrict__ cp_dst,
		      uint64_t *__restrict__ cp_len, uint64_t *__restrict__ index)
{
	const u64 *first = ecols, *count = ecols + n, *usize = ecols + 2 * n;
	const u64 *words = ecols + LDA_EXRW_E_WORDS * n;	/* words 2 .. 9, n each */
	const u32 lane = threadIdx.x & 63;
	const u64 total = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (total > out_avail)
		return;
	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 head = words[5 * n + k], h0 = words[6 * n + k], h1 = words[7 * n + k];
		const u64 at = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
		const u64 data = dsize[k], cs = csize[k];
		const bool deflated = data < usize[k];
		u8 *mem = out + at, *body = mem + head;

		if (lane == 0 && head == 8) {
			zw_put<4>(mem, (u32)h0);
			zw_put<4>(mem + 4, data);
		} else if (lane == 0 && head == 20) {
			zw_put<8>(mem, h0);
			zw_put<8>(mem + 8, h1);
			zw_put<4>(mem + 16, data);
		} else if (lane == 1 && deflated) {
			const u32 hw = lda_zlib_header(level);
			body[0] = (u8)(hw >> 8);
			body[1] = (u8)hw;
			zw_put<4>(body + 2 + cs, __builtin_bswap32(sum[k]));
		} else if (lane == 2 && index) {
			u64 *row = index + LDA_EXR_WORDS * k;
			row[0] = at + head;
			row[1] = data;
#pragma unroll
			for (u32 a = 0; a < 8; a++)
				row[2 + a] = words[a * n + k];
		}
		zw_place_pieces(lane, first[k], count[k], at + head + (deflated ? 2 : 0), deflated, pc_off,
				pc_n, slot_off, out_n, cp_src, cp_dst, cp_len);
	}
}
