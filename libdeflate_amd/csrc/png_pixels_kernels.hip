/*
 * png_pixels_kernels.hip - PNG images converted to one pixel format
 * (host_png_pixels.hip, include/libdeflate_amd.h): the selections that are not
 * yet the format, unfiltered into the scratch in PNG order, written into their
 * rooms of d_out as interleaved pixels of 1 .. 4 channels and 8 or 16 bits.
 * tools/models/png_pixels_model.py restates it on the CPU.
 *
 * The work is the pixels, not the images: a tile is LDA_PNGX_TILE = 4096
 * consecutive pixels of one selection, 16 to a thread, and the workgroups
 * stride over the tiles of all converted selections; a tile finds its
 * selection by a binary search in the prefix column x_tile_end (one word per
 * converted selection; x_sel says which selection of the call it is), the
 * same in every lane.  A thread's 16 pixels are 16 .. 128 bytes of output, a whole
 * number of 16-byte pieces, stored as such wherever the address falls (the
 * rooms start on out_align, which may be 1); only the last thread of an image
 * stores bytes.  The source is loaded in 16-byte pieces where the 16 pixels lie
 * in one scanline, and pixel by pixel where they straddle scanlines (a width
 * below 16, the padding bits of a row below 8 bits per pixel).
 *
 * The kernel is three steps with the pixels in registers between them, each
 * chosen per tile by values that are uniform in the workgroup, so that no
 * step branches per pixel: fetch<bits per pixel> (9), canon<depth, colour,
 * 16-bit output> (12 pairs x 2: the palette, the colour key, the depth; -> R, G, B, A of
 * 16 bits each at the output's depth) and store<channels, 16-bit output> (8:
 * the grey formula, the alpha dropped or kept, the byte order).
 *
 * It also runs over selections whose inflate or unfilter failed: the scratch
 * is then anything.  Every address comes from the plan's descriptors (width,
 * height, the rooms, the PLTE and tRNS ranges checked by png_plan.h), never
 * from a pixel: a palette index is at most 255 and reads the 256 words in LDS,
 * where the entries the file does not have are zero and make the selection's
 * flag 1.  The flags are zeroed by the host; lanes that meet a bad index all
 * store the same 1.  Nothing spins and no workgroup waits for another.
 */
#include "device_common.h"
#include "kernels.h"

static __device__ __forceinline__ u32 pngx_channels(u32 colour)
{
	return colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 1;
}

/* SB bytes at byte o of the words q[0 .. N), o and SB known at compile time */
template <u32 N, u32 SB>
static __device__ __forceinline__ u64 bytes_at(const u64 (&q)[N], u32 o)
{
	const u32 i = o >> 3, sh = 8 * (o & 7);
	u64 v = q[i] >> sh;
	if (sh && 8 * SB + sh > 64 && i + 1 < N)
		v |= q[i + 1] << (64 - sh);
	return SB == 8 ? v : v & (((u64)1 << (8 * (SB & 7))) - 1);
}

/*
 * The `count` pixels from pixel p0 on of an image of `width` pixels a row and
 * rowbytes bytes a row at src -> raw[j]: the pixel's bytes in memory order from
 * bit 0 up for 8 bits and more, its value below that.
 */
template <u32 BITS>
static __device__ __forceinline__ void
fetch(const u8 *__restrict__ src, u64 src_n, u32 width, u32 rowbytes, u64 p0, u32 count,
      u64 (&raw)[16])
{
	u32 y = (u32)(p0 / width);
	u32 x = (u32)(p0 - (u64)y * width);
	const bool wide = count == 16 && x + 16 <= width;

	if constexpr (BITS >= 8) {
		constexpr u32 SB = BITS / 8;
		if (wide) {
			const u8 *p = src + (u64)y * rowbytes + (u64)x * SB;
			u64 q[2 * SB];
#pragma unroll
			for (u32 i = 0; i < SB; i++) {
				uint4 v;
				__builtin_memcpy(&v, p + 16 * i, 16);	/* (may be unaligned) */
				q[2 * i] = v.x | (u64)v.y << 32;
				q[2 * i + 1] = v.z | (u64)v.w << 32;
			}
#pragma unroll
			for (u32 j = 0; j < 16; j++)
				raw[j] = bytes_at<2 * SB, SB>(q, j * SB);
		} else {
#pragma unroll
			for (u32 j = 0; j < 16; j++) {
				u64 v = 0;
				if (j < count) {
					const u8 *p = src + (u64)y * rowbytes + (u64)x * SB;
#pragma unroll
					for (u32 k = 0; k < SB; k++)
						v |= (u64)p[k] << (8 * k);
					if (++x == width) {
						x = 0;
						y++;
					}
				}
				raw[j] = v;
			}
		}
	} else {
		constexpr u32 MASK = (1u << BITS) - 1;
		if (wide) {
			const u64 bo = (u64)x * BITS;
			const uint4 v = load16_guard(src, (u64)y * rowbytes + (bo >> 3), src_n);
			const u32 sh = (u32)bo & 7;
			u64 hi = __builtin_bswap64(v.x | (u64)v.y << 32);
			const u64 lo = __builtin_bswap64(v.z | (u64)v.w << 32);
			if (sh)
				hi = hi << sh | lo >> (64 - sh);
#pragma unroll
			for (u32 j = 0; j < 16; j++)
				raw[j] = (hi >> (64 - BITS * (j + 1))) & MASK;
		} else {
#pragma unroll
			for (u32 j = 0; j < 16; j++) {
				u64 v = 0;
				if (j < count) {
					const u64 bo = (u64)x * BITS;
					const u32 b = src[(u64)y * rowbytes + (bo >> 3)];
					v = (b >> (8 - BITS - ((u32)bo & 7))) & MASK;
					if (++x == width) {
						x = 0;
						y++;
					}
				}
				raw[j] = v;
			}
		}
	}
}

/* a sample of depth D at the output's depth: bit replication upwards, round to
 * nearest downwards (png_set_scale_16) */
template <u32 D, bool OUT16>
static __device__ __forceinline__ u32 scale(u32 v)
{
	if constexpr (D == 1)
		v *= 0xFF;
	else if constexpr (D == 2)
		v *= 0x55;
	else if constexpr (D == 4)
		v *= 0x11;
	if constexpr (D == 16)
		return OUT16 ? v : (v * 255 + 32895) >> 16;
	else
		return OUT16 ? v * 257 : v;
}

/* sample k of a raw pixel of 8 bits and more */
template <u32 D>
static __device__ __forceinline__ u32 sample(u64 raw, u32 k)
{
	if constexpr (D == 16) {
		const u32 v = (u32)(raw >> (16 * k)) & 0xFFFF;
		return (v & 0xFF) << 8 | v >> 8;	/* big-endian in the file */
	} else if constexpr (D == 8) {
		return (u32)(raw >> (8 * k)) & 0xFF;
	} else {
		return (u32)raw;
	}
}

struct PngxKey {
	bool on;
	u32 r, g, b;	/* at the file's depth */
};

/*
 * raw[j] -> R | G << 16 | B << 32 | A << 48 at the output's depth: the
 * palette, the colour key on the unscaled samples, the depth.  Returns whether
 * a palette index at or above `entries` was met.
 */
template <u32 D, u32 COLOUR, bool OUT16>
static __device__ __forceinline__ bool
canon(u64 (&px)[16], const u32 *pal, u32 entries, const PngxKey &key)
{
	constexpr u32 MAXD = (1u << D) - 1;
	bool bad = false;
#pragma unroll
	for (u32 j = 0; j < 16; j++) {
		const u64 raw = px[j];
		u32 r, g, b, a;
		if constexpr (COLOUR == 3) {
			const u32 i = (u32)raw & 0xFF;
			const u32 w = pal[i];
			bad |= i >= entries;
			r = scale<8, OUT16>(w & 0xFF);
			g = scale<8, OUT16>(w >> 8 & 0xFF);
			b = scale<8, OUT16>(w >> 16 & 0xFF);
			a = scale<8, OUT16>(w >> 24);
		} else if constexpr (COLOUR == 0 || COLOUR == 4) {
			const u32 v = sample<D>(raw, 0);
			a = COLOUR == 4 ? sample<D>(raw, 1) : key.on && v == key.r ? 0 : MAXD;
			r = g = b = scale<D, OUT16>(v);
			a = scale<D, OUT16>(a);
		} else {
			r = sample<D>(raw, 0);
			g = sample<D>(raw, 1);
			b = sample<D>(raw, 2);
			a = COLOUR == 6 ? sample<D>(raw, 3) :
			    key.on && r == key.r && g == key.g && b == key.b ? 0 : MAXD;
			r = scale<D, OUT16>(r);
			g = scale<D, OUT16>(g);
			b = scale<D, OUT16>(b);
			a = scale<D, OUT16>(a);
		}
		px[j] = (u64)r | (u64)g << 16 | (u64)b << 32 | (u64)a << 48;
	}
	return bad;
}

/* a 16-bit sample as it lies in memory, read as a little-endian value */
static __device__ __forceinline__ u64 mem16(u32 v, bool le16)
{
	return le16 ? v : (v & 0xFF) << 8 | v >> 8;
}

/*
 * The `count` pixels px[] -> CH channels of 8 or 16 bits at dst: the 16 pixels
 * packed into OPP pieces of 16 bytes, a piece stored whole where all of it is
 * pixels of this image, byte by byte at the image's end.
 */
template <u32 CH, bool OUT16>
static __device__ __forceinline__ void
store(const u64 (&px)[16], u8 *__restrict__ dst, u32 count, bool le16)
{
	constexpr u32 OPP = CH * (OUT16 ? 2 : 1);	/* bytes per pixel, pieces per thread */
	constexpr u32 SHS = OUT16 ? 16 : 8;
	u32 w[4 * OPP];
#pragma unroll
	for (u32 i = 0; i < 4 * OPP; i++)
		w[i] = 0;
#pragma unroll
	for (u32 j = 0; j < 16; j++) {
		const u32 r = (u32)px[j] & 0xFFFF, g = (u32)(px[j] >> 16) & 0xFFFF,
			  b = (u32)(px[j] >> 32) & 0xFFFF, a = (u32)(px[j] >> 48);
		u64 pv = 0;
		auto put = [&](u32 k, u32 v) {
			pv |= (OUT16 ? mem16(v, le16) : (u64)v) << (SHS * k);
		};
		if constexpr (CH <= 2) {
			put(0, (19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
			if constexpr (CH == 2)
				put(1, a);
		} else {
			put(0, r);
			put(1, g);
			put(2, b);
			if constexpr (CH == 4)
				put(3, a);
		}
		const u32 o = j * OPP, i = o >> 2, sh = 8 * (o & 3);
		const u64 lo = pv << sh;
		w[i] |= (u32)lo;
		if (i + 1 < 4 * OPP)
			w[i + 1] |= (u32)(lo >> 32);
		if (sh && 8 * OPP + sh > 64 && i + 2 < 4 * OPP)
			w[i + 2] |= (u32)(pv >> (64 - sh));
	}
	const u32 valid = count * OPP;
#pragma unroll
	for (u32 i = 0; i < OPP; i++) {
		if (16 * i + 16 <= valid) {
			const uint4 v = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
			__builtin_memcpy(dst + 16 * i, &v, 16);	/* (may be unaligned) */
		} else {
#pragma unroll
			for (u32 k = 0; k < 16; k++)
				if (16 * i + k < valid)
					dst[16 * i + k] = (u8)(w[4 * i + (k >> 2)] >> (8 * (k & 3)));
		}
	}
}

template <bool OUT16>
static __device__ __forceinline__ bool
canon_any(u32 depth, u32 colour, u64 (&px)[16], const u32 *pal, u32 entries, const PngxKey &key)
{
	switch (colour << 8 | depth) {
	case 0 << 8 | 1: return canon<1, 0, OUT16>(px, pal, entries, key);
	case 0 << 8 | 2: return canon<2, 0, OUT16>(px, pal, entries, key);
	case 0 << 8 | 4: return canon<4, 0, OUT16>(px, pal, entries, key);
	case 0 << 8 | 8: return canon<8, 0, OUT16>(px, pal, entries, key);
	case 0 << 8 | 16: return canon<16, 0, OUT16>(px, pal, entries, key);
	case 2 << 8 | 8: return canon<8, 2, OUT16>(px, pal, entries, key);
	case 2 << 8 | 16: return canon<16, 2, OUT16>(px, pal, entries, key);
	/* an index below 8 bits is its value, at 8 bits its byte: one rule */
	case 3 << 8 | 1: case 3 << 8 | 2: case 3 << 8 | 4: case 3 << 8 | 8:
		return canon<8, 3, OUT16>(px, pal, entries, key);
	case 4 << 8 | 8: return canon<8, 4, OUT16>(px, pal, entries, key);
	case 4 << 8 | 16: return canon<16, 4, OUT16>(px, pal, entries, key);
	case 6 << 8 | 8: return canon<8, 6, OUT16>(px, pal, entries, key);
	case 6 << 8 | 16: return canon<16, 6, OUT16>(px, pal, entries, key);
	}
	return false;	/* (png_plan.h lets no other pair through) */
}

extern "C" __global__ void __launch_bounds__(256)
lda_pngx_convert_kernel(uint64_t n_conv, uint64_t n_tiles, uint32_t format, uint32_t le16,
			const uint64_t *__restrict__ x_tile_end, const uint64_t *__restrict__ x_sel,
			const uint64_t *__restrict__ c_src, const uint64_t *__restrict__ x_dst,
			const uint64_t *__restrict__ x_shape, const uint64_t *__restrict__ x_kind,
			const uint64_t *__restrict__ x_plte, const uint64_t *__restrict__ x_trns,
			const uint8_t *__restrict__ in, const uint8_t *__restrict__ ws,
			uint8_t *__restrict__ out_base, int32_t *__restrict__ flags)
{
	__shared__ u32 pal[256];	/* R | G << 8 | B << 16 | A << 24 */
	const u32 tid = threadIdx.x;
	const u32 ch = format & 0xF;
	const bool out16 = (format & LDA_PNGX_OUT16) != 0;
	const u32 opp = ch * (out16 ? 2 : 1);
	const u64 off48 = ((u64)1 << 48) - 1;
	u64 pal_of = ~(u64)0;	/* the selection whose palette is in LDS */

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		/* the first converted selection whose tiles end behind t: t <
		 * n_tiles = x_tile_end[n_conv - 1], so there is one */
		u64 lo = 0, hi = n_conv - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (x_tile_end[mid] > t)
				hi = mid;
			else
				lo = mid + 1;
		}
		const u64 r = lo;
		const u64 tile = t - (r ? x_tile_end[r - 1] : 0);
		const u64 kind = x_kind[r], shape = x_shape[r];
		const u32 depth = (u32)kind & 0xFF, colour = (u32)(kind >> 8) & 0xFF;
		const u32 width = (u32)shape, height = (u32)(shape >> 32);
		const u32 bits = depth * pngx_channels(colour);
		const u32 rowbytes = (u32)(((u64)width * bits + 7) >> 3);
		const u64 npix = (u64)width * height;
		const u8 *src = ws + c_src[x_sel[r]];
		u32 entries = 0;
		PngxKey key = { false, 0, 0, 0 };

		if (colour == 3) {
			const u64 plte = x_plte[r];
			entries = (u32)(plte >> 48);
			if (pal_of != r) {
				const u32 alphas = (u32)(kind >> 32);
				u32 w = 0;
				__syncthreads();	/* the tile before has read its palette */
				if (tid < entries) {
					const u8 *e = in + (plte & off48) + 3 * tid;
					const u32 a = tid < alphas ? in[(x_trns[r] & off48) + tid] : 255;
					w = e[0] | (u32)e[1] << 8 | (u32)e[2] << 16 | a << 24;
				}
				pal[tid] = w;
				__syncthreads();
				pal_of = r;
			}
		} else if (kind & LDA_PNGX_KIND_KEY) {
			const u8 *k = in + (x_trns[r] & off48);
			const u32 dm = (1u << depth) - 1;
			key.on = true;
			key.r = ((u32)k[0] << 8 | k[1]) & dm;
			if (colour == 2) {
				key.g = ((u32)k[2] << 8 | k[3]) & dm;
				key.b = ((u32)k[4] << 8 | k[5]) & dm;
			}
		}

		const u64 p0 = tile * LDA_PNGX_TILE + 16 * (u64)tid;
		if (p0 >= npix)
			continue;
		const u32 count = npix - p0 < 16 ? (u32)(npix - p0) : 16;
		const u64 src_n = (u64)height * rowbytes;
		u64 px[16];
		switch (bits) {
		case 1: fetch<1>(src, src_n, width, rowbytes, p0, count, px); break;
		case 2: fetch<2>(src, src_n, width, rowbytes, p0, count, px); break;
		case 4: fetch<4>(src, src_n, width, rowbytes, p0, count, px); break;
		case 8: fetch<8>(src, src_n, width, rowbytes, p0, count, px); break;
		case 16: fetch<16>(src, src_n, width, rowbytes, p0, count, px); break;
		case 24: fetch<24>(src, src_n, width, rowbytes, p0, count, px); break;
		case 32: fetch<32>(src, src_n, width, rowbytes, p0, count, px); break;
		case 48: fetch<48>(src, src_n, width, rowbytes, p0, count, px); break;
		default: fetch<64>(src, src_n, width, rowbytes, p0, count, px); break;
		}
		const bool bad = out16 ? canon_any<true>(depth, colour, px, pal, entries, key) :
					 canon_any<false>(depth, colour, px, pal, entries, key);
		if (bad)
			flags[x_sel[r]] = 1;
		u8 *dst = out_base + x_dst[r] + p0 * opp;
		switch (format) {
		case 1: store<1, false>(px, dst, count, false); break;
		case 2: store<2, false>(px, dst, count, false); break;
		case 3: store<3, false>(px, dst, count, false); break;
		case 4: store<4, false>(px, dst, count, false); break;
		case 1 | LDA_PNGX_OUT16: store<1, true>(px, dst, count, le16 != 0); break;
		case 2 | LDA_PNGX_OUT16: store<2, true>(px, dst, count, le16 != 0); break;
		case 3 | LDA_PNGX_OUT16: store<3, true>(px, dst, count, le16 != 0); break;
		case 4 | LDA_PNGX_OUT16: store<4, true>(px, dst, count, le16 != 0); break;
		}
	}
}

/* the verdict of every selection, the first that applies: the row's own (a
 * zero row), the gather's, the zlib decoder's, the unfilter's, the convert
 * kernel's */
extern "C" __global__ void __launch_bounds__(256)
lda_pngx_final_kernel(uint64_t n_sel, const uint64_t *__restrict__ c_meta,
		      const int32_t *__restrict__ gather, const int32_t *__restrict__ decode,
		      const int32_t *__restrict__ unfilter, const int32_t *__restrict__ convert,
		      int32_t *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n_sel)
		return;
	const s32 pre = (s32)(c_meta[r] >> 16 & 0xFFFF);
	results[r] = pre ? pre : gather[r] ? LDA_BAD_DATA : decode[r] ? decode[r] :
		     unfilter[r] || convert[r] ? LDA_BAD_DATA : LDA_SUCCESS;
}
