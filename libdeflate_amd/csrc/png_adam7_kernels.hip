/*
 * png_adam7_kernels.hip - Adam7-interlaced PNG images put together
 * (host_png_adam7.hip, include/libdeflate_amd.h): the seven pass images that
 * lda_png_unfilter_kernel left in the scratch, one unit each, woven into the
 * finished image of height rows of rowbytes bytes, and the verdicts of a call
 * whose unfilter ran over units merged per selection.
 * tools/models/png_adam7.py restates it on the CPU.
 *
 * The work is the finished images, not the passes: a tile is LDA_PNG7_TILE =
 * 1024 pieces of 16 consecutive bytes of one output row (a row's last piece is
 * shorter), four to a thread, neighbouring threads on neighbouring pieces, and
 * the workgroups stride over the tiles of all interlaced selections; a tile
 * finds its selection by a binary search in the prefix column d_tile_end, the
 * same in every lane.  Where a pixel of the finished image comes from follows
 * from its coordinates alone (PNG 8.2):
 *
 *   odd y          pass 7, row y >> 1: the whole row, so a piece is a straight
 *                  copy of 16 bytes - half of all bytes
 *   y % 4 == 2     passes 5, 6 alternating, row y >> 2 and y >> 1
 *   y % 8 == 4     passes 3, 6, 4, 6
 *   y % 8 == 0     passes 1, 6, 4, 6, 2, 6, 4, 6
 *
 * so a lane of an even row reads short runs of up to four pass rows, each of
 * them walked front to back by the lanes of the output row.  Pixels of 8 bits
 * and more move as bytes of whole pixels; depths 1, 2 and 4 are extracted bit
 * by bit, most significant first, from each pass's own packed rows, and the
 * spare low bits of an output row's last byte are written as zeros.  One code
 * path serves every pixel size: the bits per pixel are a descriptor value, the
 * same in all lanes of a tile.  The 16
 * bytes are stored as one piece where they lie inside the row, byte by byte at
 * the row's end (copy_tile()'s and the unfilter's idiom).
 *
 * It also runs over selections whose inflate or unfilter failed: the pass
 * images are then anything.  Every address and every loop bound comes from the
 * plan's descriptors (width, height, bits per pixel, rowbytes, the rooms),
 * never from a byte of an image.  Nothing spins, no wave waits for another,
 * there is no LDS.
 */
#include "device_common.h"
#include "kernels.h"

/*
 * Where the pixels of an even row y lie (PNG 8.2): the byte offsets in the
 * scratch of the up to four pass rows it draws on, by the pixel's x - odd x:
 * pass 6; x % 4 == 2: pass 4, or pass 5 where y % 4 == 2; x % 8 == 0 and x % 8
 * == 4: passes 1 and 2, or pass 3, or pass 5 - and how far x is shifted down
 * to the pixel's index in its pass row.
 */
struct P7Row {
	u64 odd, two, zero, four;
	u32 sh_two, sh_zero;	/* (odd x: 1) */
};

/* bytes of a pass row of wp pixels, ceil(wp * bits / 8) in 32 bits: at most
 * the finished image's rowbytes */
static __device__ __forceinline__ u32 p7_rb(u32 wp, u32 bits)
{
	return (wp >> 3) * bits + (((wp & 7) * bits + 7) >> 3);
}

/* pass_at: the seven pass images; width: the finished image's.  A pass is w_p
 * = ceil((width - x0) / dx) pixels wide, written out per pass. */
static __device__ __forceinline__ P7Row
p7_row(const u64 (&pass_at)[7], u32 width, u32 bits, u32 y)
{
	P7Row r;

	r.odd = pass_at[5] + (u64)(y >> 1) * p7_rb(width >> 1, bits);
	if (y & 2) {
		r.two = r.zero = r.four = pass_at[4] + (u64)(y >> 2) * p7_rb((width + 1) >> 1, bits);
		r.sh_two = r.sh_zero = 1;
	} else {
		r.two = pass_at[3] + (u64)(y >> 2) * p7_rb((width + 1) >> 2, bits);
		r.sh_two = 2;
		if (y & 4) {
			r.zero = r.four = pass_at[2] + (u64)(y >> 3) * p7_rb((width + 3) >> 2, bits);
			r.sh_zero = 2;
		} else {
			r.zero = pass_at[0] + (u64)(y >> 3) * p7_rb((width + 7) >> 3, bits);
			r.four = pass_at[1] + (u64)(y >> 3) * p7_rb((width + 3) >> 3, bits);
			r.sh_zero = 3;
		}
	}
	return r;
}

/* pixel x of the row: its pass row, and its index in it */
static __device__ __forceinline__ u64 p7_source(const P7Row &r, u32 x, u32 *xs)
{
	*xs = x >> (x & 1 ? 1 : x & 2 ? r.sh_two : r.sh_zero);
	return x & 1 ? r.odd : x & 2 ? r.two : x & 4 ? r.four : r.zero;
}

static __device__ __forceinline__ void put_byte(u64 *lo, u64 *hi, u32 i, u32 v)
{
	if (i < 8)
		*lo |= (u64)v << (8 * i);
	else
		*hi |= (u64)v << (8 * (i - 8));
}

/*
 * Piece k of row y of the finished image at dst, from the pass images in ws.
 * bits: per pixel, 1, 2, 4 or a multiple of 8 up to 64 - the same in all lanes,
 * as width and rowbytes are.
 */
static __device__ __forceinline__ void
p7_piece(const u8 *ws, const u64 (&pass_at)[7], u32 width, u32 rowbytes, u32 bits, u8 *dst, u32 y,
	 u32 k)
{
	const u32 b0 = 16 * k;
	const u32 nb = min(16u, rowbytes - b0);
	u64 lo = 0, hi = 0;

	if (y & 1) {
		/* pass 7 has the finished image's width: its row is this row */
		const u8 *src = ws + pass_at[6] + (u64)(y >> 1) * rowbytes + b0;
		if (nb == 16) {
			uint4 v;
			__builtin_memcpy(&v, src, 16);	/* (may be unaligned) */
			lo = v.x | (u64)v.y << 32;
			hi = v.z | (u64)v.w << 32;
		} else {
			for (u32 i = 0; i < nb; i++)
				put_byte(&lo, &hi, i, src[i]);
		}
	} else if (bits >= 8) {
		/* whole pixels of B bytes: byte o of pixel x, one division a piece */
		const u32 B = bits >> 3;
		const P7Row rows = p7_row(pass_at, width, bits, y);
		u32 x = b0 / B, o = b0 - x * B;
#pragma unroll
		for (u32 i = 0; i < 16; i++) {
			u32 xs;
			const u64 row = p7_source(rows, x, &xs);
			put_byte(&lo, &hi, i, ws[row + (u64)xs * B + o]);
			/* (past the row's end: its last byte again, which is not stored) */
			if (b0 + i + 1 < rowbytes && ++o == B) {
				o = 0;
				x++;
			}
		}
	} else {
		const u32 ppb = 8 / bits, mask = (1u << bits) - 1;
		const P7Row rows = p7_row(pass_at, width, bits, y);
		for (u32 i = 0; i < nb; i++) {
			u32 v = 0;
			for (u32 j = 0; j < ppb; j++) {
				const u32 x = (b0 + i) * ppb + j;	/* (at most 2^31 + 6: a width below 2^31) */
				if (x < width) {
					u32 xs;
					const u64 row = p7_source(rows, x, &xs);
					const u64 bo = (u64)xs * bits;
					const u32 byte = ws[row + (bo >> 3)];
					v |= ((byte >> (8 - bits - ((u32)bo & 7))) & mask) << (8 - bits * (j + 1));
				}
			}
			put_byte(&lo, &hi, i, v);
		}
	}
	if (bits < 8 && b0 + nb == rowbytes) {	/* the spare bits of the row's last byte */
		const u32 spare = (u32)((u64)rowbytes * 8 - (u64)width * bits);
		const u64 keep = (0xFFu << spare) & 0xFF;
		const u32 i = nb - 1;
		if (i < 8)
			lo &= ~((u64)0xFF << (8 * i)) | keep << (8 * i);
		else
			hi &= ~((u64)0xFF << (8 * (i - 8))) | keep << (8 * (i - 8));
	}
	if (nb == 16) {
		const uint4 v = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
		__builtin_memcpy(dst, &v, 16);	/* (may be unaligned) */
	} else {
		for (u32 i = 0; i < nb; i++)
			dst[i] = (u8)(i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8)));
	}
}

extern "C" __global__ void __launch_bounds__(256)
lda_png7_deinterlace_kernel(uint64_t n_il, uint64_t n_tiles, const uint64_t *__restrict__ d_tile_end,
			    const uint64_t *__restrict__ d_pass, const uint64_t *__restrict__ d_shape,
			    const uint64_t *__restrict__ d_kind, const uint64_t *__restrict__ d_dst,
			    uint8_t *ws, uint8_t *out_base)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		/* the first interlaced selection whose tiles end behind t: t <
		 * n_tiles = d_tile_end[n_il - 1], so there is one */
		u64 lo = 0, hi = n_il - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (d_tile_end[mid] > t)
				hi = mid;
			else
				lo = mid + 1;
		}
		const u64 r = lo;
		const u64 tile = t - (r ? d_tile_end[r - 1] : 0);
		const u64 kind = d_kind[r], shape = d_shape[r];
		const u32 bits = (u32)kind & 0xFF;
		const u32 rowbytes = (u32)(kind >> 16);
		const u32 width = (u32)shape, height = (u32)(shape >> 32);
		u8 *image = (kind & LDA_PNG7_KIND_ALT ? ws : out_base) + d_dst[r];
		const u32 ppr = (rowbytes + 15) >> 4;	/* pieces a row; height * ppr < 2^32 */
		const u64 pieces = (u64)height * ppr;
		u64 pass_at[7];
#pragma unroll
		for (u32 p = 0; p < 7; p++)
			pass_at[p] = d_pass[7 * r + p];
		if (bits == 0 || bits > 64 || (bits > 4 && (bits & 7)) || bits == 3)
			continue;	/* (png_plan.h lets no such row through) */

		for (u32 j = 0; j < LDA_PNG7_TILE / 256; j++) {
			const u64 piece = tile * LDA_PNG7_TILE + 256 * j + threadIdx.x;
			if (piece >= pieces)
				break;
			const u32 y = (u32)piece / ppr;
			const u32 k = (u32)piece - y * ppr;
			p7_piece(ws, pass_at, width, rowbytes, bits, image + (u64)y * rowbytes + 16 * k, y, k);
		}
	}
}

/* the verdict of every selection, the first that applies: the row's own (a
 * zero row), the gather's, the zlib decoder's, the unfilter's over the
 * selection's units (c_units: first | count << 32), the convert kernel's */
extern "C" __global__ void __launch_bounds__(256)
lda_png7_final_kernel(uint64_t n_sel, const uint64_t *__restrict__ c_meta,
		      const uint64_t *__restrict__ c_units, const int32_t *__restrict__ gather,
		      const int32_t *__restrict__ decode, const int32_t *__restrict__ unit_flags,
		      const int32_t *__restrict__ convert, int32_t *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n_sel)
		return;
	const s32 pre = (s32)(c_meta[r] >> 16 & 0xFFFF);
	const u64 units = c_units[r];
	const u32 first = (u32)units, count = (u32)(units >> 32);	/* at most seven */
	s32 unf = 0;
	for (u32 u = 0; u < count; u++)
		unf |= unit_flags[first + u];
	results[r] = pre ? pre : gather[r] ? LDA_BAD_DATA : decode[r] ? decode[r] :
		     unf || convert[r] ? LDA_BAD_DATA : LDA_SUCCESS;
}
