/*
 * png_kernels.hip - PNG files read from device memory (host_png.hip,
 * include/libdeflate_amd.h): the chunk walk of every file, the gather of the
 * IDAT payloads into the zlib stream PNG splits across chunks, and the undoing
 * of the five scanline filters behind the zlib batch decode (inflate_kernel.hip,
 * unchanged).  tools/models/png_model.py restates all of it on the CPU.
 *
 * The unfilter is the hot path.  A reconstructed byte depends on its left
 * neighbour (a), the byte above (b) and the one above left (c), so a row is
 * serial along its length and the rows are serial downwards; what is free is
 * the diagonal.  One wave takes one image - the batch is the parallelism, as
 * for the inflate in front of it - and inside the image 64 rows at a time: lane
 * L owns row 64 band + L and runs L filter units behind lane L - 1, so at step
 * t it reconstructs unit t - L with a = its own result of the step before (a
 * register), b = lane L - 1's result of the step before (one cross-lane move, two
 * where the unit is wider than four bytes) and c = the b of the step before.
 * Lane 0's upper row is the last row of the band before, which this wave stored
 * to d_out: it is read back only behind stores_visible(), the waited form of
 * store visibility (ADVICE.md finding 1, global_stores_visible() of
 * inflate_kernel.hip).  Every loop bound is a descriptor value of the host
 * (height, rowbytes), never a byte of the image; nothing spins and no wave
 * waits for another.
 */
#include "device_common.h"
#include "kernels.h"
#include "tar_copy.h"

#define PNG_SIG_LO 0x474E5089u	/* 89 50 4E 47 */
#define PNG_SIG_HI 0x0A1A0A0Du	/* 0D 0A 1A 0A */
#define PNG_IHDR 0x49484452u
#define PNG_PLTE 0x504C5445u
#define PNG_IDAT 0x49444154u
#define PNG_IEND 0x49454E44u
#define PNG_TRNS 0x74524E53u

static __device__ __forceinline__ u32 be32(const u8 *p)
{
	return (u32)p[0] << 24 | (u32)p[1] << 16 | (u32)p[2] << 8 | p[3];
}

/* a chunk's length and type, one 8-byte load (the address may be unaligned) */
static __device__ __forceinline__ void chunk_head(const u8 *p, u32 *len, u32 *type)
{
	u64 v;
	__builtin_memcpy(&v, p, 8);
	*len = __builtin_bswap32((u32)v);
	*type = __builtin_bswap32((u32)(v >> 32));
}

static __device__ __forceinline__ u32 png_channels(u32 colour)
{
	return colour == 0 || colour == 3 ? 1 : colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 0;
}

static __device__ __forceinline__ bool png_depth_ok(u32 depth, u32 colour)
{
	const bool low = depth == 1 || depth == 2 || depth == 4;
	if (colour == 0)
		return low || depth == 8 || depth == 16;
	if (colour == 3)
		return low || depth == 8;
	if (colour == 2 || colour == 4 || colour == 6)
		return depth == 8 || depth == 16;
	return false;
}

/* the bytes an Adam7 stream of this image inflates to: the seven passes'
 * rows with their filter bytes (png_adam7_plan.h).  A pass is no larger than
 * the image, whose height * (1 + rowbytes) the caller has found below 2^32 */
static __device__ __forceinline__ u64 png_raw7(u32 width, u32 height, u32 bits)
{
	/* x0, y0 and the binary logarithms of dx, dy of the passes (PNG 8.2) */
	constexpr u32 X0[7] = { 0, 4, 0, 2, 0, 1, 0 }, Y0[7] = { 0, 0, 4, 0, 2, 0, 1 };
	constexpr u32 LX[7] = { 3, 3, 2, 2, 1, 1, 0 }, LY[7] = { 3, 3, 3, 2, 2, 1, 1 };
	u64 sum = 0;
#pragma unroll
	for (u32 p = 0; p < 7; p++) {
		const u64 w = width > X0[p] ? ((u64)width - X0[p] + (1u << LX[p]) - 1) >> LX[p] : 0;
		const u64 h = height > Y0[p] ? ((u64)height - Y0[p] + (1u << LY[p]) - 1) >> LY[p] : 0;
		if (w && h)
			sum += h * (1 + ((w * bits + 7) >> 3));
	}
	return sum;
}

/*
 * One lane per file: the serial walk over the chunks.  Every step advances 12
 * bytes at least and stays inside the file's length, so the loop ends on any
 * input.  flags: 0, or LDA_PNG_ADAM7 - an interlaced file is then indexed like
 * any other, its row's interlace byte 1 (libdeflate_amd_png_index_batch_ex).
 */
extern "C" __global__ void __launch_bounds__(256)
lda_png_index_kernel(uint64_t n_files, uint32_t flags, const uint8_t *__restrict__ in,
		     const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ in_n,
		     uint64_t *__restrict__ rows, int32_t *__restrict__ results)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_files)
		return;
	const u64 off = in_off[k], n = in_n[k];
	u64 *row = rows + LDA_PNG_WORDS * k;
	const u8 *f = in + off;

	row[0] = off;
	row[1] = n;
#pragma unroll
	for (u32 w = 2; w < LDA_PNG_WORDS; w++)
		row[w] = 0;
	results[k] = LDA_BAD_DATA;
	if (n < 33 + 12)	/* the signature, IHDR and one more chunk */
		return;
	if (be32(f) != __builtin_bswap32(PNG_SIG_LO) || be32(f + 4) != __builtin_bswap32(PNG_SIG_HI))
		return;
	u32 len, type;
	chunk_head(f + 8, &len, &type);
	if (len != 13 || type != PNG_IHDR)
		return;
	u32 crc = 0xFFFFFFFFu;	/* over the type and the data: 17 bytes */
	for (u32 i = 0; i < 17; i++) {
		crc ^= f[12 + i];
#pragma unroll
		for (u32 b = 0; b < 8; b++)
			crc = (crc >> 1) ^ (0xEDB88320u & (0 - (crc & 1)));
	}
	if (~crc != be32(f + 29))
		return;
	const u32 width = be32(f + 16), height = be32(f + 20);
	const u32 depth = f[24], colour = f[25], interlace = f[28];
	if (!width || !height || width > 0x7FFFFFFFu || height > 0x7FFFFFFFu)
		return;
	if (!png_depth_ok(depth, colour) || f[26] != 0 || f[27] != 0 || interlace > 1)
		return;
	const u32 channels = png_channels(colour);
	const u32 bits = channels * depth;
	const u32 bpp = bits < 8 ? 1 : bits / 8;
	const u64 rowbytes = ((u64)width * bits + 7) / 8;

	u64 pos = 33, first = 0, sum = 0, plte = 0, trns = 0;
	u32 state = 0;	/* 0: in front of the IDAT run, 1: in it, 2: behind it */
	bool unknown = false;
	for (;;) {
		if (n - pos < 12)
			return;	/* no IEND */
		chunk_head(f + pos, &len, &type);
		if (len > n - pos - 12)
			return;
		if (type == PNG_IEND)
			break;
		if (type == PNG_IDAT) {
			if (state == 2)
				return;
			if (state == 0)
				first = off + pos;
			state = 1;
			sum += len;
		} else {
			if (state == 1)
				state = 2;
			if (type == PNG_IHDR) {
				return;
			} else if (type == PNG_PLTE) {
				if (len % 3 != 0 || len > 768 || plte)
					return;
				if (state == 0)
					plte = (off + pos + 8) | (u64)(len / 3) << 48;
			} else if (type == PNG_TRNS) {
				if (state == 0 && !trns && len <= 0xFFFF)
					trns = (off + pos + 8) | (u64)len << 48;
			} else if (!(type >> 24 & 0x20)) {
				unknown = true;	/* a critical chunk this reader does not know */
			}
		}
		pos += 12 + (u64)len;
	}
	if (state == 0 || (colour == 3 && !plte))
		return;
	bool large = rowbytes + 1 > 0xFFFFFFFFull / height;
	if (interlace && (flags & LDA_PNG_ADAM7) && !large)
		large = png_raw7(width, height, bits) > 0xFFFFFFFFull;
	if ((interlace && !(flags & LDA_PNG_ADAM7)) || unknown || large) {
		results[k] = LDA_PNG_UNSUPPORTED;
		return;
	}
	row[2] = width | (u64)height << 32;
	row[3] = depth | colour << 8 | interlace << 16 | bpp << 24 | (u64)channels << 32;
	row[4] = first;
	row[5] = sum;
	row[6] = plte;
	row[7] = trns;
	results[k] = LDA_SUCCESS;
}

/*
 * One workgroup per selection: the IDAT run walked again from the row's first
 * IDAT, every payload copied behind the last into the selection's room of zsum
 * bytes.  Thread 0 reads the chunk's head and hands it on through LDS.  The
 * walk ends where the run ends; flag 1 (BAD_DATA) where the run and the row's
 * sum disagree - a chunk that would pass the room's end is not copied - or a
 * chunk does not lie inside the file.  Reads stay inside [., end), writes
 * inside the room, whatever the bytes say.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_png_gather_kernel(uint64_t n_sel, const uint64_t *__restrict__ c_idat,
		      const uint64_t *__restrict__ c_end, const uint64_t *__restrict__ c_zsum,
		      const uint64_t *__restrict__ c_zoff, const uint8_t *__restrict__ in,
		      uint8_t *__restrict__ ws, int32_t *__restrict__ flags)
{
	__shared__ u32 head[2];
	const u32 tid = threadIdx.x;

	for (u64 r = blockIdx.x; r < n_sel; r += gridDim.x) {
		const u64 end = c_end[r], want = c_zsum[r];
		u64 pos = c_idat[r], got = 0;
		u8 *room = ws + c_zoff[r];
		bool bad = false;
		if (end == 0) {	/* a zero row */
			if (tid == 0)
				flags[r] = 0;
			continue;
		}
		for (;;) {	/* (pos + 12 <= end holds for the first chunk: png_plan.h) */
			if (end - pos < 12)
				break;
			if (tid == 0)
				chunk_head(in + pos, &head[0], &head[1]);
			__syncthreads();
			const u32 len = head[0], type = head[1];
			__syncthreads();
			if (type != PNG_IDAT)
				break;
			if (len > end - pos - 12 || len > want - got) {
				bad = true;
				break;
			}
			copy_tile(in + pos + 8, room + got, len, tid);
			got += len;
			pos += 12 + (u64)len;
		}
		if (tid == 0)
			flags[r] = bad || got != want;
	}
}

/* stores of this wave visible to loads of its other lanes: the waited form,
 * as global_stores_visible() of inflate_kernel.hip */
static __device__ __forceinline__ void stores_visible(void)
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* 16 bytes at p + off as two words, bytes at or past n read as 0 */
static __device__ __forceinline__ void
load_piece(const u8 *__restrict__ p, u64 off, u64 n, u64 *lo, u64 *hi)
{
	const uint4 v = load16_guard(p, off, n);
	*lo = v.x | (u64)v.y << 32;
	*hi = v.z | (u64)v.w << 32;
}

/* the two bytes of both halves of a word exchanged */
static __device__ __forceinline__ u32 swap16(u32 v)
{
	return (v & 0x00FF00FFu) << 8 | (v >> 8 & 0x00FF00FFu);
}

static __device__ __forceinline__ u32 paeth(u32 a, u32 b, u32 c)
{
	const s32 p = (s32)(a + b) - (s32)c;
	const u32 pa = (u32)__builtin_abs(p - (s32)a), pb = (u32)__builtin_abs(p - (s32)b),
		  pc = (u32)__builtin_abs(p - (s32)c);
	/* ties in the order a, b, c */
	return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

/*
 * The bands of one image by one wave; B: the filter unit, K = 16 / B units per
 * 16-byte piece.  A lane loads a piece of its row at a unit boundary and
 * shifts the units out of it, and collects its results in a piece that it
 * stores when it is full or the row ends.  A full piece is stored as 16 bytes
 * where they lie inside the row (its 16 - K B last bytes are zeros the same
 * lane's next piece overwrites), byte by byte at the row's end.  Returns
 * whether a filter byte above 4 was met (such a row counts as type 0).
 */
template <u32 B>
static __device__ __forceinline__ bool
unfilter_image(const u8 *__restrict__ raw, u8 *__restrict__ out, u32 height, u32 rowbytes)
{
	constexpr u32 K = 16 / B;
	constexpr u64 UMASK = B == 8 ? ~(u64)0 : ((u64)1 << (8 * (B & 7))) - 1;
	const u32 lane = lane_id();
	const u32 units = rowbytes / B;
	const u64 raw_n = (u64)height * ((u64)rowbytes + 1), out_n = (u64)height * rowbytes;
	bool bad = false;

	for (u32 row0 = 0; row0 < height; row0 += 64) {
		const u32 row = row0 + lane;
		const bool mine = row < height;
		const u32 nl = min(64u, height - row0);	/* lanes of this band */
		const u64 rin = (u64)row * ((u64)rowbytes + 1) + 1;
		const u64 rout = (u64)row * rowbytes;
		u32 ft = 0;
		if (mine) {
			ft = raw[rin - 1];
			if (ft > 4) {
				bad = true;
				ft = 0;
			}
		}
		const bool upper = lane == 0 && row0 > 0;	/* b comes from d_out */
		if (row0 > 0)
			stores_visible();
		u64 ilo = 0, ihi = 0, plo = 0, phi = 0, olo = 0, ohi = 0;
		u32 icnt = 0, ocnt = 0;
		u64 res = 0, cprev = 0;
		const u32 steps = units + nl - 1;
		for (u32 t = 0; t < steps; t++) {
			u64 up = (u32)__shfl_up((u32)res, 1, 64);
			if (B > 4)
				up |= (u64)(u32)__shfl_up((u32)(res >> 32), 1, 64) << 32;
			const u32 x = t - lane;
			if (!mine || t < lane || x >= units)
				continue;
			if (icnt == 0) {
				load_piece(raw, rin + (u64)x * B, raw_n, &ilo, &ihi);
				if (upper)
					load_piece(out, rout - rowbytes + (u64)x * B, out_n, &plo, &phi);
				icnt = K;
			}
			const u64 cur = ilo & UMASK;
			if (lane == 0)
				up = plo & UMASK;	/* zeros in band 0 */
			if constexpr (B == 8) {
				ilo = ihi;
				plo = phi;
			} else {
				ilo = ilo >> (8 * B) | ihi << (64 - 8 * B);
				ihi >>= 8 * B;
				plo = plo >> (8 * B) | phi << (64 - 8 * B);
				phi >>= 8 * B;
			}
			icnt--;
			u64 r = 0;
#pragma unroll
			for (u32 i = 0; i < B; i++) {
				const u32 v = (u32)(cur >> (8 * i)) & 0xFF;
				const u32 a = (u32)(res >> (8 * i)) & 0xFF;
				const u32 b = (u32)(up >> (8 * i)) & 0xFF;
				const u32 c = (u32)(cprev >> (8 * i)) & 0xFF;
				const u32 pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b :
						 ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
				r |= (u64)((v + pred) & 0xFF) << (8 * i);
			}
			res = r;
			cprev = up;
			const u32 sh = 8 * B * ocnt;
			if (sh < 64) {
				olo |= r << sh;
				if (sh + 8 * B > 64)
					ohi |= r >> (64 - sh);
			} else {
				ohi |= r << (sh - 64);
			}
			ocnt++;
			if (ocnt == K || x + 1 == units) {
				const u32 nb = ocnt * B;
				const u32 p0 = (x + 1) * B - nb;
				u8 *dst = out + rout + p0;
				if (p0 + 16 <= rowbytes) {
					const uint4 v = make_uint4((u32)olo, (u32)(olo >> 32), (u32)ohi,
								   (u32)(ohi >> 32));
					__builtin_memcpy(dst, &v, 16);
				} else {
					for (u32 i = 0; i < nb; i++)
						dst[i] = (u8)((i < 8 ? olo >> (8 * i) : ohi >> (8 * (i - 8))));
				}
				olo = ohi = 0;
				ocnt = 0;
			}
		}
	}
	return __ballot(bad) != 0;
}

/*
 * One wave per selection (four to a workgroup).  flags[r] = 1: a filter byte
 * above 4.  meta bit 8 (LDA_PNG_META_LE16): the 16-bit samples are swapped in
 * place in a last pass over the selection, behind stores_visible() - the
 * filters run on the bytes in PNG order, and so does the read of the upper row
 * at a band's start.  meta bit 9 (LDA_PNG_META_ALT): c_out_off counts from
 * alt_base, not from out_base (host_png_pixels.hip: the scratch).
 */
extern "C" __global__ void __launch_bounds__(256)
lda_png_unfilter_kernel(uint64_t n_sel, const uint64_t *__restrict__ c_raw_off,
			const uint64_t *__restrict__ c_raw_n, const uint64_t *__restrict__ c_out_off,
			const uint64_t *__restrict__ c_geom, const uint64_t *__restrict__ c_meta,
			const uint8_t *__restrict__ ws, uint8_t *__restrict__ out_base,
			uint8_t *__restrict__ alt_base, int32_t *__restrict__ flags)
{
	const u32 lane = lane_id();
	const u64 waves = (u64)gridDim.x * 4;

	for (u64 r = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_sel; r += waves) {
		const u64 geom = c_geom[r], meta = c_meta[r];
		const u32 height = (u32)geom, rowbytes = (u32)(geom >> 32);
		const u32 bpp = (u32)meta & 0xFF;
		const u8 *raw = ws + c_raw_off[r];
		u8 *out = (meta & LDA_PNG_META_ALT ? alt_base : out_base) + c_out_off[r];
		bool bad = false;

		if (c_raw_n[r] == 0) {	/* a zero row */
			if (lane == 0)
				flags[r] = 0;
			continue;
		}
		switch (bpp) {
		case 1: bad = unfilter_image<1>(raw, out, height, rowbytes); break;
		case 2: bad = unfilter_image<2>(raw, out, height, rowbytes); break;
		case 3: bad = unfilter_image<3>(raw, out, height, rowbytes); break;
		case 4: bad = unfilter_image<4>(raw, out, height, rowbytes); break;
		case 6: bad = unfilter_image<6>(raw, out, height, rowbytes); break;
		case 8: bad = unfilter_image<8>(raw, out, height, rowbytes); break;
		default: bad = true; break;	/* (png_plan.h lets no other through) */
		}
		if (meta & LDA_PNG_META_LE16) {
			const u64 n = (u64)height * rowbytes;	/* even: 16-bit samples */
			stores_visible();
			for (u64 at = 16 * (u64)lane; at < n; at += 16 * 64) {
				if (at + 16 <= n) {
					uint4 v;
					__builtin_memcpy(&v, out + at, 16);
					v.x = swap16(v.x);
					v.y = swap16(v.y);
					v.z = swap16(v.z);
					v.w = swap16(v.w);
					__builtin_memcpy(out + at, &v, 16);
				} else {
					for (u64 i = at; i + 1 < n; i += 2) {
						const u8 hi = out[i], lo = out[i + 1];
						out[i] = lo;
						out[i + 1] = hi;
					}
				}
			}
		}
		if (lane == 0)
			flags[r] = bad;
	}
}

/* the verdict of every selection, the first that applies: the row's own
 * (a zero row), the gather's, the zlib decoder's, the unfilter's */
extern "C" __global__ void __launch_bounds__(256)
lda_png_final_kernel(uint64_t n_sel, const uint64_t *__restrict__ c_meta,
		     const int32_t *__restrict__ gather, const int32_t *__restrict__ decode,
		     const int32_t *__restrict__ unfilter, int32_t *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n_sel)
		return;
	const s32 pre = (s32)(c_meta[r] >> 16 & 0xFFFF);
	results[r] = pre ? pre : gather[r] ? LDA_BAD_DATA : decode[r] ? decode[r] :
		     unfilter[r] ? LDA_BAD_DATA : LDA_SUCCESS;
}
