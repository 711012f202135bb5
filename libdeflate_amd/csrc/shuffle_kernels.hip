/*
 * shuffle_kernels.hip - the byte shuffle of HDF5, NetCDF-4 and Zarr chunks undone
 * and done in device memory (host_shuffle.hip:
 * libdeflate_amd_shuffle_decompress_batch; host_shuffle_write.hip:
 * libdeflate_amd_shuffle_compress_batch).  shuffle_plan.h states the transform
 * and builds the rows; tools/models/shuffle_model.py restates it on the CPU.
 *
 * The work is the bytes, not the chunks: a tile is a fixed number of
 * consecutive elements of one chunk - LDA_SHUF_TILE for element sizes 1, 2, 4
 * and 8, (LDA_SHUF_GEN_BYTES / es) & ~15 for any other - and the workgroups
 * stride over the tiles of all rows; a tile finds its row by a binary search in
 * the prefix column u_tile_end, the same in every lane.  The element size is a
 * value of the row, uniform in a tile: nothing branches per byte.
 *
 * Element sizes 2, 4 and 8 (and 1, a copy) stay in registers: a thread takes 16
 * elements, 16 bytes of each of the es planes - plane j starts at j * ne, so
 * these are unaligned - and 16 * es contiguous bytes on the other side, 16-byte
 * pieces throughout, the bytes transposed between them with v_perm_b32.
 * Neighbouring threads work on neighbouring pieces of every plane.  The thread
 * that meets the chunk's end moves the ne % 16 last elements and the n % es
 * bytes behind the elements byte by byte.
 *
 * Every other element size goes through LDS, which holds the tile as planes
 * (plane j at j * (T + 16)): global memory is read and written in 16-byte
 * pieces that run along a plane or along the elements, and the byte-granular
 * side of the transpose is LDS traffic (16 one-byte accesses per piece).
 *
 * lda_unshuffle_kernel also runs over chunks whose inflate failed: the scratch
 * is then anything.  Every address and loop bound comes from the plan's rows,
 * never from a byte, so it stays inside the rooms.  Nothing spins and no
 * workgroup waits for another.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"

#define SHUF_LDS_BYTES 20480	/* es * (tile + 16) at most: 256 * 80 */

/* the 4 x 4 byte matrix x[row] byte col -> y[col] byte row; its own inverse */
static __device__ __forceinline__ void
tr4(u32 x0, u32 x1, u32 x2, u32 x3, u32 &y0, u32 &y1, u32 &y2, u32 &y3)
{
	/* v_perm_b32: selector bytes 0 .. 3 take the second operand's bytes, 4 .. 7 the first's */
	const u32 t0 = __builtin_amdgcn_perm(x1, x0, 0x05010400u);	/* x0.0 x1.0 x0.1 x1.1 */
	const u32 t1 = __builtin_amdgcn_perm(x1, x0, 0x07030602u);	/* x0.2 x1.2 x0.3 x1.3 */
	const u32 t2 = __builtin_amdgcn_perm(x3, x2, 0x05010400u);
	const u32 t3 = __builtin_amdgcn_perm(x3, x2, 0x07030602u);
	y0 = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
	y1 = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
	y2 = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
	y3 = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

static __device__ __forceinline__ void load16(const u8 *p, u32 (&w)[4])
{
	uint4 v;
	__builtin_memcpy(&v, p, 16);	/* (may be unaligned) */
	w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

static __device__ __forceinline__ void store16(u8 *p, const u32 *w)
{
	const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
	__builtin_memcpy(p, &v, 16);	/* (may be unaligned) */
}

/* 16 elements as ES planes of 16 bytes pl[j] <-> as 4 * ES words of interleaved bytes o */
template <u32 ES, bool UN>
static __device__ __forceinline__ void transpose16(u32 (&pl)[ES][4], u32 (&o)[4 * ES])
{
#pragma unroll
	for (u32 q = 0; q < 4; q++) {
		if constexpr (ES == 1) {
			if constexpr (UN)
				o[q] = pl[0][q];
			else
				pl[0][q] = o[q];
		} else if constexpr (ES == 2) {
			if constexpr (UN) {
				o[2 * q] = __builtin_amdgcn_perm(pl[1][q], pl[0][q], 0x05010400u);
				o[2 * q + 1] = __builtin_amdgcn_perm(pl[1][q], pl[0][q], 0x07030602u);
			} else {
				pl[0][q] = __builtin_amdgcn_perm(o[2 * q + 1], o[2 * q], 0x06040200u);
				pl[1][q] = __builtin_amdgcn_perm(o[2 * q + 1], o[2 * q], 0x07050301u);
			}
		} else if constexpr (ES == 4) {
			if constexpr (UN)
				tr4(pl[0][q], pl[1][q], pl[2][q], pl[3][q], o[4 * q], o[4 * q + 1],
				    o[4 * q + 2], o[4 * q + 3]);
			else
				tr4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3], pl[0][q], pl[1][q],
				    pl[2][q], pl[3][q]);
		} else {
			/* an element is two words: bytes 0 .. 3 and 4 .. 7 */
			if constexpr (UN) {
				tr4(pl[0][q], pl[1][q], pl[2][q], pl[3][q], o[8 * q], o[8 * q + 2],
				    o[8 * q + 4], o[8 * q + 6]);
				tr4(pl[4][q], pl[5][q], pl[6][q], pl[7][q], o[8 * q + 1], o[8 * q + 3],
				    o[8 * q + 5], o[8 * q + 7]);
			} else {
				tr4(o[8 * q], o[8 * q + 2], o[8 * q + 4], o[8 * q + 6], pl[0][q], pl[1][q],
				    pl[2][q], pl[3][q]);
				tr4(o[8 * q + 1], o[8 * q + 3], o[8 * q + 5], o[8 * q + 7], pl[4][q],
				    pl[5][q], pl[6][q], pl[7][q]);
			}
		}
	}
}

/*
 * The thread's 16 elements from element e on of a chunk of n bytes, ne elements
 * of ES bytes.  UN: sh is the shuffled side (read), raw the other (written);
 * otherwise raw is read and sh written.
 */
template <u32 ES, bool UN>
static __device__ __forceinline__ void
reg_path(const u8 *__restrict__ rd, u8 *__restrict__ wr, u32 n, u32 ne, u64 e)
{
	if (e >= ne)
		return;
	if (e + 16 <= ne) {
		u32 pl[ES][4], o[4 * ES];
		if constexpr (UN) {
#pragma unroll
			for (u32 j = 0; j < ES; j++)
				load16(rd + (u64)j * ne + e, pl[j]);
			transpose16<ES, true>(pl, o);
#pragma unroll
			for (u32 i = 0; i < ES; i++)
				store16(wr + e * ES + 16 * i, o + 4 * i);
		} else {
#pragma unroll
			for (u32 i = 0; i < ES; i++) {
				u32 w[4];
				load16(rd + e * ES + 16 * i, w);
				o[4 * i] = w[0], o[4 * i + 1] = w[1], o[4 * i + 2] = w[2], o[4 * i + 3] = w[3];
			}
			transpose16<ES, false>(pl, o);
#pragma unroll
			for (u32 j = 0; j < ES; j++)
				store16(wr + (u64)j * ne + e, pl[j]);
		}
	} else {
		/* the chunk's last elements, fewer than 16 */
		for (u64 k = e; k < ne; k++) {
#pragma unroll
			for (u32 j = 0; j < ES; j++) {
				const u64 s = (u64)j * ne + k, r = k * ES + j;
				if constexpr (UN)
					wr[r] = rd[s];
				else
					wr[s] = rd[r];
			}
		}
	}
	if (e + 16 >= ne)	/* this thread has the last element: the bytes behind it */
		for (u64 b = (u64)ne * ES; b < n; b++)
			wr[b] = rd[b];
}

/*
 * Any element size, through LDS: the tile's c elements from element e0 on, as
 * planes in lds (plane j at j * tp, tp = the tile's elements + 16).  The
 * shuffled side moves in 16-byte pieces along the planes, the raw side in
 * 16-byte pieces along the elements.
 */
template <bool UN>
static __device__ __forceinline__ void
lds_path(u8 *lds, const u8 *__restrict__ rd, u8 *__restrict__ wr, u32 n, u32 es, u32 ne, u64 e0,
	 u32 c, u32 tp, u32 tid)
{
	const u32 pieces = (c + 15) / 16;	/* of a plane */
	const u32 total = c * es;		/* the tile's bytes */
	const u32 rpieces = (total + 15) / 16;	/* of the raw side */
	const u8 *sh_rd = rd;			/* UN: planes are read */
	u8 *sh_wr = wr;				/* !UN: planes are written */
	const u8 *raw_rd = rd + e0 * es;
	u8 *raw_wr = wr + e0 * es;

	if constexpr (UN) {
		for (u32 idx = tid; idx < es * pieces; idx += 256) {
			const u32 j = idx / pieces, p = idx - j * pieces;
			const u8 *s = sh_rd + (u64)j * ne + e0 + 16 * p;
			u32 w[4] = { 0, 0, 0, 0 };
			if (16 * p + 16 <= c) {
				load16(s, w);
			} else {
#pragma unroll
				for (u32 i = 0; i < 16; i++)
					if (16 * p + i < c)
						w[i >> 2] |= (u32)s[i] << (8 * (i & 3));
			}
			*(uint4 *)(lds + j * tp + 16 * p) = make_uint4(w[0], w[1], w[2], w[3]);
		}
	} else {
		for (u32 idx = tid; idx < rpieces; idx += 256) {
			const u32 b = 16 * idx;
			u32 k = b / es, j = b - k * es;
			u32 w[4] = { 0, 0, 0, 0 };
			if (b + 16 <= total) {
				load16(raw_rd + b, w);
			} else {
#pragma unroll
				for (u32 i = 0; i < 16; i++)
					if (b + i < total)
						w[i >> 2] |= (u32)raw_rd[b + i] << (8 * (i & 3));
			}
			/* (bytes past the tile's last land in the 16 spare bytes of a plane) */
#pragma unroll
			for (u32 i = 0; i < 16; i++) {
				lds[j * tp + k] = (u8)(w[i >> 2] >> (8 * (i & 3)));
				const bool wrap = ++j == es;
				j = wrap ? 0 : j;
				k += wrap;
			}
		}
	}
	__syncthreads();
	if constexpr (UN) {
		for (u32 idx = tid; idx < rpieces; idx += 256) {
			const u32 b = 16 * idx;
			u32 k = b / es, j = b - k * es;
			u32 w[4] = { 0, 0, 0, 0 };
			/* (past the tile's last byte this reads a plane's spare bytes) */
#pragma unroll
			for (u32 i = 0; i < 16; i++) {
				w[i >> 2] |= (u32)lds[j * tp + k] << (8 * (i & 3));
				const bool wrap = ++j == es;
				j = wrap ? 0 : j;
				k += wrap;
			}
			if (b + 16 <= total) {
				store16(raw_wr + b, w);
			} else {
#pragma unroll
				for (u32 i = 0; i < 16; i++)
					if (b + i < total)
						raw_wr[b + i] = (u8)(w[i >> 2] >> (8 * (i & 3)));
			}
		}
	} else {
		for (u32 idx = tid; idx < es * pieces; idx += 256) {
			const u32 j = idx / pieces, p = idx - j * pieces;
			u8 *d = sh_wr + (u64)j * ne + e0 + 16 * p;
			const uint4 v = *(const uint4 *)(lds + j * tp + 16 * p);
			const u32 w[4] = { v.x, v.y, v.z, v.w };
			if (16 * p + 16 <= c) {
				store16(d, w);
			} else {
#pragma unroll
				for (u32 i = 0; i < 16; i++)
					if (16 * p + i < c)
						d[i] = (u8)(w[i >> 2] >> (8 * (i & 3)));
			}
		}
	}
	if (e0 + c == ne)	/* the chunk's last tile: the bytes behind the elements */
		for (u64 b = (u64)ne * es + tid; b < n; b += 256)
			wr[b] = rd[b];
	__syncthreads();	/* the next tile fills lds again */
}

/* tile t of all rows: rd and wr are the row's two sides */
template <bool UN>
static __device__ __forceinline__ void
shuf_tile(u8 *lds, u64 n_u, u64 t, const u64 *__restrict__ u_tile_end,
	  const u64 *__restrict__ u_src, const u64 *__restrict__ u_dst,
	  const u64 *__restrict__ u_geom, const u8 *__restrict__ src0, const u8 *__restrict__ src1,
	  u8 *__restrict__ dst_base)
{
	/* the first row whose tiles end behind t: t < n_tiles = u_tile_end[n_u - 1],
	 * so there is one */
	u64 lo = 0, hi = n_u - 1;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (u_tile_end[mid] > t)
			hi = mid;
		else
			lo = mid + 1;
	}
	const u64 r = lo;
	const u64 tile = t - (r ? u_tile_end[r - 1] : 0);
	const u64 geom = u_geom[r], s = u_src[r];
	const u32 n = (u32)geom, es = (u32)(geom >> 32), ne = n / es;
	const u8 *rd = ((s & LDA_SHUF_SRC_ALT) ? src1 : src0) + (s & ~LDA_SHUF_SRC_ALT);
	u8 *wr = dst_base + u_dst[r];
	const u32 tid = threadIdx.x;
	const u64 e = tile * LDA_SHUF_TILE + 16 * (u64)tid;

	switch (es) {
	case 1: reg_path<1, UN>(rd, wr, n, ne, e); break;
	case 2: reg_path<2, UN>(rd, wr, n, ne, e); break;
	case 4: reg_path<4, UN>(rd, wr, n, ne, e); break;
	case 8: reg_path<8, UN>(rd, wr, n, ne, e); break;
	default: {
		const u32 T = (LDA_SHUF_GEN_BYTES / es) & ~15u;
		const u64 e0 = tile * T;
		const u32 c = ne - e0 < T ? (u32)(ne - e0) : T;
		lds_path<UN>(lds, rd, wr, n, es, ne, e0, c, T + 16, tid);
	}
	}
}

extern "C" __global__ void __launch_bounds__(256)
lda_unshuffle_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *__restrict__ u_tile_end,
		     const uint64_t *__restrict__ u_src, const uint64_t *__restrict__ u_dst,
		     const uint64_t *__restrict__ u_geom, const uint8_t *__restrict__ ws,
		     const uint8_t *__restrict__ alt, uint8_t *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) u8 lds[SHUF_LDS_BYTES];

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x)
		shuf_tile<true>(lds, n_u, t, u_tile_end, u_src, u_dst, u_geom, ws, alt, out);
}

/* the verdict of every row: its own (a NO_DEFLATE row: 0, or BAD_DATA where its
 * two sizes differ) or the decoder's for its stream */
extern "C" __global__ void __launch_bounds__(256)
lda_shuf_final_kernel(uint64_t n, const uint64_t *__restrict__ verd,
		      const int32_t *__restrict__ decode, int32_t *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n)
		return;
	const u64 v = verd[r];
	results[r] = (v & LDA_SHUF_VERD_OWN) ? (s32)(v & 0xFF) : decode[v];
}

/* the inverse: every chunk's raw bytes in `in` -> its shuffled bytes in its room */
extern "C" __global__ void __launch_bounds__(256)
lda_shuffle_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *__restrict__ u_tile_end,
		   const uint64_t *__restrict__ u_src, const uint64_t *__restrict__ u_dst,
		   const uint64_t *__restrict__ u_geom, const uint8_t *__restrict__ in,
		   uint8_t *__restrict__ rooms)
{
	__shared__ __attribute__((aligned(16))) u8 lds[SHUF_LDS_BYTES];

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x)
		shuf_tile<false>(lds, n_u, t, u_tile_end, u_src, u_dst, u_geom, in, in, rooms);
}

/* ---- the writer's assembly: as gzip_members_write_kernels.hip's, in three formats ---- */

#define SW_EMPTY 5	/* 01 00 00 ff ff: what the compress kernels make of 0 bytes */

static __device__ __forceinline__ u32 sw_head(int format)
{
	return format == LDA_FMT_ZLIB ? 2 : format == LDA_FMT_GZIP ? 10 : 0;
}

static __device__ __forceinline__ u32 sw_foot(int format)
{
	return format == LDA_FMT_ZLIB ? 4 : format == LDA_FMT_GZIP ? 8 : 0;
}

/*
 * Chunk k, pieces first[k] .. + count[k] of its room: csize[k] the bytes of its
 * DEFLATE stream - the pieces' sum; of a chunk of 0 bytes the empty final
 * stored block the place kernel writes -, sum[k] the CRC-32 (gzip; zw_combine())
 * or Adler-32 (zlib; as lda_pngw_image_kernel combines it) of the shuffled
 * bytes from the pieces' sums, sizes[k] header, stream and footer.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_shufw_chunk_kernel(u64 n, int format, const u64 *__restrict__ first,
		       const u64 *__restrict__ count, const u64 *__restrict__ usize,
		       const u64 *__restrict__ pc_off, const u64 *__restrict__ pc_n,
		       const u64 *__restrict__ out_n, const u32 *__restrict__ sums,
		       u64 *__restrict__ csize, u32 *__restrict__ sum, u64 *__restrict__ sizes)
{
	const u32 lane = threadIdx.x & 63;
	const u32 M = 65521;

	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 f = first[k], np = count[k], us = usize[k];
		u64 csum = 0;
		u32 chk = 0;

		if (format == LDA_FMT_GZIP) {
			bool missing;
			chk = zw_combine(lane, f, np, us, pc_off, pc_n, out_n, sums, &csum, &missing);
		} else {
			const u64 run = (np + 63) / 64;
			const u64 a = lane * run < np ? lane * run : np;
			const u64 b = a + run < np ? a + run : np;
			u64 sa = 0, sb = 0;
			for (u64 i = a; i < b; i++) {
				csum += out_n[f + i];
				if (format == LDA_FMT_ZLIB) {
					const u32 ad = sums[f + i];
					const u32 ai = ((ad & 0xFFFF) + M - 1) % M, bi = (ad >> 16) % M;
					const u64 t = us - (pc_off[f + i] + pc_n[f + i] - pc_off[f]);
					sa = (sa + ai) % M;
					sb = (sb + bi + (t % M) * ai) % M;
				}
			}
			csum = wave_sum64(csum);
			sa = wave_sum64(sa);
			sb = wave_sum64(sb);
			chk = (u32)(sb % M) << 16 | (u32)((1 + sa) % M);
		}
		if (lane == 0) {
			const u64 cs = np ? csum : SW_EMPTY;
			csize[k] = cs;
			sum[k] = chk;
			sizes[k] = sw_head(format) + cs + sw_foot(format);
		}
	}
}

/*
 * offsets / block_sums: the scan kernels' output over sizes[], so stream k
 * stands at offsets[k] + block_sums[k / LDA_SCAN_BLOCK] and all streams take
 * the grand total.  Writes stream k's header (zlib: lib/zlib_compress.c; gzip:
 * lib/gzip_compress.c, MTIME 0, XFL by level, OS 0xff) and footer, an empty
 * chunk's stream, piece j's copy (cp_src with ZW_FROM_SLOT into the slots) and,
 * index not NULL, the reader's row of the chunk.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_shufw_place_kernel(u64 n, int format, int level, u64 out_avail, const u64 *__restrict__ ecols,
		       const u64 *__restrict__ pc_off, const u64 *__restrict__ pc_n,
		       const u64 *__restrict__ slot_off, const u64 *__restrict__ out_n,
		       const u64 *__restrict__ csize, const u32 *__restrict__ sum,
		       const u64 *__restrict__ offsets, const u64 *__restrict__ block_sums,
		       u8 *__restrict__ out, u64 *__restrict__ cp_src, u64 *__restrict__ cp_dst,
		       u64 *__restrict__ cp_len, u64 *__restrict__ index)
{
	/* shuffle_plan.h: SHUFW_E_FIRST, _COUNT, _USIZE, _ES, _MASK, _RAW_OFF */
	const u64 *first = ecols, *count = ecols + n, *usize = ecols + 2 * n, *es = ecols + 3 * n,
		  *mask = ecols + 4 * n, *raw_off = ecols + 5 * n;
	const u32 lane = threadIdx.x & 63;
	const u64 total = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (total > out_avail)
		return;
	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 np = count[k], cs = csize[k];
		const u64 at = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
		u8 *mem = out + at;
		u8 *stream = mem + sw_head(format);

		if (lane == 0 && format == LDA_FMT_GZIP) {
			zw_put<4>(mem, 0x00088B1Fu);
			zw_put<4>(mem + 4, 0);
			zw_put<2>(mem + 8, lda_gzip_xfl(level) | 0xFF00u);
		} else if (lane == 0 && format == LDA_FMT_ZLIB) {
			const u32 hw = lda_zlib_header(level);
			mem[0] = (u8)(hw >> 8);
			mem[1] = (u8)hw;
		} else if (lane == 1 && format == LDA_FMT_GZIP) {
			zw_put<4>(stream + cs, sum[k]);
			zw_put<4>(stream + cs + 4, usize[k]);
		} else if (lane == 1 && format == LDA_FMT_ZLIB) {
			zw_put<4>(stream + cs, __builtin_bswap32(sum[k]));
		} else if (lane == 2 && !np) {
			/* BFINAL 1, BTYPE 00, LEN 0, NLEN ~0 */
			zw_put<1>(stream, 1);
			zw_put<4>(stream + 1, 0xFFFF0000u);
		} else if (lane == 3 && index) {
			u64 *row = index + 6 * k;
			row[0] = at;
			row[1] = sw_head(format) + cs + sw_foot(format);
			row[2] = raw_off[k];
			row[3] = usize[k];
			row[4] = es[k];
			row[5] = mask[k];
		}
		zw_place_pieces(lane, first[k], np, (u64)(stream - out), true, pc_off, pc_n, slot_off,
				out_n, cp_src, cp_dst, cp_len);
	}
}

/* result[0] = 0 or LIBDEFLATE_INSUFFICIENT_SPACE, [1] the streams' bytes, [2] the
 * chunks' raw bytes, [3] the chunks */
extern "C" __global__ void __launch_bounds__(64)
lda_shufw_final_kernel(u64 n, u64 raw_total, u64 out_avail, const u64 *__restrict__ total_at,
		       u64 *__restrict__ result)
{
	if (threadIdx.x != 0)
		return;
	const u64 total = *total_at;
	result[0] = total <= out_avail ? LDA_SUCCESS : LDA_INSUFFICIENT_SPACE;
	result[1] = total;
	result[2] = raw_total;
	result[3] = n;
}
