/*
 * tiff_kernels.hip - the predictors of TIFF's deflate strips and tiles undone
 * and applied in device memory (host_tiff.hip: libdeflate_amd_tiff_decode_batch;
 * host_tiff_write.hip: libdeflate_amd_tiff_encode_batch).  tiff_plan.h states
 * the transforms and builds the rows; tools/models/tiff_model.py restates them
 * on the CPU.
 *
 * lda_tiff_unpredict_kernel runs the plan's *scans*: `rows` rows of rb bytes,
 * samples of sb bytes, every sample the sum - modulo 2^(8 sb) - of the stored
 * samples at its place and at every multiple of st bytes in front of it in its
 * row; st 0 is a copy.  A row is walked by a group of G = 4, 16 or 64 lanes in
 * passes; a group carries one running pixel (st bytes) from pass to pass.  In a
 * pass a lane owns whole pixels in registers - 64 bytes where st is 1, 2, 4, 8
 * or 16, 48 bytes where it is 3, 6, 12, 24 or 48 -, unpacks them into samples,
 * scans them serially, and the lanes' last pixels, packed into dwords again,
 * are scanned across the group with wave shuffles: the adds are per sample
 * (add_packed), no carry crosses from one sample into the next.  Any other
 * stride takes the generic path, channel by channel, a lane one sample, the
 * same sums.  The work is counted in quads of 4 lanes and the plan orders the
 * scans by G, so a group never straddles a wave and lanes that take different
 * paths are never in one group: every shuffle reads lanes of its own group,
 * which run the same code.  Rows are read and written in 16-byte pieces that
 * need not be aligned; the tail of a row is read as a whole piece too - every
 * scan reads the scratch, which has room to spare behind its last room - and
 * written byte by byte.  A scan may run in
 * place: a lane stores the bytes it loaded itself, in the same pass.
 *
 * The floating-point predictor is such a scan over the byte planes of the
 * whole coded row, in place in the scratch (sb 1, st spp), and then
 * lda_tiff_gather_kernel, a launch of its own, collects the kept pixels from
 * the planes, the most significant byte's plane first.
 *
 * lda_tiff_predict_kernel is the forward direction, without a scan: every
 * thread makes 16 bytes of a segment's room from the raw pixels - the kept
 * rectangle, zero samples to its right and below it - and stores them as one
 * aligned piece.
 *
 * The unpredict and gather kernels also run over segments whose inflate
 * failed: the scratch is then anything.  Every address and loop bound comes
 * from the plan's rows, never from a byte, so they stay inside the rooms and
 * the kept rectangles.  Nothing spins and no workgroup waits for another.
 * Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"

template <u32 SB> struct tiff_sample { typedef u32 T; };
template <> struct tiff_sample<8> { typedef u64 T; };

static __device__ __forceinline__ void tf_load16(const u8 *p, u32 *w)
{
	uint4 v;
	__builtin_memcpy(&v, p, 16);	/* (may be unaligned) */
	w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

static __device__ __forceinline__ void tf_store16(u8 *p, const u32 *w)
{
	const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
	__builtin_memcpy(p, &v, 16);	/* (may be unaligned) */
}

/* M samples of SB bytes out of / into (M * SB + 3) / 4 dwords */
template <u32 SB, u32 M>
static __device__ __forceinline__ void
tf_unpack(const u32 *w, typename tiff_sample<SB>::T *s)
{
#pragma unroll
	for (u32 i = 0; i < M; i++) {
		if constexpr (SB == 1)
			s[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
		else if constexpr (SB == 2)
			s[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
		else if constexpr (SB == 4)
			s[i] = w[i];
		else
			s[i] = (u64)w[2 * i] | (u64)w[2 * i + 1] << 32;
	}
}

template <u32 SB, u32 M>
static __device__ __forceinline__ void
tf_pack(const typename tiff_sample<SB>::T *s, u32 *w)
{
#pragma unroll
	for (u32 k = 0; k < (M * SB + 3) / 4; k++)
		w[k] = 0;
#pragma unroll
	for (u32 i = 0; i < M; i++) {
		if constexpr (SB == 1)
			w[i >> 2] |= (s[i] & 0xFFu) << (8 * (i & 3));
		else if constexpr (SB == 2)
			w[i >> 1] |= (s[i] & 0xFFFFu) << (16 * (i & 1));
		else if constexpr (SB == 4)
			w[i] = s[i];
		else
			w[2 * i] = (u32)s[i], w[2 * i + 1] = (u32)(s[i] >> 32);
	}
}

/* a += b per sample of SB bytes over W dwords: no carry leaves a sample */
template <u32 SB, u32 W>
static __device__ __forceinline__ void add_packed(u32 *a, const u32 *b)
{
	if constexpr (SB == 8) {
#pragma unroll
		for (u32 k = 0; k + 1 < W; k += 2) {
			const u64 x = ((u64)a[k] | (u64)a[k + 1] << 32) + ((u64)b[k] | (u64)b[k + 1] << 32);
			a[k] = (u32)x, a[k + 1] = (u32)(x >> 32);
		}
	} else {
#pragma unroll
		for (u32 k = 0; k < W; k++) {
			if constexpr (SB == 4) {
				a[k] += b[k];
			} else {
				/* the top bit of every sample apart, so that nothing carries out of it */
				const u32 H = SB == 1 ? 0x80808080u : 0x80008000u;
				a[k] = ((a[k] & ~H) + (b[k] & ~H)) ^ ((a[k] ^ b[k]) & H);
			}
		}
	}
}

/*
 * One row through the registers: samples of SB bytes, stride ST bytes, a lane
 * NB bytes a pass.  l is the lane of its group of G; rd and wr are the row's
 * first bytes (they may be the same).
 */
template <u32 SB, u32 ST>
static __device__ __forceinline__ void
scan_reg(const u8 *rd, u8 *wr, u32 rb, u32 G, u32 l)
{
	typedef typename tiff_sample<SB>::T T;
	constexpr u32 NB = (ST % 3 == 0) ? 48 : 64;	/* the lane's bytes */
	constexpr u32 NW = NB / 4, N = NB / SB, SPP = ST / SB, TW = (ST + 3) / 4;
	u32 carry[TW];

#pragma unroll
	for (u32 k = 0; k < TW; k++)
		carry[k] = 0;
	for (u64 base = 0; base < rb; base += (u64)G * NB) {
		const u64 off = base + (u64)l * NB;
		const u32 have = off >= rb ? 0 : rb - off >= NB ? NB : (u32)(rb - off);
		u32 w[NW], tw[TW], ex[TW];
		T s[N], ps[SPP];

#pragma unroll
		for (u32 k = 0; k < NW; k++)
			w[k] = 0;
		if (have) {
			/* (the lane at a row's end reads past it - the scratch has NB bytes to
			 * spare behind its last room - and drops what it read there) */
#pragma unroll
			for (u32 k = 0; k < NW; k += 4)
				tf_load16(rd + off + 4 * k, w + k);
#pragma unroll
			for (u32 k = 0; k < NW; k++) {
				const u32 left = have > 4 * k ? have - 4 * k : 0;
				w[k] &= left >= 4 ? ~0u : (1u << (8 * left)) - 1;
			}
		}
		tf_unpack<SB, N>(w, s);
		/* the lane's own pixels */
#pragma unroll
		for (u32 i = SPP; i < N; i++)
			s[i] += s[i - SPP];
		/* its last pixel: the sum of all of them.  Inclusive over the group */
		tf_pack<SB, SPP>(s + (N - SPP), tw);
		for (u32 d = 1; d < G; d <<= 1) {
			u32 o[TW];
#pragma unroll
			for (u32 k = 0; k < TW; k++) {
				o[k] = __shfl_up(tw[k], d, G);
				o[k] = l >= d ? o[k] : 0;
			}
			add_packed<SB, TW>(tw, o);
		}
		/* what stands in front of the lane: the lanes before it and the passes before this */
#pragma unroll
		for (u32 k = 0; k < TW; k++) {
			ex[k] = __shfl_up(tw[k], 1, G);
			ex[k] = l ? ex[k] : 0;
			tw[k] = __shfl(tw[k], G - 1, G);
		}
		add_packed<SB, TW>(ex, carry);
		add_packed<SB, TW>(carry, tw);
		tf_unpack<SB, SPP>(ex, ps);
#pragma unroll
		for (u32 i = 0; i < N; i++)
			s[i] += ps[i % SPP];
		tf_pack<SB, N>(s, w);
		if (have == NB) {
#pragma unroll
			for (u32 k = 0; k < NW; k += 4)
				tf_store16(wr + off + 4 * k, w + k);
		} else {
#pragma unroll
			for (u32 i = 0; i < NB; i++)
				if (i < have)
					wr[off + i] = (u8)(w[i >> 2] >> (8 * (i & 3)));
		}
	}
}

/* stride 0: the row's bytes as they are */
static __device__ __forceinline__ void
scan_copy(const u8 *rd, u8 *wr, u32 rb, u32 G, u32 l)
{
	for (u64 off = (u64)l * 16; off < rb; off += (u64)G * 16) {
		if (rb - off >= 16) {
			u32 w[4];
			tf_load16(rd + off, w);
			tf_store16(wr + off, w);
		} else {
			for (u64 i = off; i < rb; i++)
				wr[i] = rd[i];
		}
	}
}

/* any other stride: channel by channel, a lane one sample of a pass's G pixels */
template <u32 SB>
static __device__ __forceinline__ void
scan_generic(const u8 *rd, u8 *wr, u32 rb, u32 st, u32 G, u32 l)
{
	typedef typename tiff_sample<SB>::T T;

	for (u32 c = 0; c < st; c += SB) {
		T carry = 0;
		for (u64 base = 0; base < rb; base += (u64)G * st) {
			const u64 off = base + (u64)l * st + c;
			const bool have = off < rb;	/* (rb is whole pixels) */
			T s = 0;

			if (have)
				__builtin_memcpy(&s, rd + off, SB);
			for (u32 d = 1; d < G; d <<= 1) {
				T o;
				if constexpr (SB == 8)
					o = (u64)__shfl_up((u32)s, d, G) | (u64)__shfl_up((u32)(s >> 32), d, G) << 32;
				else
					o = __shfl_up(s, d, G);
				s += l >= d ? o : 0;
			}
			s += carry;
			if constexpr (SB == 8)
				carry = (u64)__shfl((u32)s, G - 1, G) | (u64)__shfl((u32)(s >> 32), G - 1, G) << 32;
			else
				carry = __shfl(s, G - 1, G);
			if (have)
				__builtin_memcpy(wr + off, &s, SB);
		}
	}
}

#define TIFF_SCAN_CASE(SB, ST) \
	case ((ST) << 4 | (SB)): scan_reg<SB, ST>(rd, wr, rb, G, l); break;

extern "C" __global__ void __launch_bounds__(256)
lda_tiff_unpredict_kernel(uint64_t n_k, uint64_t n_quads, const uint64_t *__restrict__ kcols,
			  uint8_t *ws, uint8_t *out)
{
	/* tiff_plan.h: TIFF_K_QUAD_END, _SRC, _DST, _DPITCH, _GEOM, _SPITCH */
	const u64 *k_quad_end = kcols;
	const u32 tid = threadIdx.x;

	for (u64 q0 = (u64)blockIdx.x * 64; q0 < n_quads; q0 += (u64)gridDim.x * 64) {
		const u64 q = q0 + (tid >> 2);
		if (q >= n_quads)	/* (whole groups: the plan orders the scans by G) */
			continue;
		/* the first scan whose quads end behind q: a search for the workgroup's first
		 * quad, the same in every lane - uniform loads -, and from there one of at
		 * most 6 steps per lane, since every scan has a quad and the workgroup 64 */
		u64 lo = 0, hi = n_k - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (k_quad_end[mid] > q0)
				hi = mid;
			else
				lo = mid + 1;
		}
		hi = lo + 63 < n_k - 1 ? lo + 63 : n_k - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (k_quad_end[mid] > q)
				hi = mid;
			else
				lo = mid + 1;
		}
		const u64 k = lo, geom = kcols[4 * n_k + k], d = kcols[2 * n_k + k];
		const u32 rb = (u32)geom, sb = (u32)(geom >> 32) & 0xFF, st = (u32)(geom >> 40) & 0xFF,
			  G = (u32)(geom >> 48) & 0xFF;
		const u64 row = (q - (k ? k_quad_end[k - 1] : 0)) >> (G == 4 ? 0 : G == 16 ? 2 : 4);
		const u32 l = tid & (G - 1);
		const u8 *rd = ws + kcols[n_k + k] + row * kcols[5 * n_k + k];
		u8 *wr = ((d & LDA_TIFF_DST_WS) ? ws : out) + (d & ~LDA_TIFF_DST_WS) +
			 row * kcols[3 * n_k + k];

		switch (st << 4 | sb) {
		TIFF_SCAN_CASE(1, 1)
		TIFF_SCAN_CASE(1, 2) TIFF_SCAN_CASE(2, 2)
		TIFF_SCAN_CASE(1, 4) TIFF_SCAN_CASE(2, 4) TIFF_SCAN_CASE(4, 4)
		TIFF_SCAN_CASE(1, 8) TIFF_SCAN_CASE(2, 8) TIFF_SCAN_CASE(4, 8) TIFF_SCAN_CASE(8, 8)
		TIFF_SCAN_CASE(1, 16) TIFF_SCAN_CASE(2, 16) TIFF_SCAN_CASE(4, 16) TIFF_SCAN_CASE(8, 16)
		TIFF_SCAN_CASE(1, 3)
		TIFF_SCAN_CASE(1, 6) TIFF_SCAN_CASE(2, 6)
		TIFF_SCAN_CASE(1, 12) TIFF_SCAN_CASE(2, 12) TIFF_SCAN_CASE(4, 12)
		TIFF_SCAN_CASE(2, 24) TIFF_SCAN_CASE(4, 24) TIFF_SCAN_CASE(8, 24)
		TIFF_SCAN_CASE(4, 48) TIFF_SCAN_CASE(8, 48)
		default:
			if (st == 0)
				scan_copy(rd, wr, rb, G, l);
			else if (sb == 1)
				scan_generic<1>(rd, wr, rb, st, G, l);
			else if (sb == 2)
				scan_generic<2>(rd, wr, rb, st, G, l);
			else if (sb == 4)
				scan_generic<4>(rd, wr, rb, st, G, l);
			else
				scan_generic<8>(rd, wr, rb, st, G, l);
		}
	}
}

/* four samples of BPS bytes from BPS planes; cnt of them exist */
template <u32 BPS>
static __device__ __forceinline__ void
gather4(const u8 *planes, u64 plane, u8 *dst, u32 cnt)
{
	u32 pl[BPS], o[BPS];

	/* pl[b]: byte b of the four samples; byte 0, the least significant, lies in the last plane */
#pragma unroll
	for (u32 b = 0; b < BPS; b++) {
		const u8 *p = planes + (u64)(BPS - 1 - b) * plane;
		if (cnt == 4) {
			__builtin_memcpy(&pl[b], p, 4);
		} else {
			pl[b] = 0;
#pragma unroll
			for (u32 i = 0; i < 3; i++)
				if (i < cnt)
					pl[b] |= (u32)p[i] << (8 * i);
		}
	}
#pragma unroll
	for (u32 k = 0; k < BPS; k++)
		o[k] = 0;
#pragma unroll
	for (u32 i = 0; i < 4; i++)
#pragma unroll
		for (u32 b = 0; b < BPS; b++) {
			const u32 at = i * BPS + b;
			o[at >> 2] |= ((pl[b] >> (8 * i)) & 0xFFu) << (8 * (at & 3));
		}
	if (cnt == 4) {
		__builtin_memcpy(dst, o, 4 * BPS);	/* (may be unaligned) */
	} else {
#pragma unroll
		for (u32 at = 0; at < 3 * BPS; at++)
			if (at < cnt * BPS)
				dst[at] = (u8)(o[at >> 2] >> (8 * (at & 3)));
	}
}

/* tile t of all rows: 256 items of one segment, an item four consecutive
 * samples of one kept row; the segment's items are numbered row by row */
extern "C" __global__ void __launch_bounds__(256)
lda_tiff_gather_kernel(uint64_t n_g, uint64_t n_tiles, const uint64_t *__restrict__ g_tile_end,
		       const uint64_t *__restrict__ g_src, const uint64_t *__restrict__ g_dst,
		       const uint64_t *__restrict__ g_dpitch, const uint64_t *__restrict__ g_geom,
		       const uint64_t *__restrict__ g_plane, const uint8_t *__restrict__ ws,
		       uint8_t *__restrict__ out)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		/* (the same in every lane: uniform loads) */
		u64 lo = 0, hi = n_g - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (g_tile_end[mid] > t)
				hi = mid;
			else
				lo = mid + 1;
		}
		const u64 k = lo, geom = g_geom[k];
		const u32 plane = (u32)g_plane[k], items = (u32)(g_plane[k] >> 32);
		const u32 ns = (u32)geom, bps = (u32)(geom >> 32);
		const u32 per_row = (ns + 3) / 4;
		const u64 rel64 = (t - (k ? g_tile_end[k - 1] : 0)) * 256 + threadIdx.x;
		if (rel64 >= items)
			continue;
		const u32 rel = (u32)rel64;
		const u32 row = rel / per_row;
		const u32 i = 4 * (rel - row * per_row);
		const u32 cnt = ns - i < 4 ? ns - i : 4;
		const u8 *planes = ws + g_src[k] + (u64)row * plane * bps + i;
		u8 *dst = out + g_dst[k] + (u64)row * g_dpitch[k] + (u64)i * bps;

		if (bps == 2)
			gather4<2>(planes, plane, dst, cnt);
		else if (bps == 4)
			gather4<4>(planes, plane, dst, cnt);
		else
			gather4<8>(planes, plane, dst, cnt);
	}
}

/* ---- the forward direction ---- */

struct tiff_geom {
	const u8 *in;	/* the segment's kept pixel (0, 0) */
	u64 pitch;
	u32 cw, kw, kr, spp, bps, crb;
};

/* predictors 1 and 2: the 16 / BPS samples of a piece from byte `at` of the room on */
template <u32 BPS>
static __device__ __forceinline__ void
predict_samples(const tiff_geom &g, bool diff, u32 at, u32 (&w)[4])
{
	typedef typename tiff_sample<BPS>::T T;
	u32 row = at / g.crb, col = at - row * g.crb;
	u32 x = col / BPS / g.spp, c = col / BPS - x * g.spp;
	const u32 px = g.spp * BPS;
	T s[16 / BPS];

#pragma unroll
	for (u32 j = 0; j < 16 / BPS; j++) {
		T cur = 0, left = 0;
		if (row < g.kr) {
			/* (the first padded pixel of a row still has a kept pixel to its left) */
			const u8 *p = g.in + (u64)row * g.pitch + col;
			if (x < g.kw)
				__builtin_memcpy(&cur, p, BPS);
			if (diff && x > 0 && x - 1 < g.kw)
				__builtin_memcpy(&left, p - px, BPS);
		}
		s[j] = cur - left;
		col += BPS;
		if (++c == g.spp)
			c = 0, x++;
		if (col == g.crb)
			col = 0, row++, x = 0, c = 0;
	}
	tf_pack<BPS, 16 / BPS>(s, w);
}

/* byte i of plane pl of the shuffled row: byte bps - 1 - pl of sample i */
static __device__ __forceinline__ u32
predict_plane_byte(const tiff_geom &g, u32 row, u32 pl, u32 i, u32 x)
{
	if (row >= g.kr || x >= g.kw)
		return 0;
	return g.in[(u64)row * g.pitch + (u64)i * g.bps + (g.bps - 1 - pl)];
}

/* predictor 3: 16 bytes of the room from byte `at` on */
static __device__ __forceinline__ void
predict_float(const tiff_geom &g, u32 at, u32 (&w)[4])
{
	const u32 ns = g.cw * g.spp;	/* the samples, and a plane's bytes, of a row */
	u32 row = at / g.crb, col = at - row * g.crb;
	u32 pl = col / ns, i = col - pl * ns;
	u32 x = i / g.spp, c = i - x * g.spp;

	w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
	for (u32 j = 0; j < 16; j++) {
		u32 v = predict_plane_byte(g, row, pl, i, x);
		if (col >= g.spp) {
			/* the byte spp places earlier: in this plane, or at the end of the one before */
			if (i >= g.spp)
				v -= predict_plane_byte(g, row, pl, i - g.spp, x - 1);
			else
				v -= predict_plane_byte(g, row, pl - 1, i + ns - g.spp, g.cw - 1);
		}
		w[j >> 2] |= (v & 0xFFu) << (8 * (j & 3));
		col++, i++;
		if (++c == g.spp)
			c = 0, x++;
		if (i == ns)
			i = 0, pl++, x = 0, c = 0;
		if (col == g.crb)
			col = 0, row++, pl = 0;
	}
}

/* tile t of all segments: LDA_TIFF_PTILE bytes of one segment's room, 16 a thread */
extern "C" __global__ void __launch_bounds__(256)
lda_tiff_predict_kernel(uint64_t n, uint64_t n_tiles, const uint64_t *__restrict__ ecols,
			const uint8_t *__restrict__ in, uint8_t *__restrict__ rooms)
{
	/* tiff_plan.h: TIFFW_E_RAW_OFF 3, _PITCH, _CODED, _KEPT, _FMT, _ROOM, _TILE_END */
	const u64 *usize = ecols + 2 * n, *raw_off = ecols + 3 * n, *pitch = ecols + 4 * n,
		  *coded = ecols + 5 * n, *kept = ecols + 6 * n, *fmt = ecols + 7 * n,
		  *room = ecols + 8 * n, *tile_end = ecols + 9 * n;

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		u64 lo = 0, hi = n - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (tile_end[mid] > t)
				hi = mid;
			else
				lo = mid + 1;
		}
		const u64 k = lo;
		const u64 at = (t - (k ? tile_end[k - 1] : 0)) * LDA_TIFF_PTILE + 16 * threadIdx.x;
		if (at >= usize[k])	/* (the room ends on a 16-byte boundary behind usize) */
			continue;
		const u32 f = (u32)fmt[k], pred = (f >> 16) & 0xFF;
		tiff_geom g;
		u32 w[4];
		g.in = in + raw_off[k];
		g.pitch = pitch[k];
		g.cw = (u32)coded[k];
		g.kw = (u32)kept[k];
		g.kr = (u32)(kept[k] >> 32);
		g.spp = f & 0xFF;
		g.bps = (f >> 8) & 0xFF;
		g.crb = g.cw * g.spp * g.bps;
		if (g.kr == 1)
			g.pitch = 0;
		/* (samples behind the segment's last are rows >= coded_rows >= kept_rows: zero) */
		if (pred == 3)
			predict_float(g, (u32)at, w);
		else if (g.bps == 1)
			predict_samples<1>(g, pred == 2, (u32)at, w);
		else if (g.bps == 2)
			predict_samples<2>(g, pred == 2, (u32)at, w);
		else if (g.bps == 4)
			predict_samples<4>(g, pred == 2, (u32)at, w);
		else
			predict_samples<8>(g, pred == 2, (u32)at, w);
		*(uint4 *)(rooms + room[k] + at) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

/* the reader's row of every stream the writer placed: words 0 and 1 where it
 * stands in d_out (header 2, stream, Adler-32 4), words 2 to 7 the input's */
extern "C" __global__ void __launch_bounds__(256)
lda_tiffw_index_kernel(uint64_t n, uint64_t out_avail, const uint64_t *__restrict__ ecols,
		       const uint64_t *__restrict__ csize, const uint64_t *__restrict__ offsets,
		       const uint64_t *__restrict__ block_sums, uint64_t *__restrict__ index)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 total = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (k >= n || total > out_avail)
		return;
	u64 *row = index + LDA_TIFF_WORDS * k;
	row[0] = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
	row[1] = 2 + csize[k] + 4;
#pragma unroll
	for (u32 a = 0; a < 5; a++)
		row[2 + a] = ecols[(3 + a) * n + k];
	row[7] = 0;
}
