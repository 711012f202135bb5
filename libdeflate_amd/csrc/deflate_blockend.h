/*
 * deflate_blockend.h - the end of a block and the container around the blocks
 * (a part of deflate_kernel.hip, included by it and by deflate_entropy.hip):
 * S5 (length-limited codes, exact costs, block type) and S6 (header, token
 * encode or stored pieces) of one block in block_emit(), the gzip / zlib
 * header and trailer, and the bit output through the LDS staging area they
 * write with.  Everything here takes the LDS block as lds_t of the including
 * file, which has the members used below (freq, M, lens, codes, sorted, hw,
 * pre_*, vars[V_TMP1..3, V_NPRE], scan, nxtA as the staging area, carry), and
 * NT, VPT, NWAVES, STG_WORDS, TOK_MATCH and HUFF_LITLEN.  The fused kernels
 * run it inside their tile loop; the entropy kernel (deflate_entropy.hip) runs
 * it from the block descriptors the LZ77 stage left in HBM.
 */

/* workgroup exclusive scan of one value per thread; returns the exclusive
 * prefix and writes the total to *total.  Two barriers. */
static __device__ u32 block_scan(lds_t *L, u32 v, u32 *total)
{
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	u32 incl = wave_scan_incl(v);

	if (lane == 63)
		L->scan[0][wave] = incl;
	__syncthreads();
	/* the waves' sums one per lane, a wave scan over them (a loop over the
	 * sixteen words is six times the instructions, on every wave's path) */
	const u32 sw = lane < NWAVES ? L->scan[0][lane] : 0;
	const u32 iw = wave_scan_incl(sw);
	const u32 base = bcast_lane(iw - sw, wave);
	__syncthreads();
	*total = bcast_lane(iw, NWAVES - 1);
	return base + incl - v;
}

/* the same with ONE barrier: the partial sums alternate between two arrays
 * (*tog flips per call, uniformly), so a fast thread's next call cannot
 * overwrite what a slow thread still reads.  Every second call reuses an
 * array, and the barrier of the call in between orders that. */
static __device__ u32 block_scan1(lds_t *L, u32 v, u32 *total,
				  u32 *tog)
{
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	u32 incl = wave_scan_incl(v);
	u32 *sc = L->scan[*tog];

	*tog ^= 1;
	if (lane == 63)
		sc[wave] = incl;
	__syncthreads();
	const u32 sw = lane < NWAVES ? sc[lane] : 0;
	const u32 iw = wave_scan_incl(sw);
	*total = bcast_lane(iw, NWAVES - 1);
	return bcast_lane(iw - sw, wave) + incl - v;
}

/* length slot / extra bits (lib/deflate_compress.c:237-308 tables, computed) */
static __device__ __forceinline__ void
length_code(u32 len, u32 *slot, u32 *xbits, u32 *xval)
{
	u32 l = len - 3;
	if (l < 8) {
		*slot = l; *xbits = 0; *xval = 0;
	} else if (len == 258) {
		*slot = 28; *xbits = 0; *xval = 0;
	} else {
		u32 hb = 31 - __builtin_clz(l);
		*xbits = hb - 2;
		*slot = 4 * (hb - 1) + ((l >> (hb - 2)) & 3);
		*xval = l & ((1u << (hb - 2)) - 1);
	}
}

static __device__ __forceinline__ void
dist_code(u32 dist, u32 *slot, u32 *xbits, u32 *xval)
{
	u32 d = dist - 1;
	if (d < 4) {
		*slot = d; *xbits = 0; *xval = 0;
	} else {
		u32 hb = 31 - __builtin_clz(d);
		*xbits = hb - 1;
		*slot = 2 * hb + ((d >> (hb - 1)) & 1);
		*xval = d & ((1u << (hb - 1)) - 1);
	}
}

/* ---------------- bit output through the LDS staging area ---------------- */

struct outstate {
	u8 *out;		/* output slot of this buffer */
	u64 avail;
	u64 sg;			/* global byte offset (relative to out, may be
				 * negative via wrap) of staging word 0; 16-aligned
				 * as an absolute address */
	u64 bits;		/* bits produced so far, relative to out[0] */
};

static __device__ __forceinline__ u32 *stg_of(lds_t *L)
{
	return (u32 *)L->nxtA;
}

/* OR 'nbits' (<= 57) bits of 'code' at absolute bit position 'bitpos' */
static __device__ __forceinline__ void
stg_put(lds_t *L, const struct outstate *os, u64 bitpos, u64 code,
	u32 nbits)
{
	if (!nbits)
		return;
	u64 rel = bitpos - 8 * os->sg;	/* sg <= bitpos/8 by construction */
	u32 w = (u32)(rel >> 5), s = (u32)rel & 31;
	u32 *stg = stg_of(L);
	u64 lo = code << s;
	atomicOr((u32 *)&stg[w], (u32)lo);
	if (s + nbits > 32)
		atomicOr((u32 *)&stg[w + 1], (u32)(lo >> 32));
	if (s + nbits > 64)
		atomicOr((u32 *)&stg[w + 2], (u32)(code >> (64 - s)));
}

/*
 * Write the completed bytes of the staging area to HBM and slide the rest to
 * the front.  Whole workgroup; 'final' also writes the last partial unit.
 */
static __device__ __forceinline__ void
stg_flush(lds_t *L, struct outstate *os, bool final)
{
	u32 *stg = stg_of(L);
	u8 *stgb = (u8 *)stg;
	const u32 tid = threadIdx.x;
	u64 done_bytes = final ? (os->bits + 7) / 8 : os->bits / 8;
	u64 rel_end = done_bytes - os->sg;	/* staging bytes that are final */
	s64 first = -(s64)os->sg;		/* staging index of out[0] if sg<0 */
	u32 start = first > 0 ? (u32)first : 0;
	u32 units = final ? (u32)((rel_end + 15) / 16) : (u32)(rel_end / 16);

	__syncthreads();
	/* 16-byte units: unit u covers staging bytes [16u, 16u+16) */
	for (u32 u = tid; u < units; u += NT) {
		u32 b0 = u * 16, b1 = b0 + 16;
		u8 *g = os->out + (s64)(os->sg + b0);
		if (b0 >= start && b1 <= rel_end) {
			*(uint4 *)g = *(const uint4 *)(stgb + b0);
		} else {
			for (u32 b = b0 < start ? start : b0; b < b1 && b < rel_end; b++)
				g[b - b0] = stgb[b];
		}
	}
	/* slide the unfinished tail to the front; thread i both clears word i
	 * and (for the few tail words) rewrites it, so no barrier in between */
	u32 keep_from = units * 16;
	u32 total_words = (u32)((os->bits - 8 * os->sg + 31) / 32) + 1;
	u32 keep_words = final ? 0 : total_words - keep_from / 4;
	u32 v = 0;
	if (tid < keep_words && keep_from / 4 + tid < STG_WORDS + 8)
		v = stg[keep_from / 4 + tid];
	__syncthreads();
#if LDA_ENTROPY
	/* nothing is ever put at or behind os->bits, and nothing but this
	 * function and stg_restore() clears: the words from total_words on are
	 * still zero */
	const u32 clear_words = total_words < STG_WORDS + 8 ? total_words : STG_WORDS + 8;
#else
	const u32 clear_words = STG_WORDS + 8;
#endif
	for (u32 i = tid; i < clear_words; i += NT)
		stg[i] = 0;
	if (tid < keep_words)
		stg[tid] = v;
	os->sg += keep_from;
	/* callers put a barrier before the next stg_put by another thread */
}

/* bring back the few unfinished bytes saved in carry[] (the staging area
 * shares LDS with the tile scratch and is clobbered between blocks) */
static __device__ __forceinline__ void stg_restore(lds_t *L)
{
	u32 *stg = stg_of(L);

	__syncthreads();
	for (u32 i = threadIdx.x; i < STG_WORDS + 8; i += NT)
		stg[i] = i < 6 ? L->carry[i] : 0;
	__syncthreads();
}

static __device__ __forceinline__ void stg_save(lds_t *L, struct outstate *os)
{
	stg_flush(L, os, false);
	if (threadIdx.x < 6)
		L->carry[threadIdx.x] = stg_of(L)[threadIdx.x];
	__syncthreads();
}

/* the container header (gzip_compress.c:44-64, zlib_compress.c:45-60) at bit
 * 0: thread 0 writes it, every thread advances os.  BGZF: htslib's fixed
 * 16 bytes - FEXTRA, XFL 0 and OS 0xff at every level, XLEN 6, the "BC"
 * subfield of length 2 - and BSIZE as 0 until finish_stream() knows it */
static __device__ __forceinline__ void
put_container_header(lds_t *L, struct outstate *os, int format, int level,
		     const u8 *__restrict__ dict_pre, u32 hdr_bytes, u32 tid)
{
	if (tid == 0) {
		if (format == LDA_FMT_BGZF) {
			stg_put(L, os, 0, 0x04088B1Full, 32);
			stg_put(L, os, 32, 0, 32);	/* MTIME */
			stg_put(L, os, 64, 0xFFu << 8, 16);
			stg_put(L, os, 80, 0x0243420006ull, 48);	/* 06 00 'B' 'C' 02 00 */
		} else if (format == LDA_FMT_GZIP) {
			/* XFL 4 fastest, 2 best */
			u32 xfl = level < 2 ? 4 : level >= 8 ? 2 : 0;
			stg_put(L, os, 0, 0x00088B1Full, 32);
			stg_put(L, os, 32, 0, 32);	/* MTIME */
			stg_put(L, os, 64, xfl | (0xFFu << 8), 16);
		} else {
			u32 fl = level < 2 ? 0 : level < 6 ? 1 :
				 level < 8 ? 2 : 3;
			u32 h = (0x78u << 8) | (fl << 6);
			if (dict_pre) {
				/* FDICT, then DICTID: the Adler-32 of the
				 * whole dictionary, big-endian (RFC 1950 2.2) */
				h |= 0x20;
				h += (31 - h % 31) % 31;
				stg_put(L, os, 16, __builtin_bswap32(((const u32 *)dict_pre)[1]), 32);
			} else {
				h |= 31 - (h % 31);
			}
			stg_put(L, os, 0, ((h & 0xFF) << 8) | (h >> 8), 16);
		}
	}
	os->bits = 8 * hdr_bytes;
}

#if LDA_ENTROPY
/*
 * The entropy kernel's token encode: packed code tables and ENC_K consecutive
 * tokens per thread.  (The fused kernels keep the one-token-per-thread loop in
 * block_emit(): their LDS has no room for the wider staging area, and their
 * bytes are what tests/test_entropy_encode_gpu.py compares these with.)
 *
 * What lives in M[] when:
 *   S5 rank sort      keys [0, 320), used counts [320, 322), sortedO [324, 340)
 *   S5 two trees      the litlen tree's scratch from M + 512 (HUFF_LITLEN)
 *   S5 precode items  run starts [0, 321]
 *   S6                the tables below, [0, ENC_TAB_WORDS): written once per
 *                     dynamic or static block after its codes exist and before
 *                     its header (whose scan and flush are the barriers between
 *                     the build and the first lookup), read by the token loop
 */
#define ENC_K 4			/* tokens per thread per window: one 16-byte load */
#define ENC_LIT 0		/* [256] by byte:        codeword | bits << 24 */
#define ENC_LEN 256		/* [256] by length - 3:  codeword | extra value << code bits | (code + extra bits) << 24 */
#define ENC_OFF 512		/* [30] by offset slot:  codeword | code bits << 16 | extra bits << 20 */
#define ENC_TAB_WORDS 544
static_assert(ENC_TAB_WORDS <= sizeof(((struct deflate_lds *)0)->M) / sizeof(u32), "the tables live in M[]");
/* a window of ENC_K * NT tokens of at most 48 bits behind what a flush leaves
 * (under 16 bytes and a partial byte) must fit the staging area, with the 64
 * bits of slack the flush rule in encode_tokens() keeps */
static_assert(32 * STG_WORDS >= 48 * ENC_K * NT + 64 + 8 * 16 + 8, "a worst-case window fits the staging area");

/* 542 entries per block against its thousands of tokens: three LDS stores per
 * thread and no barrier of its own, less than one round of the token loop, so
 * there is no block too small for it */
static __device__ __forceinline__ void enc_tables_build(lds_t *L, u32 tid)
{
	u32 *tab = L->M;

	for (u32 i = tid; i < 256; i += NT) {
		u32 sl, xb, xv;
		tab[ENC_LIT + i] = L->codes[i] | ((u32)L->lens[i] << 24);
		length_code(i + 3, &sl, &xb, &xv);
		const u32 ll = L->lens[257 + sl];
		tab[ENC_LEN + i] = L->codes[257 + sl] | (xv << ll) | ((ll + xb) << 24);
	}
	if (tid < 30) {
		const u32 xb = tid < 4 ? 0 : (tid >> 1) - 1;
		tab[ENC_OFF + tid] = L->codes[288 + tid] | ((u32)L->lens[288 + tid] << 16) | (xb << 20);
	}
}

/* one token's bits (at most 48) and their count; 0 bits when !valid.  No
 * branch between literal and match: the first word is the literal's or the
 * length's entry, the offset part is masked away for a literal */
static __device__ __forceinline__ u64 enc_token(const u32 *tab, u32 tok, bool valid, u32 *nbits)
{
	const bool match = (tok & TOK_MATCH) != 0;
	const u32 e = tab[(match ? ENC_LEN : ENC_LIT) + (tok & 0xFF)];
	const u32 d = (tok >> 8) & 0x7FFF;	/* offset - 1 */
	const u32 hb = 31 - __builtin_clz(d | 2);	/* >= 1: the shift below stays defined for d < 4 */
	const u32 slot = d < 4 ? d : 2 * hb + ((d >> (hb - 1)) & 1);
	const u32 o = tab[ENC_OFF + slot];
	const u32 n1 = e >> 24, ol = (o >> 16) & 15, oxb = o >> 20;
	const u32 ov = (o & 0xFFFF) | ((d & ((1u << oxb) - 1)) << ol);	/* <= 15 + 13 bits */
	u64 v = (e & 0xFFFFFF) | (match ? (u64)ov << n1 : 0);
	u32 n = n1 + (match ? ol + oxb : 0);

	*nbits = valid ? n : 0;
	return valid ? v : 0;
}

/* OR v (< 2^48) at bit 'pos' of the 224 bits a[0..3]; pos <= 31 + 48 * J for
 * the J-th token of a thread, which says which of a[] it can reach */
template <int J>
static __device__ __forceinline__ void enc_acc(u64 (&a)[4], u64 v, u32 pos)
{
	const u32 q = pos >> 6, sh = pos & 63;
	const u64 lo = v << sh, hi = (v >> 1) >> (63 - sh);

	if (J == 0) {
		a[0] = lo;
		a[1] = hi;
		a[2] = a[3] = 0;
	} else {
		a[0] |= q == 0 ? lo : 0;
		a[1] |= q == 0 ? hi : q == 1 ? lo : 0;
		if (J < 3) {
			a[2] |= q == 1 ? hi : 0;
		} else {
			a[2] |= q == 1 ? hi : q == 2 ? lo : 0;
			a[3] |= q == 2 ? hi : 0;
		}
	}
}

/*
 * The tokens tokg[0, nseq) of a block at os->bits, ENC_K * NT at a time: every
 * thread takes ENC_K consecutive tokens (one 16-byte load; the list of a later
 * block starts anywhere, so the windows start at the 16-byte boundary at or
 * before tokg and the tokens in front of tokg[0] count as absent), joins their
 * bits in registers at the bit phase its first staging word will have, and
 * after ONE workgroup scan per window writes a run of consecutive staging
 * words: the first and the last are shared with the neighbours (ds_or), the
 * words between are this thread's alone (plain stores over zeros).  Ends with
 * the staging area flushed.  Whole workgroup.
 */
static __device__ __forceinline__ void
encode_tokens(lds_t *L, struct outstate *os, const u32 *__restrict__ tokg, u32 nseq,
	      u32 *tog, u32 tid)
{
	const u32 *tab = L->M;
	u32 *stg = stg_of(L);
	const u32 mis = ((u32)(uintptr_t)tokg >> 2) & (ENC_K - 1);
	const uint4 *__restrict__ tok4 = (const uint4 *)(tokg - mis);
	const u32 end = nseq + mis;	/* window positions [mis, end) are tokens */

	/* (the next window's tokens are requested before this one is encoded:
	 * the list is in HBM.  A 16-byte unit with a token in it lies inside
	 * the buffer's list: its base and its stride are multiples of 16 bytes) */
	uint4 nxt = make_uint4(0, 0, 0, 0);
	if (ENC_K * tid < end)
		nxt = tok4[tid];
	for (u32 b0 = 0; b0 < end; b0 += ENC_K * NT) {
		const u32 i0 = b0 + ENC_K * tid;
		const uint4 t = nxt;
		if (i0 + ENC_K * NT < end)
			nxt = tok4[(i0 + ENC_K * NT) / ENC_K];
		u32 n0, n1, n2, n3;
		const u64 v0 = enc_token(tab, t.x, i0 >= mis && i0 < end, &n0);
		const u64 v1 = enc_token(tab, t.y, i0 + 1 >= mis && i0 + 1 < end, &n1);
		const u64 v2 = enc_token(tab, t.z, i0 + 2 >= mis && i0 + 2 < end, &n2);
		const u64 v3 = enc_token(tab, t.w, i0 + 3 >= mis && i0 + 3 < end, &n3);
		const u32 nb = n0 + n1 + n2 + n3;	/* <= 192 */
		u32 tot;
		const u32 off = block_scan1(L, nb, &tot, tog);
		/* bit position relative to staging word 0 (sg <= bits / 8) */
		const u32 p = (u32)(os->bits - 8 * os->sg) + off;
		const u32 w = p >> 5, s = p & 31;
		u64 a[4];
		enc_acc<0>(a, v0, s);
		enc_acc<1>(a, v1, s + n0);
		enc_acc<2>(a, v2, s + n0 + n1);
		enc_acc<3>(a, v3, s + n0 + n1 + n2);
		if (nb) {
			const u32 last = (s + nb - 1) >> 5;	/* <= 6 */
			const u32 wd[7] = { (u32)a[0], (u32)(a[0] >> 32), (u32)a[1], (u32)(a[1] >> 32),
					    (u32)a[2], (u32)(a[2] >> 32), (u32)a[3] };
			atomicOr(&stg[w], wd[0]);
#pragma unroll
			for (u32 i = 1; i < 7; i++) {
				if (i < last)
					stg[w + i] = wd[i];
				else if (i == last)
					atomicOr(&stg[w + i], wd[i]);
			}
		}
		os->bits += tot;
		/* room for one more window of 48-bit tokens? */
		if (os->bits - 8 * os->sg + 48 * ENC_K * NT + 64 > 32 * STG_WORDS)
			stg_flush(L, os, false);
	}
	stg_flush(L, os, false);
}
#endif /* LDA_ENTROPY */

/*
 * One block at os->bits: the codes from the histogram in L->freq (without the
 * end-of-block symbol; this adds it), the cheapest of dynamic / static /
 * stored, the block written through the staging area and its unfinished
 * bytes saved in carry[].  tokg[0, nseq) are the block's tokens (TOK_MATCH),
 * inp[bstart, bstart + blen) its bytes (stored pieces).  The staging area
 * holds os's unfinished bytes in carry[] on entry (stg_save()).  Returns false,
 * with nothing written, when the block and ftr_bytes of trailer do not fit
 * os->avail.  Whole workgroup; tid / lane / wave are the caller's.
 */
static __device__ __forceinline__ bool
block_emit(lds_t *L, struct outstate *os, const u32 *__restrict__ tokg, u32 nseq,
	   const u8 *__restrict__ inp, u32 bstart, u32 blen, u32 is_final,
	   bool stored_only, u32 ftr_bytes, u32 *tog, u32 tid, u32 lane, u32 wave)
{
	PROF_DECL;
	PROF_START();
	/* ---- S5: codes, costs, block type ---- */
	u32 btype = 0;	/* 0 stored, 1 static, 2 dynamic */
	if (!stored_only) {
		if (tid == 0)
			L->freq[256]++;
		__syncthreads();
		/* rank sort of both alphabets by the whole workgroup: the
		 * used symbols are collected first (their keys, freq << 9 |
		 * symbol, in any order), then every key counts the keys
		 * below it - a block uses a third of the litlen alphabet,
		 * a small one a fifth; M[] is free scratch here */
		{
			u32 *keys = L->M;		/* [288] litlen, [288, 320) offset keys */
			u32 *usedv = L->M + 320;	/* [2] used counts */
			u16 *sortedO = (u16 *)(L->M + 324);	/* [32] */
			if (tid < 2)
				usedv[tid] = 0;
			__syncthreads();
			for (u32 vt = tid; vt < 320; vt += NT) {
				const u32 f = L->freq[vt];
				if (f) {
					if (vt < 288)
						keys[atomicAdd(&usedv[0], 1u)] = (f << 9) | vt;
					else
						keys[288 + atomicAdd(&usedv[1], 1u)] =
							(f << 9) | (vt - 288);
				}
			}
			__syncthreads();
			{
				const u32 m1 = usedv[0], m2 = usedv[1];
				for (u32 i = tid; i < m1 + m2; i += NT) {
					const bool lit = i < m1;
					const u32 lo = lit ? 0 : 288, m = lit ? m1 : m2;
					const u32 key = keys[lit ? i : 288 + i - m1];
					u32 r = 0;
					for (u32 q = 0; q < m; q++)
						r += keys[lo + q] < key;
					if (lit)
						L->sorted[r] = (u16)(key & 511);
					else
						sortedO[r] = (u16)(key & 511);
				}
			}
			__syncthreads();
			PROF_MARK(10);
			/* the two trees are built side by side on two waves */
			if (wave == 0)
				make_code(L->freq, 288, 15, L->lens, L->codes,
					  L->sorted, HUFF_LITLEN(L),
					  usedv[0], true, lane);
			else if (wave == 1)
				make_code(L->freq + 288, 32, 15, L->lens + 288,
					  L->codes + 288, sortedO,
					  (huff_scratch<32> *)L->hw,
					  usedv[1], true, lane);
		}
		__syncthreads();
		PROF_MARK(11);
		/* precode items: run-length coding of the code lengths
		 * (deflate_compress.c:1482-1557 semantics), one thread per
		 * length, then one thread per run */
		{
			u32 *starts = L->M;		/* [<= 321] run start indices */
			if (tid == 0) {
				L->vars[V_TMP1] = 257;
				L->vars[V_TMP2] = 1;
			}
			if (tid < 19)
				L->pre_freq[tid] = 0;
			__syncthreads();
			for (u32 vt = tid; vt < 320; vt += NT) {
				if (vt < 288 && vt >= 257 && L->lens[vt])
					atomicMax((u32 *)&L->vars[V_TMP1], vt + 1);
				if (vt >= 288 && L->lens[vt])
					atomicMax((u32 *)&L->vars[V_TMP2], vt - 288 + 1);
			}
			__syncthreads();
			const u32 nlit = L->vars[V_TMP1], noff = L->vars[V_TMP2];
			const u32 total = nlit + noff;
			/* element e of the concatenated lengths: thread tid owns
			 * the VPT consecutive elements from tid * VPT */
			u32 isst[VPT], nst = 0;
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				const u32 e = tid * VPT + j;
				isst[j] = 0;
				if (e < total) {
					u32 v = L->lens[e < nlit ? e : 288 + (e - nlit)];
					u32 pv = 0xFF;
					if (e)
						pv = L->lens[e - 1 < nlit ? e - 1 :
							     288 + (e - 1 - nlit)];
					isst[j] = pv != v;
				}
				nst += isst[j];
			}
			u32 nruns;
			u32 ridx = block_scan(L, nst, &nruns);
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				if (isst[j])
					starts[ridx] = tid * VPT + j;
				ridx += isst[j];
			}
			if (tid == 0)
				starts[nruns] = total;
			__syncthreads();
			/* run r: thread tid owns the runs from tid * VPT */
			u32 rv[VPT], rlen[VPT], nitems[VPT], nit = 0;
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				const u32 r = tid * VPT + j;
				rv[j] = rlen[j] = nitems[j] = 0;
				if (r < nruns) {
					u32 st = starts[r];
					rlen[j] = starts[r + 1] - st;
					rv[j] = L->lens[st < nlit ? st : 288 + (st - nlit)];
					if (rv[j] == 0) {
						u32 full = rlen[j] / 138, rem = rlen[j] % 138;
						nitems[j] = full + (rem >= 3 ? 1 : rem);
					} else if (rlen[j] >= 4) {
						u32 l1 = rlen[j] - 1;
						nitems[j] = 1 + l1 / 6 + (l1 % 6 >= 3 ? 1 : l1 % 6);
					} else {
						nitems[j] = rlen[j];
					}
				}
				nit += nitems[j];
			}
			u32 ni;
			u32 at = block_scan(L, nit, &ni);
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				if (tid * VPT + j < nruns) {
					u32 left = rlen[j];
					const u32 rvj = rv[j];
					if (rvj == 0) {
						while (left >= 11) {
							u32 r = left > 138 ? 138 : left;
							L->pre_items[at++] = 18 | ((r - 11) << 5);
							atomicAdd((u32 *)&L->pre_freq[18], 1u);
							left -= r;
						}
						if (left >= 3) {
							L->pre_items[at++] = 17 | ((left - 3) << 5);
							atomicAdd((u32 *)&L->pre_freq[17], 1u);
							left = 0;
						}
					} else if (left >= 4) {
						L->pre_items[at++] = (u16)rvj;
						left--;
						u32 n16 = 0;
						while (left >= 3) {
							u32 r = left > 6 ? 6 : left;
							L->pre_items[at++] = 16 | ((r - 3) << 5);
							n16++;
							left -= r;
						}
						atomicAdd((u32 *)&L->pre_freq[16], n16);
						atomicAdd((u32 *)&L->pre_freq[rvj], 1u);
					}
					if (left)
						atomicAdd((u32 *)&L->pre_freq[rvj], left);
					while (left) {
						L->pre_items[at++] = (u16)rvj;
						left--;
					}
				}
			}
			if (tid == 0)
				L->vars[V_NPRE] = ni;
		}
		__syncthreads();
		PROF_MARK(23);
		if (wave == 0)
			make_code(L->pre_freq, 19, 7, L->pre_lens, L->pre_codes,
				  L->sorted, (huff_scratch<32> *)L->hw,
				  0, false, lane);
		__syncthreads();
		PROF_MARK(22);
		/* exact costs (deflate_compress.c:1747-1808) */
		u32 dyn = 0, stat = 0;
		for (u32 vt = tid; vt < 320; vt += NT) {
			u32 f = L->freq[vt];
			u32 xb = 0, sl = 8;
			if (vt < 288) {
				sl = vt < 144 ? 8 : vt < 256 ? 9 : vt < 280 ? 7 : 8;
				if (vt >= 265 && vt < 285)
					xb = (vt - 261) >> 2;
			} else {
				u32 ds = vt - 288;
				sl = 5;
				if (ds >= 4)
					xb = (ds >> 1) - 1;
			}
			dyn += f * (L->lens[vt] + xb);
			stat += f * (sl + xb);
		}
		if (tid < 19) {
			u32 xb = tid == 16 ? 2 : tid == 17 ? 3 : tid == 18 ? 7 : 0;
			dyn += L->pre_freq[tid] * (L->pre_lens[tid] + xb);
		}
		u32 dyn_tot, stat_tot;
		(void)block_scan(L, dyn, &dyn_tot);
		(void)block_scan(L, stat, &stat_tot);
		static const u8 perm[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10,
					     5, 11, 4, 12, 3, 13, 2, 14,
					     1, 15 };
		u32 nexp = 19;
		while (nexp > 4 && L->pre_lens[perm[nexp - 1]] == 0)
			nexp--;
		u32 cost_dyn = 3 + 5 + 5 + 4 + 3 * nexp + dyn_tot;
		u32 cost_stat = 3 + stat_tot;
		/* stored: align + (LEN,NLEN) per <= 65535 piece */
		u32 pieces = blen ? (blen + 65534) / 65535 : 1;
		u32 pad = (u32)((0 - (os->bits + 3)) & 7);
		u64 cost_stored = 3 + pad + 32 + 8ull * blen +
				  (u64)(pieces - 1) * 40;
		u64 best = cost_stored;
		btype = 0;
		if (cost_stat < best) {
			best = cost_stat;
			btype = 1;
		}
		if (cost_dyn < best) {
			best = cost_dyn;
			btype = 2;
		}
		if ((os->bits + best + 7) / 8 + ftr_bytes > os->avail)
			return false;
		L->vars[V_TMP3] = nexp;
	} else {
		u32 pieces = blen ? (blen + 65534) / 65535 : 1;
		u64 cost = (u64)pieces * 40 + 8ull * blen;
		if ((os->bits + cost + 7) / 8 + ftr_bytes > os->avail)
			return false;
	}

	PROF_MARK(7);
	/* ---- S6: emit ---- */
	stg_restore(L);
	if (btype == 0) {
		/* stored pieces: header by thread 0, bytes as 8-bit
		 * "codes" through the same staging path */
		u32 done = 0;
		do {
			u32 piece = blen - done > 65535 ? 65535 : blen - done;
			u32 fin = (is_final && done + piece == blen) ? 1 : 0;
			u32 pad = (u32)((0 - (os->bits + 3)) & 7);
			if (tid == 0) {
				stg_put(L, os, os->bits, fin, 3);
				u64 b = os->bits + 3 + pad;
				stg_put(L, os, b, piece | ((u64)(piece ^ 0xFFFF) << 16), 32);
			}
			os->bits += 3 + pad + 32;
			__syncthreads();
#if LDA_ENTROPY
			/* the piece's bytes start at a byte boundary of the
			 * output: the few up to the next 16-byte boundary go
			 * through the staging area and complete its last unit,
			 * which leaves it empty, the 16-byte units after them
			 * are copied from the input straight to the output
			 * (the staging words stay zero, its base moves on),
			 * and the rest of under 16 bytes is staged again */
			{
				const u8 *__restrict__ src = inp + bstart + done;
				u8 *dst = os->out + (s64)(os->bits / 8);
				u32 head = (0 - (u32)(uintptr_t)dst) & 15;
				head = head < piece ? head : piece;
				const u32 mid = (piece - head) & ~15u;
				const u32 tail = piece - head - mid;
				if (tid < head)
					stg_put(L, os, os->bits + 8 * tid, src[tid], 8);
				os->bits += 8 * head;
				stg_flush(L, os, false);
				for (u32 u = tid; u < mid / 16; u += NT) {
					uint4 v;
					__builtin_memcpy(&v, src + head + 16 * u, 16);
					*(uint4 *)(dst + head + 16 * u) = v;
				}
				if (mid) {	/* (the staging area is empty) */
					os->bits += 8ull * mid;
					os->sg += mid;
				}
				__syncthreads();
				if (tid < tail)
					stg_put(L, os, os->bits + 8 * tid, src[head + mid + tid], 8);
				os->bits += 8 * tail;
				__syncthreads();
			}
#else
			for (u32 w0 = 0; w0 < piece; w0 += 2048) {
				u32 cnt = piece - w0 < 2048 ? piece - w0 : 2048;
				stg_flush(L, os, false);
				__syncthreads();
				for (u32 j = tid; j < cnt; j += NT) {
					u32 pos = bstart + done + w0 + j;
					stg_put(L, os, os->bits + 8ull * j, inp[pos], 8);
				}
				os->bits += 8ull * cnt;
				__syncthreads();
			}
#endif
			done += piece;
		} while (done < blen);
		stg_flush(L, os, false);
	} else {
		if (btype == 1) {
			/* static codes: lens fixed, canonical codewords */
			__syncthreads();
			for (u32 s = tid; s < 320; s += NT)
				L->lens[s] = s < 144 ? 8 : s < 256 ? 9 :
					     s < 280 ? 7 : s < 288 ? 8 : 5;
			__syncthreads();
			if (tid == 0) {
				u32 nc[16] = { 0 }, bl[16] = { 0 };
				for (u32 s = 0; s < 288; s++)
					bl[L->lens[s]]++;
				u32 code = 0;
				for (u32 d = 1; d < 16; d++) {
					code = (code + bl[d - 1]) << 1;
					nc[d] = code;
				}
				for (u32 s = 0; s < 288; s++) {
					u32 l = L->lens[s];
					L->codes[s] = (u16)(__brev(nc[l]++) >> (32 - l));
				}
				for (u32 s = 0; s < 32; s++)
					L->codes[288 + s] = (u16)(__brev(s) >> 27);
			}
			__syncthreads();
		}
#if LDA_ENTROPY
		enc_tables_build(L, tid);
		PROF_MARK(40);
#endif
		/* block header: thread 0 the fixed fields, threads
		 * 1..nexp the precode lengths, then one thread per
		 * precode item; bit offsets by a workgroup scan */
		{
			u64 hcode[VPT];
			u32 hbits[VPT], hsum = 0;
			const u32 nexp = btype == 2 ? L->vars[V_TMP3] : 0;
			const u32 ni = btype == 2 ? L->vars[V_NPRE] : 0;
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				const u32 vt = tid * VPT + j;	/* header item */
				hcode[j] = 0;
				hbits[j] = 0;
				if (vt == 0) {
					hcode[j] = is_final | (btype << 1);
					hbits[j] = 3;
					if (btype == 2) {
						u32 nlit = L->vars[V_TMP1], noff = L->vars[V_TMP2];
						hcode[j] |= (u64)((nlit - 257) | ((noff - 1) << 5) |
								  ((nexp - 4) << 10)) << 3;
						hbits[j] = 17;
					}
				} else if (vt <= nexp) {
					static const u8 perm2[19] = { 16, 17, 18, 0, 8, 7,
						9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
					hcode[j] = L->pre_lens[perm2[vt - 1]];
					hbits[j] = 3;
				} else if (vt <= nexp + ni) {
					u32 it = L->pre_items[vt - nexp - 1];
					u32 sym = it & 31, ex = it >> 5;
					u32 l = L->pre_lens[sym];
					u32 xb = sym == 16 ? 2 : sym == 17 ? 3 :
						 sym == 18 ? 7 : 0;
					hcode[j] = L->pre_codes[sym] | ((u64)ex << l);
					hbits[j] = l + xb;
				}
				hsum += hbits[j];
			}
			u32 htot;
			u32 hoff = block_scan(L, hsum, &htot);
#pragma unroll
			for (u32 j = 0; j < VPT; j++) {
				stg_put(L, os, os->bits + hoff, hcode[j], hbits[j]);
				hoff += hbits[j];
			}
			os->bits += htot;
		}
		stg_flush(L, os, false);

		PROF_MARK(9);
#if LDA_ENTROPY
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		encode_tokens(L, os, tokg, nseq, tog, tid);
#else
		/* tokens, NT at a time: one token per thread, a workgroup
		 * prefix sum of the bit lengths (single-barrier scan),
		 * ds_or into the staging area.  The staging area is only
		 * written out when another window might not fit (a token is
		 * at most 48 bits: 6 KiB per window in the worst case, a
		 * fifth of that on text). */
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		/* (the next window's token is requested before this one is
		 * encoded: the list is in HBM) */
		u32 tok_nxt = tid < nseq ? tokg[tid] : 0;
		for (u32 b0 = 0; b0 < nseq; b0 += NT) {
			u64 code = 0;
			u32 nb = 0;
			const u32 tok = tok_nxt;
			if (b0 + NT + tid < nseq)
				tok_nxt = tokg[b0 + NT + tid];
			if (b0 + tid < nseq) {
				if (tok & TOK_MATCH) {
					const u32 len = (tok & 0xFF) + 3, dist = ((tok >> 8) & 0x7FFF) + 1;
					u32 sl, xb, xv, ds, dxb, dxv;
					length_code(len, &sl, &xb, &xv);
					dist_code(dist, &ds, &dxb, &dxv);
					u32 ll = L->lens[257 + sl];
					u32 dl = L->lens[288 + ds];
					u64 v = L->codes[257 + sl];
					u32 sh = ll;
					v |= (u64)xv << sh;
					sh += xb;
					v |= (u64)L->codes[288 + ds] << sh;
					sh += dl;
					v |= (u64)dxv << sh;
					sh += dxb;
					code = v;
					nb = sh;
				} else {
					code = L->codes[tok];
					nb = L->lens[tok];
				}
			}
			u32 tot;
			u32 off = block_scan1(L, nb, &tot, tog);
			stg_put(L, os, os->bits + off, code, nb);
			os->bits += tot;
			/* room for one more window of 48-bit tokens? */
			if (os->bits - 8 * os->sg + 48 * NT + 64 > 32 * STG_WORDS)
				stg_flush(L, os, false);
		}
		stg_flush(L, os, false);
#endif
		__syncthreads();
		/* end of block */
		if (tid == 0)
			stg_put(L, os, os->bits, L->codes[256], L->lens[256]);
		os->bits += L->lens[256];
		__syncthreads();
	}

	/* keep the unfinished staging bytes across the next tiles
	 * (M is reused as tile scratch) */
	stg_save(L, os);
	PROF_MARK(8);
	return true;
}

/*
 * After the last block: the empty stored block that byte-aligns a segment
 * other than the last (lib/deflate_compress.c:1839-1847), the trailer
 * (gzip_compress.c:73-79 / zlib_compress.c:66-72: sum, and n for gzip and
 * BGZF), the last bytes, the stream's size - 0 when it does not fit - and a
 * BGZF member's BSIZE.  Whole workgroup.
 */
static __device__ __forceinline__ void
finish_stream(lds_t *L, struct outstate *os, bool overflow, bool seg_last,
	      int format, u32 ftr_bytes, const u32 *__restrict__ sums, u64 c, u32 n,
	      u64 *__restrict__ out_nbytes, u32 tid)
{
	__syncthreads();
	if (!overflow && !seg_last &&
	    (os->bits + 3 + 7) / 8 + 4 > os->avail)
		overflow = true;
	if (!overflow) {
		stg_restore(L);
		if (!seg_last) {
			/* empty stored block: BFINAL 0, BTYPE 00, pad, LEN 0, NLEN ~0 */
			u64 fb = 8 * ((os->bits + 3 + 7) / 8);
			if (tid == 0)
				stg_put(L, os, fb, 0xFFFF0000ull, 32);
			os->bits = fb + 32;
			__syncthreads();
		}
		if (ftr_bytes) {
			u32 sum = sums ? sums[c] : 0;
			u64 fb = 8 * ((os->bits + 7) / 8);
			if (tid == 0) {
				if (format != LDA_FMT_ZLIB) {	/* gzip, BGZF */
					stg_put(L, os, fb, sum, 32);
					stg_put(L, os, fb + 32, n, 32);
				} else {
					stg_put(L, os, fb, __builtin_bswap32(sum), 32);
				}
			}
			os->bits = fb + 8 * ftr_bytes;
			__syncthreads();
		}
		stg_flush(L, os, true);
		const u32 size = (u32)((os->bits + 7) / 8);
		if (tid == 0)
			out_nbytes[c] = size;
		if (format == LDA_FMT_BGZF) {
			/* BSIZE = size - 1 (<= 65535: os->avail is at most
			 * LDA_BGZF_MEMBER_MAX).  Bytes 16..17 went out as zeros in
			 * some thread's 16-byte unit, maybe in the flush above: every
			 * thread waits for its stores (acknowledged by the L2 that
			 * thread 0's store goes to as well), then thread 0 overwrites
			 * the two bytes with one vector store */
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__syncthreads();
			if (tid == 0) {
				const u16 bsize = (u16)(size - 1);
				__builtin_memcpy(os->out + 16, &bsize, 2);
			}
		}
	} else if (tid == 0) {
		out_nbytes[c] = 0;
	}
	__syncthreads();
}
