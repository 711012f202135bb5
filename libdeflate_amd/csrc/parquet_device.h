/*
 * parquet_device.h - what the kernels of the two Parquet calls share
 * (parquet_kernels.hip, parquet_strings_kernels.hip): the info words of a data
 * page, the wave's window on a stream, and how a slot finds its page, its level
 * and rank and its dictionary index in what lda_pq_runs_kernel listed.
 */
#ifndef LDA_PARQUET_DEVICE_H
#define LDA_PARQUET_DEVICE_H

#include "device_common.h"
#include "kernels.h"

#define PQ_WIN 4096	/* bytes of a wave's window: 64 lanes x 4 x 16 */

/* the info words of a data page */
enum { PQ_I_STATUS = 0, PQ_I_INDEX_BAD, PQ_I_LRUNS, PQ_I_IRUNS, PQ_I_VALID, PQ_I_VAL_AT, PQ_I_W };

struct pq_win {
	u8 *lds;
	const u8 *base;
	u32 len;	/* bytes behind it read as 0 */
	u32 at;		/* the window holds [at, at + PQ_WIN) */
};

static __device__ __forceinline__ void win_load(pq_win &w, u32 at)
{
	const u32 lane = lane_id();
	wave_sync();
#pragma unroll
	for (u32 i = 0; i < PQ_WIN / 1024; i++) {
		const u32 o = (i * 64 + lane) * 16;
		*(uint4 *)(w.lds + o) = load16_guard(w.base, (u64)at + o, w.len);
	}
	w.at = at;
	wave_sync();
}

static __device__ __forceinline__ void win_open(pq_win &w, const u8 *base, u32 len)
{
	w.base = base;
	w.len = len;
	win_load(w, 0);
}

/* byte p of the stream, p the same in every lane */
static __device__ __forceinline__ u32 win_byte(pq_win &w, u32 p)
{
	p = bcast_first(p);
	if (p - w.at >= PQ_WIN)
		win_load(w, p);
	return w.lds[p - w.at];
}

/* the set bits among the first `bits` at a */
static __device__ __forceinline__ u32 pq_popcount(const u8 *__restrict__ a, u32 bits)
{
	u32 c = 0, k = 0;
	for (; k + 64 <= bits; k += 64) {
		u64 v;
		__builtin_memcpy(&v, a + (k >> 3), 8);	/* (may be unaligned) */
		c += __popcll(v);
	}
	if (k < bits) {
		u64 v = 0;
		for (u32 b = 0; 8 * b < bits - k; b++)
			v |= (u64)a[(k >> 3) + b] << (8 * b);
		if (bits - k < 64)
			v &= ((u64)1 << (bits - k)) - 1;
		c += __popcll(v);
	}
	return c;
}

static __device__ __forceinline__ const u8 *
pq_place(u64 at, const u8 *__restrict__ in, const u8 *__restrict__ rooms)
{
	return (at & LDA_PQ_IN_PLACE) ? in + (at & ~LDA_PQ_IN_PLACE) : rooms + at;
}

/*
 * The last i of 0 .. n - 1 with key(i) <= v; key never falls, key(0) <= v and n
 * is at least 1.  Every load of a search waits for the one before, so the
 * search starts where v would stand if the keys were evenly spread over `span`
 * - runs of one length, as writers make them, and pages of one size are - and
 * gallops from there; what is left is bisected.  Two or three loads for even
 * keys, never more than twice a bisection's.
 */
template <typename Key>
static __device__ __forceinline__ u32 pq_search(Key key, u32 n, u64 v, u64 span)
{
	u32 lo = 0, hi = n - 1, step = 1;
	/* (a guess: its rounding does not matter, and v <= span) */
	const double at = span ? (double)v * (double)n / (double)span : 0.0;
	const u32 j = at < (double)hi ? (u32)at : hi;

	if (key(j) <= v) {
		lo = j;
		while (lo < hi) {
			const u32 t = hi - lo > step ? lo + step : hi;
			if (key(t) <= v) {
				lo = t;
				step <<= 1;
			} else {
				hi = t - 1;
				break;
			}
		}
	} else {	/* (j is at least 1) */
		hi = j - 1;
		while (lo < hi) {
			const u32 t = hi - lo >= step ? hi + 1 - step : lo;
			if (key(t) <= v || t == lo) {
				lo = t;
				break;
			}
			hi = t - 1;
			step <<= 1;
		}
	}
	while (lo < hi) {
		const u32 mid = lo + ((hi - lo + 1) >> 1);
		if (key(mid) <= v)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/* the last of the n records (n at least 1, the first starts at 0) that starts
 * at or below v, of `span` values in all */
static __device__ __forceinline__ uint4
pq_find_run(const uint4 *__restrict__ runs, u32 n, u32 v, u32 span)
{
	return runs[pq_search([&](u32 i) { return (u64)runs[i].x; }, n, v, span)];
}

/* the page that holds slot g of all `slots`: the last whose first slot is at or
 * below g (pages without slots have the first slot of the page behind them) */
static __device__ __forceinline__ u32
pq_find_page(const u64 *__restrict__ slot_end, u32 n_u, u64 g, u64 slots)
{
	return pq_search([&](u32 i) { return i ? slot_end[i - 1] : (u64)0; }, n_u, g, slots);
}

/* slot r of the `count` of data page u, which has max_def 1 and inf[PQ_I_LRUNS]
 * level runs, one at least: its level, and its rank among the valid slots */
static __device__ __forceinline__ void
pq_slot_level(u64 n_u, u64 u, u32 r, u32 count, u32 kind, const u64 *__restrict__ ucols,
	      const u8 *__restrict__ in, const u8 *__restrict__ secp, const uint4 *__restrict__ runs,
	      const u32 *__restrict__ inf, u32 &level, u32 &rank)
{
	const uint4 run = pq_find_run(runs + ucols[LDA_PQ_U_LRUNS * n_u + u], inf[PQ_I_LRUNS], r, count);
	const u32 rel = r - run.x;
	if (run.y) {
		const u8 *lev = (kind == LDA_PQ_DATA_V2 ? in + ucols[LDA_PQ_U_LEV * n_u + u] : secp) + run.z;
		level = lev[rel >> 3] >> (rel & 7) & 1;
		rank = run.w + pq_popcount(lev, rel);
	} else {
		level = run.z;
		rank = run.w + (level ? rel : 0);
	}
}

/* the dictionary index of the valid slot of rank `rank` of data page u, which
 * has inf[PQ_I_IRUNS] index runs, one at least */
static __device__ __forceinline__ u32
pq_slot_index(u64 n_u, u64 u, u32 rank, const u64 *__restrict__ ucols, const u8 *__restrict__ secp,
	      const uint4 *__restrict__ runs, const u32 *__restrict__ inf)
{
	const u32 w = inf[PQ_I_W];
	const uint4 run = pq_find_run(runs + ucols[LDA_PQ_U_IRUNS * n_u + u], inf[PQ_I_IRUNS], rank,
				       inf[PQ_I_VALID]);
	if (!run.y)
		return run.z;
	const u64 bit = (u64)(rank - run.x) * w;
	const u8 *a = secp + run.z + (bit >> 3);
	const u32 sh = (u32)bit & 7;
	u64 v = 0;
	for (u32 b = 0; 8 * b < sh + w; b++)
		v |= (u64)a[b] << (8 * b);
	return (u32)(v >> sh & (((u64)1 << w) - 1));
}

#endif /* LDA_PARQUET_DEVICE_H */
