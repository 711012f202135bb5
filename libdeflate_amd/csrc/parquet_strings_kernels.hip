/*
 * parquet_strings_kernels.hip - the BYTE_ARRAY pages of Parquet column chunks
 * turned into int64 offsets and one run of bytes (host_parquet.hip:
 * libdeflate_amd_parquet_decode_batch_ex).  parquet_strings_plan.h builds the
 * columns these kernels read; tools/models/parquet_strings_model.py restates
 * them on the CPU.  They run behind lda_pq_runs_kernel, which has walked the
 * levels and indices of the string pages like those of any other page.
 *
 * lda_pqs_walk_kernel: a wave a section of length-prefixed values (a
 * dictionary page, a PLAIN data page).  It lists where each of the values owed
 * starts and where the last one ends.  The chain next(p) = p + 4 + len(p) is
 * broken up a window of PQS_POS positions at a time: every lane computes next()
 * for its 16 positions as if each were a start, and pointer doubling in LDS -
 * jump <- jump o jump, reach[jump[p]] |= reach[p] - marks what the window's
 * first position reaches, until the chain leaves the window or breaks.  The
 * marked positions, compacted in order, are the starts; the next window opens
 * where the chain left this one.
 *
 * lda_pqs_sum_kernel and lda_pqs_offsets_kernel: tiled over the slots of all
 * string data pages laid end to end, LDA_PQ_TILE slots a workgroup in four rows
 * of 256.  A slot's length is 0 for a null, the difference of two starts less 4
 * for a PLAIN value, the dictionary entry's for an index.  The first finds the
 * lengths - the slot's page, level run, rank and index run, each a search -,
 * leaves each with the slot's source for the copy, writes the validity bytes,
 * which it has at hand, and reduces a tile to one sum; the project's scan places
 * the tiles; the second scans the lengths inside the tile and writes the int64
 * entries and every slot's place.
 *
 * lda_pqs_copy_kernel: tiled over the output bytes, PQS_COPY_TILE a
 * workgroup.  A tile finds the slots that cover it in the places just written,
 * takes places and sources into LDS PQS_COPY_SLOTS at a time, and every thread
 * fills its 16 bytes from the sources under them.
 *
 * lda_pqs_final_kernel adds the walk's and the fit verdicts to what
 * lda_pq_final_kernel left, and writes d_bytes_total.
 *
 * As in parquet_kernels.hip the bytes may be anything: a length is checked
 * against the section's end before it is trusted, a start is written only below
 * the list's capacity, a start is read only below the count the walk reached.
 * Nothing spins and no workgroup waits for another.  Plain C++, vector stores
 * only.
 */
#include "parquet_device.h"

#define PQS_POS 1024			/* positions of a walk window: 64 lanes x 16 */
#define PQS_WIN_BYTES (PQS_POS + 16)	/* their prefixes: 3 bytes more, in loads of 16 */
#define PQS_EXIT PQS_POS		/* jump: the value ends at or behind the window's end */
#define PQS_BAD (PQS_POS + 1)		/* jump: the prefix or the value leaves the section */
#define PQS_ROUNDS 11			/* 257 hops at most: 9 rounds */
#define PQS_COPY_TILE 4096		/* output bytes of a copy tile: 256 threads x 16 */
#define PQS_COPY_SLOTS 1024		/* slots in LDS at a time */

/* the areas: `walks` is [two words per walk section: failed, the values owed]
 * [the start lists], `sums` [the tile sums][their places][the scan's block sums
 * and the total], `places` [every slot's place and the total][every slot's
 * source] */
struct pqs_lds {
	u8 bytes[PQS_WIN_BYTES];
	u16 jump[PQS_WIN_BYTES];
	u8 reach[PQS_WIN_BYTES];
};

/* position i of the window at `at`: does a value start there inside the
 * section, and where does it end */
static __device__ __forceinline__ bool
pqs_next(const pqs_lds &L, u32 at, u32 i, u32 sec_n, u32 &next)
{
	const u32 p = at + i;
	/* two aligned words and a shift: a prefix lies at any byte */
	const u32 *w = (const u32 *)L.bytes + (i >> 2);
	const u32 len = (u32)(((u64)w[1] << 32 | w[0]) >> (8 * (i & 3)));
	if (p > sec_n || sec_n - p < 4 || len > sec_n - p - 4)
		return false;
	next = p + 4 + len;
	return true;
}

/*
 * The starts of the `owed` values from p0 of the section, and the end of the
 * last, listed from starts[0]: 0, or 1 for BAD_DATA.  cap: the words of the
 * list.
 */
static __device__ __forceinline__ u32
pqs_walk(pqs_lds &L, const u8 *__restrict__ sec, u32 sec_n, u32 p0, u32 owed, u32 *__restrict__ starts,
	 u32 cap)
{
	const u32 lane = lane_id();
	u32 done = 0, at = p0;

	if (owed >= cap)
		return 1;	/* more values than the section has room for prefixes */
	while (done < owed) {
		wave_sync();
#pragma unroll
		for (u32 i = 0; i < 2; i++) {
			const u32 o = (i * 64 + lane) * 16;
			if (o < PQS_WIN_BYTES)
				*(uint4 *)(L.bytes + o) = load16_guard(sec, (u64)at + o, sec_n);
		}
		wave_sync();
#pragma unroll
		for (u32 k = 0; k < 16; k++) {
			const u32 i = lane * 16 + k;
			u32 nx = 0;
			const bool ok = pqs_next(L, at, i, sec_n, nx);
			L.jump[i] = (u16)(!ok ? PQS_BAD : nx - at >= PQS_POS ? PQS_EXIT : nx - at);
			L.reach[i] = i == 0;
		}
		if (lane == 0) {
			L.jump[PQS_EXIT] = PQS_EXIT, L.jump[PQS_BAD] = PQS_BAD;
			L.reach[PQS_EXIT] = L.reach[PQS_BAD] = 0;
		}
		wave_sync();
		u32 ended = 0;
		for (u32 round = 0; round < PQS_ROUNDS && !ended; round++) {
			/* every read of a round before any of its writes: a position marked
			 * in this round must not mark its successor in the same round, or the
			 * exit could be reached over a gap */
			u32 hops[16], from = 0;	/* the hop, and the hop of the hop << 16 */
#pragma unroll
			for (u32 k = 0; k < 16; k++) {
				const u32 i = lane * 16 + k, j = L.jump[i];
				hops[k] = j | (u32)L.jump[j] << 16;
				from |= (u32)(L.reach[i] != 0) << k;
			}
			wave_sync();
#pragma unroll
			for (u32 k = 0; k < 16; k++) {
				if (from >> k & 1)
					L.reach[hops[k] & 0xFFFF] = 1;
				L.jump[lane * 16 + k] = (u16)(hops[k] >> 16);
			}
			wave_sync();
			ended = bcast_first((u32)L.reach[PQS_EXIT] | L.reach[PQS_BAD]);
		}
		if (!ended)
			return 1;	/* (cannot be: 9 rounds cover the 257 hops a window holds) */
		/* the marked positions in order: all are starts but a last one whose
		 * value breaks */
		u32 marked = 0, good = 0, nmax = 0;
#pragma unroll
		for (u32 k = 0; k < 16; k++) {
			const u32 i = lane * 16 + k;
			u32 nx = 0;
			if (L.reach[i]) {
				marked |= 1u << k;
				if (pqs_next(L, at, i, sec_n, nx)) {
					good |= 1u << k;
					nmax = nx > nmax ? nx : nmax;
				}
			}
		}
		const u32 incl = wave_scan_incl(__popc(marked));
		const u32 n_marked = bcast_lane(incl, 63), n_good = wave_sum(__popc(good));
		const u32 rem = owed - done, take = rem < n_good ? rem : n_good;
		u32 ord = incl - __popc(marked), cand = 0;
#pragma unroll
		for (u32 k = 0; k < 16; k++) {
			if (marked >> k & 1) {
				if (ord < take)
					starts[done + ord] = at + lane * 16 + k;
				if (ord == take)
					cand = at + lane * 16 + k;
				ord++;
			}
		}
		if (rem > n_good && bcast_first((u32)L.reach[PQS_BAD]))
			return 1;	/* the chain breaks before the values owed */
		/* where the chain stands now: the marked position behind the ones
		 * taken, or where the last one's value ends */
		at = bcast_first(take < n_marked ? wave_max(cand) : wave_max(nmax));
		done += take;
	}
	if (lane == 0)
		starts[owed] = at;
	return 0;
}

extern "C" __global__ void __launch_bounds__(256)
lda_pqs_walk_kernel(uint64_t n_w, const uint64_t *__restrict__ wcols, const int32_t *__restrict__ decode,
		    const uint32_t *__restrict__ info, const uint8_t *__restrict__ in,
		    const uint8_t *__restrict__ rooms, uint32_t *__restrict__ walks)
{
	__shared__ __attribute__((aligned(16))) pqs_lds lds[4];
	const u32 wave = bcast_first(threadIdx.x >> 6), lane = lane_id();

	for (u64 k = (u64)blockIdx.x * 4 + wave; k < n_w; k += (u64)gridDim.x * 4) {
		const u32 z = (u32)wcols[LDA_PQS_W_Z * n_w + k], u1 = (u32)wcols[LDA_PQS_W_U * n_w + k];
		u32 status = 0, owed = (u32)wcols[LDA_PQS_W_COUNT * n_w + k], p0 = 0;

		if (z && decode[z - 1] != 0) {
			status = 1;
		} else if (u1) {	/* a data page: what the level walk found */
			const u32 *inf = info + LDA_PQ_INFO_WORDS * (u64)(u1 - 1);
			status = inf[PQ_I_STATUS] != 0;
			owed = inf[PQ_I_VALID];
			p0 = inf[PQ_I_VAL_AT];
		}
		if (!status)
			status = pqs_walk(lds[wave], pq_place(wcols[LDA_PQS_W_SEC * n_w + k], in, rooms),
					  (u32)wcols[LDA_PQS_W_SEC_N * n_w + k], bcast_first(p0),
					  bcast_first(owed), walks + wcols[LDA_PQS_W_STARTS * n_w + k],
					  (u32)wcols[LDA_PQS_W_CAP * n_w + k]);
		if (lane == 0)
			walks[2 * k] = status, walks[2 * k + 1] = owed;
	}
}

/* what the sum and offsets kernels read of a call */
struct pqs_args {
	u64 n_u, n_s;
	const u64 *ucols, *scols;
	const u8 *in, *rooms;
	const uint4 *runs;
	u32 *info;
	const u32 *walks;
};

/* slot r of the `count` of string data page s: its level, its length and
 * where its bytes lie (as LDA_PQ_U_SEC).  A page that failed has lengths of 0;
 * an index at or above the entry count is flagged and counts as 0 */
static __device__ __forceinline__ void
pqs_slot(const pqs_args &a, u64 s, u32 r, u32 count, u32 &level, u64 &len, u64 &src)
{
	const u64 n_u = a.n_u, u = a.scols[LDA_PQS_S_U * a.n_s + s];
	const u64 k = a.scols[LDA_PQS_S_WALK * a.n_s + s];
	const u32 *inf = a.info + LDA_PQ_INFO_WORDS * u;

	level = 0, len = 0, src = 0;
	if (inf[PQ_I_STATUS])
		return;
	const u64 fields = a.ucols[LDA_PQ_U_FIELDS * n_u + u];
	const u32 kind = (u32)fields & 15, enc = (u32)fields >> 4 & 255, max_def = (u32)fields >> 13 & 1;
	const u8 *secp = pq_place(a.ucols[LDA_PQ_U_SEC * n_u + u], a.in, a.rooms);
	u32 rank = r;

	level = 1;
	if (max_def) {
		if (!inf[PQ_I_LRUNS]) {
			level = 0;
			return;
		}
		pq_slot_level(n_u, u, r, count, kind, a.ucols, a.in, secp, a.runs, inf, level, rank);
	}
	if (!level || a.walks[2 * k])
		return;
	const u32 *st = a.walks + a.scols[LDA_PQS_S_STARTS * a.n_s + s];
	u64 base = a.ucols[LDA_PQ_U_SEC * n_u + u];
	u32 at = rank;
	if (enc != LDA_PQ_PLAIN) {
		if (!inf[PQ_I_IRUNS])
			return;
		at = pq_slot_index(n_u, u, rank, a.ucols, secp, a.runs, inf);
		if (at >= (u32)a.ucols[LDA_PQ_U_DICT_N * n_u + u]) {
			atomicOr(a.info + LDA_PQ_INFO_WORDS * u + PQ_I_INDEX_BAD, 1u);
			return;
		}
		base = a.ucols[LDA_PQ_U_DICT * n_u + u];
	}
	len = st[at + 1] - st[at] - 4;
	src = base + st[at] + 4;
}

/*
 * The lengths.  Tile t holds four rows of 256 consecutive string slots, a slot
 * a thread: the slot's length goes to places[g] and its source behind the
 * places, its validity byte - which needs no place - to d_valid, and the tile's
 * sum to sums[t].
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pqs_sum_kernel(uint64_t n_u, uint64_t n_s, uint64_t n_tiles,
		   const uint64_t *__restrict__ ucols, const uint64_t *__restrict__ scols,
		   const uint8_t *__restrict__ in, const uint8_t *__restrict__ rooms,
		   const uint4 *__restrict__ runs, uint32_t *__restrict__ info,
		   const uint32_t *__restrict__ walks, uint64_t *__restrict__ sums,
		   uint8_t *__restrict__ valid, uint64_t *__restrict__ places)
{
	__shared__ u64 wsum[4];
	const pqs_args a = { n_u, n_s, ucols, scols, in, rooms, runs, info, walks };
	const u64 *slot_end = scols + LDA_PQS_S_SLOT_END * n_s;
	const u64 slots = slot_end[n_s - 1];

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		u64 mine = 0;
#pragma unroll 1
		for (u32 k = 0; k < LDA_PQ_TILE / 256; k++) {
			const u64 g = t * LDA_PQ_TILE + k * 256 + threadIdx.x;
			if (g >= slots)
				break;
			const u32 s = pq_find_page(slot_end, (u32)n_s, g, slots);
			const u64 first = s ? slot_end[s - 1] : 0, u = scols[LDA_PQS_S_U * n_s + s];
			u64 len, src;
			u32 level;

			pqs_slot(a, s, (u32)(g - first), (u32)(slot_end[s] - first), level, len, src);
			if ((ucols[LDA_PQ_U_FIELDS * n_u + u] >> 13 & 1) &&
			    !info[LDA_PQ_INFO_WORDS * u + PQ_I_STATUS])
				valid[ucols[LDA_PQ_U_VALID * n_u + u] + g - first] = (u8)level;
			places[g] = len;
			places[slots + 1 + g] = src;
			mine += len;
		}
		const u64 sum = wave_sum64(mine);
		if ((threadIdx.x & 63) == 0)
			wsum[threadIdx.x >> 6] = sum;
		__syncthreads();
		if (threadIdx.x == 0)
			sums[t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
		__syncthreads();	/* (wsum is free for the next tile) */
	}
}

/*
 * The places.  The same tiles: every row's lengths are scanned from where the
 * tile, and then the row before, ended - the scan has placed the tiles -, the
 * slot's place replaces its length in places[g], and goes to the page's int64
 * entries; the last slot of a page writes the page's entry `count` too, the
 * last slot of all the total, places[slots].
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pqs_offsets_kernel(uint64_t n_u, uint64_t n_s, uint64_t n_tiles,
		       const uint64_t *__restrict__ ucols, const uint64_t *__restrict__ scols,
		       const uint64_t *__restrict__ sums, uint8_t *__restrict__ out,
		       uint64_t *__restrict__ places)
{
	__shared__ u64 wsum[4];
	const u64 *slot_end = scols + LDA_PQS_S_SLOT_END * n_s;
	const u64 slots = slot_end[n_s - 1];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		u64 base = sums[n_tiles + t] + sums[2 * n_tiles + t / LDA_SCAN_BLOCK];
#pragma unroll 1
		for (u32 k = 0; k < LDA_PQ_TILE / 256; k++) {
			const u64 g = t * LDA_PQ_TILE + k * 256 + threadIdx.x;
			const u64 len = g < slots ? places[g] : 0;
			const u64 incl = wave_scan_incl64(len);
			if (lane == 63)
				wsum[wave] = incl;
			__syncthreads();
			u64 pos = base + incl - len;
#pragma unroll
			for (u32 w = 0; w < 4; w++) {
				const u64 v = wsum[w];
				if (w < wave)
					pos += v;
				base += v;
			}
			__syncthreads();	/* (wsum is free for the next row) */
			if (g < slots) {
				const u32 s = pq_find_page(slot_end, (u32)n_s, g, slots);
				const u64 first = s ? slot_end[s - 1] : 0, u = scols[LDA_PQS_S_U * n_s + s];
				const u64 end = pos + len;
				u8 *o = out + ucols[LDA_PQ_U_OUT * n_u + u] + 8 * (g - first);

				__builtin_memcpy(o, &pos, 8);
				if (g + 1 == slot_end[s])
					__builtin_memcpy(o + 8, &end, 8);
				places[g] = pos;
				if (g + 1 == slots)
					places[slots] = end;
			}
		}
	}
}

/* where string data page s ends in d_bytes: the place of the slot behind it */
static __device__ __forceinline__ u64
pqs_page_end(const u64 *__restrict__ slot_end, const u64 *__restrict__ ent, u64 s)
{
	return ent[slot_end[s]];
}

/* the last i of 0 .. n - 1 with a[i] <= v; a never falls, a[0] <= v, n at least 1 */
static __device__ __forceinline__ u64 pqs_last_le(const u64 *__restrict__ a, u64 n, u64 v)
{
	u64 lo = 0, hi = n - 1;
	while (lo < hi) {
		const u64 mid = lo + ((hi - lo + 1) >> 1);
		if (a[mid] <= v)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/*
 * The bytes of the pages that fit.  Pages lie in d_bytes in the order of their
 * ends, so the ones that fit are the bytes below `limit`, the end of the last
 * page that ends at or below bytes_avail.  ent[g] is where slot g starts
 * (ent[slots]: the total), srcs[g] where its bytes lie: `places`.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pqs_copy_kernel(uint64_t n_s, const uint64_t *__restrict__ scols, const uint64_t *__restrict__ places,
		    const uint8_t *__restrict__ in, const uint8_t *__restrict__ rooms,
		    uint8_t *__restrict__ bytes, uint64_t bytes_avail)
{
	__shared__ u64 e[PQS_COPY_SLOTS + 1], sp[PQS_COPY_SLOTS];
	const u64 *slot_end = scols + LDA_PQS_S_SLOT_END * n_s;
	const u64 slots = slot_end[n_s - 1];
	const u64 *ent = places, *srcs = places + slots + 1;
	const u32 tid = threadIdx.x;
	/* key(i): the end of page i - 1 */
	const u32 fit = pq_search([&](u32 i) { return i ? pqs_page_end(slot_end, ent, i - 1) : (u64)0; },
				  (u32)n_s + 1, bytes_avail, ent[slots]);
	const u64 limit = fit ? pqs_page_end(slot_end, ent, fit - 1) : 0;
	const u64 n_tiles = (limit + PQS_COPY_TILE - 1) / PQS_COPY_TILE;

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 b0 = t * PQS_COPY_TILE;
		const u64 b1 = b0 + PQS_COPY_TILE < limit ? b0 + PQS_COPY_TILE : limit;
		/* the slots that hold bytes b0 and b1 - 1: both below ent[slots] */
		const u64 g_hi = pqs_last_le(ent, slots, b1 - 1);
		const u64 o = b0 + 16 * tid;

		for (u64 g = pqs_last_le(ent, slots, b0); g <= g_hi; g += PQS_COPY_SLOTS) {
			const u32 n = g_hi - g + 1 < PQS_COPY_SLOTS ? (u32)(g_hi - g + 1) : PQS_COPY_SLOTS;
			for (u32 i = tid; i <= n; i += 256) {
				e[i] = ent[g + i];
				if (i < n)
					sp[i] = srcs[g + i];
			}
			__syncthreads();
			/* what of this thread's 16 bytes these n slots hold */
			const u64 lo = b0 > e[0] ? b0 : e[0], hi = b1 < e[n] ? b1 : e[n];
			u64 p = o > lo ? o : lo;
			const u64 pe = o + 16 < hi ? o + 16 : hi;
			if (p < pe) {
				u32 i = 0, j = n - 1;	/* the last slot that starts at or below p */
				while (i < j) {
					const u32 mid = i + ((j - i + 1) >> 1);
					if (e[mid] <= p)
						i = mid;
					else
						j = mid - 1;
				}
				if (pe - p == 16 && e[i + 1] >= pe) {
					uint4 v;
					__builtin_memcpy(&v, pq_place(sp[i], in, rooms) + (p - e[i]), 16);
					__builtin_memcpy(bytes + p, &v, 16);
				} else {
					while (p < pe) {
						while (e[i + 1] <= p)	/* (e[n] >= hi > p) */
							i++;
						const u64 seg = e[i + 1] < pe ? e[i + 1] : pe;
						const u8 *src = pq_place(sp[i], in, rooms) + (p - e[i]);
						for (; p < seg; p++)
							bytes[p] = *src++;
					}
				}
			}
			__syncthreads();
		}
	}
}

/*
 * Behind lda_pq_final_kernel, which has merged what the old call knows into
 * results: a row that it left as SUCCESS is BAD_DATA where its own walk or its
 * dictionary's failed, and INSUFFICIENT_SPACE where its bytes do not end at or
 * below bytes_avail.  A string data page without slots gets its one entry
 * here; bytes_total[0] is the total.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_pqs_final_kernel(uint64_t n, uint64_t n_u, uint64_t n_s, const uint64_t *__restrict__ svcols,
		     const uint64_t *__restrict__ ucols, const uint64_t *__restrict__ scols,
		     const uint32_t *__restrict__ winfo, const uint64_t *__restrict__ ent,
		     const uint64_t *__restrict__ total, uint64_t bytes_avail, uint8_t *__restrict__ out,
		     uint64_t *__restrict__ bytes_total, int32_t *__restrict__ results)
{	/* (winfo: the front of `walks`; ent: the front of `places`) */
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r == 0 && bytes_total)
		bytes_total[0] = total[0];
	if (r >= n)
		return;
	const u64 s1 = svcols[LDA_PQS_V_S * n + r], w1 = svcols[LDA_PQS_V_WALK * n + r];
	const u64 d1 = svcols[LDA_PQS_V_DWALK * n + r];
	if (!s1 && !w1)
		return;
	s32 res = results[r];
	u64 end = 0;
	if (s1) {
		const u64 *slot_end = scols + LDA_PQS_S_SLOT_END * n_s;
		const u64 first = s1 > 1 ? slot_end[s1 - 2] : 0;
		end = slot_end[n_s - 1] ? pqs_page_end(slot_end, ent, s1 - 1) : 0;
		if (first == slot_end[s1 - 1]) {	/* no slot: entry 0 alone */
			const u64 u = scols[LDA_PQS_S_U * n_s + s1 - 1];
			__builtin_memcpy(out + ucols[LDA_PQ_U_OUT * n_u + u], &end, 8);
		}
	}
	if (res == LDA_SUCCESS) {
		if ((w1 && winfo[2 * (w1 - 1)]) || (d1 && winfo[2 * (d1 - 1)]))
			res = LDA_BAD_DATA;
		else if (s1 && end > bytes_avail)
			res = LDA_INSUFFICIENT_SPACE;
		results[r] = res;
	}
}
