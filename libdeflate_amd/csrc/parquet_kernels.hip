/*
 * parquet_kernels.hip - the pages of flat Parquet column chunks turned into
 * columns in device memory (host_parquet.hip:
 * libdeflate_amd_parquet_decode_batch).  parquet_plan.h builds the columns these
 * kernels read; tools/models/parquet_model.py restates them on the CPU.
 *
 * lda_pq_runs_kernel: a wave a data page.  It walks the page's RLE / bit-packed
 * hybrid streams, the definition levels and then the dictionary indices, one
 * step per run, and lists the runs.  The stream is staged through LDS a window
 * of PQ_WIN bytes at a time, so that a hop reads LDS; every lane takes the same
 * steps.  A bit-packed run of levels is listed in pieces of LDA_PQ_LEVEL_PIECE
 * values, a lane a piece, each with the count of valid slots in front of it.
 * It checks everything about the page that is not a single index, and leaves
 * LDA_PQ_INFO_WORDS words per page.
 *
 * lda_pq_expand_kernel: tiled over the slots of all data pages laid end to end,
 * LDA_PQ_TILE slots a workgroup.  A slot finds its page and its level run by
 * a search that starts where pages and runs of one length would put it
 * (pq_search), ranks itself among the valid slots - the run's base plus a
 * popcount -, finds its index run the same way, fetches the PLAIN value or the
 * dictionary entry and writes the slot and its validity byte.
 *
 * lda_pq_final_kernel merges the verdicts.
 *
 * parquet_device.h holds what the BYTE_ARRAY kernels share with these
 * (parquet_strings_kernels.hip): the window, the searches, a slot's level, rank
 * and index.
 *
 * The kernels also run over pages whose bytes are anything.  A page whose
 * inflate failed is not walked; of any other every address is checked against
 * the plan's sizes before it is used: a run record is written only below the
 * list's capacity, a level or index is read only inside the bytes the walk has
 * checked, and a dictionary entry only below the entry count.  Nothing spins
 * and no workgroup waits for another.  Plain C++, vector stores only.
 */
#include "parquet_device.h"

/*
 * The runs of the stream of bit width w in [p, len) that owes `owed` values,
 * listed from runs[0]: 0, or 1 for BAD_DATA.  A record is {the first value of
 * the run, 1 for bit-packed, the RLE value or the offset of the packed bytes,
 * LEVELS: the valid slots in front}.
 */
template <bool LEVELS>
static __device__ __forceinline__ u32
pq_walk(pq_win &win, u32 p, u32 len, u32 w, u32 owed, uint4 *__restrict__ runs, u32 cap,
	u32 &n_runs, u32 &n_valid)
{
	const u32 lane = lane_id(), vb = (w + 7) / 8;
	u32 done = 0, nr = 0, valid = 0;

	while (done < owed) {
		u64 h = 0;
		for (u32 k = 0;; k++) {
			if (k == 5 || p >= len)
				return 1;	/* a sixth header byte, or the stream ends */
			const u32 b = win_byte(win, p++);
			h |= (u64)(b & 0x7F) << (7 * k);
			if (!(b & 0x80))
				break;
		}
		const u64 cnt = h >> 1;		/* below 2^34 */
		if (!cnt)
			return 1;
		if (h & 1) {
			const u64 vals = cnt * 8;
			const u32 take = vals < owed - done ? (u32)vals : owed - done;
			const u64 need = ((u64)take * w + 7) / 8;
			if (need > len - p)
				return 1;
			if (LEVELS) {
				const u32 pieces = (take + LDA_PQ_LEVEL_PIECE - 1) / LDA_PQ_LEVEL_PIECE;
				if (pieces > cap - nr)
					return 1;
				if (pieces == 1) {
					/* the common run, pyarrow's 63 groups among them: its 64
					 * bytes at most are counted out of the window, a lane a byte */
					const u32 pu = bcast_first(p);
					if (pu - win.at > PQ_WIN - 64)
						win_load(win, pu);
					u32 b = lane < (u32)need ? win.lds[pu - win.at + lane] : 0;
					if (lane == (u32)need - 1 && (take & 7))
						b &= (1u << (take & 7)) - 1;
					const u32 c = wave_sum(__popc(b));
					if (lane == 0)
						runs[nr] = make_uint4(done, 1, p, valid);
					valid += c;
				}
				for (u32 k0 = 0; pieces > 1 && k0 < pieces; k0 += 64) {
					const u32 s = k0 + lane, first = s * LDA_PQ_LEVEL_PIECE;
					u32 c = 0;
					if (s < pieces) {
						const u32 left = take - first;
						c = pq_popcount(win.base + p + first / 8,
								left < LDA_PQ_LEVEL_PIECE ? left : LDA_PQ_LEVEL_PIECE);
					}
					const u32 incl = wave_scan_incl(c);
					if (s < pieces)
						runs[nr + s] = make_uint4(done + first, 1, p + first / 8,
									  valid + incl - c);
					valid += bcast_lane(incl, 63);
				}
				nr += pieces;
			} else {
				if (nr >= cap)
					return 1;
				if (lane == 0)
					runs[nr] = make_uint4(done, 1, p, 0);
				nr++;
			}
			done += take;
			const u64 bytes = cnt * w;
			p += bytes < len - p ? (u32)bytes : len - p;
		} else {
			if (vb > len - p)
				return 1;
			u32 val = 0;
			for (u32 k = 0; k < vb; k++)
				val |= win_byte(win, p + k) << (8 * k);
			p += vb;
			if (LEVELS && val > 1)
				return 1;
			if (nr >= cap)
				return 1;
			const u32 take = cnt < owed - done ? (u32)cnt : owed - done;
			if (lane == 0)
				runs[nr] = make_uint4(done, 0, val, valid);
			nr++;
			if (LEVELS && val)
				valid += take;
			done += take;
		}
	}
	n_runs = nr;
	n_valid = valid;
	return 0;
}

extern "C" __global__ void __launch_bounds__(256)
lda_pq_runs_kernel(uint64_t n_u, const uint64_t *__restrict__ ucols,
		   const int32_t *__restrict__ decode, const uint8_t *__restrict__ in,
		   const uint8_t *__restrict__ rooms, uint4 *__restrict__ runs,
		   uint32_t *__restrict__ info)
{
	__shared__ __attribute__((aligned(16))) u8 lds[4][PQ_WIN];
	const u32 wave = bcast_first(threadIdx.x >> 6), lane = lane_id();
	pq_win win;

	win.lds = lds[wave];
	for (u64 u = (u64)blockIdx.x * 4 + wave; u < n_u; u += (u64)gridDim.x * 4) {
		const u64 fields = ucols[LDA_PQ_U_FIELDS * n_u + u], sec = ucols[LDA_PQ_U_SEC * n_u + u];
		const u32 sec_n = (u32)ucols[LDA_PQ_U_SEC_N * n_u + u];
		const u32 count = (u32)ucols[LDA_PQ_U_COUNT * n_u + u];
		const u32 z = (u32)(fields >> 32), kind = (u32)fields & 15, enc = (u32)fields >> 4 & 255;
		const u32 max_def = (u32)fields >> 13 & 1, width = ((u32)fields >> 16 & 255) + 1;
		u32 status = 0, n_lr = 0, n_ir = 0, n_valid = count, val_at = 0, w = 0, none = 0;

		if ((fields & LDA_PQ_F_SKIP) || (z && decode[z - 1] != 0)) {
			status = 1;
		} else {
			const u8 *secp = pq_place(sec, in, rooms);
			if (max_def) {
				u32 p = 0, len = 0;
				if (kind == LDA_PQ_DATA_V2) {
					len = (u32)ucols[LDA_PQ_U_LEV_N * n_u + u];
					win_open(win, in + ucols[LDA_PQ_U_LEV * n_u + u], len);
				} else {
					win_open(win, secp, sec_n);
					u32 l = 0;
					for (u32 k = 0; k < 4; k++)	/* (bytes behind sec_n read as 0) */
						l |= win_byte(win, k) << (8 * k);
					if (sec_n < 4 || l > sec_n - 4)
						status = 1;	/* the length prefix leaves the page */
					p = 4, len = val_at = 4 + l;
				}
				if (!status)
					status = pq_walk<true>(win, p, len, 1, count,
							       runs + ucols[LDA_PQ_U_LRUNS * n_u + u],
							       (u32)ucols[LDA_PQ_U_LCAP * n_u + u], n_lr, n_valid);
			}
			if (!status && enc != LDA_PQ_PLAIN) {
				if (n_valid) {	/* (no valid slot: no index, and no width byte is asked for) */
					win_open(win, secp, sec_n);
					if (val_at >= sec_n)
						status = 1;
					else if ((w = win_byte(win, val_at)) > 32)
						status = 1;
					else
						status = pq_walk<false>(win, val_at + 1, sec_n, w, n_valid,
									runs + ucols[LDA_PQ_U_IRUNS * n_u + u],
									(u32)ucols[LDA_PQ_U_ICAP * n_u + u], n_ir,
									none);
				}
			} else if (!status && (u64)n_valid * width > sec_n - val_at) {
				status = 1;	/* a short PLAIN section */
			}
		}
		if (lane == 0) {
			u32 *o = info + LDA_PQ_INFO_WORDS * u;
			o[PQ_I_STATUS] = status, o[PQ_I_INDEX_BAD] = 0, o[PQ_I_LRUNS] = n_lr;
			o[PQ_I_IRUNS] = n_ir, o[PQ_I_VALID] = n_valid, o[PQ_I_VAL_AT] = val_at;
			o[PQ_I_W] = w, o[7] = 0;
		}
	}
}

/* width bytes src -> dst, or zeros where src is NULL; either may be unaligned */
static __device__ __forceinline__ void pq_put(u8 *__restrict__ dst, const u8 *__restrict__ src, u32 width)
{
	if (width == 4) {
		u32 v = 0;
		if (src)
			__builtin_memcpy(&v, src, 4);
		__builtin_memcpy(dst, &v, 4);
	} else if (width == 8) {
		u64 v = 0;
		if (src)
			__builtin_memcpy(&v, src, 8);
		__builtin_memcpy(dst, &v, 8);
	} else {
		u32 k = 0;
		for (; k + 4 <= width; k += 4) {
			u32 v = 0;
			if (src)
				__builtin_memcpy(&v, src + k, 4);
			__builtin_memcpy(dst + k, &v, 4);
		}
		for (; k < width; k++)
			dst[k] = src ? src[k] : 0;
	}
}

/* slot r of data page u */
static __device__ __forceinline__ void
pq_slot(u64 n_u, u64 u, u32 r, u32 count, const u64 *__restrict__ ucols, const u8 *__restrict__ in,
	const u8 *__restrict__ rooms, const uint4 *__restrict__ runs, u32 *__restrict__ info,
	u8 *__restrict__ out, u8 *__restrict__ valid)
{
	const u32 *inf = info + LDA_PQ_INFO_WORDS * u;
	if (inf[PQ_I_STATUS])
		return;
	const u64 fields = ucols[LDA_PQ_U_FIELDS * n_u + u];
	const u32 kind = (u32)fields & 15, enc = (u32)fields >> 4 & 255;
	const u32 max_def = (u32)fields >> 13 & 1, width = ((u32)fields >> 16 & 255) + 1;
	const u8 *secp = pq_place(ucols[LDA_PQ_U_SEC * n_u + u], in, rooms);
	u32 level = 1, rank = r;

	if (max_def) {
		if (!inf[PQ_I_LRUNS])
			return;
		pq_slot_level(n_u, u, r, count, kind, ucols, in, secp, runs, inf, level, rank);
		valid[ucols[LDA_PQ_U_VALID * n_u + u] + r] = (u8)level;
	}
	u8 *dst = out + ucols[LDA_PQ_U_OUT * n_u + u] + (u64)r * width;
	const u8 *src = NULL;
	if (level) {
		if (enc == LDA_PQ_PLAIN) {
			src = secp + inf[PQ_I_VAL_AT] + (u64)rank * width;
		} else {
			if (!inf[PQ_I_IRUNS])
				return;
			const u32 idx = pq_slot_index(n_u, u, rank, ucols, secp, runs, inf);
			if (idx >= (u32)ucols[LDA_PQ_U_DICT_N * n_u + u]) {
				atomicOr(info + LDA_PQ_INFO_WORDS * u + PQ_I_INDEX_BAD, 1u);
				return;
			}
			src = pq_place(ucols[LDA_PQ_U_DICT * n_u + u], in, rooms) + (u64)idx * width;
		}
	}
	pq_put(dst, src, width);
}

extern "C" __global__ void __launch_bounds__(256)
lda_pq_expand_kernel(uint64_t n_u, uint64_t n_tiles, const uint64_t *__restrict__ ucols,
		     const uint8_t *__restrict__ in, const uint8_t *__restrict__ rooms,
		     const uint4 *__restrict__ runs, uint32_t *__restrict__ info,
		     uint8_t *__restrict__ out, uint8_t *__restrict__ valid)
{
	const u64 *slot_end = ucols + LDA_PQ_U_SLOT_END * n_u;
	const u64 slots = slot_end[n_u - 1];

	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 g0 = t * LDA_PQ_TILE;
		const u64 g1 = g0 + LDA_PQ_TILE < slots ? g0 + LDA_PQ_TILE : slots;
		for (u64 g = g0 + threadIdx.x; g < g1; g += 256) {
			const u64 u = pq_find_page(slot_end, (u32)n_u, g, slots);
			const u64 start = u ? slot_end[u - 1] : 0;
			pq_slot(n_u, u, (u32)(g - start), (u32)(slot_end[u] - start), ucols, in, rooms, runs,
				info, out, valid);
		}
	}
}

/* does row j, a dictionary page, fail? */
static __device__ __forceinline__ bool
pq_dict_fails(u64 n, u64 j, const u64 *__restrict__ vcols, const s32 *__restrict__ decode)
{
	const u64 z = vcols[LDA_PQ_V_Z * n + j];
	return (z && decode[z - 1] != 0) || (vcols[LDA_PQ_V_OWN * n + j] & 0xFF);
}

/* the verdict of every row: the decoder's for its section where that is not
 * success; else a dictionary page's own, BAD_DATA for a data page whose
 * dictionary fails, and what the walk and the expand kernel found */
extern "C" __global__ void __launch_bounds__(256)
lda_pq_final_kernel(uint64_t n, const uint64_t *__restrict__ vcols,
		    const int32_t *__restrict__ decode, const uint32_t *__restrict__ info,
		    int32_t *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= n)
		return;
	const u64 z = vcols[LDA_PQ_V_Z * n + r], own = vcols[LDA_PQ_V_OWN * n + r];
	const u64 dict = vcols[LDA_PQ_V_DICT * n + r];
	s32 res;
	if (z && decode[z - 1] != 0)
		res = decode[z - 1];
	else if (own & LDA_PQ_V_IS_DICT)
		res = (s32)(own & 0xFF);
	else if (dict && pq_dict_fails(n, dict - 1, vcols, decode))
		res = LDA_BAD_DATA;
	else
		res = (info[LDA_PQ_INFO_WORDS * own + PQ_I_STATUS] |
		       info[LDA_PQ_INFO_WORDS * own + PQ_I_INDEX_BAD]) ? LDA_BAD_DATA : LDA_SUCCESS;
	results[r] = res;
}
