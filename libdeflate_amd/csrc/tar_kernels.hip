/*
 * tar_kernels.hip - reading a tar archive that lies in device memory: where
 * its records are, which of them are entries and what they are called, the
 * index rows, one gather copy that puts every entry's bytes at its place, the
 * archive's result words and per-entry results (host_tar.hip;
 * tools/models/tar_walk.py is the CPU model of the whole rule, and the tests
 * run it on the same files).  What an archive is: include/libdeflate_amd.h.
 *
 *   lda_tar_scan_kernel     lda_bgzf_scan_kernel's shape in blocks of 512
 *                           bytes: one workgroup per 32 blocks.  A lane per
 *                           block reads the 8 bytes of the checksum field (one
 *                           sector of a data block); a block whose field holds
 *                           an octal number is summed by the 64 lanes of a
 *                           wave, 8 bytes each, and the rest of the header
 *                           rule follows.  A CANDIDATE is (position, 1 + data
 *                           blocks), both in blocks - a file's data may carry
 *                           headers, a tar inside a tar does - and a candidate
 *                           whose record ends at the file's end or in front of
 *                           an all-zero block is given the size that ends it
 *                           at nb, the one end the host knows.
 *   lda_bgzf_jump_kernel / lda_bgzf_top_kernel / lda_bgzf_members_kernel
 *                           (bgzf_read_kernels.hip, launched by host_finder.h)
 *                           keep the candidates that the chain from block 0
 *                           reaches.
 *   lda_tar_walk_kernel     the serial walk from block 0: what runs instead of
 *                           the two above when LDA_TAR_SERIAL asks.
 *   lda_tar_resolve_kernel  one THREAD per chain record: a record's own fields
 *                           are four short reads of one header, and the look
 *                           back over at most 8 extension records, the search
 *                           for a NUL and the pax parse are serial by nature,
 *                           so a wave per record would idle 63 lanes; records
 *                           with extension records are few, and what one
 *                           thread reads of them is bounded by 1 MiB each.
 *                           Seven words of the entry's row, its pre-extract
 *                           result, its room; the scans of compact_kernels.hip
 *                           then number the entries among the records.
 *   lda_tar_desc_kernel     behind the scans: the row at the entry's number
 *                           with out_off, the per-entry result, and the copy's
 *                           descriptor and tile count per record.
 *   lda_tar_copy_kernel     the gather: every entry cut into tiles of 64 KiB,
 *                           a grid the host sized strides over the tiles, a
 *                           workgroup finds its tile's entry by binary search
 *                           in the prefix sum of the tile counts.
 *   lda_tar_final_kernel    one workgroup: the verdict and the five words.
 *
 * The input is hostile by definition: every block read lies below nb, every
 * record of the chain was bounded by the scan (pos + 1 + d <= nb), every index
 * is checked against the candidate and record counts, and no loop takes an
 * unbounded count from the file.
 */
#include "device_common.h"
#include "kernels.h"
#include "tar_copy.h"	/* copy_tile(): the gather's copy, shared with the writer */

#define BLOCK 512u
#define SIZE_LIMIT ((u64)1 << 36)
#define NO_FIELD 0xFFFFFFFFu

/* leading spaces, octal digits, then the field's end, a NUL or a space */
static __device__ __forceinline__ bool oct_field(const u8 *p, u32 n, u64 *val, u32 *digits)
{
	u32 i = 0, d = 0;
	u64 v = 0;

	while (i < n && p[i] == 0x20)
		i++;
	while (i < n && (u32)(p[i] - 0x30) < 8) {
		v = v * 8 + (p[i] - 0x30);
		i++;
		d++;
	}
	*val = v;
	*digits = d;
	return i == n || p[i] == 0 || p[i] == 0x20;
}

/* the size field of the header h; a base-256 number that does not fit 64 bits
 * reads as 2^64 - 1, which no caller accepts */
static __device__ __forceinline__ bool hdr_size(const u8 *h, u64 *size)
{
	const u8 *f = h + 124;
	u32 digits;

	if (f[0] == 0x80) {
		u64 v = 0;
		for (u32 i = 4; i < 12; i++)
			v = v << 8 | f[i];
		*size = f[1] | f[2] | f[3] ? ~(u64)0 : v;
		return true;
	}
	if (f[0] & 0x80)
		return false;
	return oct_field(f, 12, size, &digits);
}

static __device__ __forceinline__ bool is_ext(u32 t)
{
	return t == 'L' || t == 'K' || t == 'x' || t == 'X' || t == 'g';
}

/* data blocks of a record from its type and its size field */
static __device__ __forceinline__ u64 data_blocks(u32 t, u64 size)
{
	return t >= '1' && t <= '6' ? 0 : (size + BLOCK - 1) / BLOCK;
}

static __device__ __forceinline__ u32 strnlen_dev(const u8 *p, u32 n)
{
	u32 i = 0;
	while (i < n && p[i])
		i++;
	return i;
}

static __device__ __forceinline__ u32 records_of(const u32 *__restrict__ state)
{
	return state[LDA_TAR_ZERO0] ? 0 : state[LDA_BR_MEMBERS];
}

/* verdicts 2 to 4 of include/libdeflate_amd.h, in their order */
static __device__ __forceinline__ u32
find_status(const u32 *__restrict__ state, u64 K, u64 cap, u64 max_records)
{
	if (K > cap)
		return LDA_TAR_MORE_CANDIDATES;
	if (state[LDA_TAR_ZERO0])	/* an empty archive */
		return LDA_SUCCESS;
	if (!state[LDA_BR_CHAIN])
		return LDA_BAD_DATA;
	if (state[LDA_BR_MEMBERS] > max_records)
		return LDA_TAR_MORE_RECORDS;
	return LDA_SUCCESS;
}

static __device__ __forceinline__ u32
pre_status(const u32 *__restrict__ state, u64 K, u64 cap, u64 max_records, u64 total,
	   u64 out_avail)
{
	const u32 f = find_status(state, K, cap, max_records);
	if (f != LDA_SUCCESS)
		return f;
	return total > out_avail ? LDA_INSUFFICIENT_SPACE : LDA_SUCCESS;
}

/*
 * One workgroup per LDA_BR_SCAN_WG bytes = 32 blocks (in: nb blocks).
 * offsets == NULL: counts[wg] = candidates of the workgroup's blocks, and
 * workgroup 0 notes whether block 0 is all zero.  Otherwise offsets /
 * block_sums are the scan of the counts, and the candidates below index cap
 * are written in file order.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tar_scan_kernel(const u8 *__restrict__ in, u64 nb, u64 *__restrict__ counts,
		    const u64 *__restrict__ offsets, const u64 *__restrict__ block_sums, u64 cap,
		    u64 *__restrict__ cand_pos, u32 *__restrict__ cand_size,
		    u32 *__restrict__ state)
{
	__shared__ u32 stated[LDA_TAR_SCAN_BLOCKS], csize[LDA_TAR_SCAN_BLOCKS], wsum[4];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const u64 b0 = (u64)blockIdx.x * LDA_TAR_SCAN_BLOCKS;
	u64 at = 0;

	if (offsets) {
		if (counts[blockIdx.x] == 0)
			return;
		at = offsets[blockIdx.x] + block_sums[blockIdx.x / LDA_SCAN_BLOCK];
	} else if (blockIdx.x == 0 && wave == 0 && nb) {
		u64 v;
		__builtin_memcpy(&v, in + 8 * lane, 8);
		if (__ballot(v != 0) == 0 && lane == 0)
			state[LDA_TAR_ZERO0] = 1;
	}
	/* the checksum field first: a data block costs these 8 bytes */
	if (tid < LDA_TAR_SCAN_BLOCKS) {
		u32 s = NO_FIELD;
		if (b0 + tid < nb) {
			u8 f[8];
			u64 v;
			u32 digits;
			__builtin_memcpy(f, in + (b0 + tid) * BLOCK + 148, 8);
			if (oct_field(f, 8, &v, &digits) && digits)
				s = (u32)v;
		}
		stated[tid] = s;
		csize[tid] = 0;
	}
	__syncthreads();
	for (u32 j = wave; j < LDA_TAR_SCAN_BLOCKS; j += 4) {
		const u32 s = stated[j];	/* (uniform in the wave) */
		if (s == NO_FIELD)
			continue;
		const u64 pos = b0 + j;
		const u8 *h = in + pos * BLOCK;
		u8 q[8];
		u32 sum = 0, high = 0;
		__builtin_memcpy(q, h + 8 * lane, 8);
#pragma unroll
		for (u32 i = 0; i < 8; i++) {
			const u32 b = 8 * lane + i - 148 < 8 ? 0x20 : q[i];
			sum += b;
			high += b >> 7;
		}
		sum = wave_sum(sum);
		high = wave_sum(high);
		/* unsigned chars, or signed ones */
		if (s != sum && s != sum - 256 * high)
			continue;
		u64 size;
		if (!hdr_size(h, &size) || size >= SIZE_LIMIT)
			continue;
		const u64 d = data_blocks(h[156], size);
		if (pos + 1 + d > nb)
			continue;
		u32 cs = (u32)(1 + d);
		if (pos + 1 + d < nb) {
			u64 v;
			__builtin_memcpy(&v, in + (pos + 1 + d) * BLOCK + 8 * lane, 8);
			if (__ballot(v != 0) == 0)
				cs = (u32)(nb - pos);
		}
		if (lane == 0)
			csize[j] = cs;
	}
	__syncthreads();
	const u32 mine = tid < LDA_TAR_SCAN_BLOCKS ? csize[tid] : 0;
	u32 tot;
	const u32 pre = wg_count_excl(mine != 0, wsum, &tot);
	if (offsets) {
		if (mine && at + pre < cap) {
			cand_pos[at + pre] = b0 + tid;
			cand_size[at + pre] = mine;
		}
	} else if (tid == 0) {
		counts[blockIdx.x] = tot;
	}
}

/*
 * The serial walk that defines the rule, one lane: a dependent header per
 * record.  It runs instead of the scan and the chain when LDA_TAR_SERIAL asks
 * (the baseline of tools/bench_tar.py, same results); *k_out = 0 candidates.
 */
extern "C" __global__ void __launch_bounds__(64)
lda_tar_walk_kernel(const u8 *__restrict__ in, u64 nb, u64 max_records,
		    u64 *__restrict__ rec_pos, u64 *__restrict__ rec_n, u32 *__restrict__ state,
		    u64 *__restrict__ k_out)
{
	if (threadIdx.x)
		return;
	u64 pos = 0;
	u32 count = 0, ok = nb != 0, zero0 = 0;
	while (pos < nb) {
		const u8 *h = in + pos * BLOCK;
		u64 any = 0, stated, size;
		u32 sum = 0, high = 0, digits;
		for (u32 w = 0; w < BLOCK / 8; w++) {
			u64 v;
			__builtin_memcpy(&v, h + 8 * w, 8);
			any |= v;
			for (u32 i = 0; i < 8; i++) {
				const u32 b = 8 * w + i - 148 < 8 ? 0x20 : (u32)(v >> (8 * i)) & 0xFF;
				sum += b;
				high += b >> 7;
			}
		}
		if (!any) {
			zero0 = pos == 0;
			break;
		}
		ok = oct_field(h + 148, 8, &stated, &digits) && digits &&
		     ((u32)stated == sum || (u32)stated == sum - 256 * high) && hdr_size(h, &size) &&
		     size < SIZE_LIMIT;
		const u64 d = ok ? data_blocks(h[156], size) : 0;
		ok = ok && pos + 1 + d <= nb;
		if (!ok)
			break;
		if (count < max_records) {
			rec_pos[count] = pos;
			rec_n[count] = 1 + d;
		}
		count++;
		pos += 1 + d;
	}
	state[LDA_BR_CHAIN] = ok;
	state[LDA_BR_MEMBERS] = count;
	state[LDA_TAR_FLAGS] = 0;
	state[LDA_TAR_ZERO0] = zero0;
	*k_out = 0;
}

/* the records of a pax extended header, "%d %s=%s\n" each: 0 where one does
 * not parse, else PAX_OK with PAX_PATH for a path= key - the last one's value
 * (relative to b) - and PAX_SIZE for a size= key */
#define PAX_OK 1u
#define PAX_PATH 2u
#define PAX_SIZE 4u
static __device__ __forceinline__ u32
pax_parse(const u8 *b, u32 n, u32 *path_off, u32 *path_len)
{
	u32 p = 0, seen = PAX_OK, po = 0, pl = 0;

	while (p < n) {
		u32 q = p, len = 0;
		while (q < n && q - p < 8 && (u32)(b[q] - 0x30) < 10) {
			len = len * 10 + (b[q] - 0x30);
			q++;
		}
		if (q == p || q >= n || b[q] != 0x20 || len > n - p || q + 1 >= p + len)
			return 0;
		const u32 last = p + len - 1;
		if (b[last] != 0x0A)
			return 0;
		u32 eq = q + 1;
		while (eq < last && b[eq] != '=')
			eq++;
		if (eq == last || eq == q + 1)
			return 0;
		if (eq - (q + 1) == 4) {
			const u8 *k = b + q + 1;
			const bool path = k[0] == 'p' && k[1] == 'a' && k[2] == 't' && k[3] == 'h';
			const bool size = k[0] == 's' && k[1] == 'i' && k[2] == 'z' && k[3] == 'e';
			seen |= (path ? PAX_PATH : 0) | (size ? PAX_SIZE : 0);
			po = path ? eq + 1 : po;
			pl = path ? last - (eq + 1) : pl;
		}
		p += len;
	}
	*path_off = po;
	*path_len = pl;
	return seen;
}

/*
 * Record k of the chain (rec_pos[k]: its header, in blocks).  An entry record:
 * flag[k] = 1, words 0 to 6 of its row in tmp + 7 k, res[k] its pre-extract
 * result, room[k] its room in the output.  An extension record, a surplus
 * chunk, an archive under verdicts 1 to 4: flag[k] = room[k] = 0.  The last
 * record notes where it ends by its own size (ts[LDA_TS_END], in blocks).
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tar_resolve_kernel(const u8 *__restrict__ in, u64 nb, u64 max_records, u64 align_mask,
		       u32 *__restrict__ state, const u64 *__restrict__ k_at, u64 cap,
		       const u64 *__restrict__ rec_pos, u64 *__restrict__ ts,
		       u64 *__restrict__ tmp, s32 *__restrict__ res, u64 *__restrict__ flag,
		       u64 *__restrict__ room)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_records)
		return;
	flag[k] = 0;
	room[k] = 0;
	if (find_status(state, *k_at, cap, max_records) != LDA_SUCCESS || k >= records_of(state))
		return;
	const u64 pos = rec_pos[k];
	const u8 *h = in + pos * BLOCK;
	const u32 t = h[156];
	u64 size = 0;
	hdr_size(h, &size);	/* (valid: the scan accepted the header) */
	if (k + 1 == records_of(state))
		ts[LDA_TS_END] = pos + 1 + data_blocks(t, size);
	if (t == 'L')
		atomicOr(&state[LDA_TAR_FLAGS], LDA_TAR_HAS_L);
	if (t == 'x' || t == 'X' || t == 'g')
		atomicOr(&state[LDA_TAR_FLAGS], LDA_TAR_HAS_PAX);
	if (is_ext(t))
		return;

	s32 r = LDA_SUCCESS;
	bool have_l = false, have_pax = false;
	u64 l_off = 0, pax_off = 0;
	u32 l_len = 0, pax_len = 0;
	/* the extension records in front, the nearest first: the last in file
	 * order of each kind names the entry */
	for (u32 back = 1; back <= LDA_TAR_EXT_MAX + 1 && back <= k; back++) {
		const u64 q = rec_pos[k - back];
		const u8 *e = in + q * BLOCK;
		const u32 et = e[156];
		if (!is_ext(et))
			break;
		if (back > LDA_TAR_EXT_MAX) {
			r = LDA_TAR_UNSUPPORTED;
			break;
		}
		if (et != 'L' && et != 'x' && et != 'X')
			continue;
		u64 esize = 0;
		hdr_size(e, &esize);
		if (esize > LDA_TAR_EXT_BYTES) {
			r = LDA_TAR_UNSUPPORTED;
			continue;
		}
		/* (the scan put the record's data below nb) */
		const u8 *data = e + BLOCK;
		if (et == 'L') {
			if (!have_l) {
				have_l = true;
				l_off = (q + 1) * BLOCK;
				l_len = strnlen_dev(data, (u32)esize);
			}
		} else {
			u32 po = 0, pl = 0;
			const u32 seen = pax_parse(data, (u32)esize, &po, &pl);
			if (!seen || (seen & PAX_SIZE)) {
				r = LDA_TAR_UNSUPPORTED;
			} else if ((seen & PAX_PATH) && !have_pax) {
				have_pax = true;
				pax_off = (q + 1) * BLOCK + po;
				pax_len = pl;
			}
		}
	}
	if (t == 'S' || t == 'M' || t == 'D')
		r = LDA_TAR_UNSUPPORTED;
	const u64 usize = r != LDA_SUCCESS || (t >= '1' && t <= '6') ? 0 : size;
	u64 name_off = pos * BLOCK, name_len = 0, src = LDA_TAR_NAME_HEADER;
	if (r == LDA_SUCCESS && have_pax) {
		src = LDA_TAR_NAME_PAX;
		name_off = pax_off;
		name_len = pax_len;
	} else if (r == LDA_SUCCESS && have_l) {
		src = LDA_TAR_NAME_L;
		name_off = l_off;
		name_len = l_len;
	} else {
		name_len = strnlen_dev(h, 100);
		if (h[257] == 'u' && h[258] == 's' && h[259] == 't' && h[260] == 'a' &&
		    h[261] == 'r' && h[262] == 0)
			name_len |= (u64)strnlen_dev(h + 345, 155) << 32;
	}
	u64 mtime = 0;
	u32 digits;
	if (!oct_field(h + 136, 12, &mtime, &digits))
		mtime = 0;
	u64 *row = tmp + 7 * k;
	row[0] = pos * BLOCK;
	row[1] = name_off;
	row[2] = name_len;
	row[3] = t | src << 8;
	row[4] = (pos + 1) * BLOCK;
	row[5] = usize;
	row[6] = mtime;
	res[k] = r;
	flag[k] = 1;
	room[k] = (usize + align_mask) & ~align_mask;
}

/*
 * Behind the scans of flag[] and room[] (f_off, r_off: the local prefixes,
 * f_sums, r_sums: the block sums): the entry's row at its number with out_off
 * as word 7, its result, and per record the copy's descriptor - tiles[k] is 0
 * unless the archive extracts and the entry succeeded.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tar_desc_kernel(u64 max_records, u64 out_avail, const u32 *__restrict__ state,
		    const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ tmp,
		    const s32 *__restrict__ res, const u64 *__restrict__ flag,
		    const u64 *__restrict__ f_off, const u64 *__restrict__ f_sums,
		    const u64 *__restrict__ r_off, const u64 *__restrict__ r_sums,
		    u64 *__restrict__ rows, s32 *__restrict__ results, u64 *__restrict__ cp_src,
		    u64 *__restrict__ cp_dst, u64 *__restrict__ cp_len, u64 *__restrict__ tiles)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_records)
		return;
	const u64 total = r_sums[(max_records + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];
	const u32 pre = pre_status(state, *k_at, cap, max_records, total, out_avail);
	const bool known = pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE;
	u64 s = 0, d = 0, l = 0;

	if (known && k < records_of(state) && flag[k]) {
		const u64 e = f_off[k] + f_sums[k / LDA_SCAN_BLOCK];
		const u64 uoff = r_off[k] + r_sums[k / LDA_SCAN_BLOCK];
		const u64 *t = tmp + 7 * k;
		if (rows) {
			u64 *row = rows + LDA_TAR_WORDS * e;
#pragma unroll
			for (u32 i = 0; i < 7; i++)
				row[i] = t[i];
			row[7] = uoff;
		}
		results[e] = res[k];
		if (pre == LDA_SUCCESS && res[k] == LDA_SUCCESS) {
			s = t[4];
			d = uoff;
			l = t[5];
		}
	}
	cp_src[k] = s;
	cp_dst[k] = d;
	cp_len[k] = l;
	tiles[k] = (l + LDA_TAR_COPY_TILE - 1) / LDA_TAR_COPY_TILE;
}

/*
 * Chunk k: len[k] bytes from in + src[k] to out + dst[k], in tiles of
 * LDA_TAR_COPY_TILE bytes.  Tile t of all belongs to the last chunk k whose
 * tile prefix t_off[k] + t_sums[k / LDA_SCAN_BLOCK] (t_sums NULL: t_off alone)
 * is at most t; *total_at is the number of tiles.  Nothing is written outside
 * [dst[k], dst[k] + len[k]) of any chunk.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tar_copy_kernel(u64 n_chunks, const u64 *__restrict__ t_off, const u64 *__restrict__ t_sums,
		    const u64 *__restrict__ total_at, const u64 *__restrict__ src,
		    const u64 *__restrict__ dst, const u64 *__restrict__ len,
		    const u8 *__restrict__ in, u8 *__restrict__ out)
{
	const u64 total = *total_at;

	if (!n_chunks)
		return;
	for (u64 t = blockIdx.x; t < total; t += gridDim.x) {	/* (all of this is uniform) */
		u64 lo = 0, hi = n_chunks;
		for (u32 s = 0; s < 64 && hi - lo > 1; s++) {
			const u64 mid = lo + (hi - lo) / 2;
			const u64 p = t_off[mid] + (t_sums ? t_sums[mid / LDA_SCAN_BLOCK] : 0);
			if (p <= t)
				lo = mid;
			else
				hi = mid;
		}
		const u64 first = t_off[lo] + (t_sums ? t_sums[lo / LDA_SCAN_BLOCK] : 0);
		const u64 l = len[lo];
		if (first > t || (t - first) >= (l + LDA_TAR_COPY_TILE - 1) / LDA_TAR_COPY_TILE)
			continue;	/* (cannot happen: the prefix is that of these lengths) */
		const u64 off = (t - first) * LDA_TAR_COPY_TILE;
		const u64 part = l - off < LDA_TAR_COPY_TILE ? l - off : LDA_TAR_COPY_TILE;
		copy_tile(in + src[lo] + off, out + dst[lo] + off, part, threadIdx.x);
	}
}

/*
 * One workgroup: result[0] the verdict - the pre-extract one, else the result
 * of the first entry that did not succeed -, [1] entries (the records under
 * MORE_RECORDS, the candidates under MORE_CANDIDATES), [2] the byte offset
 * where the walk ended, [3] bytes of output needed, [4] flags.  state NULL: the
 * file holds no block, which is BAD_DATA.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_tar_final_kernel(u64 nb, u64 max_records, u64 out_avail, const u32 *__restrict__ state,
		     const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ ts,
		     const u64 *__restrict__ entries_at, const u64 *__restrict__ total_at,
		     const s32 *__restrict__ results, u64 *__restrict__ result)
{
	__shared__ unsigned long long first;	/* entry << 32 | its result */
	const u32 tid = threadIdx.x;

	if (!state) {
		if (tid < LDA_TAR_RESULT_WORDS)
			result[tid] = tid == 0 ? LDA_BAD_DATA : 0;
		return;
	}
	const u64 K = *k_at, total = *total_at, entries = *entries_at;
	const u32 pre = pre_status(state, K, cap, max_records, total, out_avail);

	if (tid == 0)
		first = ~0ull;
	__syncthreads();
	if (pre == LDA_SUCCESS)
		for (u64 k = tid; k < entries; k += 256) {
			const s32 r = results[k];
			if (r != LDA_SUCCESS)
				atomicMin(&first, (unsigned long long)(k << 32 | (u32)r));
		}
	__syncthreads();
	if (tid == 0) {
		const bool known = pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE;
		const bool empty = state[LDA_TAR_ZERO0];
		const u64 end = empty ? 0 : ts[LDA_TS_END];
		result[0] = pre != LDA_SUCCESS ? pre : first != ~0ull ? (u32)first : LDA_SUCCESS;
		result[1] = known ? entries : pre == LDA_TAR_MORE_RECORDS ? state[LDA_BR_MEMBERS] :
			    pre == LDA_TAR_MORE_CANDIDATES ? K : 0;
		result[2] = known ? end * BLOCK : 0;
		result[3] = known ? total : 0;
		result[4] = known ? state[LDA_TAR_FLAGS] | (empty || end != nb ? LDA_TAR_EOF : 0) : 0;
	}
}
