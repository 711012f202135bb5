/*
 * zip_kernels.hip - reading a ZIP archive that lies in device memory: where its
 * end record, its central directory and its entries are, the descriptors of
 * ONE raw-DEFLATE decompress batch, one copy of the stored entries and ONE
 * CRC-32 batch that put and check every entry at its final place, the
 * archive's result words, index rows and per-entry results (host_zip.hip;
 * tools/models/zip_walk.py is the CPU model of the whole rule, and the tests
 * run it on the same files).  What an archive is: include/libdeflate_amd.h.
 *
 *   lda_zip_end_kernel      one workgroup over the file's last 65 557 bytes:
 *                           the highest offset that carries 50 4b 05 06 with a
 *                           comment that stays inside the file (a max
 *                           reduction), then one lane reads it, and the ZIP64
 *                           locator and end record when they are there: the
 *                           entry count, cd_off and cd_size of the archive
 *                           (zs[], device values from here on).
 *   lda_zip_scan_kernel     lda_gzm_scan_kernel's shape over the directory
 *                           alone: the grid covers the file, workgroups
 *                           outside [cd_off, cd_end) exit at once.  Every
 *                           offset p of the directory with 50 4b 01 02 and
 *                           p + 46 <= cd_end is a CANDIDATE, kept as p -
 *                           cd_off: names, extras and comments make false ones.
 *   lda_zip_size_kernel     a candidate's size, 46 + name + extra + comment,
 *                           as the chain kernels want it: 0 - no successor -
 *                           when it runs past cd_end, and for the record that
 *                           ends exactly at cd_end the size that ends it at
 *                           LDA_ZIP_CHAIN_END, the one end the host knows.
 *   lda_bgzf_jump_kernel / lda_bgzf_top_kernel / lda_bgzf_members_kernel
 *                           (bgzf_read_kernels.hip, launched by host_finder.h)
 *                           keep the candidates that the chain from cd_off
 *                           reaches.
 *   lda_zip_resolve_kernel  per entry: the central fields, the ZIP64 extra,
 *                           the local header, the checks; seven words of its
 *                           index row, its pre-decode result, its room.
 *   lda_zip_desc_kernel     behind the scan of the rooms: out_off, and the
 *                           descriptors of the decode, the copy and the CRCs.
 *   lda_zip_copy_kernel     the stored entries: 16-byte stores, ragged heads
 *                           and tails (copy_span()).
 *   lda_zip_final_kernel    one workgroup: every entry's result - the decode's,
 *                           the CRC batch's value against the directory's -,
 *                           the verdict, the five result words.
 *   lda_zip_rfinal_kernel   the same per-entry result for a selection
 *                           (libdeflate_amd_zip_read_batch).
 *
 * The input is hostile by definition: every load is checked against n (the
 * end record lies below n, the directory below the end record, every chained
 * record inside the directory, every local header and every entry's data below
 * cd_off), every index against the candidate count, the ZIP64 extra walk is
 * bounded by 65 535 / 4 records, and no loop takes an unbounded count from the
 * file.
 */
#include "device_common.h"
#include "kernels.h"

#define SIG_END 0x06054b50u	/* 50 4b 05 06 */
#define SIG_LOC64 0x07064b50u
#define SIG_END64 0x06064b50u
#define SIG_CEN 0x02014b50u
#define SIG_LOCAL 0x04034b50u
#define END_BYTES 22u
#define CEN_BYTES 46u
#define MARK32 0xFFFFFFFFull
/* flag bits 0, 5, 6, 13: encryption, patches, strong encryption, masked headers */
#define FLAGS_REFUSED 0x2061u

static __device__ __forceinline__ u32 ld16(const u8 *p)
{
	return (u32)p[0] | (u32)p[1] << 8;
}

static __device__ __forceinline__ u32 ld32(const u8 *p)
{
	return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24;
}

static __device__ __forceinline__ u64 ld64(const u8 *p)
{
	return (u64)ld32(p) | (u64)ld32(p + 4) << 32;
}

/* the directory is the chain the end record states */
static __device__ __forceinline__ bool
chain_ok(const u64 *__restrict__ zs, const u32 *__restrict__ state)
{
	if (zs[LDA_ZS_CD_SIZE] == 0)	/* no candidate, no chain: an empty archive */
		return zs[LDA_ZS_ENTRIES] == 0;
	return state[LDA_BR_CHAIN] && state[LDA_BR_MEMBERS] == zs[LDA_ZS_ENTRIES];
}

/* verdicts 1 to 4 of include/libdeflate_amd.h, in their order */
static __device__ __forceinline__ u32
find_status(const u64 *__restrict__ zs, const u32 *__restrict__ state, u64 K, u64 cap,
	    u64 max_entries)
{
	if (zs[LDA_ZS_BAD])
		return LDA_BAD_DATA;
	if (zs[LDA_ZS_ENTRIES] > max_entries)
		return LDA_ZIP_MORE_ENTRIES;
	if (K > cap)
		return LDA_ZIP_MORE_CANDIDATES;
	if (!chain_ok(zs, state))
		return LDA_BAD_DATA;
	return LDA_SUCCESS;
}

static __device__ __forceinline__ u32
pre_status(const u64 *__restrict__ zs, const u32 *__restrict__ state, u64 K, u64 cap,
	   u64 max_entries, u64 total, u64 out_avail)
{
	const u32 f = find_status(zs, state, K, cap, max_entries);
	if (f != LDA_SUCCESS)
		return f;
	return total > out_avail ? LDA_INSUFFICIENT_SPACE : LDA_SUCCESS;
}

/*
 * meta[k]: the directory's CRC-32, the entry's pre-decode result << 32, its
 * kind << 40.  An entry's final result from it, the decode batch's verdict and
 * actual_in (exact input) and the CRC batch's value.
 */
static __device__ __forceinline__ s32
entry_result(u64 meta, s32 batch_res, u64 actual_in, u64 in_n, u32 crc)
{
	const s32 pre = (s32)((meta >> 32) & 0xFF);
	const u32 kind = (u32)(meta >> 40) & 3;

	if (pre != LDA_SUCCESS || kind == LDA_ZIP_KIND_NONE)
		return pre;
	if (kind == LDA_ZIP_KIND_DEFLATE) {
		if (batch_res != LDA_SUCCESS)
			return batch_res;
		if (actual_in != in_n)
			return LDA_BAD_DATA;
	}
	return crc == (u32)meta ? LDA_SUCCESS : LDA_BAD_DATA;
}

/*
 * One workgroup.  Offsets p = w0 + r, w0 = n - min(n, 65 557), r + 22 <= n -
 * w0: thread t tests r = t, t + 1024, ...; its last hit is its highest.
 */
extern "C" __global__ void __launch_bounds__(1024)
lda_zip_end_kernel(const u8 *__restrict__ in, u64 n, u64 *__restrict__ zs)
{
	__shared__ u32 wmax[16];
	const u32 tid = threadIdx.x;
	const u64 win = n < LDA_ZIP_WINDOW ? n : LDA_ZIP_WINDOW;
	const u64 w0 = n - win;
	u32 best = 0;	/* r + 1 */

	if (win >= END_BYTES) {
		const u32 span = (u32)win - END_BYTES + 1;
		for (u32 r = tid; r < span; r += 1024) {
			const u8 *p = in + w0 + r;
			if (ld32(p) == SIG_END && r + END_BYTES + ld16(p + 20) <= (u32)win)
				best = r + 1;
		}
	}
	best = wave_max(best);
	if ((tid & 63) == 0)
		wmax[tid >> 6] = best;
	__syncthreads();
	if (tid)
		return;
	for (u32 w = 0; w < 16; w++)
		best = wmax[w] > best ? wmax[w] : best;

	u64 entries = 0, cd_off = 0, cd_size = 0, flags = 0;
	bool ok = false;
	if (best) {
		const u64 p = w0 + best - 1;
		const u8 *e = in + p;
		u64 anchor = p;	/* where the directory has to end */
		ok = ld16(e + 4) == 0 && ld16(e + 6) == 0 && ld16(e + 8) == ld16(e + 10);
		entries = ld16(e + 10);
		cd_size = ld32(e + 12);
		cd_off = ld32(e + 16);
		if (p >= 20 && ld32(e - 20) == SIG_LOC64) {
			const u64 q = ld64(e - 20 + 8);
			ok = ld32(e - 20 + 16) <= 1 && q <= p - 20 && p - 20 - q >= 56 &&
			     ld32(in + q) == SIG_END64;
			if (ok) {
				const u8 *z = in + q;
				ok = ld32(z + 16) == 0 && ld32(z + 20) == 0 &&
				     ld64(z + 24) == ld64(z + 32);
				entries = ld64(z + 32);
				cd_size = ld64(z + 40);
				cd_off = ld64(z + 48);
				anchor = q;
				flags = LDA_ZIP_ZIP64;
			}
		}
		ok = ok && cd_size <= MARK32 && cd_size <= anchor && cd_off == anchor - cd_size;
	}
	zs[LDA_ZS_BAD] = !ok;
	zs[LDA_ZS_ENTRIES] = ok ? entries : 0;
	zs[LDA_ZS_CD_OFF] = ok ? cd_off : 0;
	zs[LDA_ZS_CD_SIZE] = ok ? cd_size : 0;
	zs[LDA_ZS_FLAGS] = ok ? flags : 0;
}

/*
 * One workgroup per LDA_BR_SCAN_WG bytes of file, in steps of 4 KiB, as
 * lda_gzm_scan_kernel: 16 bytes per thread into LDS (and 16 more behind the
 * tile), every offset's four bytes against the signature.  Bytes at or past
 * cd_end read as 0; offsets below cd_off or within 45 bytes of cd_end are no
 * candidates.  Signatures cannot overlap, so a thread holds up to 4.
 * offsets == NULL: counts[wg] = candidates of the workgroup's range.
 * Otherwise offsets / block_sums are the scan of the counts, and the
 * candidates below index cap are written in file order, relative to cd_off.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_scan_kernel(const u8 *__restrict__ in, const u64 *__restrict__ zs,
		    u64 *__restrict__ counts, const u64 *__restrict__ offsets,
		    const u64 *__restrict__ block_sums, u64 cap, u64 *__restrict__ cand_pos)
{
	__shared__ __attribute__((aligned(16))) u32 tile[LDA_BR_TILE / 4 + 4];
	__shared__ u32 wsum[4];
	const u32 tid = threadIdx.x;
	const u64 wg0 = (u64)blockIdx.x * LDA_BR_SCAN_WG;
	const u64 cd_off = zs[LDA_ZS_CD_OFF], cd_end = cd_off + zs[LDA_ZS_CD_SIZE];
	u64 at = 0;	/* candidates of this workgroup so far / where they go */

	if (wg0 + LDA_BR_SCAN_WG <= cd_off || wg0 >= cd_end) {	/* (uniform) */
		if (!offsets && tid == 0)
			counts[blockIdx.x] = 0;
		return;
	}
	if (offsets) {
		if (counts[blockIdx.x] == 0)
			return;
		at = offsets[blockIdx.x] + block_sums[blockIdx.x / LDA_SCAN_BLOCK];
	}
	uint4 mine = load16_guard(in, wg0 + 16 * (u64)tid, cd_end);
	uint4 behind = { 0, 0, 0, 0 };
	if (tid == 0)
		behind = load16_guard(in, wg0 + LDA_BR_TILE, cd_end);
	for (u32 s = 0; s < LDA_BR_SCAN_WG / LDA_BR_TILE; s++) {
		const u64 base = wg0 + (u64)s * LDA_BR_TILE;
		if (base >= cd_end)
			break;	/* (uniform) */
		*(uint4 *)&tile[4 * tid] = mine;
		if (tid == 0)
			*(uint4 *)&tile[LDA_BR_TILE / 4] = behind;
		__syncthreads();
		if (s + 1 < LDA_BR_SCAN_WG / LDA_BR_TILE) {
			mine = load16_guard(in, base + LDA_BR_TILE + 16 * (u64)tid, cd_end);
			if (tid == 0)
				behind = load16_guard(in, base + 2 * LDA_BR_TILE, cd_end);
		}
		const uint4 q = *(const uint4 *)&tile[4 * tid];
		const u32 w[5] = { q.x, q.y, q.z, q.w, tile[4 * tid + 4] };
		u32 mask = 0;
#pragma unroll
		for (u32 j = 0; j < 16; j++) {
			const u32 win = j & 3 ? (w[j >> 2] >> (8 * (j & 3))) |
						(w[(j >> 2) + 1] << (32 - 8 * (j & 3))) : w[j >> 2];
			mask |= (u32)(win == SIG_CEN) << j;
		}
		const u64 p0 = base + 16 * (u64)tid;
		if (mask && (p0 < cd_off || p0 + 15 + CEN_BYTES > cd_end)) {
#pragma unroll
			for (u32 j = 0; j < 16; j++)
				if (p0 + j < cd_off || p0 + j + CEN_BYTES > cd_end)
					mask &= ~(1u << j);
		}
		u32 tot;
		const u32 pre = wg_count_excl((u32)__builtin_popcount(mask), wsum, &tot);
		if (offsets) {
			u64 dst = at + pre;
			for (u32 m = mask; m && dst < cap; m &= m - 1, dst++)
				cand_pos[dst] = p0 + (u32)__builtin_ctz(m) - cd_off;
		}
		at += tot;
		__syncthreads();	/* the tile and wsum are free again */
	}
	if (!offsets && tid == 0)
		counts[blockIdx.x] = at;
}

/* cand_size[i] for the chain kernels, which are launched with LDA_ZIP_CHAIN_END
 * as the chain's end: a record's end is at most cd_size <= 2^32 - 1, and is
 * LDA_ZIP_CHAIN_END only when it is the directory's */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_size_kernel(const u8 *__restrict__ in, const u64 *__restrict__ zs,
		    const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ cand_pos,
		    u32 *__restrict__ cand_size)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 K = *k_at;
	if (i >= cap || K > cap || i >= K)
		return;
	const u64 rel = cand_pos[i], cd_size = zs[LDA_ZS_CD_SIZE];
	/* (rel + 46 <= cd_size holds for every candidate written) */
	const u8 *c = in + zs[LDA_ZS_CD_OFF] + rel;
	const u64 end = rel + CEN_BYTES + ld16(c + 28) + ld16(c + 30) + ld16(c + 32);
	u32 size = 0;
	if (end < cd_size)
		size = (u32)(end - rel);
	else if (end == cd_size)
		size = (u32)(LDA_ZIP_CHAIN_END - rel);
	cand_size[i] = size;
}

/*
 * Entry k of the chain (rel[k]: its central record, relative to cd_off):
 * words 0 to 6 of its index row, results[k] its pre-decode result, sizes[k]
 * its room in the output - usize rounded up to the alignment, 0 for an entry
 * that is refused here and for the rest of the max_entries chunks.  Nothing is
 * written for an archive under verdicts 1 to 4 but sizes[].
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_resolve_kernel(const u8 *__restrict__ in, u64 max_entries, u64 align_mask,
		       const u64 *__restrict__ zs, const u32 *__restrict__ state,
		       const u64 *__restrict__ k_at, u64 cap, const u64 *__restrict__ rel,
		       u64 *__restrict__ rows, s32 *__restrict__ results,
		       u64 *__restrict__ sizes)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_entries)
		return;
	if (find_status(zs, state, *k_at, cap, max_entries) != LDA_SUCCESS ||
	    k >= zs[LDA_ZS_ENTRIES]) {
		sizes[k] = 0;
		return;
	}
	const u64 cd_off = zs[LDA_ZS_CD_OFF];
	const u64 c_at = cd_off + rel[k];
	/* (the chain put the whole record inside the directory) */
	const u8 *c = in + c_at;
	const u32 flags = ld16(c + 8), method = ld16(c + 10), crc = ld32(c + 16);
	const u32 name_len = ld16(c + 28), extra_len = ld16(c + 30);
	u64 csize = ld32(c + 20), usize = ld32(c + 24), lho = ld32(c + 42);
	u32 disk = ld16(c + 34);
	s32 r = LDA_SUCCESS;

	if (csize == MARK32 || usize == MARK32 || lho == MARK32 || disk == 0xFFFF) {
		const u8 *x = c + CEN_BYTES + name_len, *z = x;
		u32 at = 0, have = 0, o = 0;
		for (u32 it = 0; it < 65535 / 4 && at + 4 <= extra_len; it++) {
			const u32 id = ld16(x + at), sz = ld16(x + at + 2);
			if (at + 4 + sz > extra_len)
				break;
			if (id == 0x0001) {
				z = x + at + 4;
				have = sz;
				break;
			}
			at += 4 + sz;
		}
		if (usize == MARK32) {
			if (o + 8 <= have)
				usize = ld64(z + o);
			else
				r = LDA_BAD_DATA;
			o += 8;
		}
		if (csize == MARK32) {
			if (o + 8 <= have)
				csize = ld64(z + o);
			else
				r = LDA_BAD_DATA;
			o += 8;
		}
		if (lho == MARK32) {
			if (o + 8 <= have)
				lho = ld64(z + o);
			else
				r = LDA_BAD_DATA;
			o += 8;
		}
		if (disk == 0xFFFF) {
			if (o + 4 <= have)
				disk = ld32(z + o);
			else
				r = LDA_BAD_DATA;
		}
	}
	if (r == LDA_SUCCESS && disk != 0)
		r = LDA_BAD_DATA;
	if (r == LDA_SUCCESS && ((flags & FLAGS_REFUSED) || (method != 0 && method != 8) ||
				 csize > MARK32 || usize > MARK32))
		r = LDA_ZIP_UNSUPPORTED;
	u64 data_off = 0;
	if (r == LDA_SUCCESS) {
		r = LDA_BAD_DATA;
		if (lho <= cd_off && cd_off - lho >= 30 && ld32(in + lho) == SIG_LOCAL) {
			const u64 d = lho + 30 + ld16(in + lho + 26) + ld16(in + lho + 28);
			if (d <= cd_off) {
				data_off = d;
				if (csize <= cd_off - d)
					r = LDA_SUCCESS;
			}
		}
	}
	if (r == LDA_SUCCESS && method == 0 && csize != usize)
		r = LDA_BAD_DATA;
	u64 *row = rows + LDA_ZIP_WORDS * k;
	row[0] = c_at;
	row[1] = name_len;
	row[2] = method | flags << 16;
	row[3] = crc;
	row[4] = data_off;
	row[5] = csize;
	row[6] = usize;
	results[k] = r;
	sizes[k] = r == LDA_SUCCESS ? (usize + align_mask) & ~align_mask : 0;
}

/*
 * Behind the scan of sizes[] (out_off holds the local prefix): word 7 of the
 * index rows, and per chunk the decode batch's descriptors (method 8: exact
 * input, exact fill), the copy's (method 0), the CRC batch's (both) and
 * meta[].  Stored, refused and surplus chunks give the decode nothing, and so
 * do all of them when the archive is refused before the decode.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_desc_kernel(u64 max_entries, u64 out_avail, const u64 *__restrict__ zs,
		    const u32 *__restrict__ state, const u64 *__restrict__ k_at, u64 cap,
		    const u64 *__restrict__ block_sums, u64 *__restrict__ rows,
		    const s32 *__restrict__ results, u64 *__restrict__ in_off,
		    u64 *__restrict__ in_n, u64 *__restrict__ out_off, u64 *__restrict__ out_av,
		    u64 *__restrict__ cp_src, u64 *__restrict__ cp_len, u64 *__restrict__ crc_n,
		    u64 *__restrict__ meta)
{
	const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
	if (k >= max_entries)
		return;
	const u64 total = block_sums[(max_entries + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];
	const u32 pre = pre_status(zs, state, *k_at, cap, max_entries, total, out_avail);
	const bool known = pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE;
	const bool entry = known && k < zs[LDA_ZS_ENTRIES];
	const u64 uoff = out_off[k] + block_sums[k / LDA_SCAN_BLOCK];
	u64 *row = rows + LDA_ZIP_WORDS * k;
	u64 m = 0, io = 0, in = 0, oo = 0, oa = 0, cs = 0, cl = 0, cn = 0;

	if (entry) {
		const s32 r = results[k];
		row[7] = uoff;
		m = row[3] | (u64)(r & 0xFF) << 32;
		if (pre == LDA_SUCCESS && r == LDA_SUCCESS) {
			oo = uoff;
			cn = row[6];
			if ((row[2] & 0xFFFF) == 8) {
				m |= (u64)LDA_ZIP_KIND_DEFLATE << 40;
				io = row[4];
				in = row[5];
				oa = row[6];
			} else {
				m |= (u64)LDA_ZIP_KIND_STORED << 40;
				cs = row[4];
				cl = row[6];
			}
		}
	}
	in_off[k] = io;
	in_n[k] = in;
	out_off[k] = oo;
	out_av[k] = oa;
	cp_src[k] = cs;
	cp_len[k] = cl;
	crc_n[k] = cn;
	meta[k] = m;
}

/* chunk k: len[k] bytes from in + src[k] to out + dst[k] */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_copy_kernel(u64 n_chunks, const u64 *__restrict__ src, const u64 *__restrict__ dst,
		    const u64 *__restrict__ len, const u8 *__restrict__ in, u8 *__restrict__ out)
{
	for (u64 k = blockIdx.x; k < n_chunks; k += gridDim.x) {
		const u64 l = len[k];	/* (uniform) */
		if (l)
			copy_span(in + src[k], out + dst[k], l, threadIdx.x);
	}
}

/*
 * One workgroup behind the decode (batch_res NULL: nothing was decoded - the
 * index call, whose per-entry results stay the pre-decode ones): results[k] of
 * every entry, result[0] the verdict - the pre-decode one, else the result of
 * the first entry in directory order that did not succeed -, [1] entries (the
 * stated count under MORE_ENTRIES, the candidates under MORE_CANDIDATES), [2]
 * cd_off, [3] bytes of output needed, [4] flags.  zs NULL: the file is too
 * short to hold an end record, which is BAD_DATA.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_final_kernel(u64 max_entries, u64 out_avail, const u64 *__restrict__ zs,
		     const u32 *__restrict__ state, const u64 *__restrict__ k_at, u64 cap,
		     const u64 *__restrict__ total_at, const u64 *__restrict__ meta,
		     const u64 *__restrict__ in_n, const s32 *__restrict__ batch_res,
		     const u64 *__restrict__ actual_in, const u32 *__restrict__ crcs,
		     s32 *__restrict__ results, u64 *__restrict__ result)
{
	__shared__ unsigned long long first;	/* entry << 32 | its result */
	const u32 tid = threadIdx.x;

	if (!zs) {
		if (tid < LDA_ZIP_RESULT_WORDS)
			result[tid] = tid == 0 ? LDA_BAD_DATA : 0;
		return;
	}
	const u64 K = *k_at, total = *total_at, entries = zs[LDA_ZS_ENTRIES];
	const u32 pre = pre_status(zs, state, K, cap, max_entries, total, out_avail);

	if (tid == 0)
		first = ~0ull;
	__syncthreads();
	if (pre == LDA_SUCCESS)
		for (u64 k = tid; k < entries; k += 256) {
			s32 r;
			if (batch_res) {
				r = entry_result(meta[k], batch_res[k], actual_in[k], in_n[k], crcs[k]);
				results[k] = r;
			} else {
				r = (s32)((meta[k] >> 32) & 0xFF);
			}
			if (r != LDA_SUCCESS)
				atomicMin(&first, (unsigned long long)(k << 32 | (u32)r));
		}
	__syncthreads();
	if (tid == 0) {
		const bool known = pre == LDA_SUCCESS || pre == LDA_INSUFFICIENT_SPACE;
		result[0] = pre != LDA_SUCCESS ? pre : first != ~0ull ? (u32)first : LDA_SUCCESS;
		result[1] = known || pre == LDA_ZIP_MORE_ENTRIES ? entries :
			    pre == LDA_ZIP_MORE_CANDIDATES ? K : 0;
		result[2] = known ? zs[LDA_ZS_CD_OFF] : 0;
		result[3] = known ? total : 0;
		result[4] = known ? zs[LDA_ZS_FLAGS] : 0;
	}
}

/* libdeflate_amd_zip_read_batch: results[r] of selection r */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_rfinal_kernel(u64 n_sel, const u64 *__restrict__ meta, const u64 *__restrict__ in_n,
		      const s32 *__restrict__ batch_res, const u64 *__restrict__ actual_in,
		      const u32 *__restrict__ crcs, s32 *__restrict__ results)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r < n_sel)
		results[r] = entry_result(meta[r], batch_res[r], actual_in[r], in_n[r], crcs[r]);
}
