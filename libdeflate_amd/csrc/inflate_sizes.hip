/*
 * inflate_sizes.hip - the uncompressed size of every stream of a batch,
 * without decoding it: what a caller of the decompress calls has to know in
 * advance and a raw DEFLATE or zlib stream does not state (a gzip footer
 * states it modulo 2^32 and nothing vouches for it).
 *
 * lda_inflate_sizes_kernel is lda_inflate_wave_kernel (inflate_kernel.hip)
 * with the COUNT mode of its decoder: a wave per stream, persistent grid, the
 * same scrambled first stream and dynamic hand-out, the same inflate_block()
 * and par_round() - so headers, code rules, the overread rule, the limit and
 * the distance rule give the verdicts the decode gives - and nothing of what
 * produces bytes.  A round is its sync passes alone: every lane counts the
 * bytes of its piece and notes how far back its matches reach, a scan of the
 * counts places the lanes, and the round is valid when no match reaches
 * before the stream (or its dictionary).  There is no token row to write, no
 * group to resolve, no output mirror; stored blocks are skipped by LEN.
 * lane 0's sequential decoder (headers, the ends of a stream, every error
 * path) adds lengths where the decode copies.
 *
 * The kernel reads the input and writes results[], actual_in[] and
 * out_nbytes[]: it has no output buffer and no token scratch to be handed.
 * LDS per wave: the stream's tables and the staged input span of a round
 * (lda_inflate_sizes_lds_bytes()); the host sizes the grid by it and by the
 * kernel's register count (host_sizes.hip).
 *
 * This translation unit is built like the other inflate ones (Makefile,
 * NOLICM); inflate_kernel.o and inflate_stream.o do not change with it.
 */
#define LDA_INFLATE_DEVICE_ONLY
#include "inflate_kernel.hip"

/* waves per SIMD the register budget is set for (512 VGPRs per SIMD lane) */
#ifndef SIZES_WAVES_PER_SIMD
#define SIZES_WAVES_PER_SIMD 4
#endif
#define SIZES_STAGE_BYTES ((PAR_SPAN + 15u) & ~15u)
static_assert(SIZES_STAGE_BYTES <= PAR_STAGE_BYTES,
	      "the count mode's LDS is the decode's less the mirror, the copy scratch and the token map");

extern "C" __global__ void __launch_bounds__(64, SIZES_WAVES_PER_SIMD)
lda_inflate_sizes_kernel(u64 n_chunks, int format,
			 u32 par,	/* 0: lane 0's sequential decoder alone (LDA_INFLATE_PAR=0) */
			 u32 *__restrict__ next_stream,
			 const u32 *__restrict__ order,
			 const u8 *__restrict__ in_base,
			 const u64 *__restrict__ in_offsets,
			 const u64 *__restrict__ in_nbytes,
			 const u64 *__restrict__ limits,	/* NULL: LDA_SIZE_LIMIT_MAX */
			 s32 *__restrict__ results,
			 u64 *__restrict__ actual_in,		/* may be NULL */
			 u64 *__restrict__ out_nbytes,
			 u32 dict_len, const u32 *__restrict__ dict_id)
{
	lu8 *lds_raw = (lu8 *)(uintptr_t)0;

	/* (the order of the streams: see lda_inflate_wave_kernel) */
	u32 first = blockIdx.x;
	if (gridDim.x > 1) {
		const u32 m = (2u << (31 - __builtin_clz(gridDim.x - 1))) - 1;
		do
			first = (first ^ (first >> 3) ^ (first >> 6) ^ (first >> 9)) & m;
		while (first >= gridDim.x);
	}
	for (u64 blk = first; blk < n_chunks;) {
		inflate_block(order ? order[blk] : blk, lds_raw, par, NULL, n_chunks, format, 1,
			      in_base, in_offsets, in_nbytes, NULL, NULL, limits, results,
			      actual_in, out_nbytes, NULL, dict_len, dict_id, true);
		wave_sync();
		u32 nx = 0;
		if (lane_id() == 0)
			nx = atomicAdd(next_stream, 1u);
		blk = (u64)gridDim.x + bcast_first(nx);
	}
}

/* LDS bytes per wave: tables, the length / distance tables, the staged span */
extern "C" size_t lda_inflate_sizes_lds_bytes(void)
{
	return sizeof(struct stream_lds) + sizeof(struct shared_lds) + SIZES_STAGE_BYTES;
}

/* per-stream descriptors of libdeflate_amd_decompress_batch_packed(): the
 * sizes are known, the slots placed (offsets[] and block_sums[] of the scan,
 * compact_kernels.hip).  A stream that failed the size query or does not fit
 * the buffer is handed to the decode as an empty input with no room - the
 * decode reads and writes nothing for it - and keeps its verdict. */
extern "C" __global__ void
lda_packed_desc_kernel(u64 n, u64 capacity, const u64 *__restrict__ in_nbytes,
		       const u64 *__restrict__ sizes, const u64 *__restrict__ block_sums,
		       u64 *__restrict__ offsets, s32 *__restrict__ verdict,
		       u64 *__restrict__ dec_in_nbytes, u64 *__restrict__ dec_avail)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;

	if (i > n)
		return;
	const u64 off = offsets[i] + block_sums[i / LDA_SCAN_BLOCK];
	offsets[i] = off;	/* (entry n: the total) */
	if (i == n)
		return;
	s32 v = verdict[i];
	if (v == LDA_SUCCESS && (off > capacity || sizes[i] > capacity - off))
		v = LDA_INSUFFICIENT_SPACE;
	verdict[i] = v;
	dec_in_nbytes[i] = v == LDA_SUCCESS ? in_nbytes[i] : 0;
	dec_avail[i] = v == LDA_SUCCESS ? sizes[i] : 0;
}

/* sizes rounded up to the slots' alignment (a power of two), for the scan;
 * entry n is 0 so that the scan's entry n is the total */
extern "C" __global__ void
lda_packed_round_kernel(u64 n, u64 align_mask, const u64 *__restrict__ sizes,
			u64 *__restrict__ rounded)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;

	if (i <= n)
		rounded[i] = i < n ? (sizes[i] + align_mask) & ~align_mask : 0;
}

/* after the decode: streams that were not decoded keep the size query's
 * verdict; the others have the decode's.  A stream that did not succeed
 * reports 0 / 0 (the decode batch leaves the raw decoder's figures behind a
 * checksum that does not match). */
extern "C" __global__ void
lda_packed_merge_kernel(u64 n, const s32 *__restrict__ verdict, s32 *__restrict__ results,
			u64 *__restrict__ actual_in, u64 *__restrict__ actual_out)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;

	if (i >= n)
		return;
	if (verdict[i] != LDA_SUCCESS)
		results[i] = verdict[i];
	else if (results[i] == LDA_SUCCESS)
		return;
	if (actual_in)
		actual_in[i] = 0;
	actual_out[i] = 0;
}
