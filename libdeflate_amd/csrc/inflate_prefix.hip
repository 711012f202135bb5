/*
 * inflate_prefix.hip - the first bytes of every stream of a batch: what
 * zlib's inflate() gives with avail_out below the stream's size and the
 * reference's whole-buffer calls answer with LIBDEFLATE_INSUFFICIENT_SPACE and
 * an undefined buffer.
 *
 * lda_inflate_prefix_kernel is lda_inflate_wave_kernel (inflate_kernel.hip)
 * with the PREFIX mode of its decoder: a wave per stream, persistent grid, the
 * same scrambled first stream and dynamic hand-out, the same token rows and
 * LDS layout, the same inflate_block() and par_round().  A parallel round that
 * would cross a stream's limit is clipped to the lanes whose bytes fit (in
 * this unit alone: PAR_OK_LIMIT in inflate_kernel.hip) and ends the stream's
 * rounds; lane 0's sequential decoder walks the rest token by token, less
 * than one lane's piece, and there the token that does not fit is cut (see
 * inflate_block()): the
 * stream ends as LDA_PREFIX with exactly its limit written, and no store of
 * any width touches the byte at the limit or beyond.  A stream that ends
 * within its limit takes the unchanged LDA_SUCCESS path, footer check
 * included (lda_inflate_finalize_kernel skips every other row).
 *
 * `par` is an argument as in the size query: 0 (LDA_INFLATE_PAR=0) leaves the
 * whole stream to lane 0's sequential decoder.  That decoder does not split
 * its short copies into loads now and stores at the next token here
 * (PREFIX_NO_PENDING in inflate_block()): the registers this takes are what
 * the wave kernel spills, and this kernel spills none.
 *
 * lda_gzm_peek_desc_kernel (at the end) makes the descriptors of such a batch
 * from the device index of a gzip-members file, as inflate_sizes.hip holds
 * the descriptor kernels of the packed decode.
 *
 * This translation unit is built like the other inflate ones (Makefile,
 * NOLICM); inflate_kernel.o, inflate_sizes.o and inflate_stream.o do not
 * change with it.
 */
#define LDA_INFLATE_DEVICE_ONLY
#define LDA_INFLATE_PREFIX 1
#include "inflate_kernel.hip"

/* four waves per SIMD, 16 streams in flight per CU, as the wave kernel: the
 * host launches the decode batch's grid, LDS and token scratch (PAR_SCRATCH
 * words per wave; host_prefix.hip) */
extern "C" __global__ void __launch_bounds__(64, 4)
lda_inflate_prefix_kernel(u64 n_chunks, int format,
			  u32 par,	/* 0: lane 0's sequential decoder alone (LDA_INFLATE_PAR=0) */
			  u32 *__restrict__ tokscratch,
			  u32 *__restrict__ next_stream,
			  const u32 *__restrict__ order,
			  const u8 *__restrict__ in_base,
			  const u64 *__restrict__ in_offsets,
			  const u64 *__restrict__ in_nbytes,
			  u8 *__restrict__ out_base,
			  const u64 *__restrict__ out_offsets,
			  const u64 *__restrict__ limits,
			  s32 *__restrict__ results,
			  u64 *__restrict__ actual_in,
			  u64 *__restrict__ actual_out,
			  const u8 *__restrict__ dict, u32 dict_len,
			  const u32 *__restrict__ dict_id)
{
	lu8 *lds_raw = (lu8 *)(uintptr_t)0;
	u32 *tok = tokscratch + (size_t)blockIdx.x * PAR_SCRATCH;

	/* (the order of the streams: see lda_inflate_wave_kernel) */
	u32 first = blockIdx.x;
	if (gridDim.x > 1) {
		const u32 m = (2u << (31 - __builtin_clz(gridDim.x - 1))) - 1;
		do
			first = (first ^ (first >> 3) ^ (first >> 6) ^ (first >> 9)) & m;
		while (first >= gridDim.x);
	}
	for (u64 blk = first; blk < n_chunks;) {
		inflate_block(order ? order[blk] : blk, lds_raw, par, tok, n_chunks, format, 1,
			      in_base, in_offsets, in_nbytes, out_base, out_offsets, limits,
			      results, actual_in, actual_out, dict, dict_len, dict_id);
		wave_sync();
		u32 nx = 0;
		if (lane_id() == 0)
			nx = atomicAdd(next_stream, 1u);
		blk = (u64)gridDim.x + bcast_first(nx);
	}
}

/*
 * The heads of the members (libdeflate_amd_gzip_members_peek_batch): rows
 * r < result[1] of an index that lies in device memory become the descriptors
 * of a prefix batch - member r is [index[2r], index[2r + 2]), its limit `head`,
 * its place r * head.  The rows at and beyond the member count are empty (no
 * input, no room: the decode reads and writes nothing for them), and so are
 * all rows unless result[0] is LDA_SUCCESS: under every other verdict of the
 * index call the index is not written.  The words come from memory the caller
 * owns: a pair that does not lie inside the file makes an empty row too.
 * Launched again behind the batch, with its answers (results != NULL): the
 * empty rows, which the decode refused as streams without a header, report
 * nothing - result 0, 0 bytes.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_gzm_peek_desc_kernel(u64 max_members, u64 n, u64 head, const u64 *__restrict__ result,
			 const u64 *__restrict__ index, u64 *__restrict__ in_off,
			 u64 *__restrict__ in_n, u64 *__restrict__ out_off, u64 *__restrict__ limits,
			 s32 *__restrict__ results, u64 *__restrict__ head_nbytes)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= max_members)
		return;
	if (results) {
		if (in_n[r] == 0) {
			results[r] = LDA_SUCCESS;
			head_nbytes[r] = 0;
		}
		return;
	}
	u64 at = 0, len = 0;
	if (result[0] == LDA_SUCCESS && r < result[1]) {
		const u64 a = index[2 * r], b = index[2 * r + 2];
		if (a < b && b <= n) {
			at = a;
			len = b - a;
		}
	}
	in_off[r] = at;
	in_n[r] = len;
	out_off[r] = len ? r * head : 0;
	limits[r] = len ? head : 0;
}
