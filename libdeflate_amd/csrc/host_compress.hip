/*
 * host_compress.hip - C-ABI of the compressor: object lifetime, level table,
 * compress_bound, the device batch entry point, the host-pointer batch and
 * the three single-buffer libdeflate_*_compress calls as batches of one.
 *
 * Reference interfaces replaced: libdeflate.h:59-67 (alloc), :85-152
 * (compress + bounds), :159-160 (free).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <new>
#include <algorithm>
#include <vector>

#include "host_objects.h"
#include "kernels.h"
#include "large_plan.h"
#include "compress_plan.h"
#include "deflate_levels.h"

using namespace lda;

/* level -> (search depth, nice length, parse mode): the rows of deflate_levels.h */
struct level_cfg { uint32_t depth, nice, mode; };	/* mode: 0 greedy, 1 lazy, 2 lazy2, 3 min-cost */
static const level_cfg k_levels[13] = {
	{ LDA_LEVEL_0 }, { LDA_LEVEL_1 }, { LDA_LEVEL_2 }, { LDA_LEVEL_3 }, { LDA_LEVEL_4 },
	{ LDA_LEVEL_5 }, { LDA_LEVEL_6 }, { LDA_LEVEL_7 }, { LDA_LEVEL_8 }, { LDA_LEVEL_9 },
	{ LDA_LEVEL_10 }, { LDA_LEVEL_11 }, { LDA_LEVEL_12 },
};

/*
 * The LZ77 stage of the split path by level: the instance built for the level
 * (deflate_l<N>.hip: the level's row above as constants), or the
 * generic kernel, which reads the row from its arguments - level 0, a level
 * whose instance measured no faster (none listed here), LDA_COMPRESS_SPECIALIZE=0,
 * and the profiling build, whose phase counters are the generic kernel's.
 */
struct lz77_kernel { lda_lz77_kernel_t fn; const char *name; };
#define LZ77_K(name) { name, #name }
static const lz77_kernel k_lz77_generic = LZ77_K(lda_deflate_batch_kernel);
static const lz77_kernel k_lz77_level[10] = {
	LZ77_K(lda_deflate_batch_kernel),
	LZ77_K(lda_deflate_batch_kernel_l1), LZ77_K(lda_deflate_batch_kernel_l2),
	LZ77_K(lda_deflate_batch_kernel_l3), LZ77_K(lda_deflate_batch_kernel_l4),
	LZ77_K(lda_deflate_batch_kernel_l5), LZ77_K(lda_deflate_batch_kernel_l6),
	LZ77_K(lda_deflate_batch_kernel_l7), LZ77_K(lda_deflate_batch_kernel_l8),
	LZ77_K(lda_deflate_batch_kernel_l9),
};
#undef LZ77_K

static const lz77_kernel &lz77_kernel_of(int level)
{
#ifdef LDA_PROFILE
	return k_lz77_generic;
#else
	return env_cfg().compress_specialize && level >= 1 && level <= 9 ?
	       k_lz77_level[level] : k_lz77_generic;
#endif
}

extern "C" LIBDEFLATEAPI struct libdeflate_compressor *
libdeflate_alloc_compressor_ex(int level, const struct libdeflate_options *options)
{
	malloc_func_t m;
	free_func_t f;

	if (!pick_allocator(options, &m, &f))
		return NULL;
	if (level == -1)	/* libdeflate.h:47 */
		level = 6;
	if (level < 0 || level > 12)
		return NULL;
	if (!device_ctx()) {
		fprintf(stderr, "libdeflate_amd: alloc_compressor: no usable "
			"gfx950 device (%s); no CPU fallback\n",
			libdeflate_amd_last_error());
		return NULL;
	}
	void *mem = m(sizeof(struct libdeflate_compressor));
	if (!mem)
		return NULL;
	struct libdeflate_compressor *c = new (mem) libdeflate_compressor();
	c->free_func = f;
	c->malloc_func = m;
	c->level = level;
	c->device = 0;
	(void)hipGetDevice(&c->device);	/* (device_ctx() above has seen it work) */
	for (int k = 0; k < LDA_MAX_SHARDS; k++)
		c->shard[k] = NULL;
	return c;
}

extern "C" LIBDEFLATEAPI struct libdeflate_compressor *
libdeflate_alloc_compressor(int level)
{
	return libdeflate_alloc_compressor_ex(level, NULL);
}

extern "C" LIBDEFLATEAPI void
libdeflate_free_compressor(struct libdeflate_compressor *c)
{
	if (!c)
		return;
	for (int k = 0; k < LDA_MAX_SHARDS; k++)
		libdeflate_free_compressor(c->shard[k]);
	DeviceGuard on(c->device);
	c->scratch.release();
	c->stage.release();
	c->pinned.release();
	c->meta.release();
	c->bgzf.release();
	c->large.release();
	c->zipw.release();
	c->zipw_up.release();
	c->streams.release();
	c->side.release();	/* (idle: freeing the scratch has waited for the device) */
	free_func_t f = c->free_func;
	c->~libdeflate_compressor();
	f(c);
}

/* lib/deflate_compress.c:4087-4135: 5 bytes per 5000-byte worst-case block */
extern "C" LIBDEFLATEAPI size_t
libdeflate_deflate_compress_bound(struct libdeflate_compressor *c, size_t n)
{
	(void)c;
	size_t blocks = (n + 4999) / 5000;
	if (blocks < 1)
		blocks = 1;
	return 5 * blocks + n;
}

/* lib/zlib_compress.c:76-82 */
extern "C" LIBDEFLATEAPI size_t
libdeflate_zlib_compress_bound(struct libdeflate_compressor *c, size_t n)
{
	return 6 + libdeflate_deflate_compress_bound(c, n);
}

/* lib/gzip_compress.c:84-90 */
extern "C" LIBDEFLATEAPI size_t
libdeflate_gzip_compress_bound(struct libdeflate_compressor *c, size_t n)
{
	return 18 + libdeflate_deflate_compress_bound(c, n);
}

/*
 * Preset dictionaries: the compress kernel's ring holds W bytes ahead of a
 * buffer - 32 KiB minus two tiles (the kernel inserts one tile ahead) and the
 * lookahead, in whole tiles (20 KiB).  A dictionary of `tail` = min(dict, W)
 * bytes takes tail rounded up to whole tiles; the unused bytes in front of it
 * are never a match source.
 */
static size_t dict_window(void)
{
	const size_t tile = lda_deflate_tile();
	return (32768 - 2 * tile - 272) / tile * tile;
}

struct dict_shape { uint32_t tail, pre_len, sinfo; };

static dict_shape shape_dict(int level, size_t dict_nbytes)
{
	const size_t tile = lda_deflate_tile();
	dict_shape d;
	/* (level 0 stores: the dictionary only changes the zlib header) */
	d.tail = level == 0 ? 0 : (uint32_t)std::min(dict_nbytes, dict_window());
	d.pre_len = (uint32_t)((d.tail + tile - 1) / tile * tile);
	d.sinfo = d.pre_len | ((d.pre_len - d.tail) << 16) | 0x80000000u;
	return d;
}

/*
 * The plan of a batch call (compress_plan.h) for this compressor on its device.
 * The LZ77 launch's tail: a persistent grid that hands buffers out from a
 * counter ends spread over one buffer's time, about half a buffer of idle CU
 * at the end of every launch (estimated 0.18 ms of the bench batch's 5.81, 3 %;
 * measured: 0.14 ms x 256 CUs of entropy work run inside it, the step ends
 * 0.09 ms earlier - DESIGN 3.3, profiles/r15_overlap.md).  The split path therefore runs a slice as a head on the
 * caller's stream and a tail of R buffers per CU on the compressor's own:
 *
 *   caller's:  memset, checksums - in - K_head - E_head ------- wait tail - F
 *   side:                     wait in - K_tail - E_tail - tail
 *
 * K_tail's workgroups take the CUs K_head's leave, E_head's the CUs K_tail's
 * leave; stream order and the two events are the only hand-overs.  The entropy
 * stage as a whole cannot be hidden: LZ77 needs 5.81 x 256 CU-ms and the
 * entropy stage 0.42 x 256 CU-ms, they cannot share a CU (157 of 160 KiB of
 * LDS against 4 x 20 KiB), so only the tail is there to win.  `overlap` false:
 * the serial schedule (LDA_COMPRESS_OVERLAP=0, or no side stream).
 */
static batch_plan plan_batch(const struct libdeflate_compressor *c, size_t n,
			     size_t max_in, bool seg, bool dict, bool overlap = true)
{
	static_assert(LDA_PLAN_BLK_WORDS == LDA_BLK_WORDS && LDA_PLAN_BLK_LIST(17) == LDA_BLK_LIST(17) &&
		      LDA_PLAN_BLK_HDR_WORDS(17) == LDA_BLK_HDR_WORDS(17), "compress_plan.h, kernels.h");
	const EnvCfg &env = env_cfg();
	compress_plan_env e;
	e.num_cus = (size_t)device_ctx()->num_cus;
	e.small_max = lda_deflate_small_max();
	e.small_wgs = lda_deflate_small_wgs();
	e.no_small = env.no_small;
	e.tile = lda_deflate_tile();
	e.seq_words = lda_deflate_seq_words();
	e.dict_bytes = LDA_DICT_BLK_HDR + dict_window();
	e.tail_rounds = !overlap || !env.compress_overlap || c->side.failed ? 0 :
			env.compress_tail_rounds ? (size_t)env.compress_tail_rounds :
			LDA_COMPRESS_TAIL_ROUNDS;
	return plan_batch(e, n, max_in, c->level, seg, dict);
}

static int
compress_batch_impl(struct libdeflate_compressor *c, int format, size_t n,
		    const void *d_in, const uint64_t *d_in_offsets,
		    const uint64_t *d_in_nbytes, void *d_out,
		    const uint64_t *d_out_offsets, const uint64_t *d_out_avail,
		    uint64_t *d_out_nbytes, void *stream,
		    const uint32_t *d_seg_info, size_t max_in_nbytes = SIZE_MAX,
		    const void *d_dict = NULL, size_t dict_nbytes = 0)
{
	if (!c) {
		set_error("compress_batch: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(c->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *ctx = device_ctx();
	hipStream_t st = (hipStream_t)stream;

	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (n == 0)
		return LIBDEFLATE_AMD_OK;
	if (!c || !d_in || !d_in_offsets || !d_in_nbytes || !d_out ||
	    !d_out_offsets || !d_out_avail || !d_out_nbytes ||
	    format < LIBDEFLATE_AMD_DEFLATE || format > LIBDEFLATE_AMD_BGZF) {
		set_error("compress_batch: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	const bool dict = d_dict && dict_nbytes;
	batch_plan pl = plan_batch(c, n, max_in_nbytes, d_seg_info != NULL, dict);
	/* no side stream (once: SideStream::failed): the serial schedule */
	if (pl.overlap && !c->side.ensure())
		pl = plan_batch(c, n, max_in_nbytes, d_seg_info != NULL, dict, false);
	const bool small = pl.small;
	c->last_schedule[0] = pl.split;
	c->last_schedule[1] = 0;
	c->last_schedule[2] = (uint32_t)std::min<size_t>(n, 0xFFFFFFFFu);
	c->last_schedule[3] = 0;
	c->last_kernel = "";
	uint8_t *scr = (uint8_t *)c->scratch.reserve(pl.total);
	if (!scr)
		return LIBDEFLATE_AMD_OOM;
	uint32_t *next_chunk = (uint32_t *)(scr + pl.cnt_at);
	/* (the tail's counters lie behind the head's: cnt2_at) */
	LDA_HIP_TRY(hipMemsetAsync(next_chunk, 0, (pl.overlap ? 32 : 16) * pl.nslices, st),
		    LIBDEFLATE_AMD_NO_DEVICE);
	uint8_t *blk = NULL;
	if (dict) {
		/* the prefix every buffer starts from and, for zlib, the DICTID:
		 * both on the device, nothing waits */
		const dict_shape sh = shape_dict(c->level, dict_nbytes);
		blk = scr + pl.dict_at;
		hipLaunchKernelGGL(lda_dict_prep_kernel, dim3(1), dim3(256), 0, st,
				   (const uint8_t *)d_dict, (uint64_t)dict_nbytes, sh.tail,
				   sh.pre_len, sh.sinfo, blk);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		if (format == LIBDEFLATE_AMD_ZLIB) {
			int rc = libdeflate_amd_adler32_batch(1, d_dict, (const uint64_t *)(blk + 16),
							      (const uint64_t *)(blk + 24), NULL,
							      (uint32_t *)(blk + 4), stream);
			if (rc != LIBDEFLATE_AMD_OK)
				return rc;
		}
	}
	uint32_t *sums = NULL;
	if (format != LIBDEFLATE_AMD_DEFLATE) {
		sums = (uint32_t *)(scr + pl.sums_at);
		int rc = format == LIBDEFLATE_AMD_GZIP || format == LIBDEFLATE_AMD_BGZF ?
			libdeflate_amd_crc32_batch(n, d_in, d_in_offsets,
						   d_in_nbytes, NULL, sums, stream) :
			libdeflate_amd_adler32_batch(n, d_in, d_in_offsets,
						     d_in_nbytes, NULL, sums, stream);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	const size_t lds = small ? lda_deflate_small_lds_bytes() : lda_deflate_lds_bytes();
	if (!ctx->deflate_attr_set.load(std::memory_order_acquire)) {
		LDA_HIP_TRY(hipFuncSetAttribute(
				(const void *)lda_deflate_small_kernel,
				hipFuncAttributeMaxDynamicSharedMemorySize,
				(int)lda_deflate_small_lds_bytes()), LIBDEFLATE_AMD_NO_DEVICE);
		LDA_HIP_TRY(hipFuncSetAttribute(
				(const void *)lda_deflate_batch_kernel,
				hipFuncAttributeMaxDynamicSharedMemorySize,
				(int)lda_deflate_lds_bytes()), LIBDEFLATE_AMD_NO_DEVICE);
		LDA_HIP_TRY(hipFuncSetAttribute(
				(const void *)lda_deflate_opt_kernel,
				hipFuncAttributeMaxDynamicSharedMemorySize,
				(int)lda_deflate_lds_bytes()), LIBDEFLATE_AMD_NO_DEVICE);
		LDA_HIP_TRY(hipFuncSetAttribute(
				(const void *)lda_deflate_fused_kernel,
				hipFuncAttributeMaxDynamicSharedMemorySize,
				(int)lda_deflate_lds_bytes()), LIBDEFLATE_AMD_NO_DEVICE);
		for (int l = 1; l <= 9; l++)
			LDA_HIP_TRY(hipFuncSetAttribute(
					(const void *)k_lz77_level[l].fn,
					hipFuncAttributeMaxDynamicSharedMemorySize,
					(int)lda_deflate_lds_bytes()), LIBDEFLATE_AMD_NO_DEVICE);
		ctx->deflate_attr_set.store(true, std::memory_order_release);
	}
	const level_cfg &lv = k_levels[c->level];
	if (!pl.split && (small || lv.mode == 3)) {
		c->last_kernel = small ? "lda_deflate_small_kernel" : "lda_deflate_opt_kernel";
		hipLaunchKernelGGL(small ? lda_deflate_small_kernel : lda_deflate_opt_kernel,
				   dim3((unsigned)pl.grid),
				   dim3(small ? LDA_DEFLATE_SMALL_THREADS : LDA_DEFLATE_THREADS),
				   lds, st, (uint64_t)n, format, c->level,
				   lv.depth, lv.nice, lv.mode, (const uint8_t *)d_in,
				   d_in_offsets, d_in_nbytes, (uint8_t *)d_out,
				   d_out_offsets, d_out_avail, d_out_nbytes, sums,
				   (uint64_t *)scr, d_seg_info, next_chunk, (const uint8_t *)blk);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	if (!pl.split) {
		c->last_kernel = "lda_deflate_fused_kernel";
		hipLaunchKernelGGL(lda_deflate_fused_kernel, dim3((unsigned)pl.grid),
				   dim3(LDA_DEFLATE_THREADS), lds, st, (uint64_t)n, format,
				   c->level, lv.depth, lv.nice, lv.mode, (const uint8_t *)d_in,
				   d_in_offsets, d_in_nbytes, (uint8_t *)d_out,
				   d_out_offsets, d_out_avail, d_out_nbytes, sums,
				   (uint64_t *)scr, d_seg_info, next_chunk, (const uint8_t *)blk,
				   (const uint32_t *)NULL, (const uint32_t *)NULL);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	/* the split path, slice by slice: the LZ77 stage leaves tokens and block
	 * descriptors, the entropy kernel writes the streams, and the fused
	 * kernel compresses the buffers larger than the bound (the bound is a
	 * promise the host cannot check; what such a buffer gets does not depend
	 * on which path its batch took).  Stream order is the only hand-over:
	 * within a part on its stream, and through the two events between the
	 * head on the caller's stream and the tail on the object's (plan_batch()).
	 * A part is a batch of its own to the kernels: its rows of the caller's
	 * arrays, its token lists, block descriptors, counters and workgroup
	 * state.  The slices stay in series, they share the scratch. */
	uint32_t *tok = (uint32_t *)(scr + pl.tok_at);
	struct part {
		size_t lo, n;
		uint32_t *tok, *bd;
		/* its counters of this slice; the fused kernel's, the count of buffers
		 * listed for that one and the entropy kernel's lie nslices, 2 nslices
		 * and 3 nslices words behind the LZ77 stage's */
		uint32_t *cnt;
		uint64_t *seq;
		size_t grid_max;
	};
	const lz77_kernel &lz77 = lz77_kernel_of(c->level);
	c->last_kernel = lz77.name;
	auto lz77_entropy = [&](const part &q, hipStream_t on) -> int {
		const uint32_t *sk = sums ? sums + q.lo : NULL;
		const uint32_t *gk = d_seg_info ? d_seg_info + q.lo : NULL;
		hipLaunchKernelGGL(lz77.fn, dim3((unsigned)std::min(q.n, q.grid_max)),
				   dim3(LDA_DEFLATE_THREADS), lds, on, (uint64_t)q.n, format,
				   c->level, lv.depth, lv.nice, lv.mode, (const uint8_t *)d_in,
				   d_in_offsets + q.lo, d_in_nbytes + q.lo, (uint8_t *)d_out,
				   d_out_offsets + q.lo, d_out_avail + q.lo, d_out_nbytes + q.lo, sk,
				   q.seq, gk, q.cnt, (const uint8_t *)NULL,
				   q.tok, q.bd, pl.tok_stride, pl.blk_stride, q.cnt + 2 * pl.nslices);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		hipLaunchKernelGGL(lda_deflate_entropy_kernel, dim3((unsigned)q.n),
				   dim3(LDA_DEFLATE_ENTROPY_THREADS), lda_deflate_entropy_lds_bytes(),
				   on, (uint64_t)q.n, format, c->level, (const uint8_t *)d_in,
				   d_in_offsets + q.lo, d_in_nbytes + q.lo, (uint8_t *)d_out,
				   d_out_offsets + q.lo, d_out_avail + q.lo, d_out_nbytes + q.lo, sk, gk,
				   (const uint32_t *)q.tok, (const uint32_t *)q.bd, pl.tok_stride,
				   pl.blk_stride, q.cnt + 3 * pl.nslices);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	};
	/* (on the caller's stream for both parts: one launch after the other, so
	 * they share the head's workgroup state) */
	auto fused = [&](const part &q) -> int {
		const uint32_t *sk = sums ? sums + q.lo : NULL;
		const uint32_t *gk = d_seg_info ? d_seg_info + q.lo : NULL;
		hipLaunchKernelGGL(lda_deflate_fused_kernel, dim3((unsigned)std::min(q.n, pl.grid)),
				   dim3(LDA_DEFLATE_THREADS), lds, st, (uint64_t)q.n, format,
				   c->level, lv.depth, lv.nice, lv.mode, (const uint8_t *)d_in,
				   d_in_offsets + q.lo, d_in_nbytes + q.lo, (uint8_t *)d_out,
				   d_out_offsets + q.lo, d_out_avail + q.lo, d_out_nbytes + q.lo, sk,
				   (uint64_t *)scr, gk, q.cnt + pl.nslices,
				   (const uint8_t *)NULL, (const uint32_t *)q.bd,
				   (const uint32_t *)(q.cnt + 2 * pl.nslices));
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	};
	size_t heads = 0, tails = 0;
	for (size_t k = 0; k < pl.nslices; k++) {
		const size_t lo = k * pl.per_slice, nk = std::min(pl.per_slice, n - lo);
		const size_t tail_n = plan_tail_of(nk, (size_t)ctx->num_cus, pl.tail_rounds);
		const size_t head_n = nk - tail_n;
		const part head = { lo, head_n, tok, (uint32_t *)(scr + pl.blk_at), next_chunk + k,
				    (uint64_t *)scr, pl.grid };
		const part tail = { lo + head_n, tail_n, tok + head_n * (size_t)pl.tok_stride,
				    (uint32_t *)(scr + pl.blk2_at),
				    (uint32_t *)(scr + pl.cnt2_at) + k,
				    (uint64_t *)(scr + pl.seq2_at), pl.grid2 };
		heads += head_n;
		tails += tail_n;
		if (tail_n) {
			LDA_HIP_TRY(hipEventRecord(c->side.in, st), LIBDEFLATE_AMD_NO_DEVICE);
			LDA_HIP_TRY(hipStreamWaitEvent(c->side.side, c->side.in, 0),
				    LIBDEFLATE_AMD_NO_DEVICE);
		}
		LDA_OK_TRY(lz77_entropy(head, st));
		if (tail_n) {
			/* whatever happens to the tail's launches, the caller's stream
			 * waits for what the side stream was given */
			const int rc = lz77_entropy(tail, c->side.side);
			LDA_HIP_TRY(hipEventRecord(c->side.tail, c->side.side), LIBDEFLATE_AMD_NO_DEVICE);
			LDA_HIP_TRY(hipStreamWaitEvent(st, c->side.tail, 0), LIBDEFLATE_AMD_NO_DEVICE);
			LDA_OK_TRY(rc);
		}
		LDA_OK_TRY(fused(head));
		if (tail_n)
			LDA_OK_TRY(fused(tail));
	}
	c->last_schedule[1] = tails != 0;
	c->last_schedule[2] = (uint32_t)std::min<size_t>(heads, 0xFFFFFFFFu);
	c->last_schedule[3] = (uint32_t)std::min<size_t>(tails, 0xFFFFFFFFu);
	return LIBDEFLATE_AMD_OK;
}

/* include/libdeflate_amd.h */
extern "C" LIBDEFLATEAPI void
libdeflate_amd_compress_last_schedule(const struct libdeflate_compressor *c, uint32_t out[4])
{
	for (int i = 0; i < 4; i++)
		out[i] = c ? c->last_schedule[i] : 0;
}

/* include/libdeflate_amd.h */
extern "C" LIBDEFLATEAPI const char *
libdeflate_amd_compress_last_kernel(const struct libdeflate_compressor *c)
{
	return c ? c->last_kernel : "";
}

/* host_objects.h: what the writers' piece pipeline (host_write_pieces.hip) launches
 * its pieces through */
int lda::compress_deflate_pieces(struct libdeflate_compressor *c, size_t n, const void *d_in,
				 const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
				 void *d_out, const uint64_t *d_out_offsets,
				 const uint64_t *d_out_avail, uint64_t *d_out_nbytes, void *stream,
				 const uint32_t *d_seg_info, size_t max_in)
{
	return compress_batch_impl(c, LIBDEFLATE_AMD_DEFLATE, n, d_in, d_in_offsets, d_in_nbytes,
				   d_out, d_out_offsets, d_out_avail, d_out_nbytes, stream,
				   d_seg_info, max_in);
}

size_t lda::compress_pieces_scratch(const struct libdeflate_compressor *c, size_t n,
				    size_t max_in, bool seg)
{
	return plan_batch(c, n, max_in, seg, false).total;
}

size_t lda::compress_prime_window(void)
{
	return dict_window();
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_compress_batch_dict(struct libdeflate_compressor *c, int format,
				   size_t n, const void *d_dict, size_t dict_nbytes,
				   const void *d_in, const uint64_t *d_in_offsets,
				   const uint64_t *d_in_nbytes, void *d_out,
				   const uint64_t *d_out_offsets,
				   const uint64_t *d_out_avail,
				   uint64_t *d_out_nbytes, void *stream)
{
	/* zlib refuses a dictionary on a gzip stream */
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB) {
		set_error("compress_batch_dict: format %d takes no dictionary", format);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (dict_nbytes && !d_dict) {
		set_error("compress_batch_dict: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return compress_batch_impl(c, format, n, d_in, d_in_offsets, d_in_nbytes,
				   d_out, d_out_offsets, d_out_avail,
				   d_out_nbytes, stream, NULL, SIZE_MAX, d_dict, dict_nbytes);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_compress_batch(struct libdeflate_compressor *c, int format,
			      size_t n, const void *d_in,
			      const uint64_t *d_in_offsets,
			      const uint64_t *d_in_nbytes, void *d_out,
			      const uint64_t *d_out_offsets,
			      const uint64_t *d_out_avail,
			      uint64_t *d_out_nbytes, void *stream)
{
	return compress_batch_impl(c, format, n, d_in, d_in_offsets, d_in_nbytes,
				   d_out, d_out_offsets, d_out_avail,
				   d_out_nbytes, stream, NULL);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_compress_batch_bounded(struct libdeflate_compressor *c, int format,
				      size_t n, const void *d_in,
				      const uint64_t *d_in_offsets,
				      const uint64_t *d_in_nbytes, void *d_out,
				      const uint64_t *d_out_offsets,
				      const uint64_t *d_out_avail,
				      uint64_t *d_out_nbytes, size_t max_in_nbytes,
				      void *stream)
{
	return compress_batch_impl(c, format, n, d_in, d_in_offsets, d_in_nbytes,
				   d_out, d_out_offsets, d_out_avail,
				   d_out_nbytes, stream, NULL, max_in_nbytes);
}

static int compress_batch_host_body(struct libdeflate_compressor *c, int format,
				   size_t n, const void *const *in,
				   const size_t *in_nbytes, void *const *out,
				   const size_t *out_avail, size_t *out_nbytes)
{
	if (n == 0)
		return device_ctx() ? LIBDEFLATE_AMD_OK : LIBDEFLATE_AMD_NO_DEVICE;
	if (!c || !in || !in_nbytes || !out || !out_avail || !out_nbytes) {
		set_error("compress_batch_host: NULL argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(c->device);
	if (!on.ok() || !device_ctx())
		return LIBDEFLATE_AMD_NO_DEVICE;
	/* The batch goes through in SLICES (up to 8, >= 64 MiB of input each - a
	 * slice has to fill the GPU several times over, or its kernel's tail
	 * costs more than the overlap gives: 8 MiB slices measured slower than
	 * no slices) on run_slices(): the kernels of slice k run on the object's
	 * compute stream while the host packs and sends slice k + 1 and unpacks
	 * slice k - 1 on its copy stream.
	 * device layout: [in_off in_n out_off out_av out_n][cmp_off of every
	 * slice] [inputs] [output slots] [compacted outputs, slice after slice];
	 * everything 16-byte aligned */
	enum { MAX_SLICES = 8 };
	size_t bounds[MAX_SLICES + 1];
	const size_t ns = slice_by_bytes(n, in_nbytes, MAX_SLICES, (size_t)64 << 20, bounds);
	size_t cmp_len[MAX_SLICES], cmp_pos[MAX_SLICES], ncmp = 0;
	for (size_t k = 0; k < ns; k++) {
		cmp_pos[k] = ncmp;
		cmp_len[k] = libdeflate_amd_compact_offsets_len(bounds[k + 1] - bounds[k]);
		ncmp += cmp_len[k];
	}
	std::vector<uint64_t> desc(5 * n + ncmp);
	uint64_t *in_off = &desc[0], *in_n = &desc[n], *out_off = &desc[2 * n],
		 *out_av = &desc[3 * n], *out_n = &desc[4 * n], *cmp_off = &desc[5 * n];
	size_t pos = align_up(desc.size() * 8, 64);
	for (size_t i = 0; i < n; i++) {
		in_off[i] = pos;
		in_n[i] = in_nbytes[i];
		pos = align_up(pos + in_nbytes[i] + 16, 16);
	}
	size_t total_avail = 0;
	size_t avail_before[MAX_SLICES + 1];
	for (size_t k = 0, i = 0; k < ns; k++) {
		avail_before[k] = total_avail;
		for (; i < bounds[k + 1]; i++) {
			out_off[i] = pos;
			out_av[i] = out_avail[i];
			pos = align_up(pos + out_avail[i] + 16, 16);
			total_avail += out_avail[i];
		}
	}
	const size_t cmp_at = pos;
	uint8_t *st = (uint8_t *)c->stage.reserve(cmp_at + total_avail + 64 * ns + 64);
	if (!st)
		return LIBDEFLATE_AMD_OOM;
	if (!c->streams.enter())
		return LIBDEFLATE_AMD_NO_DEVICE;
	size_t max_in = 0;
	for (size_t i = 0; i < n; i++)
		max_in = in_nbytes[i] > max_in ? in_nbytes[i] : max_in;
	/* the kernels' scratch for the largest launch up front: growing it between
	 * two slices would free memory a running kernel uses (and synchronise).
	 * Sized by the launches that are made (compress_batch_impl(): one token
	 * list per workgroup, the grid never larger than the slice) - a one-shot
	 * call on a small buffer reserves one list, not a device's worth */
	{
		size_t max_nk = 0;
		for (size_t k = 0; k < ns; k++)
			max_nk = bounds[k + 1] - bounds[k] > max_nk ? bounds[k + 1] - bounds[k] : max_nk;
		if (!c->scratch.reserve(plan_batch(c, max_nk, max_in, false, false).total))
			return LIBDEFLATE_AMD_OOM;
	}
	/* what comes back per slice (sizes, compaction offsets) lands in pinned
	 * memory, so the copies are asynchronous and the host is free to pack the
	 * next slice while this one's kernels run */
	uint64_t *h_back = (uint64_t *)c->meta.ensure((n + ncmp) * 8);
	if (!h_back)
		return LIBDEFLATE_AMD_OOM;
	out_n = h_back;
	cmp_off = h_back + n;
	hipStream_t s_copy = c->streams.copy, s_comp = c->streams.comp;
	LDA_HIP_TRY(hipMemcpyAsync(st, desc.data(), 4 * n * 8, hipMemcpyHostToDevice,
				   s_copy), LIBDEFLATE_AMD_NO_DEVICE);
	uint64_t *d_desc = (uint64_t *)st;
	auto enqueue = [&](size_t k) -> int {
		const size_t lo = bounds[k], nk = bounds[k + 1] - lo;
		/* (returns when the slice is on the device) */
		int rc = copy_in_packed(&c->pinned, st, nk, in + lo, in_nbytes + lo, in_off + lo, s_copy);
		if (rc == LIBDEFLATE_AMD_OK)
			rc = libdeflate_amd_compress_batch_bounded(
				c, format, nk, st, d_desc + lo, d_desc + n + lo, st, d_desc + 2 * n + lo,
				d_desc + 3 * n + lo, d_desc + 4 * n + lo, max_in, s_comp);
		if (rc == LIBDEFLATE_AMD_OK)
			rc = libdeflate_amd_compact_batch(nk, st, d_desc + 2 * n + lo, d_desc + 4 * n + lo,
							  st + cmp_at + avail_before[k] + 64 * k,
							  d_desc + 5 * n + cmp_pos[k], s_comp);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
		if (hipMemcpyAsync(out_n + lo, d_desc + 4 * n + lo, nk * 8, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess ||
		    hipMemcpyAsync(cmp_off + cmp_pos[k], d_desc + 5 * n + cmp_pos[k], (nk + 1) * 8,
				   hipMemcpyDeviceToHost, s_comp) != hipSuccess) {
			set_error("compress_batch_host: %s", hipGetErrorString(hipGetLastError()));
			return LIBDEFLATE_AMD_NO_DEVICE;
		}
		return LIBDEFLATE_AMD_OK;
	};
	/* slice k's streams are complete on the device: sizes to the caller,
	 * bytes through the pinned pair */
	auto drain = [&](size_t k) -> int {
		const size_t lo = bounds[k], nk = bounds[k + 1] - lo;
		for (size_t i = lo; i < lo + nk; i++)
			out_nbytes[i] = out_n[i];
		return copy_out_packed(&c->pinned, st + cmp_at + avail_before[k] + 64 * k, nk,
				       out + lo, out_n + lo, cmp_off + cmp_pos[k], s_copy);
	};
	return run_slices("compress_batch_host", c->streams, ns, enqueue, drain);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_compress_batch_host(struct libdeflate_compressor *c, int format,
				   size_t n, const void *const *in,
				   const size_t *in_nbytes, void *const *out,
				   const size_t *out_avail, size_t *out_nbytes)
{
	return no_unwind("compress_batch_host", (int)LIBDEFLATE_AMD_OOM, [&]() {
		auto body = [&](struct libdeflate_compressor *o, size_t lo, size_t cnt) {
			return compress_batch_host_body(o, format, cnt, in + lo, in_nbytes + lo,
							out + lo, out_avail + lo, out_nbytes + lo);
		};
		/* (a bad argument is reported by the one-device path) */
		if (!c || n == 0 || !in || !in_nbytes || !out || !out_avail || !out_nbytes)
			return body(c, 0, n);
		/* several GPUs (LDA_DEVICES): shards of about equal input */
		return fanout<libdeflate_compressor>(c, n, in_nbytes, [&](const libdeflate_options *o) {
			return libdeflate_alloc_compressor_ex(c->level, o);
		}, body);
	});
}

/*
 * One LARGE buffer: the input is cut into sub-ranges
 * of LDA_SEG_BYTES that are compressed side by side, one workgroup each.
 * Every sub-range but the first is given the tail of its predecessor as a
 * dictionary (whole tiles that only prime the hash chains), every one but
 * the last ends byte aligned (non-final block + empty stored block), so the
 * pieces concatenate into ONE raw DEFLATE stream; the container header /
 * footer are written on the host, the checksum is combined from the
 * per-piece checksums:
 *   crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B)
 * (programs/gzip.c:149-185 hands the whole file to one compress call; this
 * is what makes that call use the whole GPU.)  The sub-range size, the
 * segments' descriptors and the CRC arithmetic are large_plan.h's, shared with
 * the device-memory form below (libdeflate_amd_compress_large_batch).
 */

/* x^(8 len) mod P: what appending len bytes multiplies a CRC by */
uint32_t lda::crc32_shift(uint64_t len)
{
	return lda_crc_powmod(0x00800000u /* x^8 */, len);
}

uint32_t lda::crc32_concat_shift(uint32_t crc_a, uint32_t crc_b, uint32_t shift_b)
{
	return lda_crc_mulmod(crc_a, shift_b) ^ crc_b;
}

uint32_t lda::crc32_concat(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
	return crc32_concat_shift(crc_a, crc_b, crc32_shift(len_b));
}

uint32_t lda::adler32_concat(uint32_t ad_a, uint32_t ad_b, uint64_t len_b)
{
	const uint32_t M = 65521;
	uint32_t a1 = ad_a & 0xFFFF, b1 = ad_a >> 16;
	uint32_t a2 = ad_b & 0xFFFF, b2 = ad_b >> 16;
	uint32_t rem = (uint32_t)(len_b % M);
	uint32_t a = (a1 + a2 + M - 1) % M;
	uint32_t b = (uint32_t)(((uint64_t)rem * a1 + b1 + b2 + M - rem) % M);
	return (b << 16) | a;
}

/* a device failure inside a single-buffer call: reported, and the call returns
 * 0 like any other "could not produce the stream" (libdeflate.h:73-74); the
 * reason is in libdeflate_amd_last_error() */
static size_t large_fail(const char *what)
{
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		set_error("%s: %s", what, hipGetErrorString(e));
	complain("libdeflate_*_compress", LIBDEFLATE_AMD_NO_DEVICE);
	return 0;
}

/* a segment's bytes: its own and at most dict_window() (whole tiles) in front,
 * of the previous segment or of the dictionary.  The usable window is 32 KiB
 * minus two tiles (the kernel inserts one tile ahead) and the lookahead */
static size_t large_seg_bound(size_t S)
{
	const size_t tile = lda_deflate_tile();
	return S + (dict_window() + tile - 1) / tile * tile;
}

/* the slot a segment is compressed into */
static size_t large_slot(struct libdeflate_compressor *c, size_t S)
{
	return align_up(libdeflate_deflate_compress_bound(c, S) + 32, 16);
}

/*
 * The segments go through in SLICES of up to 32 MiB of input on run_slices(),
 * like the host-pointer batches: while the kernels of slice k
 * (deflate of its segments, their checksums, the compaction of their streams)
 * run on the compute stream, the host packs slice k + 1 into the pinned
 * staging and sends it, and brings the compacted streams of slice k - 1 back.
 * Nothing runs on the null stream and nothing waits for the whole device.
 */
static size_t compress_large(struct libdeflate_compressor *c, int format,
			     const uint8_t *in, size_t n, uint8_t *out,
			     size_t out_avail, const uint8_t *dict = NULL,
			     size_t dict_nbytes = 0)
{
	/* a preset dictionary's call below LDA_LARGE_MIN is one segment */
	const size_t S = dict && n < LDA_LARGE_MIN ? (n ? n : 1) :
			 (size_t)lda_large_seg_bytes(n, env_cfg().seg_bytes);
	const size_t nseg = n ? (n + S - 1) / S : 1;
	const size_t seg_bound = large_seg_bound(S);
	const size_t slot = large_slot(c, S);
	/* the caller's dictionary primes the first segment: its prefix (see
	 * shape_dict()) lies in front of the input in the staging area */
	const dict_shape dsh = shape_dict(c->level, dict ? dict_nbytes : 0);
	const size_t pre = dict && n ? dsh.pre_len : 0;
	const uint32_t hdr = format == LIBDEFLATE_AMD_GZIP ? 10 :
			     format == LIBDEFLATE_AMD_ZLIB ? (dict ? 6 : 2) : 0;
	const uint32_t ftr = format == LIBDEFLATE_AMD_GZIP ? 8 :
			     format == LIBDEFLATE_AMD_ZLIB ? 4 : 0;

	if (out_avail <= hdr + ftr)
		return 0;
	DeviceCtx *ctx = device_ctx();
	if (!ctx || !c->streams.enter())
		return large_fail("streams");
	hipStream_t s_copy = c->streams.copy, s_comp = c->streams.comp;
	const size_t per_slice = (size_t)lda_large_per_slice(S);
	const size_t ns = (nseg + per_slice - 1) / per_slice;
	/* device layout: [7 u64 rows: in_off in_n out_off out_av out_n piece_off
	 * piece_n][seg_info u32][sums u32][compaction offsets of every slice]
	 * [input][slots][the slots' used parts, slice after slice] */
	std::vector<size_t> cmp_pos(ns + 1);
	cmp_pos[0] = 0;
	for (size_t k = 0; k < ns; k++)
		cmp_pos[k + 1] = cmp_pos[k] + libdeflate_amd_compact_offsets_len(
			std::min(per_slice, nseg - k * per_slice));
	const size_t ncmp = cmp_pos[ns];
	const size_t desc_bytes = align_up(nseg * (7 * 8 + 4 + 4) + 64, 64);
	const size_t cmp_at = desc_bytes, in_at = align_up(cmp_at + ncmp * 8 + 64, 64) + pre;
	const size_t out_at = align_up(in_at + n + 64, 64);
	const size_t pk_at = align_up(out_at + nseg * slot + 64, 64);
	uint8_t *st = (uint8_t *)c->stage.reserve(pk_at + nseg * slot + 64);
	if (!st) {
		complain("libdeflate_*_compress (device memory)", LIBDEFLATE_AMD_OOM);
		return 0;
	}
	{	/* the kernels' scratch for the largest launch, before any is queued */
		if (!c->scratch.reserve(plan_batch(c, std::min(per_slice, nseg), seg_bound, true,
						   false).total)) {
			complain("libdeflate_*_compress (device memory)", LIBDEFLATE_AMD_OOM);
			return 0;
		}
	}
	std::vector<uint64_t> d64(7 * nseg);
	std::vector<uint32_t> d32(nseg);
	uint64_t *in_off = &d64[0], *in_n = &d64[nseg], *out_off = &d64[2 * nseg],
		 *out_av = &d64[3 * nseg], *pc_off = &d64[5 * nseg], *pc_n = &d64[6 * nseg];
	const lda_large_shape shape = { n, S, dict_window(), lda_deflate_tile(), nseg, slot,
					in_at, out_at };
	for (size_t i = 0; i < nseg; i++) {
		const lda_large_seg s = lda_large_seg_of(shape, i);
		in_off[i] = s.in_off;
		in_n[i] = s.in_n;
		out_off[i] = s.out_off;
		out_av[i] = s.out_av;
		pc_off[i] = s.pc_off;
		pc_n[i] = s.pc_n;
		d32[i] = s.info;
	}
	std::vector<uint8_t> prefix(pre);
	if (pre) {
		in_off[0] -= pre;
		in_n[0] += pre;
		d32[0] |= dsh.sinfo & 0x7FFFFFFFu;
		memcpy(&prefix[pre - dsh.tail], dict + dict_nbytes - dsh.tail, dsh.tail);
	}
	uint64_t *d_desc = (uint64_t *)st;
	uint32_t *d_seg = (uint32_t *)(st + 7 * 8 * nseg);
	uint32_t *d_sums = d_seg + nseg;
	uint64_t *d_cmp = (uint64_t *)(st + cmp_at);
	/* what comes back per slice, in pinned memory: sizes, sums, the total */
	uint64_t *h_back = (uint64_t *)c->meta.ensure(nseg * 12 + ns * 8 + 64);
	if (!h_back)
		return large_fail("pinned memory");
	uint64_t *h_out_n = h_back, *h_tot = h_back + nseg;
	uint32_t *h_sums = (uint32_t *)(h_back + nseg + ns);
	if (hipMemcpyAsync(d_desc, d64.data(), 7 * 8 * nseg, hipMemcpyHostToDevice, s_copy) != hipSuccess ||
	    hipMemcpyAsync(d_seg, d32.data(), 4 * nseg, hipMemcpyHostToDevice, s_copy) != hipSuccess ||
	    (pre && hipMemcpyAsync(st + in_at - pre, prefix.data(), pre, hipMemcpyHostToDevice,
				   s_copy) != hipSuccess))
		return large_fail("copy in");
	/* A call of one slice (up to 32 MiB) takes the copy helpers' own pieces:
	 * all copy threads on its input AND on its output (16 MiB: 10.9 -> 12.2
	 * GB/s, round 6).  A call of several slices keeps pieces of 1 MiB, with
	 * which a slice's output - a third of its input - is copied by the calling
	 * thread alone: with the threads on it too, four processes of six ran
	 * 256 MiB calls in 12.3 ms instead of 10.9 (`profiles/r06_ab.md` run 35;
	 * the calling thread is what queues the next slice's kernels). */
	const size_t piece = ns > 1 ? (size_t)1 << 20 : 0;
	size_t total = hdr;	/* bytes of the output so far */
	auto enqueue = [&](size_t k) -> int {
		const size_t lo = k * per_slice, nk = std::min(per_slice, nseg - lo);
		const size_t a = lo * S, b = std::min(n, (lo + nk) * S);
		/* (returns when the slice - and, the first time, the descriptors -
		 * are on the device) */
		if (b > a ? span_in(&c->pinned, st, in_at + a, in + a, b - a, s_copy, piece) != LIBDEFLATE_AMD_OK :
			    hipStreamSynchronize(s_copy) != hipSuccess)
			return LIBDEFLATE_AMD_NO_DEVICE;
		int rc = compress_batch_impl(c, LIBDEFLATE_AMD_DEFLATE, nk, st, d_desc + lo,
					     d_desc + nseg + lo, st, d_desc + 2 * nseg + lo,
					     d_desc + 3 * nseg + lo, d_desc + 4 * nseg + lo, s_comp,
					     d_seg + lo, seg_bound);
		if (rc == LIBDEFLATE_AMD_OK && ftr)
			rc = format == LIBDEFLATE_AMD_GZIP ?
				libdeflate_amd_crc32_batch(nk, st, d_desc + 5 * nseg + lo,
							   d_desc + 6 * nseg + lo, NULL, d_sums + lo, s_comp) :
				libdeflate_amd_adler32_batch(nk, st, d_desc + 5 * nseg + lo,
							     d_desc + 6 * nseg + lo, NULL, d_sums + lo, s_comp);
		if (rc == LIBDEFLATE_AMD_OK)
			rc = libdeflate_amd_compact_batch(nk, st, d_desc + 2 * nseg + lo,
							  d_desc + 4 * nseg + lo, st + pk_at + lo * slot,
							  d_cmp + cmp_pos[k], s_comp);
		if (rc != LIBDEFLATE_AMD_OK ||
		    hipMemcpyAsync(h_out_n + lo, d_desc + 4 * nseg + lo, nk * 8, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess ||
		    hipMemcpyAsync(h_tot + k, d_cmp + cmp_pos[k] + nk, 8, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess ||
		    (ftr && hipMemcpyAsync(h_sums + lo, d_sums + lo, nk * 4, hipMemcpyDeviceToHost,
					   s_comp) != hipSuccess))
			return LIBDEFLATE_AMD_NO_DEVICE;
		return LIBDEFLATE_AMD_OK;
	};
	auto drain = [&](size_t k) -> int {
		const size_t lo = k * per_slice, nk = std::min(per_slice, nseg - lo);
		for (size_t i = lo; i < lo + nk; i++)
			if (h_out_n[i] == 0)
				return SLICES_STOP;	/* a segment did not fit its slot: cannot happen within the bound */
		const size_t tk = (size_t)h_tot[k];
		if (total + tk + ftr > out_avail)
			return SLICES_STOP;
		if (tk && span_out(&c->pinned, st, pk_at + lo * slot, out + total, tk, s_copy, piece) != LIBDEFLATE_AMD_OK)
			return LIBDEFLATE_AMD_NO_DEVICE;
		total += tk;
		return LIBDEFLATE_AMD_OK;
	};
	const int rc = run_slices("segmented compress", c->streams, ns, enqueue, drain);
	if (rc != LIBDEFLATE_AMD_OK && rc != SLICES_STOP)
		return large_fail("segmented compress");
	if (rc == SLICES_STOP || total + ftr > out_avail)
		return 0;
	const size_t at = total;
	total += ftr;
	if (format == LIBDEFLATE_AMD_GZIP) {
		/* lib/gzip_compress.c:44-79 */
		uint32_t crc = 0;
		const uint32_t shS = crc32_shift(S);	/* every piece but the last is S bytes */
		for (size_t i = 0; i < nseg; i++)
			crc = !i ? h_sums[0] :
			      pc_n[i] == S ? crc32_concat_shift(crc, h_sums[i], shS) :
					     crc32_concat(crc, h_sums[i], pc_n[i]);
		const uint8_t h[10] = { 0x1F, 0x8B, 8, 0, 0, 0, 0, 0, lda_gzip_xfl(c->level), 0xFF };
		memcpy(out, h, 10);
		uint32_t isize = (uint32_t)n;
		for (int k = 0; k < 4; k++) {
			out[at + k] = (uint8_t)(crc >> (8 * k));
			out[at + 4 + k] = (uint8_t)(isize >> (8 * k));
		}
	} else if (format == LIBDEFLATE_AMD_ZLIB) {
		/* lib/zlib_compress.c:45-72 */
		uint32_t ad = 1;
		for (size_t i = 0; i < nseg; i++)
			ad = i ? adler32_concat(ad, h_sums[i], pc_n[i]) : h_sums[0];
		uint32_t hw = lda_zlib_header(c->level);
		if (dict) {
			/* FDICT and DICTID (RFC 1950 2.2) */
			hw = (hw & 0xFFC0u) | 0x20;
			hw += (31 - hw % 31) % 31;
			const uint32_t id = libdeflate_adler32(1, dict, dict_nbytes);
			for (int k = 0; k < 4; k++)
				out[2 + k] = (uint8_t)(id >> (8 * (3 - k)));
		}
		out[0] = (uint8_t)(hw >> 8);
		out[1] = (uint8_t)hw;
		for (int k = 0; k < 4; k++)
			out[at + k] = (uint8_t)(ad >> (8 * (3 - k)));
	}
	return total;
}

static size_t compress_one(struct libdeflate_compressor *c, int format,
			   const void *in, size_t in_nbytes, void *out,
			   size_t out_avail)
{
	if (!c)
		return 0;
	DeviceGuard on(c->device);
	if (!on.ok()) {
		complain("libdeflate_*_compress", LIBDEFLATE_AMD_NO_DEVICE);
		return 0;
	}
	if (lda_large_segmented(in_nbytes, c->level, env_cfg().no_segments))
		return no_unwind("libdeflate_*_compress", (size_t)0, [&]() {
			return compress_large(c, format, (const uint8_t *)in, in_nbytes,
					      (uint8_t *)out, out_avail);
		});
	const void *ins[1] = { in };
	void *outs[1] = { out };
	size_t got = 0;
	int rc = libdeflate_amd_compress_batch_host(c, format, 1, ins, &in_nbytes,
						    outs, &out_avail, &got);

	if (rc != LIBDEFLATE_AMD_OK) {
		complain("libdeflate_*_compress", rc);
		return 0;
	}
	return got;
}

/* libdeflate.h:85-88 */
extern "C" LIBDEFLATEAPI size_t
libdeflate_deflate_compress(struct libdeflate_compressor *c, const void *in,
			    size_t in_nbytes, void *out, size_t out_avail)
{
	return compress_one(c, LIBDEFLATE_AMD_DEFLATE, in, in_nbytes, out,
			    out_avail);
}

/* libdeflate.h:122-125 */
extern "C" LIBDEFLATEAPI size_t
libdeflate_zlib_compress(struct libdeflate_compressor *c, const void *in,
			 size_t in_nbytes, void *out, size_t out_avail)
{
	return compress_one(c, LIBDEFLATE_AMD_ZLIB, in, in_nbytes, out, out_avail);
}

/* libdeflate.h:140-143 */
extern "C" LIBDEFLATEAPI size_t
libdeflate_gzip_compress(struct libdeflate_compressor *c, const void *in,
			 size_t in_nbytes, void *out, size_t out_avail)
{
	return compress_one(c, LIBDEFLATE_AMD_GZIP, in, in_nbytes, out, out_avail);
}

/* include/libdeflate_amd.h: one host buffer with a preset dictionary - the
 * segmented path, its first segment primed with the dictionary */
extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_compress_dict(struct libdeflate_compressor *c, int format,
			     const void *dict, size_t dict_nbytes, const void *in,
			     size_t in_nbytes, void *out, size_t out_avail)
{
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB) {
		set_error("libdeflate_amd_compress_dict: format %d takes no dictionary", format);
		return 0;
	}
	if (!dict_nbytes)
		return compress_one(c, format, in, in_nbytes, out, out_avail);
	if (!c || !dict || (!in && in_nbytes) || !out) {
		set_error("libdeflate_amd_compress_dict: bad argument");
		return 0;
	}
	DeviceGuard on(c->device);
	if (!on.ok()) {
		complain("libdeflate_amd_compress_dict", LIBDEFLATE_AMD_NO_DEVICE);
		return 0;
	}
	return no_unwind("libdeflate_amd_compress_dict", (size_t)0, [&]() {
		return compress_large(c, format, (const uint8_t *)in, in_nbytes, (uint8_t *)out,
				      out_avail, (const uint8_t *)dict, dict_nbytes);
	});
}

/*
 * include/libdeflate_amd.h: ONE stream from one DEVICE buffer, enqueue only.
 * The bytes are compress_one()'s: the same decision between one chunk and
 * segments, the same S, descriptors and launches of lda_large_per_slice(S)
 * segments (large_plan.h) - and what compress_large() does on the host
 * between them is done by the kernels of large_kernels.hip: the descriptors,
 * the checksum of the whole buffer from the pieces', header, footer, size.
 * c->large: [7 u64 rows][scan offsets][seg_info u32][sums u32][slots].
 * The check and the body are apart for libdeflate_amd_targz_compress_batch
 * (host_tar_write.hip), whose input is an archive it writes first.
 */
bool lda::compress_large_args_ok(const char *what, const struct libdeflate_compressor *c,
				 int format, const void *d_in, size_t in_nbytes, const void *d_out,
				 size_t out_avail, const uint64_t *d_out_nbytes)
{
	if (!c || (!d_in && in_nbytes) || !d_out || !d_out_nbytes) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB &&
	    format != LIBDEFLATE_AMD_GZIP) {
		set_error("%s: format %d is not DEFLATE, zlib or gzip", what, format);
		return false;
	}
	const uint32_t hdr = format == LIBDEFLATE_AMD_GZIP ? 10 : format == LIBDEFLATE_AMD_ZLIB ? 2 : 0;
	const uint32_t ftr = format == LIBDEFLATE_AMD_GZIP ? 8 : format == LIBDEFLATE_AMD_ZLIB ? 4 : 0;
	if (out_avail <= hdr + ftr) {
		set_error("%s: out_avail %zu cannot hold the container and a byte", what, out_avail);
		return false;
	}
	return true;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_compress_large_batch(struct libdeflate_compressor *c, int format,
				    const void *d_in, size_t in_nbytes, void *d_out,
				    size_t out_avail, uint64_t *d_out_nbytes, void *stream)
{
	if (!compress_large_args_ok("compress_large_batch", c, format, d_in, in_nbytes, d_out,
				    out_avail, d_out_nbytes))
		return LIBDEFLATE_AMD_BAD_ARG;
	return compress_large_enqueue(c, format, d_in, in_nbytes, d_out, out_avail, d_out_nbytes,
				      stream);
}

/* the scratch of a stream of n bytes: where the parts of c->large lie (one
 * chunk: its four descriptor words alone) and what the kernels take of
 * c->scratch */
struct large_layout {
	bool segmented;
	size_t S, nseg, seg_bound, slot, per_slice, cmp_at, seg_at, slots_at;
	size_t large_bytes, kernel_bytes;
};

static large_layout large_layout_of(struct libdeflate_compressor *c, size_t n)
{
	large_layout l = {};
	l.segmented = lda_large_segmented(n, c->level, env_cfg().no_segments);
	if (!l.segmented) {
		l.large_bytes = 4 * 8;
		l.kernel_bytes = plan_batch(c, 1, n, false, false).total;
		return l;
	}
	l.S = (size_t)lda_large_seg_bytes(n, env_cfg().seg_bytes);
	l.nseg = (n + l.S - 1) / l.S;
	l.seg_bound = large_seg_bound(l.S);
	l.slot = large_slot(c, l.S);
	l.per_slice = (size_t)lda_large_per_slice(l.S);
	l.cmp_at = 7 * 8 * l.nseg;
	l.seg_at = l.cmp_at + 8 * libdeflate_amd_compact_offsets_len(l.nseg);
	l.slots_at = align_up(l.seg_at + 8 * l.nseg, 256);
	l.large_bytes = l.slots_at + l.nseg * l.slot;
	l.kernel_bytes = plan_batch(c, std::min(l.per_slice, l.nseg), l.seg_bound, true, false).total;
	return l;
}

bool lda::compress_large_reserve(struct libdeflate_compressor *c, size_t in_nbytes)
{
	const large_layout l = large_layout_of(c, in_nbytes);
	return c->large.reserve(l.large_bytes) && c->scratch.reserve(l.kernel_bytes);
}

int lda::compress_large_enqueue(struct libdeflate_compressor *c, int format, const void *d_in,
				size_t in_nbytes, void *d_out, size_t out_avail,
				uint64_t *d_out_nbytes, void *stream)
{
	const uint32_t hdr = format == LIBDEFLATE_AMD_GZIP ? 10 : format == LIBDEFLATE_AMD_ZLIB ? 2 : 0;
	const uint32_t ftr = format == LIBDEFLATE_AMD_GZIP ? 8 : format == LIBDEFLATE_AMD_ZLIB ? 4 : 0;
	DeviceGuard on(c->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	hipStream_t st = (hipStream_t)stream;
	const size_t n = in_nbytes;
	const large_layout l = large_layout_of(c, n);

	if (!l.segmented) {
		/* one chunk of the ordinary batch, straight into d_out, its size
		 * straight into d_out_nbytes (compress_batch_host_body() gives the
		 * kernels the same bound) */
		uint64_t *rows = (uint64_t *)c->large.reserve(l.large_bytes);
		if (!rows)
			return LIBDEFLATE_AMD_OOM;
		hipLaunchKernelGGL(lda_large_one_desc_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n,
				   (uint64_t)out_avail, rows);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return compress_batch_impl(c, format, 1, d_in ? d_in : (const void *)rows, rows,
					   rows + 1, d_out, rows + 2, rows + 3, d_out_nbytes, stream,
					   NULL, n);
	}
	const size_t S = l.S, nseg = l.nseg, seg_bound = l.seg_bound, slot = l.slot;
	const size_t per_slice = l.per_slice, cmp_at = l.cmp_at, seg_at = l.seg_at;
	const size_t slots_at = l.slots_at;
	/* all of the call's scratch before anything is queued: growing frees
	 * memory (and waits for the device) */
	uint8_t *ws = (uint8_t *)c->large.reserve(l.large_bytes);
	if (!ws || !c->scratch.reserve(l.kernel_bytes))
		return LIBDEFLATE_AMD_OOM;
	uint64_t *rows = (uint64_t *)ws, *out_n = rows + 4 * nseg, *cmp = (uint64_t *)(ws + cmp_at);
	uint32_t *d_seg = (uint32_t *)(ws + seg_at), *d_sums = d_seg + nseg;
	uint8_t *slots = ws + slots_at;
	/* offsets into d_in and into the slots */
	const lda_large_shape shape = { n, S, dict_window(), lda_deflate_tile(), nseg, slot, 0, 0 };
	hipLaunchKernelGGL(lda_large_desc_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0,
			   st, shape, rows, d_seg);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	for (size_t lo = 0; lo < nseg; lo += per_slice) {
		const size_t nk = std::min(per_slice, nseg - lo);
		int rc = compress_batch_impl(c, LIBDEFLATE_AMD_DEFLATE, nk, d_in, rows + lo,
					     rows + nseg + lo, slots, rows + 2 * nseg + lo,
					     rows + 3 * nseg + lo, out_n + lo, stream, d_seg + lo,
					     seg_bound);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (ftr) {
		int rc = format == LIBDEFLATE_AMD_GZIP ?
			libdeflate_amd_crc32_batch(nseg, d_in, rows + 5 * nseg, rows + 6 * nseg, NULL,
						   d_sums, stream) :
			libdeflate_amd_adler32_batch(nseg, d_in, rows + 5 * nseg, rows + 6 * nseg, NULL,
						     d_sums, stream);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	/* the scans of libdeflate_amd_compact_batch(), a copy that writes nothing
	 * unless the whole stream fits, and the container around it */
	uint64_t *block_sums = cmp + nseg + 1;
	const size_t nblocks = scan_enqueue(st, nseg, out_n, cmp, block_sums);
	const size_t grid = std::min(nseg, (size_t)ctx->num_cus * 8);
	hipLaunchKernelGGL(lda_large_copy_kernel, dim3((unsigned)grid), dim3(256), 0, st,
			   (uint64_t)nseg, (const uint8_t *)slots, (uint64_t)slot,
			   (const uint64_t *)out_n, (const uint64_t *)cmp,
			   (const uint64_t *)block_sums, (uint8_t *)d_out, hdr, ftr,
			   (uint64_t)out_avail);
	/* every piece but the last is S bytes */
	const uint32_t xS = format == LIBDEFLATE_AMD_GZIP ? crc32_shift(S) : 0;
	const uint32_t xL = format == LIBDEFLATE_AMD_GZIP ? crc32_shift(n - (nseg - 1) * S) : 0;
	hipLaunchKernelGGL(lda_large_finalize_kernel, dim3(1), dim3(1024), 0, st, (uint64_t)nseg,
			   (uint64_t)n, (uint64_t)S, format, c->level, (const uint64_t *)out_n,
			   (const uint32_t *)d_sums, (const uint64_t *)(block_sums + nblocks), xS, xL,
			   (uint8_t *)d_out, (uint64_t)out_avail, d_out_nbytes);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}
