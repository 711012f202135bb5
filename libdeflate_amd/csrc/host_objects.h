/*
 * host_objects.h - the two opaque objects of the C-ABI.
 *
 * Each is ONE allocation through the selected allocator (per-object options >
 * libdeflate_set_memory_allocator > malloc), like the reference
 * (lib/deflate_compress.c:3910-3917, programs/test_custom_malloc.c:53-77).
 * Device memory hangs off the object and never goes through that allocator.
 */
#ifndef LDA_HOST_OBJECTS_H
#define LDA_HOST_OBJECTS_H

#include "host_common.h"
#include "stream_types.h"
#include <functional>

namespace lda {

typedef void *(*malloc_func_t)(size_t);
typedef void (*free_func_t)(void *);

extern malloc_func_t g_malloc;	/* libdeflate_set_memory_allocator */
extern free_func_t g_free;

/* grow-only device buffer owned by an object */
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	void *reserve(size_t n);	/* nullptr + error on failure */
	void release();
};

} /* namespace lda */

#define LDA_MAX_SHARDS 16	/* devices one host-pointer batch is spread over */

struct libdeflate_decompressor {
	lda::free_func_t free_func;
	lda::malloc_func_t malloc_func;
	int device;		/* the device the object lives on (current at allocation) */
	/* host-pointer batches over several GPUs (LDA_DEVICES): one more object
	 * per further device, built on first use, freed with this one */
	struct libdeflate_decompressor *shard[LDA_MAX_SHARDS];
	lda::DevBuf scratch;	/* per-chunk u32 sums + u64 actual_in/out */
	lda::DevBuf stage;	/* host-pointer entry points */
	lda::DevBuf tokens;	/* per-wave token scratch of the wave-per-stream kernel */
	/* one large stream on many waves (host_stream.hip): input + finder
	 * queues, chunk descriptors / results, 16-bit symbols, output bytes */
	lda::DevBuf sin, squeue, schunks, srepair, ssym, sout, swin, shdr, shint;
	/* the same for a stream in device memory (libdeflate_amd_decompress_large):
	 * the rows of possible stored blocks and the headers' classes */
	lda::DevBuf sprobe;
	lda::PinnedPair pinned;	/* host-pointer entry points */
	lda::PinnedBuf meta;	/* host-pointer entry points: per-chunk read-backs */
	lda::StreamPair streams;	/* host-pointer entry points: transfers / kernels */
	/* BGZF files read on the device (host_bgzf_read.hip): candidates, chain,
	 * descriptors, edge slots; the descriptors of a ranged read on their way
	 * up.  The reader of concatenated gzip
	 * members (host_gzip_members.hip) keeps its candidates, counts, chain and
	 * descriptors in the same buffer */
	lda::DevBuf bgzf;
	lda::Upload bgzf_up;
	/* the seek index (host_seek.hip): descriptors and results of the intervals
	 * of a build's verification or of a ranged read; a read's descriptors on
	 * their way up */
	lda::DevBuf seek;
	lda::Upload seek_up;
};

struct libdeflate_compressor {
	lda::free_func_t free_func;
	lda::malloc_func_t malloc_func;
	int device;		/* the device the object lives on (current at allocation) */
	struct libdeflate_compressor *shard[LDA_MAX_SHARDS];	/* see libdeflate_decompressor */
	int level;
	lda::DevBuf scratch;	/* parse/encode workspace + per-chunk sums */
	lda::DevBuf stage;
	lda::DevBuf bgzf;	/* BGZF files: block descriptors, member slots (host_bgzf.hip) */
	/* one stream from one device buffer (libdeflate_amd_compress_large_batch):
	 * descriptor rows, seg_info, per-piece sums, scan offsets, segment slots */
	lda::DevBuf large;
	/* a ZIP archive, a file of gzip members or PNG files written on the device:
	 * the common regions of host_write_pieces.hip (the piece columns, per-piece
	 * and per-entry results, the slots), each writer's own columns in front and
	 * its results behind them - the PNG writer's filtered scanlines last -; the
	 * tar writer's rows and archive (host_tar_write.hip); the columns on their
	 * way up */
	lda::DevBuf zipw;
	lda::Upload zipw_up;
	lda::PinnedPair pinned;	/* host-pointer entry points */
	lda::PinnedBuf meta;	/* host-pointer entry points: per-chunk read-backs */
	lda::StreamPair streams;	/* host-pointer entry points: transfers / kernels */
	lda::SideStream side;	/* the split path's tail beside its head (compress_batch_impl()) */
	/* what the last batch call did (libdeflate_amd_compress_last_schedule) */
	uint32_t last_schedule[4] = { 0, 0, 0, 0 };
	/* and the compress kernel it launched (libdeflate_amd_compress_last_kernel) */
	const char *last_kernel = "";
};

namespace lda {
/* host_decompress.hip: the allocator of an object, the way
 * lib/deflate_compress.c:3910-3917 resolves it; false = options of another size */
bool pick_allocator(const struct libdeflate_options *options,
		    malloc_func_t *m, free_func_t *f);

/*
 * host_fanout.hip: one host-pointer batch of n chunks over the GPUs of a node
 * (LDA_DEVICES).  The chunks are cut into contiguous shards of about equal
 * weight[] (what a chunk costs); shard k > 0 runs through o->shard[k], built
 * on first use by alloc() with its device current and o's allocator.
 * body(object, lo, count) runs every shard on a host thread of its own and the
 * first non-OK status is returned.  One shard, or a shard object that cannot
 * be built, is body(o, 0, n) on the calling thread.
 */
template <typename Obj>
int fanout(Obj *o, size_t n, const size_t *weight,
	   const std::function<Obj *(const struct libdeflate_options *)> &alloc,
	   const std::function<int(Obj *, size_t, size_t)> &body);

/* host_compress.hip, for the writers' piece pipeline (host_write_pieces.hip): one
 * compress batch of raw DEFLATE as the batch entry points launch it - seg_info NULL or
 * one word per chunk (large_plan.h), max_in the size bound of the chunks - the
 * kernels' scratch such a launch reserves in the object (reserve the largest
 * before the first of several is queued: growing frees memory), and the bytes
 * in front of a segment that prime it (lda_large_shape's D) */
int compress_deflate_pieces(struct libdeflate_compressor *c, size_t n, const void *d_in,
			    const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes, void *d_out,
			    const uint64_t *d_out_offsets, const uint64_t *d_out_avail,
			    uint64_t *d_out_nbytes, void *stream, const uint32_t *d_seg_info,
			    size_t max_in);
size_t compress_pieces_scratch(const struct libdeflate_compressor *c, size_t n, size_t max_in,
			       bool seg);
size_t compress_prime_window(void);

/* host_compress.hip, for the tar writer (host_tar_write.hip): what
 * libdeflate_amd_compress_large_batch refuses (false, with the error set under
 * the name `what`), and what it enqueues once its arguments have passed */
bool compress_large_args_ok(const char *what, const struct libdeflate_compressor *c, int format,
			    const void *d_in, size_t in_nbytes, const void *d_out, size_t out_avail,
			    const uint64_t *d_out_nbytes);
/* the scratch that compress_large_enqueue() of in_nbytes bytes takes of the
 * object, reserved ahead: a caller that queues work of its own in front reserves
 * first, because growing frees memory and waits for the device */
bool compress_large_reserve(struct libdeflate_compressor *c, size_t in_nbytes);
int compress_large_enqueue(struct libdeflate_compressor *c, int format, const void *d_in,
			   size_t in_nbytes, void *d_out, size_t out_avail,
			   uint64_t *d_out_nbytes, void *stream);

/* host_decompress.hip, for the prefix batch (host_prefix.hip), which launches
 * the wave kernel's geometry: dynamic LDS of a wave, waves per CU (LDS and
 * LDA_INFLATE_WAVES_PER_CU), and the bytes of d->tokens for a batch of n
 * streams - the token rows of every wave of the grid, then 16 bytes of
 * counters */
size_t inflate_wave_lds(void);
size_t inflate_waves_per_cu(void);
size_t inflate_tokens_bytes(size_t n, int num_cus);

/* host_sizes.hip: the size query on a stream (arguments checked by the
 * callers); s: sizes_scratch_bytes(n) bytes of device memory that stay
 * untouched until the query has run */
size_t sizes_scratch_bytes(size_t n);
int sizes_enqueue(DeviceCtx *c, uint8_t *s, int format, size_t n, const void *d_in,
		  const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
		  const uint64_t *d_out_limit, int32_t *d_results, uint64_t *d_actual_in,
		  uint64_t *d_out_nbytes, hipStream_t st, const void *d_dict, size_t dict_nbytes);

/* host_stream.hip: true = answered (result, sizes, output); false = the
 * caller takes the sequential path.  on_device: `in` and `out` are device
 * pointers (libdeflate_amd_decompress_large), the object's streams exist and
 * are ordered behind whatever produces `in`.
 * `seek` (seek_plan.h; NULL: nobody asks): on a SUCCESS answered here, the
 * accepted chain and the container's sizes, for a seek index. */
struct seek_export;
bool decompress_stream_parallel(struct libdeflate_decompressor *d, int format,
				const uint8_t *in, size_t in_nbytes, uint8_t *out,
				size_t out_avail, bool exact_fill, int32_t *res,
				size_t *ain, size_t *aout, bool on_device = false,
				seek_export *seek = nullptr);
/* host_stream.hip: one launch of lda_stream_count_kernel over n chunks on `st`
 * (the header cache and the hint rows: NULL where there are none) */
bool launch_count(hipStream_t st, uint32_t n, const lda_stream_chunk *d_chunks,
		  lda_stream_res *d_res, const uint8_t *d_raw, uint64_t raw_n,
		  const uint8_t *d_hlens = nullptr, const uint32_t *d_hinfo = nullptr,
		  uint16_t *d_hints = nullptr);
/* decode waves per launch of the stream decode kernels, and their token
 * scratch (48 KiB each; d->tokens): nullptr + error on failure */
const size_t STREAM_DECODE_BATCH = 4096;
uint32_t *stream_token_scratch(struct libdeflate_decompressor *d, size_t nwaves);
/* host_stream.hip: the body of libdeflate_amd_decompress_large (arguments
 * checked by the caller, `what` names it in errors); with `seek`, also what
 * libdeflate_amd_decompress_large_index (host_seek.hip) builds its index from -
 * of a stream the sequential decoder answered for, point 0 alone */
enum libdeflate_result
decompress_large_body(struct libdeflate_decompressor *d, int format, const uint8_t *d_in,
		      size_t in_nbytes, uint8_t *d_out, size_t out_avail, size_t *actual_in_ret,
		      size_t *actual_out_ret, hipStream_t user, const char *what,
		      seek_export *seek);
}

#endif /* LDA_HOST_OBJECTS_H */
