/*
 * libdeflate_amd.h - C-ABI of the MI355X-native whole-buffer DEFLATE engine.
 *
 * Two groups of entry points, all `extern "C"`, plain pointers and sizes:
 *
 *  (1) The 21 `libdeflate_*` symbols of the reference's public header
 *      (/root/reference/libdeflate.h, v1.25) with identical signatures,
 *      argument meaning, return conventions and error codes, so that a
 *      program written against libdeflate links against libdeflate_amd.so
 *      unchanged.  Each declaration cites the reference line it replaces.
 *      `in`/`out` are HOST pointers, exactly as in the reference; every call
 *      is executed as a batch of one on the GPU (H2D, kernels, D2H).  There
 *      is NO CPU fallback: without a usable gfx950 device the allocators
 *      return NULL and the checksum calls abort() with a message on stderr.
 *
 *  (2) The additive batch extension `libdeflate_amd_*`: the same operations
 *      over N independent chunks that are ALREADY RESIDENT IN HBM, described
 *      by offset/size arrays (also in HBM).  This is the hot path bench.py
 *      measures; one 64-lane wavefront (decode, checksums) or one workgroup
 *      (LZ77 parse) per chunk.  `stream` is a hipStream_t passed as void*
 *      (NULL = the default stream); the calls enqueue work and return.
 *
 * Result conventions are the reference's: compress -> bytes written, 0 when
 * the output does not fit (libdeflate.h:73-74); decompress ->
 * enum libdeflate_result (libdeflate.h:194-209).
 */
#ifndef LIBDEFLATE_AMD_H
#define LIBDEFLATE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIBDEFLATE_VERSION_MAJOR	1	/* libdeflate.h:15 */
#define LIBDEFLATE_VERSION_MINOR	25	/* libdeflate.h:16 */
#define LIBDEFLATE_VERSION_STRING	"1.25"	/* libdeflate.h:17 */
#define LIBDEFLATE_AMD_VERSION_STRING	"0.1-gfx950"

#ifndef LIBDEFLATEAPI
#  define LIBDEFLATEAPI __attribute__((visibility("default")))
#endif

struct libdeflate_compressor;	/* opaque; host object + device scratch */
struct libdeflate_decompressor;	/* opaque */

/* libdeflate.h:379-406 - per-object allocator override */
struct libdeflate_options {
	size_t sizeof_options;		/* must equal sizeof(struct) */
	void *(*malloc_func)(size_t);	/* NULL -> global / malloc */
	void (*free_func)(void *);
};

/* libdeflate.h:194-209 */
enum libdeflate_result {
	LIBDEFLATE_SUCCESS = 0,
	LIBDEFLATE_BAD_DATA = 1,
	LIBDEFLATE_SHORT_OUTPUT = 2,
	LIBDEFLATE_INSUFFICIENT_SPACE = 3,
};

/* ------------------------------------------------------------------ */
/* (1) drop-in single-buffer API (host pointers)                       */
/* ------------------------------------------------------------------ */

/* libdeflate.h:59-60; level 0..12, -1 = 6; NULL on bad level / OOM / no GPU */
LIBDEFLATEAPI struct libdeflate_compressor *
libdeflate_alloc_compressor(int compression_level);

/* libdeflate.h:65-67 */
LIBDEFLATEAPI struct libdeflate_compressor *
libdeflate_alloc_compressor_ex(int compression_level,
			       const struct libdeflate_options *options);

/* libdeflate.h:85-88 */
LIBDEFLATEAPI size_t
libdeflate_deflate_compress(struct libdeflate_compressor *compressor,
			    const void *in, size_t in_nbytes,
			    void *out, size_t out_nbytes_avail);

/* libdeflate.h:114-116; compressor may be NULL */
LIBDEFLATEAPI size_t
libdeflate_deflate_compress_bound(struct libdeflate_compressor *compressor,
				  size_t in_nbytes);

/* libdeflate.h:122-125 */
LIBDEFLATEAPI size_t
libdeflate_zlib_compress(struct libdeflate_compressor *compressor,
			 const void *in, size_t in_nbytes,
			 void *out, size_t out_nbytes_avail);

/* libdeflate.h:132-134 */
LIBDEFLATEAPI size_t
libdeflate_zlib_compress_bound(struct libdeflate_compressor *compressor,
			       size_t in_nbytes);

/* libdeflate.h:140-143 */
LIBDEFLATEAPI size_t
libdeflate_gzip_compress(struct libdeflate_compressor *compressor,
			 const void *in, size_t in_nbytes,
			 void *out, size_t out_nbytes_avail);

/* libdeflate.h:150-152 */
LIBDEFLATEAPI size_t
libdeflate_gzip_compress_bound(struct libdeflate_compressor *compressor,
			       size_t in_nbytes);

/* libdeflate.h:159-160; NULL is a no-op */
LIBDEFLATEAPI void
libdeflate_free_compressor(struct libdeflate_compressor *compressor);

/* libdeflate.h:181-182 */
LIBDEFLATEAPI struct libdeflate_decompressor *
libdeflate_alloc_decompressor(void);

/* libdeflate.h:187-188 */
LIBDEFLATEAPI struct libdeflate_decompressor *
libdeflate_alloc_decompressor_ex(const struct libdeflate_options *options);

/* libdeflate.h:242-246 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_deflate_decompress(struct libdeflate_decompressor *decompressor,
			      const void *in, size_t in_nbytes,
			      void *out, size_t out_nbytes_avail,
			      size_t *actual_out_nbytes_ret);

/* libdeflate.h:254-259 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_deflate_decompress_ex(struct libdeflate_decompressor *decompressor,
				 const void *in, size_t in_nbytes,
				 void *out, size_t out_nbytes_avail,
				 size_t *actual_in_nbytes_ret,
				 size_t *actual_out_nbytes_ret);

/* libdeflate.h:269-273 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_zlib_decompress(struct libdeflate_decompressor *decompressor,
			   const void *in, size_t in_nbytes,
			   void *out, size_t out_nbytes_avail,
			   size_t *actual_out_nbytes_ret);

/* libdeflate.h:282-287 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_zlib_decompress_ex(struct libdeflate_decompressor *decompressor,
			      const void *in, size_t in_nbytes,
			      void *out, size_t out_nbytes_avail,
			      size_t *actual_in_nbytes_ret,
			      size_t *actual_out_nbytes_ret);

/* libdeflate.h:297-301 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_gzip_decompress(struct libdeflate_decompressor *decompressor,
			   const void *in, size_t in_nbytes,
			   void *out, size_t out_nbytes_avail,
			   size_t *actual_out_nbytes_ret);

/* libdeflate.h:310-315 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_gzip_decompress_ex(struct libdeflate_decompressor *decompressor,
			      const void *in, size_t in_nbytes,
			      void *out, size_t out_nbytes_avail,
			      size_t *actual_in_nbytes_ret,
			      size_t *actual_out_nbytes_ret);

/* libdeflate.h:322-323; NULL is a no-op */
LIBDEFLATEAPI void
libdeflate_free_decompressor(struct libdeflate_decompressor *decompressor);

/* libdeflate.h:335-336; initial value 1; buffer == NULL -> 1 */
LIBDEFLATEAPI uint32_t
libdeflate_adler32(uint32_t adler, const void *buffer, size_t len);

/* libdeflate.h:345-346; initial value 0; buffer == NULL -> 0 */
LIBDEFLATEAPI uint32_t
libdeflate_crc32(uint32_t crc, const void *buffer, size_t len);

/* libdeflate.h:363-365 */
LIBDEFLATEAPI void
libdeflate_set_memory_allocator(void *(*malloc_func)(size_t),
				void (*free_func)(void *));

/* ------------------------------------------------------------------ */
/* (2) batch extension: N independent chunks resident in HBM            */
/* ------------------------------------------------------------------ */

enum libdeflate_amd_format {
	LIBDEFLATE_AMD_DEFLATE = 0,	/* raw DEFLATE     */
	LIBDEFLATE_AMD_ZLIB = 1,	/* + 2 B header, Adler-32 footer (BE) */
	LIBDEFLATE_AMD_GZIP = 2,	/* + 10 B header, CRC-32 + ISIZE (LE) */
	LIBDEFLATE_AMD_BGZF = 3,	/* gzip member with BGZF's 18 B header (below) */
};

/* status of the library itself (not of a stream) */
enum libdeflate_amd_status {
	LIBDEFLATE_AMD_OK = 0,
	LIBDEFLATE_AMD_NO_DEVICE = -1,	/* no gfx950 device / HIP runtime error */
	LIBDEFLATE_AMD_BAD_ARG = -2,
	LIBDEFLATE_AMD_OOM = -3,	/* hipMalloc of scratch failed */
};

/* 0 when a usable device is present; never falls back to the CPU */
LIBDEFLATEAPI int
libdeflate_amd_device_ready(void);
/* human-readable reason for the last non-OK status (thread-local) */
LIBDEFLATEAPI const char *
libdeflate_amd_last_error(void);
/* The tuning switches of INTEGRATION.md (LDA_* environment variables) are
 * read ONCE, when the library is loaded - not per call.  A process that
 * changes them afterwards calls this to have them read again (not to be
 * called while batches are in flight). */
LIBDEFLATEAPI void
libdeflate_amd_reload_env(void);

/*
 * Devices.  An object (compressor / decompressor) belongs to the HIP device
 * that was current when it was allocated; every call that takes the object
 * runs there, whatever device the calling thread has current, and puts the
 * caller's device back (libdeflate.h has no notion of a device).  The
 * device-pointer batch calls expect their buffers and their stream on the
 * object's device.
 *
 * The host-pointer batch calls (libdeflate_amd_*_batch_host) can use every GPU
 * of the node from ONE object: with LDA_DEVICES=all (or =N) in the environment
 * a batch is cut into contiguous shards of about equal byte counts, shard k
 * runs on visible device (own + k) through an object and a host thread of its
 * own, and every result lands where the caller asked for it - host order, no
 * gather.  Unset (the default) or one visible GPU: one shard, the
 * single-device path.  Returns the shards the calling thread's last
 * host-pointer batch was spread over.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_last_fanout(void);

/*
 * Two hardware behaviours are checked on every device before its first use
 * (~1 ms, once per device and process; LDA_NO_SELFCHECK skips it): the lane
 * order of conflicting LDS atomics (the compress kernel relies on it beyond
 * what the ISA manual states) and - a belt: the kernels wait for their stores
 * first, which is architected - that a wave's global store is visible to
 * another lane's plain load behind s_waitcnt vmcnt(0).  A device that
 * deviates is refused - the allocators return NULL and
 * libdeflate_amd_last_error() says why.  This runs the check again on the
 * current device: out[0..4] = LDS-atomic lanes checked, of them out of order,
 * same-instruction conflicts among them, loads checked, of them stale.
 * Returns LIBDEFLATE_AMD_OK when the device passes.
 */
LIBDEFLATEAPI int
libdeflate_amd_selfcheck(uint64_t *out /* [5], may be NULL */);

/*
 * Chunk i of a batch occupies bytes [offsets[i], offsets[i] + nbytes[i]) of a
 * base buffer.  `d_` pointers are device pointers.  Offsets/sizes are u64 so
 * the same descriptors serve 4 KiB filesystem blocks and multi-GiB buffers.
 *
 * Compress: for each chunk writes a complete stream of `format` into its
 * output slot and the stream size into d_out_nbytes[i] (0 = did not fit in
 * d_out_avail[i], same rule as libdeflate.h:73-74).
 * Batch counterpart of libdeflate_{deflate,zlib,gzip}_compress
 * (libdeflate.h:85-88,122-125,140-143).
 */
LIBDEFLATEAPI int
libdeflate_amd_compress_batch(struct libdeflate_compressor *compressor,
			      int format, size_t n_chunks,
			      const void *d_in, const uint64_t *d_in_offsets,
			      const uint64_t *d_in_nbytes,
			      void *d_out, const uint64_t *d_out_offsets,
			      const uint64_t *d_out_avail,
			      uint64_t *d_out_nbytes, void *stream);

/*
 * The same with an upper bound of the chunk sizes stated by the caller (the
 * sizes themselves live in HBM, where the host cannot see them): batches of
 * small chunks - at most 4096 bytes, the filesystem-block shape - run on a
 * kernel that keeps three chunks per CU in flight instead of one.  The bound
 * is a promise, and it is only CHECKED where it selects that kernel (bound <=
 * 4096, levels 0-9): there a chunk larger than the bound reports 0, like one
 * that does not fit its slot.  With any other bound, or at levels 10-12,
 * chunks of any size are compressed.  (At levels 0-9 a batch of at least four
 * chunks per CU runs in two kernels whose scratch is sized by the bound; a
 * chunk larger than the bound is compressed by the one-kernel path behind
 * them, into the same bytes.)
 */
LIBDEFLATEAPI int
libdeflate_amd_compress_batch_bounded(struct libdeflate_compressor *compressor,
				      int format, size_t n_chunks,
				      const void *d_in, const uint64_t *d_in_offsets,
				      const uint64_t *d_in_nbytes,
				      void *d_out, const uint64_t *d_out_offsets,
				      const uint64_t *d_out_avail,
				      uint64_t *d_out_nbytes, size_t max_in_nbytes,
				      void *stream);

/*
 * How the last batch call on this compressor was scheduled (diagnostics; tests
 * use it to see which schedule ran): [0] 1 = the two-kernel path, [1] 1 = its
 * last chunks (the tail) ran on the compressor's own stream beside the others
 * (the head) on the caller's, joined again before the call's work ends on the
 * caller's stream (LDA_COMPRESS_OVERLAP=0: never); [2] chunks of the head,
 * [3] of the tail, summed over the call's launches.
 */
LIBDEFLATEAPI void
libdeflate_amd_compress_last_schedule(const struct libdeflate_compressor *compressor,
				      uint32_t out[4]);

/*
 * The name of the compress kernel that call launched (diagnostics, as above):
 * on the two-kernel path the LZ77 stage, which at levels 1-9 is the kernel
 * built for the level ("lda_deflate_batch_kernel_l6") unless
 * LDA_COMPRESS_SPECIALIZE=0 keeps the one that serves every level
 * ("lda_deflate_batch_kernel").  A static string; "" before the first call.
 */
LIBDEFLATEAPI const char *
libdeflate_amd_compress_last_kernel(const struct libdeflate_compressor *compressor);

/*
 * Decompress: d_results[i] receives the enum libdeflate_result of chunk i.
 * d_actual_in / d_actual_out may be NULL; a NULL d_actual_out has the
 * reference's meaning (the stream must fill d_out_avail[i] exactly, else
 * SHORT_OUTPUT, decompress_template.h:765-770).  A failed chunk never
 * affects its neighbours.  Batch counterpart of
 * libdeflate_{deflate,zlib,gzip}_decompress_ex (libdeflate.h:254-259,
 * 282-287,310-315).
 */
LIBDEFLATEAPI int
libdeflate_amd_decompress_batch(struct libdeflate_decompressor *decompressor,
				int format, size_t n_chunks,
				const void *d_in, const uint64_t *d_in_offsets,
				const uint64_t *d_in_nbytes,
				void *d_out, const uint64_t *d_out_offsets,
				const uint64_t *d_out_avail,
				int32_t *d_results,
				uint64_t *d_actual_in, uint64_t *d_actual_out,
				void *stream);

/*
 * Preset dictionaries (zlib's deflateSetDictionary / inflateSetDictionary,
 * the FDICT / DICTID fields of RFC 1950 2.2), for LIBDEFLATE_AMD_DEFLATE and
 * LIBDEFLATE_AMD_ZLIB.  zlib refuses a dictionary on a gzip stream, and so do
 * these calls: the batch forms return LIBDEFLATE_AMD_BAD_ARG, the
 * single-buffer forms report it like their counterparts report a bad
 * argument - compress returns 0, decompress LIBDEFLATE_BAD_DATA - with the
 * reason in libdeflate_amd_last_error().
 *
 * One dictionary serves every chunk of a batch.  dict_nbytes == 0 gives
 * exactly the result of the call without a dictionary (dict may then be
 * NULL).  Semantics are zlib's:
 *  - compress primes the window with the dictionary's last
 *    min(dict_nbytes, LIBDEFLATE_AMD_DICT_WINDOW) bytes - what the compress
 *    kernel's window holds ahead of a chunk; a longer dictionary is not an
 *    error.  zlib streams get FDICT and DICTID = the Adler-32 of the WHOLE
 *    dictionary, big-endian, after the 2-byte header; the footer stays the
 *    Adler-32 of the chunk alone.  Such a stream takes 4 bytes more than
 *    libdeflate_zlib_compress_bound().
 *  - decompress accepts a dictionary of any length and uses its last 32 KiB.
 *    Raw DEFLATE: a distance may reach min(dict_nbytes, 32768) bytes before
 *    the output; further is BAD_DATA.  zlib: a stream with FDICT must name
 *    the dictionary's Adler-32 in DICTID (else BAD_DATA, also when
 *    dict_nbytes == 0); a stream without FDICT decodes as if no dictionary
 *    were given.  actual_in counts the 4 DICTID bytes.
 *  - the calls without a dictionary still reject FDICT.
 *
 * Device batches: the arguments of libdeflate_amd_compress_batch /
 * libdeflate_amd_decompress_batch plus d_dict, a device pointer on the
 * object's device that stays valid until the batch completes.  They only
 * enqueue (the DICTID is computed on the device).  Every chunk, also one of a
 * few bytes, runs on the ordinary compress kernel.
 */
#define LIBDEFLATE_AMD_DICT_WINDOW 20480

LIBDEFLATEAPI int
libdeflate_amd_compress_batch_dict(struct libdeflate_compressor *compressor,
				   int format, size_t n_chunks,
				   const void *d_dict, size_t dict_nbytes,
				   const void *d_in, const uint64_t *d_in_offsets,
				   const uint64_t *d_in_nbytes,
				   void *d_out, const uint64_t *d_out_offsets,
				   const uint64_t *d_out_avail,
				   uint64_t *d_out_nbytes, void *stream);

LIBDEFLATEAPI int
libdeflate_amd_decompress_batch_dict(struct libdeflate_decompressor *decompressor,
				     int format, size_t n_chunks,
				     const void *d_dict, size_t dict_nbytes,
				     const void *d_in, const uint64_t *d_in_offsets,
				     const uint64_t *d_in_nbytes,
				     void *d_out, const uint64_t *d_out_offsets,
				     const uint64_t *d_out_avail,
				     int32_t *d_results,
				     uint64_t *d_actual_in, uint64_t *d_actual_out,
				     void *stream);

/*
 * Uncompressed sizes of a batch, without decoding it.  Every decompress call
 * wants the output size in advance, and a raw DEFLATE or zlib stream does not
 * state it (a gzip footer states it modulo 2^32, and nothing vouches for it);
 * the reference's callers guess, decode, and double on INSUFFICIENT_SPACE.
 * Here the decoder itself counts: the same parser as the decompress calls,
 * with no output buffer, no scratch and nothing written but the results.
 *
 * For stream i with limit L[i] = d_out_limit[i] (d_out_limit NULL, or a limit
 * above it: LIBDEFLATE_AMD_SIZE_LIMIT_MAX), the call reports what
 * libdeflate_{deflate,zlib,gzip}_decompress_ex reports for the same bytes
 * with out_nbytes_avail = L[i] and a non-NULL actual_out_nbytes_ret - with ONE
 * exception: the CRC-32 / Adler-32 of the produced bytes is not checked,
 * because there are no bytes.  Everything else is: the container header's
 * rules, FDICT, reserved flags, every code and distance rule, the overread
 * rule, the footer's presence, and for gzip ISIZE == the count modulo 2^32.
 *  - SUCCESS: d_out_nbytes[i] = the reference's actual_out, d_actual_in[i] =
 *    its actual_in (header and footer included);
 *  - a failed stream (BAD_DATA, or INSUFFICIENT_SPACE when it produces more
 *    than L[i]) reports size 0 and actual_in 0, and never affects its
 *    neighbours;
 *  - a stream with a wrong checksum is SUCCESS here and BAD_DATA when decoded;
 *  - streams of 4 GiB and more are not supported: they report
 *    INSUFFICIENT_SPACE.
 * d_actual_in may be NULL.  The device forms only enqueue on `stream`;
 * LIBDEFLATE_AMD_BAD_ARG for NULL pointers and formats other than DEFLATE /
 * ZLIB / GZIP (BGZF members state their size: the BGZF reader takes it from
 * there), before any device is touched; n_chunks == 0 is OK.
 *
 * _dict: the dictionary semantics of libdeflate_amd_decompress_batch_dict (a
 * count needs the dictionary's length and, for zlib, its Adler-32, computed
 * on the device); a gzip format is BAD_ARG.
 *
 * _host: host pointers, blocking; only the inputs go to the device and three
 * small arrays come back.  out_limit and actual_in may be NULL.  Spread over
 * the GPUs of a node by LDA_DEVICES like the other host-pointer batches.
 */
#define LIBDEFLATE_AMD_SIZE_LIMIT_MAX 0xFFFFFFFFull	/* limit used for a NULL d_out_limit */

LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch(struct libdeflate_decompressor *decompressor,
				      int format, size_t n_chunks,
				      const void *d_in, const uint64_t *d_in_offsets,
				      const uint64_t *d_in_nbytes,
				      const uint64_t *d_out_limit,
				      int32_t *d_results,
				      uint64_t *d_actual_in, uint64_t *d_out_nbytes,
				      void *stream);

LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch_dict(struct libdeflate_decompressor *decompressor,
					   int format, size_t n_chunks,
					   const void *d_dict, size_t dict_nbytes,
					   const void *d_in, const uint64_t *d_in_offsets,
					   const uint64_t *d_in_nbytes,
					   const uint64_t *d_out_limit,
					   int32_t *d_results,
					   uint64_t *d_actual_in, uint64_t *d_out_nbytes,
					   void *stream);

LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch_host(struct libdeflate_decompressor *decompressor,
					   int format, size_t n_chunks,
					   const void *const *in, const size_t *in_nbytes,
					   const size_t *out_limit, int32_t *results,
					   size_t *actual_in, size_t *out_nbytes);

/*
 * Decompress a batch whose sizes nobody knows into ONE buffer, back to back:
 * sizes, places, decode - one call, nothing but enqueues on `stream`.
 *  1. the size query above with the maximum limit;
 *  2. d_out_offsets[i] = exclusive prefix sum of the sizes, each rounded up to
 *     out_align (a power of two, 1 .. 256, else BAD_ARG; 16 keeps the decode
 *     kernel's 16-byte stores aligned).  A failed stream counts 0.
 *     d_out_offsets has n_chunks + 1 entries: the last is the total the batch
 *     needs, whatever out_capacity is;
 *  3. every stream is decoded into d_out + d_out_offsets[i] with exactly its
 *     size as room, all checks including the checksums.
 * d_results[i]: a stream that failed the size query keeps that verdict and is
 * not decoded; one with d_out_offsets[i] + size > out_capacity is
 * INSUFFICIENT_SPACE, is not decoded and nothing of it is written; every
 * other stream has the verdict of libdeflate_amd_decompress_batch - so a
 * stream with a wrong checksum is BAD_DATA here, with its slot still reserved.
 * d_actual_out[i] (required) and d_actual_in[i] (may be NULL) are 0 for a
 * stream that did not succeed.  A caller whose buffer was too small reads
 * d_out_offsets[n_chunks], allocates and calls again; a caller whose buffer
 * was large enough never synchronises.
 */
LIBDEFLATEAPI int
libdeflate_amd_decompress_batch_packed(struct libdeflate_decompressor *decompressor,
				       int format, size_t n_chunks,
				       const void *d_in, const uint64_t *d_in_offsets,
				       const uint64_t *d_in_nbytes,
				       void *d_out, size_t out_capacity, size_t out_align,
				       uint64_t *d_out_offsets,
				       int32_t *d_results,
				       uint64_t *d_actual_in, uint64_t *d_actual_out,
				       void *stream);

/*
 * Single buffer, host pointers, blocking - like libdeflate_*_compress and
 * libdeflate_*_decompress_ex.  Compress returns the bytes written, 0 when
 * they do not fit; inputs of 128 KiB and more are compressed in segments side
 * by side like libdeflate_*_compress, the first primed with the dictionary.
 * Decompress runs as a batch of one: the many-wave path that
 * libdeflate_*_decompress takes for large streams does not take dictionary
 * streams.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_compress_dict(struct libdeflate_compressor *compressor, int format,
			     const void *dict, size_t dict_nbytes,
			     const void *in, size_t in_nbytes,
			     void *out, size_t out_nbytes_avail);

LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_decompress_dict_ex(struct libdeflate_decompressor *decompressor,
				  int format, const void *dict, size_t dict_nbytes,
				  const void *in, size_t in_nbytes,
				  void *out, size_t out_nbytes_avail,
				  size_t *actual_in_nbytes_ret,
				  size_t *actual_out_nbytes_ret);

/*
 * Checksums of N chunks.  d_init may be NULL (CRC: 0, Adler: 1), otherwise
 * d_init[i] is the running value to continue from (libdeflate.h:326-346).
 */
LIBDEFLATEAPI int
libdeflate_amd_crc32_batch(size_t n_chunks, const void *d_in,
			   const uint64_t *d_offsets, const uint64_t *d_nbytes,
			   const uint32_t *d_init, uint32_t *d_out,
			   void *stream);
LIBDEFLATEAPI int
libdeflate_amd_adler32_batch(size_t n_chunks, const void *d_in,
			     const uint64_t *d_offsets,
			     const uint64_t *d_nbytes,
			     const uint32_t *d_init, uint32_t *d_out,
			     void *stream);

/*
 * Compaction of a batch's ragged outputs (what a caller of the reference does
 * with the sizes libdeflate_*_compress returns: write them back to back,
 * programs/gzip.c:149-185).  Copies d_nbytes[i] bytes from d_in +
 * d_in_offsets[i] to d_out + d_out_offsets[i], where d_out_offsets[0..n) is
 * the exclusive prefix sum of d_nbytes (computed here) and d_out_offsets[n]
 * the total.  d_out_offsets must have room for
 * libdeflate_amd_compact_offsets_len(n) entries (the tail is scan scratch).
 * d_out must not overlap the inputs.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_compact_offsets_len(size_t n_chunks);
LIBDEFLATEAPI int
libdeflate_amd_compact_batch(size_t n_chunks, const void *d_in,
			     const uint64_t *d_in_offsets,
			     const uint64_t *d_nbytes, void *d_out,
			     uint64_t *d_out_offsets, void *stream);

/*
 * Objects and streams: the batch calls only ENQUEUE work on `stream`.  A
 * compressor / decompressor owns device scratch (match lists, token scratch,
 * per-chunk sums, work counters) that a batch uses until it completes, so an
 * object may have batches in flight on ONE stream at a time (they are ordered
 * by the stream); use one object per stream for concurrent batches, exactly
 * as the reference asks for one object per thread (libdeflate.h:56-57,
 * :178-179).  Chunks of 4 GiB and more are not supported by the batch
 * kernels (positions are 32-bit): such a chunk reports 0 / BAD_DATA.  The
 * single-buffer libdeflate_*_compress calls take inputs of any size (they cut
 * them into 64 KiB segments that run as one batch and stitch the streams);
 * the single-buffer decompress calls are limited to streams of less than
 * 4 GiB each.
 */

/*
 * Convenience forms taking HOST arrays of per-chunk host pointers (what a
 * cgo/JNI/ctypes caller holding ordinary buffers has).  They pack the batch
 * into pinned host memory, move it as a few large DMA transfers (not one copy
 * per chunk), run the device batch above, compact the outputs on the device
 * and bring them back the same way; blocking.
 * results/actual_* have the meaning above.
 */
LIBDEFLATEAPI int
libdeflate_amd_compress_batch_host(struct libdeflate_compressor *compressor,
				   int format, size_t n_chunks,
				   const void *const *in,
				   const size_t *in_nbytes,
				   void *const *out, const size_t *out_avail,
				   size_t *out_nbytes);
LIBDEFLATEAPI int
libdeflate_amd_decompress_batch_host(struct libdeflate_decompressor *d,
				     int format, size_t n_chunks,
				     const void *const *in,
				     const size_t *in_nbytes,
				     void *const *out, const size_t *out_avail,
				     int32_t *results, size_t *actual_in,
				     size_t *actual_out /* NULL allowed */);

/*
 * What the last single-buffer libdeflate_*_decompress[_ex] call of this thread
 * did with its stream (diagnostics; tests use it to see that a large stream
 * really went over many waves): [0] 1 = decoded on the many-wave path, 0 = on
 * one wave; [1] why not (0 none, 1 switched off or too small, 2 container
 * header, 3 chain, 4 a chunk failed, 5 no final block, 6 output does not fit,
 * 7 output does not fill, 8 decode pass disagrees, 9 device, 10 too many
 * repairs); [2] bit offsets that passed the first filter of the block finder;
 * [3] block starts found; [4] chunks planned; [5] repairs; [6] chunks decoded;
 * [7] bytes produced; [8..13] host-side microseconds of: copy in, block finder,
 * count pass + chain, queueing the decode / window / resolve / checksum kernels,
 * footer check, output copy (which waits for those kernels); [14] input windows;
 * [15] chunks the host made itself from runs of stored blocks (no count pass).
 * libdeflate_amd_decompress_large is described the same way; nothing is copied
 * in or out there, and [8] is the time for the stream's head bytes (and for
 * the bits and rows fetched where a window begins at a block boundary), [13]
 * the wait for the last kernel.
 */
#define LIBDEFLATE_AMD_STREAM_STATS 16
LIBDEFLATEAPI void
libdeflate_amd_stream_stats(uint64_t *out /* [16] */);

/*
 * A gzip buffer of SEVERAL members (concatenated .gz files, pigz -i, BGZF).
 * libdeflate_gzip_decompress decodes the first member only
 * (lib/gzip_decompress.c:103-131, libdeflate.h:289-296); its caller loops, as
 * programs/gzip.c:236-299 does.  This is that loop in one call: members that
 * state their size (BGZF "BC" extra subfield) are indexed from their headers
 * and decoded as ONE device batch, anything else member after member.  `out`
 * receives the members' outputs back to back; fails with the first member's
 * non-success result.  The three result pointers may be NULL.
 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_gzip_decompress_members(struct libdeflate_decompressor *d,
				       const void *in, size_t in_nbytes,
				       void *out, size_t out_nbytes_avail,
				       size_t *actual_in_nbytes_ret,
				       size_t *actual_out_nbytes_ret,
				       size_t *members_ret);

/*
 * BGZF (blocked gzip, SAM/BAM spec 4.1: BAM, tabix, bgzip, .vcf.gz): a file
 * is a run of gzip members of at most LIBDEFLATE_AMD_BGZF_BLOCK input bytes
 * each, ended by a fixed 28-byte empty member (the EOF marker).  Every member
 * starts with htslib's 16 bytes
 *     1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00
 * (FEXTRA, MTIME 0, XFL 0, OS 0xff, XLEN 6, subfield "BC" of length 2)
 * followed by BSIZE = member size - 1 as u16 LE, so a member is at most
 * LIBDEFLATE_AMD_BGZF_MEMBER_MAX bytes.  Its deflate body is byte for byte
 * what LIBDEFLATE_AMD_GZIP gives the same block at the same level; the
 * blocks are independent (no window crosses a member boundary), so a reader
 * may start at any member.
 *
 * LIBDEFLATE_AMD_BGZF is also a format of libdeflate_amd_compress_batch,
 * _bounded and _batch_host, for callers who cut their own blocks (htslib cuts
 * them at record boundaries): chunk i becomes one member in slot i; a chunk
 * of more than LIBDEFLATE_AMD_BGZF_BLOCK bytes, or one whose member does not
 * fit min(out_avail[i], LIBDEFLATE_AMD_BGZF_MEMBER_MAX), reports 0.  The
 * dictionary calls and the decompress batch refuse the format: members
 * decode as LIBDEFLATE_AMD_GZIP, whole files with the BGZF reader below
 * (libdeflate_amd_bgzf_decompress[_batch]) or, from host memory and for gzip
 * files of any kind, with libdeflate_amd_gzip_decompress_members.
 */
#define LIBDEFLATE_AMD_BGZF_BLOCK	65280	/* input bytes per member (htslib BGZF_BLOCK_SIZE) */
#define LIBDEFLATE_AMD_BGZF_MEMBER_MAX	65536	/* BSIZE + 1 is 16 bits */
#define LIBDEFLATE_AMD_BGZF_EOF_BYTES	28	/* the EOF member */
#define LIBDEFLATE_AMD_BGZF_NO_EOF	1	/* flag: omit the EOF member (appending writers) */

/*
 * Bytes a BGZF file of in_nbytes input needs at most: m members of at most
 * LIBDEFLATE_AMD_BGZF_MEMBER_MAX bytes, m = ceil(in_nbytes / 65280), and the
 * EOF member.  compressor may be NULL.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_bgzf_compress_bound(struct libdeflate_compressor *compressor,
				   size_t in_nbytes);

/*
 * A whole BGZF file from ONE device buffer d_in of in_nbytes bytes: block k
 * is bytes [65280 k, 65280 (k + 1)), the last one shorter; in_nbytes == 0
 * gives m = 0 members, the EOF member alone.  Enqueues on `stream` and
 * returns; d_out_nbytes[0] (device memory) receives the file's size, or 0
 * when a member did not fit (cannot happen) or the file does not fit
 * out_avail - then nothing is written past out_avail, and d_index is
 * undefined.  (With LIBDEFLATE_AMD_BGZF_NO_EOF and in_nbytes == 0 the size is
 * 0 too: there is nothing to write.)
 *
 * d_index: NULL, or device room for 2 (m + 1) u64: the pairs (compressed
 * offset, uncompressed offset) of the start of every member, and as pair m
 * (offset of the EOF member - or where it would be under NO_EOF -,
 * in_nbytes).  flags: 0 or LIBDEFLATE_AMD_BGZF_NO_EOF.
 *
 * The arguments are checked before any device work: LIBDEFLATE_AMD_BAD_ARG
 * for a NULL object or pointer, unknown flags, or an out_avail below 27 bytes
 * per member plus the EOF member (no file can fit that).  d_out must not
 * overlap d_in.  The object's scratch holds the m members before they are
 * packed (64 KiB per member).
 */
LIBDEFLATEAPI int
libdeflate_amd_bgzf_compress_batch(struct libdeflate_compressor *compressor,
				   const void *d_in, size_t in_nbytes,
				   void *d_out, size_t out_avail,
				   uint64_t *d_out_nbytes, uint64_t *d_index,
				   unsigned flags, void *stream);

/*
 * The same from and to HOST memory, blocking: returns the file's size, 0 when
 * it does not fit out_avail or an argument is bad (reason in
 * libdeflate_amd_last_error()).  index: NULL, or index_avail u64 entries of
 * which 2 (m + 1) are written as above.  The bytes are those of
 * libdeflate_amd_bgzf_compress_batch; large inputs go through in slices whose
 * transfers overlap the kernels.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_bgzf_compress(struct libdeflate_compressor *compressor,
			     const void *in, size_t in_nbytes,
			     void *out, size_t out_avail,
			     uint64_t *index, size_t index_avail, unsigned flags);

/*
 * ONE ordinary stream - raw DEFLATE, zlib or .gz, what gzip -d, zlib or a PNG
 * reader take - from ONE device buffer d_in of in_nbytes bytes, for callers
 * whose data is in device memory already and who would otherwise copy it to
 * the host for libdeflate_<format>_compress.  format: LIBDEFLATE_AMD_DEFLATE,
 * _ZLIB or _GZIP (BGZF has its own writer above).
 *
 * The bytes written to d_out and the size written to d_out_nbytes[0] are,
 * byte for byte, what libdeflate_<format>_compress() of this build returns
 * for the same bytes, level and LDA_* switches, for every in_nbytes including
 * 0: an input of 128 KiB or more at level 1 and above is cut into segments of
 * 16, 32 or 64 KiB that are compressed side by side, each primed with the
 * tail of its predecessor, anything else is one chunk of the batch.  So
 * libdeflate_<format>_compress_bound(in_nbytes) is enough room wherever it is
 * for that call, and there is no bound function of its own.
 *
 * d_in, d_out and d_out_nbytes are device pointers on the object's device;
 * d_out must not overlap d_in.  The call only ENQUEUES on `stream` and
 * returns: nothing is copied to or from the host and nothing is waited for -
 * the descriptors, the checksum of the whole buffer (combined on the device
 * from the segments' checksums), the container's header and footer and the
 * size are all written by kernels.  Only the object's scratch growing, on its
 * first call or a larger one, waits for the device, as every other growth of
 * an object's scratch does.  d_out_nbytes[0] = 0 when the stream does not fit
 * out_avail (the rule of libdeflate.h:73-74): then no byte is written at or
 * past d_out + out_avail, and what lies below it is undefined.
 *
 * The arguments are checked before any device work: LIBDEFLATE_AMD_BAD_ARG,
 * with the reason in libdeflate_amd_last_error(), for a NULL object, a NULL
 * d_in with in_nbytes != 0, a NULL d_out or d_out_nbytes, another format, or
 * an out_avail that cannot hold the container's header and footer and one
 * byte more.  Inputs of 4 GiB and more work as in the host call (64 KiB
 * segments, 64-bit offsets, gzip's ISIZE modulo 2^32), limited by the scratch
 * alone: LIBDEFLATE_AMD_OOM.  The scratch belongs to the object and goes with
 * it: per segment a slot of compress_bound(segment) + 32 bytes, seven u64 of
 * descriptors, its checksum and its offset.  The rule for objects and streams
 * above holds unchanged.  Preset dictionaries are out of scope:
 * libdeflate_amd_compress_dict stays the only large-buffer form with one.
 */
LIBDEFLATEAPI int
libdeflate_amd_compress_large_batch(struct libdeflate_compressor *compressor,
				    int format,
				    const void *d_in, size_t in_nbytes,
				    void *d_out, size_t out_avail,
				    uint64_t *d_out_nbytes, void *stream);

/*
 * The way back: ONE stream - raw DEFLATE, zlib or .gz - that lies in DEVICE
 * memory (read by GPUDirect, received from another GPU, written by the call
 * above) into device memory, on many waves (the decoder behind
 * libdeflate_<format>_decompress for large host buffers), without the stream
 * or its output ever crossing to the host.  format: LIBDEFLATE_AMD_DEFLATE,
 * _ZLIB or _GZIP.  d_in and d_out are device pointers on the object's device,
 * of any alignment; d_out must not overlap d_in.
 *
 * The result, *actual_in_nbytes_ret and *actual_out_nbytes_ret are exactly
 * those of libdeflate_<format>_decompress_ex for the same bytes and
 * out_nbytes_avail: a NULL actual_out_nbytes_ret asks for an exact fill,
 * bytes behind the stream are allowed, and of a gzip buffer the first member
 * is decoded (the caller loops on actual_in, as with the reference).  Both
 * result pointers may be NULL.  No byte is written at or past d_out +
 * out_nbytes_avail; on a result other than LIBDEFLATE_SUCCESS what lies below
 * that is undefined, as libdeflate.h says.
 *
 * The call BLOCKS - it is not one of the enqueue-only _batch calls, hence its
 * name: the many-wave decoder's chain of chunks is checked by the host.
 * Before they first read d_in, the object's own streams wait (an event wait,
 * not a host wait) for what is queued on `stream` (NULL: the default stream),
 * so d_in may be the product of kernels queued there; when the call returns,
 * d_out is complete and any stream may read it.  What crosses to the host are
 * descriptors, per-chunk results, two small tables (the places where a stored
 * block could lie, the classes of the block headers) and a few dozen bytes of
 * the stream: its first 4 KiB at most for the container header, the footer,
 * 8 bytes where an input window begins at a block boundary.
 *
 * Which decoder answers follows the host call's rule, so the result cannot
 * depend on it: the many-wave path answers for a clean success or for a
 * footer that does not match a cleanly decoded stream; everything else - a
 * stream under LDA_STREAM_PAR_MIN bytes, LDA_NO_STREAM_PAR, a gzip header that
 * runs past 4 KiB, damaged data, an output that does not fit or fill - goes
 * to libdeflate_amd_decompress_batch as a batch of one on the object's
 * stream.  libdeflate_amd_stream_stats() says which it was.
 *
 * The arguments are checked before any device work: LIBDEFLATE_BAD_DATA, with
 * the reason in libdeflate_amd_last_error(), for a NULL object, a NULL d_in
 * with in_nbytes != 0, a NULL d_out with out_nbytes_avail != 0, or another
 * format.  A library-side failure (no device, no memory) is LIBDEFLATE_BAD_DATA
 * with its reason there too.  Streams of 4 GiB and more are as limited as in
 * the host call; preset dictionaries are out of scope.  The scratch (16-bit
 * symbols of the output, finder queues, a row per 64 bytes of an input window)
 * belongs to the object and goes with it.
 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_decompress_large(struct libdeflate_decompressor *decompressor, int format,
				const void *d_in, size_t in_nbytes,
				void *d_out, size_t out_nbytes_avail,
				size_t *actual_in_nbytes_ret, size_t *actual_out_nbytes_ret,
				void *stream);

/*
 * A SEEK INDEX over one plain stream, and reads through it: the counterpart
 * of the BGZF reader below for streams nobody prepared (gzip, pigz, zlib, a
 * web server, a PNG writer), which have no member boundaries to start at.
 *
 * libdeflate_amd_decompress_large_index is libdeflate_amd_decompress_large -
 * the same arguments, result, *actual_in_nbytes_ret, *actual_out_nbytes_ret,
 * the same rule for which decoder answers, no byte written at or past d_out +
 * out_nbytes_avail, blocking - and keeps what the many-wave decoder proved on
 * the way: POINTS at which a decode can start (a chunk of its chain: output
 * offset, exact start bit, governing block header), about every `spacing`
 * bytes of output, each with the 32 KiB of output in front of it.
 *
 * `index` (HOST, index_avail u64 entries) receives rows of
 * LIBDEFLATE_AMD_SEEK_WORDS = 4 u64:
 *   row 0        { magic / version word, format, byte offset of the raw
 *                  DEFLATE stream inside d_in (the container header), n }
 *   rows 1 .. n  the points { out_off, start_bit, hdr_bit, kind }: bits
 *                  relative to the raw stream; kind 0 = the point is the block
 *                  header at hdr_bit = start_bit, kind 2 = the token boundary
 *                  start_bit inside the block whose header is at hdr_bit
 *   row n + 1    { total output bytes, bytes of the raw stream up to the end
 *                  of its final block, footer bytes, end marker }
 * so 4 (n + 2) entries are written and *points_ret = n.  Point 0 is always the
 * stream's first bit at output offset 0; out_off and start_bit rise strictly.
 * d_windows (DEVICE, windows_avail bytes, any alignment) receives window k -
 * the output bytes [out_off - 32768, out_off) of point k, zeros below offset 0
 * - at d_windows + LIBDEFLATE_AMD_SEEK_WINDOW k.  The index is plain data: it
 * may be copied and kept as long as the stream's bytes stay what they are.
 *
 * Points are taken greedily: the first chunk of the chain at least `spacing`
 * bytes of output behind the last point.  A chunk that was decoded under the
 * static codes without its block's header cannot be one (it stops at its
 * block's end): a Z_FIXED stream of one giant block keeps few or no points
 * beyond point 0.  The capacity is min(index_avail / 4 - 2, windows_avail /
 * 32768) points; when the points do not fit, `spacing` is doubled until they
 * do, so the index always covers the whole stream.  Before the call returns
 * every interval (point k to point k + 1) is parsed once more from the point's
 * own row; a point whose interval does not end exactly at the next point with
 * exactly the bytes between is dropped.  When the sequential decoder answered
 * with LIBDEFLATE_SUCCESS (a stream under LDA_STREAM_PAR_MIN bytes,
 * LDA_NO_STREAM_PAR, ...) the index is point 0 and the closing row.  On any
 * other result *points_ret = 0 and the index is undefined.
 *
 * Refused before any device work, LIBDEFLATE_BAD_DATA with the reason in
 * libdeflate_amd_last_error(): what libdeflate_amd_decompress_large refuses, a
 * capacity below 1, spacing == 0, a NULL index, points_ret or d_windows.
 * Nothing is written through the result pointers then.
 *
 * What it costs: 32 KiB of device memory and 32 bytes of host memory per
 * point, one more parse of the stream for the check, one gather kernel.  Out
 * of scope: preset dictionaries, further gzip members (the first member is
 * indexed, as libdeflate_amd_decompress_large decodes it), streams of 4 GiB
 * and more, a host-pointer form, a file format for the index.
 */
#define LIBDEFLATE_AMD_SEEK_WINDOW 32768	/* bytes of d_windows per point */
#define LIBDEFLATE_AMD_SEEK_WORDS 4		/* u64 per row of the index */

LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_decompress_large_index(struct libdeflate_decompressor *decompressor, int format,
				      const void *d_in, size_t in_nbytes,
				      void *d_out, size_t out_nbytes_avail,
				      size_t *actual_in_nbytes_ret, size_t *actual_out_nbytes_ret,
				      size_t spacing,
				      uint64_t *index, size_t index_avail,
				      size_t *points_ret,
				      void *d_windows, size_t windows_avail,
				      void *stream);

/*
 * n_ranges pieces of the stream's output through such an index, back to back
 * into d_out; enqueues on `stream` only.  d_in / in_nbytes: the stream the
 * index was made from (its first in_nbytes bytes; at least what the closing
 * row needs).  `index` (index_words u64 entries, at least 4 (n + 2)) and
 * `ranges` (pairs (offset, length) in output bytes) are HOST arrays and may be
 * reused when the call returns; d_windows is the build's window array.
 *
 * Every interval a range touches is decoded ONCE, however many ranges touch
 * it: parsed (lda_stream_count_kernel), then - only if that parse ended at
 * the next point's start bit (the last interval: with the stream's final
 * block, at the raw stream's last byte) with exactly the bytes the index says
 * - decoded into 16-bit symbols in the object's scratch, whose slots are sized
 * from the index; then every range's share of it is resolved against the
 * interval's window into its place in d_out.  d_results[r] (device) = 0, or
 * LIBDEFLATE_BAD_DATA when an interval of range r did not parse as indexed or
 * refers to bytes in front of the stream; a failed range does not affect the
 * others (its bytes in d_out are undefined).  So a d_in or d_windows that does
 * not belong to the index cannot make the call write outside the object's
 * scratch and [d_out, d_out + out_avail).  There is NO CHECKSUM of a partial
 * read - no format states one: bytes of d_in changed so that an interval still
 * parses to the same end and length are not detected.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL pointer (d_out may be NULL when the
 * ranges are all empty), a bad magic word or format, rows that do not rise
 * strictly in out_off and start_bit, an index whose closing row needs more
 * input than in_nbytes, a range past the total, ranges that need more than
 * out_avail.  LIBDEFLATE_AMD_OOM when the scratch for the touched intervals
 * (2 bytes per byte of them, and 48 KiB per decoding wave) cannot be had.
 * d_out must not overlap d_in or d_windows.  The cost: two parses per touched
 * interval and the resolve, whatever part of the interval is wanted.
 */
LIBDEFLATEAPI int
libdeflate_amd_seek_read_batch(struct libdeflate_decompressor *decompressor,
			       const void *d_in, size_t in_nbytes,
			       const uint64_t *index, size_t index_words,
			       const void *d_windows,
			       size_t n_ranges, const uint64_t *ranges,
			       void *d_out, size_t out_avail, int32_t *d_results,
			       void *stream);

/*
 * Reading a BGZF file.  What a member is (htslib's check_header rule): the
 * bytes 1f 8b 08 04, XLEN = 6 at bytes 10..11, the subfield 42 43 02 00 at
 * bytes 12..15 and BSIZE at 16..17; MTIME, XFL and OS are free.  Its size is
 * BSIZE + 1: at least 28 bytes, not past the end of the file.  ISIZE (its
 * last 4 bytes) is at most 65536, the spec's limit - above the 65280 of our
 * writer.  The chain of members starts at byte 0 and must end exactly at
 * in_nbytes.  An empty member is an ordinary member of ISIZE 0 wherever it
 * stands (`cat a.gz b.gz` leaves an EOF member in the middle of a valid
 * file); LIBDEFLATE_AMD_BGZF_HAS_EOF only says whether the LAST member is the
 * 28 fixed bytes.  An empty file is 0 members and SUCCESS.  gzip members with
 * other extra fields, or plain concatenated gzip, are LIBDEFLATE_BAD_DATA
 * here: libdeflate_amd_gzip_decompress_members stays the general loop.
 */
#define LIBDEFLATE_AMD_BGZF_MORE_MEMBERS 16	/* result[0]: the file has more members than max_members */
#define LIBDEFLATE_AMD_BGZF_HAS_EOF 1		/* result[4] bit: the last member is the 28-byte EOF member */
#define LIBDEFLATE_AMD_BGZF_RESULT_WORDS 5
#define LIBDEFLATE_AMD_BGZF_VOFFSETS 2		/* read flag: ranges are virtual-offset pairs */

/*
 * A whole BGZF file in DEVICE memory -> its bytes in device memory.  Enqueues
 * on `stream` and returns; the members are found on the device (in parallel:
 * every offset is tested for the header rule, and only the candidates
 * reachable from offset 0 count), a prefix sum of their ISIZEs gives every
 * member its place, and one decompress batch decodes all of them there
 * (exact fill: a member whose ISIZE lies fails, nothing lands elsewhere).
 *
 * max_members: the launches and the scratch are sized on the host, which
 * does not know the member count; pass what is known (from a .gzi, from the
 * compress call's index: blocks + 1), at worst in_nbytes / 28 + 1.  A
 * generous bound costs empty chunks in the batch.
 *
 * d_result[0..4] (device memory):
 *   [0] an enum libdeflate_result value or LIBDEFLATE_AMD_BGZF_MORE_MEMBERS,
 *       in this order of precedence: LIBDEFLATE_BAD_DATA for a broken chain or
 *       header, or an ISIZE above 65536 (checked on the first max_members
 *       members); MORE_MEMBERS; LIBDEFLATE_INSUFFICIENT_SPACE when the sum of
 *       the ISIZEs exceeds out_avail - all three decided BEFORE the decode,
 *       and then nothing is decoded and d_out is not written; otherwise the
 *       result of the first member in file order that failed (a lying ISIZE
 *       is that member's SHORT_OUTPUT / INSUFFICIENT_SPACE, a bad CRC
 *       BAD_DATA, a deflate stream that ends before BSIZE says BAD_DATA);
 *   [1] members found (under MORE_MEMBERS: how many the file has; 0 under a
 *       pre-decode BAD_DATA);
 *   [2] compressed bytes consumed, [3] uncompressed bytes (both 0 under
 *       BAD_DATA before the decode and under MORE_MEMBERS);
 *   [4] flags: LIBDEFLATE_AMD_BGZF_HAS_EOF.
 * No byte is written past out_avail, whatever the file says.
 *
 * d_index: NULL, or device room for 2 (max_members + 1) u64: the pairs
 * (compressed offset, uncompressed offset) of every member, empty ones
 * included, then the closing pair (result[2], result[3]).  For a file of m
 * blocks from libdeflate_amd_bgzf_compress_batch the pairs 0..m are that
 * call's.  Written unless [0] is a pre-decode BAD_DATA or MORE_MEMBERS.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work for a NULL object or pointer
 * (d_out may be NULL only for an empty file), max_members == 0 with
 * in_nbytes != 0 or above 2^28, in_nbytes above 2^36.
 */
LIBDEFLATEAPI int
libdeflate_amd_bgzf_decompress_batch(struct libdeflate_decompressor *decompressor,
				     const void *d_in, size_t in_nbytes, size_t max_members,
				     void *d_out, size_t out_avail,
				     uint64_t *d_result, uint64_t *d_index, void *stream);

/* The index and the five words alone: nothing is decoded (out_avail counts
 * as unlimited, and member results cannot show). */
LIBDEFLATEAPI int
libdeflate_amd_bgzf_index_batch(struct libdeflate_decompressor *decompressor,
				const void *d_in, size_t in_nbytes, size_t max_members,
				uint64_t *d_result, uint64_t *d_index, void *stream);

/*
 * n_ranges pieces of the uncompressed data, back to back into d_out; enqueues
 * only.  `index` (members + 1 pairs as above, closing pair included) and
 * `ranges` are HOST arrays.  Range r is the bytes [ranges[2r], ranges[2r] +
 * ranges[2r + 1]), or with LIBDEFLATE_AMD_BGZF_VOFFSETS the BAM virtual
 * offsets [ranges[2r], ranges[2r + 1]) (coffset << 16 | uoffset; the closing
 * pair's coffset with uoffset 0 names the end).  Only the members a range
 * touches are decoded, all ranges as ONE batch: members wholly inside a
 * range straight into their place, the at most two edge members of a range
 * through 64 KiB slots of the object's scratch.  d_results[r] (device) = the
 * first non-success member result of range r, else 0; a failed range does
 * not affect the others.  LIBDEFLATE_AMD_BAD_ARG before any device work: a
 * NULL pointer, unknown flags, an index that does not describe BGZF members
 * inside in_nbytes, a range past the end of the data, a virtual offset whose
 * coffset is no member start of `index`, ranges that need more than
 * out_avail.  d_out must not overlap d_in; the host arrays may be reused
 * when the call returns.
 */
LIBDEFLATEAPI int
libdeflate_amd_bgzf_read_batch(struct libdeflate_decompressor *decompressor,
			       const void *d_in, size_t in_nbytes,
			       const uint64_t *index, size_t members,
			       size_t n_ranges, const uint64_t *ranges, unsigned flags,
			       void *d_out, size_t out_avail, int32_t *d_results,
			       void *stream);

/*
 * The whole file from and to HOST memory, blocking: a strict walk of the
 * headers on the host, then the host-pointer decompress batch.  Same rule,
 * same precedence of results as the device call; MORE_MEMBERS is returned
 * (as a value of the enum's type) when `index` is given and index_avail is
 * below 2 (members + 1) - *members_ret then says how many.  index: NULL or
 * index_avail u64 entries.  A NULL object or buffer, or an index_avail below
 * 2, is LIBDEFLATE_BAD_DATA with the reason in libdeflate_amd_last_error().
 * The result pointers may be NULL.
 */
LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_bgzf_decompress(struct libdeflate_decompressor *decompressor,
			       const void *in, size_t in_nbytes,
			       void *out, size_t out_avail,
			       size_t *actual_out_ret, size_t *members_ret,
			       uint64_t *index, size_t index_avail, unsigned *flags_ret);

/*
 * Reading a file of concatenated gzip members that do not state their size:
 * `cat a.gz b.gz`, WARC archives, mgzip / pgzip output, BGZF-like writers
 * other than htslib's.  What a member is: exactly what
 * libdeflate_gzip_decompress_ex accepts at that offset with the rest of the
 * file as its input - any MTIME / XFL / OS; FEXTRA, FNAME, FCOMMENT and FHCRC
 * skipped; reserved flag bits refused - with one limit of this reader's own:
 * FNAME and FCOMMENT together are at most LIBDEFLATE_AMD_GZM_NAME_MAX bytes,
 * terminators included; a header with more is no member here
 * (LIBDEFLATE_BAD_DATA where the chain needs it).  Every look-alike of a
 * header is parsed on speculation with the rest of the file behind it, and
 * the limit is what keeps a hostile file from making each of them walk to the
 * end of the file in search of a name's end.  The file is the chain of such members
 * from byte 0 that ends exactly at in_nbytes: the loop of
 * libdeflate_amd_gzip_decompress_members, so trailing bytes that are not a
 * member (zero padding included) and in_nbytes == 0 are LIBDEFLATE_BAD_DATA,
 * as they are there.
 */
#define LIBDEFLATE_AMD_GZM_MORE_MEMBERS     16	/* result[0]; same value as the BGZF reader's */
#define LIBDEFLATE_AMD_GZM_MORE_CANDIDATES  17	/* result[0] */
#define LIBDEFLATE_AMD_GZM_RESULT_WORDS     5
#define LIBDEFLATE_AMD_GZM_SLACK            1024	/* candidate room = max_members + this */
#define LIBDEFLATE_AMD_GZM_NAME_MAX         65536	/* bytes of FNAME + FCOMMENT of a member */

/*
 * The whole file in DEVICE memory -> its bytes in device memory.  Enqueues on
 * `stream` and returns, with the conventions of
 * libdeflate_amd_bgzf_decompress_batch: device pointers on the object's
 * device, scratch of the object, d_out must not overlap d_in, and no byte is
 * ever written at or past d_out + out_avail.
 *
 * A member's end is only known once its DEFLATE stream has been parsed, so the
 * members are found by speculation: every offset p with 1f 8b 08, FLG & 0xE0
 * == 0 and p + 18 <= in_nbytes is a CANDIDATE (payloads, names and chance
 * make false ones); one size query counts all candidates at once, each with
 * the rest of the file as its input; the candidates that the chain from
 * offset 0 reaches are the members; a prefix sum of their counted sizes gives
 * every member its place, and one decompress batch (exact input, exact fill)
 * decodes all of them there.
 *
 * max_members sizes the launches and the scratch on the host: the decode batch
 * has max_members chunks and the finder has room for max_members +
 * LIBDEFLATE_AMD_GZM_SLACK candidates.  A generous bound costs empty chunks.
 *
 * d_result[0..4] (device memory):
 *   [0] the verdict, the first of these that applies:
 *       1. LIBDEFLATE_AMD_GZM_MORE_CANDIDATES: the file has more candidates
 *          than max_members + LIBDEFLATE_AMD_GZM_SLACK;
 *       2. a broken chain - some position q < in_nbytes, reached from offset 0,
 *          starts no successfully counted member: the count's verdict of the
 *          candidate at q (LIBDEFLATE_BAD_DATA, or
 *          LIBDEFLATE_INSUFFICIENT_SPACE for a member of 4 GiB or more, the
 *          size query's limit), LIBDEFLATE_BAD_DATA when no candidate stands
 *          at q.  The count checks everything the decode checks but the
 *          CRC-32, a wrong ISIZE included;
 *       3. LIBDEFLATE_AMD_GZM_MORE_MEMBERS;
 *       4. LIBDEFLATE_INSUFFICIENT_SPACE: the sum of the sizes exceeds
 *          out_avail;
 *       (1 to 4 are decided BEFORE the decode: nothing is decoded then and
 *       d_out is not written)
 *       5. otherwise the decode result of the first member in file order that
 *          failed - a wrong CRC-32 is LIBDEFLATE_BAD_DATA there -, else
 *          LIBDEFLATE_SUCCESS.
 *       This is the host loop's result for every good file - where [1], [2]
 *       and [3] are its members, actual_in and actual_out too - and for every
 *       file with a single defect.
 *   [1] members; under MORE_MEMBERS how many the file has, under
 *       MORE_CANDIDATES how many candidates it has, 0 under a broken chain;
 *   [2] compressed bytes consumed, [3] uncompressed bytes: both 0 under every
 *       pre-decode verdict except 4., where they are the totals the file needs;
 *   [4] 0 (reserved).
 *
 * d_index: NULL, or device room for 2 (max_members + 1) u64: the pairs
 * (compressed offset, uncompressed offset) of every member, empty ones
 * included, then the closing pair (result[2], result[3]).  Written unless [0]
 * is one of the verdicts 1 to 3.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_out may be NULL
 * only with out_avail == 0, d_in only with in_nbytes == 0), max_members == 0
 * or above 2^28, in_nbytes above 2^36.
 *
 * Not covered: ranged reads through the index (with the index in hand,
 * libdeflate_amd_decompress_batch_packed over the chosen members does it); a
 * host-pointer form; the fallback loop of
 * libdeflate_amd_gzip_decompress_members, which stays as it is; members large
 * enough to want the many-wave decoder - every member is decoded by one wave
 * here, correct but slow for a file of a few huge members, for which
 * libdeflate_amd_decompress_large in a caller's loop stays the tool; preset
 * dictionaries; members of 4 GiB and more.
 */
LIBDEFLATEAPI int
libdeflate_amd_gzip_members_decompress_batch(struct libdeflate_decompressor *decompressor,
					     const void *d_in, size_t in_nbytes,
					     size_t max_members, void *d_out, size_t out_avail,
					     uint64_t *d_result, uint64_t *d_index, void *stream);

/* The index and the five words alone: everything but the decode (out_avail
 * counts as unlimited, and checksum failures cannot show). */
LIBDEFLATEAPI int
libdeflate_amd_gzip_members_index_batch(struct libdeflate_decompressor *decompressor,
					const void *d_in, size_t in_nbytes, size_t max_members,
					uint64_t *d_result, uint64_t *d_index, void *stream);

/*
 * Reading a ZIP archive (.zip, .jar, .whl, .docx, .npz) that lies in device
 * memory.  The reference has no ZIP reader: a ZIP tool walks the container and
 * hands raw DEFLATE to libdeflate_deflate_decompress; here the walk happens on
 * the device too.  What an archive is (tools/models/zip_walk.py restates the
 * rule on the CPU):
 *
 * END RECORD: the highest offset p >= in_nbytes - min(in_nbytes, 65557) that
 * carries 50 4b 05 06 and has p + 22 + comment_len <= in_nbytes.  Trailing
 * bytes behind it are tolerated, as Python's zipfile tolerates them; nothing
 * at or past in_nbytes is part of the file.  Its disk numbers must be 0 and
 * "entries on this disk" must equal "entries".
 *
 * ZIP64: if 50 4b 06 07 stands at p - 20, the ZIP64 end record it points to
 * supplies the 64-bit entry count, directory size and directory offset, and
 * LIBDEFLATE_AMD_ZIP_ZIP64 is set: signature 50 4b 06 06 at an offset q with
 * q + 56 <= p - 20, total disks at most 1 (zipfile's rule); the disk rule above
 * is then checked on the ZIP64 record's fields instead.  A locator whose
 * record fails this is LIBDEFLATE_BAD_DATA.
 *
 * CENTRAL DIRECTORY: it must end exactly where the (ZIP64) end record begins -
 * cd_off + cd_size == q with ZIP64, == p without - and cd_size must be below
 * 4 GiB.  An archive with data in front whose offsets need shifting (a
 * self-extractor) is therefore LIBDEFLATE_BAD_DATA.  The directory is the
 * chain of records 50 4b 01 02 of 46 + name_len + extra_len + comment_len
 * bytes that runs from cd_off, ends exactly at cd_off + cd_size and has
 * exactly the stated number of entries.  Every offset of the directory that
 * carries the signature with 46 bytes of directory behind it is a CANDIDATE -
 * names, extras and comments may carry it -; the chain decides which are
 * entries.
 *
 * PER ENTRY, from the central record: a 32-bit field equal to 0xFFFFFFFF is
 * replaced from the ZIP64 extra (the first extra record with id 0x0001) in the
 * order uncompressed size, compressed size, local header offset, and a disk
 * field of 0xFFFF from the 4 bytes behind them; a needed value that is
 * missing, or a disk other than 0, is LIBDEFLATE_BAD_DATA for that entry.
 * Then: a method other than 0 and 8, flag bit 0, 5, 6 or 13 (encryption,
 * patches, masked headers) or a size of 4 GiB or more is
 * LIBDEFLATE_AMD_ZIP_UNSUPPORTED for that entry alone.  Then the local header:
 * it must carry 50 4b 03 04 and lie wholly below cd_off, its own name and
 * extra lengths give data_off, and data_off + csize <= cd_off must hold, else
 * LIBDEFLATE_BAD_DATA.  Sizes and CRC-32 are the central directory's, so
 * entries written with data descriptors (flag bit 3) need nothing special.
 * Method 0 (stored) requires csize == usize (LIBDEFLATE_BAD_DATA); method 8 is
 * raw DEFLATE that must use exactly csize bytes and give exactly usize bytes.
 * Overlapping entries are allowed: the output is bounded by the sum of the
 * stated sizes against out_avail, whatever the file says.
 */
#define LIBDEFLATE_AMD_ZIP_MORE_ENTRIES     16	/* result[0]; same value as the BGZF / gzip readers' */
#define LIBDEFLATE_AMD_ZIP_MORE_CANDIDATES  17	/* result[0] */
#define LIBDEFLATE_AMD_ZIP_UNSUPPORTED      18	/* a per-entry result */
#define LIBDEFLATE_AMD_ZIP_RESULT_WORDS     5
#define LIBDEFLATE_AMD_ZIP_WORDS            8	/* u64 per index row */
#define LIBDEFLATE_AMD_ZIP_SLACK            1024	/* candidate room = max_entries + this */
#define LIBDEFLATE_AMD_ZIP_ZIP64            1	/* result[4] bit */

/*
 * The whole archive in DEVICE memory -> every entry's bytes in device memory.
 * Enqueues on `stream` and returns, with the conventions of
 * libdeflate_amd_gzip_members_decompress_batch: device pointers on the
 * object's device, scratch of the object, d_out must not overlap d_in, and no
 * byte is ever written at or past d_out + out_avail.  max_entries sizes the
 * launches and the scratch on the host, because the host never learns the
 * entry count: the decode batch has max_entries chunks and the finder has room
 * for max_entries + LIBDEFLATE_AMD_ZIP_SLACK candidates.
 *
 * d_result[0..4] (device memory):
 *   [0] the verdict, the first of these that applies:
 *       1. LIBDEFLATE_BAD_DATA: no end record, an inconsistent one, or a
 *          directory out of bounds; in_nbytes == 0 falls here;
 *       2. LIBDEFLATE_AMD_ZIP_MORE_ENTRIES: the stated count exceeds
 *          max_entries ([1] is the count);
 *       3. LIBDEFLATE_AMD_ZIP_MORE_CANDIDATES: the directory holds more
 *          candidates than max_entries + LIBDEFLATE_AMD_ZIP_SLACK ([1] is how
 *          many);
 *       4. LIBDEFLATE_BAD_DATA: a broken chain, or a chain of another length
 *          than the stated count;
 *       5. LIBDEFLATE_INSUFFICIENT_SPACE: the output needed exceeds out_avail;
 *       (1 to 5 are decided BEFORE the decode, and d_out is then not written;
 *       under 5 the index, d_results - pre-decode values - and [1] to [4] are
 *       written, so the caller can allocate and call again)
 *       6. the result of the first entry in directory order that did not
 *          succeed;
 *       7. LIBDEFLATE_SUCCESS.
 *   [1] entries (0 under verdicts 1 and 4), [2] cd_off, [3] bytes of output
 *   needed, alignment included, [4] flags (LIBDEFLATE_AMD_ZIP_ZIP64); under
 *   verdicts 1 to 4 words [2] to [4] are 0 and d_index and d_results are not
 *   written.
 *
 * d_index: NULL, or device room for max_entries rows of LIBDEFLATE_AMD_ZIP_WORDS
 * u64; row k of entry k in directory order:
 *   { offset of the central record (the name is at + 46), name_len,
 *     method | flags << 16, CRC-32, data_off, csize, usize, out_off }
 * data_off is 0 for an entry that is refused before its local header told it.
 * out_off is the exclusive prefix sum of the usizes, each rounded up to
 * out_align (a power of two in 1 .. 256); an entry refused before the decode
 * counts 0.  Entry k's bytes are at d_out + out_off.
 *
 * d_results[k] (int32, room for max_entries; written for the archive's
 * entries): 0, LIBDEFLATE_BAD_DATA (ZIP64 extra, disk, local header, bounds,
 * stored size mismatch, damaged DEFLATE, input not used up, CRC-32 mismatch),
 * the decoder's LIBDEFLATE_SHORT_OUTPUT / LIBDEFLATE_INSUFFICIENT_SPACE when
 * usize lies, LIBDEFLATE_AMD_ZIP_UNSUPPORTED.  A failed entry never affects
 * its neighbours; an entry whose CRC fails keeps its slot.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_out may be NULL
 * only with out_avail == 0, d_in only with in_nbytes == 0, d_index always),
 * max_entries == 0 or above 2^28, in_nbytes above 2^36, an out_align that is
 * not a power of two in 1 .. 256.
 *
 * Not covered: encrypted entries and methods other than 0 and 8 (archives are
 * written by libdeflate_amd_zip_compress_batch below); multi-disk archives;
 * archives with prepended data; entries of 4 GiB or more; a host-pointer form.
 * Here each entry is decoded by one wave, and a stored entry is copied by one
 * workgroup: for archives with a few huge entries, take the index from
 * libdeflate_amd_zip_index_batch and read through
 * libdeflate_amd_zip_read_large below.
 */
LIBDEFLATEAPI int
libdeflate_amd_zip_decompress_batch(struct libdeflate_decompressor *decompressor,
				    const void *d_in, size_t in_nbytes, size_t max_entries,
				    void *d_out, size_t out_avail, size_t out_align,
				    uint64_t *d_result, uint64_t *d_index, int32_t *d_results,
				    void *stream);

/* The index, the per-entry pre-decode results and the five words alone:
 * everything but the decode (out_avail counts as unlimited; damaged DEFLATE
 * and CRC failures cannot show).  The same out_off as the call above. */
LIBDEFLATEAPI int
libdeflate_amd_zip_index_batch(struct libdeflate_decompressor *decompressor,
			       const void *d_in, size_t in_nbytes, size_t max_entries,
			       size_t out_align, uint64_t *d_result, uint64_t *d_index,
			       int32_t *d_results, void *stream);

/*
 * Extract a selection.  index: HOST memory, `entries` rows as
 * libdeflate_amd_zip_index_batch returned them; sel: HOST memory, n_sel entry
 * numbers in any order, duplicates allowed.  Only those entries are decoded,
 * back to back in sel order with out_align, the CRC-32 checked against the
 * row; out_offsets: NULL, or HOST room for n_sel + 1 u64 - where selection r
 * starts, and where the last one ends - filled in before the call returns.
 * d_results[r] (device, int32) as above; a row with an unsupported method or
 * flag yields LIBDEFLATE_AMD_ZIP_UNSUPPORTED, a stored row whose sizes differ
 * LIBDEFLATE_BAD_DATA, and both take no room.  Enqueues on `stream`; the host
 * arrays may be reused when the call returns.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: a NULL argument, out_align
 * as above, a selected row that does not lie inside in_nbytes (central record
 * and name, data_off + csize), a size of 4 GiB or more, a sel at or above
 * entries, a selection that needs more than out_avail.
 */
LIBDEFLATEAPI int
libdeflate_amd_zip_read_batch(struct libdeflate_decompressor *decompressor,
			      const void *d_in, size_t in_nbytes,
			      const uint64_t *index, size_t entries,
			      size_t n_sel, const uint64_t *sel,
			      void *d_out, size_t out_avail, size_t out_align,
			      uint64_t *out_offsets, int32_t *d_results, void *stream);

/*
 * The same selection for archives with a few HUGE entries (an .npz of large
 * arrays, a checkpoint, a wheel with shared objects), which the call above
 * reads correctly but on one wave or one workgroup per entry.  The arguments,
 * the refusals before any device work, the layout (back to back in sel order,
 * rounded up to out_align), out_offsets and the values of d_results[r] are
 * those of libdeflate_amd_zip_read_batch; every output byte is the same.  Two
 * rules, each read from the index row alone, decide what differs:
 *
 * - a method-8 entry with csize >= large_min is decoded by
 *   libdeflate_amd_decompress_large (format LIBDEFLATE_AMD_DEFLATE, csize
 *   bytes at d_in + data_off, exactly usize bytes at d_out + out_off); its
 *   result is the entry's, and a success that did not use up csize bytes is
 *   LIBDEFLATE_BAD_DATA as above.  Which decoder answers inside that call is
 *   its own rule - a short stream goes to the one-wave decoder there -, so no
 *   result depends on large_min.  large_min == 0: the library's default
 *   (LDA_ZIP_LARGE_MIN);
 * - an entry of either method with usize > LIBDEFLATE_AMD_ZIP_PIECE is copied
 *   (if stored) and checksummed in pieces of that many bytes, each an ordinary
 *   chunk of the copy and of the CRC-32 batch, and its CRC-32 is combined from
 *   the pieces' on the device before it is compared with the row's.
 *
 * Every other entry goes through the call above's one batch.
 *
 * The call BLOCKS while its many-wave entries decode - it is not one of the
 * enqueue-only _batch calls, hence its name: the many-wave decoder's chain of
 * chunks is checked by the host.  They are decoded first, one after another;
 * before they first read d_in, the object's own streams wait (an event wait,
 * not a host wait) for what is queued on `stream`, so d_in may be the product
 * of kernels queued there, and when the call returns their bytes are complete.
 * Everything else - the batch, the pieces' copies and CRCs, the results - is
 * then enqueued on `stream`: d_results and the bytes of the other entries are
 * ready when `stream` is.  With no many-wave entry in the selection the call
 * only enqueues, like its sibling.  The host arrays may be reused when the
 * call returns.
 *
 * LIBDEFLATE_AMD_BAD_ARG and LIBDEFLATE_AMD_OOM as in the call above, with
 * the reason in libdeflate_amd_last_error(); a library-side failure inside a
 * many-wave decode (no memory for its scratch) is that entry's
 * LIBDEFLATE_BAD_DATA, as libdeflate_amd_decompress_large reports it.  Not
 * covered: entries of 4 GiB or more; an enqueue-only form; many-wave entries
 * decoded side by side.
 */
#define LIBDEFLATE_AMD_ZIP_PIECE (1u << 20)	/* bytes per copy / CRC piece */

LIBDEFLATEAPI int
libdeflate_amd_zip_read_large(struct libdeflate_decompressor *decompressor,
			      const void *d_in, size_t in_nbytes,
			      const uint64_t *index, size_t entries,
			      size_t n_sel, const uint64_t *sel,
			      void *d_out, size_t out_avail, size_t out_align,
			      size_t large_min,
			      uint64_t *out_offsets, int32_t *d_results, void *stream);

/*
 * Reading a tar archive (.tar, and with libdeflate_amd_decompress_large_index
 * in front a .tar.gz: source releases, container layers, sdists, WebDataset
 * shards) that lies in device memory.  The reference has nothing to do with
 * tar; the oracle is Python's tarfile, and tools/models/tar_walk.py restates
 * the rule on the CPU.  The rule is defined by a serial walk, and the device
 * result is exactly the walk's, whatever finds it.
 *
 * THE WALK: blocks are 512 bytes, nb = in_nbytes / 512 (a trailing partial
 * block is ignored), pos = 0 in blocks.
 *   1. nb == 0: LIBDEFLATE_BAD_DATA (tarfile's "empty file").
 *   2. pos == nb: the archive ends without an end marker; it is accepted and
 *      LIBDEFLATE_AMD_TAR_EOF is not set.
 *   3. The block at pos is all zero: the archive ends, LIBDEFLATE_AMD_TAR_EOF
 *      is set, and what lies behind is not examined (tarfile without
 *      ignore_zeros).  Block 0 being zero is an empty archive: SUCCESS with 0
 *      entries.
 *   4. Otherwise the block must be a HEADER.  An octal field skips leading
 *      spaces, reads octal digits, and must then be at the field's end or at a
 *      NUL or a space.  The checksum field (bytes 148..155, at least one digit)
 *      must equal the sum of the block's 512 bytes with those 8 counted as
 *      spaces, the bytes taken as unsigned or as signed chars (both accepted,
 *      as in tarfile).  The size field (124..135) is such an octal number, no
 *      digits meaning 0; with byte 124 == 0x80 it is the big-endian number in
 *      bytes 125..135, any other byte 124 with bit 7 set is invalid.  A size of
 *      2^36 or more is no header.  Data blocks d = ceil(size / 512), but d = 0
 *      for typeflags '1'..'6' (links, devices, directories, FIFOs) whatever the
 *      field says, which is tarfile's rule.  pos + 1 + d <= nb must hold.  No
 *      magic is required (V7 archives).  Anything else at a position the walk
 *      reaches is a broken chain: LIBDEFLATE_BAD_DATA.
 *   5. The record is 1 + d blocks; pos += 1 + d.
 * Every block that passes rule 4 is a CANDIDATE - a file's data may hold
 * headers, a tar inside a tar does -; the chain from block 0 decides which are
 * records.
 *
 * ENTRIES: records of typeflag L, K, x, X, g are EXTENSION RECORDS.  Every
 * other record is an ENTRY, and the extension records directly in front of it
 * belong to it; extension records behind the last entry are dropped.  An
 * entry's name is the first of these that applies: the value of the last
 * path= record of its x / X records (pax records are "%d %s=%s\n"; of several
 * x / X records the last one that has a path=); else the data of its (last) L
 * record up to the first NUL; else the header's name field up to the first
 * NUL, preceded, when the magic is "ustar\0" and the prefix field (345..499)
 * is not empty, by the prefix and a '/'.  K and g records and pax keys other
 * than path and size are walked over and ignored.
 *
 * An entry is LIBDEFLATE_AMD_TAR_UNSUPPORTED for itself alone when it has more
 * than 8 extension records in front of it, an L, x or X record of more than
 * 1 MiB, a pax record that does not parse, a pax size= key, or typeflag S, M
 * or D.  Such an entry is listed with its header's own name and usize 0 and
 * takes no room.  Unknown typeflags are regular files (POSIX, tarfile): only
 * typeflags '0', NUL, '7' and unknown ones have bytes to extract, the others
 * are listed with usize 0.
 */
#define LIBDEFLATE_AMD_TAR_MORE_RECORDS     16	/* result[0]; same value as the other readers' */
#define LIBDEFLATE_AMD_TAR_MORE_CANDIDATES  17	/* result[0] */
#define LIBDEFLATE_AMD_TAR_UNSUPPORTED      18	/* a per-entry result */
#define LIBDEFLATE_AMD_TAR_RESULT_WORDS     5
#define LIBDEFLATE_AMD_TAR_WORDS            8	/* u64 per index row */
#define LIBDEFLATE_AMD_TAR_SLACK            1024	/* candidate room = max_records + this */
#define LIBDEFLATE_AMD_TAR_EOF              1	/* result[4]: the walk ended at a zero block */
#define LIBDEFLATE_AMD_TAR_HAS_L            2	/* result[4]: an L record was seen */
#define LIBDEFLATE_AMD_TAR_HAS_PAX          4	/* result[4]: an x, X or g record was seen */

/*
 * The whole archive in DEVICE memory -> every entry's bytes in device memory.
 * Enqueues on `stream` and returns, with the conventions of
 * libdeflate_amd_zip_decompress_batch: device pointers on the object's device,
 * scratch of the object, d_out must not overlap d_in, and no byte is ever
 * written at or past d_out + out_avail, nor into an entry's alignment padding.
 * max_records bounds the chain's records of every kind - entries and extension
 * records - and sizes the launches and the scratch on the host, because the
 * host never learns the counts; the finder has room for max_records +
 * LIBDEFLATE_AMD_TAR_SLACK candidates (and never for more than nb).
 *
 * d_result[0..4] (device memory):
 *   [0] the verdict, the first of these that applies:
 *       1. LIBDEFLATE_BAD_DATA: nb == 0;
 *       2. LIBDEFLATE_AMD_TAR_MORE_CANDIDATES: more blocks pass the header rule
 *          than there is room for ([1] is how many);
 *       3. LIBDEFLATE_BAD_DATA: a broken chain;
 *       4. LIBDEFLATE_AMD_TAR_MORE_RECORDS: the chain has more than
 *          max_records records ([1] is how many);
 *       5. LIBDEFLATE_INSUFFICIENT_SPACE: the output needed exceeds out_avail;
 *       (1 to 5 are decided BEFORE any byte of d_out is written; under 5 the
 *       index, d_results and [1] to [4] are written, so the caller can
 *       allocate and call again)
 *       6. the result of the first entry that did not succeed;
 *       7. LIBDEFLATE_SUCCESS.
 *   [1] entries (0 under verdicts 1 and 3), [2] the byte offset where the walk
 *   ended - the zero block, or 512 nb -, [3] bytes of output needed, alignment
 *   included, [4] flags (LIBDEFLATE_AMD_TAR_EOF, _HAS_L, _HAS_PAX); under
 *   verdicts 1 to 4 words [2] to [4] are 0 and d_index and d_results are not
 *   written.
 *
 * d_index: NULL, or device room for max_records rows of
 * LIBDEFLATE_AMD_TAR_WORDS u64; row k of entry k in file order:
 *   { offset of the entry's own header, name_off, name_len | prefix_len << 32,
 *     typeflag | name source << 8, data_off, usize, mtime, out_off }
 * name_off is absolute in the file: the pax value (name source 2), the L data
 * (1) or the header (0).  prefix_len is non-zero only for a header name with a
 * ustar prefix, which stands at header + 345.  mtime is the header's field, 0
 * if it does not parse.  out_off is the exclusive prefix sum of the usizes,
 * each rounded up to out_align (a power of two in 1 .. 256).  Entry k's bytes
 * are at d_out + out_off.
 *
 * d_results[k] (int32, room for max_records; written for the archive's
 * entries): 0 or LIBDEFLATE_AMD_TAR_UNSUPPORTED.  A refused entry never
 * affects its neighbours.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_out may be NULL
 * only with out_avail == 0, d_in only with in_nbytes == 0, d_index always),
 * max_records == 0 or above 2^28, in_nbytes above 2^36, an out_align that is
 * not a power of two in 1 .. 256.
 *
 * Not covered: GNU sparse entries with extended header blocks, and pax size=
 * overrides that make the header's size field wrong (both usually break the
 * chain and end as LIBDEFLATE_BAD_DATA); ignore_zeros; link names and pax
 * attributes other than the path; files of 2^36 bytes and more; a host-pointer
 * form.
 */
LIBDEFLATEAPI int
libdeflate_amd_tar_extract_batch(struct libdeflate_decompressor *decompressor,
				 const void *d_in, size_t in_nbytes, size_t max_records,
				 void *d_out, size_t out_avail, size_t out_align,
				 uint64_t *d_result, uint64_t *d_index, int32_t *d_results,
				 void *stream);

/* The index, the per-entry results and the five words alone: everything but
 * the copy (out_avail counts as unlimited).  The same out_off as the call
 * above. */
LIBDEFLATEAPI int
libdeflate_amd_tar_index_batch(struct libdeflate_decompressor *decompressor,
			       const void *d_in, size_t in_nbytes, size_t max_records,
			       size_t out_align, uint64_t *d_result, uint64_t *d_index,
			       int32_t *d_results, void *stream);

/*
 * Extract a selection.  index: HOST memory, `entries` rows as
 * libdeflate_amd_tar_index_batch returned them; sel: HOST memory, n_sel entry
 * numbers in any order, duplicates allowed.  Only those entries are copied,
 * back to back in sel order with out_align; out_offsets: NULL, or HOST room for
 * n_sel + 1 u64 - where selection r starts, and where the last one ends -
 * filled in before the call returns.  d_results[r] (device, int32): 0, or
 * LIBDEFLATE_AMD_TAR_UNSUPPORTED for a row of typeflag S, M or D, which takes
 * no room.  Enqueues on `stream`; the host arrays may be reused when the call
 * returns.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: a NULL argument, out_align as
 * above, a selected row that does not lie inside in_nbytes (header, name,
 * data_off + usize; data_off must be header + 512), a size of 2^36 or more, a
 * sel at or above entries, a selection that needs more than out_avail.
 */
LIBDEFLATEAPI int
libdeflate_amd_tar_read_batch(struct libdeflate_decompressor *decompressor,
			      const void *d_in, size_t in_nbytes,
			      const uint64_t *index, size_t entries,
			      size_t n_sel, const uint64_t *sel,
			      void *d_out, size_t out_avail, size_t out_align,
			      uint64_t *out_offsets, int32_t *d_results, void *stream);

/*
 * The same checks and arithmetic without a device: ranges (HOST, 2 n_sel u64)
 * receives (data_off, usize) of every selection - (data_off, 0) for a row of
 * typeflag S, M or D - and *total_ret (may be NULL) the sum of the lengths.
 * That is what libdeflate_amd_seek_read_batch takes as `ranges` for the seek
 * index of the .gz the archive came out of, so a selection of a .tar.gz is
 * read from the compressed bytes.  The rows are checked against a file of
 * 2^36 bytes; libdeflate_amd_seek_read_batch checks the ranges against the
 * stream's own size.
 */
LIBDEFLATEAPI int
libdeflate_amd_tar_ranges(const uint64_t *index, size_t entries, size_t n_sel,
			  const uint64_t *sel, uint64_t *ranges, uint64_t *total_ret);

/*
 * ---- PNG images decoded on the device ----
 *
 * A batch of PNG files in device memory -> a batch of pixel arrays in device
 * memory: the chunks of every file walked and its header checked (the index
 * call), then for a selection the IDAT payloads gathered into the zlib stream
 * PNG splits across chunks, that stream decoded by the batch decoder above, and
 * the five scanline filters undone.  The oracle is the PNG specification as
 * tools/models/png_model.py restates it, pinned against PIL where PIL is there.
 * The conventions are those of the ZIP and tar readers: device pointers lie on
 * the object's device, scratch belongs to the decompressor object (it grows on
 * the host, as everywhere else, and the plan goes up through one pinned block
 * per object), and the calls only enqueue on `stream`.
 *
 * libdeflate_amd_png_index_batch: n_files files at d_in + d_in_offsets[k],
 * d_in_nbytes[k] bytes each (device arrays, as in
 * libdeflate_amd_decompress_batch).  d_results[k] (device, int32) and one row
 * of LIBDEFLATE_AMD_PNG_WORDS u64 per file in d_index (device):
 *   { file offset in d_in, file nbytes,
 *     width | height << 32,
 *     bit_depth | colour_type << 8 | interlace << 16 | filter unit (bytes per
 *       pixel, 1 below 8 bits) << 24 | channels << 32,
 *     offset in d_in of the first IDAT chunk's length field,
 *     sum of all IDAT data lengths,
 *     PLTE data offset | entries << 48   (0: none),
 *     tRNS data offset | length << 48    (0: none, or longer than 65535) }
 * Only a PLTE and a tRNS in front of the first IDAT are noted.  A failed file's
 * row is zero beyond words 0 and 1, and it never affects its neighbours.
 *
 * LIBDEFLATE_BAD_DATA: a wrong 8-byte signature; a first chunk that is not a
 * 13-byte IHDR, or an IHDR whose CRC-32 is wrong; width or height 0 or above
 * 2^31 - 1; a depth and colour type the specification does not pair;
 * compression or filter method other than 0, interlace other than 0 or 1; a
 * chunk whose 12 + length bytes do not lie inside the file; no IDAT; an IDAT
 * after the IDAT run has ended; a second IHDR or PLTE; colour type 3 without a
 * PLTE before IDAT; a PLTE length that is no multiple of 3 or above 768; no
 * IEND before the file ends.  LIBDEFLATE_AMD_PNG_UNSUPPORTED, where none of
 * those applies: interlace 1 (Adam7); an unknown critical chunk (an uppercase
 * first letter that is not IHDR, PLTE, IDAT or IEND); an image whose height *
 * (1 + rowbytes) is 2^32 or more.  Bytes behind IEND are ignored.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: a NULL argument, n_files above
 * 2^28.
 */
#define LIBDEFLATE_AMD_PNG_UNSUPPORTED      18	/* a per-file result; the ZIP and tar readers' value */
#define LIBDEFLATE_AMD_PNG_WORDS            8	/* u64 per index row */
#define LIBDEFLATE_AMD_PNG_LE16             1	/* flag: 16-bit samples little-endian */

LIBDEFLATEAPI int
libdeflate_amd_png_index_batch(struct libdeflate_decompressor *decompressor,
			       size_t n_files, const void *d_in,
			       const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
			       uint64_t *d_index, int32_t *d_results, void *stream);

/*
 * Host arithmetic only, the counterpart of libdeflate_amd_tar_ranges: index and
 * sel are HOST memory; out_offsets (HOST, n_sel + 1 u64) receives where
 * selection r starts in the output of libdeflate_amd_png_decode_batch and where
 * the last one ends, *total_ret (may be NULL) that end.  Every image takes
 * height * rowbytes bytes - rowbytes = ceil(width * channels * depth / 8) -
 * rounded up to out_align, a power of two in 1 .. 256; a zero row (a failed
 * file) takes none.  LIBDEFLATE_AMD_BAD_ARG: a NULL argument, out_align, a sel
 * at or above entries, a row whose words 2 and 3 are not a valid IHDR.
 */
LIBDEFLATEAPI int
libdeflate_amd_png_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
			     const uint64_t *sel, size_t out_align,
			     uint64_t *out_offsets, uint64_t *total_ret);

/*
 * Decode a selection.  index: HOST memory, `entries` rows as
 * libdeflate_amd_png_index_batch wrote them; sel: HOST memory, n_sel row
 * numbers in any order, duplicates allowed; out_offsets: NULL or HOST room for
 * n_sel + 1 u64, filled in before the call returns.  Selection r's pixels lie
 * at d_out + out_offsets[r]: height rows of exactly rowbytes bytes, no filter
 * bytes and no row padding, the samples as PNG stores them - depths below 8
 * stay packed most-significant-bit first, palette images stay indices, 16-bit
 * samples are big-endian.  flags: 0 or LIBDEFLATE_AMD_PNG_LE16, which stores
 * 16-bit samples little-endian, so that the buffer views as a native uint16
 * tensor (images of other depths are not changed by it).
 *
 * d_results[r] (device, int32) is the first of these that applies:
 * LIBDEFLATE_AMD_PNG_UNSUPPORTED for a zero row; LIBDEFLATE_BAD_DATA if the
 * IDAT chain found on the device disagrees with the row (a stale or foreign
 * index); the zlib decoder's own result - the stream must decode to exactly
 * height * (1 + rowbytes) bytes and its Adler-32 must hold, so BAD_DATA,
 * SHORT_OUTPUT and INSUFFICIENT_SPACE mean what they mean in
 * libdeflate_zlib_decompress; LIBDEFLATE_BAD_DATA for a filter-type byte above
 * 4; LIBDEFLATE_SUCCESS.  Nothing is written at or past d_out + out_avail, in
 * alignment padding or in another selection's room, whatever the file holds; a
 * failed selection's room is undefined, like a failed chunk's in the batch
 * decompress.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: a NULL argument (d_out may be
 * NULL only with out_avail == 0, d_in only with in_nbytes == 0), a bad
 * out_align or an unknown flag, in_nbytes above 2^36, a sel at or above
 * entries, a row whose file, first IDAT, IDAT sum or PLTE / tRNS range does not
 * lie inside in_nbytes or whose fields are not a valid IHDR, a selection that
 * needs more than out_avail.
 *
 * Not covered: Adam7 here - the _ex calls below read it, and this call keeps
 * its verdicts; the CRCs of IDAT, PLTE and ancillary chunks - only the
 * IHDR's is checked; the zlib stream's Adler-32 vouches for the pixel bytes,
 * and nothing vouches for a palette; gamma (palette expansion, tRNS, depth
 * scaling and channel conversion are libdeflate_amd_png_decode_pixels_batch,
 * below); APNG frames (the default
 * image alone is decoded); images of 2^32 raw bytes and more; routing a few
 * huge images to the many-wave decoder, as libdeflate_amd_zip_read_large does
 * for ZIP (every image is one wave's work here); a host-pointer form.
 */
LIBDEFLATEAPI int
libdeflate_amd_png_decode_batch(struct libdeflate_decompressor *decompressor,
				const void *d_in, size_t in_nbytes,
				const uint64_t *index, size_t entries,
				size_t n_sel, const uint64_t *sel,
				void *d_out, size_t out_avail, size_t out_align,
				unsigned flags, uint64_t *out_offsets,
				int32_t *d_results, void *stream);

/*
 * Decode a selection to ONE pixel format: what libdeflate_amd_png_decode_batch
 * does, and then every image expanded to the channels and sample depth of
 * `format`, whatever its file stores (png_set_expand, png_set_gray_to_rgb and
 * png_set_scale_16 of libpng; mode=RGB of torchvision.io.decode_png).
 * format: LIBDEFLATE_AMD_PNG_GRAY, _GRAY_ALPHA, _RGB or _RGBA (the channels),
 * alone for 8-bit samples or with LIBDEFLATE_AMD_PNG_OUT16 for 16-bit ones.
 * Selection r takes height * width * channels * (1 or 2) bytes at d_out +
 * out_offsets[r], rounded up to out_align: interleaved pixels, no row padding;
 * a zero row takes none.  16-bit samples are big-endian, little-endian with
 * LIBDEFLATE_AMD_PNG_LE16 in flags.  Per pixel, in this order:
 *  1. the samples at the file's depth; depths 1, 2, 4 unpacked
 *     most-significant-bit first, the spare low bits of a row's last byte
 *     ignored;
 *  2. colour type 3: index i becomes R, G, B of PLTE entry i with alpha tRNS[i]
 *     for i < min(tRNS length, entries) and 255 otherwise, 8-bit RGBA; an index
 *     at or above `entries` makes the selection LIBDEFLATE_BAD_DATA;
 *  3. the colour key: colour type 0 with a tRNS of exactly 2 bytes - alpha 0
 *     where the sample equals the key's low `depth` bits; colour type 2 with a
 *     tRNS of exactly 6 bytes - alpha 0 where all three samples equal the key
 *     (16-bit big-endian words, their low byte at depth 8); opaque otherwise.
 *     A tRNS of another length, or of colour types 4 and 6, is ignored;
 *  4. the depth, every channel alike: 1, 2, 4 -> 8 by bit replication (v *
 *     0xFF, 0x55, 0x11); 8 -> 16 is v * 257; 16 -> 8 is (v * 255 + 32895) >> 16,
 *     round to nearest (libpng's png_set_scale_16);
 *  5. the channels: grey -> RGB by replication; RGB -> grey is (19595 R +
 *     38470 G + 7471 B + 32768) >> 16; alpha is dropped without compositing
 *     where the format has none, and is the file's, the palette's, the key's
 *     or opaque where it has one.
 * An image that already is the format is unfiltered straight into its room; the
 * others go through scratch of the decompressor object and one more kernel.
 *
 * libdeflate_amd_png_pixels_out_sizes is the host arithmetic of the rooms, as
 * libdeflate_amd_png_out_sizes.  Sizes are u64: a 1-bit image below 2^32 raw
 * bytes converts to far more than 2^32.
 *
 * d_results[r]: the first verdict of libdeflate_amd_png_decode_batch that
 * applies, then LIBDEFLATE_BAD_DATA for a palette index out of range, then
 * LIBDEFLATE_SUCCESS.  Nothing is written outside the selections' rooms; a
 * failed selection's room is undefined.  Only enqueues; nothing is read back.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: everything
 * libdeflate_amd_png_decode_batch refuses (an interlaced row among it), a
 * format whose low four bits are not 1 .. 4 or with other bits than OUT16, a
 * selection that needs more than out_avail.
 *
 * Not covered: gamma and sBIT, compositing against bKGD, APNG, a host-pointer
 * form; Adam7 here - the _ex calls below read it, and this call keeps its
 * verdicts.
 */
#define LIBDEFLATE_AMD_PNG_GRAY        1	/* format = channels ... */
#define LIBDEFLATE_AMD_PNG_GRAY_ALPHA  2
#define LIBDEFLATE_AMD_PNG_RGB         3
#define LIBDEFLATE_AMD_PNG_RGBA        4
#define LIBDEFLATE_AMD_PNG_OUT16       0x10	/* ... | this: 16-bit samples, else 8-bit */

LIBDEFLATEAPI int
libdeflate_amd_png_pixels_out_sizes(const uint64_t *index, size_t entries, size_t n_sel,
				    const uint64_t *sel, unsigned format, size_t out_align,
				    uint64_t *out_offsets, uint64_t *total_ret);

LIBDEFLATEAPI int
libdeflate_amd_png_decode_pixels_batch(struct libdeflate_decompressor *decompressor,
				       const void *d_in, size_t in_nbytes,
				       const uint64_t *index, size_t entries,
				       size_t n_sel, const uint64_t *sel, unsigned format,
				       void *d_out, size_t out_avail, size_t out_align,
				       unsigned flags, uint64_t *out_offsets,
				       int32_t *d_results, void *stream);

/*
 * Adam7-interlaced files: the three calls above with a flag that lets
 * interlace 1 through.  They are new entry points, and the calls above keep
 * their verdicts: without LIBDEFLATE_AMD_PNG_ADAM7 every result, row, offset
 * and byte of these calls is that of the older call.
 *
 * libdeflate_amd_png_index_batch_ex: flags 0 gives exactly the rows and
 * verdicts of libdeflate_amd_png_index_batch.  With LIBDEFLATE_AMD_PNG_ADAM7 an
 * interlace-1 file that passes every other rule is LIBDEFLATE_SUCCESS with a
 * full row, bit 16 of whose word 3 is set; it is
 * LIBDEFLATE_AMD_PNG_UNSUPPORTED where height * (1 + rowbytes) or raw7 is 2^32
 * or more - raw7 the bytes its zlib stream inflates to: for each of the seven
 * passes (PNG 8.2) of w_p x h_p pixels, none of them 0, h_p * (1 + ceil(w_p *
 * channels * depth / 8)).  LIBDEFLATE_BAD_DATA still comes first.  Any other
 * flag bit is LIBDEFLATE_AMD_BAD_ARG.
 *
 * libdeflate_amd_png_out_sizes_ex: host arithmetic only.  format 0 gives the
 * rooms of libdeflate_amd_png_out_sizes, any other value (a format of
 * libdeflate_amd_png_decode_pixels_batch) those of
 * libdeflate_amd_png_pixels_out_sizes.  flags: 0 or LIBDEFLATE_AMD_PNG_ADAM7;
 * an interlaced row is refused without it ("interlaced") and takes the room of
 * its non-interlaced twin with it.
 *
 * libdeflate_amd_png_decode_batch_ex: flags are LIBDEFLATE_AMD_PNG_LE16 |
 * LIBDEFLATE_AMD_PNG_ADAM7.  format 0 gives the layout and the verdict order
 * of libdeflate_amd_png_decode_batch, any other value those of
 * libdeflate_amd_png_decode_pixels_batch.  Interlaced and plain rows, zero rows
 * and duplicates mix freely in one selection; an interlaced image's bytes are
 * those of its non-interlaced twin.  An interlaced selection's d_results[r] is
 * the first of: LIBDEFLATE_AMD_PNG_UNSUPPORTED for a zero row; the gather's
 * LIBDEFLATE_BAD_DATA; the zlib decoder's own result against the exact fill of
 * raw7 bytes; LIBDEFLATE_BAD_DATA for a filter-type byte above 4 in any pass;
 * with a pixel format, LIBDEFLATE_BAD_DATA for a palette index out of range;
 * LIBDEFLATE_SUCCESS.  Nothing is written outside the selections' rooms,
 * whatever the file holds.  LIBDEFLATE_AMD_BAD_ARG before any device work:
 * what the older calls refuse, an interlaced row without the flag among it.
 * Only enqueues; scratch belongs to the decompressor object.  A selection
 * without an interlaced row queues what the older call queues.
 */
#define LIBDEFLATE_AMD_PNG_ADAM7            2	/* flag: interlace 1 is read */

LIBDEFLATEAPI int
libdeflate_amd_png_index_batch_ex(struct libdeflate_decompressor *decompressor,
				  size_t n_files, const void *d_in,
				  const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
				  unsigned flags, uint64_t *d_index, int32_t *d_results,
				  void *stream);

LIBDEFLATEAPI int
libdeflate_amd_png_out_sizes_ex(const uint64_t *index, size_t entries, size_t n_sel,
				const uint64_t *sel, unsigned format, size_t out_align,
				unsigned flags, uint64_t *out_offsets, uint64_t *total_ret);

LIBDEFLATEAPI int
libdeflate_amd_png_decode_batch_ex(struct libdeflate_decompressor *decompressor,
				   const void *d_in, size_t in_nbytes,
				   const uint64_t *index, size_t entries,
				   size_t n_sel, const uint64_t *sel, unsigned format,
				   void *d_out, size_t out_avail, size_t out_align,
				   unsigned flags, uint64_t *out_offsets,
				   int32_t *d_results, void *stream);

/*
 * ---- ZIP archives written on the device ----
 *
 * n_entries named byte ranges of one DEVICE buffer -> one ZIP archive in device
 * memory: every entry compressed (method 8) or stored (method 0), local
 * headers, central directory and end records placed by kernels.  Enqueues on
 * `stream` and returns: nothing comes back to the host and the device is not
 * waited for, with two exceptions: scratch of the object grows on the host, as
 * everywhere else, and the plan goes up through one pinned block per object,
 * so a call waits until the previous call on the same object has had its plan
 * uploaded (its stream has reached that copy, not its kernels).
 *
 * names / name_offsets (n_entries + 1, ascending), in_offsets and in_nbytes
 * are HOST arrays - a ZIP writer's caller knows them - and may be reused when
 * the call returns.  Entry k is bytes [in_offsets[k], + in_nbytes[k]) of d_in
 * and is called names[name_offsets[k] .. name_offsets[k + 1]).  Entries may
 * overlap one another; d_out must not overlap d_in.
 *
 * An entry gets method 8 when its raw DEFLATE stream - byte for byte what
 * libdeflate_deflate_compress() of this build returns for the entry's bytes at
 * the object's level and LDA_* switches - is shorter than the entry; otherwise
 * method 0 with the entry's own bytes.  Empty entries, a level-0 object and
 * LIBDEFLATE_AMD_ZIP_STORE always store, and under the last two no compress
 * kernel runs.
 *
 * The archive: per entry a local header (30 bytes, version needed 20 - 45 in
 * ZIP64 mode -, general-purpose bit 11 iff the name holds a byte >= 0x80 and
 * no other flag, time / date the low / high half of dos_datetime - 0 stands
 * for 0x00210000, 1980-01-01 00:00 -, the real CRC-32 and sizes, no extra
 * field, no data descriptor), the name and the data, back to back from offset
 * 0 in the caller's order; then the central directory (version made by 20 /
 * 45, attributes 0, no comment; in ZIP64 mode the offset field is 0xFFFFFFFF
 * and the extra field 01 00 08 00 + the u64 offset); then the 22-byte end
 * record without a comment - in ZIP64 mode the 56-byte ZIP64 end record, its
 * 20-byte locator and an end record whose counts, size and offset are
 * 0xFFFF / 0xFFFFFFFF.  ZIP64 mode is decided on the host:
 * LIBDEFLATE_AMD_ZIP_FORCE_ZIP64, n_entries >= 65535, or a plain bound of
 * 0xFFFFFFFF or more.
 *
 * libdeflate_amd_zip_compress_bound() is exact arithmetic on the host arrays:
 *   Sum(30 + name + in_nbytes) + Sum(46 + name + 12 z64) + 22 + 76 z64
 * No archive of these entries is larger, because csize <= usize.
 *
 * d_result[0 .. LIBDEFLATE_AMD_ZIPW_RESULT_WORDS) (device memory):
 *   [0] 0, or LIBDEFLATE_INSUFFICIENT_SPACE: the archive does not fit
 *       out_avail - then no byte of d_out and no row of d_index is written;
 *   [1] the archive's size, [2] cd_off, [3] the entries that got method 8
 *   ([1] to [3] are valid either way).
 * d_index: NULL, or device room for n_entries rows of LIBDEFLATE_AMD_ZIP_WORDS
 * u64: exactly the rows libdeflate_amd_zip_index_batch returns for the written
 * archive with out_align 1, so the archive can go straight into
 * libdeflate_amd_zip_read_batch.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_in may be NULL with
 * in_avail == 0, the host arrays with n_entries == 0, d_index always), unknown
 * flags, n_entries above 2^28, a name of 0 or more than 65535 bytes or
 * decreasing name_offsets, an entry of 4 GiB or more, an entry that does not
 * lie inside in_avail, out_avail below the size of the directory and end
 * records alone.  n_entries == 0 writes the 22-byte empty archive.
 *
 * Limits: the object's scratch is about the sum of the entries' sizes plus
 * descriptors; with LDA_NO_SEGMENTS a huge entry is one piece and one
 * workgroup; no host-pointer form; no per-entry method, time or alignment
 * padding; no archive comment; no encryption.
 */
#define LIBDEFLATE_AMD_ZIP_STORE         1	/* flag: every entry method 0, nothing compressed */
#define LIBDEFLATE_AMD_ZIP_FORCE_ZIP64   2	/* flag: ZIP64 records whatever the sizes */
#define LIBDEFLATE_AMD_ZIPW_RESULT_WORDS 4

LIBDEFLATEAPI size_t
libdeflate_amd_zip_compress_bound(size_t n_entries, const uint64_t *name_offsets,
				  const uint64_t *in_nbytes, unsigned flags);

LIBDEFLATEAPI int
libdeflate_amd_zip_compress_batch(struct libdeflate_compressor *compressor,
				  size_t n_entries, const void *names,
				  const uint64_t *name_offsets, const void *d_in, size_t in_avail,
				  const uint64_t *in_offsets, const uint64_t *in_nbytes,
				  void *d_out, size_t out_avail, uint64_t *d_result,
				  uint64_t *d_index, uint32_t dos_datetime, unsigned flags,
				  void *stream);

/*
 * ---- Files of concatenated gzip members written on the device ----
 *
 * n_records byte ranges of one DEVICE buffer -> one file of n_records ordinary
 * gzip members back to back (a WARC archive, `cat a.gz b.gz`, an mgzip / pgzip
 * shard): what libdeflate_amd_gzip_members_decompress_batch reads.  The
 * conventions are those of libdeflate_amd_zip_compress_batch above: the call
 * enqueues on `stream` and returns, the plan goes up through the object's
 * pinned block, scratch belongs to the object (the ZIP writer's), names /
 * name_offsets (n_records + 1, ascending), in_offsets and in_nbytes are HOST
 * arrays that may be reused when the call returns, records may overlap one
 * another, d_out must not overlap d_in, and no byte is ever written at or past
 * d_out + out_avail.
 *
 * Unlike libdeflate_amd_compress_batch in gzip format, a record is not one
 * workgroup whatever its size: records of 128 KiB and more are cut into primed
 * segments that fill the GPU (large_plan.h), exactly as the single-buffer call
 * cuts them, and records of at most 4 KiB go to the small-buffer kernel.
 *
 * names and name_offsets may both be NULL: no member has a name.  A record
 * whose name range is empty has none either.
 *
 * THE FILE: record k's member stands behind record k - 1's, from offset 0.  An
 * unnamed member written with mtime == 0 is byte for byte what
 * libdeflate_gzip_compress() of this build returns for the record's bytes at
 * the object's level and LDA_* switches - the record of 0 bytes, the records
 * under the level's pass-through size, level 0 and the segmented records
 * included.  A named member differs in three places: FLG has FNAME set, the
 * name and a 0 byte follow the 10 fixed header bytes, and mtime sits in bytes
 * 4..7 (as it does in an unnamed member when it is not 0).  DEFLATE stream,
 * CRC-32 and ISIZE are the same.  No FEXTRA, FCOMMENT or FHCRC.
 *
 * libdeflate_amd_gzip_members_compress_bound() is arithmetic on the host
 * arrays (name_offsets may be NULL): the sum of
 * libdeflate_gzip_compress_bound(in_nbytes[k]), plus the name's length and 1
 * for every named record.  No file of these records is larger.
 *
 * d_result[0 .. LIBDEFLATE_AMD_GZMW_RESULT_WORDS) (device memory):
 *   [0] 0, or LIBDEFLATE_INSUFFICIENT_SPACE: the file does not fit out_avail -
 *       then no byte of d_out and no row of d_index is written;
 *   [1] the file's size, [2] the records' bytes in all, [3] the members
 *   ([1] to [3] are valid either way).
 * d_index: NULL, or device room for 2 (n_records + 1) u64: exactly what
 * libdeflate_amd_gzip_members_index_batch returns for the written file - the
 * pairs (compressed offset, uncompressed offset) of every member, then the
 * closing pair - so the file and its index can go straight to
 * libdeflate_amd_decompress_batch_packed over chosen members.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_in may be NULL with
 * in_avail == 0, the host arrays with n_records == 0, names and name_offsets
 * together, d_index always), unknown flags (none is defined yet), n_records
 * above 2^28, decreasing name_offsets, a name that holds a 0 byte or has more
 * than 65 534 bytes (with its terminator the reader's
 * LIBDEFLATE_AMD_GZM_NAME_MAX), a record of 4 GiB or more, a record that does
 * not lie inside in_avail - and, with a level-0 object, a record above
 * 0xFFFFFF00 bytes, for which libdeflate_gzip_compress() itself returns 0.
 * n_records == 0 writes nothing and reports a file of size 0.
 *
 * Limits: the object's scratch is about the sum of the records' bounds plus
 * descriptors; a level-0 record, and with LDA_NO_SEGMENTS any record, is one
 * piece and one workgroup; one level and one mtime per call; no FEXTRA /
 * FCOMMENT / FHCRC; no host-pointer form; no preset dictionary.
 */
#define LIBDEFLATE_AMD_GZMW_RESULT_WORDS 4

LIBDEFLATEAPI size_t
libdeflate_amd_gzip_members_compress_bound(struct libdeflate_compressor *compressor,
					   size_t n_records, const uint64_t *name_offsets,
					   const uint64_t *in_nbytes);

LIBDEFLATEAPI int
libdeflate_amd_gzip_members_compress_batch(struct libdeflate_compressor *compressor,
					   size_t n_records, const void *names,
					   const uint64_t *name_offsets, const void *d_in,
					   size_t in_avail, const uint64_t *in_offsets,
					   const uint64_t *in_nbytes, void *d_out, size_t out_avail,
					   uint64_t *d_result, uint64_t *d_index, uint32_t mtime,
					   unsigned flags, void *stream);

/*
 * ---- tar archives written on the device ----
 *
 * n_entries named byte ranges of one DEVICE buffer -> one tar archive in device
 * memory (a WebDataset shard, a checkpoint bundle), or that archive compressed
 * into one gzip / zlib / DEFLATE stream (.tar.gz): what
 * libdeflate_amd_tar_extract_batch reads.  The conventions are those of
 * libdeflate_amd_zip_compress_batch above: the calls enqueue on `stream` and
 * return, the plan goes up through the object's pinned block, scratch belongs
 * to the object (the ZIP writer's), names / name_offsets (n_entries + 1,
 * ascending), in_offsets and in_nbytes are HOST arrays that may be reused when
 * the call returns, entry k is bytes [in_offsets[k], + in_nbytes[k]) of d_in,
 * entries may overlap one another, d_out must not overlap d_in and may have
 * any alignment.
 *
 * A tar archive's layout follows from the names and sizes alone, so the host
 * knows every offset and the exact size before anything runs: nothing comes
 * back from the device, there is no verdict word, and one kernel writes every
 * byte of the archive exactly once - headers, data and all padding, d_out need
 * not be clear.
 *
 * THE ARCHIVE, in blocks of 512 bytes:
 *   Per entry one header block, the entry's bytes, and zeros up to the next
 *   block boundary.  The header: name at 0 (100 bytes, NUL-padded, not
 *   terminated when it fills the field); mode "0000644\0" at 100; uid and gid
 *   "0000000\0" at 108 and 116; the size at 124 and mtime at 136, each 11
 *   octal digits and a NUL; the checksum at 148, six octal digits, a NUL and a
 *   space - the sum of the block's 512 bytes with these eight counted as
 *   spaces -; typeflag '0' at 156; linkname (100 bytes at 157) NUL; the magic
 *   "ustar\0" and version "00" at 257; uname, gname, devmajor, devminor and
 *   prefix, the rest of the block, NUL.  The ustar prefix split is never used.
 *
 *   A name of more than 100 characters (names are UTF-8), or with a byte >=
 *   0x80, has a pax extension record in front of the entry's header: a header
 *   block as above with the name "././@PaxHeader", mode "0000000\0", mtime 0,
 *   typeflag 'x' and the length of the pax data as its size; then the pax
 *   data, the one record "%d path=%s\n" - the decimal is the record's own
 *   length, itself included - zero-padded to a block boundary.  The entry's own
 *   header then carries the first 100 characters of the name with every
 *   character that is not ASCII replaced by one '?'.
 *
 *   Behind the last entry two zero blocks, then zeros up to a multiple of
 *   10 240 bytes.  n_entries == 0 writes 10 240 zero bytes.
 * Byte for byte this is what Python's tarfile writes in its default (pax)
 * format for regular files with size and an integer mtime set and every other
 * attribute at its default.
 *
 * libdeflate_amd_tar_write_size() is that archive's exact size, arithmetic on
 * the host arrays without a device (0, with the reason in
 * libdeflate_amd_last_error(), for a NULL array and for every count, name,
 * entry size and archive size that the calls below refuse: one check serves
 * all three).  libdeflate_amd_tar_write_batch writes
 * every byte of d_out[0 .. size) and no byte at or past d_out + size.
 *
 * index: NULL, or HOST room for n_entries rows of LIBDEFLATE_AMD_TAR_WORDS u64,
 * filled in before the call returns: exactly the rows
 * libdeflate_amd_tar_index_batch returns for the written archive with
 * out_align 1 - name source 0 (the header) or 2 (the pax value), name_off
 * absolute in the archive, out_off the exclusive prefix sum of the sizes - so
 * they go straight into libdeflate_amd_tar_read_batch and
 * libdeflate_amd_tar_ranges, which take host rows.
 *
 * libdeflate_amd_targz_compress_batch writes the archive into the object's
 * scratch and enqueues libdeflate_amd_compress_large_batch on it: d_out and
 * d_out_nbytes[0] (device memory) get exactly what that call gives for the
 * archive's bytes at the object's level - d_out_nbytes[0] = 0 and no byte
 * written when the stream does not fit out_avail.  format is
 * LIBDEFLATE_AMD_GZIP, _ZLIB or _DEFLATE;
 * libdeflate_gzip_compress_bound(libdeflate_amd_tar_write_size(...)) is room
 * enough.  The index rows are the archive's: with the seek index of
 * libdeflate_amd_decompress_large_index and libdeflate_amd_tar_ranges a
 * selection is read from the compressed bytes.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_in may be NULL with
 * in_avail == 0, the host arrays with n_entries == 0, index always), unknown
 * flags (none is defined yet), n_entries above 2^28, decreasing name_offsets, a
 * name that is empty, longer than 65 535 bytes, holds a 0 byte or is not valid
 * UTF-8, an entry of 8^11 bytes (8 GiB) or more - it would need a pax size=
 * record, which the reader refuses -, mtime of 8^11 or more, an entry that
 * does not lie inside in_avail, out_avail below the archive's size, an archive
 * above 2^40 - 65 536 bytes (1 TiB: what one launch of the kernel can hold);
 * for the .tar.gz call what
 * libdeflate_amd_compress_large_batch refuses of format and out_avail instead
 * of the room for the archive.
 *
 * Limits: regular files only, one mtime and mode 0644 per call; no
 * directories, links or devices; no uid / gid / uname / gname; no GNU or
 * ustar-prefix format; no appending to an archive; no host-pointer form.  The
 * .tar.gz call's scratch holds the whole archive.
 */
LIBDEFLATEAPI size_t
libdeflate_amd_tar_write_size(size_t n_entries, const uint64_t *name_offsets,
			      const void *names, const uint64_t *in_nbytes);

LIBDEFLATEAPI int
libdeflate_amd_tar_write_batch(struct libdeflate_compressor *compressor,
			       size_t n_entries, const void *names,
			       const uint64_t *name_offsets, const void *d_in, size_t in_avail,
			       const uint64_t *in_offsets, const uint64_t *in_nbytes,
			       void *d_out, size_t out_avail, uint64_t *index,
			       uint64_t mtime, unsigned flags, void *stream);

LIBDEFLATEAPI int
libdeflate_amd_targz_compress_batch(struct libdeflate_compressor *compressor, int format,
				    size_t n_entries, const void *names,
				    const uint64_t *name_offsets, const void *d_in,
				    size_t in_avail, const uint64_t *in_offsets,
				    const uint64_t *in_nbytes, void *d_out, size_t out_avail,
				    uint64_t *d_out_nbytes, uint64_t *index, uint64_t mtime,
				    unsigned flags, void *stream);

/*
 * ---- PNG images written on the device ----
 *
 * n_images pixel arrays of one DEVICE buffer -> n_images PNG files back to
 * back in device memory: the scanlines filtered by a kernel, compressed into
 * one zlib stream per image, and signature, IHDR, PLTE, tRNS, ONE IDAT and
 * IEND placed around it with their CRC-32s: what
 * libdeflate_amd_png_decode_batch reads.  The conventions are those of
 * libdeflate_amd_gzip_members_compress_batch above: the object is a
 * compressor and the level is the object's, the call enqueues on `stream` and
 * returns, the plan goes up through the object's pinned block, scratch belongs
 * to the object (the ZIP writer's), `images` is a HOST array that may be
 * reused when the call returns, d_out must not overlap d_in, and no byte is
 * ever written at or past d_out + out_avail.
 *
 * images: LIBDEFLATE_AMD_PNG_WORDS u64 per image, the reader's index row read
 * the other way - a decoded row with words 0 and 1 replaced is a valid input:
 *   { offset of the pixels in d_in, their size (height * rowbytes),
 *     width | height << 32,
 *     bit_depth | colour_type << 8 (bits 16..23, interlace, must be 0; bits 24
 *       and up are ignored),
 *     ignored, ignored,
 *     PLTE data offset in d_in | entries << 48 (0: none; required for colour
 *       type 3, allowed for 2 and 6, refused for 0 and 4; 1 .. 256 entries, for
 *       type 3 at most 1 << depth),
 *     tRNS data offset in d_in | length << 48 (0: none; the length 2 for type
 *       0, 6 for type 2, 1 .. PLTE entries for type 3; refused for 4 and 6) }
 * The pixels are what the reader writes: height rows of exactly rowbytes bytes,
 * depths below 8 packed most-significant-bit first, 16-bit samples big-endian -
 * or, with LIBDEFLATE_AMD_PNG_LE16 in flags, little-endian (a native uint16
 * tensor): they are swapped as they are loaded, so the filters see PNG's order.
 *
 * THE FILES: image k's file stands behind image k - 1's, from offset 0.  The
 * IDAT payload is byte for byte what libdeflate_zlib_compress() of this build
 * returns for the image's filtered scanlines at the object's level and LDA_*
 * switches; every chunk's CRC-32 is right.  Scanline y is a filter-type byte
 * and rowbytes filtered bytes (PNG specification 9.2; the row above row 0 is
 * zeros, the filter unit is max(1, channels * depth / 8) bytes, Average takes
 * the 9-bit sum, Paeth resolves ties a, b, c).  filter 0 .. 4: that type on
 * every row.  LIBDEFLATE_AMD_PNG_FILTER_ADAPTIVE: per row the type whose
 * filtered bytes, read as signed, have the least sum of absolute values, the
 * lowest type on a tie (libpng's heuristic).
 *
 * libdeflate_amd_png_encode_bound() is arithmetic on the host rows: per image
 * 8 + 25 + (12 + 3 entries, with a PLTE) + (12 + length, with a tRNS) + 12 +
 * libdeflate_zlib_compress_bound(height * (1 + rowbytes)) + 12.  No files of
 * these images are larger.  0 for rows the batch call refuses (what needs
 * in_avail apart).
 *
 * d_result[0 .. LIBDEFLATE_AMD_PNGW_RESULT_WORDS) (device memory):
 *   [0] 0, or LIBDEFLATE_INSUFFICIENT_SPACE: the files do not fit out_avail -
 *       then no byte of d_out and no row of d_index is written;
 *   [1] the files' bytes in all, [2] the pixels' bytes in all, [3] the images
 *   ([1] to [3] are valid either way).
 * d_index: NULL, or device room for n_images rows of LIBDEFLATE_AMD_PNG_WORDS
 * u64: exactly the rows libdeflate_amd_png_index_batch returns for the written
 * files, word 0 the file's offset in d_out, so d_out and the rows can go
 * straight to libdeflate_amd_png_decode_batch.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the reason in
 * libdeflate_amd_last_error(): a NULL object or pointer (d_in may be NULL with
 * in_avail == 0, images with n_images == 0, d_index always), a filter above 5,
 * an unknown flag, n_images above 2^28, words 2 and 3 that are no valid
 * non-interlaced IHDR (the reader's rule), word 1 not height * rowbytes,
 * height * (1 + rowbytes) of 2^32 or more, a zlib bound above 2^31 - 1 (one
 * IDAT's length field; it also excludes every image for which a level-0
 * libdeflate_zlib_compress() returns 0), pixels, PLTE or tRNS that do not lie
 * inside in_avail, a PLTE or tRNS rule above broken.  n_images == 0 writes
 * d_result alone.
 *
 * Limits: the object's scratch is about twice the pixels' bytes (the scanlines
 * and the slots) plus descriptors; one filter mode and one level per call; no
 * Adam7; one IDAT per image; no ancillary chunk but tRNS; no filter choice by
 * trial compression; no host-pointer form.
 */
#define LIBDEFLATE_AMD_PNG_FILTER_ADAPTIVE 5	/* filter: 0..4 = that type on every row */
#define LIBDEFLATE_AMD_PNGW_RESULT_WORDS   4

LIBDEFLATEAPI size_t
libdeflate_amd_png_encode_bound(struct libdeflate_compressor *compressor,
				size_t n_images, const uint64_t *images);

LIBDEFLATEAPI int
libdeflate_amd_png_encode_batch(struct libdeflate_compressor *compressor,
				size_t n_images, const uint64_t *images,
				const void *d_in, size_t in_avail,
				void *d_out, size_t out_avail,
				uint64_t *d_result, uint64_t *d_index,
				unsigned filter, unsigned flags, void *stream);

/*
 * Prefix decompress: the first bytes of every stream of a batch - zlib's
 * inflate() with avail_out below the stream's size, Python's
 * decompressobj().decompress(data, max_length) - which the whole-buffer calls
 * above answer with LIBDEFLATE_INSUFFICIENT_SPACE and an undefined buffer.
 *
 * d_limits[i] is stream i's limit; d_out + d_out_offsets[i] has room for that
 * many bytes.  d_results[i] is what
 *   libdeflate_<format>_decompress_ex(in_i, out_avail = d_limits[i],
 *                                     &actual_in, &actual_out)
 * returns, with one substitution: where that call returns
 * LIBDEFLATE_INSUFFICIENT_SPACE the result here is LIBDEFLATE_AMD_PREFIX
 * (subject to the one exception below), and then
 *   - d_out[d_out_offsets[i] .. + d_limits[i]) holds the first d_limits[i]
 *     bytes of what the stream decodes to;
 *   - d_actual_out[i] = d_limits[i] and d_actual_in[i] = 0;
 *   - the footer is not looked at (a wrong checksum cannot show).
 * The one exception is the match that the limit cuts: the reference stops
 * before it reads that match's offset, this call needs the offset and decodes
 * it by the rules of a match that fits.  An offset that reaches before the
 * stream (or its dictionary), and one whose bits do not lie inside the input,
 * make the stream LIBDEFLATE_BAD_DATA with d_actual_out[i] = 0.  Nothing else
 * about an offset is bad: an offset code without codewords, or with one, is
 * read as the reference reads it for a match that fits (an empty code stands
 * for symbol 0, distance 1 - bad at the stream's first byte only).  (A stored
 * block that the limit cuts is checked against the input in the same spirit:
 * a LEN that runs past the input is LIBDEFLATE_BAD_DATA, not a prefix.)
 *
 * LIBDEFLATE_SUCCESS means that the stream ended within its limit and was
 * checked in full, checksum and ISIZE included; d_actual_in[i] and
 * d_actual_out[i] are then the reference's.  d_limits[i] == 0 is legal.  A
 * stream that fails or is cut never affects its neighbours, and no byte is
 * written at or past a stream's limit.  Under every other result the bytes
 * below the limit are undefined and the two figures mean nothing (0 and 0
 * where the decoder itself refused the stream; what the raw decoder counted
 * where only the footer did not match, as with
 * libdeflate_amd_decompress_batch).
 *
 * The calls only enqueue on `stream`; object, scratch and stream follow
 * libdeflate_amd_decompress_batch, and so does LIBDEFLATE_AMD_BAD_ARG, which
 * comes before any device work: a NULL object or pointer (d_actual_in alone
 * may be NULL) or an unknown format; n_chunks == 0 does nothing.  The _dict
 * form follows libdeflate_amd_decompress_batch_dict: it refuses gzip, and a
 * distance may reach into the dictionary.
 *
 * Cost: a stream runs on one wave.  Whole rounds of the decode run below the
 * limit, the last of them clipped to it; behind that lane 0 walks less than
 * one lane's piece of tokens (48 bytes of input) to the cut.  A prefix of many MiB of ONE huge stream therefore runs
 * at the one-wave rate (libdeflate_amd_decompress_large has no prefix form).
 * In zlib and gzip format the checksum batch runs over every stream's
 * d_actual_out bytes, a cut stream's prefix included, though only the streams
 * that ended are compared with their footer.
 */
#define LIBDEFLATE_AMD_PREFIX 19	/* a per-stream result: cut at its limit */

LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix_batch(struct libdeflate_decompressor *decompressor, int format,
				       size_t n_chunks, const void *d_in,
				       const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
				       void *d_out, const uint64_t *d_out_offsets,
				       const uint64_t *d_limits, int32_t *d_results,
				       uint64_t *d_actual_in /* may be NULL */,
				       uint64_t *d_actual_out, void *stream);

LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix_batch_dict(struct libdeflate_decompressor *decompressor,
					    int format, size_t n_chunks, const void *d_dict,
					    size_t dict_nbytes, const void *d_in,
					    const uint64_t *d_in_offsets,
					    const uint64_t *d_in_nbytes, void *d_out,
					    const uint64_t *d_out_offsets, const uint64_t *d_limits,
					    int32_t *d_results,
					    uint64_t *d_actual_in /* may be NULL */,
					    uint64_t *d_actual_out, void *stream);

/*
 * One stream, HOST pointers, blocking: `out` has room for `limit` bytes.
 * Returns an enum libdeflate_result value or LIBDEFLATE_AMD_PREFIX, as
 * d_results[] above; *actual_out_ret (required) is set on LIBDEFLATE_SUCCESS
 * and on LIBDEFLATE_AMD_PREFIX (to `limit`), and that many bytes of `out` are
 * written.  A bad argument or a library-side failure is LIBDEFLATE_BAD_DATA
 * with the reason in libdeflate_amd_last_error(), as with the single-buffer
 * calls.  The object's staging buffer grows to in_nbytes + limit bytes of
 * device memory: `limit` is the room the caller has, not a way to say "no
 * limit" (a value above SIZE_MAX / 4 is a bad argument).
 */
LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix(struct libdeflate_decompressor *decompressor, int format,
				 const void *in, size_t in_nbytes, void *out, size_t limit,
				 size_t *actual_out_ret);

/*
 * The heads of the members of a file of concatenated gzip members: the first
 * head_nbytes bytes of every member in one enqueue, with nothing crossing to
 * the host - libdeflate_amd_gzip_members_index_batch, this call, the caller's
 * filter over the heads, then libdeflate_amd_decompress_batch_packed over the
 * chosen members, all on one stream.
 *
 * d_result and d_index are DEVICE memory as
 * libdeflate_amd_gzip_members_index_batch wrote them for (d_in, in_nbytes)
 * with at least max_members rows.  Row r < min(d_result[1], max_members) is
 * member r: d_heads[r * head_nbytes ..] gets the first head_nbytes bytes of
 * what it decodes to (all of it where it is shorter), d_head_nbytes[r] how
 * many they are and d_results[r] LIBDEFLATE_SUCCESS (the member ended within
 * head_nbytes and was checked in full), LIBDEFLATE_AMD_PREFIX, or the
 * member's failure (d_head_nbytes[r] is then meaningless, as d_actual_out of
 * libdeflate_amd_decompress_prefix_batch).  The rows at and beyond the member
 * count are empty: d_head_nbytes[r] = 0, d_results[r] = 0, no byte of their
 * d_heads row written.  So are ALL rows when d_result[0] is not
 * LIBDEFLATE_SUCCESS - a verdict under which the index is not written - and
 * every row whose index pair does not lie inside in_nbytes.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work: a NULL object or pointer
 * (d_in may be NULL with in_nbytes == 0, d_heads with head_nbytes == 0),
 * max_members == 0 or above 2^28, head_nbytes above 2^32 - 1.  No ZIP
 * counterpart: a ZIP selection goes through host rows, from which a caller
 * builds prefix descriptors itself.
 */
LIBDEFLATEAPI int
libdeflate_amd_gzip_members_peek_batch(struct libdeflate_decompressor *decompressor,
				       const void *d_in, size_t in_nbytes,
				       const uint64_t *d_result, const uint64_t *d_index,
				       size_t max_members, size_t head_nbytes, void *d_heads,
				       uint64_t *d_head_nbytes, int32_t *d_results, void *stream);

/*
 * Byte-shuffled deflate chunks: the chunked arrays of HDF5 and NetCDF-4
 * (filters shuffle, then deflate) and of Zarr (numcodecs.Shuffle, then Zlib or
 * GZip).  A chunk is one ordinary zlib, gzip or raw DEFLATE stream whose content
 * is the chunk's bytes transposed.  A chunk of n raw bytes and element size es
 * has ne = n / es elements and left = n % es bytes behind them:
 *
 *     shuffled[j * ne + k]  = raw[k * es + j]      0 <= j < es, 0 <= k < ne
 *     shuffled[es * ne + t] = raw[es * ne + t]     0 <= t < left
 *
 * (H5Z_FILTER_SHUFFLE; the identity when es == 1 or ne <= 1).  Raw bytes 0..9
 * with es 4 are shuffled 0 4 1 5 2 6 3 7 8 9.
 *
 * A chunk is described by a row of LIBDEFLATE_AMD_SHUF_WORDS uint64_t on the
 * HOST:
 *   [0] the offset of the stored chunk in the compressed buffer
 *   [1] its stored size
 *   [2] the offset of the chunk's raw bytes in the raw buffer (its room)
 *   [3] the chunk's raw size: exact, and below 2^32
 *   [4] the element size, 1 .. LIBDEFLATE_AMD_SHUF_ELEM_MAX
 *   [5] a mask: LIBDEFLATE_AMD_SHUF_NO_DEFLATE - the stored bytes are the
 *       shuffled bytes themselves (HDF5's filter mask of a chunk on which the
 *       optional deflate filter was skipped) -, LIBDEFLATE_AMD_SHUF_NO_SHUFFLE -
 *       the shuffle was skipped.  Any other bit is refused.
 *
 * The reader.  format is LIBDEFLATE_AMD_DEFLATE, _ZLIB or _GZIP.  The call only
 * enqueues on `stream`; the rows go up through the object's pinned block and
 * the scratch is the object's (object and stream rules:
 * libdeflate_amd_decompress_batch).  d_results[i] is what
 * libdeflate_<format>_decompress_ex reports for the chunk with out_nbytes_avail
 * = word 3 and a NULL actual_out: LIBDEFLATE_SUCCESS only if the stream fills
 * the raw size exactly, else SHORT_OUTPUT, INSUFFICIENT_SPACE or BAD_DATA.  A
 * NO_DEFLATE row succeeds if and only if word 1 equals word 3; otherwise it is
 * BAD_DATA and its room is not written.  A failed chunk's room is undefined; no
 * byte outside the rooms is ever written; a failed chunk never affects its
 * neighbours.  The rooms must not overlap each other or d_in (not checked).
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with the row and the reason
 * in libdeflate_amd_last_error(): a NULL object or pointer (d_in with
 * in_nbytes == 0 and d_out with out_avail == 0 may be NULL), an unknown format,
 * n_chunks above 2^28, an element size of 0 or above 256, unknown mask bits, a
 * raw size of 2^32 or more, a stored range outside in_nbytes, a room outside
 * out_avail.  n_chunks == 0 does nothing and returns 0.
 *
 * Cost: the deflated rows whose transform is not the identity are decoded into
 * scratch and transposed by one memory-bound kernel over all chunks (tiles of
 * elements, so many small chunks and one huge chunk are the same work); the
 * others are decoded straight into d_out, in a decompress batch of their own.
 * A batch that is identity throughout queues what
 * libdeflate_amd_decompress_batch queues, plus one small kernel.
 *
 * The writer.  Rows use words 2 to 5 (the raw bytes in d_in); words 0 and 1 are
 * ignored and only LIBDEFLATE_AMD_SHUF_NO_SHUFFLE is allowed in the mask: a
 * reader's row is a valid writer's row.  Stream k - header, DEFLATE stream,
 * footer - is byte for byte what libdeflate_<format>_compress() of this build
 * returns for the shuffled chunk at the object's level, and stands behind
 * stream k - 1, from offset 0 of d_out.  Chunks of many MiB are compressed as
 * primed segments like libdeflate_amd_compress_large_batch's.  d_result
 * (LIBDEFLATE_AMD_SHUFW_RESULT_WORDS uint64_t, device): [0] 0 or
 * LIBDEFLATE_INSUFFICIENT_SPACE - then nothing is written -, [1] the bytes
 * written in all, [2] the raw bytes in all, [3] the chunks.  d_index (device, may
 * be NULL) receives the reader's rows: word 0 the stream's offset in d_out,
 * word 1 its size, words 2 to 5 the input's; d_out and these rows can go
 * straight to the reader.  libdeflate_amd_shuffle_compress_bound is the sum of
 * libdeflate_<format>_compress_bound(raw size), room enough for out_avail; 0
 * for rows the call refuses.  LIBDEFLATE_AMD_BAD_ARG mirrors the reader's
 * (in_avail in the place of out_avail; d_out and d_result must not be NULL).
 * The call only enqueues; conventions are libdeflate_amd_png_encode_batch's.
 *
 * Not covered: the Fletcher-32, N-bit, scale-offset and szip filters;
 * bitshuffle, delta and blosc; parsing a file's own metadata (the caller maps
 * its chunk index onto the rows: INTEGRATION.md); element sizes above 256;
 * chunks of 2^32 bytes or more; routing huge chunks to the many-wave decoder
 * (a chunk is decoded by one wave); store-if-larger in the writer (no chunk is
 * written with NO_DEFLATE); host-pointer forms.
 */
#define LIBDEFLATE_AMD_SHUF_WORDS 6
#define LIBDEFLATE_AMD_SHUF_ELEM_MAX 256
#define LIBDEFLATE_AMD_SHUF_NO_DEFLATE 1
#define LIBDEFLATE_AMD_SHUF_NO_SHUFFLE 2
#define LIBDEFLATE_AMD_SHUFW_RESULT_WORDS 4

LIBDEFLATEAPI int
libdeflate_amd_shuffle_decompress_batch(struct libdeflate_decompressor *decompressor, int format,
					size_t n_chunks, const uint64_t *chunks /* host rows */,
					const void *d_in, size_t in_nbytes, void *d_out,
					size_t out_avail, int32_t *d_results, void *stream);

LIBDEFLATEAPI size_t
libdeflate_amd_shuffle_compress_bound(struct libdeflate_compressor *compressor, int format,
				      size_t n_chunks, const uint64_t *chunks);

LIBDEFLATEAPI int
libdeflate_amd_shuffle_compress_batch(struct libdeflate_compressor *compressor, int format,
				      size_t n_chunks, const uint64_t *chunks /* host rows */,
				      const void *d_in, size_t in_avail, void *d_out,
				      size_t out_avail, uint64_t *d_result,
				      uint64_t *d_index /* may be NULL */, void *stream);

/*
 * Predictor-coded deflate strips and tiles: TIFF with Compression = 8 (Adobe
 * deflate; 32946 is the same thing) - GeoTIFF, Cloud-Optimized GeoTIFF tiles,
 * OME-TIFF planes, float rasters.  A *segment* is a strip or a tile: one zlib
 * stream that decodes to coded_rows rows of coded_width pixels, each pixel spp
 * samples of bps bytes, pixel-interleaved, samples little-endian.  The rows of
 * a segment were coded by the file's Predictor (tag 317):
 *
 *   1  none.
 *   2  horizontal differencing: every sample minus the sample of the same
 *      channel one pixel to the left, modulo 2^(8 bps); the first pixel of a
 *      row as it is.
 *   3  floating point: the row's samples split into bps byte planes, the most
 *      significant byte's plane first, then every byte of the row of planes
 *      minus the byte spp places earlier (across the planes' boundaries).
 *
 * Undoing 2 is a prefix sum per row and channel; undoing 3 a prefix sum over
 * the bytes of the whole coded row and a gather from the planes.
 *
 * A segment is described by a row of LIBDEFLATE_AMD_TIFF_WORDS uint64_t on the
 * HOST:
 *   [0] the offset of the stored segment in the compressed buffer
 *   [1] its stored size
 *   [2] the offset, in the raw buffer, of the segment's kept pixel (0, 0)
 *   [3] the pitch in bytes between kept rows in the raw buffer
 *   [4] coded_width | coded_rows << 32; both at least 1, and coded_width *
 *       coded_rows * spp * bps below 2^32
 *   [5] kept_width | kept_rows << 32; 1 <= kept <= coded.  The rectangle that
 *       is written: an edge tile's padding is cropped, a strip is kept whole
 *   [6] spp (bits 0-7, 1 .. LIBDEFLATE_AMD_TIFF_SPP_MAX) | bps << 8 (1, 2, 4,
 *       8) | predictor << 16 (1, 2, 3; 3 needs bps 2, 4 or 8).  Any other bit
 *       is refused
 *   [7] reserved, must be 0
 *
 * The format is always zlib: TIFF prescribes it.
 *
 * The reader.  The call only enqueues on `stream`; object and stream rules are
 * libdeflate_amd_shuffle_decompress_batch's.  d_results[i] is what
 * libdeflate_zlib_decompress_ex reports for the stream with out_nbytes_avail =
 * the coded size and a NULL actual_out: LIBDEFLATE_SUCCESS only if the stream
 * fills the coded size exactly, else SHORT_OUTPUT, INSUFFICIENT_SPACE or
 * BAD_DATA.  On success the kept rectangle holds the pixels: row r of it the
 * kept_width * spp * bps bytes at word 2 + r * pitch.  The bytes of the pitch
 * behind a kept row are never written, and nothing outside the kept rectangles
 * is: neighbouring tiles interleave in one H x W x C image.  A failed segment
 * leaves only its own rectangle undefined.  The rectangles must not overlap
 * each other or d_in (not checked).
 *
 * The writer.  Rows use words 2 to 7, the raw pixels in d_in at that pitch: a
 * reader's row is a valid writer's row.  The coded segment is the kept
 * rectangle, padded on the right and at the bottom with zero samples up to the
 * coded size, then predicted.  Stream k is byte for byte what
 * libdeflate_zlib_compress() of this build returns for the predicted segment
 * at the object's level, and stands behind stream k - 1, from offset 0 of
 * d_out.  Segments of 128 KiB and more are compressed as primed segments like
 * libdeflate_amd_compress_large_batch's.  d_result
 * (LIBDEFLATE_AMD_TIFFW_RESULT_WORDS uint64_t, device): [0] 0 or
 * LIBDEFLATE_INSUFFICIENT_SPACE - then nothing is written -, [1] the bytes
 * written in all, [2] the kept rectangles' bytes in all, [3] the segments.
 * d_index (device, may be NULL) receives the reader's rows: word 0 the
 * stream's offset in d_out, word 1 its size, words 2 to 7 the input's.
 * libdeflate_amd_tiff_encode_bound is the sum of
 * libdeflate_zlib_compress_bound(coded size), room enough for out_avail; 0 for
 * rows the call refuses.  The call only enqueues; conventions are
 * libdeflate_amd_shuffle_compress_batch's.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with "row N:" and the reason
 * in libdeflate_amd_last_error(): a NULL object or pointer (the reader's d_in
 * with in_nbytes == 0 and d_out with out_avail == 0 may be NULL, the writer's
 * d_in with in_avail == 0; its d_out and d_result must not be), n_segments
 * above 2^28, a zero width or zero rows, kept above coded, spp 0 or above 16,
 * bps not 1, 2, 4 or 8, a predictor not 1, 2 or 3, predictor 3 with bps 1,
 * unknown bits in word 6, word 7 not 0, a coded size of 2^32 or more, a stored
 * range outside in_nbytes, a kept rectangle whose last byte (word 2 +
 * (kept_rows - 1) * pitch + the kept row's bytes) lies outside out_avail (the
 * writer: in_avail), overflow included, a pitch below the kept row's bytes
 * when kept_rows > 1; in the writer at level 0, a coded size above 0xFFFFFF00.
 * n_segments == 0 does nothing and returns 0.
 *
 * Cost: a row that is direct - predictor 1, kept equal to coded, the pitch
 * equal to the row's bytes or a single row - is decoded straight into d_out;
 * every other row into scratch, and one memory-bound kernel over the kept rows
 * of all segments undoes the predictor on the way to d_out (predictor 3: two
 * kernels).  A batch that is direct throughout queues what
 * libdeflate_amd_decompress_batch queues, plus one small kernel.
 *
 * Not covered: parsing the file on the device (libdeflate_amd/tiff.py walks
 * the IFDs on the host and makes the rows: INTEGRATION.md); big-endian (MM)
 * sample order; sample sizes that are not 1, 2, 4 or 8 bytes;
 * PlanarConfiguration = 2 beyond what spp = 1 rows already give (planes as
 * separate images); the LZW, JPEG, ZSTD and LERC compressions; uncompressed
 * segments; routing huge strips to the many-wave decoder (a segment is decoded
 * by one wave); writing the file's IFD on the device.
 */
#define LIBDEFLATE_AMD_TIFF_WORDS 8
#define LIBDEFLATE_AMD_TIFF_SPP_MAX 16
#define LIBDEFLATE_AMD_TIFFW_RESULT_WORDS 4

LIBDEFLATEAPI int
libdeflate_amd_tiff_decode_batch(struct libdeflate_decompressor *decompressor, size_t n_segments,
				 const uint64_t *rows /* host rows */, const void *d_in,
				 size_t in_nbytes, void *d_out, size_t out_avail,
				 int32_t *d_results, void *stream);

LIBDEFLATEAPI size_t
libdeflate_amd_tiff_encode_bound(struct libdeflate_compressor *compressor, size_t n_segments,
				 const uint64_t *rows);

LIBDEFLATEAPI int
libdeflate_amd_tiff_encode_batch(struct libdeflate_compressor *compressor, size_t n_segments,
				 const uint64_t *rows /* host rows */, const void *d_in,
				 size_t in_avail, void *d_out, size_t out_avail, uint64_t *d_result,
				 uint64_t *d_index /* may be NULL */, void *stream);

/*
 * OpenEXR chunks with the ZIP (16 scanlines a chunk) and ZIPS (1 scanline)
 * compressions, scanline blocks and tiles: what the OpenEXR library writes by
 * default.  A raw chunk holds `lines` lines of `width` pixels channel-planar:
 * for every line in turn, for every channel in the file's chlist order, the
 * line's samples of that channel, HALF (2 bytes) or FLOAT / UINT (4 bytes),
 * little-endian; n = lines * width * (the sum of the sample sizes) bytes.  The
 * file stores it coded, with h = (n + 1) / 2:
 *
 *   t[k] = raw[2k] (k < h), t[h + k] = raw[2k + 1]: the even bytes, then the odd
 *   p[0] = t[0], p[i] = t[i] - t[i - 1] + 128 (mod 256)
 *   data = the zlib stream of p - or, where that is not shorter than n, raw
 *          itself: a reader tells the two apart by dataSize alone
 *
 * Undoing it is one byte-wise running sum over the whole chunk, an XOR of 0x80
 * at the odd places, and the interleave of the two halves.
 *
 * A chunk is described by a row of LIBDEFLATE_AMD_EXR_WORDS uint64_t on the
 * HOST:
 *   [0] the offset of the chunk's data - the byte behind its dataSize field -
 *       in the compressed buffer
 *   [1] dataSize
 *   [2] the offset, in the pixel buffer, of the chunk's line 0, pixel 0
 *   [3] the pitch in bytes between lines in the pixel buffer
 *   [4] width | lines << 32; both at least 1, and n below 2^32
 *   [5] channels c (bits 0-7, 1 .. LIBDEFLATE_AMD_EXR_CHANNELS_MAX) | wide mask
 *       << 8 (bit k set: channel k of the file has 4-byte samples, else 2) |
 *       layout << 32 (LIBDEFLATE_AMD_EXR_LINES, _PIXELS).  Any other bit is
 *       refused
 *   [6] PIXELS: 4 bits per channel, the slot of the file's channel k in the
 *       pixel; a permutation of 0 .. c - 1.  LINES: 0
 *   [7] the length of the chunk's head in bytes: 0 (none), 8 (a scanline
 *       chunk: y, dataSize) or 20 (a tile: tileX, tileY, levelX, levelY,
 *       dataSize)
 *   [8], [9] the head's int32 values in front of dataSize, the low half first
 *       (length 8: one value, length 20: four).  The reader ignores them
 *
 * LINES is the file's own arrangement at a pitch: line y at word 2 + y *
 * pitch holds the channels' planes one after another.  PIXELS interleaves:
 * pixel x of line y stands at word 2 + y * pitch + x * px, px the sum of the
 * sample sizes, and inside it the channels stand in slot order, each with its
 * own size - so the file's A, B, G, R become an H x W x 4 RGBA tensor with
 * slots 3, 2, 1, 0.  Samples are never converted: half stays half.  Lines of
 * neighbouring chunks and tiles interleave in one image through offset and
 * pitch; an edge tile's row has the tile's own width and lines.
 *
 * The reader.  The call only enqueues on `stream`; object, stream, scratch and
 * pinned-block rules are libdeflate_amd_tiff_decode_batch's.  d_results[i]:
 * dataSize == n: LIBDEFLATE_SUCCESS, the data is raw and is laid out; dataSize
 * > n: LIBDEFLATE_BAD_DATA; else what libdeflate_zlib_decompress_ex reports
 * for the stream with out_nbytes_avail = n and a NULL actual_out -
 * LIBDEFLATE_SUCCESS only if the stream fills n exactly, else SHORT_OUTPUT,
 * INSUFFICIENT_SPACE or BAD_DATA.  The bytes of the pitch behind a line are
 * never written, and nothing outside the chunks' lines is.  A failed chunk
 * leaves only its own lines undefined.  The chunks' lines must not overlap
 * each other or d_in (not checked).
 *
 * The writer.  Rows use words 2 to 9, the pixels in d_in: a reader's row is a
 * valid writer's row.  Every chunk's lines are gathered into the raw chunk and
 * coded, and the coded bytes compressed to, byte for byte, what
 * libdeflate_zlib_compress() of this build returns for them at the object's
 * level (chunks of 128 KiB and more as primed segments like
 * libdeflate_amd_compress_large_batch's).  Chunk k is written behind chunk k -
 * 1, from offset 0 of d_out: the head's ints, int32 dataSize (a head of 0
 * bytes: neither), then the data - the zlib stream if it is shorter than n,
 * else the raw chunk with dataSize = n.  The choice is the format's and is not
 * optional; at level 0 every chunk ends up raw.  d_result
 * (LIBDEFLATE_AMD_EXRW_RESULT_WORDS uint64_t, device): [0] 0 or
 * LIBDEFLATE_INSUFFICIENT_SPACE - then nothing is written -, [1] the bytes
 * written in all, [2] the raw bytes in all, [3] the chunks.  d_index (device,
 * may be NULL) receives the reader's rows: word 0 the offset of the data in
 * d_out (the head starts word 7 bytes earlier), word 1 the chosen dataSize,
 * words 2 to 9 the input's.  libdeflate_amd_exr_encode_bound is the sum of
 * head + n, which no output exceeds; 0 for rows the call refuses.  The call
 * only enqueues; conventions are libdeflate_amd_tiff_encode_batch's.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with "row N:" and the reason
 * in libdeflate_amd_last_error(): a NULL object or pointer (as the TIFF calls),
 * n_chunks above 2^28, unknown bits in word 5, c of 0 or above 16, a mask bit
 * at or above c, a zero width or zero lines, word 6 not 0 for LINES or not a
 * permutation for PIXELS, a head length that is not 0, 8 or 20, n of 2^32 or
 * more, a stored range outside in_nbytes, a pitch below the line's bytes when
 * lines > 1, a last byte (word 2 + (lines - 1) * pitch + the line's bytes)
 * outside out_avail (the writer: in_avail), overflow included; in the writer
 * at level 0, n above 0xFFFFFF00.  n_chunks == 0 does nothing and returns 0.
 *
 * Cost: a zlib chunk is inflated into scratch; three memory-bound launches
 * over the bytes of all chunks (sums, carries, tiles) undo the coding - a row
 * that is direct (LINES at a pitch equal to the line's bytes, or one line)
 * straight into d_out, any other into a second room that the layout kernel
 * reads.  A raw chunk is copied, or laid out straight from d_in.  A batch of
 * direct raw rows queues one copy kernel and one small kernel.
 *
 * Not covered: the PXR24, PIZ, RLE, B44 and DWA compressions; multi-part and
 * deep files; mip and rip levels; subsampled channels; half-to-float
 * conversion; routing huge chunks to the many-wave decoder (a chunk is decoded
 * by one wave); parsing the file on the device (libdeflate_amd/exr.py reads
 * the header and the chunk heads on the host and makes the rows:
 * INTEGRATION.md); host-pointer forms.  No file written by the OpenEXR library
 * has been read yet: the format facts above are the specification this was
 * built against.
 */
#define LIBDEFLATE_AMD_EXR_WORDS 10
#define LIBDEFLATE_AMD_EXR_CHANNELS_MAX 16
#define LIBDEFLATE_AMD_EXRW_RESULT_WORDS 4
#define LIBDEFLATE_AMD_EXR_LINES 0
#define LIBDEFLATE_AMD_EXR_PIXELS 1

LIBDEFLATEAPI int
libdeflate_amd_exr_decode_batch(struct libdeflate_decompressor *decompressor, size_t n_chunks,
				const uint64_t *rows /* host rows */, const void *d_in,
				size_t in_nbytes, void *d_out, size_t out_avail, int32_t *d_results,
				void *stream);

LIBDEFLATEAPI size_t
libdeflate_amd_exr_encode_bound(struct libdeflate_compressor *compressor, size_t n_chunks,
				const uint64_t *rows);

LIBDEFLATEAPI int
libdeflate_amd_exr_encode_batch(struct libdeflate_compressor *compressor, size_t n_chunks,
				const uint64_t *rows /* host rows */, const void *d_in,
				size_t in_avail, void *d_out, size_t out_avail, uint64_t *d_result,
				uint64_t *d_index /* may be NULL */, void *stream);

/*
 * The pages of flat Parquet column chunks, GZIP-coded or uncompressed, turned
 * into columns: what pandas.to_parquet(compression="gzip") and the warehouse
 * exports write.  A column chunk is a sequence of pages, each behind a Thrift
 * header that states its sizes: an optional dictionary page, then data pages.
 * With the GZIP codec a compressed page is one gzip member (Arrow's reader
 * takes zlib streams too: `format`).  A flat column has max_repetition_level
 * 0; a nullable one has max_definition_level 1 and stores, per slot (row), a
 * definition level 1 (a value follows) or 0 (null), and values for the valid
 * slots only.
 *
 *   data page V1   body = [levels, if max_def 1: a 4-byte LE length, then that
 *                  many bytes of hybrid stream of bit width 1][values]; the
 *                  whole body is compressed
 *   data page V2   body = [levels, definition_levels_byte_length bytes of
 *                  hybrid stream, never compressed and with no length in
 *                  front][values, compressed where is_compressed says so]
 *   dictionary     body = entries x width bytes, PLAIN; compressed as a whole
 *   values         PLAIN: the valid slots' values, width bytes each, back to
 *                  back.  PLAIN_DICTIONARY / RLE_DICTIONARY: one byte w, the
 *                  bit width, then a hybrid stream of bit width w of indices
 *                  into the chunk's dictionary, one per valid slot
 *
 * The RLE / bit-packed hybrid stream.  A stream of bit width w that owes N
 * values is a sequence of runs, each behind a ULEB128 header h.  h & 1 set: h
 * >> 1 groups of 8 values, bit-packed LSB-first in (h >> 1) * w bytes; only
 * the bytes that cover the values still owed must lie inside the stream.  h &
 * 1 clear: h >> 1 copies of the value in the next ceil(w / 8) bytes,
 * little-endian.  Values behind the Nth, and bytes behind the last run that is
 * needed, are ignored.
 *
 * A page is described by a row of LIBDEFLATE_AMD_PARQUET_WORDS uint64_t on the
 * HOST (libdeflate_amd/parquet.py makes them from a file's footer and page
 * headers):
 *   [0] the offset of the page body - the byte behind its Thrift header - in
 *       d_in
 *   [1] compressed_page_size
 *   [2] uncompressed_page_size; both below 2^31
 *   [3] kind (bits 0-3: LIBDEFLATE_AMD_PARQUET_DATA_V1 0, _DICT 2, _DATA_V2 3)
 *       | encoding << 4 (0 PLAIN, 2 PLAIN_DICTIONARY, 8 RLE_DICTIONARY; a
 *       dictionary page: 0) | body_is_compressed << 12 (V2: is_compressed)
 *       | max_def << 13 (0 or 1; a dictionary page: 0) | (width - 1) << 16
 *       (the value's bytes, 1 .. 256: INT32 and FLOAT 4, INT64 and DOUBLE 8,
 *       INT96 12, FIXED_LEN_BYTE_ARRAY its length).  Any other bit is refused
 *   [4] num_values (the slots, nulls included; a dictionary page: its entries;
 *       below 2^31) | definition_levels_byte_length << 32 (a V2 data page
 *       with max_def 1 only, else 0)
 *   [5] a data page: the byte offset in d_out of the page's slot 0
 *   [6] a data page with max_def 1: the byte offset in d_valid of slot 0's
 *       validity byte
 *   [7] a dictionary-coded data page: the index, in this call, of the row of
 *       its dictionary page, which must come earlier and have the same width
 *   A dictionary page ignores words 5 to 7, a PLAIN data page word 7, a page
 *   with max_def 0 word 6.
 *
 * Output.  Slot r of a page holds its value at word 5 + r * width, or width
 * zero bytes for a null; d_valid holds one byte per slot, 1 or 0 - a
 * torch.bool tensor as it lies -, written only for rows with max_def 1.
 * Nothing outside the pages' slots and validity bytes is written.  A failed
 * page leaves only its own slots and validity bytes undefined.  The pages'
 * slots must not overlap each other or d_in (not checked).  The call only
 * enqueues on `stream`; object, stream, scratch and pinned-block rules are
 * libdeflate_amd_tiff_decode_batch's.
 *
 * d_results[i], one enum libdeflate_result per row.  The *section* of a page
 * is what the codec covers: the body of a V1 data page or a dictionary page,
 * the values behind the levels of a V2 page (a V2 page's levels are never part
 * of it).  A compressed section: what libdeflate_<format>_decompress_ex reports
 * for it with out_nbytes_avail = the section's uncompressed size (word 2, less
 * the level bytes of a V2 page) and a NULL actual_out - SUCCESS only if it
 * fills that size exactly, else SHORT_OUTPUT, INSUFFICIENT_SPACE or BAD_DATA.
 * Where that is SUCCESS, and for an uncompressed section:
 *   a dictionary page: LIBDEFLATE_BAD_DATA where the section is shorter than
 *   entries x width, else SUCCESS;
 *   a data page whose dictionary page did not end in SUCCESS:
 *   LIBDEFLATE_BAD_DATA;
 *   any other data page: LIBDEFLATE_BAD_DATA for a run of 0 groups or 0 copies;
 *   a run header of more than 5 bytes; a run that leaves its stream before N
 *   is reached (a missing bit-width byte included); an index bit width w above
 *   32; an RLE level above 1; a V1 level length prefix that leaves the page; an
 *   index at or above the dictionary's entry count among the values owed; a
 *   values section shorter than (the valid slots) x width; else SUCCESS.  A
 *   dictionary-coded page without a valid slot needs no values section at all.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, with "row N:" and the reason
 * in libdeflate_amd_last_error(): a NULL object or pointer (d_in, d_out with a
 * size of 0 may be NULL; d_valid may be NULL while no row has max_def 1), a
 * format other than DEFLATE, ZLIB and GZIP, n_pages above 2^28, unknown bits,
 * kinds or encodings in word 3, a dictionary encoding or max_def on a
 * dictionary page, a size or count of 2^31 or more, level bytes on a row that
 * is not a V2 data page with max_def 1 or beyond either size, an uncompressed
 * body with word 1 != word 2, a dictionary reference that is not an earlier
 * dictionary row of the same width, a body outside in_nbytes, slots outside
 * out_avail or validity bytes outside valid_avail (overflow included), d_valid
 * NULL while a row has max_def 1.  n_pages == 0 does nothing and returns 0.
 *
 * Cost: compressed sections are inflated into scratch in one batch, a page by
 * one wave; one wave per data page then walks its hybrid streams run by run
 * (the only serial part, a step per run) and lists the runs in scratch - up to
 * 16 bytes per slot of a page with levels or indices -; one memory-bound launch
 * over the slots of all pages writes values and validity.
 *
 * Not covered: BYTE_ARRAY (strings: libdeflate_amd_parquet_decode_batch_ex
 * below reads them) and BOOLEAN columns; nested and repeated
 * columns (max_rep above 0, max_def above 1); the DELTA_* encodings and
 * BYTE_STREAM_SPLIT; the Snappy, ZSTD, LZ4 and Brotli codecs; page CRCs;
 * encryption; the page index and bloom filters; writing; host-pointer forms;
 * routing pages so large that they want the many-wave decoder (a page is
 * decoded by one wave); parsing the file on the device
 * (libdeflate_amd/parquet.py reads the footer and the page headers on the host
 * and makes the rows: INTEGRATION.md).
 */
#define LIBDEFLATE_AMD_PARQUET_WORDS 8
#define LIBDEFLATE_AMD_PARQUET_DATA_V1 0
#define LIBDEFLATE_AMD_PARQUET_DICT 2
#define LIBDEFLATE_AMD_PARQUET_DATA_V2 3

LIBDEFLATEAPI int
libdeflate_amd_parquet_decode_batch(struct libdeflate_decompressor *decompressor, int format,
				    size_t n_pages, const uint64_t *rows /* host rows */,
				    const void *d_in, size_t in_nbytes, void *d_out, size_t out_avail,
				    void *d_valid /* may be NULL */, size_t valid_avail,
				    int32_t *d_results, void *stream);

/*
 * The same call with BYTE_ARRAY columns - Parquet's `string` and `binary` -
 * read into Arrow's large layout: int64 offsets in d_out and one run of bytes
 * in d_bytes.  A row without LIBDEFLATE_AMD_PARQUET_BYTE_ARRAY (word 3 bit 14)
 * means exactly what it means above and is decoded by the same kernels in the
 * same call; a row with it describes a BYTE_ARRAY page, and its width field
 * must be 0.  (libdeflate_amd_parquet_decode_batch goes on refusing the bit.)
 *
 * A BYTE_ARRAY value is a 4-byte little-endian length and that many bytes.  A
 * dictionary page holds `entries` of them, a PLAIN data page one per valid
 * slot; a dictionary-coded data page holds indices as above.
 *
 * Output of a BYTE_ARRAY data page.  Word 5 is the byte offset in d_out, a
 * multiple of 8, of count + 1 little-endian int64 entries: entry r is where
 * slot r's bytes start in d_bytes, entry `count` where they end.  A null slot
 * has length 0.  The entries are absolute positions in d_bytes: the bytes of
 * all BYTE_ARRAY data pages of the call lie back to back in d_bytes in row
 * order from 0, so that nothing has to come back to the host to place them,
 * and the consecutive data pages of one column - while no other column's
 * BYTE_ARRAY data page stands between them in the call (not checked) - make one
 * Arrow array: lay page k + 1's entries at page k's entry `count`, which both
 * write with the same value.  (Arrow allows offsets[0] != 0.)  Dictionary pages
 * and fixed-width rows take no room.  Validity bytes are as above (word 6).
 *
 * Capacity.  d_bytes_total[0] (device memory) is always written: the room the
 * call's BYTE_ARRAY pages take.  A page whose bytes do not end at or below
 * bytes_avail writes none of them and ends as LIBDEFLATE_INSUFFICIENT_SPACE;
 * its entries and validity bytes are still written, and no byte at or behind
 * bytes_avail is touched.  d_bytes NULL with bytes_avail 0 is the sizing call.
 * A failed page's entries and bytes are undefined; it takes no room where its
 * levels, its indices, its values' walk or its dictionary failed, and else -
 * an index at or above the entry count - the room of its other slots, the bad
 * index counting as length 0.
 *
 * d_results[i] of a BYTE_ARRAY row: as above, with width 1 wherever a width is
 * asked for, and where that is SUCCESS: LIBDEFLATE_BAD_DATA for a dictionary
 * page whose section ends before `entries` length-prefixed values do (inside a
 * prefix included), for a PLAIN data page whose values section ends before
 * (the valid slots) values do, and for a data page whose dictionary failed so;
 * else LIBDEFLATE_INSUFFICIENT_SPACE as said; else SUCCESS.
 *
 * LIBDEFLATE_AMD_BAD_ARG before any device work, beyond the list above: bit 14
 * with a non-zero width field; word 5 of a BYTE_ARRAY data page not a multiple
 * of 8; a dictionary reference across types (bit 14 on one side only); entries
 * outside out_avail for (count + 1) * 8; d_bytes_total NULL while a row has bit
 * 14; d_bytes NULL with bytes_avail != 0; non-zero flags.  d_bytes_total may
 * be NULL otherwise.  The call only enqueues; object, stream, scratch and
 * pinned-block rules are the old call's.
 *
 * Cost beyond the old call's: a wave per dictionary page and PLAIN data page
 * lists the starts of its values (4 bytes of scratch per value) - the chain of
 * length prefixes is broken up by pointer doubling in windows of 1 KiB, so a
 * long string is a jump and 256 empty ones nine rounds -; two launches over
 * the slots sum and scan the lengths and write the entries (16 bytes of scratch
 * per slot); one launch over the output bytes, 4 KiB a workgroup, gathers them.
 *
 * Not covered: int32 offsets; BOOLEAN; DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY
 * and the other DELTA encodings; UTF-8 validation; and what the old call does
 * not cover.
 */
#define LIBDEFLATE_AMD_PARQUET_BYTE_ARRAY ((uint64_t)1 << 14)

LIBDEFLATEAPI int
libdeflate_amd_parquet_decode_batch_ex(struct libdeflate_decompressor *decompressor, int format,
				       size_t n_pages, const uint64_t *rows /* host rows */,
				       const void *d_in, size_t in_nbytes, void *d_out,
				       size_t out_avail, void *d_valid /* may be NULL */,
				       size_t valid_avail, void *d_bytes /* may be NULL */,
				       size_t bytes_avail, uint64_t *d_bytes_total /* uint64_t[1] */,
				       uint64_t flags /* 0 */, int32_t *d_results, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LIBDEFLATE_AMD_H */
