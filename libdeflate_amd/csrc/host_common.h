/*
 * host_common.h - host-side plumbing shared by the C-ABI translation units:
 * per-device context (constant tables, staging buffer), error reporting.
 */
#ifndef LDA_HOST_COMMON_H
#define LDA_HOST_COMMON_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <exception>
#include <functional>
#include <mutex>

#include "../../include/libdeflate_amd.h"

namespace lda {

void set_error(const char *fmt, ...);

#define LDA_HIP_TRY(expr, failret)                                           \
	do {                                                                 \
		hipError_t e_ = (expr);                                      \
		if (e_ != hipSuccess) {                                      \
			lda::set_error("%s: %s", #expr, hipGetErrorString(e_)); \
			return failret;                                      \
		}                                                            \
	} while (0)
/* ... for a call of ours that returns a LIBDEFLATE_AMD_* status */
#define LDA_OK_TRY(expr)                                                     \
	do {                                                                 \
		int rc_ = (expr);                                            \
		if (rc_ != LIBDEFLATE_AMD_OK)                                \
			return rc_;                                          \
	} while (0)
/* ... in a function that says "not done here" with false */
#define LDA_TRY(expr) LDA_HIP_TRY(expr, false)

struct DeviceCtx {
	int device = -1;
	int num_cus = 0;
	uint32_t *d_crc_tables = nullptr;	/* 17*256 words */
	uint32_t *d_crc_xpow8 = nullptr;	/* 1024 words */
	/* staging area used by the host-pointer entry points */
	std::mutex stage_mu;
	void *d_stage = nullptr;
	size_t stage_cap = 0;
	/* the kernels' dynamic-LDS limits are raised once per device (setting
	 * them again is harmless, so a race between two first calls only repeats
	 * it); part of the context so that no table is indexed by a device id */
	std::atomic<bool> deflate_attr_set{false}, inflate_attr_set{false}, stream_attr_set{false};
	/* waves per CU the size query's kernel fits (host_sizes.hip; 0: not asked yet) */
	std::atomic<int> sizes_waves_fit{0};
};

/* context of the calling thread's current device; nullptr (+error) if none */
DeviceCtx *device_ctx();
/* the hardware self-check on the current device (selfcheck_kernels.hip):
 * out[0..4] = lanes, order mismatches, conflicts seen, loads, stale loads;
 * true = the device behaves as the kernels need */
bool device_selfcheck(int num_cus, uint64_t out[5]);

/*
 * An object belongs to the device that was current when it was allocated (its
 * scratch, staging and streams live there).  Every entry point that takes an
 * object makes that device current for its duration and puts the caller's
 * back: a caller that drives several GPUs from one thread - or calls with
 * another device current - launches where the object's memory is, not where
 * the thread happens to point (libdeflate.h has no notion of a device: the
 * drop-in must not grow one).  ok() == false: the device could not be made
 * current (the reason is in libdeflate_amd_last_error()).
 */
struct DeviceGuard {
	int prev = -1;
	bool switched = false, good = true;
	explicit DeviceGuard(int device);
	~DeviceGuard();
	bool ok() const { return good; }
	DeviceGuard(const DeviceGuard &) = delete;
	DeviceGuard &operator=(const DeviceGuard &) = delete;
};

/* the environment switches (tuning aids), read ONCE per
 * process at the first use - not per call */
struct EnvCfg {
	bool no_small = false;		/* LDA_NO_SMALL */
	bool no_segments = false;	/* LDA_NO_SEGMENTS */
	int inflate_lpw = 0;		/* LDA_INFLATE_LPW (0 = automatic) */
	bool inflate_par = true;	/* LDA_INFLATE_PAR */
	int inflate_waves_per_cu = 16;	/* LDA_INFLATE_WAVES_PER_CU */
	int sizes_waves_per_cu = 0;	/* LDA_SIZES_WAVES_PER_CU: the size query's (0 = what its registers and LDS allow) */
	int host_threads = 4;		/* LDA_HOST_THREADS: packing threads of the host-pointer batches */
	size_t seg_bytes = 0;		/* LDA_SEG_BYTES: sub-range of the segmented single-buffer compress (0 = by size) */
	bool no_stream_par = false;	/* LDA_NO_STREAM_PAR: single streams stay on one wave */
	size_t stream_par_min = 16384;	/* LDA_STREAM_PAR_MIN: smallest stream (bytes in) for the many-wave path */
	/* LDA_ZIP_LARGE_MIN: smallest deflated ZIP entry (csize) that
	 * libdeflate_amd_zip_read_large hands to the many-wave decoder when its
	 * large_min is 0.  Measured: the smallest value within the spread of the
	 * best in the sweep of tools/bench_zip_large.py
	 * (profiles/zip_large_bench.json: 32 KiB to 4 MiB lie within 0.15 ms of
	 * each other there, 16 KiB - every 64 KiB entry a blocking call of
	 * 0.62 ms - costs 2.5 s) */
	size_t zip_large_min = (size_t)128 << 10;
	size_t stream_window = 0;	/* LDA_STREAM_WINDOW: first input window of that path (0 = 4 MiB) */
	size_t stream_chunk = 0;	/* LDA_STREAM_CHUNK: input bytes per chunk of that path (0 = by size) */
	int devices = 1;		/* LDA_DEVICES: GPUs a host-pointer batch is spread over (N, or "all" = -1) */
	bool no_selfcheck = false;	/* LDA_NO_SELFCHECK: skip the per-device hardware self-check */
	bool bgzf_serial = false;	/* LDA_BGZF_SERIAL: the BGZF reader finds the members by the serial walk */
	bool tar_serial = false;	/* LDA_TAR_SERIAL: the tar reader finds the records by the serial walk */
	bool fanout_oversub = false;	/* LDA_FANOUT_OVERSUB: more shards than visible devices (a test aid: several shards share a GPU) */
	bool compress_overlap = true;	/* LDA_COMPRESS_OVERLAP: 0 = the split path's kernels in series on the caller's stream */
	bool compress_specialize = true;	/* LDA_COMPRESS_SPECIALIZE: 0 = the split path's LZ77 stage is the generic kernel at every level */
	int compress_tail_rounds = 0;	/* LDA_COMPRESS_TAIL_ROUNDS: buffers per CU of a slice's tail (0 = compress_plan.h's) */
};
const EnvCfg &env_cfg();

/* grow-only device staging; caller holds ctx->stage_mu */
void *stage_reserve(DeviceCtx *ctx, size_t nbytes);

/* abort with a message: ONLY where the reference API has no error channel
 * (libdeflate_crc32 / libdeflate_adler32); prints the real HIP error */
[[noreturn]] void die(const char *what);

/* a failure inside a single-buffer libdeflate_* call that does have an error
 * return: one line on stderr (the error is also in libdeflate_amd_last_error) */
void complain(const char *what, int status);

/*
 * Two pinned host buffers the host-pointer batch entry points pack into /
 * unpack from while the other one is in flight: a batch crosses PCIe as a few
 * large DMA transfers instead of one blocking copy per chunk.
 */
struct PinnedPair {
	uint8_t *buf[2] = { nullptr, nullptr };
	hipEvent_t ev[2] = { nullptr, nullptr };
	size_t cap = 0;
	/* grow-only, sized to what the batch needs (a call on a few KiB pins a
	 * few KiB: 64 KiB at least, LDA_PINNED_SLICE at most per buffer); false
	 * + error if pinned memory is unavailable */
	bool ensure(size_t want);
	void release();
};
/* a small grow-only pinned buffer: what a batch reads back per chunk (sizes,
 * offsets, result codes).  An asynchronous copy to pageable memory is staged
 * by the runtime and blocks the host until the stream gets there; to pinned
 * memory it is a real asynchronous copy and the host looks after the event */
struct PinnedBuf {
	void *p = nullptr;
	size_t cap = 0;
	void *ensure(size_t want);	/* nullptr + error on failure */
	void release();
};
/*
 * Host arrays on their way to an object's device scratch, through a pinned
 * block in one asynchronous copy.  The block of the last call may still be on
 * its way up, so begin() waits for the event behind that copy (and makes the
 * event on first use); the caller then reserves its device scratch, fills
 * pinned(bytes) and hands it to send().
 */
struct Upload {
	PinnedBuf desc;
	hipEvent_t up = nullptr;
	int begin();					/* OK or NO_DEVICE */
	void *pinned(size_t bytes) { return desc.ensure(bytes < 64 ? 64 : bytes); }	/* nullptr + error on failure */
	int send(void *d_dst, size_t bytes, hipStream_t st);	/* OK or NO_DEVICE */
	void release();
};
#define LDA_PINNED_SLICE ((size_t)32 << 20)
#define LDA_PINNED_MIN ((size_t)64 << 10)

/*
 * Two streams of an object for its host-pointer batch entry points: the batch
 * goes through in slices, the transfers of a slice on `copy`, its kernels on
 * `comp`, so that the kernels of slice k run while the host packs and sends
 * slice k + 1 and unpacks slice k - 1.
 */
struct StreamPair {
	hipStream_t copy = nullptr, comp = nullptr;
	hipEvent_t mark = nullptr;	/* a point on `comp` that `copy` may wait for */
	hipEvent_t mark2 = nullptr;	/* and one on `copy` that `comp` may wait for */
	bool ensure();
	/* ensure(), for a call that takes no stream of the caller's (the
	 * host-pointer entry points): the streams are not ordered behind anything,
	 * and batches the caller has queued on a stream of their own may still use
	 * the object's scratch, which such a call is about to reserve and reuse.
	 * The call blocks anyway, so it waits here, on the host, until the device
	 * has nothing in flight.  (The blocking calls that do take a stream wait
	 * for it with an event instead: decompress_large_body().) */
	bool enter();
	void release();
};

/*
 * The stream of a compressor that the tail of a split compress launch runs on
 * beside its head on the caller's stream (compress_batch_impl()), and the two
 * events that order them: `in` on the caller's stream, which the tail waits
 * for, `tail` behind the tail, which the caller's stream waits for.  Made on
 * first use; where that fails once, the object keeps the serial schedule.
 */
struct SideStream {
	hipStream_t side = nullptr;
	hipEvent_t in = nullptr, tail = nullptr;
	bool failed = false;
	bool ensure();
	void release();
};

/*
 * The slice pipeline of the host-pointer calls, on an object's StreamPair.
 * For k = 0 .. ns - 1, enqueue(k) sends slice k on `copy` and returns once
 * its bytes are on the device, then queues the slice's kernels and its
 * read-backs into pinned memory on `comp`.  The runner records slice k's
 * event on `comp`; for k > 0 it waits for slice k - 1's event and calls
 * drain(k - 1), which hands the read-backs to the caller and brings the
 * slice's output back on `copy`, returning once it is on the host.  The last
 * slice is drained after the loop.  So drain(k - 1) has returned before
 * enqueue(k + 1) starts: a staging area that slices k - 1 and k + 1 share is
 * free again when slice k + 1 is sent into it.
 *
 * The run stops at the first status of either callback that is not
 * LIBDEFLATE_AMD_OK and returns it; a drain returns SLICES_STOP to end the
 * run without an error (the output does not fit).  A failed event call sets
 * the error "<what>: <HIP error>" and returns LIBDEFLATE_AMD_NO_DEVICE.
 * However it returns (an exception included), both streams are synchronised
 * and the events destroyed.
 */
enum { SLICES_STOP = 1 };
int run_slices(const char *what, const StreamPair &sp, size_t ns,
	       const std::function<int(size_t)> &enqueue, const std::function<int(size_t)> &drain);

/* cut n chunks into at most `max_slices` consecutive slices of about equal
 * byte counts (each at least `min_bytes`, as far as the total allows);
 * bounds[0..k] with bounds[0] = 0, bounds[k] = n; returns k >= 1 */
size_t slice_by_bytes(size_t n, const size_t *nbytes, size_t max_slices,
		      size_t min_bytes, size_t *bounds);

/* host chunks -> device, packed at d_base + off[i] (off ascending); blocking
 * only on its own pinned buffers */
int copy_in_packed(PinnedPair *pp, uint8_t *d_base, size_t n,
		   const void *const *in, const size_t *in_nbytes,
		   const uint64_t *off, hipStream_t st);
/* device bytes at d_base + off[i] (off ascending) -> out[i], nbytes[i] each
 * (0 = skip); the stream must already hold the work that produces them */
int copy_out_packed(PinnedPair *pp, const uint8_t *d_base, size_t n,
		    void *const *out, const uint64_t *nbytes,
		    const uint64_t *off, hipStream_t st);

/* one contiguous host range <-> device range, in pieces the copy threads share
 * (`piece` bytes each; 0: sixteen to a slice, see host_context.hip) */
int span_in(PinnedPair *pp, uint8_t *d_base, uint64_t d_off, const uint8_t *src, size_t n,
	    hipStream_t st, size_t piece = 0);
int span_out(PinnedPair *pp, const uint8_t *d_base, uint64_t d_off, uint8_t *dst, size_t n,
	     hipStream_t st, size_t piece = 0);

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* carves arrays out of one device allocation; p == NULL only sizes it */
struct Carve {
	uint8_t *p;
	size_t at = 0;
	explicit Carve(void *base) : p((uint8_t *)base) {}
	template <typename T> T *take(size_t count, size_t align = 16)
	{
		at = align_up(at, align);
		T *r = p ? (T *)(p + at) : nullptr;
		at += count * sizeof(T);
		return r;
	}
};

/* host_compact.hip: the exclusive prefix sum of n sizes on `st`, in blocks of
 * LDA_SCAN_BLOCK: the place of size i is offsets[i] + block_sums[i /
 * LDA_SCAN_BLOCK], and the total is at block_sums + the block count, which
 * scan_enqueue() returns (block_sums: scan_blocks(n) + 1 words).  n == 0
 * writes the total alone */
size_t scan_blocks(size_t n);
size_t scan_enqueue(hipStream_t st, size_t n, const uint64_t *sizes, uint64_t *offsets,
		    uint64_t *block_sums);

/*
 * Nothing may unwind through an extern "C" entry point: the reference is C and
 * its callers have no handlers, an exception that reaches them ends the
 * process.  The entry points whose bodies use the standard library's
 * containers or threads run them through this: a failed host allocation
 * becomes the call's failure value, with the reason in
 * libdeflate_amd_last_error().
 */
template <typename R, typename F> static inline R no_unwind(const char *what, R failed, F body)
{
	try {
		return body();
	} catch (const std::exception &e) {
		set_error("%s: %s", what, e.what());
	} catch (...) {
		set_error("%s: exception", what);
	}
	return failed;
}

/* checksum of A || B from the checksums of A and B and the length of B
 * (host_compress.hip) */
uint32_t crc32_concat(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* the same with x^(8 len_b) mod P computed once for many pieces of one length */
uint32_t crc32_shift(uint64_t len);
uint32_t crc32_concat_shift(uint32_t crc_a, uint32_t crc_b, uint32_t shift_b);
uint32_t adler32_concat(uint32_t ad_a, uint32_t ad_b, uint64_t len_b);

} /* namespace lda */

#endif /* LDA_HOST_COMMON_H */
