/*
 * host_bgzf.hip - C-ABI of BGZF files (SAM/BAM spec 4.1; include/libdeflate_amd.h).
 *
 * One buffer is cut into blocks of LIBDEFLATE_AMD_BGZF_BLOCK bytes, the
 * blocks run as ONE compress batch of format LIBDEFLATE_AMD_BGZF (a member
 * per block, in a slot of LIBDEFLATE_AMD_BGZF_MEMBER_MAX bytes each), and the
 * kernels of compact_kernels.hip pack the members, append the EOF member and
 * write the size and the index.  Everything is enqueued; nothing waits for
 * the device.  The host form runs the same calls over slices of its input.
 */
#include <string.h>
#include <algorithm>

#include "host_objects.h"
#include "kernels.h"

using namespace lda;

#define BGZF_BLOCK ((size_t)LIBDEFLATE_AMD_BGZF_BLOCK)
#define BGZF_MEMBER_MAX ((size_t)LIBDEFLATE_AMD_BGZF_MEMBER_MAX)
#define BGZF_EOF ((size_t)LIBDEFLATE_AMD_BGZF_EOF_BYTES)
/* the smallest member: 18 bytes of header, 8 of trailer, a byte of deflate */
#define BGZF_MIN_MEMBER 27

static const uint8_t k_bgzf_eof[BGZF_EOF] = {
	0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
	0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
};

static size_t bgzf_members(size_t n)
{
	return (n + BGZF_BLOCK - 1) / BGZF_BLOCK;
}

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_bgzf_compress_bound(struct libdeflate_compressor *c, size_t n)
{
	(void)c;
	return bgzf_members(n) * BGZF_MEMBER_MAX + BGZF_EOF;
}

/* what every entry point checks before it touches a device */
static bool bgzf_args_ok(const char *what, const struct libdeflate_compressor *c,
			 const void *in, size_t n, const void *out, size_t out_avail,
			 const void *out_nbytes, unsigned flags)
{
	if (!c || (!in && n) || !out || !out_nbytes) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (flags & ~(unsigned)LIBDEFLATE_AMD_BGZF_NO_EOF) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return false;
	}
	const size_t m = bgzf_members(n);
	const size_t eof = flags & LIBDEFLATE_AMD_BGZF_NO_EOF ? 0 : BGZF_EOF;
	if (out_avail < m * BGZF_MIN_MEMBER + eof) {
		set_error("%s: out_avail %zu cannot hold %zu members%s", what, out_avail, m,
			  eof ? " and the EOF member" : "");
		return false;
	}
	return true;
}

/* the object's BGZF scratch for m blocks: [in_off in_n slot_off slot_avail
 * sizes: u64 x m each][scan offsets: compact_offsets_len(m)][slots] */
static size_t bgzf_slots_at(size_t m)
{
	return align_up((5 * m + libdeflate_amd_compact_offsets_len(m)) * 8, 256);
}

static size_t bgzf_scratch_bytes(size_t m)
{
	return bgzf_slots_at(m) + m * BGZF_MEMBER_MAX;
}

static int bgzf_enqueue(struct libdeflate_compressor *c, const uint8_t *d_in, size_t n,
			uint8_t *d_out, size_t out_avail, uint64_t *d_out_nbytes,
			uint64_t *d_index, unsigned flags, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t m = bgzf_members(n);
	const uint32_t eof = flags & LIBDEFLATE_AMD_BGZF_NO_EOF ? 0 : (uint32_t)BGZF_EOF;
	const uint64_t *sizes = NULL, *total_at = NULL;
	if (m) {
		uint8_t *ws = (uint8_t *)c->bgzf.reserve(bgzf_scratch_bytes(m));
		if (!ws)
			return LIBDEFLATE_AMD_OOM;
		uint64_t *in_off = (uint64_t *)ws, *in_n = in_off + m, *slot_off = in_off + 2 * m,
			 *slot_av = in_off + 3 * m, *out_n = in_off + 4 * m, *cmp = in_off + 5 * m;
		uint8_t *slots = ws + bgzf_slots_at(m);
		hipLaunchKernelGGL(lda_bgzf_desc_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256),
				   0, st, (uint64_t)m, (uint64_t)n, in_off, in_n, slot_off, slot_av);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		/* the bound: large files take the split path, small ones the
		 * fused kernel (compress_batch_impl() decides) */
		int rc = libdeflate_amd_compress_batch_bounded(c, LIBDEFLATE_AMD_BGZF, m, d_in, in_off,
							       in_n, slots, slot_off, slot_av, out_n,
							       BGZF_BLOCK, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
		/* the scans of libdeflate_amd_compact_batch(), then a copy that
		 * writes nothing unless the whole file fits */
		uint64_t *block_sums = cmp + m + 1;
		const size_t nblocks = scan_enqueue(st, m, out_n, cmp, block_sums);
		const size_t grid = std::min(m, (size_t)ctx->num_cus * 8);
		hipLaunchKernelGGL(lda_bgzf_copy_kernel, dim3((unsigned)grid), dim3(256), 0, st,
				   (uint64_t)m, (const uint8_t *)slots, (const uint64_t *)out_n,
				   (const uint64_t *)cmp, (const uint64_t *)block_sums, d_out,
				   (uint64_t)out_avail, eof, d_index);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		sizes = out_n;
		total_at = block_sums + nblocks;
	}
	hipLaunchKernelGGL(lda_bgzf_finalize_kernel, dim3(1), dim3(256), 0, st, (uint64_t)m,
			   (uint64_t)n, sizes, total_at, d_out, (uint64_t)out_avail, eof,
			   d_out_nbytes, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_bgzf_compress_batch(struct libdeflate_compressor *c, const void *d_in,
				   size_t in_nbytes, void *d_out, size_t out_avail,
				   uint64_t *d_out_nbytes, uint64_t *d_index, unsigned flags,
				   void *stream)
{
	if (!bgzf_args_ok("bgzf_compress_batch", c, d_in, in_nbytes, d_out, out_avail,
			  d_out_nbytes, flags))
		return LIBDEFLATE_AMD_BAD_ARG;
	DeviceGuard on(c->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return bgzf_enqueue(c, (const uint8_t *)d_in, in_nbytes, (uint8_t *)d_out, out_avail,
			    d_out_nbytes, d_index, flags, (hipStream_t)stream);
}

/*
 * Host memory: the blocks go through in slices of 8 per CU, twice what the
 * split path asks for (LDA_SPLIT_MIN_PER_CU in host_compress.hip), so every
 * slice but a short last one takes it; each slice is a file of its own
 * without the EOF member (bgzf_enqueue() with NO_EOF), since the members are
 * independent the slices' files concatenate into the whole one.  On
 * run_slices(): while the kernels of slice k run on the compute stream, the
 * host sends slice k + 1 and brings back slice k - 1 (two input and two
 * output areas alternate).  Nothing is primed and no checksum is stitched.
 */
static size_t bgzf_host(struct libdeflate_compressor *c, const uint8_t *in, size_t n,
			uint8_t *out, size_t out_avail, uint64_t *index, unsigned flags)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx || !c->streams.enter()) {
		complain("libdeflate_amd_bgzf_compress", LIBDEFLATE_AMD_NO_DEVICE);
		return 0;
	}
	const size_t m = bgzf_members(n);
	const size_t eof = flags & LIBDEFLATE_AMD_BGZF_NO_EOF ? 0 : BGZF_EOF;
	const size_t per = std::min(m, (size_t)8 * ctx->num_cus);
	const size_t ns = per ? (m + per - 1) / per : 0;
	size_t total = 0;	/* bytes of the file so far */
	if (ns) {
		/* device layout: [meta of 2 slices: size, index pairs (u64)]
		 * [input of 2 slices][members of 2 slices] */
		const size_t meta_words = 1 + 2 * (per + 1);
		const size_t in_cap = align_up(std::min(n, per * BGZF_BLOCK), 64);
		const size_t out_cap = align_up(per * BGZF_MEMBER_MAX, 64);
		const size_t in_at = align_up(2 * meta_words * 8, 64), out_at = in_at + 2 * in_cap;
		uint8_t *st = (uint8_t *)c->stage.reserve(out_at + 2 * out_cap);
		uint64_t *h_meta = (uint64_t *)c->meta.ensure(2 * meta_words * 8);
		if (!st || !h_meta || !c->bgzf.reserve(bgzf_scratch_bytes(per))) {
			complain("libdeflate_amd_bgzf_compress (memory)", LIBDEFLATE_AMD_OOM);
			return 0;
		}
		hipStream_t s_copy = c->streams.copy, s_comp = c->streams.comp;
		const size_t piece = ns > 1 ? (size_t)1 << 20 : 0;
		/* slice k uses the areas k & 1: run_slices() has drained slice
		 * k - 2 before it sends slice k */
		auto enqueue = [&](size_t k) -> int {
			const size_t lo = k * per, mk = std::min(per, m - lo);
			const size_t a = lo * BGZF_BLOCK, b = std::min(n, (lo + mk) * BGZF_BLOCK);
			uint64_t *d_meta = (uint64_t *)st + (k & 1) * meta_words;
			/* (returns when the slice is on the device) */
			if (span_in(&c->pinned, st, in_at + (k & 1) * in_cap, in + a, b - a, s_copy,
				    piece) != LIBDEFLATE_AMD_OK ||
			    bgzf_enqueue(c, st + in_at + (k & 1) * in_cap, b - a,
					 st + out_at + (k & 1) * out_cap, mk * BGZF_MEMBER_MAX, d_meta,
					 index ? d_meta + 1 : NULL, LIBDEFLATE_AMD_BGZF_NO_EOF,
					 s_comp) != LIBDEFLATE_AMD_OK ||
			    hipMemcpyAsync(h_meta + (k & 1) * meta_words, d_meta,
					   (index ? 1 + 2 * mk : 1) * 8, hipMemcpyDeviceToHost,
					   s_comp) != hipSuccess)
				return LIBDEFLATE_AMD_NO_DEVICE;
			return LIBDEFLATE_AMD_OK;
		};
		auto drain = [&](size_t k) -> int {
			const size_t lo = k * per, mk = std::min(per, m - lo);
			const uint64_t *h = h_meta + (k & 1) * meta_words;
			const size_t tk = (size_t)h[0];
			if (!tk || total + tk > out_avail - eof) {
				if (!tk)
					set_error("libdeflate_amd_bgzf_compress: a member did not fit");
				return SLICES_STOP;
			}
			if (span_out(&c->pinned, st, out_at + (k & 1) * out_cap, out + total, tk, s_copy,
				     piece) != LIBDEFLATE_AMD_OK)
				return LIBDEFLATE_AMD_NO_DEVICE;
			if (index)
				for (size_t j = 0; j < mk; j++) {
					index[2 * (lo + j)] = total + h[1 + 2 * j];
					index[2 * (lo + j) + 1] = lo * BGZF_BLOCK + h[2 + 2 * j];
				}
			total += tk;
			return LIBDEFLATE_AMD_OK;
		};
		const int rc = run_slices("libdeflate_amd_bgzf_compress", c->streams, ns, enqueue, drain);
		if (rc == SLICES_STOP)
			return 0;
		if (rc != LIBDEFLATE_AMD_OK) {
			hipError_t e = hipGetLastError();
			if (e != hipSuccess)
				set_error("libdeflate_amd_bgzf_compress: %s", hipGetErrorString(e));
			complain("libdeflate_amd_bgzf_compress", LIBDEFLATE_AMD_NO_DEVICE);
			return 0;
		}
	}
	memcpy(out + total, k_bgzf_eof, eof);
	if (index) {
		index[2 * m] = total;
		index[2 * m + 1] = n;
	}
	return total + eof;
}

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_bgzf_compress(struct libdeflate_compressor *c, const void *in, size_t in_nbytes,
			     void *out, size_t out_avail, uint64_t *index, size_t index_avail,
			     unsigned flags)
{
	const char *what = "libdeflate_amd_bgzf_compress";
	if (!bgzf_args_ok(what, c, in, in_nbytes, out, out_avail, out, flags))
		return 0;
	const size_t m = bgzf_members(in_nbytes);
	if (index && index_avail < 2 * (m + 1)) {
		set_error("%s: index_avail %zu < 2 (m + 1) = %zu", what, index_avail, 2 * (m + 1));
		return 0;
	}
	DeviceGuard on(c->device);
	if (!on.ok()) {
		complain(what, LIBDEFLATE_AMD_NO_DEVICE);
		return 0;
	}
	return no_unwind(what, (size_t)0, [&]() {
		return bgzf_host(c, (const uint8_t *)in, in_nbytes, (uint8_t *)out, out_avail,
				 index, flags);
	});
}
