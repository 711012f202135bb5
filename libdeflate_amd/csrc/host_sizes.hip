/*
 * host_sizes.hip - C-ABI of the size query (inflate_sizes.hip) and of the
 * packed batch decompress built on it:
 *
 *   libdeflate_amd_decompress_sizes_batch[_dict]  device arrays, enqueue only
 *   libdeflate_amd_decompress_sizes_batch_host    host pointers: the shared
 *                                                 slice pipeline and fan-out
 *   libdeflate_amd_decompress_batch_packed        sizes -> scan -> decode into
 *                                                 place, enqueue only
 *
 * The reference's callers learn a stream's size by decoding it into a guess
 * and doubling on LIBDEFLATE_INSUFFICIENT_SPACE (programs/gzip.c:236-299); on
 * a device batch that is a host round trip per attempt.  Here the sizes are
 * counted by the decoder itself with nothing written, and the packed call
 * places and decodes the streams behind the count on the same stream.
 */
#include <vector>

#include "host_objects.h"
#include "kernels.h"

using namespace lda;

static bool format_takes_sizes(int format)
{
	return format >= LIBDEFLATE_AMD_DEFLATE && format <= LIBDEFLATE_AMD_GZIP;
}

/* waves (= streams in flight) per CU: what the kernel's registers (512 per
 * SIMD lane, in steps of 8) and its LDS leave room for; LDA_SIZES_WAVES_PER_CU
 * lowers it */
static size_t sizes_waves_per_cu(DeviceCtx *c)
{
	int fit = c->sizes_waves_fit.load(std::memory_order_acquire);

	if (!fit) {
		hipFuncAttributes a;
		size_t per_simd = 4;
		if (hipFuncGetAttributes(&a, (const void *)lda_inflate_sizes_kernel) == hipSuccess &&
		    a.numRegs > 0) {
			per_simd = 512 / (((size_t)a.numRegs + 7) & ~(size_t)7);
			if (per_simd > 8)
				per_simd = 8;
			if (per_simd < 1)
				per_simd = 1;
		}
		const size_t by_lds = 163840 / lda_inflate_sizes_lds_bytes();
		fit = (int)(4 * per_simd < by_lds ? 4 * per_simd : by_lds);
		c->sizes_waves_fit.store(fit, std::memory_order_release);
	}
	const size_t want = (size_t)env_cfg().sizes_waves_per_cu;
	return want && want < (size_t)fit ? want : (size_t)fit;
}

/* for the build's checks (tests/test_sizes_abi.py), not part of the interface:
 * LDS bytes per wave of the size query's kernel and of the decode's */
extern "C" __attribute__((visibility("default"))) void lda_sizes_lds_report(size_t out[2])
{
	out[0] = lda_inflate_sizes_lds_bytes();
	out[1] = lda_inflate_lds_per_stream() + lda_inflate_lds_shared() + lda_inflate_window_bytes();
}

/* scratch of one size query: [counter 16][order u32 x n][dictionary block] */
size_t lda::sizes_scratch_bytes(size_t n)
{
	return align_up(16 + 4 * n, 64) + LDA_DICT_BLK_HDR;
}

/* arguments checked by the callers; s: sizes_scratch_bytes(n) of device memory */
int lda::sizes_enqueue(DeviceCtx *c, uint8_t *s, int format, size_t n, const void *d_in,
		       const uint64_t *d_in_offsets, const uint64_t *d_in_nbytes,
		       const uint64_t *d_out_limit, int32_t *d_results, uint64_t *d_actual_in,
		       uint64_t *d_out_nbytes, hipStream_t st, const void *d_dict,
		       size_t dict_nbytes)
{
	uint32_t *next = (uint32_t *)s, *order = NULL, *dict_id = NULL;
	uint32_t dlen = 0;

	if (d_dict && dict_nbytes) {
		/* only the dictionary's length matters to a count, and for zlib its
		 * Adler-32 (the DICTID the stream names), computed on the device */
		dlen = (uint32_t)(dict_nbytes < 32768 ? dict_nbytes : 32768);
		if (format == LIBDEFLATE_AMD_ZLIB) {
			uint8_t *blk = s + align_up(16 + 4 * n, 64);
			hipLaunchKernelGGL(lda_dict_prep_kernel, dim3(1), dim3(64), 0, st,
					   (const uint8_t *)d_dict, (uint64_t)dict_nbytes, 0u, 0u, 0u, blk);
			LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
			dict_id = (uint32_t *)(blk + 4);
			int rc = libdeflate_amd_adler32_batch(1, d_dict, (const uint64_t *)(blk + 16),
							      (const uint64_t *)(blk + 24), NULL, dict_id,
							      (void *)st);
			if (rc != LIBDEFLATE_AMD_OK)
				return rc;
		}
	}
	const size_t grid_max = (size_t)c->num_cus * sizes_waves_per_cu(c);
	const size_t grid = grid_max < n ? grid_max : n;
	LDA_HIP_TRY(hipMemsetAsync(next, 0, 16, st), LIBDEFLATE_AMD_NO_DEVICE);
	/* more streams than wave slots: costliest (longest input) first, as in
	 * the decode batch */
	if (n > grid && n < 0xFFFFFFFFull) {
		order = (uint32_t *)(s + 16);
		hipLaunchKernelGGL(lda_inflate_order_kernel, dim3(1), dim3(1024), 0, st,
				   (uint64_t)n, d_in_nbytes, (const uint64_t *)NULL, order);
	}
	hipLaunchKernelGGL(lda_inflate_sizes_kernel, dim3((unsigned)grid), dim3(64),
			   lda_inflate_sizes_lds_bytes(), st, (uint64_t)n, format,
			   env_cfg().inflate_par ? 1u : 0u, next, (const uint32_t *)order,
			   (const uint8_t *)d_in, d_in_offsets, d_in_nbytes, d_out_limit, d_results,
			   d_actual_in, d_out_nbytes, dlen, (const uint32_t *)dict_id);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int sizes_batch_impl(const char *what, struct libdeflate_decompressor *d, int format,
			    size_t n, const void *d_in, const uint64_t *d_in_offsets,
			    const uint64_t *d_in_nbytes, const uint64_t *d_out_limit,
			    int32_t *d_results, uint64_t *d_actual_in, uint64_t *d_out_nbytes,
			    void *stream, const void *d_dict, size_t dict_nbytes)
{
	if (!d || !format_takes_sizes(format)) {
		set_error("%s: bad argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (n == 0)
		return LIBDEFLATE_AMD_OK;
	if (!d_in || !d_in_offsets || !d_in_nbytes || !d_results || !d_out_nbytes) {
		set_error("%s: bad argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *c = device_ctx();
	if (!c)
		return LIBDEFLATE_AMD_NO_DEVICE;
	uint8_t *s = (uint8_t *)d->scratch.reserve(sizes_scratch_bytes(n));
	if (!s)
		return LIBDEFLATE_AMD_OOM;
	return sizes_enqueue(c, s, format, n, d_in, d_in_offsets, d_in_nbytes, d_out_limit,
			     d_results, d_actual_in, d_out_nbytes, (hipStream_t)stream, d_dict,
			     dict_nbytes);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch(struct libdeflate_decompressor *d, int format,
				      size_t n, const void *d_in,
				      const uint64_t *d_in_offsets,
				      const uint64_t *d_in_nbytes,
				      const uint64_t *d_out_limit, int32_t *d_results,
				      uint64_t *d_actual_in, uint64_t *d_out_nbytes,
				      void *stream)
{
	return sizes_batch_impl("decompress_sizes_batch", d, format, n, d_in, d_in_offsets,
				d_in_nbytes, d_out_limit, d_results, d_actual_in, d_out_nbytes,
				stream, NULL, 0);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch_dict(struct libdeflate_decompressor *d, int format,
					   size_t n, const void *d_dict, size_t dict_nbytes,
					   const void *d_in, const uint64_t *d_in_offsets,
					   const uint64_t *d_in_nbytes,
					   const uint64_t *d_out_limit, int32_t *d_results,
					   uint64_t *d_actual_in, uint64_t *d_out_nbytes,
					   void *stream)
{
	/* zlib refuses a dictionary on a gzip stream */
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB) {
		set_error("decompress_sizes_batch_dict: format %d takes no dictionary", format);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (dict_nbytes && !d_dict) {
		set_error("decompress_sizes_batch_dict: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return sizes_batch_impl("decompress_sizes_batch_dict", d, format, n, d_in, d_in_offsets,
				d_in_nbytes, d_out_limit, d_results, d_actual_in, d_out_nbytes,
				stream, d_dict, dict_nbytes);
}

/*
 * Host pointers.  Slices on run_slices() like the decode's host form, but only
 * inputs go up and three small arrays come back.  Staging: [in_off in_n limit
 * ain size: u64 x n each][results s32 x n][inputs].
 */
static int sizes_batch_host_body(struct libdeflate_decompressor *d, int format, size_t n,
				 const void *const *in, const size_t *in_nbytes,
				 const size_t *out_limit, int32_t *results, size_t *actual_in,
				 size_t *out_nbytes)
{
	DeviceGuard on(d->device);
	if (!on.ok() || !device_ctx())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *c = device_ctx();
	enum { MAX_SLICES = 8 };
	size_t bounds[MAX_SLICES + 1];
	/* (slices of at least 16 MiB of input: some thousand streams of the
	 * benchmark's shape, a grid-full of waves) */
	const size_t ns = slice_by_bytes(n, in_nbytes, MAX_SLICES, (size_t)16 << 20, bounds);
	std::vector<uint64_t> desc(3 * n);
	uint64_t *in_off = &desc[0], *in_n = &desc[n], *lim = &desc[2 * n];
	size_t pos = align_up(5 * n * 8 + n * 4, 64);
	for (size_t i = 0; i < n; i++) {
		in_off[i] = pos;
		in_n[i] = in_nbytes[i];
		lim[i] = out_limit ? out_limit[i] : LIBDEFLATE_AMD_SIZE_LIMIT_MAX;
		pos = align_up(pos + in_nbytes[i] + 16, 16);
	}
	uint8_t *st = (uint8_t *)d->stage.reserve(pos + 64);
	if (!st)
		return LIBDEFLATE_AMD_OOM;
	if (!d->streams.enter())
		return LIBDEFLATE_AMD_NO_DEVICE;
	uint8_t *scr = (uint8_t *)d->scratch.reserve(sizes_scratch_bytes(n));
	if (!scr)
		return LIBDEFLATE_AMD_OOM;
	uint64_t *h_back = (uint64_t *)d->meta.ensure(n * (8 + 8 + 4));
	if (!h_back)
		return LIBDEFLATE_AMD_OOM;
	uint64_t *h_ain = h_back, *h_size = h_back + n;
	int32_t *h_res = (int32_t *)(h_back + 2 * n);
	hipStream_t s_copy = d->streams.copy, s_comp = d->streams.comp;
	LDA_HIP_TRY(hipMemcpyAsync(st, desc.data(), 3 * n * 8, hipMemcpyHostToDevice, s_copy),
		    LIBDEFLATE_AMD_NO_DEVICE);
	uint64_t *d_desc = (uint64_t *)st;
	int32_t *d_res = (int32_t *)(st + 5 * n * 8);
	auto enqueue = [&](size_t k) -> int {
		const size_t lo = bounds[k], nk = bounds[k + 1] - lo;
		int rc = copy_in_packed(&d->pinned, st, nk, in + lo, in_nbytes + lo, in_off + lo, s_copy);
		if (rc == LIBDEFLATE_AMD_OK)
			rc = sizes_enqueue(c, scr, format, nk, st, d_desc + lo, d_desc + n + lo,
					   d_desc + 2 * n + lo, d_res + lo, d_desc + 3 * n + lo,
					   d_desc + 4 * n + lo, s_comp, NULL, 0);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
		if (hipMemcpyAsync(h_ain + lo, d_desc + 3 * n + lo, nk * 8, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess ||
		    hipMemcpyAsync(h_size + lo, d_desc + 4 * n + lo, nk * 8, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess ||
		    hipMemcpyAsync(h_res + lo, d_res + lo, nk * 4, hipMemcpyDeviceToHost,
				   s_comp) != hipSuccess) {
			set_error("decompress_sizes_batch_host: %s", hipGetErrorString(hipGetLastError()));
			return LIBDEFLATE_AMD_NO_DEVICE;
		}
		return LIBDEFLATE_AMD_OK;
	};
	auto drain = [&](size_t k) -> int {
		for (size_t i = bounds[k]; i < bounds[k + 1]; i++) {
			results[i] = h_res[i];
			if (actual_in)
				actual_in[i] = h_ain[i];
			out_nbytes[i] = h_size[i];
		}
		return LIBDEFLATE_AMD_OK;
	};
	return run_slices("decompress_sizes_batch_host", d->streams, ns, enqueue, drain);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_sizes_batch_host(struct libdeflate_decompressor *d, int format,
					   size_t n, const void *const *in,
					   const size_t *in_nbytes, const size_t *out_limit,
					   int32_t *results, size_t *actual_in, size_t *out_nbytes)
{
	if (!d || !format_takes_sizes(format)) {
		set_error("decompress_sizes_batch_host: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (n == 0)
		return LIBDEFLATE_AMD_OK;
	if (!in || !in_nbytes || !results || !out_nbytes) {
		set_error("decompress_sizes_batch_host: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind("decompress_sizes_batch_host", (int)LIBDEFLATE_AMD_OOM, [&]() {
		auto body = [&](struct libdeflate_decompressor *o, size_t lo, size_t cnt) {
			return sizes_batch_host_body(o, format, cnt, in + lo, in_nbytes + lo,
						     out_limit ? out_limit + lo : NULL, results + lo,
						     actual_in ? actual_in + lo : NULL, out_nbytes + lo);
		};
		/* several GPUs (LDA_DEVICES): shards of about equal INPUT (what a
		 * stream costs to count) */
		return fanout<libdeflate_decompressor>(d, n, in_nbytes,
						       libdeflate_alloc_decompressor_ex, body);
	});
}

/*
 * Sizes, places, decode: nothing but enqueues.  Scratch of the object:
 * [what the decode batch and the size query use][verdict s32 x n][rounded
 * sizes u64 x n + 1][block sums of the scan][input lengths and room of the
 * decode: u64 x n each] - reserved in one piece before the first launch, so
 * that the decode's own reservation finds it large enough and moves nothing.
 */
extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_batch_packed(struct libdeflate_decompressor *d, int format,
				       size_t n, const void *d_in,
				       const uint64_t *d_in_offsets,
				       const uint64_t *d_in_nbytes, void *d_out,
				       size_t out_capacity, size_t out_align,
				       uint64_t *d_out_offsets, int32_t *d_results,
				       uint64_t *d_actual_in, uint64_t *d_actual_out,
				       void *stream)
{
	if (!d || !format_takes_sizes(format) || out_align == 0 || out_align > 256 ||
	    (out_align & (out_align - 1))) {
		set_error("decompress_batch_packed: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (n && (!d_in || !d_in_offsets || !d_in_nbytes || (!d_out && out_capacity) ||
		  !d_results || !d_actual_out)) {
		set_error("decompress_batch_packed: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!d_out_offsets) {
		set_error("decompress_batch_packed: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *c = device_ctx();
	hipStream_t st = (hipStream_t)stream;
	if (!c)
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (n == 0) {	/* the total of nothing */
		LDA_HIP_TRY(hipMemsetAsync(d_out_offsets, 0, 8, st), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	const size_t nblocks = scan_blocks(n + 1);
	size_t front = align_up(n * 4, 16) + 16 * n + 4 * n + 16;	/* decompress_batch */
	if (front < sizes_scratch_bytes(n))
		front = sizes_scratch_bytes(n);
	front = align_up(front, 64);
	const size_t verdict_at = front, rounded_at = verdict_at + align_up(4 * n, 64);
	const size_t sums_at = rounded_at + align_up(8 * (n + 1), 64);
	const size_t dec_in_at = sums_at + align_up(8 * (nblocks + 1), 64);
	const size_t dec_av_at = dec_in_at + align_up(8 * n, 64);
	uint8_t *s = (uint8_t *)d->scratch.reserve(dec_av_at + align_up(8 * n, 64));
	if (!s)
		return LIBDEFLATE_AMD_OOM;
	int32_t *verdict = (int32_t *)(s + verdict_at);
	uint64_t *rounded = (uint64_t *)(s + rounded_at), *block_sums = (uint64_t *)(s + sums_at);
	uint64_t *dec_in = (uint64_t *)(s + dec_in_at), *dec_av = (uint64_t *)(s + dec_av_at);

	/* 1. sizes with the maximum limit (into d_actual_out: the decode's own
	 *    figures replace them) */
	int rc = sizes_enqueue(c, s, format, n, d_in, d_in_offsets, d_in_nbytes, NULL, verdict,
			       NULL, d_actual_out, st, NULL, 0);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	/* 2. slots: exclusive prefix sum of the rounded sizes; entry n the total */
	const unsigned g1 = (unsigned)((n + 1 + 255) / 256);
	hipLaunchKernelGGL(lda_packed_round_kernel, dim3(g1), dim3(256), 0, st, (uint64_t)n,
			   (uint64_t)out_align - 1, (const uint64_t *)d_actual_out, rounded);
	scan_enqueue(st, n + 1, rounded, d_out_offsets, block_sums);
	hipLaunchKernelGGL(lda_packed_desc_kernel, dim3(g1), dim3(256), 0, st, (uint64_t)n,
			   (uint64_t)out_capacity, d_in_nbytes, (const uint64_t *)d_actual_out,
			   (const uint64_t *)block_sums, d_out_offsets, verdict, dec_in, dec_av);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	/* 3. decode into place, every check included; a stream without a slot
	 *    is an empty input there and gets its verdict back behind it */
	rc = libdeflate_amd_decompress_batch(d, format, n, d_in, d_in_offsets, dec_in,
					     d_out ? d_out : (void *)s, d_out_offsets, dec_av,
					     d_results, d_actual_in, d_actual_out, stream);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	hipLaunchKernelGGL(lda_packed_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256),
			   0, st, (uint64_t)n, (const int32_t *)verdict, d_results, d_actual_in,
			   d_actual_out);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}
