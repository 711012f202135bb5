/*
 * host_prefix.hip - C-ABI of the prefix decompress (inflate_prefix.hip):
 *
 *   libdeflate_amd_decompress_prefix_batch[_dict]  device arrays, enqueue only
 *   libdeflate_amd_decompress_prefix               one stream, host pointers
 *   libdeflate_amd_gzip_members_peek_batch         the heads of the members of
 *                                                  an indexed gzip file
 *
 * The reference's whole-buffer calls decode a stream whole or not at all
 * (libdeflate.h:216-217: the buffer is undefined on INSUFFICIENT_SPACE); zlib's
 * inflate() with a small avail_out is what their callers use to look at the
 * head of a stream.  Here that is a batch call: the decode kernel's PREFIX
 * mode, then the checksum and the footer check of the decode batch, which
 * touch only the streams that ended within their limit.
 */
#include "host_objects.h"
#include "kernels.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PREFIX == 19, "inflate_kernel.hip: LDA_PREFIX");

/* scratch of one call: [sums u32 x n][actual_in u64 x n][order u32 x n]
 * [dictionary block: its header, see lda_dict_prep_kernel()] */
static size_t prefix_dict_at(size_t n)
{
	return align_up(align_up(n * 4, 16) + 8 * n + 4 * n + 16, 64);
}

static size_t prefix_scratch_bytes(size_t n)
{
	return prefix_dict_at(n) + LDA_DICT_BLK_HDR;
}

static bool prefix_args_ok(const char *what, const struct libdeflate_decompressor *d, int format,
			   size_t n, const void *d_in, const uint64_t *d_in_offsets,
			   const uint64_t *d_in_nbytes, const void *d_out,
			   const uint64_t *d_out_offsets, const uint64_t *d_limits,
			   const int32_t *d_results, const uint64_t *d_actual_out)
{
	if (!d || format < LIBDEFLATE_AMD_DEFLATE || format > LIBDEFLATE_AMD_GZIP ||
	    (n && (!d_in || !d_in_offsets || !d_in_nbytes || !d_out || !d_out_offsets ||
		   !d_limits || !d_results || !d_actual_out))) {
		set_error("%s: bad argument", what);
		return false;
	}
	return true;
}

/* arguments checked by the callers, n > 0 */
static int prefix_enqueue(struct libdeflate_decompressor *d, int format, size_t n,
			  const void *d_in, const uint64_t *d_in_offsets,
			  const uint64_t *d_in_nbytes, void *d_out, const uint64_t *d_out_offsets,
			  const uint64_t *d_limits, int32_t *d_results, uint64_t *d_actual_in,
			  uint64_t *d_actual_out, hipStream_t st, const void *d_dict,
			  size_t dict_nbytes)
{
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	DeviceCtx *c = device_ctx();
	if (!c)
		return LIBDEFLATE_AMD_NO_DEVICE;
	uint8_t *s = (uint8_t *)d->scratch.reserve(prefix_scratch_bytes(n));
	if (!s)
		return LIBDEFLATE_AMD_OOM;
	const size_t sums_bytes = align_up(n * 4, 16);
	uint32_t *sums = (uint32_t *)s;
	uint64_t *ain = d_actual_in ? d_actual_in : (uint64_t *)(s + sums_bytes);
	/* a preset dictionary: as in the decode batch */
	const uint8_t *dtail = NULL;
	uint32_t dlen = 0;
	uint32_t *dict_id = NULL;
	if (d_dict && dict_nbytes) {
		dlen = (uint32_t)(dict_nbytes < 32768 ? dict_nbytes : 32768);
		dtail = (const uint8_t *)d_dict + dict_nbytes - dlen;
		uint8_t *blk = s + prefix_dict_at(n);
		hipLaunchKernelGGL(lda_dict_prep_kernel, dim3(1), dim3(64), 0, st,
				   (const uint8_t *)d_dict, (uint64_t)dict_nbytes, 0u, 0u, 0u, blk);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		if (format == LIBDEFLATE_AMD_ZLIB) {
			dict_id = (uint32_t *)(blk + 4);
			int rc = libdeflate_amd_adler32_batch(1, d_dict, (const uint64_t *)(blk + 16),
							      (const uint64_t *)(blk + 24), NULL, dict_id,
							      (void *)st);
			if (rc != LIBDEFLATE_AMD_OK)
				return rc;
		}
	}
	/* token rows of every wave, then the counter the waves take their second
	 * and later streams from */
	/* (the decode batch's grid, LDS and token scratch: the kernel has the wave
	 * kernel's geometry, inflate_prefix.hip asserts it) */
	const size_t grid_max = (size_t)c->num_cus * inflate_waves_per_cu();
	const size_t grid = grid_max < n ? grid_max : n;
	const size_t tok_bytes = grid * lda_inflate_tokcap() * 4;
	uint32_t *tok = (uint32_t *)d->tokens.reserve(inflate_tokens_bytes(n, c->num_cus));
	if (!tok)
		return LIBDEFLATE_AMD_OOM;
	uint32_t *next = (uint32_t *)((uint8_t *)tok + tok_bytes);
	LDA_HIP_TRY(hipMemsetAsync(next, 0, 16, st), LIBDEFLATE_AMD_NO_DEVICE);
	/* more streams than wave slots: costliest first.  What a stream costs
	 * follows its input, but no further than its limit lets the decode go:
	 * the order's rule for stored data (input about as long as the room)
	 * puts a short prefix of a long stream among the cheap ones */
	uint32_t *order = NULL;
	if (n > grid && n < 0xFFFFFFFFull) {
		order = (uint32_t *)(s + sums_bytes + 8 * n);
		hipLaunchKernelGGL(lda_inflate_order_kernel, dim3(1), dim3(1024), 0, st,
				   (uint64_t)n, d_in_nbytes, d_limits, order);
	}
	hipLaunchKernelGGL(lda_inflate_prefix_kernel, dim3((unsigned)grid), dim3(64),
			   inflate_wave_lds(), st, (uint64_t)n, format,
			   env_cfg().inflate_par ? 1u : 0u, tok, next, (const uint32_t *)order,
			   (const uint8_t *)d_in, d_in_offsets, d_in_nbytes, (uint8_t *)d_out,
			   d_out_offsets, d_limits, d_results, ain, d_actual_out, dtail, dlen,
			   (const uint32_t *)dict_id);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (format == LIBDEFLATE_AMD_DEFLATE)
		return LIBDEFLATE_AMD_OK;
	/* the checksum of what every stream produced.  A cut stream's is computed
	 * too, over its limit's bytes, and not used - the footer check skips every
	 * row that is not SUCCESS: the checksum batch takes its lengths from
	 * d_actual_out and cannot see the results.  One more pass over the
	 * prefixes, at the checksum kernels' rate */
	int rc = format == LIBDEFLATE_AMD_GZIP ?
		libdeflate_amd_crc32_batch(n, d_out, d_out_offsets, d_actual_out, NULL, sums,
					   (void *)st) :
		libdeflate_amd_adler32_batch(n, d_out, d_out_offsets, d_actual_out, NULL, sums,
					     (void *)st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	hipLaunchKernelGGL(lda_inflate_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256),
			   0, st, (uint64_t)n, format, 0, (const uint8_t *)d_in, d_in_offsets,
			   d_limits, sums, d_results, ain, d_actual_out);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix_batch(struct libdeflate_decompressor *d, int format, size_t n,
				       const void *d_in, const uint64_t *d_in_offsets,
				       const uint64_t *d_in_nbytes, void *d_out,
				       const uint64_t *d_out_offsets, const uint64_t *d_limits,
				       int32_t *d_results, uint64_t *d_actual_in,
				       uint64_t *d_actual_out, void *stream)
{
	if (!prefix_args_ok("decompress_prefix_batch", d, format, n, d_in, d_in_offsets,
			    d_in_nbytes, d_out, d_out_offsets, d_limits, d_results, d_actual_out))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (n == 0)
		return LIBDEFLATE_AMD_OK;
	return prefix_enqueue(d, format, n, d_in, d_in_offsets, d_in_nbytes, d_out, d_out_offsets,
			      d_limits, d_results, d_actual_in, d_actual_out, (hipStream_t)stream,
			      NULL, 0);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix_batch_dict(struct libdeflate_decompressor *d, int format,
					    size_t n, const void *d_dict, size_t dict_nbytes,
					    const void *d_in, const uint64_t *d_in_offsets,
					    const uint64_t *d_in_nbytes, void *d_out,
					    const uint64_t *d_out_offsets, const uint64_t *d_limits,
					    int32_t *d_results, uint64_t *d_actual_in,
					    uint64_t *d_actual_out, void *stream)
{
	/* zlib refuses a dictionary on a gzip stream */
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB) {
		set_error("decompress_prefix_batch_dict: format %d takes no dictionary", format);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (dict_nbytes && !d_dict) {
		set_error("decompress_prefix_batch_dict: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (!prefix_args_ok("decompress_prefix_batch_dict", d, format, n, d_in, d_in_offsets,
			    d_in_nbytes, d_out, d_out_offsets, d_limits, d_results, d_actual_out))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (n == 0)
		return LIBDEFLATE_AMD_OK;
	return prefix_enqueue(d, format, n, d_in, d_in_offsets, d_in_nbytes, d_out, d_out_offsets,
			      d_limits, d_results, d_actual_in, d_actual_out, (hipStream_t)stream,
			      d_dict, dict_nbytes);
}

/*
 * One host buffer: a batch of one on the object's compute stream.  Staging:
 * [in_off in_n out_off limit ain aout][result][input][output].
 */
static int prefix_one_body(struct libdeflate_decompressor *d, int format, const void *in,
			   size_t in_nbytes, void *out, size_t limit, size_t *actual_out_ret)
{
	const char *what = "libdeflate_amd_decompress_prefix";
	DeviceGuard on(d->device);
	if (!on.ok() || !device_ctx()) {
		complain(what, LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_BAD_DATA;	/* a library-side failure: see decompress_one() */
	}
	/* (the staging holds input and limit: checked by the caller not to wrap) */
	const size_t in_at = 64, out_at = align_up(in_at + in_nbytes + 16, 64);
	uint8_t *st = (uint8_t *)d->stage.reserve(out_at + limit + 64);
	if (!st || !d->streams.enter()) {
		complain(what, st ? LIBDEFLATE_AMD_NO_DEVICE : LIBDEFLATE_AMD_OOM);
		return LIBDEFLATE_BAD_DATA;
	}
	hipStream_t sc = d->streams.comp;
	uint64_t desc[6] = { in_at, in_nbytes, out_at, limit, 0, 0 };
	uint64_t *dd = (uint64_t *)st;
	int32_t res = LIBDEFLATE_BAD_DATA;
	int rc = LIBDEFLATE_AMD_OK;
	if (hipMemcpyAsync(st, desc, sizeof(desc), hipMemcpyHostToDevice, sc) != hipSuccess ||
	    (in_nbytes && hipMemcpyAsync(st + in_at, in, in_nbytes, hipMemcpyHostToDevice,
					 sc) != hipSuccess))
		rc = LIBDEFLATE_AMD_NO_DEVICE;
	if (rc == LIBDEFLATE_AMD_OK)
		rc = prefix_enqueue(d, format, 1, st, dd, dd + 1, st, dd + 2, dd + 3,
				    (int32_t *)(st + 48), dd + 4, dd + 5, sc, NULL, 0);
	if (rc == LIBDEFLATE_AMD_OK &&
	    (hipMemcpyAsync(desc, st, sizeof(desc), hipMemcpyDeviceToHost, sc) != hipSuccess ||
	     hipMemcpyAsync(&res, st + 48, 4, hipMemcpyDeviceToHost, sc) != hipSuccess ||
	     hipStreamSynchronize(sc) != hipSuccess))
		rc = LIBDEFLATE_AMD_NO_DEVICE;
	const bool bytes = res == LIBDEFLATE_SUCCESS || res == LIBDEFLATE_AMD_PREFIX;
	if (rc == LIBDEFLATE_AMD_OK && bytes) {
		if (desc[5] > limit)	/* (cannot be: no read past the caller's room) */
			rc = LIBDEFLATE_AMD_NO_DEVICE;
		else if (desc[5] &&
			 hipMemcpy(out, st + out_at, desc[5], hipMemcpyDeviceToHost) != hipSuccess)
			rc = LIBDEFLATE_AMD_NO_DEVICE;
	}
	if (rc != LIBDEFLATE_AMD_OK) {
		(void)hipStreamSynchronize(sc);
		complain(what, rc);
		return LIBDEFLATE_BAD_DATA;
	}
	if (bytes)
		*actual_out_ret = desc[5];
	return res;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_decompress_prefix(struct libdeflate_decompressor *d, int format, const void *in,
				 size_t in_nbytes, void *out, size_t limit, size_t *actual_out_ret)
{
	if (!d || format < LIBDEFLATE_AMD_DEFLATE || format > LIBDEFLATE_AMD_GZIP ||
	    (!in && in_nbytes) || (!out && limit) || !actual_out_ret) {
		set_error("libdeflate_amd_decompress_prefix: bad argument");
		return LIBDEFLATE_BAD_DATA;
	}
	/* the object's staging buffer holds in_nbytes + limit bytes: sizes whose
	 * sum is no size are refused (a limit is the room the caller has, not
	 * "no limit") */
	if (in_nbytes > SIZE_MAX / 4 || limit > SIZE_MAX / 4) {
		set_error("libdeflate_amd_decompress_prefix: bad argument (in_nbytes + limit)");
		return LIBDEFLATE_BAD_DATA;
	}
	return no_unwind("libdeflate_amd_decompress_prefix", (int)LIBDEFLATE_BAD_DATA, [&]() {
		return prefix_one_body(d, format, in, in_nbytes, out, limit, actual_out_ret);
	});
}

/*
 * The heads of an indexed gzip-members file.  Scratch of the object: [what the
 * prefix batch uses][in_off in_n out_off limit: u64 x M each] - reserved in
 * one piece before the first launch, so that the batch's own reservation finds
 * it large enough and moves nothing.
 */
extern "C" LIBDEFLATEAPI int
libdeflate_amd_gzip_members_peek_batch(struct libdeflate_decompressor *d, const void *d_in,
				       size_t in_nbytes, const uint64_t *d_result,
				       const uint64_t *d_index, size_t max_members,
				       size_t head_nbytes, void *d_heads, uint64_t *d_head_nbytes,
				       int32_t *d_results, void *stream)
{
	const size_t M = max_members;
	if (!d || (!d_in && in_nbytes) || !d_result || !d_index || !d_head_nbytes || !d_results ||
	    (!d_heads && head_nbytes) || M == 0 || M > ((size_t)1 << 28) ||
	    head_nbytes > 0xFFFFFFFFull) {
		set_error("gzip_members_peek_batch: bad argument");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (!device_ctx())
		return LIBDEFLATE_AMD_NO_DEVICE;
	hipStream_t st = (hipStream_t)stream;
	const size_t front = align_up(prefix_scratch_bytes(M), 64), col = align_up(8 * M, 64);
	uint8_t *s = (uint8_t *)d->scratch.reserve(front + 4 * col);
	if (!s)
		return LIBDEFLATE_AMD_OOM;
	uint64_t *in_off = (uint64_t *)(s + front), *in_n = (uint64_t *)(s + front + col),
		 *out_off = (uint64_t *)(s + front + 2 * col),
		 *limits = (uint64_t *)(s + front + 3 * col);
	hipLaunchKernelGGL(lda_gzm_peek_desc_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
			   st, (uint64_t)M, (uint64_t)in_nbytes, (uint64_t)head_nbytes, d_result,
			   d_index, in_off, in_n, out_off, limits, (int32_t *)NULL,
			   (uint64_t *)NULL);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	/* (a NULL d_heads has head_nbytes 0: nothing is written) */
	int rc = prefix_enqueue(d, LIBDEFLATE_AMD_GZIP, M, d_in, in_off, in_n,
				d_heads ? d_heads : (void *)s, out_off, limits, d_results, NULL,
				d_head_nbytes, st, NULL, 0);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	/* the rows without a member report nothing */
	hipLaunchKernelGGL(lda_gzm_peek_desc_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
			   st, (uint64_t)M, (uint64_t)in_nbytes, (uint64_t)head_nbytes, d_result,
			   d_index, in_off, in_n, out_off, limits, d_results, d_head_nbytes);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}
