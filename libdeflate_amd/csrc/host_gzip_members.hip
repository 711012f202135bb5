/*
 * host_gzip_members.hip - C-ABI of reading a file of concatenated gzip members
 * from device memory (include/libdeflate_amd.h).
 *
 * The shared finder (host_finder.h) lists every offset that looks like a gzip
 * header and, once ONE size query (host_sizes.hip) has count-parsed all of
 * them, keeps the candidates reachable from offset 0; a prefix sum of their
 * counted sizes gives every member its place in one contiguous output, and
 * ONE decompress batch of max_members
 * chunks (format GZIP, exact input, exact fill) decodes there directly; the
 * chunks behind the file's last member are empty, and so are all of them when
 * the file is refused before the decode.  Nothing waits for the device and
 * nothing comes from the host but the launch sizes, which is what max_members
 * is for.
 */
#include <algorithm>

#include "host_finder.h"
#include "host_objects.h"

using namespace lda;


#define GZM_MAX_MEMBERS_MSG "%s: max_members %zu (1 .. 2^28)"

static_assert(LIBDEFLATE_AMD_GZM_MORE_MEMBERS == LDA_BR_MORE &&
	      LIBDEFLATE_AMD_GZM_MORE_CANDIDATES == LDA_GZM_MORE_CANDIDATES &&
	      LIBDEFLATE_AMD_GZM_RESULT_WORDS == LDA_GZM_RESULT_WORDS &&
	      LIBDEFLATE_AMD_GZM_NAME_MAX == LDA_GZM_NAME_MAX,
	      "kernels.h holds copies of the header's constants");

struct MembersScratch {
	Finder f;
	/* the candidates: the size query's descriptors and answers */
	uint64_t *c_in_off, *c_in_n, *c_ain, *c_out;
	int32_t *c_res;
	/* the members: sizes, the decode batch */
	uint64_t *msize, *bsum_b, *in_off, *in_n, *out_off, *out_av, *ain;
	int32_t *results;
	uint8_t *sizes;		/* the size query's own scratch */
	size_t bytes;
};

static MembersScratch members_scratch(void *base, size_t n, size_t M)
{
	MembersScratch s;
	Carve c(base);
	/* two candidates start 3 bytes apart at least */
	s.f.carve(c, n, std::min(M + LIBDEFLATE_AMD_GZM_SLACK, n / 3 + 1));
	const size_t cap = s.f.cap;
	s.c_in_off = c.take<uint64_t>(cap);
	s.c_in_n = c.take<uint64_t>(cap);
	s.c_ain = c.take<uint64_t>(cap);
	s.c_out = c.take<uint64_t>(cap);
	s.msize = c.take<uint64_t>(M);
	s.bsum_b = c.take<uint64_t>(scan_blocks(M) + 1);
	s.in_off = c.take<uint64_t>(M);
	s.in_n = c.take<uint64_t>(M);
	s.out_off = c.take<uint64_t>(M);
	s.out_av = c.take<uint64_t>(M);
	s.ain = c.take<uint64_t>(M);
	s.c_res = c.take<int32_t>(cap);
	s.f.carve_chain(c);
	s.results = c.take<int32_t>(M);
	s.sizes = c.take<uint8_t>(sizes_scratch_bytes(cap), 64);
	s.bytes = c.at;
	return s;
}

static int members_enqueue(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n,
			   size_t M, uint8_t *d_out, uint64_t out_avail, uint64_t *d_result,
			   uint64_t *d_index, bool decode, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (n == 0) {	/* no member at offset 0: BAD_DATA, as the host loop says */
		hipLaunchKernelGGL(lda_gzm_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)0,
				   (uint64_t)M, out_avail, (const uint64_t *)NULL, (uint64_t)0,
				   (const uint32_t *)NULL, (const uint64_t *)NULL,
				   (const uint64_t *)NULL, (const int32_t *)NULL,
				   (const uint64_t *)NULL, d_result, d_index);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	void *ws = d->bgzf.reserve(members_scratch(NULL, n, M).bytes);
	if (!ws)
		return LIBDEFLATE_AMD_OOM;
	const MembersScratch s = members_scratch(ws, n, M);
	const Finder &f = s.f;
	const uint64_t *k_at = f.k_at();
	const uint64_t cap = f.cap;
	const unsigned per256 = (unsigned)((M + 255) / 256);
	const unsigned cap256 = (unsigned)((f.cap + 255) / 256);

	LDA_OK_TRY(finder_list(f, st, [&](const uint64_t *offs, const uint64_t *bsum) {
		hipLaunchKernelGGL(lda_gzm_scan_kernel, dim3((unsigned)f.nwg), dim3(256), 0, st, d_in,
				   (uint64_t)n, f.counts, offs, bsum, cap, f.cand_pos);
	}));
	/* the speculation: every candidate whose header is bounded counted as a
	 * member that runs to the end of the file at most (none of what follows
	 * does anything when the candidates overflowed their room) */
	hipLaunchKernelGGL(lda_gzm_slots_kernel, dim3(cap256), dim3(256), 0, st, d_in, (uint64_t)n, k_at,
			   cap, (const uint64_t *)f.cand_pos, s.c_in_off, s.c_in_n);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	int rc = sizes_enqueue(ctx, s.sizes, LIBDEFLATE_AMD_GZIP, f.cap, d_in, s.c_in_off, s.c_in_n, NULL,
			   s.c_res, s.c_ain, s.c_out, st, NULL, 0);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	hipLaunchKernelGGL(lda_gzm_size32_kernel, dim3(cap256), dim3(256), 0, st, k_at, cap,
			   s.c_res, (const uint64_t *)s.c_ain, f.cand_size);
	finder_chain(f, st, n, M, s.in_off, s.in_n);
	hipLaunchKernelGGL(lda_gzm_break_kernel, dim3(1), dim3(64), 0, st, k_at, cap,
			   (const uint64_t *)f.cand_pos, (const uint32_t *)f.next,
			   (const uint32_t *)f.exit_at, (const int32_t *)s.c_res, f.state);
	/* counted sizes -> places in the output -> descriptors and index */
	hipLaunchKernelGGL(lda_gzm_msize_kernel, dim3(per256), dim3(256), 0, st, (uint64_t)M, k_at,
			   cap, (const uint64_t *)f.cand_pos, (const uint64_t *)s.c_out,
			   (const uint32_t *)f.state, (const uint64_t *)s.in_off, s.msize);
	const uint64_t *total_at = s.bsum_b + scan_enqueue(st, M, s.msize, s.out_off, s.bsum_b);
	hipLaunchKernelGGL(lda_gzm_desc_kernel, dim3(per256), dim3(256), 0, st, (uint64_t)M,
			   out_avail, k_at, cap, (const uint32_t *)f.state, (const uint64_t *)s.msize,
			   (const uint64_t *)s.bsum_b, s.in_off, s.in_n, s.out_off, s.out_av, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (decode) {
		/* exact fill: no byte lands outside a member's place.  (A NULL d_out
		 * has out_avail 0: only empty members are decoded, nothing is written) */
		rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_GZIP, M, d_in, s.in_off, s.in_n,
						     d_out ? (void *)d_out : ws, s.out_off, s.out_av,
						     s.results, s.ain, NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	hipLaunchKernelGGL(lda_gzm_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)n, (uint64_t)M,
			   out_avail, k_at, cap, (const uint32_t *)f.state, total_at,
			   (const uint64_t *)s.in_n,
			   (const int32_t *)(decode ? s.results : NULL), (const uint64_t *)s.ain,
			   d_result, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_gzip_members_decompress_batch(struct libdeflate_decompressor *d, const void *d_in,
					     size_t in_nbytes, size_t max_members, void *d_out,
					     size_t out_avail, uint64_t *d_result, uint64_t *d_index,
					     void *stream)
{
	const char *what = "gzip_members_decompress_batch";
	if (!finder_args_ok(what, d, d_in, in_nbytes, GZM_MAX_MEMBERS_MSG, max_members, 1, d_result))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!d_out && out_avail) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return members_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_members, (uint8_t *)d_out,
			       out_avail, d_result, d_index, true, (hipStream_t)stream);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_gzip_members_index_batch(struct libdeflate_decompressor *d, const void *d_in,
					size_t in_nbytes, size_t max_members, uint64_t *d_result,
					uint64_t *d_index, void *stream)
{
	if (!finder_args_ok("gzip_members_index_batch", d, d_in, in_nbytes, GZM_MAX_MEMBERS_MSG,
			    max_members, 1, d_result))
		return LIBDEFLATE_AMD_BAD_ARG;
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return members_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_members, NULL, ~(uint64_t)0,
			       d_result, d_index, false, (hipStream_t)stream);
}

/* for tools/bench_gzip_members.py, not part of the interface: the candidate
 * scan's count pass alone (d_counts: one u64 per 16 KiB of file) */
extern "C" __attribute__((visibility("default"))) int
lda_gzm_scan_bench(const void *d_in, size_t n, uint64_t *d_counts, void *stream)
{
	if (!d_in || !n || !d_counts || n > LDA_FINDER_MAX_FILE)
		return LIBDEFLATE_AMD_BAD_ARG;
	hipLaunchKernelGGL(lda_gzm_scan_kernel,
			   dim3((unsigned)((n + LDA_BR_SCAN_WG - 1) / LDA_BR_SCAN_WG)), dim3(256), 0,
			   (hipStream_t)stream, (const uint8_t *)d_in, (uint64_t)n, d_counts,
			   (const uint64_t *)NULL, (const uint64_t *)NULL, (uint64_t)0,
			   (uint64_t *)NULL);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}
