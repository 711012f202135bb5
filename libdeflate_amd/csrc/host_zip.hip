/*
 * host_zip.hip - C-ABI of reading a ZIP archive from device memory
 * (include/libdeflate_amd.h).
 *
 * The kernels of zip_kernels.hip find the end record; the shared finder
 * (host_finder.h) lists every offset of the central directory that looks like
 * a directory record and, once they are sized, keeps the candidates reachable
 * from cd_off; every
 * entry is resolved against its local header; a prefix sum of the stated sizes
 * gives every entry its place in one contiguous output; ONE decompress batch
 * of max_entries chunks (format DEFLATE, exact input, exact fill) decodes the
 * method-8 entries there, one copy kernel places the stored ones, and ONE
 * CRC-32 batch over the places is compared with the directory's values.  The
 * chunks of stored, refused and surplus entries are empty, and so are all of
 * them when the archive is refused before the decode.  Nothing waits for the
 * device and nothing comes from the host but the launch sizes, which is what
 * max_entries is for.
 *
 * A selection (libdeflate_amd_zip_read_batch) takes the index rows and the
 * entry numbers from the host: zip_plan.h checks them and builds the
 * descriptors, which go up in one copy.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "zip_plan.h"

using namespace lda;

#define ZIP_END_BYTES 22

static_assert(LIBDEFLATE_AMD_ZIP_MORE_ENTRIES == LDA_ZIP_MORE_ENTRIES &&
	      LIBDEFLATE_AMD_ZIP_MORE_ENTRIES == LDA_BR_MORE &&
	      LIBDEFLATE_AMD_ZIP_MORE_CANDIDATES == LDA_ZIP_MORE_CANDIDATES &&
	      LIBDEFLATE_AMD_ZIP_UNSUPPORTED == LDA_ZIP_UNSUPPORTED &&
	      LIBDEFLATE_AMD_ZIP_RESULT_WORDS == LDA_ZIP_RESULT_WORDS &&
	      LIBDEFLATE_AMD_ZIP_WORDS == LDA_ZIP_WORDS &&
	      LIBDEFLATE_AMD_ZIP_ZIP64 == LDA_ZIP_ZIP64,
	      "kernels.h holds copies of the header's constants");
static_assert(ZIP_UNSUPPORTED == LDA_ZIP_UNSUPPORTED && ZIP_BAD_DATA == LIBDEFLATE_BAD_DATA &&
	      ZIP_ROW_WORDS == LDA_ZIP_WORDS && ZIP_KIND_NONE == LDA_ZIP_KIND_NONE &&
	      ZIP_KIND_STORED == LDA_ZIP_KIND_STORED && ZIP_KIND_DEFLATE == LDA_ZIP_KIND_DEFLATE,
	      "zip_plan.h holds copies of them too");

struct ZipScratch {
	Finder f;
	uint64_t *zs;
	/* the entries: rows (when the caller wants no index), rooms, the batches */
	uint64_t *rows, *sizes, *bsum_b, *in_off, *in_n, *out_off, *out_av, *ain;
	uint64_t *cp_src, *cp_len, *crc_n, *meta;
	int32_t *bres;
	uint32_t *crcs;
	size_t bytes;
};

static ZipScratch zip_scratch(void *base, size_t n, size_t M, bool own_rows)
{
	ZipScratch s;
	Carve c(base);
	/* two signatures start 4 bytes apart at least */
	s.f.carve(c, n, std::min(M + LIBDEFLATE_AMD_ZIP_SLACK, n / 4 + 1));
	s.zs = c.take<uint64_t>(LDA_ZS_WORDS);
	s.rows = c.take<uint64_t>(own_rows ? LDA_ZIP_WORDS * M : 0);
	s.sizes = c.take<uint64_t>(M);
	s.bsum_b = c.take<uint64_t>(scan_blocks(M) + 1);
	s.in_off = c.take<uint64_t>(M);
	s.in_n = c.take<uint64_t>(M);
	s.out_off = c.take<uint64_t>(M);
	s.out_av = c.take<uint64_t>(M);
	s.ain = c.take<uint64_t>(M);
	s.cp_src = c.take<uint64_t>(M);
	s.cp_len = c.take<uint64_t>(M);
	s.crc_n = c.take<uint64_t>(M);
	s.meta = c.take<uint64_t>(M);
	s.f.carve_chain(c);
	s.bres = c.take<int32_t>(M);
	s.crcs = c.take<uint32_t>(M);
	s.bytes = c.at;
	return s;
}

/* what the two device-only calls check before they touch a device */
static bool zip_args_ok(const char *what, const struct libdeflate_decompressor *d,
			const void *d_in, size_t n, size_t max_entries, size_t out_align,
			const void *d_result, const void *d_results)
{
	if (!d_results) {
		set_error("%s: NULL argument", what);
		return false;
	}
	return finder_args_ok(what, d, d_in, n, "%s: max_entries %zu (1 .. 2^28)", max_entries, 1,
			      d_result) &&
	       read_align_ok(what, out_align);
}

static int zip_enqueue(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n, size_t M,
		       uint8_t *d_out, uint64_t out_avail, size_t out_align, uint64_t *d_result,
		       uint64_t *d_index, int32_t *d_results, bool decode, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (n < ZIP_END_BYTES) {	/* no room for an end record: BAD_DATA */
		hipLaunchKernelGGL(lda_zip_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)M,
				   out_avail, (const uint64_t *)NULL, (const uint32_t *)NULL,
				   (const uint64_t *)NULL, (uint64_t)0, (const uint64_t *)NULL,
				   (const uint64_t *)NULL, (const uint64_t *)NULL,
				   (const int32_t *)NULL, (const uint64_t *)NULL,
				   (const uint32_t *)NULL, d_results, d_result);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	void *ws = d->bgzf.reserve(zip_scratch(NULL, n, M, !d_index).bytes);
	if (!ws)
		return LIBDEFLATE_AMD_OOM;
	const ZipScratch s = zip_scratch(ws, n, M, !d_index);
	const Finder &f = s.f;
	const uint64_t *k_at = f.k_at();
	const uint64_t cap = f.cap;
	uint64_t *rows = d_index ? d_index : s.rows;
	const unsigned per256 = (unsigned)((M + 255) / 256);
	const unsigned cap256 = (unsigned)((f.cap + 255) / 256);

	hipLaunchKernelGGL(lda_zip_end_kernel, dim3(1), dim3(1024), 0, st, d_in, (uint64_t)n, s.zs);
	/* the candidates of the directory */
	LDA_OK_TRY(finder_list(f, st, [&](const uint64_t *offs, const uint64_t *bsum) {
		hipLaunchKernelGGL(lda_zip_scan_kernel, dim3((unsigned)f.nwg), dim3(256), 0, st, d_in,
				   (const uint64_t *)s.zs, f.counts, offs, bsum, cap, f.cand_pos);
	}));
	hipLaunchKernelGGL(lda_zip_size_kernel, dim3(cap256), dim3(256), 0, st, d_in,
			   (const uint64_t *)s.zs, k_at, cap, (const uint64_t *)f.cand_pos,
			   f.cand_size);
	/* the chain in positions relative to cd_off: it starts at 0 and ends at
	 * LDA_ZIP_CHAIN_END (lda_zip_size_kernel) */
	finder_chain(f, st, LDA_ZIP_CHAIN_END, M, s.in_off, s.in_n);
	/* entries -> rooms -> places in the output -> descriptors and index */
	hipLaunchKernelGGL(lda_zip_resolve_kernel, dim3(per256), dim3(256), 0, st, d_in, (uint64_t)M,
			   (uint64_t)(out_align - 1), (const uint64_t *)s.zs,
			   (const uint32_t *)f.state, k_at, cap, (const uint64_t *)s.in_off, rows,
			   d_results, s.sizes);
	const uint64_t *total_at = s.bsum_b + scan_enqueue(st, M, s.sizes, s.out_off, s.bsum_b);
	hipLaunchKernelGGL(lda_zip_desc_kernel, dim3(per256), dim3(256), 0, st, (uint64_t)M,
			   out_avail, (const uint64_t *)s.zs, (const uint32_t *)f.state, k_at, cap,
			   (const uint64_t *)s.bsum_b, rows, (const int32_t *)d_results, s.in_off,
			   s.in_n, s.out_off, s.out_av, s.cp_src, s.cp_len, s.crc_n, s.meta);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (decode) {
		/* (a NULL d_out has out_avail 0: only empty entries are live, nothing
		 * is written and nothing is read) */
		uint8_t *out = d_out ? d_out : (uint8_t *)ws;
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_DEFLATE, M, d_in, s.in_off,
						     s.in_n, out, s.out_off, s.out_av, s.bres, s.ain,
						     NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
		hipLaunchKernelGGL(lda_zip_copy_kernel, dim3(copy_grid(ctx, M)), dim3(256), 0, st,
				   (uint64_t)M, (const uint64_t *)s.cp_src,
				   (const uint64_t *)s.out_off, (const uint64_t *)s.cp_len, d_in, out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		rc = libdeflate_amd_crc32_batch(M, out, s.out_off, s.crc_n, NULL, s.crcs, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	hipLaunchKernelGGL(lda_zip_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)M, out_avail,
			   (const uint64_t *)s.zs, (const uint32_t *)f.state, k_at, cap, total_at,
			   (const uint64_t *)s.meta,
			   (const uint64_t *)s.in_n, (const int32_t *)(decode ? s.bres : NULL),
			   (const uint64_t *)s.ain, (const uint32_t *)s.crcs, d_results, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_zip_decompress_batch(struct libdeflate_decompressor *d, const void *d_in,
				    size_t in_nbytes, size_t max_entries, void *d_out,
				    size_t out_avail, size_t out_align, uint64_t *d_result,
				    uint64_t *d_index, int32_t *d_results, void *stream)
{
	const char *what = "zip_decompress_batch";
	if (!zip_args_ok(what, d, d_in, in_nbytes, max_entries, out_align, d_result, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!d_out && out_avail) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return zip_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_entries, (uint8_t *)d_out,
			   out_avail, out_align, d_result, d_index, d_results, true,
			   (hipStream_t)stream);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_zip_index_batch(struct libdeflate_decompressor *d, const void *d_in,
			       size_t in_nbytes, size_t max_entries, size_t out_align,
			       uint64_t *d_result, uint64_t *d_index, int32_t *d_results,
			       void *stream)
{
	if (!zip_args_ok("zip_index_batch", d, d_in, in_nbytes, max_entries, out_align, d_result,
			 d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return zip_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_entries, NULL, ~(uint64_t)0,
			   out_align, d_result, d_index, d_results, false, (hipStream_t)stream);
}

/* ---- a selection of entries, index rows on the host ---- */

int lda::zip_read_entries(struct libdeflate_decompressor *d, size_t n, const uint64_t *const *col,
			  int32_t *g_res, uint64_t *g_ain, uint32_t *g_crc, const uint8_t *in,
			  uint8_t *out, hipStream_t st, size_t n_pieces, const uint64_t *pc_src,
			  const uint64_t *pc_dst, const uint64_t *pc_len)
{
	DeviceCtx *ctx = device_ctx();
	LDA_OK_TRY(libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_DEFLATE, n, in, col[ZIP_COL_IN_OFF],
						   col[ZIP_COL_IN_N], out, col[ZIP_COL_OUT_OFF],
						   col[ZIP_COL_OUT_AV], g_res, g_ain, NULL, st));
	hipLaunchKernelGGL(lda_zip_copy_kernel, dim3(copy_grid(ctx, n)), dim3(256), 0, st, (uint64_t)n,
			   col[ZIP_COL_CP_SRC], col[ZIP_COL_OUT_OFF], col[ZIP_COL_CP_LEN], in, out);
	if (n_pieces)
		hipLaunchKernelGGL(lda_zip_copy_kernel, dim3(copy_grid(ctx, n_pieces)), dim3(256), 0, st,
				   (uint64_t)n_pieces, pc_src, pc_dst, pc_len, in, out);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return libdeflate_amd_crc32_batch(n, out, col[ZIP_COL_OUT_OFF], col[ZIP_COL_CRC_N], NULL, g_crc,
					  st);
}

static int zip_read(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		    const std::vector<uint64_t> &cols, uint8_t *d_out, int32_t *d_results,
		    hipStream_t st)
{
	/* device: [the plan's columns][ain][batch results][crcs] */
	uint64_t *g_cols = NULL, *g_ain = NULL;
	int32_t *g_res = NULL;
	uint32_t *g_crc = NULL;
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		g_cols = cv.take<uint64_t>(ZIP_COLS * n_sel);
		const ReadUp up = { g_cols, cv.at };
		g_ain = cv.take<uint64_t>(n_sel);
		g_res = cv.take<int32_t>(n_sel);
		g_crc = cv.take<uint32_t>(n_sel);
		return up;
	}, s));
	memcpy(s.h, cols.data(), s.up.bytes);
	LDA_OK_TRY(read_send(d, s, st));
	const uint64_t *col[ZIP_COLS];
	for (size_t a = 0; a < ZIP_COLS; a++)
		col[a] = g_cols + a * n_sel;
	/* (a NULL d_out has out_avail 0: nothing is written, nothing is read) */
	uint8_t *out = d_out ? d_out : s.ws;
	LDA_OK_TRY(zip_read_entries(d, n_sel, col, g_res, g_ain, g_crc, d_in, out, st));
	hipLaunchKernelGGL(lda_zip_rfinal_kernel, dim3((unsigned)((n_sel + 255) / 256)), dim3(256),
			   0, st, (uint64_t)n_sel, col[ZIP_COL_META], col[ZIP_COL_IN_N],
			   (const int32_t *)g_res, (const uint64_t *)g_ain, (const uint32_t *)g_crc,
			   d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_zip_read_batch(struct libdeflate_decompressor *d, const void *d_in,
			      size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			      const uint64_t *sel, void *d_out, size_t out_avail, size_t out_align,
			      uint64_t *out_offsets, int32_t *d_results, void *stream)
{
	const char *what = "zip_read_batch";
	if (!read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			  out_align, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	typedef std::vector<uint64_t> Cols;
	return read_call<Cols>(what, d, n_sel, [&](Cols &cols, std::string &err) {
		return zip_plan_read(index, entries, n_sel, sel, in_nbytes, out_avail, out_align - 1,
				     cols, out_offsets, NULL, err);
	}, [&](const Cols &cols) {
		return zip_read(d, (const uint8_t *)d_in, n_sel, cols, (uint8_t *)d_out, d_results,
				(hipStream_t)stream);
	});
}
