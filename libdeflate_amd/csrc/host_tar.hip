/*
 * host_tar.hip - C-ABI of reading a tar archive from device memory
 * (include/libdeflate_amd.h).
 *
 * The scan kernel of tar_kernels.hip lists every block that passes the header
 * rule, as (position, size) in blocks; the shared finder (host_finder.h) keeps
 * the candidates reachable from block 0; every record of the chain is
 * resolved - is it an entry, what is it called, how many bytes has it -; two
 * prefix sums over the records number the entries and give every entry its
 * place in one contiguous output, a third counts the tiles of the gather copy
 * in front of every entry, and one copy kernel on a grid sized from out_avail
 * and max_records moves the bytes.  Nothing waits for the device and nothing
 * comes from the host but the launch sizes, which is what max_records is for.
 *
 * A selection (libdeflate_amd_tar_read_batch) takes the index rows and the
 * entry numbers from the host: tar_plan.h checks them and builds the copy's
 * columns, which go up in one copy.  libdeflate_amd_tar_ranges is the same
 * arithmetic without a device.
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "tar_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_TAR_MORE_RECORDS == LDA_TAR_MORE_RECORDS &&
	      LIBDEFLATE_AMD_TAR_MORE_RECORDS == LDA_BR_MORE &&
	      LIBDEFLATE_AMD_TAR_MORE_CANDIDATES == LDA_TAR_MORE_CANDIDATES &&
	      LIBDEFLATE_AMD_TAR_UNSUPPORTED == LDA_TAR_UNSUPPORTED &&
	      LIBDEFLATE_AMD_TAR_RESULT_WORDS == LDA_TAR_RESULT_WORDS &&
	      LIBDEFLATE_AMD_TAR_WORDS == LDA_TAR_WORDS &&
	      LIBDEFLATE_AMD_TAR_EOF == LDA_TAR_EOF && LIBDEFLATE_AMD_TAR_HAS_L == LDA_TAR_HAS_L &&
	      LIBDEFLATE_AMD_TAR_HAS_PAX == LDA_TAR_HAS_PAX,
	      "kernels.h holds copies of the header's constants");
static_assert(TAR_UNSUPPORTED == LDA_TAR_UNSUPPORTED && TAR_ROW_WORDS == LDA_TAR_WORDS &&
	      TAR_COPY_TILE == LDA_TAR_COPY_TILE && TAR_MAX_FILE == LDA_FINDER_MAX_FILE &&
	      LDA_TAR_SCAN_BLOCKS * TAR_BLOCK == LDA_BR_SCAN_WG,
	      "tar_plan.h holds copies of them too");

struct TarScratch {
	Finder f;
	uint64_t *ts, *rec_pos, *rec_n, *tmp;
	uint64_t *flag, *f_off, *f_sums, *room, *r_off, *r_sums, *tiles, *t_off, *t_sums;
	uint64_t *cp_src, *cp_dst, *cp_len;
	int32_t *res;
	size_t bytes;
};

static TarScratch tar_scratch(void *base, size_t nb, size_t M)
{
	TarScratch s;
	Carve c(base);
	const size_t sb = scan_blocks(M) + 1;
	/* a candidate is a block */
	s.f.carve(c, nb * TAR_BLOCK, std::min(M + LIBDEFLATE_AMD_TAR_SLACK, nb));
	s.ts = c.take<uint64_t>(LDA_TS_WORDS);
	s.rec_pos = c.take<uint64_t>(M);
	s.rec_n = c.take<uint64_t>(M);
	s.tmp = c.take<uint64_t>(7 * M);
	s.flag = c.take<uint64_t>(M);
	s.f_off = c.take<uint64_t>(M);
	s.f_sums = c.take<uint64_t>(sb);
	s.room = c.take<uint64_t>(M);
	s.r_off = c.take<uint64_t>(M);
	s.r_sums = c.take<uint64_t>(sb);
	s.tiles = c.take<uint64_t>(M);
	s.t_off = c.take<uint64_t>(M);
	s.t_sums = c.take<uint64_t>(sb);
	s.cp_src = c.take<uint64_t>(M);
	s.cp_dst = c.take<uint64_t>(M);
	s.cp_len = c.take<uint64_t>(M);
	s.f.carve_chain(c);
	s.res = c.take<int32_t>(M);
	s.bytes = c.at;
	return s;
}

/* what the two device-only calls check before they touch a device */
static bool tar_args_ok(const char *what, const struct libdeflate_decompressor *d,
			const void *d_in, size_t n, size_t max_records, size_t out_align,
			const void *d_result, const void *d_results)
{
	if (!d_results) {
		set_error("%s: NULL argument", what);
		return false;
	}
	return finder_args_ok(what, d, d_in, n, "%s: max_records %zu (1 .. 2^28)", max_records, 1,
			      d_result) &&
	       read_align_ok(what, out_align);
}

static int tar_enqueue(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n, size_t M,
		       uint8_t *d_out, uint64_t out_avail, size_t out_align, uint64_t *d_result,
		       uint64_t *d_index, int32_t *d_results, bool extract, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t nb = n / TAR_BLOCK;
	if (nb == 0) {	/* tarfile's "empty file": BAD_DATA */
		hipLaunchKernelGGL(lda_tar_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)0,
				   (uint64_t)M, out_avail, (const uint32_t *)NULL,
				   (const uint64_t *)NULL, (uint64_t)0, (const uint64_t *)NULL,
				   (const uint64_t *)NULL, (const uint64_t *)NULL,
				   (const int32_t *)NULL, d_result);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	void *ws = d->bgzf.reserve(tar_scratch(NULL, nb, M).bytes);
	if (!ws)
		return LIBDEFLATE_AMD_OOM;
	const TarScratch s = tar_scratch(ws, nb, M);
	const Finder &f = s.f;
	const uint64_t *k_at = f.k_at();
	const uint64_t cap = f.cap;
	const unsigned per256 = (unsigned)((M + 255) / 256);

	if (env_cfg().tar_serial) {
		hipLaunchKernelGGL(lda_tar_walk_kernel, dim3(1), dim3(64), 0, st, d_in, (uint64_t)nb,
				   (uint64_t)M, s.rec_pos, s.rec_n, f.state, (uint64_t *)k_at);
	} else {
		/* the candidates, sized as the chain wants them, and the chain to nb */
		LDA_OK_TRY(finder_list(f, st, [&](const uint64_t *offs, const uint64_t *bsum) {
			hipLaunchKernelGGL(lda_tar_scan_kernel, dim3((unsigned)f.nwg), dim3(256), 0, st,
					   d_in, (uint64_t)nb, f.counts, offs, bsum, cap, f.cand_pos,
					   f.cand_size, f.state);
		}));
		finder_chain(f, st, nb, M, s.rec_pos, s.rec_n);
	}
	/* records -> entries, rooms -> numbers, places -> rows, descriptors */
	hipLaunchKernelGGL(lda_tar_resolve_kernel, dim3(per256), dim3(256), 0, st, d_in, (uint64_t)nb,
			   (uint64_t)M, (uint64_t)(out_align - 1), f.state, k_at, cap,
			   (const uint64_t *)s.rec_pos, s.ts, s.tmp, s.res, s.flag, s.room);
	const uint64_t *entries_at = s.f_sums + scan_enqueue(st, M, s.flag, s.f_off, s.f_sums);
	const uint64_t *total_at = s.r_sums + scan_enqueue(st, M, s.room, s.r_off, s.r_sums);
	hipLaunchKernelGGL(lda_tar_desc_kernel, dim3(per256), dim3(256), 0, st, (uint64_t)M, out_avail,
			   (const uint32_t *)f.state, k_at, cap, (const uint64_t *)s.tmp,
			   (const int32_t *)s.res, (const uint64_t *)s.flag,
			   (const uint64_t *)s.f_off, (const uint64_t *)s.f_sums,
			   (const uint64_t *)s.r_off, (const uint64_t *)s.r_sums, d_index, d_results,
			   s.cp_src, s.cp_dst, s.cp_len, s.tiles);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (extract && d_out) {
		/* (a NULL d_out has out_avail 0: only empty entries fit, no tile) */
		const uint64_t *tiles_at = s.t_sums + scan_enqueue(st, M, s.tiles, s.t_off, s.t_sums);
		/* every entry ends in at most one tile that is not full */
		const uint64_t bound = out_avail / TAR_COPY_TILE + M;
		hipLaunchKernelGGL(lda_tar_copy_kernel, dim3(copy_grid(ctx, bound)), dim3(256), 0, st,
				   (uint64_t)M, (const uint64_t *)s.t_off, (const uint64_t *)s.t_sums,
				   tiles_at, (const uint64_t *)s.cp_src, (const uint64_t *)s.cp_dst,
				   (const uint64_t *)s.cp_len, d_in, d_out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_tar_final_kernel, dim3(1), dim3(256), 0, st, (uint64_t)nb, (uint64_t)M,
			   out_avail, (const uint32_t *)f.state, k_at, cap, (const uint64_t *)s.ts,
			   entries_at, total_at, (const int32_t *)d_results, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tar_extract_batch(struct libdeflate_decompressor *d, const void *d_in,
				 size_t in_nbytes, size_t max_records, void *d_out,
				 size_t out_avail, size_t out_align, uint64_t *d_result,
				 uint64_t *d_index, int32_t *d_results, void *stream)
{
	const char *what = "tar_extract_batch";
	if (!tar_args_ok(what, d, d_in, in_nbytes, max_records, out_align, d_result, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!d_out && out_avail) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return tar_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_records, (uint8_t *)d_out,
			   out_avail, out_align, d_result, d_index, d_results, true,
			   (hipStream_t)stream);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tar_index_batch(struct libdeflate_decompressor *d, const void *d_in,
			       size_t in_nbytes, size_t max_records, size_t out_align,
			       uint64_t *d_result, uint64_t *d_index, int32_t *d_results,
			       void *stream)
{
	if (!tar_args_ok("tar_index_batch", d, d_in, in_nbytes, max_records, out_align, d_result,
			 d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return tar_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_records, NULL, ~(uint64_t)0,
			   out_align, d_result, d_index, d_results, false, (hipStream_t)stream);
}

/* ---- a selection of entries, index rows on the host ---- */

static int tar_read(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
		    const std::vector<uint64_t> &cols, const std::vector<int32_t> &results,
		    uint8_t *d_out, int32_t *d_results, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	/* device: [the plan's columns][the tile count][the results] */
	const size_t col_bytes = cols.size() * sizeof(uint64_t);
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		uint8_t *up = cv.take<uint8_t>(col_bytes + n_sel * sizeof(int32_t));
		return ReadUp{ up, cv.at };
	}, s));
	memcpy(s.h, cols.data(), col_bytes);
	memcpy(s.h + col_bytes, results.data(), n_sel * sizeof(int32_t));
	LDA_OK_TRY(read_send(d, s, st));
	const uint64_t *g = (const uint64_t *)s.ws;
	const uint64_t tiles = cols[TAR_COLS * n_sel];
	LDA_HIP_TRY(hipMemcpyAsync(d_results, s.ws + col_bytes, n_sel * sizeof(int32_t),
				   hipMemcpyDeviceToDevice, st),
		    LIBDEFLATE_AMD_NO_DEVICE);
	if (tiles) {	/* (then d_out is not NULL) */
		hipLaunchKernelGGL(lda_tar_copy_kernel, dim3(copy_grid(ctx, tiles)), dim3(256), 0, st,
				   (uint64_t)n_sel, g + TAR_COL_TILE * n_sel, (const uint64_t *)NULL,
				   g + TAR_COLS * n_sel, g + TAR_COL_SRC * n_sel,
				   g + TAR_COL_DST * n_sel, g + TAR_COL_LEN * n_sel, d_in, d_out);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tar_read_batch(struct libdeflate_decompressor *d, const void *d_in,
			      size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			      const uint64_t *sel, void *d_out, size_t out_avail, size_t out_align,
			      uint64_t *out_offsets, int32_t *d_results, void *stream)
{
	const char *what = "tar_read_batch";
	if (!read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			  out_align, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	struct Plan {
		std::vector<uint64_t> cols;
		std::vector<int32_t> results;
	};
	return read_call<Plan>(what, d, n_sel, [&](Plan &p, std::string &err) {
		return tar_plan_read(index, entries, n_sel, sel, in_nbytes, out_avail, out_align - 1,
				     p.cols, p.results, out_offsets, NULL, err);
	}, [&](const Plan &p) {
		return tar_read(d, (const uint8_t *)d_in, n_sel, p.cols, p.results, (uint8_t *)d_out,
				d_results, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tar_ranges(const uint64_t *index, size_t entries, size_t n_sel, const uint64_t *sel,
			  uint64_t *ranges, uint64_t *total_ret)
{
	const char *what = "tar_ranges";
	if (!read_sel_args_ok(what, index, entries, n_sel, sel))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (n_sel && !ranges) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return read_plan_call(what, [&](std::string &err) {
		uint64_t total = 0;
		if (!tar_plan_ranges(index, entries, n_sel, sel, ranges, &total, err))
			return false;
		if (total_ret)
			*total_ret = total;
		return true;
	});
}
