/*
 * host_zip_large.hip - libdeflate_amd_zip_read_large (include/libdeflate_amd.h):
 * libdeflate_amd_zip_read_batch for archives with a few huge entries.
 *
 * zip_large_plan.h takes the sibling's plan and lifts out of it the entries
 * that one wave or one workgroup would sit on: a deflated entry of large_min
 * compressed bytes and more goes to libdeflate_amd_decompress_large, an entry
 * above LIBDEFLATE_AMD_ZIP_PIECE bytes is copied and checksummed in pieces of
 * that size - ordinary chunks of lda_zip_copy_kernel and of the CRC-32 batch -
 * and lda_zip_lfinal_kernel (zip_large_kernels.hip) combines the pieces'
 * CRC-32 and writes those entries' results.  Everything else is the sibling's
 * one batch over the sibling's columns.
 *
 * The order: all of the object's reader scratch is reserved first, for the
 * columns, the tables, the pieces' CRCs and the batch's results, and nothing
 * grows it later.  Then the many-wave entries are decoded, one blocking call
 * after another; each waits for what is queued on `stream` before it reads
 * d_in, and its output is complete when it returns.  Their results are
 * written into the table on the host, so the columns and both tables go up in
 * ONE copy behind the last of them.  Only then is the rest enqueued on
 * `stream`: the batch, the two copies, the two CRC batches - the pieces' reads
 * what the many-wave decodes wrote -, lda_zip_rfinal_kernel over the runs of
 * rows it owns and lda_zip_lfinal_kernel over the others.  Decoding first
 * also keeps the blocking call's one-wave answer (a batch of one on the
 * object's stream, with the object's decode scratch) from meeting this call's
 * own batch in that scratch.  Without a many-wave entry nothing blocks.
 */
#include <string.h>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "zip_large_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_ZIP_PIECE == LDA_ZIP_PIECE, "kernels.h holds a copy of the constant");
static_assert(ZIPL_OWNED == LDA_ZIPL_OWNED && ZIPL_MANY_WAVE == LDA_ZIPL_MANY_WAVE &&
	      ZIPL_PIECED == LDA_ZIPL_PIECED,
	      "zip_large_plan.h holds copies of kernels.h's constants");

static int zip_read_large(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n_sel,
			  ZipLargePlan &p, uint8_t *d_out, int32_t *d_results, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t L = (size_t)p.n_own, P = (size_t)p.n_pieces;
	/* device: [the plan's columns][the owned entries][the pieces][ain][batch
	 * results][crcs][the pieces' crcs] */
	uint64_t *g_cols = NULL, *g_own = NULL, *g_pcs = NULL, *g_ain = NULL;
	int32_t *g_res = NULL;
	uint32_t *g_crc = NULL, *g_pcrc = NULL;
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		g_cols = cv.take<uint64_t>(ZIP_COLS * n_sel, 8);
		g_own = cv.take<uint64_t>(ZIPL_COLS * L, 8);
		g_pcs = cv.take<uint64_t>(ZIPP_COLS * P, 8);
		const ReadUp up = { g_cols, cv.at };
		g_ain = cv.take<uint64_t>(n_sel);
		g_res = cv.take<int32_t>(n_sel);
		g_crc = cv.take<uint32_t>(n_sel);
		g_pcrc = cv.take<uint32_t>(P);
		return up;
	}, s));
	uint8_t *h = s.h;
	/* (a NULL d_out has out_avail 0: nothing is written, nothing is read) */
	uint8_t *out = d_out ? d_out : s.ws;

	/* the many-wave entries, one after another, each filling the device */
	uint64_t *own[ZIPL_COLS];
	for (size_t a = 0; a < ZIPL_COLS; a++)
		own[a] = p.own.data() + a * L;
	for (size_t j = 0; j < L; j++) {
		if (!(own[ZIPL_COL_FLAGS][j] & ZIPL_MANY_WAVE))
			continue;
		const uint64_t usize = own[ZIPL_COL_USIZE][j];
		size_t ain = 0;
		const int res = libdeflate_amd_decompress_large(
			d, LIBDEFLATE_AMD_DEFLATE, d_in + own[ZIPL_COL_IN_OFF][j],
			(size_t)own[ZIPL_COL_IN_N][j], d_out ? d_out + own[ZIPL_COL_OUT_OFF][j] : NULL,
			(size_t)usize, &ain, NULL, st);
		own[ZIPL_COL_RES][j] = (uint64_t)(uint32_t)res;
		own[ZIPL_COL_AIN][j] = res == LIBDEFLATE_SUCCESS ? ain : 0;
	}

	const size_t b_cols = sizeof(uint64_t) * ZIP_COLS * n_sel;
	const size_t b_own = sizeof(uint64_t) * ZIPL_COLS * L;
	memcpy(h, p.cols.data(), b_cols);
	if (L)
		memcpy(h + b_cols, p.own.data(), b_own);
	if (P)
		memcpy(h + b_cols + b_own, p.pieces.data(), sizeof(uint64_t) * ZIPP_COLS * P);
	LDA_OK_TRY(read_send(d, s, st));
	const uint64_t *col[ZIP_COLS], *lc[ZIPL_COLS], *pc[ZIPP_COLS];
	for (size_t a = 0; a < ZIP_COLS; a++)
		col[a] = g_cols + a * n_sel;
	for (size_t a = 0; a < ZIPL_COLS; a++)
		lc[a] = g_own + a * L;
	for (size_t a = 0; a < ZIPP_COLS; a++)
		pc[a] = g_pcs + a * P;

	/* the sibling's batch, the pieces' copy behind the entries' */
	LDA_OK_TRY(zip_read_entries(d, n_sel, col, g_res, g_ain, g_crc, d_in, out, st, P,
				    pc[ZIPP_COL_SRC], pc[ZIPP_COL_DST], pc[ZIPP_COL_CP]));
	if (P)
		LDA_OK_TRY(libdeflate_amd_crc32_batch(P, out, pc[ZIPP_COL_DST], pc[ZIPP_COL_LEN], NULL,
						      g_pcrc, st));
	/* the two final kernels never write the same row: the runs are the rows
	 * without the mark that lda_zip_lfinal_kernel looks for */
	for (size_t k = 0; k + 1 < p.runs.size(); k += 2) {
		const size_t r0 = (size_t)p.runs[k], nr = (size_t)p.runs[k + 1];
		hipLaunchKernelGGL(lda_zip_rfinal_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256),
				   0, st, (uint64_t)nr, col[ZIP_COL_META] + r0, col[ZIP_COL_IN_N] + r0,
				   (const int32_t *)g_res + r0, (const uint64_t *)g_ain + r0,
				   (const uint32_t *)g_crc + r0, d_results + r0);
	}
	if (L)
		hipLaunchKernelGGL(lda_zip_lfinal_kernel, dim3(tile_grid(ctx, (L + 3) / 4)), dim3(256), 0,
				   st, (uint64_t)L, (uint64_t)n_sel, (uint64_t)P,
				   lc[ZIPL_COL_SEL], lc[ZIPL_COL_FLAGS], lc[ZIPL_COL_IN_N],
				   lc[ZIPL_COL_USIZE], lc[ZIPL_COL_FIRST], lc[ZIPL_COL_COUNT],
				   lc[ZIPL_COL_RES], lc[ZIPL_COL_AIN], col[ZIP_COL_META],
				   (const int32_t *)g_res, (const uint64_t *)g_ain, (const uint32_t *)g_crc,
				   pc[ZIPP_COL_DST], pc[ZIPP_COL_LEN], (const uint32_t *)g_pcrc, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_zip_read_large(struct libdeflate_decompressor *d, const void *d_in,
			      size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
			      const uint64_t *sel, void *d_out, size_t out_avail, size_t out_align,
			      size_t large_min, uint64_t *out_offsets, int32_t *d_results,
			      void *stream)
{
	const char *what = "zip_read_large";
	if (!read_args_ok(what, d, d_in, in_nbytes, index, entries, n_sel, sel, d_out, out_avail,
			  out_align, d_results))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!large_min)
		large_min = env_cfg().zip_large_min;
	return read_call<ZipLargePlan>(what, d, n_sel, [&](ZipLargePlan &plan, std::string &err) {
		return zip_plan_read_large(index, entries, n_sel, sel, in_nbytes, out_avail,
					   out_align - 1, large_min, LIBDEFLATE_AMD_ZIP_PIECE, plan,
					   out_offsets, NULL, err);
	}, [&](ZipLargePlan &plan) {
		return zip_read_large(d, (const uint8_t *)d_in, n_sel, plan, (uint8_t *)d_out,
				      d_results, (hipStream_t)stream);
	});
}
