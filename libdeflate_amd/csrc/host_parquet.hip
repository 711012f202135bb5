/*
 * host_parquet.hip - C-ABI of reading the pages of flat Parquet column chunks
 * from device memory (include/libdeflate_amd.h:
 * libdeflate_amd_parquet_decode_batch).
 *
 * parquet_plan.h checks the rows and builds the columns, which go up through
 * the object's pinned block in ONE copy.  The compressed sections are decoded
 * into rooms of the object's scratch in ONE decompress batch; uncompressed
 * sections and the levels of V2 pages are read in place.  Then three launches
 * (parquet_kernels.hip): lda_pq_runs_kernel lists the runs of every data
 * page's hybrid streams, lda_pq_expand_kernel writes the slots and validity
 * bytes of all pages, lda_pq_final_kernel merges the verdicts.  Nothing waits
 * for the device and nothing is read back.
 * d->bgzf: [the rooms][the run records][the pages' info][the plan's columns]
 * [the decoder's results].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "parquet_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PARQUET_WORDS == PQ_WORDS && LDA_PQ_TILE == PQ_TILE &&
	      LDA_PQ_LEVEL_PIECE == PQ_LEVEL_PIECE && LDA_PQ_RUN_WORDS == PQ_RUN_WORDS &&
	      LDA_PQ_INFO_WORDS == PQ_INFO_WORDS && LDA_PQ_DATA_V2 == PQ_DATA_V2 &&
	      LDA_PQ_PLAIN == PQ_PLAIN && LDA_PQ_IN_PLACE == PQ_IN_PLACE &&
	      LDA_PQ_F_SKIP == PQ_F_SKIP && LDA_PQ_V_IS_DICT == PQ_V_IS_DICT &&
	      (int)LDA_PQ_UCOLS == (int)PQ_UCOLS && (int)LDA_PQ_U_ICAP == (int)PQ_U_ICAP &&
	      (int)LDA_PQ_U_FIELDS == (int)PQ_U_FIELDS && (int)LDA_PQ_V_DICT == (int)PQ_V_DICT &&
	      LIBDEFLATE_AMD_PARQUET_DATA_V1 == PQ_DATA_V1 && LIBDEFLATE_AMD_PARQUET_DICT == PQ_DICT &&
	      LIBDEFLATE_AMD_PARQUET_DATA_V2 == PQ_DATA_V2 && sizeof(uint4) == 4 * PQ_RUN_WORDS,
	      "parquet_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_parquet_stages) */
enum { PQ_STAGE_INFLATE = 1, PQ_STAGE_RUNS = 2, PQ_STAGE_EXPAND = 4, PQ_STAGE_ALL = 7 };

static int pq_decode(struct libdeflate_decompressor *d, int format, const pq_plan &p,
		     const uint8_t *d_in, uint8_t *d_out, uint8_t *d_valid, int32_t *d_results,
		     unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n, n_z = (size_t)p.n_z, n_u = (size_t)p.n_u;
	uint8_t *g_rooms = NULL;
	uint4 *g_runs = NULL;
	uint32_t *g_info = NULL;
	ChunkStage g;
	LDA_OK_TRY(chunk_stage(d, p.cols, n_z, d_in, d_out, st, g, [&](Carve &cv) {
		g_rooms = cv.take<uint8_t>((size_t)p.room_bytes + 16, 256);
		g_runs = cv.take<uint4>((size_t)p.run_records + 1);
		g_info = cv.take<uint32_t>(PQ_INFO_WORDS * n_u + 1);
	}));
	const uint64_t *ucols = g.cols + p.u_at, *vcols = g.cols + p.v_at;
	const uint8_t *in = g.in;
	/* (NULL d_valid: no row uses it) */
	uint8_t *out = g.out, *valid = d_valid ? d_valid : g.ws;
	const int32_t *g_decode = g.decode;

	if (stages & PQ_STAGE_INFLATE)
		LDA_OK_TRY(chunk_inflate(d, format, g, n_z, g_rooms, 0, st));
	if (n_u && (stages & PQ_STAGE_RUNS))
		hipLaunchKernelGGL(lda_pq_runs_kernel, dim3(wave_grid(ctx, n_u)), dim3(256), 0, st,
				   (uint64_t)n_u, ucols, (const int32_t *)g_decode, in,
				   (const uint8_t *)g_rooms, g_runs, g_info);
	if (p.tiles && (stages & PQ_STAGE_EXPAND))
		hipLaunchKernelGGL(lda_pq_expand_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n_u, p.tiles, ucols, in, (const uint8_t *)g_rooms,
				   (const uint4 *)g_runs, g_info, out, valid);
	hipLaunchKernelGGL(lda_pq_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, vcols, (const int32_t *)g_decode, (const uint32_t *)g_info,
			   d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int pq_call(const char *what, struct libdeflate_decompressor *d, int format, size_t n_pages,
		   const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		   size_t out_avail, void *d_valid, size_t valid_avail, int32_t *d_results,
		   unsigned stages, void *stream)
{
	return chunk_read_call<pq_plan>(what, d, n_pages, rows, d_in, in_nbytes, d_out, out_avail, d_results,
					[&](pq_plan &p, std::string &err) {
		if (!pq_check(format, n_pages, rows, in_nbytes, out_avail, valid_avail, d_valid != NULL,
			      err))
			return false;
		pq_plan_build(n_pages, rows, p);
		return true;
	}, [&](const pq_plan &p) {
		return pq_decode(d, format, p, (const uint8_t *)d_in, (uint8_t *)d_out,
				 (uint8_t *)d_valid, d_results, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_parquet_decode_batch(struct libdeflate_decompressor *d, int format, size_t n_pages,
				    const uint64_t *rows, const void *d_in, size_t in_nbytes,
				    void *d_out, size_t out_avail, void *d_valid, size_t valid_avail,
				    int32_t *d_results, void *stream)
{
	return pq_call("parquet_decode_batch", d, format, n_pages, rows, d_in, in_nbytes, d_out,
		       out_avail, d_valid, valid_avail, d_results, PQ_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 inflate, 2 the run lists, 4 the expand kernel; 0: the upload and the
 * verdict kernel alone), so that tools/bench_parquet.py can time the kernels
 * alone on scratch an earlier full call has filled */
extern "C" LIBDEFLATEAPI int
lda_parquet_stages(struct libdeflate_decompressor *d, int format, size_t n_pages,
		   const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		   size_t out_avail, void *d_valid, size_t valid_avail, int32_t *d_results,
		   unsigned stages, void *stream)
{
	return pq_call("parquet_stages", d, format, n_pages, rows, d_in, in_nbytes, d_out, out_avail,
		       d_valid, valid_avail, d_results, stages & PQ_STAGE_ALL, stream);
}
