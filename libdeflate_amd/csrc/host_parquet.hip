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
 *
 * libdeflate_amd_parquet_decode_batch_ex takes BYTE_ARRAY rows too
 * (parquet_strings_plan.h, parquet_strings_kernels.hip).  Its rows go through
 * the same inflate batch, run walk and verdict merge; the expand kernel writes
 * the fixed-width pages as before, and between the run walk and it
 * lda_pqs_walk_kernel lists the starts of the length-prefixed values,
 * lda_pqs_sum_kernel sums the string slots' lengths per tile, scan_enqueue()
 * places the tiles, lda_pqs_offsets_kernel writes the entries and
 * lda_pqs_copy_kernel gathers the bytes; lda_pqs_final_kernel, the call's last
 * launch, adds the strings' verdicts and writes d_bytes_total.  Behind the
 * pages' info d->bgzf then holds [two words per walk section][the start lists]
 * [every string slot's place][and source][the tile sums, their places and the
 * scan's block sums].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_read_plan.h"
#include "parquet_plan.h"
#include "parquet_strings_plan.h"

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
static_assert(LIBDEFLATE_AMD_PARQUET_BYTE_ARRAY == PQ_BYTE_ARRAY && LDA_SCAN_BLOCK == PQS_SCAN_BLOCK &&
	      (int)LDA_PQS_WCOLS == (int)PQS_WCOLS && (int)LDA_PQS_W_CAP == (int)PQS_W_CAP &&
	      (int)LDA_PQS_SCOLS == (int)PQS_SCOLS && (int)LDA_PQS_S_STARTS == (int)PQS_S_STARTS &&
	      (int)LDA_PQS_VCOLS == (int)PQS_VCOLS && (int)LDA_PQS_V_DWALK == (int)PQS_V_DWALK,
	      "parquet_strings_plan.h and kernels.h hold copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_parquet_stages) */
enum {
	PQ_STAGE_INFLATE = 1, PQ_STAGE_RUNS = 2, PQ_STAGE_EXPAND = 4, PQ_STAGE_ALL = 7,
	/* the _ex call's */
	PQS_STAGE_WALK = 8, PQS_STAGE_SUM = 16, PQS_STAGE_OFFSETS = 32, PQS_STAGE_COPY = 64,
	PQS_STAGE_ALL = 127
};

/* what the _ex call has beyond the old one */
struct PqsCall {
	const pqs_plan *plan;
	uint8_t *d_bytes;
	uint64_t bytes_avail;
	uint64_t *d_bytes_total;
};

/* the string pages' launches between the run walk and the expand kernel.
 * g_walks: [two words per walk section][the start lists]; g_places: [every
 * string slot's place, the total][every slot's source]; g_sums: [the tile sums]
 * [their places][the scan's block sums and the total] */
static void
pqs_enqueue(DeviceCtx *ctx, const pq_plan &p, const PqsCall &sp, const uint64_t *ucols,
	    const uint64_t *cols, const int32_t *g_decode, const uint8_t *in, const uint8_t *g_rooms,
	    const uint4 *g_runs, uint32_t *g_info, uint32_t *g_walks, uint64_t *g_places, uint64_t *g_sums,
	    uint8_t *out, uint8_t *valid, unsigned stages, hipStream_t st)
{
	const pqs_plan &q = *sp.plan;
	const uint64_t *wcols = cols + q.w_at, *scols = cols + q.s_at;

	if (q.n_w && (stages & PQS_STAGE_WALK))
		hipLaunchKernelGGL(lda_pqs_walk_kernel, dim3(wave_grid(ctx, (size_t)q.n_w)), dim3(256), 0, st,
				   q.n_w, wcols, g_decode, (const uint32_t *)g_info, in, g_rooms, g_walks);
	if (q.tiles && (stages & PQS_STAGE_SUM))
		hipLaunchKernelGGL(lda_pqs_sum_kernel, dim3(tile_grid(ctx, q.tiles)), dim3(256), 0, st,
				   p.n_u, q.n_s, q.tiles, ucols, scols, in, g_rooms, g_runs, g_info,
				   (const uint32_t *)g_walks, g_sums, valid, g_places);
	/* (no tile: the total alone, 0) */
	scan_enqueue(st, (size_t)q.tiles, g_sums, g_sums + q.tiles, g_sums + 2 * q.tiles);
	if (q.tiles && (stages & PQS_STAGE_OFFSETS))
		hipLaunchKernelGGL(lda_pqs_offsets_kernel, dim3(tile_grid(ctx, q.tiles)), dim3(256), 0, st,
				   p.n_u, q.n_s, q.tiles, ucols, scols, (const uint64_t *)g_sums, out,
				   g_places);
	if (q.tiles && sp.bytes_avail && (stages & PQS_STAGE_COPY))
		hipLaunchKernelGGL(lda_pqs_copy_kernel,
				   dim3(copy_grid(ctx, sp.bytes_avail / 4096 + 1)), dim3(256), 0, st, q.n_s,
				   scols, (const uint64_t *)g_places, in, g_rooms, sp.d_bytes, sp.bytes_avail);
}

/* sp NULL: the old call */
static int pq_decode(struct libdeflate_decompressor *d, int format, const pq_plan &p, const PqsCall *sp,
		     const uint8_t *d_in, uint8_t *d_out, uint8_t *d_valid, int32_t *d_results,
		     unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	const size_t n = (size_t)p.n, n_z = (size_t)p.n_z, n_u = (size_t)p.n_u;
	uint8_t *g_rooms = NULL;
	uint4 *g_runs = NULL;
	uint32_t *g_info = NULL, *g_walks = NULL;
	uint64_t *g_places = NULL, *g_sums = NULL;
	ChunkStage g;
	LDA_OK_TRY(chunk_stage(d, p.cols, n_z, d_in, d_out, st, g, [&](Carve &cv) {
		g_rooms = cv.take<uint8_t>((size_t)p.room_bytes + 16, 256);
		g_runs = cv.take<uint4>((size_t)p.run_records + 1);
		g_info = cv.take<uint32_t>(PQ_INFO_WORDS * n_u + 1);
		if (sp) {
			g_walks = cv.take<uint32_t>((size_t)sp->plan->walk_words + 1);
			g_places = cv.take<uint64_t>(2 * ((size_t)sp->plan->slots + 1));
			g_sums = cv.take<uint64_t>((size_t)sp->plan->sum_words);
		}
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
	if (sp)
		pqs_enqueue(ctx, p, *sp, ucols, g.cols, g_decode, in, g_rooms, g_runs, g_info, g_walks,
			    g_places, g_sums, out, valid, stages, st);
	if (p.tiles && (stages & PQ_STAGE_EXPAND))
		hipLaunchKernelGGL(lda_pq_expand_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n_u, p.tiles, ucols, in, (const uint8_t *)g_rooms,
				   (const uint4 *)g_runs, g_info, out, valid);
	hipLaunchKernelGGL(lda_pq_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, vcols, (const int32_t *)g_decode, (const uint32_t *)g_info,
			   d_results);
	if (sp) {
		const pqs_plan &q = *sp->plan;
		const uint64_t blocks = (q.tiles + PQS_SCAN_BLOCK - 1) / PQS_SCAN_BLOCK;
		hipLaunchKernelGGL(lda_pqs_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
				   (uint64_t)n, (uint64_t)n_u, q.n_s, (const uint64_t *)(g.cols + q.v_at), ucols,
				   (const uint64_t *)(g.cols + q.s_at), (const uint32_t *)g_walks,
				   (const uint64_t *)g_places, (const uint64_t *)(g_sums + 2 * q.tiles + blocks),
				   sp->bytes_avail, out, sp->d_bytes_total, d_results);
	}
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
		return pq_decode(d, format, p, NULL, (const uint8_t *)d_in, (uint8_t *)d_out,
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

static int pqs_call(const char *what, struct libdeflate_decompressor *d, int format, size_t n_pages,
		    const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		    size_t out_avail, void *d_valid, size_t valid_avail, void *d_bytes, size_t bytes_avail,
		    uint64_t *d_bytes_total, uint64_t flags, int32_t *d_results, unsigned stages,
		    void *stream)
{
	return chunk_read_call<pqs_plan>(what, d, n_pages, rows, d_in, in_nbytes, d_out, out_avail,
					 d_results, [&](pqs_plan &p, std::string &err) {
		std::vector<uint64_t> masked;
		if (!pqs_check(format, n_pages, rows, in_nbytes, out_avail, valid_avail, d_valid != NULL,
			       d_bytes != NULL, bytes_avail, d_bytes_total != NULL, flags, masked, err))
			return false;
		pqs_plan_build(n_pages, rows, masked.data(), p);
		return true;
	}, [&](const pqs_plan &p) {
		const PqsCall sp = { &p, (uint8_t *)d_bytes, bytes_avail, d_bytes_total };
		return pq_decode(d, format, p.base, &sp, (const uint8_t *)d_in, (uint8_t *)d_out,
				 (uint8_t *)d_valid, d_results, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_parquet_decode_batch_ex(struct libdeflate_decompressor *d, int format, size_t n_pages,
				       const uint64_t *rows, const void *d_in, size_t in_nbytes,
				       void *d_out, size_t out_avail, void *d_valid, size_t valid_avail,
				       void *d_bytes, size_t bytes_avail, uint64_t *d_bytes_total,
				       uint64_t flags, int32_t *d_results, void *stream)
{
	return pqs_call("parquet_decode_batch_ex", d, format, n_pages, rows, d_in, in_nbytes, d_out,
			out_avail, d_valid, valid_avail, d_bytes, bytes_avail, d_bytes_total, flags,
			d_results, PQS_STAGE_ALL, stream);
}

/* not part of the interface: lda_parquet_stages for the _ex call (8 the start
 * lists, 16 the lengths and tile sums, 32 the offsets, 64 the copy), for
 * tools/bench_parquet_strings.py.  The offsets kernel reads the lengths and the
 * copy the places: queue 32 only with 16, and 64 only with both */
extern "C" LIBDEFLATEAPI int
lda_parquet_ex_stages(struct libdeflate_decompressor *d, int format, size_t n_pages,
		      const uint64_t *rows, const void *d_in, size_t in_nbytes, void *d_out,
		      size_t out_avail, void *d_valid, size_t valid_avail, void *d_bytes,
		      size_t bytes_avail, uint64_t *d_bytes_total, uint64_t flags, int32_t *d_results,
		      unsigned stages, void *stream)
{
	return pqs_call("parquet_ex_stages", d, format, n_pages, rows, d_in, in_nbytes, d_out, out_avail,
			d_valid, valid_avail, d_bytes, bytes_avail, d_bytes_total, flags, d_results,
			stages & PQS_STAGE_ALL, stream);
}
