/*
 * host_read_plan.h - what the readers that take their plan from the host share:
 * the selections of the ZIP, tar and PNG readers, the BGZF ranged read
 * (host_zip.hip, host_zip_large.hip, host_tar.hip, host_png*.hip,
 * host_bgzf_read.hip) and the chunk codecs - byte-shuffled chunks, TIFF
 * segments, OpenEXR chunks, Parquet pages (host_shuffle.hip, host_tiff.hip,
 * host_exr.hip, host_parquet.hip).  The counterpart of host_write_pieces.h:
 * the refusals made before any device work, the envelope of a call around its
 * plan, the staging of the plan's columns through d->bgzf and the pinned block
 * of d->bgzf_up, the chunk codecs' inflate step and verdict launch, and the
 * grids of the kernels that stride over entries, tiles or chunks - the
 * writers' too.
 *
 * The object's rule lives in read_stage() alone: bgzf_up.begin() before
 * anything is reserved, and all of the call's scratch reserved before anything
 * is queued (growing frees memory and waits for the device).
 */
#ifndef LDA_HOST_READ_PLAN_H
#define LDA_HOST_READ_PLAN_H

#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "chunk_plan.h"
#include "host_finder.h"
#include "host_objects.h"

namespace lda {

/* ---- the refusals ---- */

static inline bool read_align_ok(const char *what, size_t out_align)
{
	if (!out_align || out_align > 256 || (out_align & (out_align - 1))) {
		set_error("%s: out_align %zu is not a power of two in 1 .. 256", what, out_align);
		return false;
	}
	return true;
}

/* the index rows and the selection, as the host-only calls take them too */
static inline bool read_sel_args_ok(const char *what, const uint64_t *index, size_t entries,
				    size_t n_sel, const uint64_t *sel)
{
	if ((!index && entries) || (n_sel && !sel)) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (entries > LDA_FINDER_MAX_RECORDS || n_sel > LDA_FINDER_MAX_RECORDS) {
		set_error("%s: entries %zu, n_sel %zu (at most 2^28)", what, entries, n_sel);
		return false;
	}
	return true;
}

/* what a selection's call refuses before it looks at the rows */
static inline bool
read_args_ok(const char *what, const struct libdeflate_decompressor *d, const void *d_in,
	     size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
	     const uint64_t *sel, const void *d_out, size_t out_avail, size_t out_align,
	     const int32_t *d_results)
{
	if (!d || (!d_in && in_nbytes) || (!d_out && out_avail) || (n_sel && !d_results)) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (!read_sel_args_ok(what, index, entries, n_sel, sel))
		return false;
	if (in_nbytes > LDA_FINDER_MAX_FILE) {
		set_error("%s: in_nbytes %zu above 2^36", what, in_nbytes);
		return false;
	}
	return read_align_ok(what, out_align);
}

/* ---- the envelope of a call ---- */

/* plan(err) -> bool: the host arithmetic; false is the call's BAD_ARG, with
 * the plan's reason under the call's name */
template <typename Plan> static inline bool read_plan_ok(const char *what, Plan &plan)
{
	std::string err;
	if (plan(err))
		return true;
	set_error("%s: %s", what, err.c_str());
	return false;
}

/* a call that is its plan alone: no device */
template <typename Plan> static inline int read_plan_call(const char *what, Plan plan)
{
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		return read_plan_ok(what, plan) ? LIBDEFLATE_AMD_OK : LIBDEFLATE_AMD_BAD_ARG;
	});
}

/* a call with a plan of type P, which lives here: plan(p, err) -> bool fills
 * it, then - of n rows, none: nothing to do - run(p) -> int queues it on the
 * object's device */
template <typename P, typename Plan, typename Run>
static inline int read_call(const char *what, struct libdeflate_decompressor *d, size_t n, Plan plan,
			    Run run)
{
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		P p;
		auto filled = [&](std::string &err) { return plan(p, err); };
		if (!read_plan_ok(what, filled))
			return LIBDEFLATE_AMD_BAD_ARG;
		if (n == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return run(p);
	});
}

/* ---- the staging ---- */

/* what of a layout goes up: `bytes` from the pinned block to `dst`, the first
 * region of the layout or one behind an area the kernels fill */
struct ReadUp {
	void *dst;
	size_t bytes;
};

struct ReadStage {
	uint8_t *ws = NULL;	/* d->bgzf, laid out */
	uint8_t *h = NULL;	/* the pinned block: up.bytes for the caller to fill */
	ReadUp up = { NULL, 0 };
};

/* lay(Carve &) -> ReadUp carves the call's regions out of d->bgzf; it runs
 * twice, for the sizes and on the memory.  Behind it everything the call needs
 * of d->bgzf (and `slack` bytes) and of the pinned block is reserved: OK, OOM
 * or NO_DEVICE */
template <typename Lay>
static inline int read_stage(struct libdeflate_decompressor *d, Lay lay, ReadStage &s,
			     size_t slack = 16)
{
	Carve sizes(NULL);
	const size_t up_bytes = lay(sizes).bytes;
	LDA_OK_TRY(d->bgzf_up.begin());
	s.ws = (uint8_t *)d->bgzf.reserve(sizes.at + slack);
	s.h = (uint8_t *)d->bgzf_up.pinned(up_bytes);
	if (!s.ws || !s.h)
		return LIBDEFLATE_AMD_OOM;
	Carve real(s.ws);
	s.up = lay(real);
	return LIBDEFLATE_AMD_OK;
}

/* the filled pinned block on its way to where the layout wants it */
static inline int read_send(struct libdeflate_decompressor *d, const ReadStage &s, hipStream_t st)
{
	return d->bgzf_up.send(s.up.dst, s.up.bytes, st);
}

/* ---- the chunk codecs: shuffle, TIFF, OpenEXR, Parquet (chunk_plan.h) ---- */

/* read_call() behind the pointers such a call refuses */
template <typename P, typename Plan, typename Run>
static inline int
chunk_read_call(const char *what, struct libdeflate_decompressor *d, size_t n, const uint64_t *rows,
		const void *d_in, size_t in_nbytes, const void *d_out, size_t out_avail,
		const int32_t *d_results, Plan plan, Run run)
{
	if (!d || (n && (!rows || !d_results)) || (!d_in && in_nbytes) || (!d_out && out_avail)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return read_call<P>(what, d, n, plan, run);
}

/* a plan's columns on the device */
struct ChunkStage {
	uint8_t *ws;				/* d->bgzf */
	uint64_t *cols;
	const uint64_t *dcol[CHUNK_DCOLS];	/* the decode batches' columns */
	int32_t *decode;			/* and their results */
	/* d_in and d_out; of a NULL one, whose size is 0 and which no row that
	 * passed the checks touches, ws stands in */
	const uint8_t *in;
	uint8_t *out;
};

/* d->bgzf laid out as [what front(Carve &) takes: the format's rooms and work
 * areas][the plan's columns][the decoder's results, n_dec + 1], and the columns
 * on their way up through the pinned block in ONE copy */
template <typename Front>
static inline int
chunk_stage(struct libdeflate_decompressor *d, const std::vector<uint64_t> &cols, size_t n_dec,
	    const void *d_in, void *d_out, hipStream_t st, ChunkStage &g, Front front)
{
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		front(cv);
		g.cols = cv.take<uint64_t>(cols.size());
		g.decode = cv.take<int32_t>(n_dec + 1);
		return ReadUp{ g.cols, cols.size() * sizeof(uint64_t) };
	}, s));
	memcpy(s.h, cols.data(), s.up.bytes);
	LDA_OK_TRY(read_send(d, s, st));
	for (size_t a = 0; a < CHUNK_DCOLS; a++)
		g.dcol[a] = g.cols + a * n_dec;
	g.ws = s.ws;
	g.in = d_in ? (const uint8_t *)d_in : s.ws;
	g.out = d_out ? (uint8_t *)d_out : s.ws;
	return LIBDEFLATE_AMD_OK;
}

/* the scratch rows, which stand first in the columns, into `rooms`, the d_out
 * rows behind them into d_out: one decompress batch per output base, each left
 * out when it has no row */
static inline int
chunk_inflate(struct libdeflate_decompressor *d, int format, const ChunkStage &g, size_t n_ws,
	      uint8_t *rooms, size_t n_out, hipStream_t st)
{
	for (int k = 0; k < 2; k++) {
		const size_t lo = k ? n_ws : 0, cnt = k ? n_out : n_ws;
		if (!cnt)
			continue;
		int rc = libdeflate_amd_decompress_batch(d, format, cnt, g.in, g.dcol[CHUNK_D_IN_OFF] + lo,
							 g.dcol[CHUNK_D_IN_N] + lo, k ? g.out : rooms,
							 g.dcol[CHUNK_D_OUT_OFF] + lo,
							 g.dcol[CHUNK_D_OUT_N] + lo, g.decode + lo, NULL,
							 NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	return LIBDEFLATE_AMD_OK;
}

/* the n verdict words at verd_at of the columns merged with the decoder's
 * results into d_results; the call's last launch */
static inline int chunk_verdicts(const ChunkStage &g, size_t n, uint64_t verd_at, int32_t *d_results,
				 hipStream_t st)
{
	hipLaunchKernelGGL(lda_shuf_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, (const uint64_t *)(g.cols + verd_at), (const int32_t *)g.decode,
			   d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

/* ---- the grids, 256 threads a workgroup ---- */

/* kernels that give every entry a wave, four to a workgroup: sixteen
 * workgroups fill a CU's wave slots, and the grid strides over what is beyond */
static inline unsigned wave_grid(const DeviceCtx *ctx, size_t n)
{
	return (unsigned)std::max((size_t)1, std::min((n + 3) / 4, (size_t)ctx->num_cus * 16));
}

/* kernels whose workgroups stride over tiles: eight to a CU fill its wave
 * slots.  No tile, no launch: the callers see to that */
static inline unsigned tile_grid(const DeviceCtx *ctx, uint64_t tiles)
{
	return (unsigned)std::min(tiles, (uint64_t)ctx->num_cus * 8);
}

/* the same over the chunks of a copy, which is launched for none as well */
static inline unsigned copy_grid(const DeviceCtx *ctx, uint64_t n)
{
	return std::max(1u, tile_grid(ctx, n));
}

/* ---- host_zip.hip, for host_zip_large.hip too ---- */

/* a selection's entries over the ZIP_COLS columns col[] of n words: ONE
 * decompress batch, lda_zip_copy_kernel for the stored ones - and behind it
 * for the n_pieces chunks (src, dst, len) of the large path -, ONE CRC-32
 * batch over the places */
int zip_read_entries(struct libdeflate_decompressor *d, size_t n, const uint64_t *const *col,
		     int32_t *g_res, uint64_t *g_ain, uint32_t *g_crc, const uint8_t *in, uint8_t *out,
		     hipStream_t st, size_t n_pieces = 0, const uint64_t *pc_src = NULL,
		     const uint64_t *pc_dst = NULL, const uint64_t *pc_len = NULL);

} /* namespace lda */

#endif /* LDA_HOST_READ_PLAN_H */
