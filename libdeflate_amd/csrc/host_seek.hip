/*
 * host_seek.hip - a seek index over ONE plain DEFLATE / zlib / gzip stream in
 * device memory, and ranged reads through it (the counterpart of
 * host_bgzf_read.hip for streams without member boundaries).
 *
 * The many-wave decoder (host_stream.hip) proves every chunk's exact start
 * bit, governing block header and output offset; its decode kernel decodes a
 * chunk from such a state into 16-bit symbols in which everything in front of
 * the chunk is a marker into "the 32 KiB in front of the chunk".  So a POINT
 * of the index is a chunk descriptor of the accepted chain plus 32 KiB copied
 * from the output, and a read decodes the intervals (point to point) its
 * ranges touch, each against its own stored window: no window chain, no block
 * finder, no host round trip.  The arithmetic is seek_plan.h's.
 */
#include <string.h>
#include <algorithm>
#include <vector>

#include "host_objects.h"
#include "stream_kernels.h"
#include "seek_plan.h"

static_assert(LDA_SEEK_ROW == LIBDEFLATE_AMD_SEEK_WORDS && LDA_SEEK_WIN == LIBDEFLATE_AMD_SEEK_WINDOW,
	      "seek_plan.h restates libdeflate_amd.h");

namespace lda {

/* interval k of pts[] as a chunk: from the point's state up to the next
 * point's start bit (the last: to the end of the raw stream) */
static lda_stream_chunk interval_chunk(uint64_t hdr_bit, uint64_t start_bit, uint32_t kind,
				       uint64_t limit_bit, uint64_t slot)
{
	lda_stream_chunk c = {};
	c.hdr_bit = hdr_bit;
	c.start_bit = c.target_bit = start_bit;
	c.limit_bit = limit_bit;
	c.out_off = slot;
	c.kind = kind;
	return c;
}

/*
 * The build's check: every interval counted once by lda_stream_count_kernel
 * from its point's own descriptor; it must end exactly at the next point - the
 * same bit, the same kind of state - with exactly the bytes between.  Points
 * that fail leave (seek_drop_failed()) and the merged intervals are counted
 * again: one launch per round, until nothing fails or point 0 is alone (its
 * interval to the end is the stream the call has just decoded).
 */
static bool verify_points(struct libdeflate_decompressor *d, const uint8_t *d_raw,
			  const seek_export &x, std::vector<seek_link> &pts)
{
	hipStream_t sc = d->streams.comp;
	std::vector<uint8_t> recount(pts.size(), 1);
	while (pts.size() > 1) {
		const size_t n = pts.size();
		std::vector<uint32_t> which;
		for (size_t k = 0; k < n; k++)
			if (recount[k])
				which.push_back((uint32_t)k);
		const size_t nw = which.size();
		if (!nw)
			break;
		const size_t res_at = align_up(nw * sizeof(lda_stream_chunk), 64);
		const size_t bytes = res_at + nw * sizeof(lda_stream_res);
		uint8_t *dv = (uint8_t *)d->seek.reserve(bytes + 64);
		uint8_t *h = (uint8_t *)d->meta.ensure(bytes + 64);
		if (!dv || !h)
			return false;
		lda_stream_chunk *hc = (lda_stream_chunk *)h;
		for (size_t i = 0; i < nw; i++) {
			const size_t k = which[i];
			hc[i] = interval_chunk(pts[k].hdr_bit, pts[k].start_bit, pts[k].kind,
					       k + 1 < n ? pts[k + 1].start_bit : 8 * x.raw_nbytes, 0);
		}
		LDA_TRY(hipMemcpyAsync(dv, h, nw * sizeof(lda_stream_chunk), hipMemcpyHostToDevice, sc));
		if (!launch_count(sc, (uint32_t)nw, (const lda_stream_chunk *)dv,
				  (lda_stream_res *)(dv + res_at), d_raw, x.raw_nbytes))
			return false;
		LDA_TRY(hipMemcpyAsync(h + res_at, dv + res_at, nw * sizeof(lda_stream_res),
				       hipMemcpyDeviceToHost, sc));
		LDA_TRY(hipStreamSynchronize(sc));
		const lda_stream_res *hr = (const lda_stream_res *)(h + res_at);
		std::vector<uint8_t> failed(n, 0);
		bool any = false;
		for (size_t i = 0; i < nw; i++) {
			const size_t k = which[i];
			const lda_stream_res &r = hr[i];
			const bool last = k + 1 == n;
			const uint64_t nbytes = (last ? x.total : pts[k + 1].out_off) - pts[k].out_off;
			bool ok = r.nout == nbytes && !(r.flags & LDA_RES_BAD_DIST);
			if (last) {
				ok = ok && r.status == LDA_STREAM_FINAL && (r.end_bit + 7) / 8 == x.raw_nbytes;
			} else {
				const seek_link &nx = pts[k + 1];
				const bool bnd = r.flags & LDA_RES_BOUNDARY;
				ok = ok && r.status == LDA_STREAM_OK && r.end_bit == nx.start_bit &&
				     bnd == (nx.kind == LDA_CHUNK_HEADER) && (bnd || r.end_hdr_bit == nx.hdr_bit);
			}
			failed[k] = !ok;
			any = any || !ok;
		}
		if (!any)
			break;
		if (!seek_drop_failed(pts, failed, recount))
			break;
	}
	return true;
}

static enum libdeflate_result
index_body(struct libdeflate_decompressor *d, int format, const uint8_t *d_in, size_t in_nbytes,
	   uint8_t *d_out, size_t out_avail, size_t *actual_in_ret, size_t *actual_out_ret,
	   size_t spacing, uint64_t *index, size_t index_avail, size_t *points_ret,
	   uint8_t *d_windows, size_t windows_avail, hipStream_t user)
{
	const char *what = "libdeflate_amd_decompress_large_index";
	seek_export x;
	size_t ain = 0, aout = 0;
	*points_ret = 0;
	const enum libdeflate_result res =
		decompress_large_body(d, format, d_in, in_nbytes, d_out, out_avail, &ain,
				      actual_out_ret ? &aout : NULL, user, what, &x);
	if (res != LIBDEFLATE_SUCCESS)
		return res;
	auto failed = [&](int rc) {
		complain(what, rc);
		return LIBDEFLATE_BAD_DATA;	/* a library-side failure, as everywhere */
	};
	if (!x.known || x.chain.empty()) {
		set_error("%s: the stream's container header could not be read back for the index", what);
		return failed(LIBDEFLATE_AMD_BAD_ARG);
	}
	DeviceGuard on(d->device);
	if (!on.ok() || !device_ctx())
		return failed(LIBDEFLATE_AMD_NO_DEVICE);
	hipStream_t sc = d->streams.comp;
	const size_t capacity = seek_capacity(index_avail, windows_avail);
	std::vector<seek_link> pts;
	for (size_t i : seek_thin(x.chain, x.total, spacing, capacity, NULL))
		pts.push_back(x.chain[i]);
	if (!verify_points(d, d_in + x.raw_off, x, pts))
		return failed(LIBDEFLATE_AMD_NO_DEVICE);
	/* the windows: the 32 KiB of output in front of every point */
	const size_t n = pts.size();
	uint64_t *h = (uint64_t *)d->meta.ensure(n * 8 + 64);
	uint64_t *dv = (uint64_t *)d->seek.reserve(n * 8 + 64);
	if (!h || !dv)
		return failed(LIBDEFLATE_AMD_OOM);
	for (size_t k = 0; k < n; k++)
		h[k] = pts[k].out_off;
	if (hipMemcpyAsync(dv, h, n * 8, hipMemcpyHostToDevice, sc) != hipSuccess)
		return failed(LIBDEFLATE_AMD_NO_DEVICE);
	hipLaunchKernelGGL(lda_seek_window_kernel, dim3((unsigned)n), dim3(256), 0, sc, (uint32_t)n,
			   (const uint64_t *)dv, (const uint8_t *)d_out, d_windows);
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sc) != hipSuccess) {
		set_error("%s: %s", what, hipGetErrorString(hipGetLastError()));
		return failed(LIBDEFLATE_AMD_NO_DEVICE);
	}
	seek_write_index(index, format, x, pts);
	*points_ret = n;
	if (actual_in_ret)
		*actual_in_ret = ain;
	if (actual_out_ret)
		*actual_out_ret = aout;
	return LIBDEFLATE_SUCCESS;
}

/* a bump allocator over one buffer: device and pinned copy share the layout */
struct Lay {
	size_t at = 0;
	size_t take(size_t bytes)
	{
		const size_t a = at;
		at = align_up(at + bytes, 64);
		return a;
	}
};

static int read_body(struct libdeflate_decompressor *d, const uint8_t *d_in, const seek_view &v,
		     const seek_read_plan &pl, const uint8_t *d_windows, size_t n_ranges,
		     uint8_t *d_out, int32_t *d_results, hipStream_t st)
{
	const size_t N = pl.iv.size(), P = pl.pieces.size();
	const size_t BATCH = STREAM_DECODE_BATCH;
	Lay lay;
	const size_t chunks_at = lay.take(N * sizeof(lda_stream_chunk));
	const size_t want_at = lay.take(2 * N * 8);
	const size_t winof_at = lay.take(N * 8);
	const size_t pieces_at = lay.take(4 * P * 8);
	const size_t first_at = lay.take((n_ranges + 1) * 8);
	const size_t lowest_at = lay.take(N * 4);
	const size_t fail_at = lay.take(N * 4);
	const size_t up_bytes = lay.at;
	const size_t counted_at = lay.take(N * sizeof(lda_stream_res));
	const size_t res_at = lay.take(N * sizeof(lda_stream_res));
	LDA_OK_TRY(d->seek_up.begin());
	uint8_t *ws = (uint8_t *)d->seek.reserve(lay.at + 64);
	uint8_t *h = (uint8_t *)d->seek_up.pinned(up_bytes + 64);
	uint16_t *d_sym = N ? (uint16_t *)d->ssym.reserve((size_t)pl.sym_words * 2 + 64) : nullptr;
	uint32_t *d_tok = N ? stream_token_scratch(d, N) : nullptr;
	if (!ws || !h || (N && (!d_sym || !d_tok)))
		return LIBDEFLATE_AMD_OOM;
	memset(h, 0, up_bytes);
	lda_stream_chunk *hc = (lda_stream_chunk *)(h + chunks_at);
	uint64_t *hwant = (uint64_t *)(h + want_at), *hwin = (uint64_t *)(h + winof_at);
	uint64_t *hp = (uint64_t *)(h + pieces_at), *hf = (uint64_t *)(h + first_at);
	uint32_t *hlow = (uint32_t *)(h + lowest_at);
	for (size_t j = 0; j < N; j++) {
		const seek_interval &iv = pl.iv[j];
		const bool last = iv.k + 1 == v.n;
		hc[j] = interval_chunk(v.hdr_bit(iv.k), v.start_bit(iv.k), v.kind(iv.k),
				       last ? 8 * v.raw_nbytes : v.start_bit(iv.k + 1), iv.slot);
		hwant[2 * j] = last ? ((uint64_t)1 << 63) | v.raw_nbytes : v.start_bit(iv.k + 1);
		hwant[2 * j + 1] = iv.nbytes;
		hwin[j] = iv.k;
		hlow[j] = iv.out_off < LDA_SEEK_WIN ? LDA_SEEK_WIN - (uint32_t)iv.out_off : 0;
	}
	uint64_t longest = 0;
	for (size_t p = 0; p < P; p++) {
		const seek_piece &pc = pl.pieces[p];
		hp[4 * p] = (uint64_t)pc.interval | (uint64_t)pc.range << 32;
		hp[4 * p + 1] = pl.iv[pc.interval].slot + pc.src;
		hp[4 * p + 2] = pc.dst;
		hp[4 * p + 3] = pc.len;
		longest = std::max(longest, pc.len);
	}
	memcpy(hf, pl.first.data(), (n_ranges + 1) * 8);
	LDA_OK_TRY(d->seek_up.send(ws, up_bytes, st));
	const lda_stream_chunk *g_chunks = (const lda_stream_chunk *)(ws + chunks_at);
	lda_stream_res *g_counted = (lda_stream_res *)(ws + counted_at);
	lda_stream_res *g_res = (lda_stream_res *)(ws + res_at);
	const uint64_t *g_want = (const uint64_t *)(ws + want_at);
	const uint64_t *g_pieces = (const uint64_t *)(ws + pieces_at);
	uint32_t *g_fail = (uint32_t *)(ws + fail_at);
	const uint8_t *d_raw = d_in + v.raw_off;
	if (N) {
		/* count: nothing written but results */
		if (!launch_count(st, (uint32_t)N, g_chunks, g_counted, d_raw, v.raw_nbytes))
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* the gated decode, into the slots */
		for (size_t lo = 0; lo < N; lo += BATCH) {
			const uint32_t nk = (uint32_t)std::min(BATCH, N - lo);
			hipLaunchKernelGGL(lda_seek_decode_kernel, dim3(nk), dim3(64), lda_stream_chunk_lds(),
					   st, nk, g_chunks + lo, (const lda_stream_res *)g_counted + lo,
					   g_want + 2 * lo, g_res + lo, d_raw, v.raw_nbytes, d_sym, d_tok,
					   g_fail + lo);
		}
	}
	if (P) {
		/* (256 lanes x 8 bytes a step; grid.y <= 65535: batches of pieces) */
		const unsigned gx = (unsigned)std::min<uint64_t>(std::max<uint64_t>((longest + 2047) / 2048, 1), 64);
		for (size_t p0 = 0; p0 < P; p0 += 32768)
			hipLaunchKernelGGL(lda_seek_resolve_kernel,
					   dim3(gx, (unsigned)std::min<size_t>(32768, P - p0)), dim3(256), 0, st,
					   (uint32_t)P, (uint32_t)p0, g_pieces,
					   (const uint64_t *)(ws + winof_at), (const uint32_t *)(ws + lowest_at),
					   (const uint16_t *)d_sym, d_windows, d_out, g_fail);
	}
	hipLaunchKernelGGL(lda_seek_verdict_kernel, dim3((unsigned)((n_ranges + 255) / 256)), dim3(256),
			   0, st, (uint32_t)n_ranges, (const uint64_t *)(ws + first_at), g_pieces,
			   (const uint32_t *)g_fail, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

} /* namespace lda */

extern "C" LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_decompress_large_index(struct libdeflate_decompressor *d, int format,
				      const void *d_in, size_t in_nbytes, void *d_out,
				      size_t out_nbytes_avail, size_t *actual_in_nbytes_ret,
				      size_t *actual_out_nbytes_ret, size_t spacing, uint64_t *index,
				      size_t index_avail, size_t *points_ret, void *d_windows,
				      size_t windows_avail, void *stream)
{
	using namespace lda;
	const char *what = "libdeflate_amd_decompress_large_index";
	if (!d) {
		set_error("%s: NULL decompressor", what);
		return LIBDEFLATE_BAD_DATA;
	}
	if (!d_in && in_nbytes) {
		set_error("%s: NULL d_in with in_nbytes != 0", what);
		return LIBDEFLATE_BAD_DATA;
	}
	if (!d_out && out_nbytes_avail) {
		set_error("%s: NULL d_out with out_nbytes_avail != 0", what);
		return LIBDEFLATE_BAD_DATA;
	}
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB &&
	    format != LIBDEFLATE_AMD_GZIP) {
		set_error("%s: format %d is not DEFLATE, zlib or gzip", what, format);
		return LIBDEFLATE_BAD_DATA;
	}
	if (!index || !points_ret || !d_windows) {
		set_error("%s: NULL %s", what, !index ? "index" : !points_ret ? "points_ret" : "d_windows");
		return LIBDEFLATE_BAD_DATA;
	}
	if (spacing == 0) {
		set_error("%s: spacing is 0", what);
		return LIBDEFLATE_BAD_DATA;
	}
	if (seek_capacity(index_avail, windows_avail) < 1) {
		set_error("%s: a capacity of no point: index_avail %zu (4 (points + 2) entries), "
			  "windows_avail %zu (32768 bytes per point)", what, index_avail, windows_avail);
		return LIBDEFLATE_BAD_DATA;
	}
	return no_unwind(what, LIBDEFLATE_BAD_DATA, [&]() {
		return index_body(d, format, (const uint8_t *)d_in, in_nbytes, (uint8_t *)d_out,
				  out_nbytes_avail, actual_in_nbytes_ret, actual_out_nbytes_ret, spacing,
				  index, index_avail, points_ret, (uint8_t *)d_windows, windows_avail,
				  (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_seek_read_batch(struct libdeflate_decompressor *d, const void *d_in,
			       size_t in_nbytes, const uint64_t *index, size_t index_words,
			       const void *d_windows, size_t n_ranges, const uint64_t *ranges,
			       void *d_out, size_t out_avail, int32_t *d_results, void *stream)
{
	using namespace lda;
	const char *what = "seek_read_batch";
	if (!d || !d_in || !index || !d_windows || (n_ranges && (!ranges || !d_results))) {
		set_error("%s: NULL argument (%s)", what,
			  !d ? "decompressor" : !d_in ? "d_in" : !index ? "index" :
			  !d_windows ? "d_windows" : !ranges ? "ranges" : "d_results");
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		seek_view v;
		std::string why = seek_check_index(index, index_words, in_nbytes, &v);
		seek_read_plan pl;
		if (why.empty())
			why = seek_plan_ranges(v, n_ranges, ranges, out_avail, &pl);
		if (why.empty() && pl.out_bytes && !d_out)
			why = "NULL argument (d_out)";
		if (!why.empty()) {
			set_error("%s: %s", what, why.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_ranges == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return read_body(d, (const uint8_t *)d_in, v, pl, (const uint8_t *)d_windows, n_ranges,
				 (uint8_t *)d_out, d_results, (hipStream_t)stream);
	});
}
