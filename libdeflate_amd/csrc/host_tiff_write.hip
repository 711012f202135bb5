/*
 * host_tiff_write.hip - C-ABI of writing predictor-coded deflate strips and
 * tiles (TIFF, GeoTIFF) in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_tiff_encode_batch).
 *
 * tiff_plan.h checks the rows, gives every segment a room for its predicted
 * bytes in the object's scratch and cuts the rooms into pieces; its columns go
 * up; lda_tiff_predict_kernel (tiff_kernels.hip) fills the rooms from the raw
 * pixels in d_in - the kept rectangle, zero samples up to the coded size -;
 * ONE Adler-32 batch runs over the pieces in the rooms, the pieces are
 * compressed into slots (the shared piece pipeline, host_write_pieces.hip),
 * and the shuffle writer's kernels (shuffle_kernels.hip, format zlib) size the
 * streams and place headers and footers; lda_tiffw_index_kernel writes the
 * reader's rows.
 * c->zipw: [segment columns][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize][sum]
 * [sums][rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "tiff_plan.h"

using namespace lda;

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_tiff_encode_bound(struct libdeflate_compressor *c, size_t n_segments,
				 const uint64_t *rows)
{
	(void)c;	/* (no level has another bound: libdeflate_zlib_compress_bound()) */
	if (n_segments && !rows) {
		set_error("tiff_encode_bound: NULL argument");
		return 0;
	}
	return (size_t)tiff_bound(n_segments, rows);
}

struct TiffwScratch : PiecesScratch {
	uint64_t *ecols, *csize;
	uint32_t *sum, *sums;
	uint8_t *rooms;
	size_t bytes;
};

static TiffwScratch tiffw_scratch(void *base, const tiff_write_plan &p)
{
	TiffwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.ecols = c.take<uint64_t>(p.ecols.size());
	pieces_carve(c, p, n, 0, s);
	s.csize = c.take<uint64_t>(n);
	s.sum = c.take<uint32_t>(n);
	s.sums = c.take<uint32_t>(np);
	s.rooms = c.take<uint8_t>((size_t)p.rooms_bytes + 64, 256);
	s.bytes = c.at + 16;
	return s;
}

static int tiffw_enqueue(struct libdeflate_compressor *c, const tiff_write_plan &p, const uint8_t *d_in,
			 uint8_t *d_out, uint64_t out_avail, uint64_t *d_result, uint64_t *d_index,
			 hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np;
	const TiffwScratch sz = tiffw_scratch(NULL, p);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const TiffwScratch s = tiffw_scratch(ws, p), hs = tiffw_scratch(h, p);
	if (sz.up_bytes && !p.ecols.empty())
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *ecol[TIFFW_ECOLS], *const *pcol = s.pcol;
	for (size_t a = 0; a < TIFFW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;

	if (p.tiles)
		hipLaunchKernelGGL(lda_tiff_predict_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n, p.tiles, (const uint64_t *)s.ecols, d_in, s.rooms);
	LDA_OK_TRY(libdeflate_amd_adler32_batch(np, s.rooms, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						NULL, s.sums, st));
	LDA_OK_TRY(pieces_compress(c, s, launches, s.rooms, st));
	const unsigned grid = wave_grid(ctx, n);
	if (n)
		hipLaunchKernelGGL(lda_shufw_chunk_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   (int)LIBDEFLATE_AMD_ZLIB, ecol[TIFFW_E_FIRST], ecol[TIFFW_E_COUNT],
				   ecol[TIFFW_E_USIZE], pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
				   (const uint64_t *)s.out_n, (const uint32_t *)s.sums, s.csize, s.sum,
				   s.sizes);
	/* (of no segments, the total alone: 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n) {
		/* (its index rows are the shuffle calls': ours come from lda_tiffw_index_kernel) */
		hipLaunchKernelGGL(lda_shufw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   (int)LIBDEFLATE_AMD_ZLIB, c->level, out_avail, (const uint64_t *)s.ecols,
				   pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], pcol[ZIPW_P_SLOT_OFF],
				   (const uint64_t *)s.out_n, (const uint64_t *)s.csize,
				   (const uint32_t *)s.sum, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst, s.cp_len,
				   (uint64_t *)NULL);
		if (d_index)
			hipLaunchKernelGGL(lda_tiffw_index_kernel, dim3((unsigned)((n + 255) / 256)),
					   dim3(256), 0, st, (uint64_t)n, out_avail,
					   (const uint64_t *)s.ecols, (const uint64_t *)s.csize,
					   (const uint64_t *)s.offs, (const uint64_t *)s.bsum, d_index);
	}
	pieces_copy(ctx, s, np, total_at, out_avail, 0, d_in, d_out, st);
	hipLaunchKernelGGL(lda_shufw_final_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n, p.raw_total,
			   out_avail, total_at, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tiff_encode_batch(struct libdeflate_compressor *c, size_t n_segments,
				 const uint64_t *rows, const void *d_in, size_t in_avail, void *d_out,
				 size_t out_avail, uint64_t *d_result, uint64_t *d_index, void *stream)
{
	const char *what = "tiff_encode_batch";

	if (!c || !d_out || !d_result || (!d_in && in_avail) || (n_segments && !rows)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!tiff_check(n_segments, rows, false, 0, in_avail, c->level, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_segments == 0)	/* nothing to do: d_result is not written either */
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (level 0 too: its stored blocks are the compress kernel's) */
		const zipw_params pr = pieces_params(c, false);
		tiff_write_plan p;
		tiff_write_plan_build(pr, n_segments, rows, p);
		return tiffw_enqueue(c, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result,
				     d_index, (hipStream_t)stream);
	});
}
