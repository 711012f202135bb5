/*
 * host_exr_write.hip - C-ABI of writing OpenEXR ZIP and ZIPS chunks, scanline
 * blocks and tiles, in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_exr_encode_batch).
 *
 * exr_plan.h checks the rows, gives every chunk a room in each of two areas of
 * the object's scratch - raw and coded, at the same offset - and cuts the
 * coded rooms into pieces; its columns go up; lda_exr_gather_kernel
 * (exr_kernels.hip) collects every chunk's lines or pixels from d_in into its
 * raw room and lda_exr_code_kernel codes the raw room into the coded room; ONE
 * Adler-32 batch runs over the pieces in the coded rooms, the pieces are
 * compressed into slots (the shared piece pipeline, host_write_pieces.hip) and
 * the shuffle writer's lda_shufw_chunk_kernel (format zlib) sizes the streams;
 * lda_exrw_choose_kernel keeps a stream where it is shorter than its raw
 * chunk, the sizes are scanned, and lda_exrw_place_kernel writes heads, zlib
 * headers and footers and the reader's rows and lists the copies: of a kept
 * stream from the slots, of a raw chunk the same ranges of the raw area, which
 * is what lda_zipw_copy_kernel reads as its source.
 * c->zipw: [chunk and layout columns][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize]
 * [dsize][sum][sums][raw rooms][coded rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "exr_plan.h"

using namespace lda;

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_exr_encode_bound(struct libdeflate_compressor *c, size_t n_chunks, const uint64_t *rows)
{
	(void)c;	/* (no level has another bound: a chunk is never written longer than raw) */
	if (n_chunks && !rows) {
		set_error("exr_encode_bound: NULL argument");
		return 0;
	}
	return (size_t)exr_bound(n_chunks, rows);
}

struct ExrwScratch : PiecesScratch {
	uint64_t *ecols, *csize, *dsize;
	uint32_t *sum, *sums;
	uint8_t *raw, *coded;
	size_t bytes;
};

static ExrwScratch exrw_scratch(void *base, const exr_write_plan &p)
{
	ExrwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.ecols = c.take<uint64_t>(p.ecols.size());
	pieces_carve(c, p, n, 0, s);
	s.csize = c.take<uint64_t>(n);
	s.dsize = c.take<uint64_t>(n);
	s.sum = c.take<uint32_t>(n);
	s.sums = c.take<uint32_t>(np);
	s.raw = c.take<uint8_t>((size_t)p.rooms_bytes + 64, 256);
	s.coded = c.take<uint8_t>((size_t)p.rooms_bytes + 64, 256);
	s.bytes = c.at + 16;
	return s;
}

static int exrw_enqueue(struct libdeflate_compressor *c, const exr_write_plan &p, const uint8_t *d_in,
			uint8_t *d_out, uint64_t out_avail, uint64_t *d_result, uint64_t *d_index,
			hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np;
	const ExrwScratch sz = exrw_scratch(NULL, p);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const ExrwScratch s = exrw_scratch(ws, p), hs = exrw_scratch(h, p);
	memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *ecol[EXRW_ECOLS], *const *pcol = s.pcol;
	for (size_t a = 0; a < EXRW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;

	hipLaunchKernelGGL(lda_exr_gather_kernel, dim3(tile_grid(ctx, p.ltiles)), dim3(256), 0, st,
			   (uint64_t)n, p.ltiles, (const uint64_t *)(s.ecols + p.l_at), d_in, s.raw);
	hipLaunchKernelGGL(lda_exr_code_kernel, dim3(tile_grid(ctx, p.ctiles)), dim3(256), 0, st,
			   (uint64_t)n, p.ctiles, (const uint64_t *)s.ecols, (const uint8_t *)s.raw,
			   s.coded);
	LDA_OK_TRY(libdeflate_amd_adler32_batch(np, s.coded, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						NULL, s.sums, st));
	LDA_OK_TRY(pieces_compress(c, s, launches, s.coded, st));
	const unsigned grid = wave_grid(ctx, n);
	hipLaunchKernelGGL(lda_shufw_chunk_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
			   (int)LIBDEFLATE_AMD_ZLIB, ecol[EXRW_E_FIRST], ecol[EXRW_E_COUNT],
			   ecol[EXRW_E_USIZE], pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
			   (const uint64_t *)s.out_n, (const uint32_t *)s.sums, s.csize, s.sum, s.sizes);
	hipLaunchKernelGGL(lda_exrw_choose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
			   (uint64_t)n, (const uint64_t *)s.ecols, s.dsize, s.sizes);
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	hipLaunchKernelGGL(lda_exrw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n, c->level,
			   out_avail, (const uint64_t *)s.ecols, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
			   pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n, (const uint64_t *)s.csize,
			   (const uint32_t *)s.sum, (const uint64_t *)s.dsize, (const uint64_t *)s.offs,
			   (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst, s.cp_len, d_index);
	/* (a raw chunk's pieces are read from the raw area: the copy kernel's `in`) */
	pieces_copy(ctx, s, np, total_at, out_avail, 0, s.raw, d_out, st);
	hipLaunchKernelGGL(lda_shufw_final_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n, p.raw_total,
			   out_avail, total_at, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_exr_encode_batch(struct libdeflate_compressor *c, size_t n_chunks, const uint64_t *rows,
				const void *d_in, size_t in_avail, void *d_out, size_t out_avail,
				uint64_t *d_result, uint64_t *d_index, void *stream)
{
	const char *what = "exr_encode_batch";

	if (!c || !d_out || !d_result || (!d_in && in_avail) || (n_chunks && !rows)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!exr_check(n_chunks, rows, false, 0, in_avail, c->level, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		if (n_chunks == 0)	/* nothing to do: d_result is not written either */
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (level 0 too: its stored blocks are longer than raw, so every chunk goes raw) */
		const zipw_params pr = pieces_params(c, false);
		exr_write_plan p;
		exr_write_plan_build(pr, n_chunks, rows, p);
		return exrw_enqueue(c, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result,
				    d_index, (hipStream_t)stream);
	});
}
