/*
 * host_shuffle_write.hip - C-ABI of writing byte-shuffled deflate chunks (HDF5,
 * NetCDF-4, Zarr) in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_shuffle_compress_batch).
 *
 * shuffle_plan.h checks the rows, gives every chunk a room for its shuffled
 * bytes in the object's scratch and cuts the rooms into pieces; its columns go
 * up; lda_shuffle_kernel (shuffle_kernels.hip) fills the rooms from the raw
 * bytes in d_in - identity and NO_SHUFFLE chunks are copied there as element
 * size 1, because the piece pipeline compresses from one source base -; ONE
 * Adler-32 (zlib) or CRC-32 (gzip) batch runs over the pieces in the rooms, the
 * pieces are compressed into slots (the shared piece pipeline,
 * host_write_pieces.hip), and the kernels of shuffle_kernels.hip size the
 * streams and place headers and footers.
 * c->zipw: [chunk columns, kernel rows][piece columns][seg_info] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize][sum]
 * [sums][rooms].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "shuffle_plan.h"

using namespace lda;

/* the stages of a call; the benchmark times each alone (lda_shuffle_write_stages) */
enum { SHUFW_STAGE_SHUFFLE = 1, SHUFW_STAGE_COMPRESS = 2, SHUFW_STAGE_ASSEMBLE = 4, SHUFW_STAGE_ALL = 7 };

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_shuffle_compress_bound(struct libdeflate_compressor *c, int format, size_t n_chunks,
				      const uint64_t *chunks)
{
	(void)c;	/* (no level has another bound: libdeflate_<format>_compress_bound()) */
	if (n_chunks && !chunks) {
		set_error("shuffle_compress_bound: NULL argument");
		return 0;
	}
	return (size_t)shuf_bound(format, n_chunks, chunks);
}

struct ShufwScratch : PiecesScratch {
	uint64_t *ecols, *csize;
	uint32_t *sum, *sums;
	uint8_t *rooms;
	size_t bytes;
};

static ShufwScratch shufw_scratch(void *base, const shuf_write_plan &p)
{
	ShufwScratch s;
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

static int shufw_enqueue(struct libdeflate_compressor *c, int format, const shuf_write_plan &p,
			 const uint8_t *d_in, uint8_t *d_out, uint64_t out_avail, uint64_t *d_result,
			 uint64_t *d_index, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np, n_u = (size_t)p.n_u;
	const ShufwScratch sz = shufw_scratch(NULL, p);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const ShufwScratch s = shufw_scratch(ws, p), hs = shufw_scratch(h, p);
	if (sz.up_bytes && !p.ecols.empty())
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *ecol[SHUFW_ECOLS], *ucol[SHUF_UCOLS], *const *pcol = s.pcol;
	for (size_t a = 0; a < SHUFW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;
	for (size_t a = 0; a < SHUF_UCOLS; a++)
		ucol[a] = s.ecols + SHUFW_ECOLS * n + a * n_u;

	if (p.tiles && (stages & SHUFW_STAGE_SHUFFLE)) {
		hipLaunchKernelGGL(lda_shuffle_kernel, dim3(tile_grid(ctx, p.tiles)), dim3(256), 0, st,
				   (uint64_t)n_u, p.tiles, ucol[SHUF_U_TILE_END], ucol[SHUF_U_SRC], ucol[SHUF_U_DST],
				   ucol[SHUF_U_GEOM], d_in, s.rooms);
	}
	int rc = LIBDEFLATE_AMD_OK;
	if ((stages & SHUFW_STAGE_COMPRESS) && format == LIBDEFLATE_AMD_ZLIB)
		rc = libdeflate_amd_adler32_batch(np, s.rooms, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						  NULL, s.sums, st);
	else if ((stages & SHUFW_STAGE_COMPRESS) && format == LIBDEFLATE_AMD_GZIP)
		rc = libdeflate_amd_crc32_batch(np, s.rooms, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						NULL, s.sums, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	if (stages & SHUFW_STAGE_COMPRESS)
		LDA_OK_TRY(pieces_compress(c, s, launches, s.rooms, st));
	if (!(stages & SHUFW_STAGE_ASSEMBLE)) {
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	const unsigned grid = wave_grid(ctx, n);
	if (n)
		hipLaunchKernelGGL(lda_shufw_chunk_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   format, ecol[SHUFW_E_FIRST], ecol[SHUFW_E_COUNT], ecol[SHUFW_E_USIZE],
				   pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], (const uint64_t *)s.out_n,
				   (const uint32_t *)s.sums, s.csize, s.sum, s.sizes);
	/* (of no chunks, the total alone: 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_shufw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   format, c->level, out_avail, (const uint64_t *)s.ecols,
				   pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], pcol[ZIPW_P_SLOT_OFF],
				   (const uint64_t *)s.out_n, (const uint64_t *)s.csize,
				   (const uint32_t *)s.sum, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst, s.cp_len,
				   d_index);
	pieces_copy(ctx, s, np, total_at, out_avail, 0, d_in, d_out, st);
	hipLaunchKernelGGL(lda_shufw_final_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n, p.raw_total,
			   out_avail, total_at, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int shufw_call(const char *what, struct libdeflate_compressor *c, int format, size_t n_chunks,
		      const uint64_t *chunks, const void *d_in, size_t in_avail, void *d_out,
		      size_t out_avail, uint64_t *d_result, uint64_t *d_index, unsigned stages,
		      void *stream)
{
	if (!c || !d_out || !d_result || (!d_in && in_avail) || (n_chunks && !chunks)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!shuf_check(format, n_chunks, chunks, false, 0, in_avail, c->level, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (level 0 too: its stored blocks are the compress kernel's) */
		const zipw_params pr = pieces_params(c, false);
		shuf_write_plan p;
		shuf_write_plan_build(pr, n_chunks, chunks, p);
		return shufw_enqueue(c, format, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail,
				     d_result, d_index, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_shuffle_compress_batch(struct libdeflate_compressor *c, int format, size_t n_chunks,
				      const uint64_t *chunks, const void *d_in, size_t in_avail,
				      void *d_out, size_t out_avail, uint64_t *d_result,
				      uint64_t *d_index, void *stream)
{
	return shufw_call("shuffle_compress_batch", c, format, n_chunks, chunks, d_in, in_avail, d_out,
			  out_avail, d_result, d_index, SHUFW_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 the shuffle kernel, 2 checksums and compress, 4 the assembly), so
 * that tools/bench_shuffle.py can time each alone on scratch an earlier full
 * call has filled */
extern "C" LIBDEFLATEAPI int
lda_shuffle_write_stages(struct libdeflate_compressor *c, int format, size_t n_chunks,
			 const uint64_t *chunks, const void *d_in, size_t in_avail, void *d_out,
			 size_t out_avail, uint64_t *d_result, uint64_t *d_index, unsigned stages,
			 void *stream)
{
	return shufw_call("shuffle_write_stages", c, format, n_chunks, chunks, d_in, in_avail, d_out,
			  out_avail, d_result, d_index, stages & SHUFW_STAGE_ALL, stream);
}
