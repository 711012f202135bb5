/*
 * host_gzip_members_write.hip - C-ABI of writing a file of concatenated gzip
 * members in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_gzip_members_compress_batch).
 *
 * gzip_members_write_plan.h checks the host arrays and cuts the records into
 * pieces; its columns and the names go up, ONE CRC-32 batch runs over the
 * pieces, the pieces are compressed into slots (the shared piece pipeline,
 * host_write_pieces.hip), and the kernels of gzip_members_write_kernels.hip
 * size the members and place header, name and footer.
 * c->zipw: [record columns][piece columns][seg_info][names] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize][crc]
 * [crcs].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "gzip_members_write_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_GZMW_RESULT_WORDS == GZMW_RESULT_WORDS &&
	      GZMW_NAME_MAX + 2 == LIBDEFLATE_AMD_GZM_NAME_MAX &&
	      GZMW_MAX_RECORDS == (uint64_t)1 << 28,
	      "gzip_members_write_plan.h holds copies of the header's constants");

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_gzip_members_compress_bound(struct libdeflate_compressor *c, size_t n_records,
					   const uint64_t *name_offsets, const uint64_t *in_nbytes)
{
	(void)c;	/* (no level has another bound: libdeflate_gzip_compress_bound()) */
	if (n_records && !in_nbytes) {
		set_error("gzip_members_compress_bound: NULL argument");
		return 0;
	}
	return (size_t)gzmw_bound(n_records, name_offsets, in_nbytes);
}

struct GzmwScratch : PiecesScratch {
	uint64_t *ecols, *csize;
	uint32_t *crc, *crcs;
	size_t bytes;
};

static GzmwScratch gzmw_scratch(void *base, const gzmw_plan &p)
{
	GzmwScratch s;
	Carve c(base);

	s.ecols = c.take<uint64_t>(GZMW_ECOLS * (size_t)p.n);
	pieces_carve(c, p, (size_t)p.n, (size_t)p.names_bytes, s);
	s.csize = c.take<uint64_t>((size_t)p.n);
	s.crc = c.take<uint32_t>((size_t)p.n);
	s.crcs = c.take<uint32_t>((size_t)p.np);
	s.bytes = c.at + 16;
	return s;
}

static int gzmw_enqueue(struct libdeflate_compressor *c, const gzmw_plan &p, const uint8_t *names,
			const uint8_t *d_in, uint8_t *d_out, uint64_t out_avail, uint64_t *d_result,
			uint64_t *d_index, uint32_t mtime, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np;
	const GzmwScratch sz = gzmw_scratch(NULL, p);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const GzmwScratch s = gzmw_scratch(ws, p), hs = gzmw_scratch(h, p);
	if (sz.up_bytes) {
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
		if (p.names_bytes)
			memcpy(hs.behind, names, (size_t)p.names_bytes);
	}
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *ecol[GZMW_ECOLS], *const *pcol = s.pcol;
	for (size_t a = 0; a < GZMW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;

	int rc = libdeflate_amd_crc32_batch(np, d_in, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], NULL,
					    s.crcs, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	LDA_OK_TRY(pieces_compress(c, s, launches, d_in, st));
	const unsigned grid = wave_grid(ctx, n);
	if (n)
		hipLaunchKernelGGL(lda_gzmw_member_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   ecol[GZMW_E_FIRST], ecol[GZMW_E_COUNT], ecol[GZMW_E_NAME_LEN],
				   ecol[GZMW_E_USIZE], pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
				   (const uint64_t *)s.out_n, (const uint32_t *)s.crcs, s.csize, s.crc,
				   s.sizes);
	/* (of no records, the total alone: a file of 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_gzmw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   c->level, mtime, out_avail, ecol[GZMW_E_FIRST], ecol[GZMW_E_COUNT],
				   ecol[GZMW_E_NAME_OFF], ecol[GZMW_E_NAME_LEN], ecol[GZMW_E_USIZE],
				   ecol[GZMW_E_UOFF], (const uint8_t *)s.behind, pcol[ZIPW_P_PC_OFF],
				   pcol[ZIPW_P_PC_N], pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n,
				   (const uint64_t *)s.csize, (const uint32_t *)s.crc,
				   (const uint64_t *)s.offs, (const uint64_t *)s.bsum, d_out, s.cp_src,
				   s.cp_dst, s.cp_len, d_index);
	pieces_copy(ctx, s, np, total_at, out_avail, 0, d_in, d_out, st);
	hipLaunchKernelGGL(lda_gzmw_final_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n,
			   p.usize_total, out_avail, total_at, d_result, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_gzip_members_compress_batch(struct libdeflate_compressor *c, size_t n_records,
					   const void *names, const uint64_t *name_offsets,
					   const void *d_in, size_t in_avail,
					   const uint64_t *in_offsets, const uint64_t *in_nbytes,
					   void *d_out, size_t out_avail, uint64_t *d_result,
					   uint64_t *d_index, uint32_t mtime, unsigned flags,
					   void *stream)
{
	const char *what = "gzip_members_compress_batch";
	if (!c || !d_out || !d_result || (!d_in && in_avail) || !names != !name_offsets ||
	    (n_records && (!in_offsets || !in_nbytes))) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		/* (before the count is known to be sane, no array is walked past it) */
		if (!gzmw_check(n_records, (const uint8_t *)names, name_offsets, in_offsets, in_nbytes,
				in_avail, flags, c->level, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (level 0 too: its stored blocks are the compress kernel's) */
		const zipw_params pr = pieces_params(c, false);
		gzmw_plan p;
		gzmw_plan_build(pr, n_records, name_offsets, in_offsets, in_nbytes, p);
		return gzmw_enqueue(c, p,
				    p.names_bytes ? (const uint8_t *)names + name_offsets[0] : NULL,
				    (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result, d_index,
				    mtime, (hipStream_t)stream);
	});
}
