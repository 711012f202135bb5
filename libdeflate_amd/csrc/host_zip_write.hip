/*
 * host_zip_write.hip - C-ABI of writing a ZIP archive in device memory
 * (include/libdeflate_amd.h: libdeflate_amd_zip_compress_batch).
 *
 * zip_write_plan.h checks the host arrays, decides ZIP64 and cuts the entries
 * into pieces; its columns and the names go up, ONE CRC-32 batch runs over the
 * pieces, the pieces are compressed into slots (the shared piece pipeline,
 * host_write_pieces.hip), and the kernels of zip_write_kernels.hip decide
 * deflate or stored per entry and place headers, data, directory and end
 * records.
 * c->zipw: [entry columns][piece columns][seg_info][names] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][e_info][crcs].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "zip_write_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_ZIP_STORE == ZIPW_STORE &&
	      LIBDEFLATE_AMD_ZIP_FORCE_ZIP64 == ZIPW_FORCE_ZIP64 &&
	      LIBDEFLATE_AMD_ZIPW_RESULT_WORDS == ZIPW_RESULT_WORDS &&
	      ZIPW_MAX_ENTRIES == (uint64_t)1 << 28,
	      "zip_write_plan.h holds copies of the header's constants");

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_zip_compress_bound(size_t n_entries, const uint64_t *name_offsets,
				  const uint64_t *in_nbytes, unsigned flags)
{
	if (n_entries && (!name_offsets || !in_nbytes)) {
		set_error("zip_compress_bound: NULL argument");
		return 0;
	}
	return (size_t)zipw_bound(n_entries, name_offsets, in_nbytes, flags, NULL, NULL, NULL);
}

struct ZipwScratch : PiecesScratch {
	uint64_t *ecols, *e_info;
	uint32_t *crcs;
	size_t bytes;
};

static ZipwScratch zipw_scratch(void *base, const zipw_plan &p, size_t names_bytes)
{
	ZipwScratch s;
	Carve c(base);

	s.ecols = c.take<uint64_t>(ZIPW_ECOLS * (size_t)p.n);
	pieces_carve(c, p, (size_t)p.n, names_bytes, s);
	s.e_info = c.take<uint64_t>((size_t)p.n);
	s.crcs = c.take<uint32_t>((size_t)p.np);
	s.bytes = c.at + 16;
	return s;
}

static int zipw_enqueue(struct libdeflate_compressor *c, const zipw_plan &p, const uint8_t *names,
			size_t names_bytes, const uint8_t *d_in, uint8_t *d_out, uint64_t out_avail,
			uint64_t *d_result, uint64_t *d_index, uint32_t dos_datetime, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np;
	const uint64_t tail = p.cd_size + p.end_bytes;
	const ZipwScratch sz = zipw_scratch(NULL, p, names_bytes);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const ZipwScratch s = zipw_scratch(ws, p, names_bytes), hs = zipw_scratch(h, p, names_bytes);
	if (sz.up_bytes) {
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
		memcpy(hs.behind, names, names_bytes);
	}
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *ecol[ZIPW_ECOLS], *const *pcol = s.pcol;
	for (size_t a = 0; a < ZIPW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;
	const bool compressed = !p.groups.empty();

	int rc = libdeflate_amd_crc32_batch(np, d_in, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], NULL,
					    s.crcs, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	LDA_OK_TRY(pieces_compress(c, s, launches, d_in, st));
	const unsigned grid = wave_grid(ctx, n);
	if (n)
		hipLaunchKernelGGL(lda_zipw_entry_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   ecol[ZIPW_E_FIRST], ecol[ZIPW_E_COUNT], ecol[ZIPW_E_NAME_LEN],
				   ecol[ZIPW_E_USIZE], pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
				   (const uint64_t *)(compressed ? s.out_n : NULL),
				   (const uint32_t *)s.crcs, s.e_info, s.sizes);
	/* (of no entries, the total alone: cd_off 0) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_zipw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   (uint32_t)p.zip64, dos_datetime, out_avail, tail, ecol[ZIPW_E_FIRST],
				   ecol[ZIPW_E_COUNT], ecol[ZIPW_E_NAME_OFF], ecol[ZIPW_E_NAME_LEN],
				   ecol[ZIPW_E_CEN], ecol[ZIPW_E_USIZE], ecol[ZIPW_E_UOFF],
				   (const uint8_t *)s.behind, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
				   pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n,
				   (const uint64_t *)s.e_info, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst, s.cp_len,
				   d_index);
	pieces_copy(ctx, s, np, total_at, out_avail, tail, d_in, d_out, st);
	hipLaunchKernelGGL(lda_zipw_final_kernel, dim3(1), dim3(1024), 0, st, (uint64_t)n,
			   (uint32_t)p.zip64, out_avail, p.cd_size, tail, ecol[ZIPW_E_USIZE],
			   (const uint64_t *)s.e_info, total_at, d_out,
			   d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_zip_compress_batch(struct libdeflate_compressor *c, size_t n_entries,
				  const void *names, const uint64_t *name_offsets,
				  const void *d_in, size_t in_avail, const uint64_t *in_offsets,
				  const uint64_t *in_nbytes, void *d_out, size_t out_avail,
				  uint64_t *d_result, uint64_t *d_index, uint32_t dos_datetime,
				  unsigned flags, void *stream)
{
	const char *what = "zip_compress_batch";
	if (!c || !d_out || !d_result || (!d_in && in_avail) ||
	    (n_entries && (!names || !name_offsets || !in_offsets || !in_nbytes))) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		/* (before the count is known to be sane, no array is walked past it) */
		if (!zipw_check(n_entries, name_offsets, in_offsets, in_nbytes, in_avail, out_avail,
				flags, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		const zipw_params pr = pieces_params(c, c->level == 0 || (flags & LIBDEFLATE_AMD_ZIP_STORE));
		zipw_plan p;
		const uint8_t *nm = n_entries ? (const uint8_t *)names + name_offsets[0] : NULL;
		zipw_plan_build(pr, n_entries, (const uint8_t *)names, name_offsets, in_offsets,
				in_nbytes, flags, p);
		return zipw_enqueue(c, p, nm,
				    n_entries ? (size_t)(name_offsets[n_entries] - name_offsets[0]) : 0,
				    (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result, d_index,
				    dos_datetime ? dos_datetime : 0x00210000u, (hipStream_t)stream);
	});
}
