/*
 * host_gzip_members_write.hip - C-ABI of writing a file of concatenated gzip
 * members in device memory (include/libdeflate_amd.h:
 * libdeflate_amd_gzip_members_compress_batch).
 *
 * The ZIP writer's pipeline (host_zip_write.hip) with a simpler container:
 * gzip_members_write_plan.h checks the host arrays and cuts the records into
 * the ZIP writer's pieces; its columns and the names go up through the
 * object's pinned block in ONE copy; ONE CRC-32 batch runs over the pieces,
 * the compress batches of every launch group run into slots in the object's
 * scratch (compress_deflate_pieces()), and the kernels of
 * gzip_members_write_kernels.hip size the members, place header, name and
 * footer and - through the ZIP writer's copy kernel - the pieces.  Nothing
 * comes back, and the device is waited for only where the pinned block is
 * still on its way up from the previous call on the same object (and where
 * scratch grows).  The scratch and the pinned block are the ZIP writer's
 * (c->zipw, c->zipw_up): [record columns][piece columns][seg_info][names]
 * (what goes up), [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums]
 * [csize][crc][crcs][slots].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_objects.h"
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

struct GzmwScratch {
	/* what goes up */
	uint64_t *ecols, *pcols;
	uint32_t *seg;
	uint8_t *names;
	size_t up_bytes;
	/* what the kernels leave */
	uint64_t *out_n, *cp_src, *cp_dst, *cp_len, *sizes, *offs, *bsum, *csize;
	uint32_t *crc, *crcs;
	uint8_t *slots;
	size_t bytes;
};

static GzmwScratch gzmw_scratch(void *base, const gzmw_plan &p)
{
	GzmwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.ecols = c.take<uint64_t>(GZMW_ECOLS * n);
	s.pcols = c.take<uint64_t>(ZIPW_PCOLS * np);
	s.seg = c.take<uint32_t>(np);
	s.names = c.take<uint8_t>((size_t)p.names_bytes);
	s.up_bytes = c.at;
	s.out_n = c.take<uint64_t>(np);
	s.cp_src = c.take<uint64_t>(np);
	s.cp_dst = c.take<uint64_t>(np);
	s.cp_len = c.take<uint64_t>(np);
	s.sizes = c.take<uint64_t>(n);
	s.offs = c.take<uint64_t>(n);
	s.bsum = c.take<uint64_t>(scan_blocks(n) + 1);
	s.csize = c.take<uint64_t>(n);
	s.crc = c.take<uint32_t>(n);
	s.crcs = c.take<uint32_t>(np);
	s.slots = c.take<uint8_t>((size_t)p.slots_bytes, 256);
	s.bytes = c.at + 16;
	return s;
}

/* pieces per compress launch of a group: segments as the segmented
 * single-buffer path slices them, whole records in one call */
static size_t gzmw_per_launch(const zipw_group &g)
{
	return g.S ? (size_t)lda_large_per_slice(g.S) : (size_t)(g.hi - g.lo);
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

	LDA_OK_TRY(c->zipw_up.begin());
	/* all of the call's scratch before anything is queued: growing frees
	 * memory (and waits for the device) */
	size_t kernels = 0;
	for (const zipw_group &g : p.groups)
		kernels = std::max(kernels, compress_pieces_scratch(
			c, std::min(gzmw_per_launch(g), (size_t)(g.hi - g.lo)), (size_t)g.max_in,
			g.S != 0));
	uint8_t *ws = (uint8_t *)c->zipw.reserve(sz.bytes);
	uint8_t *h = (uint8_t *)c->zipw_up.pinned(sz.up_bytes);
	if (!ws || !h || (kernels && !c->scratch.reserve(kernels)))
		return LIBDEFLATE_AMD_OOM;
	const GzmwScratch s = gzmw_scratch(ws, p), hs = gzmw_scratch(h, p);
	if (sz.up_bytes) {
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
		memcpy(hs.pcols, p.pcols.data(), p.pcols.size() * 8);
		memcpy(hs.seg, p.seg_info.data(), p.seg_info.size() * 4);
		if (p.names_bytes)
			memcpy(hs.names, names, (size_t)p.names_bytes);
		LDA_OK_TRY(c->zipw_up.send(ws, sz.up_bytes, st));
	}
	const uint64_t *ecol[GZMW_ECOLS], *pcol[ZIPW_PCOLS];
	for (size_t a = 0; a < GZMW_ECOLS; a++)
		ecol[a] = s.ecols + a * n;
	for (size_t a = 0; a < ZIPW_PCOLS; a++)
		pcol[a] = s.pcols + a * np;

	int rc = libdeflate_amd_crc32_batch(np, d_in, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N], NULL,
					    s.crcs, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	for (const zipw_group &g : p.groups) {
		const size_t per = gzmw_per_launch(g);
		for (size_t lo = (size_t)g.lo; lo < g.hi; lo += per) {
			const size_t nk = std::min(per, (size_t)g.hi - lo);
			rc = compress_deflate_pieces(c, nk, d_in, pcol[ZIPW_P_IN_OFF] + lo,
						     pcol[ZIPW_P_IN_N] + lo, s.slots,
						     pcol[ZIPW_P_SLOT_OFF] + lo,
						     pcol[ZIPW_P_SLOT_AV] + lo, s.out_n + lo, st,
						     g.S ? s.seg + lo : NULL, (size_t)g.max_in);
			if (rc != LIBDEFLATE_AMD_OK)
				return rc;
		}
	}
	const unsigned wave_grid = (unsigned)std::max((size_t)1, std::min((n + 3) / 4, (size_t)ctx->num_cus * 16));
	if (n)
		hipLaunchKernelGGL(lda_gzmw_member_kernel, dim3(wave_grid), dim3(256), 0, st, (uint64_t)n,
				   ecol[GZMW_E_FIRST], ecol[GZMW_E_COUNT], ecol[GZMW_E_NAME_LEN],
				   ecol[GZMW_E_USIZE], pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
				   (const uint64_t *)s.out_n, (const uint32_t *)s.crcs, s.csize, s.crc,
				   s.sizes);
	/* (of no records, the total alone: a file of 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_gzmw_place_kernel, dim3(wave_grid), dim3(256), 0, st, (uint64_t)n,
				   c->level, mtime, out_avail, ecol[GZMW_E_FIRST], ecol[GZMW_E_COUNT],
				   ecol[GZMW_E_NAME_OFF], ecol[GZMW_E_NAME_LEN], ecol[GZMW_E_USIZE],
				   ecol[GZMW_E_UOFF], (const uint8_t *)s.names, pcol[ZIPW_P_PC_OFF],
				   pcol[ZIPW_P_PC_N], pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n,
				   (const uint64_t *)s.csize, (const uint32_t *)s.crc,
				   (const uint64_t *)s.offs, (const uint64_t *)s.bsum, d_out, s.cp_src,
				   s.cp_dst, s.cp_len, d_index);
	if (np) {
		const size_t grid = std::min(np, (size_t)ctx->num_cus * 8);
		hipLaunchKernelGGL(lda_zipw_copy_kernel, dim3((unsigned)grid), dim3(256), 0, st,
				   (uint64_t)np, total_at, out_avail, (uint64_t)0,
				   (const uint64_t *)s.cp_src, (const uint64_t *)s.cp_dst,
				   (const uint64_t *)s.cp_len, d_in, (const uint8_t *)s.slots, d_out);
	}
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
		const EnvCfg &env = env_cfg();
		zipw_params pr;
		pr.level = c->level;
		pr.store = false;	/* level 0 too: its stored blocks are the compress kernel's */
		pr.no_segments = env.no_segments;
		pr.env_seg = env.seg_bytes;
		pr.D = compress_prime_window();
		pr.tile = lda_deflate_tile();
		pr.small_max = c->level <= 9 && !env.no_small ? lda_deflate_small_max() : 0;
		gzmw_plan p;
		gzmw_plan_build(pr, n_records, name_offsets, in_offsets, in_nbytes, p);
		return gzmw_enqueue(c, p,
				    p.names_bytes ? (const uint8_t *)names + name_offsets[0] : NULL,
				    (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result, d_index,
				    mtime, (hipStream_t)stream);
	});
}
