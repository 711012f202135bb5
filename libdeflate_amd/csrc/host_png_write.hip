/*
 * host_png_write.hip - C-ABI of writing PNG files in device memory
 * (include/libdeflate_amd.h: libdeflate_amd_png_encode_batch).
 *
 * png_write_plan.h checks the image rows, gives every image a room for its
 * filtered scanlines in the object's scratch and cuts the rooms into pieces;
 * its columns and the filter kernel's work list go up; the filter kernel
 * (png_write_kernels.hip) fills the rooms from the pixels in d_in, one launch
 * per group class; ONE Adler-32 batch runs over the pieces, the pieces are
 * compressed from the rooms into slots (the shared piece pipeline,
 * host_write_pieces.hip), ONE CRC-32 batch runs over the COMPRESSED pieces in
 * their slots - an IDAT chunk's CRC covers compressed bytes -, and the kernels
 * of png_write_kernels.hip size the files and place their fixed parts.
 * c->zipw: [image columns][piece columns][seg_info][work list] (what goes up),
 * [out_n][cp_src cp_dst cp_len][sizes][offsets][block sums][slots][csize]
 * [adler crc][adlers crcs][scanlines].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_write_pieces.h"
#include "kernels.h"
#include "png_write_plan.h"

using namespace lda;

static_assert(LIBDEFLATE_AMD_PNGW_RESULT_WORDS == PNGW_RESULT_WORDS &&
	      LIBDEFLATE_AMD_PNG_FILTER_ADAPTIVE == PNGW_FILTER_ADAPTIVE &&
	      LIBDEFLATE_AMD_PNG_WORDS == PNG_ROW_WORDS && LIBDEFLATE_AMD_PNG_LE16 == PNG_LE16 &&
	      PNGW_MAX_IMAGES == (uint64_t)1 << 28,
	      "png_write_plan.h holds copies of the header's constants");

/* the stages of a call; the benchmark times each alone (lda_png_encode_stages) */
enum { PNGW_STAGE_FILTER = 1, PNGW_STAGE_COMPRESS = 2, PNGW_STAGE_ASSEMBLE = 4, PNGW_STAGE_ALL = 7 };

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_png_encode_bound(struct libdeflate_compressor *c, size_t n_images,
				const uint64_t *images)
{
	if (!c || (n_images && !images)) {
		set_error("png_encode_bound: NULL argument");
		return 0;
	}
	return (size_t)pngw_bound(n_images, images, c->level);
}

struct PngwScratch : PiecesScratch {
	uint64_t *icols, *csize;
	uint32_t *adler, *crc, *adlers, *crcs;
	uint8_t *scan;
	size_t bytes;
};

static PngwScratch pngw_scratch(void *base, const pngw_plan &p)
{
	PngwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.icols = c.take<uint64_t>(PNGW_ICOLS * n);
	pieces_carve(c, p, n, p.work.size() * 8, s);
	s.csize = c.take<uint64_t>(n);
	s.adler = c.take<uint32_t>(n);
	s.crc = c.take<uint32_t>(n);
	s.adlers = c.take<uint32_t>(np);
	s.crcs = c.take<uint32_t>(np);
	s.scan = c.take<uint8_t>((size_t)p.scan_bytes + 64, 256);
	s.bytes = c.at + 16;
	return s;
}

static int pngw_enqueue(struct libdeflate_compressor *c, const pngw_plan &p, const uint8_t *d_in,
			uint8_t *d_out, uint64_t out_avail, uint64_t *d_result, uint64_t *d_index,
			unsigned filter, unsigned stages, hipStream_t st)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n, np = (size_t)p.np;
	const PngwScratch sz = pngw_scratch(NULL, p);
	const std::vector<zipw_launch> launches = zipw_launches(p);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const PngwScratch s = pngw_scratch(ws, p), hs = pngw_scratch(h, p);
	if (sz.up_bytes) {
		memcpy(hs.icols, p.icols.data(), p.icols.size() * 8);
		memcpy(hs.behind, p.work.data(), p.work.size() * 8);
	}
	LDA_OK_TRY(pieces_upload(c, hs, p, ws, st));
	const uint64_t *const *pcol = s.pcol, *work = (const uint64_t *)s.behind;

	for (unsigned cls = 0; cls < PNGW_CLASSES && (stages & PNGW_STAGE_FILTER); cls++) {
		const size_t items = (size_t)(p.items[cls + 1] - p.items[cls]);
		if (!items)
			continue;
		const size_t grid = std::min(items, (size_t)ctx->num_cus * 16);
		hipLaunchKernelGGL(cls == 0 ? lda_pngw_filter4_kernel :
				   cls == 1 ? lda_pngw_filter16_kernel : lda_pngw_filter64_kernel,
				   dim3((unsigned)grid), dim3(256), 0, st, (uint64_t)n, (uint64_t)items,
				   (uint32_t)filter,
				   work + PNGW_WORK_WORDS * p.items[cls],
				   (const uint64_t *)s.icols, d_in, s.scan);
	}
	int rc = LIBDEFLATE_AMD_OK;
	if (stages & PNGW_STAGE_COMPRESS)
		rc = libdeflate_amd_adler32_batch(np, s.scan, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						  NULL, s.adlers, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	if (stages & PNGW_STAGE_COMPRESS)
		rc = pieces_compress(c, s, launches, s.scan, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	if (stages & PNGW_STAGE_COMPRESS)
		rc = libdeflate_amd_crc32_batch(np, s.slots, pcol[ZIPW_P_SLOT_OFF], s.out_n, NULL, s.crcs,
						st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	if (!(stages & PNGW_STAGE_ASSEMBLE)) {
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	const unsigned grid = wave_grid(ctx, n);
	if (n)
		hipLaunchKernelGGL(lda_pngw_image_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   (uint64_t)np, pngw_idat_head_crc(c->level), (const uint64_t *)s.icols,
				   (const uint64_t *)s.pcols, (const uint64_t *)s.out_n,
				   (const uint32_t *)s.adlers, (const uint32_t *)s.crcs, s.csize, s.adler,
				   s.crc, s.sizes);
	/* (of no images, the total alone: 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_pngw_place_kernel, dim3(grid), dim3(256), 0, st, (uint64_t)n,
				   (uint64_t)np, c->level, out_avail, (const uint64_t *)s.icols,
				   (const uint64_t *)s.pcols, (const uint64_t *)s.out_n,
				   (const uint64_t *)s.csize, (const uint32_t *)s.adler,
				   (const uint32_t *)s.crc, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_in, d_out, s.cp_src, s.cp_dst, s.cp_len,
				   d_index);
	pieces_copy(ctx, s, np, total_at, out_avail, 0, d_in, d_out, st);
	hipLaunchKernelGGL(lda_pngw_final_kernel, dim3(1), dim3(64), 0, st, (uint64_t)n,
			   p.pixels_total, out_avail, total_at, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

static int pngw_call(const char *what, struct libdeflate_compressor *c, size_t n_images,
		     const uint64_t *images, const void *d_in, size_t in_avail, void *d_out,
		     size_t out_avail, uint64_t *d_result, uint64_t *d_index, unsigned filter,
		     unsigned flags, unsigned stages, void *stream)
{
	if (!c || !d_out || !d_result || (!d_in && in_avail) || (n_images && !images)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::string err;
		if (!pngw_check(n_images, images, in_avail, filter, flags, c->level, err)) {
			set_error("%s: %s", what, err.c_str());
			return LIBDEFLATE_AMD_BAD_ARG;
		}
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		/* (level 0 too: its stored blocks are the compress kernel's) */
		const zipw_params pr = pieces_params(c, false);
		pngw_plan p;
		pngw_plan_build(pr, n_images, images, flags, p);
		return pngw_enqueue(c, p, (const uint8_t *)d_in, (uint8_t *)d_out, out_avail, d_result,
				    d_index, filter, stages, (hipStream_t)stream);
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_png_encode_batch(struct libdeflate_compressor *c, size_t n_images,
				const uint64_t *images, const void *d_in, size_t in_avail,
				void *d_out, size_t out_avail, uint64_t *d_result, uint64_t *d_index,
				unsigned filter, unsigned flags, void *stream)
{
	return pngw_call("png_encode_batch", c, n_images, images, d_in, in_avail, d_out, out_avail,
			 d_result, d_index, filter, flags, PNGW_STAGE_ALL, stream);
}

/* not part of the interface: the same call with only the stages of `stages`
 * queued (1 the filter kernel, 2 checksums and compress, 4 the assembly), so
 * that tools/bench_png_write.py can time each alone on scratch an earlier full
 * call has filled */
extern "C" LIBDEFLATEAPI int
lda_png_encode_stages(struct libdeflate_compressor *c, size_t n_images, const uint64_t *images,
		      const void *d_in, size_t in_avail, void *d_out, size_t out_avail,
		      uint64_t *d_result, uint64_t *d_index, unsigned filter, unsigned flags,
		      unsigned stages, void *stream)
{
	return pngw_call("png_encode_stages", c, n_images, images, d_in, in_avail, d_out, out_avail,
			 d_result, d_index, filter, flags, stages & PNGW_STAGE_ALL, stream);
}
