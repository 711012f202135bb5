/*
 * host_png_write.hip - C-ABI of writing PNG files in device memory
 * (include/libdeflate_amd.h: libdeflate_amd_png_encode_batch).
 *
 * The gzip-members writer's pipeline (host_gzip_members_write.hip) behind one
 * kernel of its own: png_write_plan.h checks the image rows, gives every image
 * a room for its filtered scanlines in the object's scratch and cuts the rooms
 * into the ZIP writer's pieces; its columns and the filter kernel's work list
 * go up through the object's pinned block in ONE copy; the filter kernel
 * (png_write_kernels.hip) fills the rooms from the pixels in d_in, one launch
 * per group class; ONE Adler-32 batch runs over the pieces, the compress
 * batches of every launch group run into slots (compress_deflate_pieces()),
 * ONE CRC-32 batch runs over the COMPRESSED pieces in their slots - an IDAT
 * chunk's CRC covers compressed bytes -, and the kernels of
 * png_write_kernels.hip size the files, place their fixed parts and - through
 * the ZIP writer's copy kernel - the pieces.  Nothing comes back.  The scratch
 * and the pinned block are the ZIP writer's (c->zipw, c->zipw_up): [image
 * columns][piece columns][seg_info][work list] (what goes up), [out_n][cp_src
 * cp_dst cp_len][sizes][offsets][block sums][csize][adler crc][adlers crcs]
 * [slots][scanlines].
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_objects.h"
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

struct PngwScratch {
	/* what goes up */
	uint64_t *icols, *pcols;
	uint32_t *seg;
	uint64_t *work;
	size_t up_bytes;
	/* what the kernels leave */
	uint64_t *out_n, *cp_src, *cp_dst, *cp_len, *sizes, *offs, *bsum, *csize;
	uint32_t *adler, *crc, *adlers, *crcs;
	uint8_t *slots, *scan;
	size_t bytes;
};

static PngwScratch pngw_scratch(void *base, const pngw_plan &p)
{
	PngwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.icols = c.take<uint64_t>(PNGW_ICOLS * n);
	s.pcols = c.take<uint64_t>(ZIPW_PCOLS * np);
	s.seg = c.take<uint32_t>(np);
	s.work = c.take<uint64_t>(p.work.size());
	s.up_bytes = c.at;
	s.out_n = c.take<uint64_t>(np);
	s.cp_src = c.take<uint64_t>(np);
	s.cp_dst = c.take<uint64_t>(np);
	s.cp_len = c.take<uint64_t>(np);
	s.sizes = c.take<uint64_t>(n);
	s.offs = c.take<uint64_t>(n);
	s.bsum = c.take<uint64_t>(scan_blocks(n) + 1);
	s.csize = c.take<uint64_t>(n);
	s.adler = c.take<uint32_t>(n);
	s.crc = c.take<uint32_t>(n);
	s.adlers = c.take<uint32_t>(np);
	s.crcs = c.take<uint32_t>(np);
	s.slots = c.take<uint8_t>((size_t)p.slots_bytes, 256);
	s.scan = c.take<uint8_t>((size_t)p.scan_bytes + 64, 256);
	s.bytes = c.at + 16;
	return s;
}

/* pieces per compress launch of a group: segments as the segmented
 * single-buffer path slices them, whole images in one call */
static size_t pngw_per_launch(const zipw_group &g)
{
	return g.S ? (size_t)lda_large_per_slice(g.S) : (size_t)(g.hi - g.lo);
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

	LDA_OK_TRY(c->zipw_up.begin());
	/* all of the call's scratch before anything is queued: growing frees
	 * memory (and waits for the device) */
	size_t kernels = 0;
	for (const zipw_group &g : p.groups)
		kernels = std::max(kernels, compress_pieces_scratch(
			c, std::min(pngw_per_launch(g), (size_t)(g.hi - g.lo)), (size_t)g.max_in,
			g.S != 0));
	uint8_t *ws = (uint8_t *)c->zipw.reserve(sz.bytes);
	uint8_t *h = (uint8_t *)c->zipw_up.pinned(sz.up_bytes);
	if (!ws || !h || (kernels && !c->scratch.reserve(kernels)))
		return LIBDEFLATE_AMD_OOM;
	const PngwScratch s = pngw_scratch(ws, p), hs = pngw_scratch(h, p);
	if (sz.up_bytes) {
		memcpy(hs.icols, p.icols.data(), p.icols.size() * 8);
		memcpy(hs.pcols, p.pcols.data(), p.pcols.size() * 8);
		memcpy(hs.seg, p.seg_info.data(), p.seg_info.size() * 4);
		memcpy(hs.work, p.work.data(), p.work.size() * 8);
		LDA_OK_TRY(c->zipw_up.send(ws, sz.up_bytes, st));
	}
	const uint64_t *pcol[ZIPW_PCOLS];
	for (size_t a = 0; a < ZIPW_PCOLS; a++)
		pcol[a] = s.pcols + a * np;

	for (unsigned cls = 0; cls < PNGW_CLASSES && (stages & PNGW_STAGE_FILTER); cls++) {
		const size_t items = (size_t)(p.items[cls + 1] - p.items[cls]);
		if (!items)
			continue;
		const size_t grid = std::min(items, (size_t)ctx->num_cus * 16);
		hipLaunchKernelGGL(cls == 0 ? lda_pngw_filter4_kernel :
				   cls == 1 ? lda_pngw_filter16_kernel : lda_pngw_filter64_kernel,
				   dim3((unsigned)grid), dim3(256), 0, st, (uint64_t)n, (uint64_t)items,
				   (uint32_t)filter,
				   (const uint64_t *)s.work + PNGW_WORK_WORDS * p.items[cls],
				   (const uint64_t *)s.icols, d_in, s.scan);
	}
	int rc = LIBDEFLATE_AMD_OK;
	if (stages & PNGW_STAGE_COMPRESS)
		rc = libdeflate_amd_adler32_batch(np, s.scan, pcol[ZIPW_P_PC_OFF], pcol[ZIPW_P_PC_N],
						  NULL, s.adlers, st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	for (const zipw_group &g : p.groups) {
		if (!(stages & PNGW_STAGE_COMPRESS))
			break;
		const size_t per = pngw_per_launch(g);
		for (size_t lo = (size_t)g.lo; lo < g.hi; lo += per) {
			const size_t nk = std::min(per, (size_t)g.hi - lo);
			rc = compress_deflate_pieces(c, nk, s.scan, pcol[ZIPW_P_IN_OFF] + lo,
						     pcol[ZIPW_P_IN_N] + lo, s.slots,
						     pcol[ZIPW_P_SLOT_OFF] + lo,
						     pcol[ZIPW_P_SLOT_AV] + lo, s.out_n + lo, st,
						     g.S ? s.seg + lo : NULL, (size_t)g.max_in);
			if (rc != LIBDEFLATE_AMD_OK)
				return rc;
		}
	}
	if (stages & PNGW_STAGE_COMPRESS)
		rc = libdeflate_amd_crc32_batch(np, s.slots, pcol[ZIPW_P_SLOT_OFF], s.out_n, NULL, s.crcs,
						st);
	if (rc != LIBDEFLATE_AMD_OK)
		return rc;
	if (!(stages & PNGW_STAGE_ASSEMBLE)) {
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	const unsigned wave_grid = (unsigned)std::max((size_t)1, std::min((n + 3) / 4, (size_t)ctx->num_cus * 16));
	if (n)
		hipLaunchKernelGGL(lda_pngw_image_kernel, dim3(wave_grid), dim3(256), 0, st, (uint64_t)n,
				   (uint64_t)np, pngw_idat_head_crc(c->level), (const uint64_t *)s.icols,
				   (const uint64_t *)s.pcols, (const uint64_t *)s.out_n,
				   (const uint32_t *)s.adlers, (const uint32_t *)s.crcs, s.csize, s.adler,
				   s.crc, s.sizes);
	/* (of no images, the total alone: 0 bytes) */
	const uint64_t *total_at = s.bsum + scan_enqueue(st, n, s.sizes, s.offs, s.bsum);
	if (n)
		hipLaunchKernelGGL(lda_pngw_place_kernel, dim3(wave_grid), dim3(256), 0, st, (uint64_t)n,
				   (uint64_t)np, c->level, out_avail, (const uint64_t *)s.icols,
				   (const uint64_t *)s.pcols, (const uint64_t *)s.out_n,
				   (const uint64_t *)s.csize, (const uint32_t *)s.adler,
				   (const uint32_t *)s.crc, (const uint64_t *)s.offs,
				   (const uint64_t *)s.bsum, d_in, d_out, s.cp_src, s.cp_dst, s.cp_len,
				   d_index);
	if (np) {
		const size_t grid = std::min(np, (size_t)ctx->num_cus * 8);
		hipLaunchKernelGGL(lda_zipw_copy_kernel, dim3((unsigned)grid), dim3(256), 0, st,
				   (uint64_t)np, total_at, out_avail, (uint64_t)0,
				   (const uint64_t *)s.cp_src, (const uint64_t *)s.cp_dst,
				   (const uint64_t *)s.cp_len, d_in, (const uint8_t *)s.slots, d_out);
	}
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
		const EnvCfg &env = env_cfg();
		zipw_params pr;
		pr.level = c->level;
		pr.store = false;	/* level 0 too: its stored blocks are the compress kernel's */
		pr.no_segments = env.no_segments;
		pr.env_seg = env.seg_bytes;
		pr.D = compress_prime_window();
		pr.tile = lda_deflate_tile();
		pr.small_max = c->level <= 9 && !env.no_small ? lda_deflate_small_max() : 0;
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
