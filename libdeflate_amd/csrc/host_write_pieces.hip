/*
 * host_write_pieces.hip - the piece pipeline of the writers that compress many
 * buffers into one output in device memory: ZIP archives (host_zip_write.hip),
 * files of gzip members (host_gzip_members_write.hip) and PNG files
 * (host_png_write.hip).  write_pieces_plan.h cuts the buffers into pieces;
 * here they go through the object: the plan's columns up through the pinned
 * block in ONE copy (Upload, host_common.h), the compress batches of the
 * launch list into slots in c->zipw (compress_deflate_pieces(): the launches
 * of the batch entry points, sliced like the segmented single-buffer path),
 * and lda_zipw_copy_kernel (zip_write_device.h) from the slots or the source
 * to where the writer's place kernel wants every piece.  Nothing comes back,
 * and the device is waited for only where the pinned block is still on its way
 * up from the previous call on the same object (and where scratch grows).
 */
#include <string.h>
#include <algorithm>

#include "host_write_pieces.h"
#include "kernels.h"

using namespace lda;

zipw_params lda::pieces_params(const struct libdeflate_compressor *c, bool store)
{
	const EnvCfg &env = env_cfg();
	zipw_params pr;
	pr.level = c->level;
	pr.store = store;
	pr.no_segments = env.no_segments;
	pr.env_seg = env.seg_bytes;
	pr.D = compress_prime_window();
	pr.tile = lda_deflate_tile();
	pr.small_max = c->level <= 9 && !env.no_small ? lda_deflate_small_max() : 0;
	return pr;
}

void lda::pieces_carve(Carve &c, const zipw_pieces &p, size_t n, size_t behind_bytes,
		       PiecesScratch &s)
{
	const size_t np = (size_t)p.np;

	s.pcols = c.take<uint64_t>(ZIPW_PCOLS * np);
	s.seg = c.take<uint32_t>(np);
	s.behind = c.take<uint8_t>(behind_bytes);
	s.up_bytes = c.at;
	s.out_n = c.take<uint64_t>(np);
	s.cp_src = c.take<uint64_t>(np);
	s.cp_dst = c.take<uint64_t>(np);
	s.cp_len = c.take<uint64_t>(np);
	s.sizes = c.take<uint64_t>(n);
	s.offs = c.take<uint64_t>(n);
	s.bsum = c.take<uint64_t>(scan_blocks(n) + 1);
	s.slots = c.take<uint8_t>((size_t)p.slots_bytes, 256);
	for (size_t a = 0; a < ZIPW_PCOLS; a++)
		s.pcol[a] = s.pcols ? s.pcols + a * np : NULL;
}

int lda::pieces_reserve(struct libdeflate_compressor *c, const std::vector<zipw_launch> &launches,
			size_t bytes, size_t up_bytes, uint8_t **ws, uint8_t **pinned)
{
	LDA_OK_TRY(c->zipw_up.begin());
	/* all of the call's scratch before anything is queued: growing frees
	 * memory (and waits for the device) */
	size_t kernels = 0;
	for (const zipw_launch &l : launches)
		kernels = std::max(kernels, compress_pieces_scratch(c, (size_t)l.count, (size_t)l.max_in,
								    l.segmented));
	*ws = (uint8_t *)c->zipw.reserve(bytes);
	*pinned = (uint8_t *)c->zipw_up.pinned(up_bytes);
	if (!*ws || !*pinned || (kernels && !c->scratch.reserve(kernels)))
		return LIBDEFLATE_AMD_OOM;
	return LIBDEFLATE_AMD_OK;
}

int lda::pieces_upload(struct libdeflate_compressor *c, const PiecesScratch &hs, const zipw_pieces &p,
		       uint8_t *ws, hipStream_t st)
{
	if (!hs.up_bytes)
		return LIBDEFLATE_AMD_OK;
	memcpy(hs.pcols, p.pcols.data(), p.pcols.size() * 8);
	memcpy(hs.seg, p.seg_info.data(), p.seg_info.size() * 4);
	return c->zipw_up.send(ws, hs.up_bytes, st);
}

int lda::pieces_compress(struct libdeflate_compressor *c, const PiecesScratch &s,
			 const std::vector<zipw_launch> &launches, const uint8_t *src, hipStream_t st)
{
	for (const zipw_launch &l : launches)
		LDA_OK_TRY(compress_deflate_pieces(c, (size_t)l.count, src, s.pcol[ZIPW_P_IN_OFF] + l.lo,
						   s.pcol[ZIPW_P_IN_N] + l.lo, s.slots,
						   s.pcol[ZIPW_P_SLOT_OFF] + l.lo,
						   s.pcol[ZIPW_P_SLOT_AV] + l.lo, s.out_n + l.lo, st,
						   l.segmented ? s.seg + l.lo : NULL, (size_t)l.max_in));
	return LIBDEFLATE_AMD_OK;
}

void lda::pieces_copy(const DeviceCtx *ctx, const PiecesScratch &s, size_t np, const uint64_t *total_at,
		      uint64_t out_avail, uint64_t tail, const uint8_t *d_in, uint8_t *d_out,
		      hipStream_t st)
{
	if (!np)
		return;
	hipLaunchKernelGGL(lda_zipw_copy_kernel, dim3(tile_grid(ctx, np)), dim3(256), 0, st, (uint64_t)np,
			   total_at, out_avail, tail, (const uint64_t *)s.cp_src,
			   (const uint64_t *)s.cp_dst, (const uint64_t *)s.cp_len, d_in,
			   (const uint8_t *)s.slots, d_out);
}
