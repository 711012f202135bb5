/*
 * host_write_pieces.hip - the piece pipeline of the writers that compress many
 * buffers into one output in device memory: ZIP archives (host_zip_write.hip),
 * files of gzip members (host_gzip_members_write.hip), PNG files
 * (host_png_write.hip) and the chunk codecs - shuffled chunks, TIFF segments,
 * OpenEXR chunks (host_shuffle_write.hip, host_tiff_write.hip,
 * host_exr_write.hip).  write_pieces_plan.h cuts the buffers into pieces;
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

/* ---- the chunk codecs' writers ---- */

static ChunkwScratch chunkw_carve(void *base, const chunk_write_plan &p, bool two_areas)
{
	ChunkwScratch s;
	Carve c(base);
	const size_t n = (size_t)p.n, np = (size_t)p.np;

	s.ecols = c.take<uint64_t>(p.ecols.size());
	pieces_carve(c, p, n, 0, s);
	s.csize = c.take<uint64_t>(n);
	s.dsize = c.take<uint64_t>(two_areas ? n : 0);
	s.sum = c.take<uint32_t>(n);
	s.sums = c.take<uint32_t>(np);
	s.raw = c.take<uint8_t>(two_areas ? (size_t)p.rooms_bytes + 64 : 0, 256);
	s.rooms = c.take<uint8_t>((size_t)p.rooms_bytes + 64, 256);
	s.bytes = c.at + 16;
	return s;
}

int lda::chunkw_begin(struct libdeflate_compressor *c, const chunk_write_plan &p,
		      const std::vector<zipw_launch> &launches, hipStream_t st, ChunkwScratch &s,
		      bool two_areas)
{
	const ChunkwScratch sz = chunkw_carve(NULL, p, two_areas);
	uint8_t *ws, *h;

	LDA_OK_TRY(pieces_reserve(c, launches, sz.bytes, sz.up_bytes, &ws, &h));
	const ChunkwScratch hs = chunkw_carve(h, p, two_areas);
	s = chunkw_carve(ws, p, two_areas);
	if (sz.up_bytes && !p.ecols.empty())
		memcpy(hs.ecols, p.ecols.data(), p.ecols.size() * 8);
	return pieces_upload(c, hs, p, ws, st);
}

int lda::chunkw_compress(struct libdeflate_compressor *c, int format, const chunk_write_plan &p,
			 const ChunkwScratch &s, const std::vector<zipw_launch> &launches,
			 const uint8_t *src, hipStream_t st)
{
	if (format == LIBDEFLATE_AMD_ZLIB)
		LDA_OK_TRY(libdeflate_amd_adler32_batch((size_t)p.np, src, s.pcol[ZIPW_P_PC_OFF],
							s.pcol[ZIPW_P_PC_N], NULL, s.sums, st));
	else if (format == LIBDEFLATE_AMD_GZIP)
		LDA_OK_TRY(libdeflate_amd_crc32_batch((size_t)p.np, src, s.pcol[ZIPW_P_PC_OFF],
						      s.pcol[ZIPW_P_PC_N], NULL, s.sums, st));
	return pieces_compress(c, s, launches, src, st);
}

void lda::chunkw_sizes(const DeviceCtx *ctx, int format, const chunk_write_plan &p,
		       const ChunkwScratch &s, hipStream_t st)
{
	const size_t n = (size_t)p.n;

	if (n)
		hipLaunchKernelGGL(lda_shufw_chunk_kernel, dim3(wave_grid(ctx, n)), dim3(256), 0, st,
				   (uint64_t)n, format, (const uint64_t *)(s.ecols + CHUNKW_E_FIRST * n),
				   (const uint64_t *)(s.ecols + CHUNKW_E_COUNT * n),
				   (const uint64_t *)(s.ecols + CHUNKW_E_USIZE * n), s.pcol[ZIPW_P_PC_OFF],
				   s.pcol[ZIPW_P_PC_N], (const uint64_t *)s.out_n, (const uint32_t *)s.sums,
				   s.csize, s.sum, s.sizes);
}

const uint64_t *lda::chunkw_scan(const chunk_write_plan &p, const ChunkwScratch &s, hipStream_t st)
{
	/* (of no rows, the total alone: 0 bytes) */
	return s.bsum + scan_enqueue(st, (size_t)p.n, s.sizes, s.offs, s.bsum);
}

void lda::chunkw_place(const DeviceCtx *ctx, int format, int level, const chunk_write_plan &p,
		       const ChunkwScratch &s, uint64_t out_avail, uint8_t *d_out, uint64_t *d_index,
		       hipStream_t st)
{
	if (!p.n)
		return;
	hipLaunchKernelGGL(lda_shufw_place_kernel, dim3(wave_grid(ctx, (size_t)p.n)), dim3(256), 0, st,
			   p.n, format, level, out_avail, (const uint64_t *)s.ecols, s.pcol[ZIPW_P_PC_OFF],
			   s.pcol[ZIPW_P_PC_N], s.pcol[ZIPW_P_SLOT_OFF], (const uint64_t *)s.out_n,
			   (const uint64_t *)s.csize, (const uint32_t *)s.sum, (const uint64_t *)s.offs,
			   (const uint64_t *)s.bsum, d_out, s.cp_src, s.cp_dst, s.cp_len, d_index);
}

int lda::chunkw_finish(const DeviceCtx *ctx, const chunk_write_plan &p, const ChunkwScratch &s,
		       const uint64_t *total_at, uint64_t out_avail, const uint8_t *copy_src,
		       uint8_t *d_out, uint64_t *d_result, hipStream_t st)
{
	pieces_copy(ctx, s, (size_t)p.np, total_at, out_avail, 0, copy_src, d_out, st);
	hipLaunchKernelGGL(lda_shufw_final_kernel, dim3(1), dim3(64), 0, st, p.n, p.raw_total, out_avail,
			   total_at, d_result);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
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
