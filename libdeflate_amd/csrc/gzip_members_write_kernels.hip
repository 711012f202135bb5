/*
 * gzip_members_write_kernels.hip - a file of gzip members assembled in device
 * memory (host_gzip_members_write.hip:
 * libdeflate_amd_gzip_members_compress_batch).
 *
 * The compress batches have left every piece's raw DEFLATE bytes in a slot and
 * the CRC-32 batch every piece's checksum (gzip_members_write_plan.h).  Three
 * kernels of this file and one of the ZIP writer's make the file of them:
 *
 *   lda_gzmw_member_kernel  a wave per record: the pieces' sizes summed, the
 *                           record's CRC-32 combined from the pieces', the
 *                           size of its member
 *   (the scan kernels of compact_kernels.hip over those sizes)
 *   lda_gzmw_place_kernel   a wave per record: header, name, footer, the empty
 *                           record's stream, every piece's source and
 *                           destination, the index pair
 *   lda_zipw_copy_kernel    (zip_write_kernels.hip) workgroups stride over the
 *                           PIECES, so one huge record among small ones is
 *                           copied by every CU
 *   lda_gzmw_final_kernel   d_result and the closing index pair
 *
 * The last three write nothing into the file or the index unless all of the
 * file fits out_avail.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"

#define GW_HEADER 10	/* gzip_members_write_plan.h: GZMW_HEADER_BYTES */
#define GW_FOOTER 8
#define GW_EMPTY 5	/* GZMW_EMPTY_STREAM */

/* the name field: the name and its terminator, or nothing */
static __device__ __forceinline__ u64 gw_name_bytes(u64 nl)
{
	return nl ? nl + 1 : 0;
}

/*
 * Record k, pieces first[k] .. + count[k]: csize[k] the bytes of its DEFLATE
 * stream - the pieces' sum; of a record without pieces (0 bytes) the empty
 * final stored block the place kernel writes -, crc[k] its CRC-32 and sizes[k]
 * its member: header, name field, stream, footer.  (Every piece fits its slot:
 * the slot is libdeflate_deflate_compress_bound() of the piece.)
 */
extern "C" __global__ void __launch_bounds__(256)
lda_gzmw_member_kernel(u64 n, const u64 *__restrict__ first, const u64 *__restrict__ count,
		       const u64 *__restrict__ name_len, const u64 *__restrict__ usize,
		       const u64 *__restrict__ pc_off, const u64 *__restrict__ pc_n,
		       const u64 *__restrict__ out_n, const u32 *__restrict__ crcs,
		       u64 *__restrict__ csize, u32 *__restrict__ crc, u64 *__restrict__ sizes)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 np = count[k];
		u64 csum;
		bool missing;
		const u32 sum = zw_combine(lane, first[k], np, usize[k], pc_off, pc_n, out_n, crcs,
					   &csum, &missing);
		if (lane == 0) {
			const u64 cs = np ? csum : GW_EMPTY;
			csize[k] = cs;
			crc[k] = sum;
			sizes[k] = GW_HEADER + gw_name_bytes(name_len[k]) + cs + GW_FOOTER;
		}
	}
}

/*
 * offsets / block_sums: the scan kernels' output over sizes[], so member k
 * stands at offsets[k] + block_sums[k / LDA_SCAN_BLOCK] and the file's size is
 * the grand total.  Writes member k's header (lib/gzip_compress.c:44-64: XFL by
 * level, OS 0xff; FLG 8 and the name with its terminator where the record has
 * one), its footer, piece j's copy (cp_src with ZW_FROM_SLOT into the slots;
 * cp_dst into the file; cp_len) and, index not NULL, the pair
 * libdeflate_amd_gzip_members_index_batch returns for the member.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_gzmw_place_kernel(u64 n, int level, u32 mtime, u64 out_avail,
		      const u64 *__restrict__ first, const u64 *__restrict__ count,
		      const u64 *__restrict__ name_off, const u64 *__restrict__ name_len,
		      const u64 *__restrict__ usize, const u64 *__restrict__ uoff,
		      const u8 *__restrict__ names, const u64 *__restrict__ pc_off,
		      const u64 *__restrict__ pc_n, const u64 *__restrict__ slot_off,
		      const u64 *__restrict__ out_n, const u64 *__restrict__ csize,
		      const u32 *__restrict__ crc, const u64 *__restrict__ offsets,
		      const u64 *__restrict__ block_sums, u8 *__restrict__ out,
		      u64 *__restrict__ cp_src, u64 *__restrict__ cp_dst, u64 *__restrict__ cp_len,
		      u64 *__restrict__ index)
{
	const u32 lane = threadIdx.x & 63;
	const u64 total = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];

	if (total > out_avail)
		return;
	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 np = count[k], nl = name_len[k], cs = csize[k];
		const u64 at = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
		u8 *mem = out + at;
		u8 *stream = mem + GW_HEADER + gw_name_bytes(nl);

		if (lane == 0) {
			zw_put<4>(mem, 0x00088B1Fu | (nl ? 0x08000000u : 0));
			zw_put<4>(mem + 4, mtime);
			zw_put<2>(mem + 8, lda_gzip_xfl(level) | 0xFF00u);
			if (nl)
				stream[-1] = 0;
		} else if (lane == 1) {
			zw_put<4>(stream + cs, crc[k]);
			zw_put<4>(stream + cs + 4, usize[k]);
		} else if (lane == 2 && !np) {
			/* BFINAL 1, BTYPE 00, LEN 0, NLEN ~0 */
			zw_put<1>(stream, 1);
			zw_put<4>(stream + 1, 0xFFFF0000u);
		} else if (lane == 3 && index) {
			index[2 * k] = at;
			index[2 * k + 1] = uoff[k];
		}
		for (u64 i = lane; i < nl; i += 64)
			mem[GW_HEADER + i] = names[name_off[k] + i];
		zw_place_pieces(lane, first[k], np, (u64)(stream - out), true, pc_off, pc_n, slot_off,
				out_n, cp_src, cp_dst, cp_len);
	}
}

/*
 * result[0] = 0 or LIBDEFLATE_INSUFFICIENT_SPACE, [1] the file's size, [2] the
 * records' bytes, [3] the members - and, when the file fits, the closing pair
 * of the index.
 */
extern "C" __global__ void __launch_bounds__(64)
lda_gzmw_final_kernel(u64 n, u64 usize_total, u64 out_avail, const u64 *__restrict__ total_at,
		      u64 *__restrict__ result, u64 *__restrict__ index)
{
	if (threadIdx.x != 0)
		return;
	const u64 total = *total_at;
	const bool ok = total <= out_avail;
	result[0] = ok ? LDA_SUCCESS : LDA_INSUFFICIENT_SPACE;
	result[1] = total;
	result[2] = usize_total;
	result[3] = n;
	if (ok && index) {
		index[2 * n] = total;
		index[2 * n + 1] = usize_total;
	}
}
