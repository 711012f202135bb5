/*
 * zip_large_kernels.hip - the one kernel of libdeflate_amd_zip_read_large
 * (host_zip_large.hip; the plan is zip_large_plan.h): the results of the
 * entries that left the one-wave batch.
 *
 *   lda_zip_lfinal_kernel  a wave per owned entry (many-wave, pieced or both):
 *                          the CRC-32 of a pieced entry combined from its
 *                          pieces' values (zw_combine(), zip_write_device.h),
 *                          compared with the row's; the decoder's verdict from
 *                          where it is - the host's columns for a many-wave
 *                          entry, the batch's for any other; the result word.
 *
 * Every other row of the selection is lda_zip_rfinal_kernel's (zip_kernels.hip),
 * which the host launches over the runs of rows in between: bit LDA_ZIPL_OWNED
 * of meta[r] marks the rows of this kernel, and it writes no other.  The
 * tables come from the host's plan; their indices are checked all the same
 * against the sizes the host passed.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"

/*
 * lda_zip_rfinal_kernel's precedence (entry_result() of zip_kernels.hip): the
 * pre-decode result, the decoder's, "input not used up", the CRC-32.
 */
static __device__ __forceinline__ s32
lfinal_result(u64 meta, s32 dec_res, u64 actual_in, u64 in_n, u32 crc)
{
	const s32 pre = (s32)((meta >> 32) & 0xFF);
	const u32 kind = (u32)(meta >> 40) & 3;

	if (pre != LDA_SUCCESS || kind == LDA_ZIP_KIND_NONE)
		return pre;
	if (kind == LDA_ZIP_KIND_DEFLATE) {
		if (dec_res != LDA_SUCCESS)
			return dec_res;
		if (actual_in != in_n)
			return LDA_BAD_DATA;
	}
	return crc == (u32)meta ? LDA_SUCCESS : LDA_BAD_DATA;
}

/*
 * Owned entry j: selection l_sel[j], flags l_flags[j], csize l_in_n[j], usize
 * l_usize[j], pieces l_first[j] .. + l_count[j] of the n_pieces pieces (p_dst:
 * where a piece lies in the output, p_len: its bytes, p_crcs: its CRC-32), and
 * for a many-wave entry l_res[j] / l_ain[j], the result and actual_in of its
 * libdeflate_amd_decompress_large.  meta, batch_res, batch_ain, batch_crcs:
 * the n_sel words lda_zip_rfinal_kernel reads.  An entry whose tables do not
 * hold together - they always do - is LDA_BAD_DATA.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zip_lfinal_kernel(u64 n_own, u64 n_sel, u64 n_pieces, const u64 *__restrict__ l_sel,
		      const u64 *__restrict__ l_flags, const u64 *__restrict__ l_in_n,
		      const u64 *__restrict__ l_usize, const u64 *__restrict__ l_first,
		      const u64 *__restrict__ l_count, const u64 *__restrict__ l_res,
		      const u64 *__restrict__ l_ain, const u64 *__restrict__ meta,
		      const s32 *__restrict__ batch_res, const u64 *__restrict__ batch_ain,
		      const u32 *__restrict__ batch_crcs, const u64 *__restrict__ p_dst,
		      const u64 *__restrict__ p_len, const u32 *__restrict__ p_crcs,
		      s32 *__restrict__ results)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 j = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); j < n_own;
	     j += (u64)gridDim.x * ZW_WAVES) {
		const u64 r = l_sel[j];	/* (uniform, as everything of entry j) */
		if (r >= n_sel)
			continue;
		const u64 m = meta[r];
		if (!(m >> LDA_ZIPL_OWNED & 1))
			continue;
		const u64 flags = l_flags[j], f = l_first[j], np = l_count[j], us = l_usize[j];
		const bool many = flags & LDA_ZIPL_MANY_WAVE, pieced = flags & LDA_ZIPL_PIECED;
		bool sound = many || pieced;
		u32 crc = 0;

		if (pieced) {
			if (np == 0 || f > n_pieces || np > n_pieces - f) {
				sound = false;
			} else {
				u64 csum;
				bool missing;
				crc = zw_combine(lane, f, np, us, p_dst, p_len, NULL, p_crcs, &csum,
						 &missing);
			}
		} else {
			crc = batch_crcs[r];
		}
		const s32 dec_res = many ? (s32)l_res[j] : batch_res[r];
		const u64 dec_ain = many ? l_ain[j] : batch_ain[r];
		if (lane == 0)
			results[r] = sound ? lfinal_result(m, dec_res, dec_ain, l_in_n[j], crc) :
					     LDA_BAD_DATA;
	}
}
