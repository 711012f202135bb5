/*
 * zip_write_kernels.hip - a ZIP archive assembled in device memory
 * (host_zip_write.hip: libdeflate_amd_zip_compress_batch).
 *
 * The compress batches have left every piece's raw DEFLATE bytes in a slot and
 * the CRC-32 batch every piece's checksum (zip_write_plan.h).  Four kernels
 * make the archive of them:
 *
 *   lda_zipw_entry_kernel  a wave per entry: the pieces' sizes summed, the
 *                          decision between method 8 and stored, the entry's
 *                          CRC-32 combined from the pieces', the size of its
 *                          local record
 *   (the scan kernels of compact_kernels.hip over those sizes)
 *   lda_zipw_place_kernel  a wave per entry: local header and name, central
 *                          record, every piece's source and destination, the
 *                          index row
 *   lda_zipw_copy_kernel   workgroups stride over the PIECES, so one huge
 *                          entry among small ones is copied by every CU
 *   lda_zipw_final_kernel  one workgroup: the end records and d_result
 *
 * The last three write nothing into the archive unless all of it fits
 * out_avail.  Plain C++, vector stores only.
 */
#include "device_common.h"
#include "kernels.h"
#include "zip_write_device.h"

#define ZW_FIN_THREADS 1024

/* does the archive - cd_off bytes of local records, then tail bytes of
 * directory and end records - fit out_avail?  (no sum that could wrap) */
static __device__ __forceinline__ bool zw_fits(u64 cd_off, u64 tail, u64 out_avail)
{
	return cd_off <= out_avail && out_avail - cd_off >= tail;
}

/*
 * Entry k, pieces first[k] .. + count[k]: e_info[k] = csize | CRC-32 << 32 and
 * sizes[k] = 30 + name + csize.  Method 8 - csize < usize, which is how the
 * later kernels tell - when every piece fitted its slot (out_n != 0) and the
 * sum is shorter than the entry; else stored, csize = usize.  out_n NULL:
 * nothing was compressed.
 *
 * The sums and the CRC-32 are zw_combine()'s (zip_write_device.h).
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zipw_entry_kernel(u64 n, const u64 *__restrict__ first, const u64 *__restrict__ count,
		      const u64 *__restrict__ name_len, const u64 *__restrict__ usize,
		      const u64 *__restrict__ pc_off, const u64 *__restrict__ pc_n,
		      const u64 *__restrict__ out_n, const u32 *__restrict__ crcs,
		      u64 *__restrict__ e_info, u64 *__restrict__ sizes)
{
	const u32 lane = threadIdx.x & 63;

	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 f = first[k], np = count[k], us = usize[k];
		u64 csum;
		bool missing;
		const u32 crc = zw_combine(lane, f, np, us, pc_off, pc_n, out_n, crcs, &csum, &missing);
		const bool deflated = out_n && np && !missing && csum < us;
		if (lane == 0) {
			const u64 cs = deflated ? csum : us;
			e_info[k] = cs | (u64)crc << 32;
			sizes[k] = 30 + (name_len[k] & 0xFFFF) + cs;
		}
	}
}

/*
 * offsets / block_sums: the scan kernels' output over sizes[], so entry k's
 * local header stands at offsets[k] + block_sums[k / LDA_SCAN_BLOCK] and cd_off
 * is the grand total.  Writes entry k's local header and name, its central
 * record at cd_off + cen[k], piece j's copy (cp_src: into d_in, or with
 * ZW_FROM_SLOT into the slots; cp_dst into the archive; cp_len) and, index not
 * NULL, the row libdeflate_amd_zip_index_batch returns for the entry.
 */
extern "C" __global__ void __launch_bounds__(256)
lda_zipw_place_kernel(u64 n, u32 zip64, u32 dos_datetime, u64 out_avail, u64 tail,
		      const u64 *__restrict__ first, const u64 *__restrict__ count,
		      const u64 *__restrict__ name_off, const u64 *__restrict__ name_len,
		      const u64 *__restrict__ cen, const u64 *__restrict__ usize,
		      const u64 *__restrict__ uoff, const u8 *__restrict__ names,
		      const u64 *__restrict__ pc_off, const u64 *__restrict__ pc_n,
		      const u64 *__restrict__ slot_off, const u64 *__restrict__ out_n,
		      const u64 *__restrict__ e_info, const u64 *__restrict__ offsets,
		      const u64 *__restrict__ block_sums, u8 *__restrict__ out,
		      u64 *__restrict__ cp_src, u64 *__restrict__ cp_dst, u64 *__restrict__ cp_len,
		      u64 *__restrict__ index)
{
	const u32 lane = threadIdx.x & 63;
	const u64 cd_off = block_sums[(n + LDA_SCAN_BLOCK - 1) / LDA_SCAN_BLOCK];
	const u32 ver = zip64 ? 45 : 20;

	if (!zw_fits(cd_off, tail, out_avail))
		return;
	for (u64 k = (u64)blockIdx.x * ZW_WAVES + (threadIdx.x >> 6); k < n;
	     k += (u64)gridDim.x * ZW_WAVES) {
		const u64 f = first[k], np = count[k], us = usize[k];
		const u64 cs = e_info[k] & 0xFFFFFFFFull, crc = e_info[k] >> 32;
		const u32 nl = (u32)(name_len[k] & 0xFFFF);
		const u32 gp = name_len[k] >> 32 ? 0x800 : 0;
		const u32 method = cs < us ? 8 : 0;
		const u64 lho = offsets[k] + block_sums[k / LDA_SCAN_BLOCK];
		u8 *loc = out + lho, *rec = out + cd_off + cen[k];

		if (lane == 0) {
			zw_put<4>(loc, 0x04034B50u);
			zw_put<2>(loc + 4, ver);
			zw_put<2>(loc + 6, gp);
			zw_put<2>(loc + 8, method);
			zw_put<4>(loc + 10, dos_datetime);	/* time, date */
			zw_put<4>(loc + 14, crc);
			zw_put<4>(loc + 18, cs);
			zw_put<4>(loc + 22, us);
			zw_put<2>(loc + 26, nl);
			zw_put<2>(loc + 28, 0);
		} else if (lane == 1) {
			zw_put<4>(rec, 0x02014B50u);
			zw_put<2>(rec + 4, ver);	/* made by: 2.0 / 4.5, MS-DOS attributes */
			zw_put<2>(rec + 6, ver);
			zw_put<2>(rec + 8, gp);
			zw_put<2>(rec + 10, method);
			zw_put<4>(rec + 12, dos_datetime);
			zw_put<4>(rec + 16, crc);
			zw_put<4>(rec + 20, cs);
			zw_put<4>(rec + 24, us);
			zw_put<2>(rec + 28, nl);
			zw_put<2>(rec + 30, zip64 ? 12 : 0);
			zw_put<8>(rec + 32, 0);		/* comment, disk, attributes */
			zw_put<2>(rec + 40, 0);
			zw_put<4>(rec + 42, zip64 ? 0xFFFFFFFFu : lho);
		} else if (lane == 2 && zip64) {
			zw_put<4>(rec + 46 + nl, 0x00080001u);
			zw_put<8>(rec + 50 + nl, lho);
		} else if (lane == 3 && index) {
			u64 *row = index + LDA_ZIP_WORDS * k;
			row[0] = cd_off + cen[k];
			row[1] = nl;
			row[2] = method | gp << 16;
			row[3] = crc;
			row[4] = lho + 30 + nl;
			row[5] = cs;
			row[6] = us;
			row[7] = uoff[k];
		}
		for (u32 i = lane; i < nl; i += 64) {
			const u8 ch = names[name_off[k] + i];
			loc[30 + i] = ch;
			rec[46 + i] = ch;
		}
		/* the pieces back to back behind the name */
		zw_place_pieces(lane, f, np, lho + 30 + nl, method != 0, pc_off, pc_n, slot_off, out_n,
				cp_src, cp_dst, cp_len);
	}
}

/* piece c: cp_len[c] bytes from d_in or from the slots to out + cp_dst[c] */
extern "C" __global__ void __launch_bounds__(256)
lda_zipw_copy_kernel(u64 np, const u64 *__restrict__ total_at, u64 out_avail, u64 tail,
		     const u64 *__restrict__ cp_src, const u64 *__restrict__ cp_dst,
		     const u64 *__restrict__ cp_len, const u8 *__restrict__ in,
		     const u8 *__restrict__ slots, u8 *__restrict__ out)
{
	const u32 tid = threadIdx.x;

	if (!zw_fits(*total_at, tail, out_avail))
		return;
	for (u64 c = blockIdx.x; c < np; c += gridDim.x) {
		const u64 s = cp_src[c];
		const u8 *src = s & ZW_FROM_SLOT ? slots + (s & ~ZW_FROM_SLOT) : in + s;
		copy_span(src, out + cp_dst[c], cp_len[c], tid);
	}
}

/*
 * One workgroup: result[0] = 0 or LIBDEFLATE_INSUFFICIENT_SPACE, [1] the
 * archive's size, [2] cd_off, [3] the entries that got method 8 - and, when
 * the archive fits, the records behind the directory: in ZIP64 mode the ZIP64
 * end record, its locator and an end record of sentinels, else the plain one.
 */
extern "C" __global__ void __launch_bounds__(ZW_FIN_THREADS)
lda_zipw_final_kernel(u64 n, u32 zip64, u64 out_avail, u64 cd_size, u64 tail,
		      const u64 *__restrict__ usize, const u64 *__restrict__ e_info,
		      const u64 *__restrict__ total_at, u8 *__restrict__ out,
		      u64 *__restrict__ result)
{
	__shared__ u64 sh[ZW_FIN_THREADS / 64];
	const u32 tid = threadIdx.x;
	u64 deflated = 0;

	for (u64 k = tid; k < n; k += ZW_FIN_THREADS)
		deflated += (e_info[k] & 0xFFFFFFFFull) < usize[k];
	deflated = wave_sum64(deflated);
	if ((tid & 63) == 0)
		sh[tid >> 6] = deflated;
	__syncthreads();
	if (tid != 0)
		return;
	deflated = 0;
	for (u32 w = 0; w < ZW_FIN_THREADS / 64; w++)
		deflated += sh[w];
	const u64 cd_off = *total_at;
	const bool ok = zw_fits(cd_off, tail, out_avail);
	if (ok) {
		u8 *p = out + cd_off + cd_size;
		if (zip64) {
			zw_put<4>(p, 0x06064B50u);
			zw_put<8>(p + 4, 44);		/* bytes of the record behind this field */
			zw_put<2>(p + 12, 45);
			zw_put<2>(p + 14, 45);
			zw_put<8>(p + 16, 0);		/* this disk, the directory's disk */
			zw_put<8>(p + 24, n);
			zw_put<8>(p + 32, n);
			zw_put<8>(p + 40, cd_size);
			zw_put<8>(p + 48, cd_off);
			zw_put<4>(p + 56, 0x07064B50u);
			zw_put<4>(p + 60, 0);
			zw_put<8>(p + 64, cd_off + cd_size);
			zw_put<4>(p + 72, 1);		/* disks in all */
			p += 76;
		}
		zw_put<4>(p, 0x06054B50u);
		zw_put<4>(p + 4, 0);			/* this disk, the directory's disk */
		zw_put<2>(p + 8, zip64 ? 0xFFFFu : n);
		zw_put<2>(p + 10, zip64 ? 0xFFFFu : n);
		zw_put<4>(p + 12, zip64 ? 0xFFFFFFFFu : cd_size);
		zw_put<4>(p + 16, zip64 ? 0xFFFFFFFFu : cd_off);
		zw_put<2>(p + 20, 0);			/* no comment */
	}
	result[0] = ok ? LDA_SUCCESS : LDA_INSUFFICIENT_SPACE;
	result[1] = cd_off + tail;
	result[2] = cd_off;
	result[3] = deflated;
}
