/*
 * zip_write_device.h - what the kernels of the two container writers share
 * (zip_write_kernels.hip, gzip_members_write_kernels.hip): both assemble their
 * file from pieces that the compress batches left in slots and whose CRC-32
 * the checksum batch left beside them (zip_write_plan.h: zipw_cut_pieces()), a
 * wave per entry.  Plain C++, vector stores only.
 */
#ifndef LDA_ZIP_WRITE_DEVICE_H
#define LDA_ZIP_WRITE_DEVICE_H

#include "device_common.h"
#include "large_plan.h"

#define ZW_X8 0x00800000u		/* x^8: what appending one byte multiplies a CRC by */
#define ZW_WAVES 4			/* entries per 256-thread workgroup */
#define ZW_FROM_SLOT ((u64)1 << 63)	/* cp_src: an offset into the slots, not into d_in */

/* nbytes of v, little endian, at any alignment */
template <u32 NBYTES> static __device__ __forceinline__ void zw_put(u8 *p, u64 v)
{
#pragma unroll
	for (u32 i = 0; i < NBYTES; i++)
		p[i] = (u8)(v >> (8 * i));
}

/*
 * One wave, one entry of us bytes, pieces [f, f + np): the CRC-32 of the whole
 * from the pieces' (returned in every lane), the sum of the pieces' compressed
 * sizes (out_n NULL: nothing was compressed, 0) and whether a piece did not fit
 * its slot (out_n == 0).
 *
 * The CRC-32 as lda_large_finalize_kernel combines it: every lane takes a
 * contiguous run of the pieces in Horner form - a multiply by x^(8 len) per
 * piece, xS for the pieces as long as the first - and one multiply by
 * x^(8 bytes behind the run); XOR over the lanes.
 */
static __device__ __forceinline__ u32
zw_combine(u32 lane, u64 f, u64 np, u64 us, const u64 *__restrict__ pc_off,
	   const u64 *__restrict__ pc_n, const u64 *__restrict__ out_n,
	   const u32 *__restrict__ crcs, u64 *csum_ret, bool *missing_ret)
{
	const u64 run = (np + 63) / 64;
	const u64 a = lane * run < np ? lane * run : np;
	const u64 b = a + run < np ? a + run : np;
	const u64 S = np ? pc_n[f] : 0;
	const u32 xS = lda_crc_powmod(ZW_X8, S);
	u64 csum = 0;
	u32 acc = 0;
	bool missing = false;

	for (u64 i = a; i < b; i++) {
		const u64 len = pc_n[f + i];
		acc = lda_crc_mulmod(acc, len == S ? xS : lda_crc_powmod(ZW_X8, len)) ^
		      crcs[f + i];
		if (out_n) {
			const u64 o = out_n[f + i];
			csum += o;
			missing |= o == 0;
		}
	}
	if (a < b) {
		const u64 behind = us - (pc_off[f + b - 1] + pc_n[f + b - 1] - pc_off[f]);
		if (behind)
			acc = lda_crc_mulmod(acc, lda_crc_powmod(ZW_X8, behind));
	}
	*csum_ret = wave_sum64(csum);
	*missing_ret = __ballot(missing) != 0;
	return wave_xor(acc);
}

/*
 * One wave: the copies of an entry's pieces, back to back from offset `at` of
 * the file - from their slots (out_n bytes each) or, from_slot false, the
 * pieces' own bytes in d_in.  Returns the offset behind the last.
 */
static __device__ __forceinline__ u64
zw_place_pieces(u32 lane, u64 f, u64 np, u64 at, bool from_slot, const u64 *__restrict__ pc_off,
		const u64 *__restrict__ pc_n, const u64 *__restrict__ slot_off,
		const u64 *__restrict__ out_n, u64 *__restrict__ cp_src, u64 *__restrict__ cp_dst,
		u64 *__restrict__ cp_len)
{
	for (u64 base = 0; base < np; base += 64) {
		const u64 j = f + base + lane;
		const bool live = base + lane < np;
		const u64 len = !live ? 0 : from_slot ? out_n[j] : pc_n[j];
		const u64 incl = wave_scan_incl64(len);
		if (live) {
			cp_src[j] = from_slot ? slot_off[j] | ZW_FROM_SLOT : pc_off[j];
			cp_dst[j] = at + incl - len;
			cp_len[j] = len;
		}
		at += wave_sum64(len);
	}
	return at;
}

#endif /* LDA_ZIP_WRITE_DEVICE_H */
