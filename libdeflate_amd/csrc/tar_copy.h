/*
 * tar_copy.h - the workgroup copy of the tar reader's gather
 * (tar_kernels.hip) and of the tar writer's pack (tar_write_kernels.hip), and
 * the writer's zero fill in the same shape.
 */
#ifndef LDA_TAR_COPY_H
#define LDA_TAR_COPY_H

#include "device_common.h"

/* len bytes src -> dst by a 256-thread workgroup, as copy_span(): bytes up to
 * the first 16-byte boundary of dst, 16-byte stores with four loads in flight
 * per thread, the tail */
static __device__ __forceinline__ void
copy_tile(const u8 *__restrict__ src, u8 *__restrict__ dst, u64 len, u32 tid)
{
	u64 head = (0 - (uintptr_t)dst) & 15;
	if (head > len)
		head = len;
	if (tid < head)
		dst[tid] = src[tid];
	const u64 body = (len - head) & ~(u64)15;
	const u8 *s = src + head;
	u8 *d = dst + head;
	u64 k = 16 * (u64)tid;
	for (; k + 3 * 4096 < body; k += 4 * 4096) {
		uint4 v[4];
#pragma unroll
		for (u32 i = 0; i < 4; i++)
			__builtin_memcpy(&v[i], s + k + 4096 * i, 16);	/* source may be unaligned */
#pragma unroll
		for (u32 i = 0; i < 4; i++)
			*(uint4 *)(d + k + 4096 * i) = v[i];
	}
	for (; k < body; k += 4096) {
		uint4 v;
		__builtin_memcpy(&v, s + k, 16);
		*(uint4 *)(d + k) = v;
	}
	const u64 tail = head + body;
	if (tail + tid < len)
		dst[tail + tid] = src[tail + tid];
}

/* len zero bytes (no more than a tile) at dst by a 256-thread workgroup, in
 * the same three parts */
static __device__ __forceinline__ void zero_tile(u8 *__restrict__ dst, u32 len, u32 tid)
{
	u32 head = (0 - (u32)(uintptr_t)dst) & 15;
	if (head > len)
		head = len;
	if (tid < head)
		dst[tid] = 0;
	const u32 body = (len - head) & ~15u;
	u8 *d = dst + head;
	for (u32 k = 16 * tid; k < body; k += 4096)
		*(uint4 *)(d + k) = make_uint4(0, 0, 0, 0);
	const u32 tail = head + body;
	if (tail + tid < len)
		dst[tail + tid] = 0;
}

#endif /* LDA_TAR_COPY_H */
