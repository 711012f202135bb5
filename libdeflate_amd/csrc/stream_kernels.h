/*
 * stream_kernels.h - what inflate_stream.hip (the kernels that decode ONE
 * large stream on many waves) shares with host_stream.hip.
 */
#ifndef LDA_STREAM_KERNELS_H
#define LDA_STREAM_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stream_types.h"

extern "C" __global__ void
lda_stream_count_kernel(uint32_t nchunks, const struct lda_stream_chunk *chunks,
			struct lda_stream_res *res, const uint8_t *inp, uint64_t in_n,
			uint32_t *tokscratch, const uint8_t *hdr_lens, const uint32_t *hdr_info,
			uint16_t *hints);
extern "C" __global__ void
lda_stream_decode_kernel(uint32_t nchunks, const struct lda_stream_chunk *chunks,
			 struct lda_stream_res *res, const uint8_t *inp, uint64_t in_n,
			 uint16_t *sym, uint32_t *tokscratch, const uint8_t *hdr_lens,
			 const uint32_t *hdr_info, const uint16_t *hints);
extern "C" __global__ void
lda_stream_hdr_cache_kernel(const uint8_t *inp, uint64_t in_n, const uint64_t *cand,
			    const uint32_t *ncand, uint32_t nslots, uint8_t *hdr_lens,
			    uint32_t *hdr_info);
extern "C" size_t lda_stream_hdr_cache_lds(void);
#define LDA_STREAM_HDR_SLOTS 8192u	/* headers of a window parsed ahead (320 + 16 bytes each) */
extern "C" __global__ void
lda_stream_find_a_kernel(const uint8_t *inp, uint64_t in_n, uint64_t bit0, uint64_t nbits,
			 uint64_t *queue, uint32_t *qcount, uint32_t qcap);
extern "C" __global__ void
lda_stream_find_b_kernel(const uint8_t *inp, uint64_t in_n, const uint64_t *queue,
			 const uint32_t *qcount, uint32_t qcap, uint64_t *cand,
			 uint32_t *ncand, uint32_t ccap);
extern "C" __global__ void
lda_stream_window_kernel(uint32_t nchunks, uint32_t per_group, uint32_t phase,
			 const uint64_t *out_off, const uint16_t *sym, uint8_t *out,
			 uint16_t *gwin, const uint16_t *fwin, uint32_t *err);
extern "C" __global__ void
lda_stream_window_scan_kernel(uint32_t n, uint32_t h, const uint16_t *src, uint16_t *dst);
extern "C" __global__ void
lda_stream_resolve_kernel(uint32_t nchunks, uint32_t chunk0, const uint64_t *out_off,
			  const uint16_t *sym, uint8_t *out, uint32_t *err);
extern "C" size_t lda_stream_chunk_lds(void);
extern "C" size_t lda_stream_find_b_lds(void);
extern "C" size_t lda_stream_tokcap(void);	/* u32 words of token scratch per decode wave */

/* stream_probe_kernels.hip: what the host reads out of a stream in host memory
 * itself, for a stream in device memory.  rows[]: struct lda_stored_row
 * (stored_rows.h) as one 16-byte store each; cls[i] = { longest literal
 * codeword of a block of one codeword length or 0, bits from the header of
 * slot i to its first token }. */
extern "C" __global__ void
lda_stream_find_stored_kernel(const uint8_t *inp, uint64_t in_n, uint64_t bp0, uint4 *rows,
			      uint32_t *count, uint32_t cap);
extern "C" __global__ void
lda_stream_hdr_class_kernel(const uint32_t *ncand, uint32_t nslots, const uint8_t *hdr_lens,
			    const uint32_t *hdr_info, uint2 *cls);

/*
 * The seek index and its ranged reads (host_seek.hip, seek_plan.h).
 * lda_seek_decode_kernel (inflate_stream.hip): interval j into its slot of the
 * symbol scratch, if the count pass ended where the index says: want[2j] = the
 * end bit (last interval: 2^63 | bytes of the raw stream), want[2j + 1] = the
 * bytes; else fail[j] = 1 and nothing is written.
 * seek_kernels.hip: the 32 KiB in front of every point out of the output; one
 * piece (a range's share of an interval) from symbols to bytes - piece p is
 * pieces[4p ..] = { interval | range << 32, first symbol, offset in out, bytes },
 * lowest[j] = the first marker index that exists in window j; a range's
 * verdict from its pieces' intervals.
 */
extern "C" __global__ void
lda_seek_decode_kernel(uint32_t nchunks, const struct lda_stream_chunk *chunks,
		       const struct lda_stream_res *counted, const uint64_t *want,
		       struct lda_stream_res *res, const uint8_t *inp, uint64_t in_n,
		       uint16_t *sym, uint32_t *tokscratch, uint32_t *fail);
extern "C" __global__ void
lda_seek_window_kernel(uint32_t npoints, const uint64_t *out_off, const uint8_t *out,
		       uint8_t *windows);
extern "C" __global__ void
lda_seek_resolve_kernel(uint32_t npieces, uint32_t piece0, const uint64_t *pieces,
			const uint64_t *win_of, const uint32_t *lowest, const uint16_t *sym,
			const uint8_t *windows, uint8_t *out, uint32_t *fail);
extern "C" __global__ void
lda_seek_verdict_kernel(uint32_t nranges, const uint64_t *first, const uint64_t *pieces,
			const uint32_t *fail, int32_t *results);

#endif /* LDA_STREAM_KERNELS_H */
