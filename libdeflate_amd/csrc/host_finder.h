/*
 * host_finder.h - the candidate finder the readers of BGZF files
 * (host_bgzf_read.hip), concatenated gzip members (host_gzip_members.hip) and
 * ZIP directories (host_zip.hip) share: a scan kernel of the format lists the
 * offsets that look like a record, and the chain kernels of
 * bgzf_read_kernels.hip keep the candidates that the chain of record sizes
 * reaches from position 0.  What fills cand_size between the two is the
 * format's own.
 */
#ifndef LDA_HOST_FINDER_H
#define LDA_HOST_FINDER_H

#include "host_common.h"
#include "kernels.h"

namespace lda {

/* the limits of the three readers: candidate indices and record counts are 32 bits */
#define LDA_FINDER_MAX_RECORDS ((size_t)1 << 28)
#define LDA_FINDER_MAX_FILE ((size_t)1 << 36)

/* the finder's part of a reader's scratch */
struct Finder {
	size_t cap, nwg, nsb_a, nblk;	/* room for candidates, scan workgroups, their scan blocks, chain blocks */
	uint32_t *state;		/* LDA_BR_STATE_WORDS */
	uint64_t *cand_pos, *counts, *offs, *bsum_a;
	uint32_t *cand_size, *next, *exit_at, *hops, *entry, *base;

	/* a file of n bytes, room for cap_ candidates: the candidates and their
	 * scan.  The arrays of the chain follow behind the reader's own u64
	 * arrays (carve_chain()), so every array lies where it lay before the
	 * readers shared this */
	void carve(Carve &c, size_t n, size_t cap_)
	{
		cap = cap_;
		nwg = (n + LDA_BR_SCAN_WG - 1) / LDA_BR_SCAN_WG;
		nsb_a = scan_blocks(nwg);
		nblk = (cap + LDA_BR_JUMP - 1) / LDA_BR_JUMP;
		state = c.take<uint32_t>(LDA_BR_STATE_WORDS);
		cand_pos = c.take<uint64_t>(cap);
		counts = c.take<uint64_t>(nwg);
		offs = c.take<uint64_t>(nwg);
		bsum_a = c.take<uint64_t>(nsb_a + 1);
	}
	void carve_chain(Carve &c)
	{
		cand_size = c.take<uint32_t>(cap);
		next = c.take<uint32_t>(cap);
		exit_at = c.take<uint32_t>(cap);
		hops = c.take<uint32_t>(cap);
		entry = c.take<uint32_t>(nblk);
		base = c.take<uint32_t>(nblk);
	}
	/* where the device finds the candidate count */
	const uint64_t *k_at() const { return bsum_a + nsb_a; }
};

/* the state words cleared and the candidates listed: count, scan, write in
 * file order.  scan(offsets, block_sums) launches the format's scan kernel
 * over f.nwg workgroups, with NULLs for the count pass */
template <typename Scan> static inline int finder_list(const Finder &f, hipStream_t st, Scan scan)
{
	LDA_HIP_TRY(hipMemsetAsync(f.state, 0, LDA_BR_STATE_WORDS * 4, st), LIBDEFLATE_AMD_NO_DEVICE);
	scan((const uint64_t *)NULL, (const uint64_t *)NULL);
	scan_enqueue(st, f.nwg, f.counts, f.offs, f.bsum_a);
	scan((const uint64_t *)f.offs, (const uint64_t *)f.bsum_a);
	return LIBDEFLATE_AMD_OK;
}

/* the chain among the candidates, from position 0 to `end`: record k's
 * position lands in in_off[k], its size in in_n[k], for k < M (none of these
 * does anything when the candidates overflowed their room) */
static inline void finder_chain(const Finder &f, hipStream_t st, uint64_t end, size_t M,
				uint64_t *in_off, uint64_t *in_n)
{
	const uint64_t *k_at = f.k_at();
	const uint64_t cap = f.cap;

	hipLaunchKernelGGL(lda_bgzf_jump_kernel, dim3((unsigned)f.nblk), dim3(LDA_BR_JUMP), 0, st, end,
			   k_at, cap, (const uint64_t *)f.cand_pos, (const uint32_t *)f.cand_size,
			   f.next, f.exit_at, f.hops, f.entry);
	hipLaunchKernelGGL(lda_bgzf_top_kernel, dim3(1), dim3(64), 0, st, k_at, cap,
			   (const uint64_t *)f.cand_pos, (const uint32_t *)f.exit_at,
			   (const uint32_t *)f.hops, f.entry, f.base, f.state);
	hipLaunchKernelGGL(lda_bgzf_members_kernel, dim3((unsigned)f.nblk), dim3(LDA_BR_JUMP), 0, st,
			   k_at, cap, (uint64_t)M, (const uint64_t *)f.cand_pos,
			   (const uint32_t *)f.cand_size, (const uint32_t *)f.next,
			   (const uint32_t *)f.hops, (const uint32_t *)f.entry,
			   (const uint32_t *)f.base, (const uint32_t *)f.state, in_off, in_n);
}

/* what the device calls of the three readers check before they touch a
 * device: count_msg (what, max_count, n) is the message for a max_count
 * outside min_count .. 2^28 */
static inline bool finder_args_ok(const char *what, const void *d, const void *d_in, size_t n,
				  const char *count_msg, size_t max_count, size_t min_count,
				  const void *d_result)
{
	if (!d || (!d_in && n) || !d_result) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (max_count < min_count || max_count > LDA_FINDER_MAX_RECORDS) {
		set_error(count_msg, what, max_count, n);
		return false;
	}
	if (n > LDA_FINDER_MAX_FILE) {
		set_error("%s: in_nbytes %zu above 2^36", what, n);
		return false;
	}
	return true;
}

} /* namespace lda */

#endif /* LDA_HOST_FINDER_H */
