/*
 * write_pieces_plan.h - the pieces of the writers that compress many buffers
 * into one output (zip_write_plan.h, gzip_members_write_plan.h,
 * png_write_plan.h): every buffer cut into the pieces the compress and
 * checksum batches run on, the pieces' slots, the launch groups and the list of
 * compress launches host_write_pieces.hip walks.  Free of HIP:
 * tools/test_zip_write_plan.cpp runs it on the CPU.
 *
 * A buffer for which lda_large_segmented() holds is cut exactly as
 * libdeflate_amd_compress_large_batch cuts its one buffer (large_plan.h: S by
 * size, every segment primed with the tiles in front of it); any other buffer
 * is one piece; an empty buffer has none.  Where nothing is compressed (store)
 * the pieces only carry the checksum and the copy, and every buffer of
 * LDA_LARGE_MIN bytes or more is cut.
 *
 * The pieces are ordered by the LAUNCH GROUP of their buffer, buffers in the
 * caller's order inside a group: buffers the small-buffer kernel takes, other
 * whole buffers, and one group per segment size S.  Every group is compressed
 * by launches of its own, so each piece meets the kernel, the seg_info and the
 * size bound that a single-buffer call on its buffer would give it.
 */
#ifndef LDA_WRITE_PIECES_PLAN_H
#define LDA_WRITE_PIECES_PLAN_H

#include <stdint.h>
#include <vector>

#include "large_plan.h"

namespace lda {

enum {
	/* the per-piece columns, np words each */
	ZIPW_P_IN_OFF = 0,	/* what the compress kernel reads: the prime in front */
	ZIPW_P_IN_N,
	ZIPW_P_SLOT_OFF,	/* its slot, from the start of the slots */
	ZIPW_P_SLOT_AV,
	ZIPW_P_PC_OFF,		/* the piece itself, in its source: what the checksum covers */
	ZIPW_P_PC_N,
	ZIPW_PCOLS
};

/* what the object and the build decide */
struct zipw_params {
	int level;
	bool store;		/* level 0 or LIBDEFLATE_AMD_ZIP_STORE: nothing is compressed */
	bool no_segments;	/* LDA_NO_SEGMENTS */
	uint64_t env_seg;	/* LDA_SEG_BYTES, 0 = by size */
	uint64_t D, tile;	/* lda_large_shape's */
	uint64_t small_max;	/* entries up to this take the small-buffer kernel; 0: none does */
};

/* pieces [lo, hi): one kind of compress launch */
struct zipw_group {
	uint64_t lo, hi;
	uint64_t max_in;	/* the size bound of its launches */
	uint64_t S;		/* segment size, 0: whole entries (no seg_info) */
};

/* the pieces of many entries: what zipw_cut_pieces() leaves */
struct zipw_pieces {
	uint64_t np, slots_bytes;
	std::vector<uint64_t> pcols;	/* ZIPW_PCOLS x np */
	std::vector<uint32_t> seg_info;	/* np */
	std::vector<zipw_group> groups;	/* empty where nothing is compressed */
};

/* one compress launch: pieces [lo, lo + count) of one group.  count, max_in and
 * segmented are also what the launch asks of compress_pieces_scratch() */
struct zipw_launch {
	uint64_t lo, count;
	uint64_t max_in;	/* its group's */
	bool segmented;		/* with seg_info */
};

/* every compress launch of the pieces, in piece order: a group of segments as
 * the segmented single-buffer path slices it, lda_large_per_slice(S) pieces a
 * launch, a group of whole entries in one launch (which slices itself where
 * its token lists need it) */
static inline std::vector<zipw_launch> zipw_launches(const zipw_pieces &p)
{
	std::vector<zipw_launch> out;
	out.reserve(p.groups.size());	/* (one launch a group, but for large segmented ones) */
	for (const zipw_group &g : p.groups) {
		const uint64_t per = g.S ? lda_large_per_slice(g.S) : g.hi - g.lo;
		for (uint64_t lo = g.lo; lo < g.hi; lo += per) {
			const zipw_launch l = { lo, per < g.hi - lo ? per : g.hi - lo, g.max_in, g.S != 0 };
			out.push_back(l);
		}
	}
	return out;
}

/* the slot a piece of len bytes is compressed into: room for
 * libdeflate_deflate_compress_bound(len) - 5 bytes per 5000-byte block - as
 * the segmented single-buffer path sizes its slots */
static inline uint64_t zipw_slot(uint64_t len)
{
	uint64_t blocks = (len + 4999) / 5000;
	if (blocks < 1)
		blocks = 1;
	return (5 * blocks + len + 32 + 15) / 16 * 16;
}

/* is the entry cut into segments, and of what size? */
static inline uint64_t zipw_seg_bytes(const zipw_params &pr, uint64_t usize)
{
	const bool cut = pr.store ? usize >= LDA_LARGE_MIN :
				    lda_large_segmented(usize, pr.level, pr.no_segments);
	return cut ? lda_large_seg_bytes(usize, pr.env_seg) : 0;
}

/* a segment's bytes: its own and at most D (whole tiles) in front */
static inline uint64_t zipw_seg_bound(const zipw_params &pr, uint64_t S)
{
	return S + (pr.D + pr.tile - 1) / pr.tile * pr.tile;
}

/*
 * Entries of in_nbytes[k] bytes at in_offsets[k], cut into pieces: first[k] and
 * cnt[k] (n words each) get every entry's piece range, p the pieces' columns in
 * launch-group order, their slots and the groups.
 */
static inline void
zipw_cut_pieces(const zipw_params &pr, uint64_t n, const uint64_t *in_offsets,
		const uint64_t *in_nbytes, uint64_t *first, uint64_t *cnt, zipw_pieces &p)
{
	enum { G_SMALL = 0, G_WHOLE = 1, G_SEG = 2 };
	std::vector<uint64_t> seg_sizes;	/* the distinct S, in the order met */
	std::vector<uint64_t> count(G_SEG);
	std::vector<uint32_t> group_of((size_t)n);

	for (uint64_t k = 0; k < n; k++) {
		const uint64_t usize = in_nbytes[k];
		const uint64_t S = zipw_seg_bytes(pr, usize);
		uint32_t g = G_SMALL;
		if (pr.store) {
			g = G_SMALL;	/* one group: nothing is launched for it */
		} else if (S) {
			size_t s = 0;
			while (s < seg_sizes.size() && seg_sizes[s] != S)
				s++;
			if (s == seg_sizes.size()) {
				seg_sizes.push_back(S);
				count.push_back(0);
			}
			g = G_SEG + (uint32_t)s;
		} else if (usize > pr.small_max) {
			g = G_WHOLE;
		}
		group_of[(size_t)k] = g;
		cnt[k] = S ? (usize + S - 1) / S : usize ? 1 : 0;
		count[g] += cnt[k];
	}
	/* the groups' piece ranges, then every entry's pieces at its group's cursor */
	std::vector<uint64_t> cursor(count.size());
	p.np = 0;
	p.groups.clear();
	for (size_t g = 0; g < count.size(); g++) {
		cursor[g] = p.np;
		if (count[g] && !pr.store) {
			zipw_group gr = { p.np, p.np + count[g], 0, 0 };
			if (g >= G_SEG) {
				gr.S = seg_sizes[g - G_SEG];
				gr.max_in = zipw_seg_bound(pr, gr.S);
			}
			p.groups.push_back(gr);
		}
		p.np += count[g];
	}
	const uint64_t np = p.np;
	p.pcols.assign((size_t)(ZIPW_PCOLS * np), 0);
	p.seg_info.assign((size_t)np, 0);
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t usize = in_nbytes[k], S = zipw_seg_bytes(pr, usize);
		const uint32_t g = group_of[(size_t)k];
		first[k] = cursor[g];
		if (S) {
			const lda_large_shape shape = { usize, S, pr.D, pr.tile, cnt[k],
							pr.store ? 0 : zipw_slot(S), in_offsets[k], 0 };
			for (uint64_t i = 0; i < cnt[k]; i++) {
				const lda_large_seg s = lda_large_seg_of(shape, i);
				const uint64_t j = cursor[g] + i;
				p.pcols[ZIPW_P_IN_OFF * np + j] = s.in_off;
				p.pcols[ZIPW_P_IN_N * np + j] = s.in_n;
				p.pcols[ZIPW_P_SLOT_AV * np + j] = s.out_av;
				p.pcols[ZIPW_P_PC_OFF * np + j] = s.pc_off;
				p.pcols[ZIPW_P_PC_N * np + j] = s.pc_n;
				p.seg_info[(size_t)j] = s.info;
			}
		} else if (usize) {
			const uint64_t j = cursor[g];
			p.pcols[ZIPW_P_IN_OFF * np + j] = in_offsets[k];
			p.pcols[ZIPW_P_IN_N * np + j] = usize;
			p.pcols[ZIPW_P_SLOT_AV * np + j] = pr.store ? 0 : zipw_slot(usize);
			p.pcols[ZIPW_P_PC_OFF * np + j] = in_offsets[k];
			p.pcols[ZIPW_P_PC_N * np + j] = usize;
			p.seg_info[(size_t)j] = 0x80000000u;
		}
		cursor[g] += cnt[k];
	}
	/* slots back to back in piece order; a whole-entry group's size bound */
	uint64_t at = 0;
	for (uint64_t j = 0; j < np; j++) {
		p.pcols[ZIPW_P_SLOT_OFF * np + j] = at;
		at += p.pcols[ZIPW_P_SLOT_AV * np + j];
	}
	p.slots_bytes = at;
	for (zipw_group &gr : p.groups)
		if (!gr.S)
			for (uint64_t j = gr.lo; j < gr.hi; j++)
				if (p.pcols[ZIPW_P_IN_N * np + j] > gr.max_in)
					gr.max_in = p.pcols[ZIPW_P_IN_N * np + j];
}

} /* namespace lda */

#endif /* LDA_WRITE_PIECES_PLAN_H */
