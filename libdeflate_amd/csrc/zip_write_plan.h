/*
 * zip_write_plan.h - the host arithmetic of libdeflate_amd_zip_compress_batch
 * (host_zip_write.hip): the argument checks, the ZIP64 decision and the exact
 * bound, and the plan over many entries - every entry cut into the pieces the
 * compress and CRC-32 batches run on, the pieces' slots, the per-entry columns
 * the assembly kernels (zip_write_kernels.hip) read.  Free of HIP:
 * tools/test_zip_write_plan.cpp runs it on the CPU.
 *
 * An entry for which lda_large_segmented() holds is cut exactly as
 * libdeflate_amd_compress_large_batch cuts its one buffer (large_plan.h: S by
 * size, every segment primed with the tiles in front of it); any other entry
 * is one piece; an empty entry has none.  Where nothing is compressed (level
 * 0, LIBDEFLATE_AMD_ZIP_STORE) the pieces only carry the CRC-32 and the copy,
 * and every entry of LDA_LARGE_MIN bytes or more is cut.
 *
 * The pieces are ordered by the LAUNCH GROUP of their entry, entries in the
 * caller's order inside a group: entries the small-buffer kernel takes, other
 * whole entries, and one group per segment size S.  Every group is compressed
 * by launches of its own, so each piece meets the kernel, the seg_info and the
 * size bound that a single-buffer call on its entry would give it.
 */
#ifndef LDA_ZIP_WRITE_PLAN_H
#define LDA_ZIP_WRITE_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "large_plan.h"

namespace lda {

enum {
	ZIPW_STORE = 1,		/* LIBDEFLATE_AMD_ZIP_STORE */
	ZIPW_FORCE_ZIP64 = 2,	/* LIBDEFLATE_AMD_ZIP_FORCE_ZIP64 */
	ZIPW_RESULT_WORDS = 4,	/* LIBDEFLATE_AMD_ZIPW_RESULT_WORDS */
	ZIPW_LOCAL_BYTES = 30,
	ZIPW_CEN_BYTES = 46,
	ZIPW_CEN64_EXTRA = 12,	/* 01 00 08 00 + the u64 local-header offset */
	ZIPW_END_BYTES = 22,
	ZIPW_END64_BYTES = 76,	/* the ZIP64 end record (56) and its locator (20) */
	/* the per-entry columns, n words each, in the order they go up */
	ZIPW_E_FIRST = 0,	/* first piece */
	ZIPW_E_COUNT,		/* pieces */
	ZIPW_E_NAME_OFF,	/* the name in the names' bytes */
	ZIPW_E_NAME_LEN,	/* its length; bit 32: a byte >= 0x80 (flag bit 11) */
	ZIPW_E_CEN,		/* the central record's offset from cd_off */
	ZIPW_E_USIZE,
	ZIPW_E_UOFF,		/* exclusive prefix sum of the usizes: the index row's out_off */
	ZIPW_ECOLS,
	/* the per-piece columns, np words each */
	ZIPW_P_IN_OFF = 0,	/* what the compress kernel reads: the prime in front */
	ZIPW_P_IN_N,
	ZIPW_P_SLOT_OFF,	/* its slot, from the start of the slots */
	ZIPW_P_SLOT_AV,
	ZIPW_P_PC_OFF,		/* the piece itself, in d_in: what the CRC-32 covers */
	ZIPW_P_PC_N,
	ZIPW_PCOLS
};
#define ZIPW_MAX_ENTRIES ((uint64_t)1 << 28)
#define ZIPW_NAME_UTF8 ((uint64_t)1 << 32)

/* Sum(30 + name + usize) + Sum(46 + name + 12 z64) + 22 + 76 z64, z64 decided
 * here: the flag, 65 535 entries or more, or the plain sum at or above
 * 0xFFFFFFFF.  cd_size / end_bytes: the directory and what follows it. */
static inline uint64_t
zipw_bound(uint64_t n, const uint64_t *name_offsets, const uint64_t *in_nbytes, unsigned flags,
	   bool *zip64_ret, uint64_t *cd_size_ret, uint64_t *end_bytes_ret)
{
	uint64_t locals = 0, cd = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t nl = name_offsets[k + 1] - name_offsets[k];
		locals += ZIPW_LOCAL_BYTES + nl + in_nbytes[k];
		cd += ZIPW_CEN_BYTES + nl;
	}
	const bool z = (flags & ZIPW_FORCE_ZIP64) || n >= 65535 ||
		       locals + cd + ZIPW_END_BYTES >= 0xFFFFFFFFull;
	if (z)
		cd += ZIPW_CEN64_EXTRA * n;
	const uint64_t end = ZIPW_END_BYTES + (z ? ZIPW_END64_BYTES : 0);
	if (zip64_ret)
		*zip64_ret = z;
	if (cd_size_ret)
		*cd_size_ret = cd;
	if (end_bytes_ret)
		*end_bytes_ret = end;
	return locals + cd + end;
}

/* true, or false with the reason in err: what the call refuses before any
 * device work, pointers apart (the arrays are there when n != 0) */
static inline bool
zipw_check(uint64_t n, const uint64_t *name_offsets, const uint64_t *in_offsets,
	   const uint64_t *in_nbytes, uint64_t in_avail, uint64_t out_avail, unsigned flags,
	   std::string &err)
{
	char msg[200];

	if (flags & ~(unsigned)(ZIPW_STORE | ZIPW_FORCE_ZIP64)) {
		snprintf(msg, sizeof(msg), "unknown flags 0x%x", flags);
		err = msg;
		return false;
	}
	if (n > ZIPW_MAX_ENTRIES) {
		snprintf(msg, sizeof(msg), "n_entries %llu above 2^28", (unsigned long long)n);
		err = msg;
		return false;
	}
	for (uint64_t k = 0; k < n; k++) {
		const char *why = NULL;
		if (name_offsets[k + 1] < name_offsets[k])
			why = "name_offsets decrease";
		else if (name_offsets[k + 1] == name_offsets[k])
			why = "an empty name";
		else if (name_offsets[k + 1] - name_offsets[k] > 65535)
			why = "a name of more than 65535 bytes";
		else if (in_nbytes[k] > 0xFFFFFFFFull)
			why = "an entry of 4 GiB or more";
		else if (in_offsets[k] > in_avail || in_avail - in_offsets[k] < in_nbytes[k])
			why = "its bytes do not lie inside in_avail";
		if (why) {
			snprintf(msg, sizeof(msg), "entry %llu: %s", (unsigned long long)k, why);
			err = msg;
			return false;
		}
	}
	uint64_t cd = 0, end = 0;
	zipw_bound(n, name_offsets, in_nbytes, flags, NULL, &cd, &end);
	if (out_avail < cd + end) {
		snprintf(msg, sizeof(msg), "out_avail %llu cannot hold the directory and end "
			 "records alone (%llu bytes)", (unsigned long long)out_avail,
			 (unsigned long long)(cd + end));
		err = msg;
		return false;
	}
	return true;
}

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

/* the pieces of many entries: what zipw_cut_pieces() leaves, for this plan and
 * for the gzip-members writer's (gzip_members_write_plan.h) */
struct zipw_pieces {
	uint64_t np, slots_bytes;
	std::vector<uint64_t> pcols;	/* ZIPW_PCOLS x np */
	std::vector<uint32_t> seg_info;	/* np */
	std::vector<zipw_group> groups;	/* empty where nothing is compressed */
};

struct zipw_plan : zipw_pieces {
	bool zip64;
	uint64_t n, cd_size, end_bytes, bound;
	std::vector<uint64_t> ecols;	/* ZIPW_ECOLS x n */
};

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

/* the arguments have passed zipw_check() */
static inline void
zipw_plan_build(const zipw_params &pr, uint64_t n, const uint8_t *names,
		const uint64_t *name_offsets, const uint64_t *in_offsets,
		const uint64_t *in_nbytes, unsigned flags, zipw_plan &p)
{
	p.n = n;
	p.bound = zipw_bound(n, name_offsets, in_nbytes, flags, &p.zip64, &p.cd_size, &p.end_bytes);
	p.ecols.assign((size_t)(ZIPW_ECOLS * n), 0);
	uint64_t cen = 0, uoff = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t nl = name_offsets[k + 1] - name_offsets[k], usize = in_nbytes[k];
		uint64_t utf8 = 0;
		for (uint64_t b = name_offsets[k]; b < name_offsets[k + 1]; b++)
			if (names[b] >= 0x80)
				utf8 = ZIPW_NAME_UTF8;
		p.ecols[ZIPW_E_NAME_OFF * n + k] = name_offsets[k] - name_offsets[0];
		p.ecols[ZIPW_E_NAME_LEN * n + k] = nl | utf8;
		p.ecols[ZIPW_E_CEN * n + k] = cen;
		p.ecols[ZIPW_E_USIZE * n + k] = usize;
		p.ecols[ZIPW_E_UOFF * n + k] = uoff;
		cen += ZIPW_CEN_BYTES + nl + (p.zip64 ? ZIPW_CEN64_EXTRA : 0);
		uoff += usize;
	}
	zipw_cut_pieces(pr, n, in_offsets, in_nbytes, p.ecols.data() + ZIPW_E_FIRST * n,
			p.ecols.data() + ZIPW_E_COUNT * n, p);
}

} /* namespace lda */

#endif /* LDA_ZIP_WRITE_PLAN_H */
