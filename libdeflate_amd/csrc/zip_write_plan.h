/*
 * zip_write_plan.h - the host arithmetic of libdeflate_amd_zip_compress_batch
 * (host_zip_write.hip): the argument checks, the ZIP64 decision and the exact
 * bound, and the plan over many entries - every entry cut into the pieces the
 * compress and CRC-32 batches run on and the pieces' slots
 * (write_pieces_plan.h: zipw_cut_pieces(), store where the level is 0 or the
 * call says LIBDEFLATE_AMD_ZIP_STORE), the per-entry columns the assembly
 * kernels (zip_write_kernels.hip) read.  Free of HIP:
 * tools/test_zip_write_plan.cpp runs it on the CPU.
 */
#ifndef LDA_ZIP_WRITE_PLAN_H
#define LDA_ZIP_WRITE_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "write_pieces_plan.h"

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
	ZIPW_ECOLS
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

struct zipw_plan : zipw_pieces {
	bool zip64;
	uint64_t n, cd_size, end_bytes, bound;
	std::vector<uint64_t> ecols;	/* ZIPW_ECOLS x n */
};

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
