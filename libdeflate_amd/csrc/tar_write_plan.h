/*
 * tar_write_plan.h - the host arithmetic of libdeflate_amd_tar_write_batch and
 * libdeflate_amd_targz_compress_batch (host_tar_write.hip): the argument
 * checks, the UTF-8 check of the names, which names get a pax record and how
 * long that record is, every entry's place in the archive, the archive's exact
 * size and the index rows.  Free of HIP: tools/test_tar_write_plan.cpp runs it
 * on the CPU.
 *
 * The layout (include/libdeflate_amd.h states the bytes): entry k begins at
 * the block off[k].  A name of more than 100 characters or with a byte >= 0x80
 * has a pax header block and ceil(pax / 512) blocks of pax data in front of the
 * entry's own header block; the data follows the header in ceil(size / 512)
 * blocks.  Behind the last entry stand two zero blocks, and zeros up to a
 * multiple of 10 240 bytes.  Every block of the archive is therefore a pure
 * function of the rows below, which is all the kernel
 * (tar_write_kernels.hip) reads.
 */
#ifndef LDA_TAR_WRITE_PLAN_H
#define LDA_TAR_WRITE_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace lda {

enum {
	TARW_BLOCK = 512,
	TARW_RECORD = 10240,	/* the archive's size is a multiple of this */
	TARW_NAME_FIELD = 100,	/* the header's name field, and tarfile's limit in characters */
	TARW_NAME_MAX = 65535,
	TARW_ROW_WORDS = 8,	/* LIBDEFLATE_AMD_TAR_WORDS */
	TARW_PAX_KEY = 6,	/* " path=" between the decimal and the name */
	/* the words of an entry's row: the kernel walks the entries of a tile
	 * one after the other, and a row is one read */
	TARW_E_OFF = 0,		/* the archive offset of the entry's first block */
	TARW_E_PAX,		/* the length of its pax record, 0: it has none */
	TARW_E_NAME_OFF,	/* the name in the names' bytes */
	TARW_E_NAME_LEN,
	TARW_E_SRC,		/* the entry's bytes in d_in */
	TARW_E_SIZE,
	TARW_ECOLS
};
#define TARW_MAX_ENTRIES ((uint64_t)1 << 28)
#define TARW_FIELD_LIMIT ((uint64_t)1 << 33)	/* 8^11: what 11 octal digits cannot hold */
/* the largest archive: the kernel runs a workgroup of 256 threads per tile of
 * 64 KiB, and a launch holds fewer than 2^32 threads, so fewer than 2^24 tiles */
#define TARW_MAX_ARCHIVE (((uint64_t)1 << 40) - 65536)

/* Is p[0 .. n) well-formed UTF-8 without a 0 byte (no overlong form, no
 * surrogate, nothing above U+10FFFF)?  *chars: its characters; *high: does it
 * hold a byte >= 0x80. */
static inline bool tarw_utf8(const uint8_t *p, uint64_t n, uint64_t *chars, bool *high)
{
	uint64_t i = 0, c = 0;
	bool h = false;

	while (i < n) {
		const uint8_t b = p[i];
		uint64_t more;
		uint32_t cp, least;
		if (b == 0)
			return false;
		if (b < 0x80) {
			i++;
			c++;
			continue;
		}
		h = true;
		if ((b & 0xE0) == 0xC0) {
			more = 1;
			cp = b & 0x1F;
			least = 0x80;
		} else if ((b & 0xF0) == 0xE0) {
			more = 2;
			cp = b & 0x0F;
			least = 0x800;
		} else if ((b & 0xF8) == 0xF0) {
			more = 3;
			cp = b & 0x07;
			least = 0x10000;
		} else {
			return false;
		}
		if (n - i <= more)
			return false;
		for (uint64_t j = 1; j <= more; j++) {
			if ((p[i + j] & 0xC0) != 0x80)
				return false;
			cp = cp << 6 | (p[i + j] & 0x3F);
		}
		if (cp < least || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF))
			return false;
		i += more + 1;
		c++;
	}
	*chars = c;
	*high = h;
	return true;
}

static inline uint64_t tarw_digits(uint64_t v)
{
	uint64_t d = 1;
	while (v >= 10) {
		v /= 10;
		d++;
	}
	return d;
}

/* the length of the pax record "%d path=%s\n" of a name of name_len bytes: the
 * decimal counts itself, so it is the fixed point of n = name_len + 7 +
 * digits(n), reached from below */
static inline uint64_t tarw_pax_len(uint64_t name_len)
{
	const uint64_t l = name_len + TARW_PAX_KEY + 1;	/* ' ' "path=" the name '\n' */
	uint64_t p = 0;

	for (;;) {
		const uint64_t n = l + tarw_digits(p);
		if (n == p)
			return p;
		p = n;
	}
}

/* Entry k of the host arrays, for the size query and the plan alike: NULL with
 * *pax the length of the name's pax record (0: it has none), or why no archive
 * holds the entry.  in_offsets NULL: the entry's place in d_in is not asked. */
static inline const char *
tarw_entry_check(uint64_t k, const uint8_t *names, const uint64_t *name_offsets,
		 const uint64_t *in_offsets, const uint64_t *in_nbytes, uint64_t in_avail,
		 uint64_t *pax)
{
	uint64_t chars = 0;
	bool high = false;
	const uint64_t nl = name_offsets[k + 1] - name_offsets[k];

	if (name_offsets[k + 1] < name_offsets[k])
		return "name_offsets decrease";
	if (nl == 0)
		return "an empty name";
	if (nl > TARW_NAME_MAX)
		return "a name of more than 65535 bytes";
	if (!tarw_utf8(names + name_offsets[k], nl, &chars, &high))
		return "a name that holds a 0 byte or is not valid UTF-8";
	if (in_nbytes[k] >= TARW_FIELD_LIMIT)
		return "an entry of 8 GiB or more";
	if (in_offsets && (in_offsets[k] > in_avail || in_avail - in_offsets[k] < in_nbytes[k]))
		return "its bytes do not lie inside in_avail";
	*pax = high || chars > TARW_NAME_FIELD ? tarw_pax_len(nl) : 0;
	return NULL;
}

static inline uint64_t tarw_blocks(uint64_t bytes)
{
	return (bytes + TARW_BLOCK - 1) / TARW_BLOCK;
}

/* the bytes of an entry: its pax header and data blocks, its header, its data */
static inline uint64_t tarw_entry_bytes(uint64_t pax, uint64_t size)
{
	return ((pax ? 1 + tarw_blocks(pax) : 0) + 1 + tarw_blocks(size)) * TARW_BLOCK;
}

/* the archive's size from where its last entry ends */
static inline uint64_t tarw_total(uint64_t end)
{
	return (end + 2 * TARW_BLOCK + TARW_RECORD - 1) / TARW_RECORD * TARW_RECORD;
}

/* libdeflate_amd_tar_write_size(): the arrays are there when n != 0; 0 for
 * arrays no archive can come from */
static inline uint64_t
tarw_size(uint64_t n, const uint64_t *name_offsets, const uint8_t *names, const uint64_t *in_nbytes)
{
	uint64_t at = 0;

	if (n > TARW_MAX_ENTRIES)
		return 0;
	for (uint64_t k = 0; k < n; k++) {
		uint64_t pax;
		if (tarw_entry_check(k, names, name_offsets, NULL, in_nbytes, 0, &pax))
			return 0;
		at += tarw_entry_bytes(pax, in_nbytes[k]);
	}
	return tarw_total(at) > TARW_MAX_ARCHIVE ? 0 : tarw_total(at);
}

struct tarw_plan {
	uint64_t n;
	uint64_t end, size;		/* where the last entry ends; the archive's size */
	std::vector<uint64_t> erows;	/* n rows of TARW_ECOLS words */
};

/*
 * true with the plan, or false with the reason in err: what the calls refuse
 * before any device work, pointers apart (the arrays are there when n != 0).
 * out_avail: the room for the ARCHIVE (the targz call passes the size itself).
 */
static inline bool
tarw_plan_build(uint64_t n, const uint8_t *names, const uint64_t *name_offsets,
		const uint64_t *in_offsets, const uint64_t *in_nbytes, uint64_t in_avail,
		const uint64_t *out_avail, uint64_t mtime, unsigned flags, tarw_plan &p,
		std::string &err)
{
	char msg[200];

	if (flags) {
		snprintf(msg, sizeof(msg), "unknown flags 0x%x", flags);
		err = msg;
		return false;
	}
	if (n > TARW_MAX_ENTRIES) {
		snprintf(msg, sizeof(msg), "n_entries %llu above 2^28", (unsigned long long)n);
		err = msg;
		return false;
	}
	if (mtime >= TARW_FIELD_LIMIT) {
		snprintf(msg, sizeof(msg), "mtime %llu does not fit 11 octal digits",
			 (unsigned long long)mtime);
		err = msg;
		return false;
	}
	p.n = n;
	p.erows.assign((size_t)(TARW_ECOLS * n), 0);
	uint64_t at = 0;
	for (uint64_t k = 0; k < n; k++) {
		uint64_t pax = 0;
		const char *why = tarw_entry_check(k, names, name_offsets, in_offsets, in_nbytes,
						   in_avail, &pax);
		if (why) {
			snprintf(msg, sizeof(msg), "entry %llu: %s", (unsigned long long)k, why);
			err = msg;
			return false;
		}
		p.erows[TARW_ECOLS * k + TARW_E_OFF] = at;
		p.erows[TARW_ECOLS * k + TARW_E_PAX] = pax;
		p.erows[TARW_ECOLS * k + TARW_E_NAME_OFF] = name_offsets[k] - name_offsets[0];
		p.erows[TARW_ECOLS * k + TARW_E_NAME_LEN] = name_offsets[k + 1] - name_offsets[k];
		p.erows[TARW_ECOLS * k + TARW_E_SRC] = in_offsets[k];
		p.erows[TARW_ECOLS * k + TARW_E_SIZE] = in_nbytes[k];
		at += tarw_entry_bytes(pax, in_nbytes[k]);
	}
	p.end = at;
	p.size = tarw_total(at);
	if (p.size > TARW_MAX_ARCHIVE) {
		snprintf(msg, sizeof(msg), "an archive of %llu bytes, 1 TiB or more",
			 (unsigned long long)p.size);
		err = msg;
		return false;
	}
	if (out_avail && *out_avail < p.size) {
		snprintf(msg, sizeof(msg), "out_avail %llu below the archive's %llu bytes",
			 (unsigned long long)*out_avail, (unsigned long long)p.size);
		err = msg;
		return false;
	}
	return true;
}

/*
 * The rows libdeflate_amd_tar_index_batch returns for the archive with
 * out_align 1: { header, name_off, name_len, '0' | name source << 8, data_off,
 * usize, mtime, out_off }.  A name in the header (source 0) is at the header's
 * offset and has no prefix; a pax name (source 2) is the record's value, behind
 * the decimal and " path=" in the block after the pax header.
 */
static inline void tarw_rows(const tarw_plan &p, uint64_t mtime, uint64_t *rows)
{
	const uint64_t n = p.n;
	uint64_t out_off = 0;

	for (uint64_t k = 0; k < n; k++) {
		const uint64_t off = p.erows[TARW_ECOLS * k + TARW_E_OFF], pax = p.erows[TARW_ECOLS * k + TARW_E_PAX];
		const uint64_t size = p.erows[TARW_ECOLS * k + TARW_E_SIZE];
		const uint64_t hdr = off + (pax ? 1 + tarw_blocks(pax) : 0) * TARW_BLOCK;
		uint64_t *row = rows + TARW_ROW_WORDS * k;
		row[0] = hdr;
		row[1] = pax ? off + TARW_BLOCK + tarw_digits(pax) + TARW_PAX_KEY : hdr;
		row[2] = p.erows[TARW_ECOLS * k + TARW_E_NAME_LEN];
		row[3] = '0' | (pax ? 2u : 0u) << 8;
		row[4] = hdr + TARW_BLOCK;
		row[5] = size;
		row[6] = mtime;
		row[7] = out_off;
		out_off += size;
	}
}

} /* namespace lda */

#endif /* LDA_TAR_WRITE_PLAN_H */
