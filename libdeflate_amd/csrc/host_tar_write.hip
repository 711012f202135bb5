/*
 * host_tar_write.hip - C-ABI of writing a tar archive in device memory
 * (include/libdeflate_amd.h: libdeflate_amd_tar_write_size,
 * libdeflate_amd_tar_write_batch, libdeflate_amd_targz_compress_batch).
 *
 * tar_write_plan.h checks the host arrays and the names, decides which names
 * get a pax record, places every entry and knows the archive's exact size and
 * its index rows, so nothing comes back from the device and there is no
 * verdict word.  The plan's rows and the names go up through the object's
 * pinned block in ONE copy (Upload, host_common.h), as the ZIP writer's do,
 * and ONE kernel (tar_write_kernels.hip) writes every byte of the archive.
 * The .tar.gz call writes the archive into the object's scratch and hands it
 * to the body of libdeflate_amd_compress_large_batch (host_compress.hip).
 * c->zipw: [entry rows][names] (what goes up), [the archive] (.tar.gz only).
 */
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "host_objects.h"
#include "kernels.h"
#include "tar_write_plan.h"

using namespace lda;

static_assert(TARW_ROW_WORDS == LIBDEFLATE_AMD_TAR_WORDS && TARW_ROW_WORDS == LDA_TAR_WORDS &&
	      TARW_MAX_ENTRIES == (uint64_t)1 << 28 && LDA_TARW_TILE % TARW_BLOCK == 0,
	      "tar_write_plan.h holds copies of the header's constants");
static_assert(TARW_E_OFF == LDA_TARW_E_OFF && TARW_E_PAX == LDA_TARW_E_PAX &&
	      TARW_E_NAME_OFF == LDA_TARW_E_NAME_OFF && TARW_E_NAME_LEN == LDA_TARW_E_NAME_LEN &&
	      TARW_E_SRC == LDA_TARW_E_SRC && TARW_E_SIZE == LDA_TARW_E_SIZE &&
	      TARW_ECOLS == LDA_TARW_ECOLS,
	      "kernels.h holds copies of the plan's row");
static_assert((TARW_MAX_ARCHIVE + LDA_TARW_TILE - 1) / LDA_TARW_TILE * 256 < (uint64_t)1 << 32,
	      "one launch of 256-thread workgroups, a tile each, holds the largest archive");

extern "C" LIBDEFLATEAPI size_t
libdeflate_amd_tar_write_size(size_t n_entries, const uint64_t *name_offsets, const void *names,
			      const uint64_t *in_nbytes)
{
	if (n_entries && (!name_offsets || !names || !in_nbytes)) {
		set_error("tar_write_size: NULL argument");
		return 0;
	}
	const uint64_t size = tarw_size(n_entries, name_offsets, (const uint8_t *)names, in_nbytes);
	if (!size)
		set_error("tar_write_size: n_entries above 2^28, an entry or a name that "
			  "tar_write_batch refuses, or an archive of 1 TiB or more");
	return (size_t)size;
}

struct TarwScratch {
	uint64_t *erows;
	uint8_t *names;
	size_t up_bytes;
	uint8_t *archive;
	size_t bytes;
};

static TarwScratch tarw_scratch(void *base, const tarw_plan &p, size_t names_bytes, bool archive)
{
	TarwScratch s;
	Carve c(base);

	s.erows = c.take<uint64_t>(TARW_ECOLS * (size_t)p.n);
	s.names = c.take<uint8_t>(names_bytes);
	s.up_bytes = c.at;
	s.archive = c.take<uint8_t>(archive ? (size_t)p.size : 0, 256);
	s.bytes = c.at + 16;
	return s;
}

/* the plan up and the pack kernel on st; d_out NULL: the archive goes into the
 * object's scratch, and *archive_ret says where */
static int tarw_enqueue(struct libdeflate_compressor *c, const tarw_plan &p, const uint8_t *names,
			size_t names_bytes, const uint8_t *d_in, uint8_t *d_out, uint64_t mtime,
			hipStream_t st, uint8_t **archive_ret)
{
	DeviceCtx *ctx = device_ctx();
	if (!ctx)
		return LIBDEFLATE_AMD_NO_DEVICE;
	const size_t n = (size_t)p.n;
	/* a workgroup per tile of the archive (the plan has bounded its size) */
	const uint64_t tiles = (p.size + LDA_TARW_TILE - 1) / LDA_TARW_TILE;
	const TarwScratch sz = tarw_scratch(NULL, p, names_bytes, !d_out);

	LDA_OK_TRY(c->zipw_up.begin());
	uint8_t *ws = (uint8_t *)c->zipw.reserve(sz.bytes);
	uint8_t *h = (uint8_t *)c->zipw_up.pinned(sz.up_bytes);
	if (!ws || !h)
		return LIBDEFLATE_AMD_OOM;
	const TarwScratch s = tarw_scratch(ws, p, names_bytes, !d_out);
	if (sz.up_bytes) {
		const TarwScratch hs = tarw_scratch(h, p, names_bytes, false);
		memcpy(hs.erows, p.erows.data(), p.erows.size() * 8);
		memcpy(hs.names, names, names_bytes);
		LDA_OK_TRY(c->zipw_up.send(ws, sz.up_bytes, st));
	}
	uint8_t *out = d_out ? d_out : s.archive;
	hipLaunchKernelGGL(lda_tarw_pack_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (uint64_t)n,
			   p.end, p.size, mtime, (const uint64_t *)s.erows, (const uint8_t *)s.names,
			   d_in, out);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (archive_ret)
		*archive_ret = out;
	return LIBDEFLATE_AMD_OK;
}

/* what both calls check of the entries, and the plan; out_avail: NULL, or the
 * room for the archive itself */
static bool tarw_args(const char *what, const struct libdeflate_compressor *c, size_t n_entries,
		      const void *names, const uint64_t *name_offsets, const void *d_in,
		      size_t in_avail, const uint64_t *in_offsets, const uint64_t *in_nbytes,
		      const uint64_t *out_avail, uint64_t mtime, unsigned flags, tarw_plan &p)
{
	if (!c || (!d_in && in_avail) ||
	    (n_entries && (!names || !name_offsets || !in_offsets || !in_nbytes))) {
		set_error("%s: NULL argument", what);
		return false;
	}
	std::string err;
	/* (before the count is known to be sane, no array is walked past it) */
	if (!tarw_plan_build(n_entries, (const uint8_t *)names, name_offsets, in_offsets, in_nbytes,
			     in_avail, out_avail, mtime, flags, p, err)) {
		set_error("%s: %s", what, err.c_str());
		return false;
	}
	return true;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_tar_write_batch(struct libdeflate_compressor *c, size_t n_entries,
			       const void *names, const uint64_t *name_offsets, const void *d_in,
			       size_t in_avail, const uint64_t *in_offsets, const uint64_t *in_nbytes,
			       void *d_out, size_t out_avail, uint64_t *index, uint64_t mtime,
			       unsigned flags, void *stream)
{
	const char *what = "tar_write_batch";
	if (!d_out) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		tarw_plan p;
		const uint64_t avail = out_avail;
		if (!tarw_args(what, c, n_entries, names, name_offsets, d_in, in_avail, in_offsets,
			       in_nbytes, &avail, mtime, flags, p))
			return LIBDEFLATE_AMD_BAD_ARG;
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		const uint8_t *nm = n_entries ? (const uint8_t *)names + name_offsets[0] : NULL;
		const int rc = tarw_enqueue(c, p, nm, n_entries ? (size_t)(name_offsets[n_entries] -
									  name_offsets[0]) : 0,
					    (const uint8_t *)d_in, (uint8_t *)d_out, mtime,
					    (hipStream_t)stream, NULL);
		if (rc == LIBDEFLATE_AMD_OK && index)
			tarw_rows(p, mtime, index);
		return rc;
	});
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_targz_compress_batch(struct libdeflate_compressor *c, int format, size_t n_entries,
				    const void *names, const uint64_t *name_offsets,
				    const void *d_in, size_t in_avail, const uint64_t *in_offsets,
				    const uint64_t *in_nbytes, void *d_out, size_t out_avail,
				    uint64_t *d_out_nbytes, uint64_t *index, uint64_t mtime,
				    unsigned flags, void *stream)
{
	const char *what = "targz_compress_batch";
	/* (the stream's input is an archive of at least 10 240 bytes in the
	 * object's scratch: d_out stands in for it here) */
	if (!compress_large_args_ok(what, c, format, d_out, 1, d_out, out_avail, d_out_nbytes))
		return LIBDEFLATE_AMD_BAD_ARG;
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		tarw_plan p;
		if (!tarw_args(what, c, n_entries, names, name_offsets, d_in, in_avail, in_offsets,
			       in_nbytes, NULL, mtime, flags, p))
			return LIBDEFLATE_AMD_BAD_ARG;
		DeviceGuard on(c->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		const uint8_t *nm = n_entries ? (const uint8_t *)names + name_offsets[0] : NULL;
		/* all of the call's scratch before anything is queued: growing frees
		 * memory (and waits for the device) */
		if (!compress_large_reserve(c, (size_t)p.size))
			return LIBDEFLATE_AMD_OOM;
		uint8_t *archive = NULL;
		int rc = tarw_enqueue(c, p, nm, n_entries ? (size_t)(name_offsets[n_entries] -
								    name_offsets[0]) : 0,
				      (const uint8_t *)d_in, NULL, mtime, (hipStream_t)stream, &archive);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
		/* (its scratch is c->large and c->scratch: the archive stays where it is) */
		rc = compress_large_enqueue(c, format, archive, (size_t)p.size, d_out, out_avail,
					    d_out_nbytes, stream);
		if (rc == LIBDEFLATE_AMD_OK && index)
			tarw_rows(p, mtime, index);
		return rc;
	});
}
