/*
 * host_zip_args.h - what the ZIP reader's entry points share (host_zip.hip,
 * host_zip_large.hip): the refusals made before any device work, and the grid
 * of the copy kernel.
 */
#ifndef LDA_HOST_ZIP_ARGS_H
#define LDA_HOST_ZIP_ARGS_H

#include <algorithm>

#include "host_finder.h"
#include "host_objects.h"

namespace lda {

static inline bool zip_align_ok(const char *what, size_t out_align)
{
	if (!out_align || out_align > 256 || (out_align & (out_align - 1))) {
		set_error("%s: out_align %zu is not a power of two in 1 .. 256", what, out_align);
		return false;
	}
	return true;
}

/* what a selection's call refuses before it looks at the rows */
static inline bool
zip_read_args_ok(const char *what, const struct libdeflate_decompressor *d, const void *d_in,
		 size_t in_nbytes, const uint64_t *index, size_t entries, size_t n_sel,
		 const uint64_t *sel, const void *d_out, size_t out_avail, size_t out_align,
		 const int32_t *d_results)
{
	if (!d || (!d_in && in_nbytes) || (!index && entries) || (!d_out && out_avail) ||
	    (n_sel && (!sel || !d_results))) {
		set_error("%s: NULL argument", what);
		return false;
	}
	if (entries > LDA_FINDER_MAX_RECORDS || n_sel > LDA_FINDER_MAX_RECORDS) {
		set_error("%s: entries %zu, n_sel %zu (at most 2^28)", what, entries, n_sel);
		return false;
	}
	if (in_nbytes > LDA_FINDER_MAX_FILE) {
		set_error("%s: in_nbytes %zu above 2^36", what, in_nbytes);
		return false;
	}
	return zip_align_ok(what, out_align);
}

/* lda_zip_copy_kernel's workgroups stride over the chunks */
static inline unsigned zip_copy_grid(const DeviceCtx *ctx, size_t n_chunks)
{
	return (unsigned)std::max((size_t)1, std::min(n_chunks, (size_t)ctx->num_cus * 8));
}

} /* namespace lda */

#endif /* LDA_HOST_ZIP_ARGS_H */
