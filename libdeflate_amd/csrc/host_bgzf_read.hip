/*
 * host_bgzf_read.hip - C-ABI of reading BGZF files (include/libdeflate_amd.h).
 *
 * A file in device memory: the shared finder (host_finder.h) with the scan
 * kernel of bgzf_read_kernels.hip finds its members, a prefix sum of their ISIZEs gives every member its place in one
 * contiguous output, and ONE decompress batch of max_members chunks (format
 * GZIP, exact fill) decodes there directly; the chunks behind the file's last
 * member are empty, and so are all of them when the file is refused before
 * the decode.  Nothing waits for the device and nothing comes from the host
 * but the launch sizes, which is what max_members is for.
 *
 * Ranged reads take the index and the ranges from the host: the descriptors
 * of the members the ranges touch are built here and go up in one copy.
 * The host form walks the headers itself and runs the host-pointer batch.
 */
#include <string.h>
#include <algorithm>
#include <vector>

#include "host_read_plan.h"

using namespace lda;

#define BR_SLOT ((size_t)LIBDEFLATE_AMD_BGZF_MEMBER_MAX)
#define BR_MIN_MEMBER 28

struct FileScratch {
	Finder f;
	uint64_t *isize, *bsum_b, *in_off, *in_n, *out_off, *out_av, *ain;
	int32_t *results;
	size_t bytes;
};

static FileScratch file_scratch(void *base, size_t n, size_t M)
{
	FileScratch s;
	Carve c(base);
	/* two members start 16 bytes apart at least (bgzf_read_kernels.hip) */
	s.f.carve(c, n, std::min(4 * M + 1024, n / 16 + 1));
	s.isize = c.take<uint64_t>(M);
	s.bsum_b = c.take<uint64_t>(scan_blocks(M) + 1);
	s.in_off = c.take<uint64_t>(M);
	s.in_n = c.take<uint64_t>(M);
	s.out_off = c.take<uint64_t>(M);
	s.out_av = c.take<uint64_t>(M);
	s.ain = c.take<uint64_t>(M);
	s.f.carve_chain(c);
	s.results = c.take<int32_t>(M);
	s.bytes = c.at;
	return s;
}

/* a file of no bytes may have room for no member */
#define BR_MAX_MEMBERS_MSG "%s: max_members %zu (1 .. 2^28 for a file of %zu bytes)"

static int read_enqueue(struct libdeflate_decompressor *d, const uint8_t *d_in, size_t n,
			size_t M, uint8_t *d_out, uint64_t out_avail, uint64_t *d_result,
			uint64_t *d_index, bool decode, hipStream_t st)
{
	if (!device_ctx())
		return LIBDEFLATE_AMD_NO_DEVICE;
	if (n == 0) {	/* 0 members, SUCCESS */
		hipLaunchKernelGGL(lda_bgzf_rfinal_kernel, dim3(1), dim3(256), 0, st, d_in,
				   (uint64_t)0, (uint64_t)0, out_avail, (const uint32_t *)NULL,
				   (const uint64_t *)NULL, (const uint64_t *)NULL,
				   (const uint64_t *)NULL, (const int32_t *)NULL,
				   (const uint64_t *)NULL, d_result, d_index);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_AMD_OK;
	}
	void *ws = d->bgzf.reserve(file_scratch(NULL, n, M).bytes);
	if (!ws)
		return LIBDEFLATE_AMD_OOM;
	const FileScratch s = file_scratch(ws, n, M);
	const Finder &f = s.f;
	const bool serial = env_cfg().bgzf_serial;
	const uint64_t *k_at = NULL;
	const unsigned per256 = (unsigned)((M + 255) / 256);

	if (serial) {
		LDA_HIP_TRY(hipMemsetAsync(f.state, 0, LDA_BR_STATE_WORDS * 4, st),
			    LIBDEFLATE_AMD_NO_DEVICE);
	} else {
		LDA_OK_TRY(finder_list(f, st, [&](const uint64_t *offs, const uint64_t *bsum) {
			hipLaunchKernelGGL(lda_bgzf_scan_kernel, dim3((unsigned)f.nwg), dim3(256), 0, st,
					   d_in, (uint64_t)n, f.counts, offs, bsum, (uint64_t)f.cap,
					   f.cand_pos, f.cand_size);
		}));
		k_at = f.k_at();
		/* when the candidates overflowed their room the chain does nothing
		 * and the walk below runs */
		finder_chain(f, st, n, M, s.in_off, s.in_n);
		LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	}
	hipLaunchKernelGGL(lda_bgzf_walk_kernel, dim3(1), dim3(64), 0, st, d_in, (uint64_t)n,
			   (uint64_t)M, k_at, (uint64_t)f.cap, (int)serial, s.in_off, s.in_n, f.state);
	/* ISIZEs -> places in the output -> descriptors and index */
	hipLaunchKernelGGL(lda_bgzf_isize_kernel, dim3(per256), dim3(256), 0, st, d_in, (uint64_t)n,
			   (uint64_t)M, (const uint64_t *)s.in_off, (const uint64_t *)s.in_n, f.state,
			   s.isize);
	const uint64_t *total_at = s.bsum_b + scan_enqueue(st, M, s.isize, s.out_off, s.bsum_b);
	hipLaunchKernelGGL(lda_bgzf_rdesc_kernel, dim3(per256), dim3(256), 0, st, (uint64_t)M,
			   out_avail, (const uint32_t *)f.state, (const uint64_t *)s.isize,
			   (const uint64_t *)s.bsum_b, s.in_off, s.in_n, s.out_off, s.out_av, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	if (decode) {
		/* exact fill: a member whose ISIZE lies is SHORT_OUTPUT /
		 * INSUFFICIENT_SPACE, and no byte lands outside its place */
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_GZIP, M, d_in, s.in_off,
							 s.in_n, d_out, s.out_off, s.out_av, s.results,
							 s.ain, NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	hipLaunchKernelGGL(lda_bgzf_rfinal_kernel, dim3(1), dim3(256), 0, st, d_in, (uint64_t)n,
			   (uint64_t)M, out_avail, (const uint32_t *)f.state, total_at,
			   (const uint64_t *)s.in_off, (const uint64_t *)s.in_n,
			   (const int32_t *)(decode ? s.results : NULL),
			   (const uint64_t *)s.ain, d_result, d_index);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_bgzf_decompress_batch(struct libdeflate_decompressor *d, const void *d_in,
				     size_t in_nbytes, size_t max_members, void *d_out,
				     size_t out_avail, uint64_t *d_result, uint64_t *d_index,
				     void *stream)
{
	const char *what = "bgzf_decompress_batch";
	if (!finder_args_ok(what, d, d_in, in_nbytes, BR_MAX_MEMBERS_MSG, max_members, !!in_nbytes,
			    d_result))
		return LIBDEFLATE_AMD_BAD_ARG;
	if (!d_out && in_nbytes) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return read_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_members, (uint8_t *)d_out,
			    out_avail, d_result, d_index, true, (hipStream_t)stream);
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_bgzf_index_batch(struct libdeflate_decompressor *d, const void *d_in,
				size_t in_nbytes, size_t max_members, uint64_t *d_result,
				uint64_t *d_index, void *stream)
{
	if (!finder_args_ok("bgzf_index_batch", d, d_in, in_nbytes, BR_MAX_MEMBERS_MSG, max_members, !!in_nbytes,
			    d_result))
		return LIBDEFLATE_AMD_BAD_ARG;
	DeviceGuard on(d->device);
	if (!on.ok())
		return LIBDEFLATE_AMD_NO_DEVICE;
	return read_enqueue(d, (const uint8_t *)d_in, in_nbytes, max_members, NULL, ~(uint64_t)0,
			    d_result, d_index, false, (hipStream_t)stream);
}

/* ---- ranged reads ---- */

/* the index as the reader needs it: members + 1 pairs, member sizes of 28 ..
 * 65536 bytes inside the file, at most 65536 bytes of output each */
static bool index_ok(const char *what, const uint64_t *index, size_t members, size_t in_nbytes)
{
	if (index[0] != 0 || index[1] != 0 || index[2 * members] > in_nbytes) {
		set_error("%s: the index does not start at (0, 0) or ends past in_nbytes", what);
		return false;
	}
	for (size_t j = 0; j < members; j++) {
		const uint64_t c0 = index[2 * j], c1 = index[2 * j + 2];
		const uint64_t u0 = index[2 * j + 1], u1 = index[2 * j + 3];
		if (c1 < c0 || c1 - c0 < BR_MIN_MEMBER || c1 - c0 > BR_SLOT || u1 < u0 ||
		    u1 - u0 > BR_SLOT) {
			set_error("%s: index pair %zu is no BGZF member", what, j);
			return false;
		}
	}
	return true;
}

/* a virtual offset -> uncompressed offset; false: its coffset is no member
 * start (the closing pair counts, with uoffset 0), or its uoffset lies past
 * the member's data */
static bool voffset_to_u(const uint64_t *index, size_t members, uint64_t v, uint64_t *u)
{
	const uint64_t co = v >> 16, uo = v & 0xFFFF;
	size_t lo = 0, hi = members + 1;
	while (lo < hi) {
		const size_t mid = lo + (hi - lo) / 2;
		if (index[2 * mid] < co)
			lo = mid + 1;
		else
			hi = mid;
	}
	if (lo > members || index[2 * lo] != co)
		return false;
	const uint64_t isize = lo < members ? index[2 * lo + 3] - index[2 * lo + 1] : 0;
	if (uo > isize)
		return false;
	*u = index[2 * lo + 1] + uo;
	return true;
}

/* the ranges as uncompressed offsets [rb, re), checked against the data and
 * out_avail: host arithmetic on host arrays, before any device work */
static bool ranges_ok(const char *what, const uint64_t *index, size_t members, size_t n_ranges,
		      const uint64_t *ranges, unsigned flags, size_t out_avail,
		      std::vector<uint64_t> &rb, std::vector<uint64_t> &re)
{
	const uint64_t total = index[2 * members + 1];
	uint64_t need = 0;
	rb.resize(n_ranges);
	re.resize(n_ranges);
	for (size_t r = 0; r < n_ranges; r++) {
		if (flags & LIBDEFLATE_AMD_BGZF_VOFFSETS) {
			if (!voffset_to_u(index, members, ranges[2 * r], &rb[r]) ||
			    !voffset_to_u(index, members, ranges[2 * r + 1], &re[r])) {
				set_error("%s: range %zu: a virtual offset names no member start", what, r);
				return false;
			}
		} else {
			rb[r] = ranges[2 * r];
			re[r] = rb[r] + ranges[2 * r + 1];
			if (re[r] < rb[r])
				re[r] = ~(uint64_t)0;
		}
		if (rb[r] > re[r] || re[r] > total) {
			set_error("%s: range %zu lies past the end of the data (%llu bytes)", what, r,
				  (unsigned long long)total);
			return false;
		}
		need += re[r] - rb[r];
		if (need > out_avail) {
			set_error("%s: the ranges need more than out_avail %zu bytes", what, out_avail);
			return false;
		}
	}
	return true;
}

static int read_ranges(struct libdeflate_decompressor *d, const uint8_t *d_in,
		       const uint64_t *index, size_t members, size_t n_ranges,
		       const std::vector<uint64_t> &rb, const std::vector<uint64_t> &re,
		       uint8_t *d_out, int32_t *d_results, hipStream_t st)
{
	/* the chunks: every non-empty member a range touches, range by range.
	 * in_off in_n out_off out_av per chunk, first[] per range, src dst len
	 * per trim; an edge member's out_off is filled in below */
	std::vector<uint64_t> ch, first(n_ranges + 1), trims;
	std::vector<size_t> edge_chunk;
	uint64_t outpos = 0;
	for (size_t r = 0; r < n_ranges; r++) {
		first[r] = ch.size() / 4;
		const uint64_t b = rb[r], e = re[r];
		/* the first member that ends behind b */
		size_t lo = 0, hi = members;
		while (lo < hi) {
			const size_t mid = lo + (hi - lo) / 2;
			if (index[2 * mid + 3] <= b)
				lo = mid + 1;
			else
				hi = mid;
		}
		for (size_t j = lo; j < members && index[2 * j + 1] < e; j++) {
			const uint64_t u0 = index[2 * j + 1], u1 = index[2 * j + 3];
			if (u1 == u0)
				continue;
			ch.push_back(index[2 * j]);
			ch.push_back(index[2 * j + 2] - index[2 * j]);
			if (u0 >= b && u1 <= e) {	/* straight into its place */
				ch.push_back(outpos + (u0 - b));
			} else {	/* through a slot: the wanted part is copied out */
				const uint64_t from = std::max(b, u0), to = std::min(e, u1);
				trims.push_back(edge_chunk.size() * BR_SLOT + (from - u0));
				trims.push_back(outpos + (from - b));
				trims.push_back(to - from);
				edge_chunk.push_back(ch.size());
				ch.push_back(0);
			}
			ch.push_back(u1 - u0);
		}
		outpos += e - b;
	}
	const size_t N = ch.size() / 4, T = edge_chunk.size();
	first[n_ranges] = N;

	/* device: [descriptors, transposed][first][trims][ain][results][range
	 * results are the caller's][slots] */
	uint64_t *g_desc = NULL, *g_first = NULL, *g_trims = NULL, *g_ain = NULL;
	int32_t *g_res = NULL;
	uint8_t *g_slots = NULL;
	ReadStage s;
	LDA_OK_TRY(read_stage(d, [&](Carve &cv) {
		g_desc = cv.take<uint64_t>(4 * N);
		g_first = cv.take<uint64_t>(n_ranges + 1, 8);
		g_trims = cv.take<uint64_t>(3 * T, 8);
		const ReadUp up = { g_desc, cv.at };
		g_ain = cv.take<uint64_t>(N);
		g_res = cv.take<int32_t>(N);
		g_slots = cv.take<uint8_t>(T * BR_SLOT + 16, 256);
		return up;
	}, s, 0));	/* (the slots end in the slack) */
	uint64_t *h = (uint64_t *)s.h;
	/* an edge member's slot as an offset from d_out: the batch has one output
	 * base, and base + offset is computed modulo 2^64 on both sides */
	for (size_t t = 0; t < T; t++)
		ch[edge_chunk[t]] = (uint64_t)(uintptr_t)(g_slots + t * BR_SLOT) -
				    (uint64_t)(uintptr_t)d_out;
	for (size_t i = 0; i < N; i++)
		for (size_t a = 0; a < 4; a++)
			h[a * N + i] = ch[4 * i + a];
	memcpy(h + 4 * N, first.data(), (n_ranges + 1) * 8);
	if (T)
		memcpy(h + 4 * N + n_ranges + 1, trims.data(), 3 * T * 8);
	LDA_OK_TRY(read_send(d, s, st));
	if (N) {
		int rc = libdeflate_amd_decompress_batch(d, LIBDEFLATE_AMD_GZIP, N, d_in, g_desc, g_desc + N,
						     d_out, g_desc + 2 * N, g_desc + 3 * N, g_res, g_ain,
						     NULL, st);
		if (rc != LIBDEFLATE_AMD_OK)
			return rc;
	}
	if (T) {
		hipLaunchKernelGGL(lda_bgzf_trim_kernel, dim3(tile_grid(device_ctx(), T)), dim3(256), 0, st,
				   (uint64_t)T, (const uint64_t *)g_trims, (const uint8_t *)g_slots,
				   d_out);
	}
	hipLaunchKernelGGL(lda_bgzf_range_kernel, dim3((unsigned)((n_ranges + 255) / 256)),
			   dim3(256), 0, st, (uint64_t)n_ranges, (const uint64_t *)g_first,
			   (const uint64_t *)(g_desc + N), (const int32_t *)g_res,
			   (const uint64_t *)g_ain, d_results);
	LDA_HIP_TRY(hipGetLastError(), LIBDEFLATE_AMD_NO_DEVICE);
	return LIBDEFLATE_AMD_OK;
}

extern "C" LIBDEFLATEAPI int
libdeflate_amd_bgzf_read_batch(struct libdeflate_decompressor *d, const void *d_in,
			       size_t in_nbytes, const uint64_t *index, size_t members,
			       size_t n_ranges, const uint64_t *ranges, unsigned flags, void *d_out,
			       size_t out_avail, int32_t *d_results, void *stream)
{
	const char *what = "bgzf_read_batch";
	if (!d || (!d_in && in_nbytes) || !index || (n_ranges && (!ranges || !d_results || !d_out))) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (flags & ~(unsigned)LIBDEFLATE_AMD_BGZF_VOFFSETS) {
		set_error("%s: unknown flags 0x%x", what, flags);
		return LIBDEFLATE_AMD_BAD_ARG;
	}
	if (members > LDA_FINDER_MAX_RECORDS || !index_ok(what, index, members, in_nbytes))
		return LIBDEFLATE_AMD_BAD_ARG;
	return no_unwind(what, (int)LIBDEFLATE_AMD_OOM, [&]() -> int {
		std::vector<uint64_t> rb, re;
		if (!ranges_ok(what, index, members, n_ranges, ranges, flags, out_avail, rb, re))
			return LIBDEFLATE_AMD_BAD_ARG;
		if (n_ranges == 0)
			return LIBDEFLATE_AMD_OK;
		DeviceGuard on(d->device);
		if (!on.ok() || !device_ctx())
			return LIBDEFLATE_AMD_NO_DEVICE;
		return read_ranges(d, (const uint8_t *)d_in, index, members, n_ranges, rb, re,
				   (uint8_t *)d_out, d_results, (hipStream_t)stream);
	});
}

/* ---- host memory ---- */

static enum libdeflate_result
bgzf_decompress_body(struct libdeflate_decompressor *d, const uint8_t *in, size_t n,
		     uint8_t *out, size_t out_avail, size_t *actual_out_ret, size_t *members_ret,
		     uint64_t *index, size_t index_avail, unsigned *flags_ret)
{
	/* the strict walk: htslib's header rule, the chain from 0 exactly to n */
	std::vector<size_t> off, len, osz;
	size_t pos = 0, total = 0;
	while (pos < n) {
		const uint8_t *p = in + pos;
		const size_t left = n - pos;
		if (left < BR_MIN_MEMBER || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4 ||
		    p[10] != 6 || p[11] != 0 || p[12] != 'B' || p[13] != 'C' || p[14] != 2 || p[15] != 0)
			return LIBDEFLATE_BAD_DATA;
		const size_t size = (size_t)(p[16] | p[17] << 8) + 1;
		if (size < BR_MIN_MEMBER || size > left)
			return LIBDEFLATE_BAD_DATA;
		const size_t isize = p[size - 4] | (size_t)p[size - 3] << 8 |
				     (size_t)p[size - 2] << 16 | (size_t)p[size - 1] << 24;
		if (isize > BR_SLOT)
			return LIBDEFLATE_BAD_DATA;
		off.push_back(pos);
		len.push_back(size);
		osz.push_back(isize);
		total += isize;
		pos += size;
	}
	const size_t m = off.size();
	if (members_ret)
		*members_ret = m;
	if (index && index_avail < 2 * (m + 1)) {
		set_error("libdeflate_amd_bgzf_decompress: index_avail %zu < 2 (members + 1) = %zu",
			  index_avail, 2 * (m + 1));
		return (enum libdeflate_result)LIBDEFLATE_AMD_BGZF_MORE_MEMBERS;
	}
	if (total > out_avail)
		return LIBDEFLATE_INSUFFICIENT_SPACE;
	if (m) {
		std::vector<const void *> ins(m);
		std::vector<void *> outs(m);
		std::vector<int32_t> res(m);
		std::vector<size_t> ain(m);
		size_t o = 0;
		for (size_t i = 0; i < m; i++) {
			ins[i] = in + off[i];
			outs[i] = out + o;
			o += osz[i];
		}
		int rc = libdeflate_amd_decompress_batch_host(d, LIBDEFLATE_AMD_GZIP, m, ins.data(),
							      len.data(), outs.data(), osz.data(),
							      res.data(), ain.data(), NULL);
		if (rc != LIBDEFLATE_AMD_OK) {
			complain("libdeflate_amd_bgzf_decompress", rc);
			return LIBDEFLATE_BAD_DATA;	/* a library-side failure, as everywhere */
		}
		for (size_t i = 0; i < m; i++) {
			if (res[i] != LIBDEFLATE_SUCCESS)
				return (enum libdeflate_result)res[i];
			if (ain[i] != len[i])	/* the member is shorter than it says */
				return LIBDEFLATE_BAD_DATA;
		}
	}
	if (index) {
		size_t u = 0;
		for (size_t i = 0; i < m; i++) {
			index[2 * i] = off[i];
			index[2 * i + 1] = u;
			u += osz[i];
		}
		index[2 * m] = n;
		index[2 * m + 1] = total;
	}
	if (actual_out_ret)
		*actual_out_ret = total;
	if (flags_ret) {
		static const uint8_t eof[28] = {
			0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
			0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
		};
		*flags_ret = m && len[m - 1] == 28 && !memcmp(in + off[m - 1], eof, 28) ?
				     LIBDEFLATE_AMD_BGZF_HAS_EOF : 0;
	}
	return LIBDEFLATE_SUCCESS;
}

extern "C" LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_bgzf_decompress(struct libdeflate_decompressor *d, const void *in,
			       size_t in_nbytes, void *out, size_t out_avail,
			       size_t *actual_out_ret, size_t *members_ret, uint64_t *index,
			       size_t index_avail, unsigned *flags_ret)
{
	const char *what = "libdeflate_amd_bgzf_decompress";
	if (!d || (!in && in_nbytes) || (!out && out_avail)) {
		set_error("%s: NULL argument", what);
		return LIBDEFLATE_BAD_DATA;
	}
	if (index && index_avail < 2) {
		set_error("%s: index_avail %zu < 2", what, index_avail);
		return LIBDEFLATE_BAD_DATA;
	}
	return no_unwind(what, LIBDEFLATE_BAD_DATA, [&]() {
		return bgzf_decompress_body(d, (const uint8_t *)in, in_nbytes, (uint8_t *)out,
					    out_avail, actual_out_ret, members_ret, index,
					    index_avail, flags_ret);
	});
}
