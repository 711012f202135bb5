/*
 * host_stream.hip - ONE large stream on many waves: the host side of
 * inflate_stream.hip (find -> plan -> count -> chain -> decode -> window ->
 * resolve -> checksum; see that file's header for what each step is).
 *
 * Entered from the single-buffer libdeflate_{deflate,zlib,gzip}_decompress[_ex]
 * calls (host_decompress.hip) for streams of LDA_STREAM_PAR_MIN bytes and up -
 * what programs/gzip.c:187-303 and programs/benchmark.c:543-544 hand to the
 * library.  It only ever ANSWERS for a clean success (or a footer that does not
 * match a cleanly decoded stream): anything else - an invalid header, a chain
 * that does not close, an output that does not fit or does not fill - is left
 * to the sequential kernel, which follows the reference's result codes bit for
 * bit, so the codes cannot depend on which path ran.
 *
 * In here: the device plumbing (struct StreamRun, a method per phase) and the
 * verdict.  The arithmetic on bit offsets - the plan, the chain - is
 * stream_plan.h's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <unordered_map>
#include <vector>

#include "host_objects.h"
#include "kernels.h"
#include "stream_kernels.h"
#include "stored_rows.h"
#include "stream_plan.h"
#include "seek_plan.h"

namespace lda {

static thread_local uint64_t g_stats[LIBDEFLATE_AMD_STREAM_STATS];

/* gzip / zlib container: offset of the raw stream and the footer's size; false
 * if the sequential path should look at it (lib/gzip_decompress.c:45-107,
 * lib/zlib_decompress.c:45-72).  `have`: how many of the buffer's n bytes are
 * at `in` - all of them, or the head of a stream that lies in device memory:
 * a header that runs past the head is the sequential path's */
static bool container(int format, const uint8_t *in, size_t n, size_t have, size_t *hdr,
		      size_t *ftr)
{
	*hdr = *ftr = 0;
	if (format == LIBDEFLATE_AMD_DEFLATE)
		return true;
	if (have < (n < 18 ? n : 18))
		return false;
	if (format == LIBDEFLATE_AMD_ZLIB) {
		if (n < 6)
			return false;
		const uint32_t h = ((uint32_t)in[0] << 8) | in[1];
		if (h % 31 || ((h >> 8) & 0xF) != 8 || (h >> 12) > 7 || ((h >> 5) & 1))
			return false;
		*hdr = 2;
		*ftr = 4;
		return true;
	}
	if (n < 18 || in[0] != 0x1F || in[1] != 0x8B || in[2] != 8 || (in[3] & 0xE0))
		return false;
	const uint32_t flg = in[3];
	size_t p = 10;
	if (flg & 0x04) {
		const size_t xlen = in[p] | ((size_t)in[p + 1] << 8);
		p += 2;
		if (n - p < xlen + 8)
			return false;
		p += xlen;
	}
	for (int k = 0; k < 2; k++)
		if (flg & (k ? 0x10 : 0x08)) {
			if (p >= have)
				return false;
			while (in[p++] != 0 && p != n)
				if (p >= have)
					return false;
			if (n - p < 8)
				return false;
		}
	if (flg & 0x02) {
		p += 2;
		if (n - p < 8)
			return false;
	}
	if (p > have)
		return false;
	*hdr = p;
	*ftr = 8;
	return true;
}

bool launch_count(hipStream_t st, uint32_t n, const lda_stream_chunk *d_chunks,
		  lda_stream_res *d_res, const uint8_t *d_raw, uint64_t raw_n,
		  const uint8_t *d_hlens, const uint32_t *d_hinfo, uint16_t *d_hints)
{
	hipLaunchKernelGGL(lda_stream_count_kernel, dim3(n), dim3(64), lda_stream_chunk_lds(),
			   st, n, d_chunks, d_res, d_raw, raw_n, (uint32_t *)NULL, d_hlens, d_hinfo,
			   d_hints);
	LDA_TRY(hipGetLastError());
	return true;
}

uint32_t *stream_token_scratch(struct libdeflate_decompressor *d, size_t nwaves)
{
	return (uint32_t *)d->tokens.reserve(
		std::min(nwaves, STREAM_DECODE_BATCH) * lda_stream_tokcap() * 4 + 64);
}

namespace {

/*
 * One call of decompress_stream_parallel(): what outlives a phase, and a
 * method per phase.  A method returns false for "not answered here"; the
 * reason is in S[1] (WHY_DEVICE unless something better is known).
 */
struct StreamRun {
	/*
	 * THE INPUT SOURCE.  dev == false: `in` is the caller's host
	 * buffer; it is copied to d->sin window by window, the host reads what it
	 * decides itself out of `in`, and the output goes through d->sout to the
	 * host buffer `out`.  dev == true (libdeflate_amd_decompress_large):
	 * `in` and `out` are device pointers.  The kernels read the caller's
	 * buffer in place and write the caller's output, and the five things the
	 * host reads out of the stream come to it otherwise: (a) the container
	 * header and the bits at bit 0 from the first 4 KiB, fetched once; (b) the
	 * footer with the decode pass's results; (c) the bits at a carried-in
	 * boundary as 8 bytes fetched when a window begins there; (d) runs of
	 * stored blocks from the rows of lda_stream_find_stored_kernel; (e) blocks
	 * of one codeword length from lda_stream_hdr_class_kernel.
	 */
	struct libdeflate_decompressor *const d;
	const int format;
	const uint8_t *const in;
	const size_t in_nbytes;
	uint8_t *const out;
	const size_t out_avail;
	const bool exact_fill, dev;
	uint64_t *const S = g_stats;
	DeviceCtx *ctx = nullptr;
	const EnvCfg &env = env_cfg();
	/* host-side phase clock: S[8..13] = microseconds of copy in, find, count +
	 * chain, decode + window + resolve, checksum, copy out */
	std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
	/* LDA_STREAM_DEBUG: where the host's time goes inside a phase (stderr) */
	const bool debug = getenv("LDA_STREAM_DEBUG") != nullptr;
	hipStream_t s_copy = nullptr, s_comp = nullptr;
	/* The small transfers of every phase (descriptors down, results back) go
	 * through pinned memory: from and to pageable memory each of them would
	 * be staged by the runtime and cost a host-blocking round trip of its own.
	 * pin_phase() sizes the arena (nothing may be in flight), up() / back()
	 * queue a copy, pin_sync() waits and delivers what came back. */
	uint8_t *pin_base = nullptr;
	size_t pin_used = 0;
	struct pending_t { void *dst; const void *src; size_t n; };
	std::vector<pending_t> pin_pending;
	/* the container: the raw stream is in[hdr .. in_nbytes - ftr) */
	size_t hdr = 0, ftr = 0;
	uint64_t raw_n = 0, raw_bits = 0;
	/* the host has the stream too: bits of it, for what it can decide itself.
	 * Of a stream in device memory it has 8 bytes at a time: pk[] holds the
	 * raw stream's bytes from pk_at on (the head's at first, fetch_pk() for
	 * the boundary a later window begins at). */
	stored_probe_bytes host_bytes = { nullptr, 0 };
	uint8_t pk[8] = { 0 };
	uint64_t pk_at = 0;
	/* (d) the rows of the current window: every offset of it at which a stored
	 * block's LEN / NLEN could lie (stored_rows.h), sorted.  The kernel is
	 * queued once per window - ahead of everything when the window begins at
	 * a stored block, otherwise beside the block finder, whose round trip then
	 * brings the rows too.  Scratch: [count][classes of (e)][rows]. */
	std::vector<lda_stored_row> rows;
	bool rows_queued = false;
	uint32_t rows_cap = 0, rows_cnt = 0;
	static constexpr uint32_t ROWS_FIRST = 4096;	/* rows read back with the count */
	static constexpr size_t cls_at = 64, rows_at = cls_at + (size_t)LDA_STREAM_HDR_SLOTS * 8;
	uint8_t *d_probe = nullptr;
	/* device memory follows the windows, not the caller's buffer: the input
	 * copy grows with them (a regrown buffer is filled again from the start:
	 * a quarter more bytes copied at worst), the finder's queues are sized by
	 * the window searched */
	static constexpr size_t in_at = 64;
	uint8_t *sin = nullptr, *d_raw = nullptr;
	uint64_t *d_queue = nullptr, *d_cand = nullptr;
	uint32_t *d_cnt = nullptr;	/* [0] queue, [1] candidates, [2] error flag */
	uint32_t qcap = 0, ccap = 0;
	/* The headers the finder accepts are parsed ONCE each, by a wave of their
	 * own, beside the host's planning (lda_stream_hdr_cache_kernel on the copy
	 * stream, which has nothing to do then): slot i holds the code lengths of
	 * candidate i of the current window, and every chunk at or inside that
	 * block takes them from there instead of parsing the header again (one
	 * lane's loop: 40 us of every chunk of the count pass and of the decode
	 * pass).  hdr_bit -> slot + 1: */
	uint8_t *d_hlens = nullptr;
	uint32_t *d_hinfo = nullptr;
	uint16_t *d_hints = nullptr;	/* the last window's rows of lane starts (chunk.hint) */
	std::unordered_map<uint64_t, uint32_t> hdr_slot;
	/* (e) of a stream in device memory the host has no header to read:
	 * lda_stream_hdr_class_kernel applies one_length_code()'s final rule to
	 * the lengths in the slots, and hcls[slot] = { longest literal codeword or
	 * 0, bits from the header to the first token } comes back before the
	 * plan.  A header without a slot counts as an ordinary block. */
	struct hdr_class { uint32_t hi, used; };
	std::vector<hdr_class> hcls;

	std::vector<lda_stream_chunk> acc;	/* accepted chunks, exact starts */
	std::vector<lda_stream_res> accr;
	/* where the next window's first chunk starts */
	lda_stream_chunk carry = header_chunk(0);
	/* the state carried in lies inside a static block (carry.hdr_bit ==
	 * LDA_HDR_STATIC): is that block the stream's last?  (the chunks planned
	 * under the static codes cannot know, see stream_types.h) */
	bool carry_gf = false;
	size_t copied = 0;	/* bytes of the caller's buffer on the device */
	uint64_t dev_n = 0;	/* raw bytes the kernels may read (the last window's) */
	bool final_seen = false;
	/* the current window: does it hold the stream's end, the raw bytes the
	 * kernels may read, the bit its chunks end in front of; what find(),
	 * plan() and count() hand on */
	bool whole = false, cache_queued = false;
	uint64_t win_n = 0, R1 = 0;
	std::vector<uint64_t> cands;
	std::vector<planned> plan_;
	uint32_t nexact = 0;
	std::vector<lda_stream_chunk> hc;
	std::vector<lda_stream_res> hr;
	/* the verdict */
	uint64_t total = 0;
	size_t consumed = 0;
	uint32_t sum = 0;
	uint8_t fbytes[8] = { 0 };	/* (b) the footer of a stream in device memory */

	StreamRun(struct libdeflate_decompressor *d_, int format_, const uint8_t *in_, size_t in_nbytes_,
		  uint8_t *out_, size_t out_avail_, bool exact_fill_, bool on_device)
		: d(d_), format(format_), in(in_), in_nbytes(in_nbytes_), out(out_), out_avail(out_avail_),
		  exact_fill(exact_fill_), dev(on_device)
	{
		memset(g_stats, 0, sizeof(g_stats));
	}

	void lap(int slot)
	{
		const auto now = std::chrono::steady_clock::now();
		S[slot] += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(now - t_last).count();
		t_last = now;
	}
	void dbg(const char *what) const
	{
		if (debug)
			fprintf(stderr, "  %-28s +%lld us\n", what,
				(long long)std::chrono::duration_cast<std::chrono::microseconds>(
					std::chrono::steady_clock::now() - t_last).count());
	}

	bool pin_phase(size_t need)
	{
		pin_base = (uint8_t *)d->meta.ensure(need + 1024);
		pin_used = 0;
		return pin_base != nullptr;
	}
	hipError_t up(void *dev_p, const void *src, size_t n)
	{
		uint8_t *q = pin_base + pin_used;
		pin_used += align_up(n, 64);
		memcpy(q, src, n);
		return hipMemcpyAsync(dev_p, q, n, hipMemcpyHostToDevice, s_comp);
	}
	hipError_t back(void *dst, const void *dev_p, size_t n)
	{
		uint8_t *q = pin_base + pin_used;
		pin_used += align_up(n, 64);
		pin_pending.push_back({ dst, q, n });
		return hipMemcpyAsync(q, dev_p, n, hipMemcpyDeviceToHost, s_comp);
	}
	hipError_t pin_sync()
	{
		const hipError_t e = hipStreamSynchronize(s_comp);
		for (const pending_t &c : pin_pending)
			memcpy(c.dst, c.src, c.n);
		pin_pending.clear();
		pin_used = 0;
		return e;
	}
	/*
	 * A list a kernel made, of at most `cap` entries: its count - the last of
	 * the `cnt_words` words at d_cnt - and its first entries come with the
	 * round trip that is being queued anyway (list_back(); a stream of a few
	 * MiB has a few hundred candidates), the remainder in a second trip if the
	 * count says so (list_rest(), behind that round trip).
	 */
	template <typename T>
	hipError_t list_back(std::vector<T> &v, uint32_t first, uint32_t cap, uint32_t *cnt,
			     const uint32_t *d_cnt_, size_t cnt_words, const T *d_items)
	{
		v.resize(std::min(cap, first));
		const hipError_t e = back(cnt, d_cnt_, cnt_words * 4);
		return e != hipSuccess ? e : back(v.data(), d_items, v.size() * sizeof(T));
	}
	template <typename T>
	bool list_rest(std::vector<T> &v, uint32_t cap, uint32_t count, const T *d_items)
	{
		const uint32_t n = std::min(count, cap), first = (uint32_t)v.size();
		v.resize(n);
		if (n > first) {
			if (!pin_phase((size_t)(n - first) * sizeof(T)))
				return false;
			LDA_TRY(back(v.data() + first, d_items + first, (size_t)(n - first) * sizeof(T)));
			LDA_TRY(pin_sync());
		}
		return true;
	}

	uint32_t peek(uint64_t bit, unsigned n) const	/* n <= 24; zeros past the end */
	{
		if (!dev)
			return host_bytes.peek(bit, n);
		uint32_t v = 0;
		const uint64_t b0 = bit >> 3;
		for (unsigned k = 0; k < 4; k++)
			if (b0 + k < raw_n && b0 + k >= pk_at && b0 + k < pk_at + 8)
				v |= (uint32_t)pk[b0 + k - pk_at] << (8 * k);
		return (v >> (bit & 7)) & ((1u << n) - 1);
	}
	/* (pk_queue(): as part of a round trip that is being queued anyway) */
	hipError_t pk_queue(uint64_t bit)
	{
		const uint64_t b0 = bit >> 3;
		if (b0 == pk_at)
			return hipSuccess;
		memset(pk, 0, sizeof(pk));
		pk_at = b0;
		if (hdr + b0 >= in_nbytes)
			return hipSuccess;
		return back(pk, in + hdr + b0, std::min<size_t>(8, in_nbytes - hdr - b0));
	}
	bool fetch_pk(uint64_t bit)
	{
		if ((bit >> 3) == pk_at)
			return true;
		if (!pin_phase(64))
			return false;
		LDA_TRY(pk_queue(bit));
		LDA_TRY(pin_sync());
		return true;
	}

	bool rows_queue(uint64_t bp0)
	{
		const uint64_t span = win_n > bp0 ? win_n - bp0 : 0;
		rows_cap = (uint32_t)std::min<uint64_t>(span / 64 + 4096, 1u << 28);
		d_probe = (uint8_t *)d->sprobe.reserve(rows_at + (size_t)rows_cap * 16 + 64);
		if (!d_probe)
			return false;
		LDA_TRY(hipMemsetAsync(d_probe, 0, 16, s_comp));
		if (span >= 4) {
			const uint64_t blocks = (span + 15 + 4095) / 4096 + 1;
			hipLaunchKernelGGL(lda_stream_find_stored_kernel,
					   dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(256), 0,
					   s_comp, d_raw, win_n, bp0, (uint4 *)(d_probe + rows_at),
					   (uint32_t *)d_probe, rows_cap);
			LDA_TRY(hipGetLastError());
		}
		rows_queued = true;
		return true;
	}
	/* (the two halves of the read-back: queued with a round trip, looked at
	 * behind it) */
	hipError_t rows_back()
	{
		return list_back(rows, ROWS_FIRST, rows_cap, &rows_cnt, (const uint32_t *)d_probe, 1,
				 (const lda_stored_row *)(d_probe + rows_at));
	}
	bool rows_done()
	{
		if (!list_rest(rows, rows_cap, rows_cnt, (const lda_stored_row *)(d_probe + rows_at)))
			return false;
		sort_stored_rows(rows.data(), rows.size());
		return true;
	}
	/*
	 * A RUN OF STORED BLOCKS from the block boundary `p` on, walked by the
	 * host (5 header bytes per block of up to 65535: lib/decompress_template.h:
	 * 247-285): the finder does not look for stored blocks, and a chunk that
	 * walked such a run alone copied it alone - a level-0 file at one wave's
	 * speed.  Every stored block (several small ones together, up to `group`
	 * bits of input) becomes a chunk of its own whose result is known without
	 * a count pass; the decode pass copies them side by side.  Stops in front
	 * of the first block that is not stored, is not wholly inside the first
	 * `dev_bytes` of the stream (what the kernels can read), or is invalid
	 * (the kernels - and after them the sequential path - say what the
	 * reference says about that one).  Returns the bit it stopped at.  The
	 * walk itself is walk_stored_run() of stored_rows.h, over the stream's
	 * bytes or over the rows.
	 */
	uint64_t walk_stored(uint64_t p, uint64_t dev_bytes, std::vector<lda_stream_chunk> &oc,
			     std::vector<lda_stream_res> &orr, bool *fin_ret)
	{
		const uint64_t group = 8 * (uint64_t)(env.stream_chunk ? env.stream_chunk : 16384);
		auto emit = [&](uint64_t from, uint64_t to, uint64_t nout, bool fin) {
			lda_stream_chunk c = header_chunk(from);
			lda_stream_res r = {};
			r.start_bit = from;
			r.nout = nout;
			c.limit_bit = to;
			r.end_bit = r.end_hdr_bit = to;
			r.status = fin ? LDA_STREAM_FINAL : LDA_STREAM_OK;
			r.flags = LDA_RES_BOUNDARY;
			oc.push_back(c);
			orr.push_back(r);
			S[15]++;
		};
		if (!dev)
			return walk_stored_run(p, raw_n, dev_bytes, group, host_bytes, emit, fin_ret);
		const stored_probe_rows by_rows = { rows.data(), rows.size() };
		return walk_stored_run(p, raw_n, dev_bytes, group, by_rows, emit, fin_ret);
	}

	uint32_t cache_of(uint64_t hdr_bit) const
	{
		const auto it = hdr_slot.find(hdr_bit);
		return it == hdr_slot.end() ? 0 : it->second;
	}
	uint32_t one_length_slot(uint64_t hb, uint64_t *first_token) const
	{
		const uint32_t slot = cache_of(hb);
		if (!slot || slot > hcls.size() || !hcls[slot - 1].hi ||
		    hb + hcls[slot - 1].used >= raw_bits)
			return 0;
		*first_token = hb + hcls[slot - 1].used;
		return hcls[slot - 1].hi;
	}

	/* the streams, the container, the scratch every window shares */
	bool head()
	{
		ctx = device_ctx();
		if (!ctx || env.no_stream_par || in_nbytes < env.stream_par_min) {
			S[1] = WHY_DISABLED;
			return false;
		}
		/* (a) a stream in device memory: its first bytes, for the container
		 * header and the bits at bit 0 */
		std::vector<uint8_t> first;
		if (dev) {
			S[1] = WHY_DEVICE;
			s_copy = d->streams.copy;
			s_comp = d->streams.comp;
			first.resize(std::min<size_t>(in_nbytes, 4096));
			if (!first.empty()) {
				if (!pin_phase(first.size()))
					return false;
				LDA_TRY(back(first.data(), in, first.size()));
				LDA_TRY(pin_sync());
			}
			lap(8);
		}
		if (!container(format, dev ? first.data() : in, in_nbytes, dev ? first.size() : in_nbytes,
			       &hdr, &ftr) ||
		    (dev && hdr + 8 > first.size())) {
			S[1] = WHY_HEADER;
			return false;
		}
		raw_n = in_nbytes - hdr - ftr;
		raw_bits = 8 * raw_n;
		if (raw_n < 8) {
			S[1] = WHY_HEADER;
			return false;
		}
		S[1] = WHY_DEVICE;	/* until something better is known */
		if (!dev) {
			if (!d->streams.enter())
				return false;
			s_copy = d->streams.copy;
			s_comp = d->streams.comp;
			host_bytes = { in + hdr, raw_n };
		} else {
			memcpy(pk, first.data() + hdr, 8);
		}
		d_hlens = (uint8_t *)d->shdr.reserve((size_t)LDA_STREAM_HDR_SLOTS * (320 + 16) + 64);
		if (!d_hlens)
			return false;
		d_hinfo = (uint32_t *)(d_hlens + (size_t)LDA_STREAM_HDR_SLOTS * 320);
		return true;
	}

	/* ---- this window's input ---- */
	bool window_input(size_t W)
	{
		/* (the parsed headers are the current window's) */
		hdr_slot.clear();
		for (lda_stream_chunk &c : acc)
			c.hdr_cache = c.hint = 0;
		d_hints = nullptr;
		cache_queued = false;
		const size_t upto = std::min<size_t>(in_nbytes, std::max(copied, hdr) + W);
		if (dev) {
			/* (in place: the windows only bound what is searched) */
			d_raw = (uint8_t *)in + hdr;
			copied = upto;
			rows.clear();
			rows_queued = false;
		} else if (!sin || in_at + upto + 64 > d->sin.cap) {
			sin = (uint8_t *)d->sin.reserve(in_at + std::min<size_t>(in_nbytes, 2 * upto) + 64);
			if (!sin)
				return false;
			d_raw = sin + in_at + hdr;
			copied = 0;
		}
		if (!dev && upto > copied) {
			if (span_in(&d->pinned, sin, in_at + copied, in + copied, upto - copied, s_copy) !=
			    LIBDEFLATE_AMD_OK)
				return false;
			copied = upto;
		}
		whole = copied == in_nbytes;
		/* raw bytes the kernels may read; chunks of a partial window end a few
		 * KiB in front of that (a round stages up to 3 KiB ahead, a header 704
		 * bytes) */
		/* (never the footer: a partial window that ends inside it would let a
		 * run of stored blocks be walked past the end of the raw stream, which
		 * the reference - it hands the decoder in_nbytes - hdr - ftr bytes -
		 * rejects) */
		win_n = whole ? raw_n : std::min<uint64_t>(copied - hdr, raw_n);
		dev_n = win_n;
		R1 = whole ? raw_bits : 8 * (win_n > 8192 ? win_n - 8192 : 0);
		S[14]++;
		return true;
	}

	/* stored blocks at the carried-in boundary: the host's */
	bool carried_stored_run()
	{
		if (carry.kind != LDA_CHUNK_HEADER)
			return true;
		/* (in device memory: the bits at the boundary say whether a run
		 * begins there; only then are the rows made ahead of the finder,
		 * at the price of a round trip) */
		if (dev) {
			if (!fetch_pk(carry.start_bit))
				return false;
			if (carry.start_bit + 3 <= raw_bits && (peek(carry.start_bit, 3) >> 1) == 0) {
				if (!rows_queue((carry.start_bit + 10) >> 3) ||
				    !pin_phase(64 + (size_t)ROWS_FIRST * 16))
					return false;
				LDA_TRY(rows_back());
				LDA_TRY(pin_sync());
				if (!rows_done())
					return false;
			}
		}
		const uint64_t q = walk_stored(carry.start_bit, win_n, acc, accr, &final_seen);
		if (!final_seen && q != carry.start_bit)
			carry = header_chunk(q);
		return true;
	}

	/* ---- block starts in [carry, R1) ---- */
	bool find()
	{
		cands.clear();
		const uint64_t fb0 = carry.start_bit & ~(uint64_t)7;
		const uint64_t nbits = R1 > 80 ? R1 - 80 : 0;	/* a header needs its bits */
		{
			/* about one offset in 500 passes the first filter on compressed
			 * data and a real block is rarely under a few hundred bits; a
			 * queue that overflows only loses entry points */
			const uint64_t span = nbits > fb0 ? nbits - fb0 : 0;
			qcap = (uint32_t)std::min<uint64_t>(span / 128 + 4096, 1u << 28);
			ccap = (uint32_t)std::min<uint64_t>(span / 512 + 4096, 1u << 26);
			uint8_t *sq = (uint8_t *)d->squeue.reserve(((size_t)qcap + ccap) * 8 + 128);
			if (!sq)
				return false;
			d_queue = (uint64_t *)sq;
			d_cand = d_queue + qcap;
			d_cnt = (uint32_t *)(d_cand + ccap);
		}
		LDA_TRY(hipMemsetAsync(d_cnt, 0, 16, s_comp));
		if (nbits <= fb0)
			return true;
		const bool rows_here = dev && !rows_queued;
		if (rows_here && !rows_queue((carry.start_bit + 10) >> 3))
			return false;
		for (uint64_t b0 = fb0; b0 < nbits; b0 += 1ull << 31) {
			const uint64_t nb = std::min<uint64_t>(nbits - b0, 1ull << 31);
			/* (a workgroup of four waves takes 16 windows of 4 x 64 bytes) */
			hipLaunchKernelGGL(lda_stream_find_a_kernel, dim3((unsigned)((nb + 32767) / 32768)),
					   dim3(256), 0, s_comp, d_raw, win_n, b0, nbits, d_queue, d_cnt, qcap);
		}
		hipLaunchKernelGGL(lda_stream_find_b_kernel,
				   dim3(std::min<unsigned>((qcap + 63) / 64, 8u * (unsigned)ctx->num_cus)),
				   dim3(64), lda_stream_find_b_lds(),
				   s_comp, d_raw, win_n, d_queue, d_cnt, qcap, d_cand, d_cnt + 1, ccap);
		LDA_TRY(hipGetLastError());
		LDA_TRY(hipEventRecord(d->streams.mark, s_comp));
		LDA_TRY(hipStreamWaitEvent(s_copy, d->streams.mark, 0));
		hipLaunchKernelGGL(lda_stream_hdr_cache_kernel, dim3(8u * (unsigned)ctx->num_cus), dim3(64),
				   lda_stream_hdr_cache_lds(), s_copy, d_raw, win_n, d_cand, d_cnt + 1,
				   std::min<uint32_t>(ccap, LDA_STREAM_HDR_SLOTS), d_hlens, d_hinfo);
		LDA_TRY(hipGetLastError());
		uint2 *d_cls = nullptr;
		if (dev && !env.stream_chunk) {
			/* (the scratch exists: the rows of this window were queued) */
			d_cls = (uint2 *)(d_probe + cls_at);
			hipLaunchKernelGGL(lda_stream_hdr_class_kernel, dim3(LDA_STREAM_HDR_SLOTS / 64),
					   dim3(64), 0, s_copy, d_cnt + 1,
					   std::min<uint32_t>(ccap, LDA_STREAM_HDR_SLOTS), d_hlens, d_hinfo,
					   d_cls);
			LDA_TRY(hipGetLastError());
		}
		LDA_TRY(hipEventRecord(d->streams.mark2, s_copy));
		cache_queued = true;
		/* the counts and the first candidates in one round trip */
		const uint32_t first = std::min<uint32_t>(ccap, 2048);
		uint32_t cnt[2];
		if (!pin_phase(64 + (size_t)first * 8 + (rows_here ? 128 + (size_t)ROWS_FIRST * 16 : 0)))
			return false;
		LDA_TRY(list_back(cands, first, ccap, cnt, d_cnt, 2, d_cand));
		if (rows_here)
			LDA_TRY(rows_back());
		if (dev && carry.kind == LDA_CHUNK_HEADER)
			LDA_TRY(pk_queue(carry.start_bit));
		LDA_TRY(pin_sync());
		if (rows_here && !rows_done())
			return false;
		if (!list_rest(cands, ccap, cnt[1], d_cand))
			return false;
		const uint32_t nc = (uint32_t)cands.size();
		for (uint32_t i = 0; i < nc && i < LDA_STREAM_HDR_SLOTS; i++)
			hdr_slot.emplace(cands[i], i + 1);
		hcls.clear();
		if (d_cls && nc) {
			/* the classes of the headers in the slots, behind the kernel that
			 * parsed them: the plan needs them */
			hcls.resize(std::min<uint32_t>(nc, LDA_STREAM_HDR_SLOTS));
			if (!pin_phase(hcls.size() * 8))
				return false;
			LDA_TRY(hipMemcpyAsync(pin_base, d_cls, hcls.size() * 8, hipMemcpyDeviceToHost, s_copy));
			LDA_TRY(hipStreamSynchronize(s_copy));
			memcpy(hcls.data(), pin_base, hcls.size() * 8);
		}
		std::sort(cands.begin(), cands.end());
		S[2] += cnt[0];
		S[3] += nc;
		return true;
	}

	/* ---- plan ----
	 * chunks of a few KiB of input: up to about two thousand for a window
	 * that has them (a wave slot each on 256 CUs, one launch of the decode
	 * pass), never under 2 KiB (the warm-up in front of an inner chunk is
	 * 1 KiB) */
	bool plan()
	{
		uint64_t T = env.stream_chunk ? (uint64_t)env.stream_chunk :
						(R1 - carry.start_bit) / 8 / 1536;
		T = 8 * std::min<uint64_t>(std::max<uint64_t>(T, 2048), 65536);
		if (dev && carry.kind == LDA_CHUNK_HEADER && !fetch_pk(carry.start_bit))
			return false;
		const bool static_at_carry =
			carry.kind == LDA_CHUNK_HEADER && (peek(carry.start_bit, 3) >> 1) == 1;
		auto one_length = [&](uint64_t hb, uint64_t *first_token) -> uint32_t {
			return env.stream_chunk ? 0 :
			       dev ? one_length_slot(hb, first_token) :
				     one_length_code(host_bytes, raw_bits, hb, first_token);
		};
		plan_ = plan_window(carry, cands, R1, T, static_at_carry, one_length, &nexact);
		if (!hdr_slot.empty())
			for (planned &q : plan_)
				q.c.hdr_cache = cache_of(q.c.hdr_bit);
		S[4] += plan_.size();
		dbg("planned");
		if (cache_queued)
			LDA_TRY(hipStreamWaitEvent(s_comp, d->streams.mark2, 0));
		return true;
	}

	/* ---- count ---- */
	bool count()
	{
		const uint32_t np = (uint32_t)plan_.size();
		const size_t res_at = align_up((size_t)np * sizeof(lda_stream_chunk) + 64, 64);
		uint8_t *sch = (uint8_t *)d->schunks.reserve(
			res_at + align_up((size_t)np * sizeof(lda_stream_res) + 64, 64));
		if (!sch)
			return false;
		lda_stream_chunk *d_chunks = (lda_stream_chunk *)sch;
		lda_stream_res *d_res = (lda_stream_res *)(sch + res_at);
		hc.resize(np);
		for (uint32_t i = 0; i < np; i++)
			hc[i] = plan_[i].c;
		hr.assign(np, lda_stream_res());
		if (!pin_phase((size_t)np * (sizeof(lda_stream_chunk) + sizeof(lda_stream_res)) + 256))
			return false;
		LDA_TRY(up(d_chunks, hc.data(), (size_t)np * sizeof(lda_stream_chunk)));
		/* (the chunks counted together leave the decode pass their lanes' starts:
		 * a row of 64 per chunk of this launch, see phase_count()) */
		if (nexact) {
			d_hints = (uint16_t *)d->shint.reserve((size_t)np * 128 + 64);
			if (!d_hints)
				return false;
		}
		if (!launch_count(s_comp, np, d_chunks, d_res, d_raw, win_n, d_hlens, d_hinfo,
				  nexact ? d_hints : nullptr))
			return false;
		LDA_TRY(back(hr.data(), d_res, (size_t)np * sizeof(lda_stream_res)));
		dbg("count queued");
		LDA_TRY(pin_sync());
		dbg("counted");
		return true;
	}

	/* one round of repairs (stream_chain::close()): counted like the plan */
	bool count_repairs(const stream_chain &ch, std::vector<lda_stream_chunk> &rc,
			   std::vector<lda_stream_res> &rr)
	{
		if (debug) {
			const uint32_t e = ch.path.back();
			dbg("walked");
			fprintf(stderr, "round %d: walk of %zu stops after chunk %u (kind %u hdr %llu start %llu) "
				"end %llu bnd %u endhdr %llu status %u nout %llu\n", ch.round, ch.path.size(), e,
				ch.pc[e].kind, (unsigned long long)ch.pc[e].hdr_bit,
				(unsigned long long)ch.pr[e].start_bit, (unsigned long long)ch.pr[e].end_bit,
				ch.pr[e].flags & 1, (unsigned long long)ch.pr[e].end_hdr_bit, ch.pr[e].status,
				(unsigned long long)ch.pr[e].nout);
		}
		const uint32_t nr = (uint32_t)rc.size();
		if (!hdr_slot.empty())
			for (lda_stream_chunk &c : rc)
				c.hdr_cache = cache_of(c.hdr_bit);
		uint8_t *rp = (uint8_t *)d->srepair.reserve(
			(size_t)nr * (sizeof(lda_stream_chunk) + sizeof(lda_stream_res)) + 128);
		if (!rp)
			return false;
		lda_stream_chunk *d_rc = (lda_stream_chunk *)rp;
		lda_stream_res *d_rr = (lda_stream_res *)(rp + align_up((size_t)nr * sizeof(lda_stream_chunk), 64));
		if (!pin_phase((size_t)nr * (sizeof(lda_stream_chunk) + sizeof(lda_stream_res)) + 256))
			return false;
		LDA_TRY(up(d_rc, rc.data(), (size_t)nr * sizeof(lda_stream_chunk)));
		if (!launch_count(s_comp, nr, d_rc, d_rr, d_raw, win_n, d_hlens, d_hinfo, nullptr))
			return false;
		LDA_TRY(back(rr.data(), d_rr, (size_t)nr * sizeof(lda_stream_res)));
		dbg("repairs queued");
		LDA_TRY(pin_sync());
		dbg("repairs counted");
		return true;
	}

	/* ---- chain ---- (stream_plan.h), and what the window leaves: its part
	 * of the accepted chain and the state the next window goes on from */
	bool chain()
	{
		const uint32_t np = (uint32_t)plan_.size();
		stream_chain ch(plan_, hc, hr);
		dbg("pool built");
		const uint64_t stop = std::min<uint64_t>(win_n, (R1 + 7) / 8 + 65536 + 16);
		const int why = ch.close(
			carry_gf, whole, R1,
			[&](uint64_t bit, std::vector<lda_stream_chunk> &oc, std::vector<lda_stream_res> &orr) {
				bool fin = false;
				(void)walk_stored(bit, stop, oc, orr, &fin);
			},
			[&](std::vector<lda_stream_chunk> &rc, std::vector<lda_stream_res> &rr) {
				return count_repairs(ch, rc, rr);
			},
			&S[5]);
		if (why != WHY_OK) {
			S[1] = why;
			return false;
		}
		final_seen = ch.final_seen;
		for (uint32_t i : ch.path) {
			lda_stream_chunk c = ch.pc[i];
			/* (one of the starts counted together in the window's first
			 * launch: row i holds where its parse entered the pieces) */
			c.hint = ch.pc[i].phases && i < np && d_hints ? i + 1 : 0;
			c.phases = 0;
			if (c.kind == LDA_CHUNK_WARM) {
				c.kind = LDA_CHUNK_EXACT;
				c.start_bit = ch.pr[i].start_bit;
			}
			acc.push_back(c);
			accr.push_back(ch.pr[i]);
		}
		if (!ch.path.empty() && !final_seen) {
			/* the next window goes on from where this one's chain ends */
			const lda_stream_res &e = ch.pr[ch.path.back()];
			carry = carry_from(e);
			carry_gf = !(e.flags & LDA_RES_BOUNDARY) && ch.gf_end;
		}
		lap(10);
		if (whole && !final_seen) {
			S[1] = WHY_NOFINAL;
			return false;
		}
		/* an output buffer that is already too small is known now: no further
		 * window is copied and searched for a call that cannot succeed here
		 * (programs/gzip.c retries with a larger buffer: every attempt would
		 * pay for all windows) */
		uint64_t sofar = 0;
		for (const lda_stream_res &r : accr)
			sofar += r.nout;
		if (sofar > out_avail) {
			S[1] = WHY_SPACE;
			return false;
		}
		return true;
	}

	/*
	 * The input is taken in WINDOWS (4 to 16 MiB of it, then four times as much
	 * each time, up to all of it): copied to the device, searched for block starts,
	 * planned, counted and chained - and when the chain reaches the stream's
	 * final block inside a window, the rest of the input is never touched.  The
	 * reference's callers hand the decompressor everything that is left of a
	 * file (programs/gzip.c:236-299 loops over the members of a .gz that way):
	 * without windows every call on a multi-member file would copy and search
	 * the whole remainder.  A window that ends before the final block hands its
	 * last accepted state (position, governing header) to the next one.
	 */
	bool windows()
	{
		/* (the first window by the output space: a stream rarely takes more input
		 * than half of what it produces, so one that fits the caller's buffer
		 * usually ends inside a window of out_avail / 2) */
		const size_t W0 = env.stream_window ? env.stream_window :
				  std::min<size_t>(std::max<size_t>(out_avail / 2, (size_t)4 << 20), (size_t)16 << 20);
		for (size_t W = W0; !final_seen; W = W < ((size_t)1 << 40) ? W * 4 : W) {
			if (!window_input(W) || !carried_stored_run())
				return false;
			if (final_seen)
				break;
			if (R1 <= carry.start_bit + 4096 && !whole)
				continue;
			lap(8);
			if (!find())
				return false;
			lap(9);
			if (!plan() || !count() || !chain())
				return false;
		}
		return true;
	}

	/* the accepted chain's output offsets; is the stream this path's to answer? */
	bool totals()
	{
		const uint32_t na = (uint32_t)acc.size();
		S[6] = na;
		total = 0;
		for (uint32_t i = 0; i < na; i++) {
			acc[i].out_off = total;
			total += accr[i].nout;
		}
		const uint64_t end_bit = accr[na - 1].end_bit;
		if (end_bit > raw_bits) {
			/* a chain that closes beyond the raw stream (inside the footer): the
			 * sequential kernel decides what the reference would say, and the
			 * footer is never read at f = in + hdr + consumed past the buffer */
			S[1] = WHY_NOFINAL;
			return false;
		}
		if (total > out_avail) {
			S[1] = WHY_SPACE;
			return false;
		}
		if (exact_fill && total != out_avail) {
			S[1] = WHY_FILL;
			return false;
		}
		consumed = (size_t)((end_bit + 7) / 8);
		return true;
	}

	/* the window chain: groups of chunks side by side with a symbolic
	 * window, the groups' windows composed by a prefix scan (log2
	 * launches), the groups again from their real windows.  Up to 512
	 * groups - two workgroups of 64 KiB LDS per CU - of at least four
	 * chunks (round 5: sqrt(chunks) / 2 groups, because a serial link
	 * step per group had to be paid) */
	bool launch_windows(uint32_t na, const uint64_t *d_off, const uint16_t *d_sym, uint8_t *d_out)
	{
		uint32_t per_group = 4;
		while ((uint64_t)per_group * 512 < na)
			per_group++;
		const uint32_t groups = (na + per_group - 1) / per_group;
		uint8_t *gw = (uint8_t *)d->swin.reserve((size_t)groups * 65536 * 2 + 64);
		if (!gw)
			return false;
		uint16_t *d_gwin = (uint16_t *)gw;
		uint16_t *d_gwin2 = d_gwin + (size_t)groups * 32768;
		const uint16_t *d_fwin = d_gwin;
		if (!ctx->stream_attr_set.load(std::memory_order_acquire)) {
			LDA_TRY(hipFuncSetAttribute((const void *)lda_stream_window_kernel,
						    hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
			LDA_TRY(hipFuncSetAttribute((const void *)lda_stream_window_scan_kernel,
						    hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
			ctx->stream_attr_set.store(true, std::memory_order_release);
		}
		if (groups > 1) {
			hipLaunchKernelGGL(lda_stream_window_kernel, dim3(groups), dim3(1024), 65536,
					   s_comp, na, per_group, 0u, d_off, d_sym, d_out, d_gwin,
					   d_fwin, d_cnt + 2);
			/* (the window behind the last group is nobody's) */
			uint16_t *src = d_gwin, *dst = d_gwin2;
			for (uint32_t h = 1; h < groups - 1; h *= 2) {
				hipLaunchKernelGGL(lda_stream_window_scan_kernel, dim3(groups - 1), dim3(1024),
						   65536, s_comp, groups - 1, h, src, dst);
				std::swap(src, dst);
			}
			d_fwin = src;
		}
		hipLaunchKernelGGL(lda_stream_window_kernel, dim3(groups), dim3(1024), 65536, s_comp,
				   na, per_group, 2u, d_off, d_sym, d_out, d_gwin, d_fwin, d_cnt + 2);
		return true;
	}

	/* ---- decode -> window -> resolve -> checksum, one round trip ----
	 * Everything is queued on the compute stream; what comes back (the decode
	 * pass's per-chunk results, the error flag, the pieces' checksums) is
	 * looked at after ONE synchronisation, and the output is on its way to the
	 * caller meanwhile: the copy stream waits for the resolve pass, not for the
	 * host.  (Output is undefined on failure, libdeflate.h:216-217; when the
	 * sequential kernel has to decide it writes the buffer again.) */
	bool finish()
	{
		const uint32_t na = (uint32_t)acc.size();
		sum = format == LIBDEFLATE_AMD_GZIP ? 0u : 1u;
		if (!total) {
			/* (b) the footer of a stream in device memory */
			if (dev && ftr) {
				if (!pin_phase(64))
					return false;
				LDA_TRY(back(fbytes, in + hdr + consumed, ftr));
				LDA_TRY(pin_sync());
			}
			return true;
		}
		std::vector<uint64_t> offs(na + 1);
		for (uint32_t i = 0; i < na; i++)
			offs[i] = acc[i].out_off;
		offs[na] = total;
		if (!d_cnt) {
			/* (no window went through the block finder: every block was
			 * the host's) */
			uint8_t *sq = (uint8_t *)d->squeue.reserve(128);
			if (!sq)
				return false;
			d_cnt = (uint32_t *)sq;
		}
		/* [2]: the error flag of the window / resolve kernels */
		LDA_TRY(hipMemsetAsync(d_cnt, 0, 16, s_comp));
		uint16_t *d_sym = (uint16_t *)d->ssym.reserve((size_t)total * 2 + 64);
		/* (the window and resolve kernels write bytes and, guarded by
		 * i + 8 <= the chunk's end, 8-byte words at any alignment: nothing at or
		 * past d_out + total, so they can write a caller's device buffer) */
		uint8_t *d_out = dev ? out : (uint8_t *)d->sout.reserve((size_t)total + 64);
		uint32_t *d_tok = stream_token_scratch(d, na);
		if (!d_sym || !d_out || !d_tok)
			return false;
		/* (the accepted chain may hold more chunks than were planned) */
		const size_t res2_at = align_up((size_t)na * sizeof(lda_stream_chunk) + 64, 64);
		const size_t off2_at = res2_at + align_up((size_t)na * sizeof(lda_stream_res) + 64, 64);
		uint8_t *sch = (uint8_t *)d->schunks.reserve(off2_at + ((size_t)na + 2) * 8 + 64);
		if (!sch)
			return false;
		lda_stream_chunk *d_chunks = (lda_stream_chunk *)sch;
		lda_stream_res *d_res = (lda_stream_res *)(sch + res2_at);
		uint64_t *d_off = (uint64_t *)(sch + off2_at);
		/* pieces of the output for the checksum kernels */
		const uint64_t piece = std::max<uint64_t>(65536, align_up(total / 4096, 4096));
		const size_t npc = ftr ? (size_t)((total + piece - 1) / piece) : 0;
		std::vector<uint64_t> po(2 * npc);
		for (size_t i = 0; i < npc; i++) {
			po[i] = i * piece;
			po[npc + i] = std::min<uint64_t>(piece, total - i * piece);
		}
		uint8_t *scr = npc ? (uint8_t *)d->scratch.reserve(npc * 20 + 64) : nullptr;
		if (npc && !scr)
			return false;
		uint64_t *d_po = (uint64_t *)scr;
		uint32_t *d_sums = (uint32_t *)(scr + npc * 16);
		if (!pin_phase((size_t)na * (sizeof(lda_stream_chunk) + sizeof(lda_stream_res) + 8) +
			       npc * 20 + 1024))
			return false;
		LDA_TRY(up(d_chunks, acc.data(), (size_t)na * sizeof(lda_stream_chunk)));
		LDA_TRY(up(d_off, offs.data(), ((size_t)na + 1) * 8));
		if (npc)
			LDA_TRY(up(d_po, po.data(), npc * 16));
		for (size_t lo = 0; lo < na; lo += STREAM_DECODE_BATCH) {
			const uint32_t nk = (uint32_t)std::min<size_t>(STREAM_DECODE_BATCH, na - lo);
			hipLaunchKernelGGL(lda_stream_decode_kernel, dim3(nk), dim3(64),
					   lda_stream_chunk_lds(), s_comp, nk, d_chunks + lo,
					   d_res + lo, d_raw, dev_n, d_sym, d_tok, d_hlens, d_hinfo, d_hints);
		}
		if (!launch_windows(na, d_off, d_sym, d_out))
			return false;
		uint64_t longest = 0;
		for (uint32_t i = 0; i < na; i++)
			longest = std::max(longest, accr[i].nout);
		if (longest > 32768) {
			const unsigned gx = (unsigned)std::min<uint64_t>((longest - 32768 + 2047) / 2048, 64);
			/* (grid.y <= 65535: a window of small blocks can have more
			 * chunks than that) */
			for (uint32_t c0 = 0; c0 < na; c0 += 32768)
				hipLaunchKernelGGL(lda_stream_resolve_kernel,
						   dim3(gx, std::min<uint32_t>(32768, na - c0)), dim3(256),
						   0, s_comp, na, c0, d_off, d_sym, d_out, d_cnt + 2);
		}
		LDA_TRY(hipGetLastError());
		LDA_TRY(hipEventRecord(d->streams.mark, s_comp));	/* the bytes are final */
		if (npc) {
			const int rc = format == LIBDEFLATE_AMD_GZIP ?
				libdeflate_amd_crc32_batch(npc, d_out, d_po, d_po + npc, NULL, d_sums, s_comp) :
				libdeflate_amd_adler32_batch(npc, d_out, d_po, d_po + npc, NULL, d_sums, s_comp);
			if (rc != LIBDEFLATE_AMD_OK)
				return false;
		}
		std::vector<lda_stream_res> dr(na);
		std::vector<uint32_t> sums(npc);
		uint32_t err = 0;
		LDA_TRY(back(dr.data(), d_res, (size_t)na * sizeof(lda_stream_res)));
		LDA_TRY(back(&err, d_cnt + 2, 4));
		if (npc)
			LDA_TRY(back(sums.data(), d_sums, npc * 4));
		if (dev && ftr)
			LDA_TRY(back(fbytes, in + hdr + consumed, ftr));
		lap(11);
		if (debug) {
			LDA_TRY(hipEventSynchronize(d->streams.mark));
			dbg("decode .. resolve kernels");
		}
		/* the output, beside the checksum kernels and the read-backs */
		if (!dev) {
			LDA_TRY(hipStreamWaitEvent(s_copy, d->streams.mark, 0));
			if (span_out(&d->pinned, d_out, 0, out, (size_t)total, s_copy) != LIBDEFLATE_AMD_OK)
				return false;
			lap(13);
		}
		LDA_TRY(pin_sync());
		if (dev)
			lap(13);	/* (nothing to copy: the wait for the last kernel) */
		bool same = err == 0;
		for (uint32_t i = 0; i < na && same; i++)
			same = dr[i].end_bit == accr[i].end_bit && dr[i].nout == accr[i].nout &&
			       dr[i].status == accr[i].status && !(dr[i].flags & LDA_RES_BAD_DIST);
		if (!same) {
			S[1] = WHY_DECODE;
			return false;
		}
		const uint32_t shp = format == LIBDEFLATE_AMD_GZIP ? crc32_shift(piece) : 0;
		for (size_t i = 0; i < npc; i++)
			sum = i == 0 ? sums[0] :
			      format != LIBDEFLATE_AMD_GZIP ? adler32_concat(sum, sums[i], po[npc + i]) :
			      po[npc + i] == piece ? crc32_concat_shift(sum, sums[i], shp) :
						     crc32_concat(sum, sums[i], po[npc + i]);
		return true;
	}

	/* the container's footer against what was decoded */
	int32_t footer() const
	{
		if (!ftr)
			return LIBDEFLATE_SUCCESS;
		const uint8_t *f = dev ? fbytes : in + hdr + consumed;
		if (format == LIBDEFLATE_AMD_GZIP) {
			const uint32_t want = f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) |
					      ((uint32_t)f[3] << 24);
			const uint32_t isize = f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) |
					       ((uint32_t)f[7] << 24);
			return want != sum || isize != (uint32_t)total ? LIBDEFLATE_BAD_DATA : LIBDEFLATE_SUCCESS;
		}
		const uint32_t want = ((uint32_t)f[0] << 24) | ((uint32_t)f[1] << 16) |
				      ((uint32_t)f[2] << 8) | f[3];
		return want != sum ? LIBDEFLATE_BAD_DATA : LIBDEFLATE_SUCCESS;
	}

	/* the chain that was proved, for a seek index (host_seek.hip) */
	void export_seek(seek_export *seek) const
	{
		seek->parallel = seek->known = true;
		seek->raw_off = hdr;
		seek->raw_nbytes = consumed;
		seek->ftr = ftr;
		seek->total = total;
		seek->chain.resize(acc.size());
		for (size_t i = 0; i < acc.size(); i++)
			seek->chain[i] = { acc[i].out_off, acc[i].start_bit, acc[i].hdr_bit, acc[i].kind };
	}

	bool body(int32_t *res, size_t *ain, size_t *aout, seek_export *seek)
	{
		if (!head() || !windows() || !totals() || !finish())
			return false;
		const int32_t result = footer();
		lap(12);
		*res = result;
		if (result == LIBDEFLATE_SUCCESS) {
			*ain = hdr + consumed + ftr;
			*aout = (size_t)total;
			if (seek)
				export_seek(seek);
		}
		S[0] = 1;
		S[1] = WHY_OK;
		S[7] = total;
		return true;
	}

	/* THE ONE EXIT.  A refusal may come while kernels of this call are still
	 * queued (the header cache and the header classes on the copy stream
	 * behind a failed round trip, say), and the sequential path that takes
	 * over uses the same object: nothing of this call is in flight on d->sin,
	 * d->squeue, d->shdr or d->sprobe when it starts - however the call is
	 * left, an exception included.  (Both streams are idle in every refusal
	 * but a device error.) */
	bool answered = false;
	bool run(int32_t *res, size_t *ain, size_t *aout, seek_export *seek)
	{
		return answered = body(res, ain, aout, seek);
	}
	~StreamRun()
	{
		if (!answered && s_copy) {
			(void)hipStreamSynchronize(s_copy);
			(void)hipStreamSynchronize(s_comp);
		}
	}
};

} /* namespace */

/*
 * true: *res (and on success *ain / *aout, the output in `out`) are final.
 * false: not answered here - the caller takes the sequential path (the reason
 * is in the stats; a device failure is also in last_error).
 */
bool decompress_stream_parallel(struct libdeflate_decompressor *d, int format,
				const uint8_t *in, size_t in_nbytes, uint8_t *out,
				size_t out_avail, bool exact_fill, int32_t *res,
				size_t *ain, size_t *aout, bool on_device, seek_export *seek)
{
	StreamRun run(d, format, in, in_nbytes, out, out_avail, exact_fill, on_device);
	return run.run(res, ain, aout, seek);
}

} /* namespace lda */

/*
 * ONE large stream in DEVICE memory -> its bytes in device memory.  The
 * many-wave path answers for what it decoded cleanly; everything else is the
 * device batch of one on the same stream, the sequential kernel that follows
 * the reference's result codes bit for bit - the rule of decompress_one()
 * (host_decompress.hip).  Blocking: the chain check is the host's.
 */
namespace lda {
enum libdeflate_result
decompress_large_body(struct libdeflate_decompressor *d, int format, const uint8_t *d_in,
		      size_t in_nbytes, uint8_t *d_out, size_t out_avail, size_t *actual_in_ret,
		      size_t *actual_out_ret, hipStream_t user, const char *what, seek_export *seek)
{
	DeviceGuard on(d->device);
	if (!on.ok() || !device_ctx() || !d->streams.ensure()) {
		complain(what, LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_BAD_DATA;	/* a library-side failure, see decompress_one() */
	}
	hipStream_t sc = d->streams.comp;
	/* the object's streams go on behind what is queued on the caller's: d_in
	 * may be the product of kernels there */
	if (hipEventRecord(d->streams.mark, user) != hipSuccess ||
	    hipStreamWaitEvent(sc, d->streams.mark, 0) != hipSuccess ||
	    hipStreamWaitEvent(d->streams.copy, d->streams.mark, 0) != hipSuccess) {
		set_error("%s: %s", what, hipGetErrorString(hipGetLastError()));
		complain(what, LIBDEFLATE_AMD_NO_DEVICE);
		return LIBDEFLATE_BAD_DATA;
	}
	int32_t res = LIBDEFLATE_BAD_DATA;
	size_t ain = 0, aout = 0;
	bool answered = d_in && d_out &&
			no_unwind("libdeflate_amd_decompress_large (many waves)", false, [&]() {
				return decompress_stream_parallel(d, format, d_in, in_nbytes, d_out, out_avail,
								  actual_out_ret == NULL, &res, &ain, &aout,
								  true, seek);
			});
	if (!d_in || !d_out) {
		memset(g_stats, 0, sizeof(g_stats));
		g_stats[1] = WHY_DISABLED;
	}
	if (!answered) {
		/* [in_off in_n out_off out_avail ain aout][result]; a NULL buffer of
		 * size 0 is any valid address */
		uint8_t *st = (uint8_t *)d->stage.reserve(256);
		uint64_t *desc = st ? (uint64_t *)d->meta.ensure(256) : nullptr;
		if (!desc) {
			(void)hipStreamSynchronize(sc);
			complain(what, LIBDEFLATE_AMD_OOM);
			return LIBDEFLATE_BAD_DATA;
		}
		uint64_t *dd = (uint64_t *)st;
		desc[0] = 0;
		desc[1] = in_nbytes;
		desc[2] = 0;
		desc[3] = out_avail;
		desc[4] = desc[5] = 0;
		desc[6] = (uint64_t)LIBDEFLATE_BAD_DATA;
		int rc = LIBDEFLATE_AMD_OK;
		if (hipMemcpyAsync(st, desc, 56, hipMemcpyHostToDevice, sc) != hipSuccess)
			rc = LIBDEFLATE_AMD_NO_DEVICE;
		if (rc == LIBDEFLATE_AMD_OK)
			rc = libdeflate_amd_decompress_batch(d, format, 1, d_in ? d_in : st, dd, dd + 1,
							     d_out ? d_out : st + 128, dd + 2, dd + 3,
							     (int32_t *)(dd + 6), dd + 4,
							     actual_out_ret ? dd + 5 : NULL, sc);
		if (rc == LIBDEFLATE_AMD_OK &&
		    hipMemcpyAsync(desc, st, 56, hipMemcpyDeviceToHost, sc) != hipSuccess)
			rc = LIBDEFLATE_AMD_NO_DEVICE;
		if (hipStreamSynchronize(sc) != hipSuccess && rc == LIBDEFLATE_AMD_OK)
			rc = LIBDEFLATE_AMD_NO_DEVICE;
		if (rc != LIBDEFLATE_AMD_OK) {
			if (rc == LIBDEFLATE_AMD_NO_DEVICE)
				set_error("%s: %s", what, hipGetErrorString(hipGetLastError()));
			complain(what, rc);
			return LIBDEFLATE_BAD_DATA;
		}
		res = (int32_t)desc[6];
		ain = (size_t)desc[4];
		aout = (size_t)desc[5];
	}
	if (seek && !answered && res == LIBDEFLATE_SUCCESS) {
		/* the sequential decoder answered: the index is point 0 alone, and it
		 * needs the container's sizes (the header from the stream's first
		 * bytes, fetched here: 4 KiB, or 1 MiB for a gzip header that long) */
		size_t hdr = 0, ftr = 0;
		bool have = false;
		for (size_t want : { (size_t)4096, (size_t)1 << 20 }) {
			const size_t n = std::min(in_nbytes, want);
			uint8_t *h = n ? (uint8_t *)d->meta.ensure(n) : nullptr;
			if (n && (!h || hipMemcpyAsync(h, d_in, n, hipMemcpyDeviceToHost, sc) != hipSuccess ||
				  hipStreamSynchronize(sc) != hipSuccess))
				break;
			if (container(format, h, in_nbytes, n, &hdr, &ftr) && hdr + ftr <= ain) {
				have = true;
				break;
			}
			if (n == in_nbytes)
				break;
		}
		seek->parallel = false;
		seek->known = have;
		seek->raw_off = hdr;
		seek->raw_nbytes = have ? ain - hdr - ftr : 0;
		seek->ftr = ftr;
		seek->total = actual_out_ret ? aout : out_avail;
		seek->chain.assign(1, seek_link{ 0, 0, 0, LDA_CHUNK_HEADER });
	}
	if (res == LIBDEFLATE_SUCCESS) {
		if (actual_in_ret)
			*actual_in_ret = ain;
		if (actual_out_ret)
			*actual_out_ret = aout;
	}
	return (enum libdeflate_result)res;
}
} /* namespace lda */

extern "C" LIBDEFLATEAPI enum libdeflate_result
libdeflate_amd_decompress_large(struct libdeflate_decompressor *d, int format,
				const void *d_in, size_t in_nbytes, void *d_out,
				size_t out_nbytes_avail, size_t *actual_in_nbytes_ret,
				size_t *actual_out_nbytes_ret, void *stream)
{
	using namespace lda;
	if (!d) {
		set_error("libdeflate_amd_decompress_large: NULL decompressor");
		return LIBDEFLATE_BAD_DATA;
	}
	if (!d_in && in_nbytes) {
		set_error("libdeflate_amd_decompress_large: NULL d_in with in_nbytes != 0");
		return LIBDEFLATE_BAD_DATA;
	}
	if (!d_out && out_nbytes_avail) {
		set_error("libdeflate_amd_decompress_large: NULL d_out with out_nbytes_avail != 0");
		return LIBDEFLATE_BAD_DATA;
	}
	if (format != LIBDEFLATE_AMD_DEFLATE && format != LIBDEFLATE_AMD_ZLIB &&
	    format != LIBDEFLATE_AMD_GZIP) {
		set_error("libdeflate_amd_decompress_large: format %d is not DEFLATE, zlib or gzip",
			  format);
		return LIBDEFLATE_BAD_DATA;
	}
	return no_unwind("libdeflate_amd_decompress_large", LIBDEFLATE_BAD_DATA, [&]() {
		return decompress_large_body(d, format, (const uint8_t *)d_in, in_nbytes,
					     (uint8_t *)d_out, out_nbytes_avail, actual_in_nbytes_ret,
					     actual_out_nbytes_ret, (hipStream_t)stream,
					     "libdeflate_amd_decompress_large", nullptr);
	});
}

extern "C" LIBDEFLATEAPI void libdeflate_amd_stream_stats(uint64_t *out)
{
	memcpy(out, lda::g_stats, sizeof(lda::g_stats));
}
