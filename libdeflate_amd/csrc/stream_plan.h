/*
 * stream_plan.h - the host arithmetic of ONE large stream on many waves
 * (host_stream.hip): which chunks a window of the input is cut into (the
 * plan), and how the counted chunks are joined into one proved parse from the
 * carried-in state to the window's end or the stream's final block (the
 * chain).  Bit offsets in, chunk descriptors out: no HIP, no decompressor
 * object and no globals in here - tools/test_stream_plan.cpp compiles it with
 * the host compiler alone and drives the chain with a model of the count
 * kernel.
 */
#ifndef LDA_STREAM_PLAN_H
#define LDA_STREAM_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "stream_types.h"

namespace lda {

/* why the many-wave path did not answer (slot 1 of the stream stats) */
enum { WHY_OK = 0, WHY_DISABLED, WHY_HEADER, WHY_CHAIN, WHY_ERRCHUNK, WHY_NOFINAL,
       WHY_SPACE, WHY_FILL, WHY_DECODE, WHY_DEVICE, WHY_REPAIRS };

struct planned {
	lda_stream_chunk c;
	uint64_t at;	/* nominal start: hdr_bit (HEADER) or target_bit (WARM) */
};

/* a warm-up is at most OV bits, and never starts within HDRSAFE bits of the
 * header that a HEADER first chunk reads */
static const uint64_t STREAM_OV = 8192, STREAM_HDRSAFE = 4608;
/* (the starts of one position are counted together by ONE wave,
 * phase_count() of inflate_stream.hip, when the chunk is one
 * round of input: 1.5 x TN <= 64 pieces of 384 bits) */
static const uint64_t STREAM_TN = 15360;
/* phase candidates (see stream_chain::repairs()): starts asked at one position */
static const uint32_t STREAM_PHASES = 10;

/* the chunk that starts at the block header at `bit` */
static inline lda_stream_chunk header_chunk(uint64_t bit)
{
	lda_stream_chunk c = {};
	c.kind = LDA_CHUNK_HEADER;
	c.hdr_bit = c.start_bit = c.target_bit = bit;
	return c;
}

/* the chunk that goes on exactly where `e` ended (its limit is the caller's) */
static inline lda_stream_chunk carry_from(const lda_stream_res &e)
{
	if (e.flags & LDA_RES_BOUNDARY)
		return header_chunk(e.end_bit);
	lda_stream_chunk c = {};
	c.kind = LDA_CHUNK_EXACT;
	c.hdr_bit = e.end_hdr_bit;
	c.start_bit = c.target_bit = e.end_bit;
	return c;
}

/*
 * Is the dynamic block whose header starts at bit `hb` one whose parses
 * do not fall in step - literal codewords of (nearly) ONE length, the
 * block a compressor writes over incompressible bytes inside a stream of
 * other data?  The host reads the header itself (the precode and the
 * literal lengths, lib/deflate_decompress.c:1227-1359 restated for the
 * first 256 symbols; a few hundred bits): returns the longest literal
 * codeword when the literals of one length fill 98 % of the code
 * space, 0 otherwise (or when the header is not a
 * valid dynamic one: the kernels say what is wrong with it).  Only the
 * plan depends on the answer, never the result.
 * `bits.peek(bit, n)`: n <= 24 bits of the raw stream, zeros past its end.
 */
template <typename Bits>
static inline uint32_t one_length_code(const Bits &bits, uint64_t raw_bits, uint64_t hb,
				       uint64_t *first_token)
{
	static const uint8_t perm[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
	uint64_t p = hb;
	if (p + 17 + 19 * 3 > raw_bits || ((bits.peek(p, 3) >> 1) & 3) != 2)
		return 0;
	const uint32_t nl = 257 + bits.peek(p + 3, 5), nd = 1 + bits.peek(p + 8, 5),
		       nc = 4 + bits.peek(p + 13, 4);
	p += 17;
	uint8_t pl[19] = { 0 };
	for (uint32_t i = 0; i < nc; i++, p += 3)
		pl[perm[i]] = (uint8_t)bits.peek(p, 3);
	uint32_t cnt[8] = { 0 }, first[8] = { 0 }, base[8] = { 0 };
	uint8_t sorted[19];
	uint32_t ns = 0;
	for (uint32_t len = 1; len < 8; len++)
		for (uint32_t sy = 0; sy < 19; sy++)
			if (pl[sy] == len) {
				sorted[ns++] = (uint8_t)sy;
				cnt[len]++;
			}
	for (uint32_t len = 1, code = 0; len < 8; len++) {
		code = (code + cnt[len - 1]) << 1;
		first[len] = code;
		base[len] = len > 1 ? base[len - 1] + cnt[len - 1] : 0;
	}
	/* (all lengths are read, the offsets' too: behind them is the block's
	 * first token, where the first of the exact starts lies) */
	uint8_t lens[320 + 138];
	uint32_t n = 0;
	const uint32_t want = nl < 256 ? nl : 256, total = nl + nd;
	/* (an ordinary block is told apart after two dozen lengths: under
	 * three quarters of the literals seen so far on one length - a stream
	 * of 1 GiB has 3600 blocks, and parsing every header in full was 2 ms
	 * of its call) */
	uint32_t seen[16] = { 0 }, nz = 0, most = 0;
	while (n < total) {
		if (n < want && nz >= 24 && 4 * most < 3 * nz)
			return 0;
		if (p + 32 > raw_bits)
			return 0;
		uint32_t c = 0, sy = 99;
		const uint32_t v7 = bits.peek(p, 7);
		for (uint32_t len = 1; len < 8; len++) {
			c = (c << 1) | ((v7 >> (len - 1)) & 1);
			if (c - first[len] < cnt[len]) {
				sy = sorted[base[len] + c - first[len]];
				p += len;
				break;
			}
		}
		if (sy < 16) {
			lens[n++] = (uint8_t)sy;
			if (sy && n <= want) {
				nz++;
				most = std::max(most, ++seen[sy]);
			}
		} else if (sy == 16) {
			if (!n)
				return 0;
			const uint32_t r = 3 + bits.peek(p, 2);
			p += 2;
			for (uint32_t k = 0; k < r; k++, n++)
				lens[n] = lens[n - 1];
			if (lens[n - 1] && n <= want) {
				nz += r;
				seen[lens[n - 1]] += r;
				most = std::max(most, seen[lens[n - 1]]);
			}
		} else if (sy == 17 || sy == 18) {
			const uint32_t r = sy == 17 ? 3 + bits.peek(p, 3) : 11 + bits.peek(p, 7);
			p += sy == 17 ? 3 : 7;
			for (uint32_t k = 0; k < r; k++)
				lens[n++] = 0;
		} else {
			return 0;
		}
	}
	uint32_t hist[16] = { 0 }, hi = 0, top = 1;
	for (uint32_t sy = 0; sy < want; sy++)
		hist[lens[sy]]++;
	for (uint32_t len = 1; len < 16; len++) {
		if (hist[len])
			hi = len;
		if (hist[len] > hist[top])
			top = len;
	}
	/* 98 % of the code space at one length.  (Two parses that are d bits
	 * apart drift by a bit where one of them meets a codeword of another
	 * length: with a share p of those they meet after ~10 / 2p tokens -
	 * at 5 % well inside the 1 KiB warm-up, which then costs a ninth of
	 * what the exact starts cost; at 0.5 % - 256 literals of 8 bits and
	 * what a compressor squeezes in beside them - in a thousand.) */
	if (n != total || p >= raw_bits)
		return 0;
	*first_token = p;
	return hist[top] >= 32 && hi <= 11 && 50 * hist[top] >= 49 * (1u << top) ? hi : 0;
}

/* the hi + 1 EXACT starts of the planned position `at`: at, at + 1, .. at + hi */
static inline void plan_exact_group(std::vector<planned> &plan, uint32_t *nexact, uint64_t at,
				    uint32_t hi, uint64_t under)
{
	for (uint32_t j = 0; j <= hi; j++) {
		planned q = {};
		q.c.kind = LDA_CHUNK_EXACT;
		q.c.hdr_bit = under;
		q.c.start_bit = q.c.target_bit = at + j;
		q.c.phases = j ? ~0u : hi + 1;
		q.at = at;
		plan.push_back(q);
		(*nexact)++;
	}
}

/* a block (or, for the carried-in state, what is left of one): its
 * first chunk, then inner chunks up to `next` */
/* (`inner`: the block's tables are known without looking - from its
 * header at first.hdr_bit, or the static codes', `under` =
 * LDA_HDR_STATIC) */
template <typename OneLength>
static inline void plan_block(std::vector<planned> &plan, uint32_t *nexact,
			      const lda_stream_chunk &first, uint64_t next, bool inner,
			      uint64_t under, uint64_t R1, uint64_t T, const OneLength &one_length)
{
	planned p = {};
	p.c = first;
	p.at = first.start_bit;
	plan.push_back(p);
	if (!inner)
		return;
	const uint64_t start = first.start_bit;
	/* a block of one codeword length (one_length_code()): no warm-up
	 * falls in step there, and a count pass that walks on such a
	 * block is slow (ten parses per piece, par_phase_starts()).  Its
	 * inner chunks are small - 2 KiB of input - and start EXACTLY,
	 * at every bit a literal that overhangs the planned start can
	 * end at: P, P + 1, .. P + longest literal codeword.  One of them
	 * is the true parse; the chain finds it by its key, in the first
	 * count pass.  (A match across P is not covered: a repair.) */
	uint64_t tok0 = 0;
	const uint32_t hi = first.kind != LDA_CHUNK_HEADER ? 0 : one_length(first.hdr_bit, &tok0);
	const uint64_t TN = STREAM_TN;
	if (hi && *nexact + ((next - start) / TN + 1) * (hi + 1) <= 65536) {
		/* (the first of them at the block's first token - the host has
		 * read the header to its end -, so that the chunk that reads
		 * the header holds no tokens: as the only chunk of the block
		 * counted alone it was the only one the decode pass had no
		 * starts for, 1.1 M cycles against 0.4.  The other positions
		 * stay where they were.) */
		const uint64_t P1 = start + TN;
		const bool more = P1 + TN / 2 <= next;
		const uint64_t lim0 = more ? P1 : next;
		if (tok0 > start && tok0 + hi + 2 < lim0 && lim0 - tok0 <= 24000)
			plan_exact_group(plan, nexact, tok0, hi, under);
		for (uint64_t P = start + TN; P + TN / 2 <= next; P += TN)
			plan_exact_group(plan, nexact, P, hi, under);
		return;
	}
	const uint64_t safe = first.kind == LDA_CHUNK_HEADER ? start + STREAM_HDRSAFE : start;
	/* (the block in equal parts of at most T: with steps of T and what
	 * is left added to the last, a block's last chunk was up to 1.5 T -
	 * and the count and decode launches last as long as their longest
	 * chunk) */
	/* (not the window's last block: a chunk that starts within T of
	 * the end of the input runs its last rounds through the
	 * sequential tail code, and one that close to the end was the
	 * slowest chunk of the count launch by a factor of two) */
	const uint64_t blen = next > start ? next - start : 0;
	const uint64_t nparts = std::max<uint64_t>(1, (blen + T - 1) / T);
	const uint64_t step = next == R1 ? T : std::max<uint64_t>(T / 2, blen / nparts);
	for (uint64_t P = start + step; P + step / 2 <= next; P += step) {
		uint64_t ws = P > STREAM_OV ? P - STREAM_OV : 0;
		if (ws < safe)
			ws = safe;
		if (ws + STREAM_OV / 4 > P)
			continue;
		planned q = {};
		q.c.kind = LDA_CHUNK_WARM;
		q.c.hdr_bit = under;
		q.c.start_bit = ws;
		q.c.target_bit = P;
		q.at = P;
		plan.push_back(q);
	}
}

/*
 * THE PLAN of one window: the chunks of [carry, R1), chunks of about T bits of
 * input, with the bit each ends at (limit_bit).  `cands`: the block starts the
 * finder accepted, sorted.  `static_at_carry`: the header bits at a carry that
 * stands at a block boundary say STATIC (whoever can read them looks).
 * one_length(hdr_bit, &first_token): one_length_code() of that header, from
 * wherever the caller has it; 0 for an ordinary block.  Returns the plan;
 * *nexact = chunks planned at exact starts (blocks of one codeword length).
 */
template <typename OneLength>
static inline std::vector<planned>
plan_window(const lda_stream_chunk &carry, const std::vector<uint64_t> &cands, uint64_t R1,
	    uint64_t T, bool static_at_carry, const OneLength &one_length, uint32_t *nexact)
{
	std::vector<planned> plan;
	plan.reserve(4096 + cands.size() * 8);
	*nexact = 0;
	/* block starts: the carried-in state, then the candidates behind
	 * it.  A block's inner chunks end at the next candidate whatever
	 * becomes of it; a small block close behind a chunk start gets no
	 * chunk of its own (the chunk in front of it walks through), so
	 * chunk starts are at least T / 8 apart however small the blocks
	 * are */
	std::vector<uint64_t> cs;
	bool carry_dynamic = carry.kind != LDA_CHUNK_HEADER;	/* inside a Huffman block */
	for (uint64_t c : cands) {
		if (c == carry.start_bit && carry.kind == LDA_CHUNK_HEADER)
			carry_dynamic = true;
		else if (c > carry.start_bit)
			cs.push_back(c);
	}
	uint64_t last_at = carry.start_bit;
	/* a STATIC block at the carried-in state (the host sees the
	 * header, or the state says so): chunks under the static
	 * codes up to the next candidate.  They stop at the block's
	 * end; what follows there is found by the chain (repairs). */
	const bool carry_static = carry.kind == LDA_CHUNK_HEADER ? !carry_dynamic && static_at_carry :
								   carry.hdr_bit == LDA_HDR_STATIC;
	plan_block(plan, nexact, carry, cs.empty() ? R1 : cs[0], carry_dynamic || carry_static,
		   carry_static ? LDA_HDR_STATIC : carry.hdr_bit, R1, T, one_length);
	for (size_t i = 0; i < cs.size(); i++) {
		const uint64_t next = i + 1 < cs.size() ? cs[i + 1] : R1;
		if (cs[i] - last_at < T / 8 && next - cs[i] < T / 2)
			continue;
		plan_block(plan, nexact, header_chunk(cs[i]), next, true, cs[i], R1, T, one_length);
		last_at = cs[i];
	}
	/* (a chunk ends at the next planned start: the starts of one planned
	 * position - see plan_block() - share theirs) */
	for (size_t i = plan.size(), nxt_at = R1; i-- > 0;) {
		if (i + 1 < plan.size() && plan[i + 1].at != plan[i].at)
			nxt_at = plan[i + 1].at;
		plan[i].c.limit_bit = nxt_at;
	}
	return plan;
}

/*
 * THE CHAIN of one window.
 * Every counted chunk is a pool entry keyed by its exact start state.
 * The walk from the window's first chunk follows end state -> start
 * state; where an end state has no chunk starting there (a block the
 * finder does not look for, a false candidate, a warm-up that did not
 * fall in step) a REPAIR chunk is counted from that state up to the
 * next planned start.  Repairs are made for every open end in the pool
 * at once, one launch per round, so the number of host round trips is
 * the longest run of consecutive breaks, not the number of breaks.
 */
struct stream_chain {
	typedef std::pair<uint64_t, uint64_t> key_t;	/* (start_bit * 2 + boundary, header) */
	/* (hashed: a window of blocks of one codeword length has ten
	 * thousand entries, and an ordered map's inserts were a third of
	 * its count phase) */
	struct key_hash {
		size_t operator()(const key_t &k) const {
			uint64_t h = k.first * 0x9E3779B97F4A7C15ull ^ (k.second + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
			return (size_t)(h ^ (h >> 29));
		}
	};
	/* The K exact starts of one planned position (phases != 0) are
	 * consecutive entries at consecutive bits: they are found by
	 * position, not through the map (four fifths of a window's
	 * entries where it has such blocks: their inserts were 0.2 ms of
	 * the 16 MiB mix's count phase). */
	struct pgroup { uint64_t P, hdr; uint32_t first, K; };

	std::vector<lda_stream_chunk> pc;	/* the pool: the planned chunks, then what was added */
	std::vector<lda_stream_res> pr;
	/* how many repairs in a row led to an entry (0: planned): a
	 * repair behind a repair reaches twice as far as the one before
	 * it - a block whose parse never falls in step (codewords of one
	 * length) is walked in a few long strides, not chunk by chunk */
	std::vector<uint8_t> depth;
	std::unordered_map<key_t, uint32_t, key_hash> by_start;
	std::vector<pgroup> groups;	/* sorted by P */
	std::vector<uint64_t> ats;	/* the planned chunks' nominal starts */
	/* phase candidates (see repairs()): planned starts that have theirs,
	 * and how many there are (they do not count as repairs for the limit) */
	std::vector<uint8_t> phased;
	uint32_t np = 0, ncand = 0, nrepairs = 0, first_open = 0;
	int round = 0;
	/* what walk() leaves */
	std::vector<uint32_t> path;
	bool closed = false;		/* the walk ended: final block, or the window's end */
	bool final_seen = false;	/* ... at the stream's final block */
	bool gf_end = false;		/* the walk's end lies in the stream's final (static) block */

	/* the planned chunks as they were counted (hc[i] = plan[i].c) and their results */
	stream_chain(const std::vector<planned> &plan, const std::vector<lda_stream_chunk> &hc,
		     const std::vector<lda_stream_res> &hr)
		: pc(hc), pr(hr), depth(plan.size(), 0), ats(plan.size()), phased(plan.size() + 1, 0),
		  np((uint32_t)plan.size())
	{
		by_start.reserve((size_t)np / 2 + 4096);
		for (uint32_t i = 0; i < np; i++)
			add(i);
		for (uint32_t i = 0; i < np; i++)
			ats[i] = plan[i].at;
	}

	key_t start_key(uint32_t i) const
	{
		if (pc[i].kind == LDA_CHUNK_HEADER)
			return key_t(pc[i].hdr_bit * 2 + 1, pc[i].hdr_bit);
		return key_t(pr[i].start_bit * 2, pc[i].hdr_bit);
	}
	key_t end_key(uint32_t i) const
	{
		const bool bnd = pr[i].flags & LDA_RES_BOUNDARY;
		return key_t(pr[i].end_bit * 2 + (bnd ? 1 : 0), bnd ? pr[i].end_bit : pr[i].end_hdr_bit);
	}
	/* pool entry i (pc[i], pr[i] are set) becomes findable */
	void add(uint32_t i)
	{
		if (pc[i].phases == ~0u)
			return;
		if (pc[i].phases) {
			const pgroup g = { pc[i].start_bit, pc[i].hdr_bit, i, pc[i].phases };
			groups.insert(std::upper_bound(groups.begin(), groups.end(), g.P,
						       [](uint64_t v, const pgroup &a) { return v < a.P; }), g);
			return;
		}
		if (pc[i].kind == LDA_CHUNK_HEADER || pr[i].status != LDA_STREAM_ERR)
			by_start.emplace(start_key(i), i);
	}
	/* the entry that starts in state k, or -1 */
	int64_t find(const key_t &k) const
	{
		const auto it = by_start.find(k);
		if (it != by_start.end())
			return it->second;
		if ((k.first & 1) || groups.empty())
			return -1;	/* (a start at a block boundary is a header chunk's) */
		const uint64_t e = k.first >> 1;
		auto g = std::upper_bound(groups.begin(), groups.end(), e,
					  [](uint64_t v, const pgroup &a) { return v < a.P; });
		if (g == groups.begin())
			return -1;
		--g;
		if (e - g->P >= g->K || g->hdr != k.second)
			return -1;
		const uint32_t idx = g->first + (uint32_t)(e - g->P);
		return pr[idx].status != LDA_STREAM_ERR ? (int64_t)idx : -1;
	}
	/* chunks planned under the static codes: not a header, not a real block */
	bool under_static(uint32_t i) const
	{
		return pc[i].kind != LDA_CHUNK_HEADER && pc[i].hdr_bit == LDA_HDR_STATIC;
	}

	/*
	 * The walk from the window's first chunk.  carry_gf: the carried-in state
	 * lies inside the stream's final (static) block.  whole: the window holds
	 * the stream's end.  stored_run(bit, chunks, results): the run of stored
	 * blocks at the block boundary `bit`, as chunks whose results are known
	 * (nothing appended: none there).  Returns WHY_OK - `closed` says whether
	 * the walk ended or stands at an open end, path.back() - or why the
	 * stream is not this path's.
	 */
	template <typename StoredRun>
	int walk(bool carry_gf, bool whole, uint64_t R1, const StoredRun &stored_run)
	{
		path.clear();
		uint32_t cur = 0;
		bool gf = carry_gf;
		for (;;) {
			if (pr[cur].status == LDA_STREAM_ERR) {
				if (whole)
					return WHY_ERRCHUNK;
				closed = true;	/* (it may only have run out of window) */
				break;
			}
			path.push_back(cur);
			if (pr[cur].status == LDA_STREAM_FINAL) {
				closed = final_seen = true;
				break;
			}
			/* is the block the walk stands in the stream's last?  A
			 * chunk that read the header says so itself; one under
			 * the static codes inherits it - and when it stopped at
			 * its block's end, that was the end of the stream */
			const bool bnd_end = pr[cur].flags & LDA_RES_BOUNDARY;
			if (!under_static(cur))
				gf = pr[cur].flags & LDA_RES_GOV_FINAL;
			else if (bnd_end && gf) {
				/* (its status stays OK: that is what the decode
				 * pass will report for it too) */
				closed = final_seen = true;
				break;
			}
			if (bnd_end)
				gf = false;
			gf_end = gf;
			if (pr[cur].end_bit >= R1 || path.size() > pc.size()) {
				if (whole)
					return WHY_NOFINAL;	/* ran out of input without a final block */
				closed = true;
				break;
			}
			int64_t nxt = find(end_key(cur));
			if (nxt < 0 && bnd_end) {
				/* a run of stored blocks behind this boundary: the
				 * host's (no count pass, no round trip) */
				std::vector<lda_stream_chunk> oc;
				std::vector<lda_stream_res> orr;
				stored_run(pr[cur].end_bit, oc, orr);
				for (size_t k = 0; k < oc.size(); k++) {
					pc.push_back(oc[k]);
					pr.push_back(orr[k]);
					depth.push_back(0);
					add((uint32_t)pc.size() - 1);
				}
				nxt = find(end_key(cur));
			}
			if (nxt < 0)
				break;
			cur = (uint32_t)nxt;
		}
		return WHY_OK;
	}

	/*
	 * Repairs for every open end (entries added in earlier rounds were looked
	 * at then: start at first_open), and the phase candidates that go with
	 * them: rc[] with rdepth[].  Returns WHY_OK, WHY_CHAIN when there is
	 * nothing to ask, WHY_REPAIRS past the limit of 64 + 2 np repairs.
	 */
	int repairs(uint64_t R1, std::vector<lda_stream_chunk> &rc, std::vector<uint8_t> &rdepth)
	{
		rc.clear();
		rdepth.clear();
		const uint32_t max_repairs = 64 + 2 * np;
		const uint32_t npool = (uint32_t)pc.size();
		std::unordered_map<key_t, int, key_hash> asked;
		for (uint32_t i = first_open; i < npool; i++) {
			if (pr[i].status != LDA_STREAM_OK || pr[i].end_bit >= R1)
				continue;
			const key_t k = end_key(i);
			if (find(k) >= 0 || asked.count(k))
				continue;
			asked[k] = 1;
			const bool bnd = pr[i].flags & LDA_RES_BOUNDARY;
			lda_stream_chunk c = carry_from(pr[i]);
			/* up to the next planned start - or, behind a repair,
			 * twice as many planned starts further than that one */
			const uint32_t dp = std::min<uint32_t>((uint32_t)depth[i] + 1, 12);
			size_t nx = (size_t)(std::upper_bound(ats.begin(), ats.end(), pr[i].end_bit) -
					     ats.begin());
			const size_t nx0 = nx;	/* the next planned start behind this end */
			nx += ((size_t)1 << (dp - 1)) - 1;
			c.limit_bit = nx >= ats.size() ? R1 : ats[nx];
			rc.push_back(c);
			rdepth.push_back((uint8_t)dp);
			/* PHASE CANDIDATES.  The planned chunk q that should have
			 * gone on from this end did not (its warm-up ended on
			 * another token boundary) - and its own end is open too
			 * or it failed (a parse out of step meets an end-of-block
			 * codeword sooner or later and reads a header that is
			 * none): a code whose parses do not fall in step
			 * (codewords of nearly one length: a dynamic block over
			 * incompressible bytes).  Repairs alone would walk
			 * such a block one stride per round trip.  But the end of
			 * whatever comes to the next planned start P from the
			 * true parse is the first token boundary at or behind P:
			 * a literal's codeword is at most a dozen bits, so one of
			 * the chunks that start EXACTLY at P, P + 1, .. P + K - 1
			 * is the true parse, and the chain finds it by its key.
			 * Every open end of the block asks for the K starts at
			 * its own next planned start, in this same round. */
			const size_t nq = nx0 ? nx0 - 1 : 0;
			if (!bnd && i < np && nx0 >= 1 && nx0 < np && nq != i && nq < np &&
			    pc[nq].kind == LDA_CHUNK_WARM &&
			    pc[nq].hdr_bit == pr[i].end_hdr_bit &&
			    (pr[nq].status != LDA_STREAM_OK ||
			     find(end_key((uint32_t)nq)) < 0) &&
			    pc[nx0].kind == LDA_CHUNK_WARM &&
			    pc[nx0].hdr_bit == pr[i].end_hdr_bit && !phased[nx0] &&
			    ncand + STREAM_PHASES <= 4096) {
				phased[nx0] = 1;
				const uint64_t lim2 = nx0 + 1 < np ? ats[nx0 + 1] : R1;
				/* (one wave for all of them when they are one round
				 * of input: phase_count() of inflate_stream.hip) */
				const bool together = pr[i].end_hdr_bit != LDA_HDR_STATIC &&
						      lim2 > ats[nx0] + STREAM_PHASES &&
						      lim2 - ats[nx0] <= 24000;
				for (uint32_t j = 0; j < STREAM_PHASES && ats[nx0] + j < lim2; j++) {
					lda_stream_chunk k2 = {};
					k2.kind = LDA_CHUNK_EXACT;
					k2.hdr_bit = pr[i].end_hdr_bit;
					k2.start_bit = k2.target_bit = ats[nx0] + j;
					k2.limit_bit = lim2;
					k2.phases = !together ? 0 : j ? ~0u : STREAM_PHASES;
					rc.push_back(k2);
					rdepth.push_back(0);
					ncand++;
				}
			}
		}
		/* the open end of the walk is always among them (round 0 looks at
		 * all entries; later rounds at the new ones, and the walk can only
		 * have stopped at a new one) */
		first_open = npool;
		nrepairs += (uint32_t)rc.size();
		if (rc.empty())
			return WHY_CHAIN;
		return nrepairs > max_repairs + ncand ? WHY_REPAIRS : WHY_OK;
	}

	/* the counted repairs join the pool */
	void accept(const std::vector<lda_stream_chunk> &rc, const std::vector<uint8_t> &rdepth,
		    const std::vector<lda_stream_res> &rr)
	{
		const uint32_t npool = (uint32_t)pc.size(), nr = (uint32_t)rc.size();
		for (uint32_t i = 0; i < nr; i++) {
			pc.push_back(rc[i]);
			pr.push_back(rr[i]);
			depth.push_back(rdepth[i]);
		}
		for (uint32_t i = 0; i < nr; i++)
			add(npool + i);
	}

	/*
	 * Walk, ask, count, accept - up to 16 rounds, until the walk ends.
	 * count(rc, rr): the count pass over rc[] into rr[]; false = it failed.
	 * *asked grows by the chunks handed to count() or refused for their
	 * number.  Returns WHY_OK with `closed` set, or why not.
	 */
	template <typename StoredRun, typename Count>
	int close(bool carry_gf, bool whole, uint64_t R1, const StoredRun &stored_run,
		  const Count &count, uint64_t *asked)
	{
		std::vector<lda_stream_chunk> rc;
		std::vector<uint8_t> rdepth;
		std::vector<lda_stream_res> rr;
		for (round = 0; round < 16; round++) {
			int why = walk(carry_gf, whole, R1, stored_run);
			if (why != WHY_OK)
				return why;
			if (closed)
				return WHY_OK;
			why = repairs(R1, rc, rdepth);
			*asked += rc.size();
			if (why != WHY_OK)
				return why;
			rr.assign(rc.size(), lda_stream_res());
			if (!count(rc, rr))
				return WHY_DEVICE;
			accept(rc, rdepth, rr);
		}
		return WHY_CHAIN;
	}
};

} /* namespace lda */

#endif /* LDA_STREAM_PLAN_H */
