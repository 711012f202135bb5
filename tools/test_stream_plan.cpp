/*
 * test_stream_plan.cpp - the host arithmetic of the many-wave single-stream
 * decoder (libdeflate_amd/csrc/stream_plan.h): the planner, the chain and
 * one_length_code(), without a device.  The chain is driven by a MODEL in
 * place of the count kernel: a model stream is a sorted list of token
 * boundaries with the block each lies in and the bytes produced up to it.
 * Stand-alone:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_stream_plan tools/test_stream_plan.cpp && ./test_stream_plan
 *
 * (tests/test_stream_plan.py does exactly that.)
 */
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <random>
#include <set>

#include "stored_rows.h"
#include "stream_plan.h"

using namespace lda;

static int g_fail = 0;
#define CHECK(cond)                                                              \
	do {                                                                     \
		if (!(cond)) {                                                   \
			printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			if (++g_fail > 20)                                       \
				exit(1);                                         \
		}                                                                \
	} while (0)

/* ------------------------------------------------------------------ model */

struct mblock {
	uint64_t hdr, end;	/* first bit of the header, bit behind the block */
	bool is_static, is_final, is_stored;
};
struct mpos {
	uint64_t bit, out;
	uint32_t block;		/* the block the position lies in (a block's first bit: that block) */
};

struct model {
	std::vector<mblock> blocks;
	std::vector<mpos> pos;	/* sorted: every block's first bit and every token boundary in it */
	uint64_t end_bit = 0, total = 0;
	/* scripts: a WARM chunk with this target lands there (0: ERR) */
	std::map<uint64_t, uint64_t> warm_script;
	std::set<uint64_t> bad_headers;	/* a HEADER chunk here is ERR */
	std::set<uint64_t> bad_exact;	/* an EXACT chunk here is ERR */

	/* a block of ntok tokens `spacing` bits apart, `bytes` of output each,
	 * behind a header of hdr_bits */
	void add(bool is_static, bool is_final, uint64_t hdr_bits, uint64_t ntok, uint64_t spacing,
		 uint64_t bytes, bool is_stored = false)
	{
		const uint32_t b = (uint32_t)blocks.size();
		mblock blk = { end_bit, 0, is_static, is_final, is_stored };
		pos.push_back({ end_bit, total, b });
		uint64_t p = end_bit + hdr_bits;
		for (uint64_t k = 0; k < ntok; k++) {
			pos.push_back({ p, total, b });
			p += spacing;
			total += bytes;
		}
		blk.end = end_bit = p;
		blocks.push_back(blk);
	}
	size_t at_or_behind(uint64_t bit) const
	{
		return (size_t)(std::lower_bound(pos.begin(), pos.end(), bit,
						 [](const mpos &a, uint64_t v) { return a.bit < v; }) -
				pos.begin());
	}
	bool is_block_start(size_t i) const { return i < pos.size() && blocks[pos[i].block].hdr == pos[i].bit; }
	uint64_t gov(size_t i) const
	{
		const mblock &b = blocks[pos[i].block];
		return is_block_start(i) ? pos[i].bit : b.is_static ? LDA_HDR_STATIC : b.hdr;
	}

	/* the count kernel's answer for one chunk */
	lda_stream_res count(const lda_stream_chunk &c) const
	{
		lda_stream_res r = {};
		r.status = LDA_STREAM_ERR;
		size_t i;
		const bool blind = c.kind != LDA_CHUNK_HEADER && c.hdr_bit == LDA_HDR_STATIC;
		if (c.kind == LDA_CHUNK_HEADER) {
			i = at_or_behind(c.start_bit);
			if (i == pos.size() || pos[i].bit != c.start_bit || !is_block_start(i) ||
			    bad_headers.count(c.start_bit))
				return r;
		} else if (c.kind == LDA_CHUNK_EXACT) {
			i = at_or_behind(c.start_bit);
			if (i == pos.size() || pos[i].bit != c.start_bit || is_block_start(i) ||
			    gov(i) != c.hdr_bit || bad_exact.count(c.start_bit))
				return r;
		} else {
			uint64_t land = c.target_bit;
			const auto s = warm_script.find(c.target_bit);
			if (s != warm_script.end()) {
				if (!s->second)
					return r;
				land = s->second;
			}
			i = at_or_behind(land);
			if (i < pos.size() && is_block_start(i))
				i++;	/* (a start inside a block is a token boundary) */
			if (i >= pos.size() || gov(i) != c.hdr_bit)
				return r;
		}
		r.start_bit = pos[i].bit;
		const uint64_t out0 = pos[i].out;
		const uint32_t b0 = pos[i].block;
		/* to the first boundary at or behind the limit; a chunk under the
		 * static codes stops at its block's end whatever the limit */
		size_t j = i;
		bool read_hdr = c.kind == LDA_CHUNK_HEADER;
		uint32_t hdr_of = b0;	/* the last block whose header the chunk read */
		for (;;) {
			if (j > i && is_block_start(j)) {
				if (blind)
					break;
				read_hdr = true;
				hdr_of = pos[j].block;
			}
			if (pos[j].bit >= c.limit_bit && !(j == i && is_block_start(j)))
				break;
			if (j + 1 == pos.size()) {
				/* the last token of the last block: the stream's end */
				const mblock &lb = blocks[pos[j].block];
				if (blind) {
					r.end_bit = r.end_hdr_bit = lb.end;
					r.nout = total - out0;
					r.status = LDA_STREAM_OK;
					r.flags = LDA_RES_BOUNDARY;
					return r;
				}
				if (!lb.is_final)
					return r;	/* ran out of input */
				r.end_bit = r.end_hdr_bit = lb.end;
				r.nout = total - out0;
				r.status = LDA_STREAM_FINAL;
				r.flags = LDA_RES_BOUNDARY;
				return r;
			}
			j++;
		}
		r.end_bit = pos[j].bit;
		r.nout = pos[j].out - out0;
		r.status = LDA_STREAM_OK;
		if (is_block_start(j)) {
			r.end_hdr_bit = r.end_bit;
			r.flags = LDA_RES_BOUNDARY;
		} else {
			r.end_hdr_bit = gov(j);
			if (read_hdr && hdr_of == pos[j].block && blocks[hdr_of].is_final)
				r.flags |= LDA_RES_GOV_FINAL;
		}
		return r;
	}
	std::vector<lda_stream_res> count(const std::vector<lda_stream_chunk> &cs) const
	{
		std::vector<lda_stream_res> rs;
		for (const lda_stream_chunk &c : cs)
			rs.push_back(count(c));
		return rs;
	}
	/* the host's walk over a run of stored blocks, as host_stream.hip binds it */
	void stored_run(uint64_t bit, std::vector<lda_stream_chunk> &oc, std::vector<lda_stream_res> &orr) const
	{
		for (const mblock &b : blocks) {
			if (b.hdr != bit || !b.is_stored)
				continue;
			lda_stream_chunk c = header_chunk(bit);
			c.limit_bit = b.end;
			lda_stream_res r = {};
			r.start_bit = bit;
			r.end_bit = r.end_hdr_bit = b.end;
			r.nout = (at_or_behind(b.end) < pos.size() ? pos[at_or_behind(b.end)].out : total) -
				 pos[at_or_behind(bit)].out;
			r.status = b.is_final ? LDA_STREAM_FINAL : LDA_STREAM_OK;
			r.flags = LDA_RES_BOUNDARY;
			oc.push_back(c);
			orr.push_back(r);
			bit = b.end;
		}
	}
};

static uint32_t ordinary(uint64_t, uint64_t *) { return 0; }

/* plan a whole model stream (every dynamic block a candidate), count it, chain it */
struct driven {
	std::vector<planned> plan;
	std::vector<lda_stream_chunk> hc;
	std::vector<lda_stream_res> hr;
	int rounds = 0, stored_asked = 0;
	std::vector<std::vector<lda_stream_chunk>> asked;	/* what each round's count got */
	uint64_t nasked = 0;
};

static std::vector<uint64_t> dynamic_headers(const model &m)
{
	std::vector<uint64_t> cands;
	for (const mblock &b : m.blocks)
		if (!b.is_static && !b.is_stored)
			cands.push_back(b.hdr);
	return cands;
}

static void count_plan(const model &m, driven &dr)
{
	dr.hc.clear();
	for (const planned &p : dr.plan)
		dr.hc.push_back(p.c);
	dr.hr = m.count(dr.hc);
}

static int close_chain(const model &m, driven &dr, stream_chain &ch, bool carry_gf, bool whole, uint64_t R1)
{
	return ch.close(
		carry_gf, whole, R1,
		[&](uint64_t bit, std::vector<lda_stream_chunk> &oc, std::vector<lda_stream_res> &orr) {
			dr.stored_asked++;
			m.stored_run(bit, oc, orr);
		},
		[&](std::vector<lda_stream_chunk> &rc, std::vector<lda_stream_res> &rr) {
			dr.rounds++;
			dr.asked.push_back(rc);
			rr = m.count(rc);
			return true;
		},
		&dr.nasked);
}

/* the accepted path: contiguous from the first chunk on, and its bytes */
static uint64_t check_path(const stream_chain &ch, uint64_t from_bit)
{
	uint64_t nout = 0;
	CHECK(!ch.path.empty());
	for (size_t k = 0; k < ch.path.size(); k++) {
		const uint32_t i = ch.path[k];
		CHECK(ch.pr[i].status != LDA_STREAM_ERR);
		CHECK(ch.pr[i].start_bit == (k ? ch.pr[ch.path[k - 1]].end_bit : from_bit));
		if (k) {
			const lda_stream_chunk want = carry_from(ch.pr[ch.path[k - 1]]);
			CHECK(want.kind == LDA_CHUNK_HEADER ? ch.pc[i].kind == LDA_CHUNK_HEADER :
							      ch.pc[i].kind != LDA_CHUNK_HEADER &&
								      ch.pc[i].hdr_bit == want.hdr_bit);
		}
		nout += ch.pr[i].nout;
	}
	return nout;
}

/* three dynamic blocks, tokens 11 bits apart */
static model three_blocks()
{
	model m;
	m.add(false, false, 300, 6000, 11, 3);
	m.add(false, false, 411, 7000, 11, 2);
	m.add(false, true, 250, 5000, 11, 1);
	return m;
}

static void test_in_step()
{
	const model m = three_blocks();
	driven dr;
	uint32_t nexact = 0;
	dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, false, ordinary, &nexact);
	CHECK(nexact == 0 && dr.plan.size() > 8);
	count_plan(m, dr);
	stream_chain ch(dr.plan, dr.hc, dr.hr);
	CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_OK);
	CHECK(ch.closed && ch.final_seen && dr.rounds == 0 && dr.nasked == 0);
	CHECK(ch.path.size() == dr.plan.size());
	CHECK(check_path(ch, 0) == m.total);
	CHECK(ch.pr[ch.path.back()].status == LDA_STREAM_FINAL && ch.pr[ch.path.back()].end_bit == m.end_bit);
}

static void test_one_repair(bool err)
{
	model m = three_blocks();
	driven dr;
	uint32_t nexact = 0;
	dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, false, ordinary, &nexact);
	/* the third planned chunk is a warm-up inside block 0 */
	const size_t q = 2;
	CHECK(dr.plan[q].c.kind == LDA_CHUNK_WARM && dr.plan[q + 1].c.kind == LDA_CHUNK_WARM);
	const uint64_t P = dr.plan[q].c.target_bit;
	m.warm_script[P] = err ? 0 : m.pos[m.at_or_behind(P) + 2].bit;
	count_plan(m, dr);
	stream_chain ch(dr.plan, dr.hc, dr.hr);
	CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_OK);
	CHECK(ch.closed && ch.final_seen && dr.rounds == 1);
	const lda_stream_chunk &r = dr.asked[0][0];
	CHECK(r.kind == LDA_CHUNK_EXACT && r.hdr_bit == 0);
	CHECK(r.start_bit == dr.hr[q - 1].end_bit && r.start_bit == m.pos[m.at_or_behind(P)].bit);
	CHECK(r.limit_bit == dr.plan[q + 1].at);
	/* (a failed chunk in front of a warm-up also asks for that one's phases;
	 * one that only landed elsewhere goes on itself: nothing more to ask) */
	CHECK(dr.asked[0].size() == (err ? 1 + STREAM_PHASES : 1));
	CHECK(check_path(ch, 0) == m.total);
	CHECK(ch.path.size() == dr.plan.size());	/* the repair stands where q stood */
}

/* one block, tokens 40 bits apart from bit 200; planned starts at 1 mod 40, so
 * that no phase candidate (P .. P + 9) is a token boundary */
static void test_doubling()
{
	model m;
	m.add(false, true, 200, 5000, 40, 4);
	driven dr;
	const uint32_t NP = 11;
	for (uint32_t k = 0; k < NP; k++) {
		planned p = {};
		if (k == 0) {
			p.c = header_chunk(0);
		} else {
			p.c.kind = LDA_CHUNK_WARM;
			p.c.hdr_bit = 0;
			p.c.target_bit = 16001 + 16000 * (uint64_t)(k - 1);
			p.c.start_bit = p.c.target_bit - 8000;
		}
		p.at = p.c.target_bit;
		dr.plan.push_back(p);
	}
	for (uint32_t k = 0; k < NP; k++)
		dr.plan[k].c.limit_bit = k + 1 < NP ? dr.plan[k + 1].at : m.end_bit;
	for (uint32_t k = 1; k <= 4; k++)	/* four breaks in a row */
		m.warm_script[dr.plan[k].at] = 0;
	count_plan(m, dr);
	stream_chain ch(dr.plan, dr.hc, dr.hr);
	CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_OK);
	CHECK(ch.closed && ch.final_seen);
	/* strides of 1, 2 and 4 planned starts: three round trips for four breaks */
	CHECK(dr.rounds == 3);
	CHECK(dr.asked[0][0].limit_bit == dr.plan[2].at);
	CHECK(dr.asked[1].size() == 1 && dr.asked[1][0].limit_bit == dr.plan[4].at);
	CHECK(dr.asked[2].size() == 1 && dr.asked[2][0].limit_bit == dr.plan[8].at);
	CHECK(dr.asked[1][0].start_bit >= dr.plan[2].at && dr.asked[2][0].start_bit >= dr.plan[4].at);
	CHECK(check_path(ch, 0) == m.total);
	/* the depth is capped at 12: 2^11 planned starts further, however deep */
	{
		std::vector<planned> plan(5000);
		for (size_t k = 0; k < plan.size(); k++) {
			plan[k].c = k ? lda_stream_chunk() : header_chunk(0);
			plan[k].c.kind = k ? LDA_CHUNK_WARM : LDA_CHUNK_HEADER;
			plan[k].at = plan[k].c.target_bit = 1000 * k;
		}
		std::vector<lda_stream_chunk> hc;
		for (const planned &p : plan)
			hc.push_back(p.c);
		std::vector<lda_stream_res> hr(plan.size());
		for (lda_stream_res &r : hr)
			r.status = LDA_STREAM_ERR;
		for (unsigned deep : { 11u, 12u, 200u }) {
			stream_chain c2(plan, hc, hr);
			lda_stream_res e = {};
			e.start_bit = 10;
			e.end_bit = 1500;	/* the next planned start behind it: index 2 */
			e.end_hdr_bit = 0;
			lda_stream_chunk c = {};
			c.kind = LDA_CHUNK_EXACT;
			c.start_bit = c.target_bit = 10;
			c2.first_open = (uint32_t)c2.pc.size();
			c2.accept({ c }, { (uint8_t)deep }, { e });
			std::vector<lda_stream_chunk> rc;
			std::vector<uint8_t> rd;
			CHECK(c2.repairs(5000000, rc, rd) == WHY_OK && rc.size() == 1);
			CHECK(rd[0] == 12);
			CHECK(rc[0].limit_bit == plan[2 + 2047].at);
		}
	}
}

static void test_phase_group()
{
	const uint32_t K = 9;
	const uint64_t P = 20000;
	std::vector<planned> plan(1 + K);
	plan[0].c = header_chunk(0);
	plan[0].c.limit_bit = P;
	for (uint32_t j = 0; j < K; j++) {
		planned &q = plan[1 + j];
		q.c.kind = LDA_CHUNK_EXACT;
		q.c.hdr_bit = 0;
		q.c.start_bit = q.c.target_bit = P + j;
		q.c.phases = j ? ~0u : K;
		q.c.limit_bit = 40000;
		q.at = P;
	}
	std::vector<lda_stream_chunk> hc;
	for (const planned &p : plan)
		hc.push_back(p.c);
	std::vector<lda_stream_res> hr(plan.size());
	for (uint32_t j = 0; j < K; j++) {
		hr[1 + j].start_bit = P + j;
		hr[1 + j].end_bit = 40000 + j;
		hr[1 + j].status = j == 5 ? LDA_STREAM_ERR : LDA_STREAM_OK;
	}
	hr[0].end_bit = P + 3;
	stream_chain ch(plan, hc, hr);
	CHECK(ch.by_start.size() == 1 && ch.groups.size() == 1);	/* by position, never through the map */
	typedef stream_chain::key_t key_t;
	for (uint32_t j = 0; j < K; j++)
		CHECK(ch.find(key_t((P + j) * 2, 0)) == (j == 5 ? -1 : (int64_t)(1 + j)));
	CHECK(ch.find(ch.end_key(0)) == 4);
	CHECK(ch.find(key_t((P + 3) * 2, 77)) == -1);		/* another header */
	CHECK(ch.find(key_t((P + 3) * 2, LDA_HDR_STATIC)) == -1);
	CHECK(ch.find(key_t((P + K) * 2, 0)) == -1);		/* an offset >= K */
	CHECK(ch.find(key_t((P - 1) * 2, 0)) == -1);
	CHECK(ch.find(key_t((P + 3) * 2 + 1, 0)) == -1);	/* a block boundary is a header chunk's */
}

/* planned warm-ups every 16000 bits that all run out of step */
static void phase_plan(uint32_t np, std::vector<planned> &plan, std::vector<lda_stream_chunk> &hc,
		       std::vector<lda_stream_res> &hr, uint64_t step)
{
	plan.assign(np, planned());
	for (uint32_t k = 0; k < np; k++) {
		plan[k].c = k ? lda_stream_chunk() : header_chunk(0);
		plan[k].c.kind = k ? LDA_CHUNK_WARM : LDA_CHUNK_HEADER;
		plan[k].at = plan[k].c.target_bit = step * k;
		plan[k].c.limit_bit = step * (k + 1);
	}
	hc.clear();
	for (const planned &p : plan)
		hc.push_back(p.c);
	hr.assign(np, lda_stream_res());
	for (uint32_t k = 0; k < np; k++) {
		hr[k].start_bit = step * k + (k ? 2 : 0);
		hr[k].end_bit = step * (k + 1) + 1;	/* chunk k + 1 started one bit behind it */
		hr[k].end_hdr_bit = 0;
		hr[k].status = LDA_STREAM_OK;
	}
}

static void test_phase_candidates()
{
	std::vector<planned> plan;
	std::vector<lda_stream_chunk> hc, rc;
	std::vector<lda_stream_res> hr;
	std::vector<uint8_t> rd;
	for (uint64_t step : { (uint64_t)16000, (uint64_t)24000, (uint64_t)24001 }) {
		/* chunk 0 ends in front of chunk 2's start; chunk 1 failed; so does a
		 * second open end (chunk 3's, scripted into the same stretch) */
		phase_plan(6, plan, hc, hr, step);
		const uint64_t R1 = step * 6;
		hr[0].end_bit = step + 5;
		hr[1].status = LDA_STREAM_ERR;
		hr[3].end_bit = step + 7;
		for (uint32_t k = 2; k < 6; k++)
			if (k != 3)
				hr[k].end_bit = R1;	/* nothing open behind them */
		stream_chain ch(plan, hc, hr);
		CHECK(ch.repairs(R1, rc, rd) == WHY_OK);
		/* two repairs, and the ten starts at chunk 2's position ONCE */
		CHECK(rc.size() == 2 + STREAM_PHASES && ch.ncand == STREAM_PHASES && ch.phased[2] == 1);
		CHECK(rc[0].kind == LDA_CHUNK_EXACT && rc[0].start_bit == step + 5 && rd[0] == 1);
		const bool together = step <= 24000;
		for (uint32_t j = 0; j < STREAM_PHASES; j++) {
			const lda_stream_chunk &k2 = rc[1 + j];
			CHECK(k2.kind == LDA_CHUNK_EXACT && k2.hdr_bit == 0 && k2.start_bit == 2 * step + j &&
			      k2.target_bit == k2.start_bit && k2.limit_bit == 3 * step && rd[1 + j] == 0);
			CHECK(k2.phases == (!together ? 0 : j ? ~0u : STREAM_PHASES));
		}
		CHECK(rc[1 + STREAM_PHASES].start_bit == step + 7);
		/* under the static codes they are never counted together */
		for (lda_stream_chunk &c : hc)
			if (c.kind == LDA_CHUNK_WARM)
				c.hdr_bit = LDA_HDR_STATIC;
		for (lda_stream_res &r : hr)
			r.end_hdr_bit = LDA_HDR_STATIC;
		stream_chain cs(plan, hc, hr);
		CHECK(cs.repairs(R1, rc, rd) == WHY_OK && rc.size() == 2 + STREAM_PHASES);
		CHECK(rc[1].phases == 0 && rc[2].phases == 0);
	}
	/* every planned chunk out of step: phase candidates up to 4096, not beyond */
	phase_plan(500, plan, hc, hr, 16000);
	stream_chain ch(plan, hc, hr);
	CHECK(ch.repairs(16000 * 500, rc, rd) == WHY_OK);
	CHECK(ch.ncand == 4090 && ch.ncand + STREAM_PHASES > 4096);
	CHECK(rc.size() == 499 + 4090);		/* (the last chunk ends at R1: not open) */
}

static void test_under_static()
{
	/* one static block, the stream's last: the chunks under the static codes
	 * inherit "final" from the chunk that read the header */
	{
		model m;
		m.add(true, true, 3, 6000, 9, 2);
		driven dr;
		uint32_t nexact = 0;
		dr.plan = plan_window(header_chunk(0), {}, m.end_bit, 16384, true, ordinary, &nexact);
		CHECK(dr.plan.size() > 2 && dr.plan[1].c.hdr_bit == LDA_HDR_STATIC);
		/* (a partial window would not stop them at R1: make the last one stop
		 * at its block's end by looking only that far) */
		count_plan(m, dr);
		CHECK(dr.hr[0].flags & LDA_RES_GOV_FINAL);
		CHECK(dr.hr.back().status == LDA_STREAM_OK && (dr.hr.back().flags & LDA_RES_BOUNDARY));
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(m, dr, ch, false, true, m.end_bit + 64) == WHY_OK);
		CHECK(ch.closed && ch.final_seen && dr.rounds == 0);
		CHECK(ch.pr[ch.path.back()].status == LDA_STREAM_OK);
		CHECK(check_path(ch, 0) == m.total);
		/* carried in: the flag comes with the carry */
		std::vector<planned> tail(dr.plan.begin() + 2, dr.plan.end());
		std::vector<lda_stream_chunk> hc(dr.hc.begin() + 2, dr.hc.end());
		std::vector<lda_stream_res> hr(dr.hr.begin() + 2, dr.hr.end());
		stream_chain with(tail, hc, hr), without(tail, hc, hr);
		CHECK(close_chain(m, dr, with, true, true, m.end_bit + 64) == WHY_OK && with.final_seen);
		/* without it the boundary is a block's end like any other: the walk
		 * goes on, and there is nothing there */
		CHECK(close_chain(m, dr, without, false, true, m.end_bit + 64) != WHY_OK || !without.final_seen);
	}
	/* a static block that is not the last, a dynamic block behind it */
	{
		model m;
		m.add(true, false, 3, 6000, 9, 2);
		m.add(false, true, 300, 3000, 11, 1);
		driven dr;
		uint32_t nexact = 0;
		dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, true, ordinary, &nexact);
		count_plan(m, dr);
		CHECK(!(dr.hr[0].flags & LDA_RES_GOV_FINAL));
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_OK);
		CHECK(ch.closed && ch.final_seen && dr.rounds == 0);
		CHECK(ch.pr[ch.path.back()].status == LDA_STREAM_FINAL);
		CHECK(check_path(ch, 0) == m.total);
		/* the window ends inside the static block of a stream that ends
		 * with it: gf_end goes to the next window's carry */
		model m2;
		m2.add(true, true, 3, 6000, 9, 2);
		driven d2;
		const uint64_t R1 = 30000;
		d2.plan = plan_window(header_chunk(0), {}, R1, 16384, true, ordinary, &nexact);
		count_plan(m2, d2);
		stream_chain c2(d2.plan, d2.hc, d2.hr);
		CHECK(close_chain(m2, d2, c2, false, false, R1) == WHY_OK);
		CHECK(c2.closed && !c2.final_seen && c2.gf_end);
		const lda_stream_chunk carry = carry_from(c2.pr[c2.path.back()]);
		CHECK(carry.kind == LDA_CHUNK_EXACT && carry.hdr_bit == LDA_HDR_STATIC && carry.start_bit >= R1);
	}
}

static void test_walk_ends()
{
	/* the second block's header is invalid */
	model m = three_blocks();
	m.bad_headers.insert(m.blocks[1].hdr);
	driven dr;
	uint32_t nexact = 0;
	dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, false, ordinary, &nexact);
	count_plan(m, dr);
	{
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_ERRCHUNK);
	}
	{
		/* a partial window: it may only have run out of window - closed, and
		 * the carry is the last accepted chunk's end */
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(m, dr, ch, false, false, m.end_bit) == WHY_OK);
		CHECK(ch.closed && !ch.final_seen && !ch.path.empty());
		const lda_stream_chunk carry = carry_from(ch.pr[ch.path.back()]);
		CHECK(carry.kind == LDA_CHUNK_HEADER && carry.start_bit == m.blocks[1].hdr &&
		      carry.hdr_bit == carry.start_bit && carry.target_bit == carry.start_bit);
		check_path(ch, 0);
	}
	/* the walk reaches R1 and there was no final block */
	const model g = three_blocks();
	const uint64_t R1 = g.blocks[2].hdr + 20000;
	dr.plan = plan_window(header_chunk(0), dynamic_headers(g), R1, 16384, false, ordinary, &nexact);
	count_plan(g, dr);
	{
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(g, dr, ch, false, true, R1) == WHY_NOFINAL);
		stream_chain part(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(g, dr, part, false, false, R1) == WHY_OK);
		CHECK(part.closed && !part.final_seen && part.pr[part.path.back()].end_bit >= R1);
		const lda_stream_chunk carry = carry_from(part.pr[part.path.back()]);
		CHECK(carry.kind == LDA_CHUNK_EXACT && carry.hdr_bit == g.blocks[2].hdr);
	}
}

static void test_stored_run()
{
	/* static block, two stored blocks, dynamic final block: the chunk under
	 * the static codes stops at a boundary where no counted chunk starts */
	model m;
	m.add(true, false, 3, 6000, 9, 2);
	m.add(false, false, 35, 1, 8 * 1000, 1000, true);
	m.add(false, false, 35, 1, 8 * 500, 500, true);
	m.add(false, true, 300, 3000, 11, 1);
	driven dr;
	uint32_t nexact = 0;
	dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, true, ordinary, &nexact);
	count_plan(m, dr);
	stream_chain ch(dr.plan, dr.hc, dr.hr);
	const size_t pool0 = ch.pc.size();
	CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_OK);
	CHECK(ch.closed && ch.final_seen && dr.rounds == 0 && dr.stored_asked == 1);
	CHECK(ch.pc.size() == pool0 + 2 && ch.depth.size() == ch.pc.size());
	CHECK(ch.path.size() == dr.plan.size() + 2);
	CHECK(check_path(ch, 0) == m.total);
}

static void test_refusals()
{
	/* the only repair fails: nothing left to ask */
	{
		model m = three_blocks();
		driven dr;
		uint32_t nexact = 0;
		dr.plan = plan_window(header_chunk(0), dynamic_headers(m), m.end_bit, 16384, false, ordinary, &nexact);
		const uint64_t P = dr.plan[2].c.target_bit;
		m.warm_script[P] = m.pos[m.at_or_behind(P) + 2].bit;
		m.bad_exact.insert(m.pos[m.at_or_behind(P)].bit);
		count_plan(m, dr);
		stream_chain ch(dr.plan, dr.hc, dr.hr);
		CHECK(close_chain(m, dr, ch, false, true, m.end_bit) == WHY_CHAIN);
		CHECK(dr.rounds == 1 && !ch.closed);
	}
	/* every repair ends at a new open end */
	std::vector<planned> plan;
	std::vector<lda_stream_chunk> hc;
	std::vector<lda_stream_res> hr;
	auto open_again = [](std::vector<lda_stream_chunk> &rc, std::vector<lda_stream_res> &rr) {
		for (size_t i = 0; i < rc.size(); i++) {
			rr[i] = lda_stream_res();
			rr[i].start_bit = rc[i].start_bit;
			rr[i].end_bit = rc[i].start_bit + 3;
			rr[i].end_hdr_bit = rc[i].hdr_bit;
			rr[i].status = LDA_STREAM_OK;
		}
		return true;
	};
	auto no_stored = [](uint64_t, std::vector<lda_stream_chunk> &, std::vector<lda_stream_res> &) {};
	{
		/* one at a time: sixteen rounds and no more */
		phase_plan(2, plan, hc, hr, 16000);
		hr[1].status = LDA_STREAM_ERR;
		hr[0].end_bit = 5;
		stream_chain ch(plan, hc, hr);
		uint64_t asked = 0;
		CHECK(ch.close(false, true, 1000000, no_stored, open_again, &asked) == WHY_CHAIN);
		CHECK(ch.round == 16 && asked == 16 && ch.nrepairs == 16);
	}
	{
		/* forty at a time: past 64 + 2 * 40 in the fourth round.  (The ends lie
		 * in front of the first planned warm-up: no phase candidates.) */
		phase_plan(40, plan, hc, hr, 16000);
		for (uint32_t k = 0; k < 40; k++) {
			hr[k].start_bit = 100 * k;
			hr[k].end_bit = 100 * k + 50;
		}
		stream_chain ch(plan, hc, hr);
		uint64_t asked = 0;
		CHECK(ch.close(false, true, 1000000, no_stored, open_again, &asked) == WHY_REPAIRS);
		CHECK(ch.round == 3 && ch.nrepairs == 160 && ch.ncand == 0 && asked == 160);
	}
	{
		/* phase candidates do not count */
		phase_plan(500, plan, hc, hr, 16000);
		stream_chain ch(plan, hc, hr);
		std::vector<lda_stream_chunk> rc;
		std::vector<uint8_t> rd;
		CHECK(ch.repairs(16000 * 500, rc, rd) == WHY_OK && ch.nrepairs > 64 + 2 * 500);
	}
}

/* ---------------------------------------------------------------- planner */

static void check_plan(const lda_stream_chunk &carry, const std::vector<uint64_t> &cands, uint64_t R1,
		       uint64_t T, bool static_at_carry, const std::map<uint64_t, std::pair<uint32_t, uint64_t>> &onelen)
{
	uint32_t nexact = 0;
	auto one_length = [&](uint64_t hb, uint64_t *tok0) -> uint32_t {
		const auto it = onelen.find(hb);
		if (it == onelen.end())
			return 0;
		*tok0 = it->second.second;
		return it->second.first;
	};
	const std::vector<planned> plan = plan_window(carry, cands, R1, T, static_at_carry, one_length, &nexact);
	CHECK(!plan.empty() && plan[0].at == carry.start_bit && plan[0].c.kind == carry.kind);
	uint32_t seen_exact = 0;
	uint64_t block_start = carry.start_bit;	/* of the block the chunk belongs to */
	bool block_is_header = carry.kind == LDA_CHUNK_HEADER;
	std::vector<uint64_t> kept;
	for (size_t i = 0; i < plan.size(); i++) {
		const planned &p = plan[i];
		if (i)
			CHECK(p.at >= plan[i - 1].at);
		/* the limit: the next distinct `at`, or R1 */
		uint64_t want = R1;
		for (size_t k = i + 1; k < plan.size(); k++)
			if (plan[k].at != p.at) {
				want = plan[k].at;
				break;
			}
		CHECK(p.c.limit_bit == want);
		if (i && p.c.kind == LDA_CHUNK_HEADER) {
			block_start = p.c.start_bit;
			block_is_header = true;
			kept.push_back(p.c.start_bit);
			CHECK(p.c.hdr_bit == p.c.start_bit && p.c.target_bit == p.c.start_bit && p.at == p.c.start_bit);
			CHECK(std::binary_search(cands.begin(), cands.end(), p.c.start_bit));
		}
		if (p.c.kind == LDA_CHUNK_WARM) {
			CHECK(p.c.start_bit >= block_start + (block_is_header ? STREAM_HDRSAFE : 0));
			CHECK(p.c.start_bit + STREAM_OV / 4 <= p.c.target_bit);
			CHECK(p.c.target_bit - p.c.start_bit <= STREAM_OV && p.at == p.c.target_bit);
			CHECK(p.c.phases == 0);
		}
		if (p.c.kind == LDA_CHUNK_EXACT && i) {
			seen_exact++;
			if (p.c.phases != ~0u) {
				/* the first of a group: K = hi + 1 starts at consecutive bits */
				const uint32_t K = p.c.phases;
				const auto it = onelen.find(block_start);
				CHECK(it != onelen.end() && K == it->second.first + 1 && i + K <= plan.size());
				for (uint32_t j = 0; j < K && i + j < plan.size(); j++) {
					const planned &q = plan[i + j];
					CHECK(q.c.kind == LDA_CHUNK_EXACT && q.c.start_bit == p.c.start_bit + j &&
					      q.c.target_bit == q.c.start_bit && q.at == p.c.start_bit &&
					      q.c.phases == (j ? ~0u : K) && q.c.hdr_bit == p.c.hdr_bit);
				}
				CHECK(i + K == plan.size() || plan[i + K].c.phases != ~0u);
			} else {
				CHECK(plan[i - 1].c.kind == LDA_CHUNK_EXACT && plan[i - 1].c.phases != 0);
			}
		}
	}
	CHECK(seen_exact == nexact && nexact <= 65536);
	/* block starts: which candidates behind the carry got a chunk of their own */
	std::vector<uint64_t> cs;
	for (uint64_t c : cands)
		if (c > carry.start_bit)
			cs.push_back(c);
	uint64_t last_at = carry.start_bit;
	size_t k = 0;
	for (size_t i = 0; i < cs.size(); i++) {
		const uint64_t next = i + 1 < cs.size() ? cs[i + 1] : R1;
		const bool is_kept = k < kept.size() && kept[k] == cs[i];
		/* never closer than T / 8 to the start in front, unless the block is
		 * at least T / 2 long - and nothing else is skipped */
		CHECK(is_kept == (cs[i] - last_at >= T / 8 || next - cs[i] >= T / 2));
		if (is_kept) {
			k++;
			last_at = cs[i];
		}
	}
	CHECK(k == kept.size());
}

static void test_planner()
{
	std::mt19937_64 rng(0x57AEA);
	const std::map<uint64_t, std::pair<uint32_t, uint64_t>> none;
	/* (T below the caller's 2 KiB too: only there a warm-up is left out for
	 * lack of room behind a header) */
	for (uint64_t T : { (uint64_t)4800, (uint64_t)6000, (uint64_t)7200, (uint64_t)10000, (uint64_t)16384,
			    (uint64_t)8 * 4096, (uint64_t)8 * 65536 }) {
		/* no candidate at all: a carry inside a block, at a static header, at
		 * a header nobody knows */
		lda_stream_chunk mid = {};
		mid.kind = LDA_CHUNK_EXACT;
		mid.hdr_bit = 1000;
		mid.start_bit = mid.target_bit = 5000;
		check_plan(mid, {}, 3000000, T, false, none);
		mid.hdr_bit = LDA_HDR_STATIC;
		check_plan(mid, {}, 3000000, T, false, none);
		check_plan(header_chunk(64), {}, 3000000, T, true, none);
		uint32_t nexact = 0;
		CHECK(plan_window(header_chunk(64), {}, 3000000, T, false, ordinary, &nexact).size() == 1);
		CHECK(plan_window(header_chunk(64), {}, 3000000, T, true, ordinary, &nexact)[1].c.hdr_bit == LDA_HDR_STATIC);
		/* one: at the carry, behind it, in front of it */
		check_plan(header_chunk(64), { 64 }, 3000000, T, false, none);
		check_plan(header_chunk(64), { 200000 }, 3000000, T, false, none);
		check_plan(header_chunk(64), { 8 }, 3000000, T, false, none);
		CHECK(plan_window(header_chunk(64), { 64 }, 3000000, T, true, ordinary, &nexact)[1].c.hdr_bit == 64);
		/* about fifty, with runs of tiny blocks */
		for (int rep = 0; rep < 40; rep++) {
			std::vector<uint64_t> cands;
			uint64_t at = rng() % 3 ? 0 : 64;
			for (int b = 0; b < 50; b++) {
				cands.push_back(at);
				const unsigned what = (unsigned)(rng() % 10);
				at += what < 4 ? 100 + rng() % (T / 8) :	/* tiny */
				      what < 7 ? T / 8 + rng() % T :
						 T + rng() % (6 * T);
			}
			const uint64_t R1 = rng() % 2 ? at : cands.back() + 1 + rng() % 500;
			std::map<uint64_t, std::pair<uint32_t, uint64_t>> onelen;
			for (uint64_t c : cands)
				if (rng() % 5 == 0)
					onelen[c] = { 8 + (uint32_t)(rng() % 4), c + 300 + rng() % 2000 };
			check_plan(header_chunk(cands[0]), cands, R1, T, false, rep % 2 ? onelen : none);
			mid.hdr_bit = cands[3];
			mid.start_bit = mid.target_bit = cands[3] + 77;
			check_plan(mid, cands, R1, T, false, rep % 2 ? onelen : none);
		}
	}
	/* a block of one codeword length: hi + 1 starts at the first token and at
	 * every TN behind the header */
	{
		uint32_t nexact = 0;
		auto nine = [](uint64_t hb, uint64_t *tok0) -> uint32_t { *tok0 = hb + 700; return 9; };
		std::vector<planned> plan = plan_window(header_chunk(0), { 0 }, 100000, 16384, false, nine, &nexact);
		/* header, group at 700, groups at TN .. 6 TN (6.5 TN = 99840 <= 100000) */
		CHECK(nexact == 70 && plan.size() == 71);
		CHECK(plan[1].at == 700 && plan[11].at == STREAM_TN && plan[61].at == 6 * STREAM_TN);
		CHECK(plan[0].c.limit_bit == 700 && plan[10].c.limit_bit == STREAM_TN && plan[70].c.limit_bit == 100000);
		/* past 65536 exact chunks the block is planned with warm-ups */
		const uint64_t big = (uint64_t)STREAM_TN * 6554;
		plan = plan_window(header_chunk(0), { 0 }, big, 8 * 65536, false, nine, &nexact);
		CHECK(nexact == 0 && plan.size() > 100 && plan[1].c.kind == LDA_CHUNK_WARM);
		/* (6552 TN and a half: (6552 + 1) x 10 fits, 10 + 6552 x 10 are planned) */
		plan = plan_window(header_chunk(0), { 0 }, big - 2 * STREAM_TN + STREAM_TN / 2, 8 * 65536, false,
				   nine, &nexact);
		CHECK(nexact == 65530 && plan[1].c.kind == LDA_CHUNK_EXACT);
		/* ... counted over the window: the second such block does not fit */
		plan = plan_window(header_chunk(0), { 0, big / 2 }, big, 8 * 65536, false, nine, &nexact);
		CHECK(nexact > 0 && nexact <= 65536 && plan.back().c.kind == LDA_CHUNK_WARM);
	}
}

/* -------------------------------------------------------- one_length_code */

struct bit_writer {
	std::vector<uint8_t> bytes;
	uint64_t nbits = 0;
	void put(uint32_t v, unsigned n)	/* a field: least significant bit first */
	{
		for (unsigned k = 0; k < n; k++, nbits++) {
			if (nbits / 8 == bytes.size())
				bytes.push_back(0);
			bytes[nbits / 8] |= (uint8_t)(((v >> k) & 1) << (nbits % 8));
		}
	}
	void code(uint32_t c, unsigned len)	/* a Huffman codeword: most significant bit first */
	{
		for (unsigned k = len; k-- > 0;)
			put((c >> k) & 1, 1);
	}
};

/* A dynamic header whose precode gives every one of its 19 symbols 5 bits
 * (symbol s has the codeword s).  syms: precode symbols, 16 / 17 / 18 with
 * their repeat counts in the high half.  Returns the bit of the first token. */
static uint64_t write_header(bit_writer &w, uint32_t nl, uint32_t nd, const std::vector<uint32_t> &syms)
{
	w.put(0, 1);
	w.put(2, 2);
	w.put(nl - 257, 5);
	w.put(nd - 1, 5);
	w.put(19 - 4, 4);
	for (int i = 0; i < 19; i++)
		w.put(5, 3);	/* (in the precode's order: all the same) */
	for (uint32_t s : syms) {
		const uint32_t sy = s & 0xFFFF, rep = s >> 16;
		w.code(sy, 5);
		if (sy == 16)
			w.put(rep - 3, 2);
		else if (sy == 17)
			w.put(rep - 3, 3);
		else if (sy == 18)
			w.put(rep - 11, 7);
	}
	const uint64_t first_token = w.nbits;
	for (int k = 0; k < 16; k++)
		w.put(0xA5, 8);	/* tokens */
	return first_token;
}

static uint32_t run_olc(const bit_writer &w, uint64_t hb, uint64_t raw_bits, uint64_t *tok)
{
	const stored_probe_bytes bits = { w.bytes.data(), w.bytes.size() };
	*tok = ~(uint64_t)0;
	return one_length_code(bits, raw_bits, hb, tok);
}

/* `n8` literals of 8 bits, the other 256 - n8 and the end-of-block symbol of 9 */
static std::vector<uint32_t> mostly_eight(uint32_t n8)
{
	std::vector<uint32_t> syms;
	for (uint32_t i = 0; i < 257; i++)
		syms.push_back(i < n8 ? 8 : 9);
	syms.push_back(5);	/* one offset code */
	return syms;
}

static void test_one_length_code()
{
	uint64_t tok;
	{
		/* 256 literals of 8 bits and the end-of-block symbol, behind 13 bits
		 * of something else */
		bit_writer w;
		w.put(0x1ABC, 13);
		std::vector<uint32_t> syms(257, 8);
		syms.push_back(0);
		const uint64_t t0 = write_header(w, 257, 1, syms);
		CHECK(run_olc(w, 13, 8 * w.bytes.size(), &tok) == 8 && tok == t0);
		/* the same lengths by repeat codes */
		bit_writer r;
		std::vector<uint32_t> rs = { 8 };
		for (int k = 0; k < 42; k++)
			rs.push_back(16 | 6u << 16);
		rs.push_back(16 | 4u << 16);	/* 1 + 42 * 6 + 4 = 257 */
		rs.push_back(17 | 3u << 16);	/* three offset codes of length 0 */
		const uint64_t t1 = write_header(r, 257, 3, rs);
		CHECK(run_olc(r, 0, 8 * r.bytes.size(), &tok) == 8 && tok == t1);
		/* cut short by raw_bits: in the precode, in the lengths, at the first token */
		CHECK(run_olc(w, 13, 13 + 60, &tok) == 0);
		CHECK(run_olc(w, 13, 13 + 17 + 57 + 5 * 100, &tok) == 0);
		CHECK(run_olc(w, 13, t0, &tok) == 0 && tok == ~(uint64_t)0);
		CHECK(run_olc(w, 13, t0 + 32, &tok) == 8);
		/* not a dynamic block there */
		CHECK(run_olc(w, 12, 8 * w.bytes.size(), &tok) == 0);
	}
	{
		/* the 98 % rule: 50 * hist >= 49 * 2^8 holds from 251 literals on */
		bit_writer a, b;
		const uint64_t ta = write_header(a, 257, 1, mostly_eight(251));
		CHECK(run_olc(a, 0, 8 * a.bytes.size(), &tok) == 9 && tok == ta);
		write_header(b, 257, 1, mostly_eight(250));
		CHECK(run_olc(b, 0, 8 * b.bytes.size(), &tok) == 0);
	}
	{
		/* a text-like code: three quarters of the first literals on one length
		 * (no early exit), the rest spread - read to its end, refused there */
		bit_writer w;
		std::vector<uint32_t> syms;
		for (uint32_t i = 0; i < 256; i++)
			syms.push_back(i < 192 ? 8 : 7 + 2 * (i & 1));
		syms.push_back(9);
		syms.push_back(5);
		write_header(w, 257, 1, syms);
		CHECK(run_olc(w, 0, 8 * w.bytes.size(), &tok) == 0);
		/* spread from the start: the two dozen lengths say so first - what
		 * stands behind them is never read (here: a repeat of nothing) */
		bit_writer e;
		syms.clear();
		for (uint32_t i = 0; i < 30; i++)
			syms.push_back(5 + i % 6);
		syms.push_back(19);	/* (no precode symbol: never reached) */
		write_header(e, 257, 1, syms);
		CHECK(run_olc(e, 0, 8 * e.bytes.size(), &tok) == 0);
	}
	{
		/* a repeat code with nothing in front */
		bit_writer w;
		std::vector<uint32_t> syms = { 16 | 3u << 16 };
		for (uint32_t i = 0; i < 255; i++)
			syms.push_back(8);
		syms.push_back(0);
		write_header(w, 257, 1, syms);
		CHECK(run_olc(w, 0, 8 * w.bytes.size(), &tok) == 0);
	}
}

int main()
{
	test_in_step();
	test_one_repair(true);
	test_one_repair(false);
	test_doubling();
	test_phase_group();
	test_phase_candidates();
	test_under_static();
	test_walk_ends();
	test_stored_run();
	test_refusals();
	test_planner();
	test_one_length_code();
	if (g_fail) {
		printf("%d checks failed\n", g_fail);
		return 1;
	}
	printf("stream plan ok\n");
	return 0;
}
