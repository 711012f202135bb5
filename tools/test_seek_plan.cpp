/*
 * test_seek_plan.cpp - the host arithmetic of the seek index
 * (libdeflate_amd/csrc/seek_plan.h) against brute-force models: which chunks
 * of a chain become points, what happens to points that do not verify, the
 * tables of a ranged read, and every malformed index refused.  Stand-alone:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_seek_plan tools/test_seek_plan.cpp && ./test_seek_plan
 *
 * (tests/test_seek_plan.py does exactly that.)
 */
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <random>
#include <set>

#include "seek_plan.h"

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

static std::vector<seek_link> random_chain(std::mt19937_64 &rng, size_t n, uint64_t *total)
{
	std::vector<seek_link> ch;
	uint64_t out = 0, bit = 0, hdr = 0;
	for (size_t i = 0; i < n; i++) {
		seek_link c = {};
		c.out_off = out;
		c.start_bit = bit;
		const unsigned what = i == 0 ? 0 : (unsigned)(rng() % 10);
		if (what < 3) {			/* a block header */
			c.kind = LDA_CHUNK_HEADER;
			c.hdr_bit = hdr = bit;
		} else if (what < 8) {		/* inside the block of the last header */
			c.kind = bit > hdr ? LDA_CHUNK_EXACT : LDA_CHUNK_HEADER;
			c.hdr_bit = hdr = c.kind == LDA_CHUNK_HEADER ? bit : hdr;
		} else {			/* under the static codes, no header: never a point */
			c.kind = LDA_CHUNK_EXACT;
			c.hdr_bit = LDA_HDR_STATIC;
		}
		ch.push_back(c);
		out += rng() % 5 == 0 ? 0 : rng() % 40000;
		bit += 1 + rng() % 90000;
	}
	*total = out + rng() % 1000;
	return ch;
}

static void check_points(const std::vector<seek_link> &ch, uint64_t total,
			 const std::vector<size_t> &pts, uint64_t spacing)
{
	CHECK(!pts.empty() && pts[0] == 0);
	/* the model: walk the chain, take what the rule says */
	std::vector<size_t> model(1, 0);
	for (size_t i = 1; i < ch.size(); i++) {
		const seek_link &l = ch[model.back()];
		if (seek_eligible(ch[i]) && ch[i].out_off < total && ch[i].out_off >= l.out_off &&
		    ch[i].out_off - l.out_off >= spacing && ch[i].start_bit > l.start_bit)
			model.push_back(i);
	}
	CHECK(model == pts);
	for (size_t k = 1; k < pts.size(); k++) {
		CHECK(seek_eligible(ch[pts[k]]));
		CHECK(ch[pts[k]].out_off - ch[pts[k - 1]].out_off >= spacing);
	}
}

static void test_thinning()
{
	std::mt19937_64 rng(0x5EEC);
	for (int it = 0; it < 300; it++) {
		uint64_t total = 0;
		const std::vector<seek_link> ch = random_chain(rng, 1 + rng() % 400, &total);
		const uint64_t spacing = 1 + rng() % 100000;
		/* room for everything: the spacing stays */
		uint64_t used = 0;
		std::vector<size_t> pts = seek_thin(ch, total, spacing, ch.size() + 1, &used);
		CHECK(used == spacing);
		check_points(ch, total, pts, spacing);
		const size_t all = pts.size();
		/* every smaller capacity: doubled until it fits, and no further */
		for (size_t cap : { (size_t)1, (size_t)2, (size_t)3, all / 2 + 1, all }) {
			pts = seek_thin(ch, total, spacing, cap, &used);
			CHECK(pts.size() >= 1 && pts.size() <= cap);
			check_points(ch, total, pts, used);
			uint64_t s = spacing;
			while (s < used) {
				CHECK(seek_thin(ch, total, s, ch.size() + 1, NULL).size() > cap);
				s *= 2;
			}
			CHECK(s == used);
			if (cap == 1)
				CHECK(pts.size() == 1 && pts[0] == 0);
		}
	}
	/* nothing to plan with */
	std::vector<seek_link> one(1);
	CHECK(seek_thin(one, 10, 0, 4, NULL).empty());
	CHECK(seek_thin(one, 10, 5, 0, NULL).empty());
	CHECK(seek_thin(one, 0, 5, 4, NULL).size() == 1);
	CHECK(seek_capacity(0, 1 << 20) == 0 && seek_capacity(11, 1 << 20) == 0);
	CHECK(seek_capacity(12, 32767) == 0 && seek_capacity(12, 32768) == 1);
	CHECK(seek_capacity(4 * 12, 5 * 32768) == 5 && seek_capacity(4 * 6, 9 * 32768) == 4);
}

static void test_dropping()
{
	std::vector<seek_link> pts(6);
	for (size_t k = 0; k < 6; k++)
		pts[k].out_off = 100 * k;
	std::vector<uint8_t> failed = { 0, 0, 1, 1, 0, 0 }, recount;
	CHECK(seek_drop_failed(pts, failed, recount) == 2);
	CHECK(pts.size() == 4 && pts[1].out_off == 100 && pts[2].out_off == 400);
	CHECK((recount == std::vector<uint8_t>{ 0, 1, 0, 0 }));
	failed = { 1, 0, 0, 1 };	/* point 0 stays: its successor goes */
	CHECK(seek_drop_failed(pts, failed, recount) == 2);
	CHECK(pts.size() == 2 && pts[0].out_off == 0 && pts[1].out_off == 400);
	CHECK((recount == std::vector<uint8_t>{ 1, 1 }));
	failed = { 1, 1 };
	CHECK(seek_drop_failed(pts, failed, recount) == 1 && pts.size() == 1);
	failed = { 1 };
	CHECK(seek_drop_failed(pts, failed, recount) == 0 && pts.size() == 1);
}

/* an index over `total` bytes with points at the given offsets */
static std::vector<uint64_t> make_index(const std::vector<uint64_t> &offs, uint64_t total,
					uint64_t raw_off, uint64_t raw_n, uint64_t ftr)
{
	seek_export x;
	x.raw_off = raw_off;
	x.raw_nbytes = raw_n;
	x.ftr = ftr;
	x.total = total;
	std::vector<seek_link> pts;
	for (size_t k = 0; k < offs.size(); k++) {
		seek_link l = {};
		l.out_off = offs[k];
		l.start_bit = k ? 3 + 11 * offs[k] / 4 : 0;
		l.kind = k % 2 ? LDA_CHUNK_EXACT : LDA_CHUNK_HEADER;
		l.hdr_bit = k % 2 ? l.start_bit - 1 : l.start_bit;
		pts.push_back(l);
	}
	std::vector<uint64_t> idx(LDA_SEEK_ROW * (offs.size() + 2));
	seek_write_index(idx.data(), 2, x, pts);
	return idx;
}

static void check_plan(const seek_view &v, const std::vector<uint64_t> &ranges,
		       const seek_read_plan &pl)
{
	const size_t nr = ranges.size() / 2;
	/* the model: byte by byte */
	auto interval_of = [&](uint64_t b) {
		size_t k = 0;
		while (k + 1 < v.n && v.out_off(k + 1) <= b)
			k++;
		return k;
	};
	std::set<size_t> touched;
	uint64_t sum = 0;
	for (size_t r = 0; r < nr; r++) {
		for (uint64_t b = ranges[2 * r]; b < ranges[2 * r] + ranges[2 * r + 1]; b++)
			touched.insert(interval_of(b));
		sum += ranges[2 * r + 1];
	}
	CHECK(pl.out_bytes == sum);
	/* every touched interval once, ascending; slots disjoint, first at 64 Ki */
	CHECK(pl.iv.size() == touched.size());
	size_t j = 0;
	uint64_t slot_end = LDA_SEEK_SLOT0;
	for (size_t k : touched) {
		CHECK(j < pl.iv.size());
		if (j >= pl.iv.size())
			break;
		const seek_interval &iv = pl.iv[j++];
		CHECK(iv.k == k && iv.out_off == v.out_off(k) && iv.nbytes == v.out_off(k + 1) - v.out_off(k));
		CHECK(iv.slot >= slot_end && iv.slot % 2 == 0);
		slot_end = iv.slot + iv.nbytes;
	}
	CHECK(pl.sym_words >= slot_end && pl.sym_words >= LDA_SEEK_SLOT0);
	/* the pieces: in range order, then in stream order; they tile the range
	 * and its place in the output, each inside one interval */
	CHECK(pl.first.size() == nr + 1 && pl.first[0] == 0 && pl.first[nr] == pl.pieces.size());
	uint64_t outpos = 0;
	for (size_t r = 0; r < nr; r++) {
		uint64_t at = ranges[2 * r];
		const uint64_t end = at + ranges[2 * r + 1];
		CHECK(pl.first[r] <= pl.first[r + 1]);
		for (uint64_t p = pl.first[r]; p < pl.first[r + 1]; p++) {
			const seek_piece &pc = pl.pieces[p];
			CHECK(pc.range == r && pc.len > 0 && pc.interval < pl.iv.size());
			const seek_interval &iv = pl.iv[pc.interval];
			CHECK(iv.k == interval_of(at));
			CHECK(iv.out_off + pc.src == at && pc.dst == outpos);
			CHECK(pc.src + pc.len <= iv.nbytes);
			/* as far as the interval or the range goes */
			CHECK(at + pc.len == end || pc.src + pc.len == iv.nbytes);
			at += pc.len;
			outpos += pc.len;
		}
		CHECK(at == end || (ranges[2 * r + 1] == 0 && pl.first[r] == pl.first[r + 1]));
		if (ranges[2 * r + 1] == 0)
			CHECK(pl.first[r] == pl.first[r + 1]);
	}
	CHECK(outpos == sum);
}

static void test_ranges()
{
	std::mt19937_64 rng(0xA11);
	for (int it = 0; it < 200; it++) {
		const uint64_t total = it == 0 ? 0 : 1 + rng() % 3000;
		std::vector<uint64_t> offs(1, 0);
		while (total && offs.size() < 12) {
			const uint64_t nx = offs.back() + 1 + rng() % 600;
			if (nx >= total)
				break;
			offs.push_back(nx);
		}
		const uint64_t raw_n = 4000;
		const std::vector<uint64_t> idx = make_index(offs, total, 10, raw_n, 8);
		seek_view v;
		const std::string why = seek_check_index(idx.data(), idx.size(), 10 + raw_n + 8 + it % 3, &v);
		CHECK(why.empty());
		if (!why.empty()) {
			printf("%s\n", why.c_str());
			continue;
		}
		CHECK(v.n == offs.size() && v.total == total && v.raw_off == 10 && v.ftr == 8);
		std::vector<uint64_t> rg;
		auto add = [&](uint64_t at, uint64_t len) {
			rg.push_back(at);
			rg.push_back(len);
		};
		add(0, 0);
		add(total, 0);
		add(0, total);
		if (total) {
			add(0, 1);
			add(total - 1, 1);
		}
		for (size_t k = 0; k + 1 < offs.size(); k++) {
			add(offs[k], offs[k + 1] - offs[k]);		/* exactly an interval */
			add(offs[k + 1] - 1, 2 <= total - (offs[k + 1] - 1) ? 2 : 1);	/* straddling */
			add(offs[k], offs[k + 1] - offs[k]);		/* the same again */
			if (offs[k + 1] - offs[k] > 2)
				add(offs[k] + 1, offs[k + 1] - offs[k] - 2);	/* inside */
		}
		for (int k = 0; k < 20 && total; k++) {
			const uint64_t at = rng() % (total + 1);
			add(at, rng() % (total - at + 1));
		}
		/* unsorted */
		for (size_t i = rg.size() / 2; i-- > 1;) {
			const size_t o = rng() % (i + 1);
			std::swap(rg[2 * i], rg[2 * o]);
			std::swap(rg[2 * i + 1], rg[2 * o + 1]);
		}
		uint64_t sum = 0;
		for (size_t r = 0; r < rg.size() / 2; r++)
			sum += rg[2 * r + 1];
		seek_read_plan pl;
		CHECK(seek_plan_ranges(v, rg.size() / 2, rg.data(), sum, &pl).empty());
		check_plan(v, rg, pl);
		if (sum) {
			const std::string w = seek_plan_ranges(v, rg.size() / 2, rg.data(), sum - 1, &pl);
			CHECK(w.find("out_avail") != std::string::npos);
		}
		/* a range past the total */
		std::vector<uint64_t> bad = { total, 1 };
		CHECK(seek_plan_ranges(v, 1, bad.data(), 100, &pl).find("past the end") != std::string::npos);
		bad = { total + 1, 0 };
		CHECK(seek_plan_ranges(v, 1, bad.data(), 100, &pl).find("past the end") != std::string::npos);
		bad = { 1, ~(uint64_t)0 };
		CHECK(seek_plan_ranges(v, 1, bad.data(), 100, &pl).find("past the end") != std::string::npos);
		/* no ranges at all */
		CHECK(seek_plan_ranges(v, 0, NULL, 0, &pl).empty() && pl.iv.empty() && pl.pieces.empty());
	}
}

static void test_malformed()
{
	const std::vector<uint64_t> good = make_index({ 0, 100, 250, 900 }, 1000, 10, 500, 8);
	const size_t in_n = 10 + 500 + 8;
	seek_view v;
	CHECK(seek_check_index(good.data(), good.size(), in_n, &v).empty());
	CHECK(seek_check_index(good.data(), good.size() + 5, in_n + 5, &v).empty());
	auto refused = [&](std::vector<uint64_t> idx, size_t words, size_t n, const char *word) {
		const std::string w = seek_check_index(idx.data(), words, n, NULL);
		if (w.empty() || w.find(word) == std::string::npos)
			printf("not refused with \"%s\": \"%s\"\n", word, w.c_str());
		return !w.empty() && w.find(word) != std::string::npos;
	};
	auto with = [&](size_t at, uint64_t val) {
		std::vector<uint64_t> idx = good;
		idx[at] = val;
		return idx;
	};
	const size_t R = LDA_SEEK_ROW, end = R * 5;
	CHECK(refused(good, 11, in_n, "index_words"));
	CHECK(refused(with(0, LDA_SEEK_MAGIC + 1), good.size(), in_n, "magic"));
	CHECK(refused(with(1, 3), good.size(), in_n, "format"));
	CHECK(refused(with(3, 0), good.size(), in_n, "points"));
	CHECK(refused(with(3, 5), good.size(), in_n, "points"));		/* more rows than words */
	CHECK(refused(with(3, ~(uint64_t)0), good.size(), in_n, "points"));
	CHECK(refused(good, good.size() - 1, in_n, "points"));
	CHECK(refused(with(3, 3), good.size(), in_n, "end marker"));		/* row 4 is no closing row */
	CHECK(refused(with(end + 3, 0), good.size(), in_n, "end marker"));
	CHECK(refused(good, good.size(), in_n - 1, "in_nbytes"));		/* the closing row needs more */
	CHECK(refused(with(2, 11), good.size(), in_n, "in_nbytes"));
	CHECK(refused(with(end + 1, 501), good.size(), in_n, "in_nbytes"));
	CHECK(refused(with(end + 2, 9), good.size(), in_n, "in_nbytes"));
	CHECK(refused(with(2, ~(uint64_t)0), good.size(), in_n, "in_nbytes"));
	CHECK(refused(with(R + 0, 1), good.size(), in_n, "point 0"));
	CHECK(refused(with(R + 1, 1), good.size(), in_n, "point 0"));
	CHECK(refused(with(R + 3, LDA_CHUNK_EXACT), good.size(), in_n, "point 0"));
	CHECK(refused(with(2 * R + 0, 0), good.size(), in_n, "row 2"));		/* out_off does not rise */
	CHECK(refused(with(3 * R + 0, 100), good.size(), in_n, "row 3"));
	CHECK(refused(with(3 * R + 0, 99), good.size(), in_n, "row 3"));
	CHECK(refused(with(4 * R + 0, 1000), good.size(), in_n, "row 4"));	/* at the total */
	CHECK(refused(with(end + 0, 900), good.size(), in_n, "row 4"));
	{
		std::vector<uint64_t> idx = good;	/* start_bit does not rise */
		idx[3 * R + 1] = idx[2 * R + 1];
		idx[3 * R + 2] = idx[3 * R + 1];
		CHECK(refused(idx, idx.size(), in_n, "row 3"));
		idx = good;				/* a start past the raw stream */
		idx[4 * R + 1] = 8 * 500;
		idx[4 * R + 2] = idx[4 * R + 1] - 1;
		CHECK(refused(idx, idx.size(), in_n, "row 4"));
	}
	CHECK(refused(with(2 * R + 3, 1), good.size(), in_n, "row 2"));		/* a kind that is none */
	CHECK(refused(with(2 * R + 3, 7), good.size(), in_n, "row 2"));
	CHECK(refused(with(2 * R + 2, good[2 * R + 1]), good.size(), in_n, "row 2"));	/* EXACT at its own header */
	CHECK(refused(with(2 * R + 2, LDA_HDR_STATIC), good.size(), in_n, "row 2"));
	CHECK(refused(with(3 * R + 2, 5), good.size(), in_n, "row 3"));		/* HEADER elsewhere */
}

int main()
{
	test_thinning();
	test_dropping();
	test_ranges();
	test_malformed();
	if (g_fail) {
		printf("%d checks failed\n", g_fail);
		return 1;
	}
	printf("seek plan ok\n");
	return 0;
}
