/*
 * test_zip_write_plan.cpp - the host arithmetic of
 * libdeflate_amd_zip_compress_batch (csrc/zip_write_plan.h) on the CPU: the
 * bound and the ZIP64 decision, the refusals, and the plan's columns against a
 * plain model - pieces that tile their entry, primes that never reach in
 * front of it, slots that never overlap, launch groups that cover every piece
 * once, and the list of compress launches (csrc/write_pieces_plan.h) over those
 * groups.  Stand-alone: tests/test_zip_write_plan.py builds it with the host
 * compiler under the address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zip_write_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t MiB = 1 << 20;

/* the plain model: is an entry cut, and how finely */
static uint64_t model_S(const zipw_params &pr, uint64_t usize)
{
	if (usize < 131072)
		return 0;
	if (!pr.store && (pr.level == 0 || (pr.no_segments && usize < 0xFFFF0000ull)))
		return 0;
	if (pr.env_seg)
		return pr.env_seg;
	return usize <= 4 * MiB ? 16384 : usize <= 8 * MiB ? 32768 : 65536;
}

static uint64_t model_slot(uint64_t len)
{
	uint64_t b = len + 5 * ((len + 4999) / 5000 ? (len + 4999) / 5000 : 1) + 32;
	return (b + 15) & ~(uint64_t)15;
}

/* the launch list: every piece of every group exactly once, in piece order, no
 * launch across two groups, a whole-entry group in one launch, a segmented
 * group in launches of lda_large_per_slice(S) pieces but for the last */
static void check_launches(const zipw_pieces &p)
{
	const std::vector<zipw_launch> ls = zipw_launches(p);
	size_t at = 0;
	for (const zipw_group &g : p.groups) {
		/* the model: 32 MiB of segments a launch, one at least */
		const uint64_t per = !g.S ? g.hi - g.lo : 32 * MiB / g.S ? 32 * MiB / g.S : 1;
		const uint64_t want = (g.hi - g.lo + per - 1) / per;
		CHECK(g.S ? per == lda_large_per_slice(g.S) : want == 1);
		for (uint64_t i = 0; i < want; i++, at++) {
			CHECK(at < ls.size());
			if (at >= ls.size())
				return;
			const zipw_launch &l = ls[at];
			CHECK(l.lo == g.lo + i * per);
			CHECK(l.count == (i + 1 < want ? per : g.hi - g.lo - i * per) && l.count >= 1);
			CHECK(l.lo + l.count <= g.hi);
			CHECK(l.max_in == g.max_in && l.segmented == (g.S != 0));
		}
		CHECK(ls[at - 1].lo + ls[at - 1].count == g.hi);
	}
	CHECK(at == ls.size());
	if (p.groups.empty())
		CHECK(ls.empty());
}

static void check_plan(const zipw_params &pr, const std::vector<std::string> &names,
		       const std::vector<uint64_t> &in_off, const std::vector<uint64_t> &in_n,
		       unsigned flags)
{
	const uint64_t n = in_n.size();
	std::string blob = "##";	/* the names start at name_offsets[0] = 2 */
	std::vector<uint64_t> noff(n + 1);
	for (uint64_t k = 0; k < n; k++) {
		noff[k] = blob.size();
		blob += names[k];
	}
	noff[n] = blob.size();
	zipw_plan p;
	zipw_plan_build(pr, n, (const uint8_t *)blob.data(), noff.data(), in_off.data(), in_n.data(),
			flags, p);
	const uint64_t np = p.np;
	auto E = [&](int col, uint64_t k) { return p.ecols[col * n + k]; };
	auto P = [&](int col, uint64_t j) { return p.pcols[col * np + j]; };

	CHECK(p.n == n && p.ecols.size() == ZIPW_ECOLS * n && p.pcols.size() == ZIPW_PCOLS * np &&
	      p.seg_info.size() == np);
	uint64_t plain = 22;
	for (uint64_t k = 0; k < n; k++)
		plain += 30 + 46 + 2 * names[k].size() + in_n[k];
	CHECK(p.zip64 == ((flags & ZIPW_FORCE_ZIP64) != 0 || n >= 65535 || plain >= 0xFFFFFFFFull));
	CHECK(p.bound == plain + (p.zip64 ? 12 * n + 76 : 0) && p.end_bytes == (p.zip64 ? 98u : 22u));
	std::vector<int> owner(np, 0);
	std::vector<uint64_t> seg_of(np, 0);
	uint64_t cen = 0, uoff = 0, pieces = 0;
	for (uint64_t k = 0; k < n; k++) {
		bool utf8 = false;
		for (char ch : names[k])
			utf8 |= (unsigned char)ch >= 0x80;
		CHECK(E(ZIPW_E_NAME_OFF, k) == noff[k] - 2);
		CHECK(E(ZIPW_E_NAME_LEN, k) == (names[k].size() | (utf8 ? ZIPW_NAME_UTF8 : 0)));
		CHECK(E(ZIPW_E_CEN, k) == cen && E(ZIPW_E_USIZE, k) == in_n[k] && E(ZIPW_E_UOFF, k) == uoff);
		cen += 46 + names[k].size() + (p.zip64 ? 12 : 0);
		uoff += in_n[k];
		const uint64_t S = model_S(pr, in_n[k]);
		const uint64_t want = S ? (in_n[k] + S - 1) / S : in_n[k] ? 1 : 0;
		const uint64_t f = E(ZIPW_E_FIRST, k);
		CHECK(E(ZIPW_E_COUNT, k) == want && f + want <= np);
		if (f + want > np)
			return;
		pieces += want;
		uint64_t at = in_off[k];
		for (uint64_t i = 0; i < want; i++) {
			const uint64_t j = f + i;
			owner[j]++;
			seg_of[j] = S;
			/* the pieces tile the entry */
			CHECK(P(ZIPW_P_PC_OFF, j) == at);
			CHECK(P(ZIPW_P_PC_N, j) == (i + 1 < want ? S : in_n[k] - i * (S ? S : 0)));
			CHECK(P(ZIPW_P_PC_N, j) > 0);
			/* the prime: whole tiles, at most D, never in front of the entry */
			const uint64_t prime = P(ZIPW_P_PC_OFF, j) - P(ZIPW_P_IN_OFF, j);
			const uint64_t before = at - in_off[k];
			CHECK(P(ZIPW_P_IN_OFF, j) >= in_off[k] && P(ZIPW_P_IN_OFF, j) <= at);
			CHECK(P(ZIPW_P_IN_OFF, j) + P(ZIPW_P_IN_N, j) == at + P(ZIPW_P_PC_N, j));
			CHECK(prime == (i ? (pr.D < before ? pr.D : before) / pr.tile * pr.tile : 0));
			CHECK(p.seg_info[j] == (prime | (i + 1 == want ? 0x80000000u : 0)));
			CHECK(P(ZIPW_P_SLOT_AV, j) == (pr.store ? 0 : model_slot(S ? S : in_n[k])));
			at += P(ZIPW_P_PC_N, j);
		}
		CHECK(at == in_off[k] + in_n[k]);
	}
	CHECK(cen == p.cd_size && pieces == np);
	for (uint64_t j = 0; j < np; j++)
		CHECK(owner[j] == 1);
	/* slots back to back, none overlapping */
	uint64_t slot_at = 0;
	for (uint64_t j = 0; j < np; j++) {
		CHECK(P(ZIPW_P_SLOT_OFF, j) == slot_at && slot_at % 16 == 0);
		slot_at += P(ZIPW_P_SLOT_AV, j);
	}
	CHECK(p.slots_bytes == slot_at);
	check_launches(p);
	/* the launch groups: every piece once, of one kind each */
	if (pr.store) {
		CHECK(p.groups.empty() && p.slots_bytes == 0);
		return;
	}
	uint64_t g_at = 0;
	int smalls = 0, wholes = 0;
	for (const zipw_group &g : p.groups) {
		CHECK(g.lo == g_at && g.hi > g.lo && g.hi <= np);
		g_at = g.hi;
		uint64_t mx = 0;
		for (uint64_t j = g.lo; j < g.hi && j < np; j++) {
			CHECK(seg_of[j] == g.S);
			mx = P(ZIPW_P_IN_N, j) > mx ? P(ZIPW_P_IN_N, j) : mx;
		}
		if (g.S) {
			CHECK(g.max_in == g.S + (pr.D + pr.tile - 1) / pr.tile * pr.tile && mx <= g.max_in);
		} else {
			CHECK(g.max_in == mx);
			const bool small = mx <= pr.small_max;
			for (uint64_t j = g.lo; j < g.hi && j < np; j++)
				CHECK((P(ZIPW_P_IN_N, j) <= pr.small_max) == small);
			smalls += small;
			wholes += !small;
		}
		for (const zipw_group &o : p.groups)
			CHECK(&o == &g || o.S != g.S || (!g.S && (o.max_in <= pr.small_max) != (g.max_in <= pr.small_max)));
	}
	CHECK(g_at == np && smalls <= 1 && wholes <= 1);
}

static void plans(void)
{
	const std::vector<uint64_t> sizes = {
		0, 1, 100, 4096, 4097, 70000, 131071, 131072, 131073, 0, 4 * MiB - 1, 4 * MiB,
		4 * MiB + 1, 8 * MiB - 1, 8 * MiB, 8 * MiB + 1, 5, 131072, 300000,
	};
	std::vector<std::string> names;
	std::vector<uint64_t> in_off;
	uint64_t at = 7;
	for (size_t k = 0; k < sizes.size(); k++) {
		names.push_back(std::string(1 + k * 13 % 40, (char)('a' + k)) + (k % 4 == 3 ? "\xC3\xA9" : ""));
		/* gaps, and now and then an entry that overlaps the one before */
		in_off.push_back(k % 5 == 4 ? at - (sizes[k] < at ? sizes[k] : at) / 2 : at + k);
		at = in_off.back() + sizes[k];
	}
	for (int level : { 0, 1, 6, 9, 12 })
		for (unsigned flags = 0; flags < 4; flags++)
			for (int variant = 0; variant < 4; variant++) {
				zipw_params pr = {};
				pr.level = level;
				pr.store = level == 0 || (flags & ZIPW_STORE);
				pr.no_segments = variant == 1;
				pr.env_seg = variant == 2 ? 20000 : 0;
				pr.tile = variant == 3 ? 2048 : 4096;
				pr.D = (32768 - 2 * pr.tile - 272) / pr.tile * pr.tile;
				pr.small_max = level <= 9 && variant != 3 ? 4096 : 0;
				check_plan(pr, names, in_off, sizes, flags);
			}
	/* no entry at all; entries that are all empty */
	zipw_params pr = {};
	pr.level = 6;
	pr.tile = 4096;
	pr.D = 20480;
	pr.small_max = 4096;
	check_plan(pr, {}, {}, {}, 0);
	check_plan(pr, { "a", "b" }, { 0, 0 }, { 0, 0 }, ZIPW_FORCE_ZIP64);
	/* 65 535 entries: ZIP64 by the count */
	{
		const uint64_t n = 65535;
		std::vector<std::string> nm(n, "n");
		std::vector<uint64_t> off(n), sz(n);
		for (uint64_t k = 0; k < n; k++) {
			off[k] = 3 * k;
			sz[k] = k % 4;
		}
		check_plan(pr, nm, off, sz, 0);
	}
	/* an entry just below 4 GiB: 65 536 segments whose offsets pass 2^32 */
	check_plan(pr, { "big", "tail" }, { 5000000000ull, 1 }, { 0xFFFFFFFFull, 9 }, 0);
	/* segmented groups of exactly one launch's pieces, one more, and twice as
	 * many: 512 segments of 64 KiB a launch, and 1600 of 20 000 bytes */
	for (uint64_t env_seg : { (uint64_t)0, (uint64_t)20000 }) {
		pr.env_seg = env_seg;
		const uint64_t S = env_seg ? env_seg : 65536, per = 32 * MiB / S;
		for (uint64_t pieces : { per, per + 1, 2 * per }) {
			check_plan(pr, { "seg", "small" }, { 64, 3 }, { pieces * S, 50 }, 0);
			check_plan(pr, { "seg" }, { 0 }, { (pieces - 1) * S + 1 }, 0);
			zipw_plan p;
			const uint64_t noff[2] = { 0, 1 }, off = 0, size = pieces * S;
			zipw_plan_build(pr, 1, (const uint8_t *)"s", noff, &off, &size, 0, p);
			const std::vector<zipw_launch> ls = zipw_launches(p);
			CHECK(p.groups.size() == 1 && p.np == pieces && ls.size() == (pieces + per - 1) / per);
			CHECK(ls.size() && ls[0].count == per && ls.back().count == (pieces % per ? pieces % per : per));
		}
	}
	pr.env_seg = 0;
	/* a store plan has pieces and no groups: nothing is launched */
	{
		zipw_params st = pr;
		st.store = true;
		zipw_plan p;
		const uint64_t noff[3] = { 0, 1, 2 }, off[2] = { 0, 9 }, size[2] = { 9, 40 * MiB };
		zipw_plan_build(st, 2, (const uint8_t *)"ab", noff, off, size, ZIPW_STORE, p);
		CHECK(p.np == 1 + 640 && p.groups.empty() && zipw_launches(p).empty());
		check_plan(st, { "a", "b" }, { 0, 9 }, { 9, 40 * MiB }, ZIPW_STORE);
		/* n == 0 */
		zipw_plan_build(pr, 0, NULL, noff, NULL, NULL, 0, p);
		CHECK(p.np == 0 && p.groups.empty() && zipw_launches(p).empty());
	}
}

static void bounds_and_refusals(void)
{
	bool z;
	uint64_t cd, end;
	const uint64_t noff[4] = { 10, 11, 13, 20 }, sz[3] = { 100, 0, 1ull << 40 };
	CHECK(zipw_bound(0, NULL, NULL, 0, &z, &cd, &end) == 22 && !z && cd == 0 && end == 22);
	CHECK(zipw_bound(0, NULL, NULL, ZIPW_FORCE_ZIP64, &z, &cd, &end) == 98 && z && end == 98);
	CHECK(zipw_bound(2, noff, sz, 0, &z, &cd, &end) == 30 + 1 + 100 + 30 + 2 + 46 + 1 + 46 + 2 + 22);
	CHECK(!z && cd == 95 && end == 22);
	CHECK(zipw_bound(3, noff, sz, 0, &z, &cd, &end) ==
	      (1ull << 40) + 100 + 3 * 30 + 2 * 10 + 3 * (46 + 12) + 98);
	CHECK(z && cd == 3 * 58 + 10 && end == 98);

	std::string err;
	const uint64_t ioff[2] = { 0, 100 }, inn[2] = { 100, 50 };
	CHECK(zipw_check(2, noff, ioff, inn, 150, 117, 0, err));
	CHECK(!zipw_check(2, noff, ioff, inn, 150, 116, 0, err) && err.find("out_avail") != err.npos);
	CHECK(zipw_check(2, noff, ioff, inn, 150, 217, ZIPW_FORCE_ZIP64 | ZIPW_STORE, err));
	CHECK(!zipw_check(2, noff, ioff, inn, 150, 216, ZIPW_FORCE_ZIP64, err));
	CHECK(!zipw_check(2, noff, ioff, inn, 149, 1000, 0, err) && err.find("entry 1") != err.npos);
	CHECK(!zipw_check(2, noff, ioff, inn, 150, 1000, 4, err) && err.find("flags") != err.npos);
	CHECK(!zipw_check((1ull << 28) + 1, noff, ioff, inn, 150, 1000, 0, err) &&
	      err.find("n_entries") != err.npos);
	const uint64_t empty[3] = { 5, 5, 6 }, back[3] = { 5, 4, 6 }, longn[3] = { 0, 65536, 65537 };
	CHECK(!zipw_check(2, empty, ioff, inn, 150, 1000, 0, err) && err.find("empty name") != err.npos);
	CHECK(!zipw_check(2, back, ioff, inn, 150, 1000, 0, err) && err.find("decrease") != err.npos);
	CHECK(!zipw_check(2, longn, ioff, inn, 150, 1ull << 20, 0, err) && err.find("65535") != err.npos);
	const uint64_t huge[2] = { 100, 1ull << 32 };
	CHECK(!zipw_check(2, noff, ioff, huge, 1ull << 40, 1ull << 40, 0, err) &&
	      err.find("4 GiB") != err.npos);
	const uint64_t far[2] = { 0, ~0ull - 5 };
	CHECK(!zipw_check(2, noff, far, inn, 150, 1000, 0, err) && err.find("in_avail") != err.npos);
	CHECK(zipw_check(0, NULL, NULL, NULL, 0, 22, 0, err) && !zipw_check(0, NULL, NULL, NULL, 0, 21, 0, err));
}

int main(void)
{
	bounds_and_refusals();
	plans();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("zip write plan ok\n");
	return 0;
}
