/*
 * test_gzip_members_write_plan.cpp - the host arithmetic of
 * libdeflate_amd_gzip_members_compress_batch
 * (csrc/gzip_members_write_plan.h) on the CPU: the bound, the refusals, and the
 * plan's columns against a plain model - pieces that tile their record, primes
 * that never reach in front of it, slots that never overlap, launch groups
 * that cover every piece once.  Stand-alone:
 * tests/test_gzip_members_write_plan.py builds it with the host compiler under
 * the address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gzip_members_write_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t MiB = 1 << 20;

/* the plain model: is a record cut, and how finely.  Unlike the ZIP plan's,
 * level 0 never cuts: its records go whole through the compress kernel */
static uint64_t model_S(const zipw_params &pr, uint64_t usize)
{
	if (usize < 131072 || pr.level == 0 || (pr.no_segments && usize < 0xFFFF0000ull))
		return 0;
	if (pr.env_seg)
		return pr.env_seg;
	return usize <= 4 * MiB ? 16384 : usize <= 8 * MiB ? 32768 : 65536;
}

static uint64_t model_deflate_bound(uint64_t len)
{
	const uint64_t blocks = (len + 4999) / 5000;
	return len + 5 * (blocks ? blocks : 1);
}

static uint64_t model_slot(uint64_t len)
{
	return (model_deflate_bound(len) + 32 + 15) & ~(uint64_t)15;
}

/* names: NULL for a call without names */
static void check_plan(const zipw_params &pr, const std::vector<std::string> *names,
		       const std::vector<uint64_t> &in_off, const std::vector<uint64_t> &in_n)
{
	const uint64_t n = in_n.size();
	std::string blob = "###";	/* the names start at name_offsets[0] = 3 */
	std::vector<uint64_t> noff(n + 1);
	for (uint64_t k = 0; names && k < n; k++) {
		noff[k] = blob.size();
		blob += (*names)[k];
	}
	noff[n] = blob.size();
	std::string err;
	uint64_t avail = 0;
	for (uint64_t k = 0; k < n; k++)
		avail = in_off[k] + in_n[k] > avail ? in_off[k] + in_n[k] : avail;
	CHECK(gzmw_check(n, names ? (const uint8_t *)blob.data() : NULL, names ? noff.data() : NULL,
			 in_off.data(), in_n.data(), avail, 0, pr.level, err));
	gzmw_plan p;
	gzmw_plan_build(pr, n, names ? noff.data() : NULL, in_off.data(), in_n.data(), p);
	const uint64_t np = p.np;
	auto E = [&](int col, uint64_t k) { return p.ecols[col * n + k]; };
	auto P = [&](int col, uint64_t j) { return p.pcols[col * np + j]; };

	CHECK(p.n == n && p.ecols.size() == GZMW_ECOLS * n && p.pcols.size() == ZIPW_PCOLS * np &&
	      p.seg_info.size() == np);
	CHECK(p.names_bytes == (names ? blob.size() - 3 : 0));
	uint64_t bound = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t nl = names ? (*names)[k].size() : 0;
		bound += 18 + model_deflate_bound(in_n[k]) + (nl ? nl + 1 : 0);
	}
	CHECK(p.bound == bound);
	CHECK(gzmw_bound(n, names ? noff.data() : NULL, in_n.data()) == bound);
	std::vector<int> owner(np, 0);
	std::vector<uint64_t> seg_of(np, 0);
	uint64_t uoff = 0, pieces = 0;
	for (uint64_t k = 0; k < n; k++) {
		CHECK(E(GZMW_E_NAME_OFF, k) == (names ? noff[k] - 3 : 0));
		CHECK(E(GZMW_E_NAME_LEN, k) == (names ? (*names)[k].size() : 0));
		CHECK(E(GZMW_E_USIZE, k) == in_n[k] && E(GZMW_E_UOFF, k) == uoff);
		uoff += in_n[k];
		const uint64_t S = model_S(pr, in_n[k]);
		/* only the record of 0 bytes has no piece: its stream is the place kernel's */
		const uint64_t want = S ? (in_n[k] + S - 1) / S : in_n[k] ? 1 : 0;
		const uint64_t f = E(GZMW_E_FIRST, k);
		CHECK(E(GZMW_E_COUNT, k) == want && f + want <= np);
		if (f + want > np)
			return;
		pieces += want;
		uint64_t at = in_off[k];
		for (uint64_t i = 0; i < want; i++) {
			const uint64_t j = f + i;
			owner[j]++;
			seg_of[j] = S;
			/* the pieces tile the record */
			CHECK(P(ZIPW_P_PC_OFF, j) == at);
			CHECK(P(ZIPW_P_PC_N, j) == (i + 1 < want ? S : in_n[k] - i * S));
			CHECK(P(ZIPW_P_PC_N, j) > 0 && P(ZIPW_P_IN_N, j) <= GZMW_PIECE_MAX);
			/* the prime: whole tiles, at most D, never in front of the record */
			const uint64_t prime = P(ZIPW_P_PC_OFF, j) - P(ZIPW_P_IN_OFF, j);
			const uint64_t before = at - in_off[k];
			CHECK(P(ZIPW_P_IN_OFF, j) >= in_off[k] && P(ZIPW_P_IN_OFF, j) <= at);
			CHECK(P(ZIPW_P_IN_OFF, j) + P(ZIPW_P_IN_N, j) == at + P(ZIPW_P_PC_N, j));
			CHECK(prime == (i ? (pr.D < before ? pr.D : before) / pr.tile * pr.tile : 0));
			CHECK(p.seg_info[j] == (prime | (i + 1 == want ? 0x80000000u : 0)));
			/* the slot holds libdeflate_deflate_compress_bound() of the piece */
			CHECK(P(ZIPW_P_SLOT_AV, j) == model_slot(S ? S : in_n[k]));
			CHECK(P(ZIPW_P_SLOT_AV, j) >= model_deflate_bound(P(ZIPW_P_PC_N, j)));
			at += P(ZIPW_P_PC_N, j);
		}
		CHECK(at == in_off[k] + in_n[k]);
	}
	CHECK(uoff == p.usize_total && pieces == np);
	for (uint64_t j = 0; j < np; j++)
		CHECK(owner[j] == 1);
	/* slots back to back, none overlapping */
	uint64_t slot_at = 0;
	for (uint64_t j = 0; j < np; j++) {
		CHECK(P(ZIPW_P_SLOT_OFF, j) == slot_at && slot_at % 16 == 0);
		slot_at += P(ZIPW_P_SLOT_AV, j);
	}
	CHECK(p.slots_bytes == slot_at);
	/* the launch groups: every piece once, of one kind each - at level 0 too */
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
		/* every third record has no name */
		names.push_back(k % 3 == 1 ? std::string() :
				std::string(1 + k * 13 % 40, (char)('a' + k)) + (k % 4 == 3 ? "\xC3\xA9" : ""));
		/* gaps, and now and then a record that overlaps the one before */
		in_off.push_back(k % 5 == 4 ? at - (sizes[k] < at ? sizes[k] : at) / 2 : at + k);
		at = in_off.back() + sizes[k];
	}
	for (int level : { 0, 1, 6, 9, 12 })
		for (int variant = 0; variant < 4; variant++)
			for (int named = 0; named < 2; named++) {
				zipw_params pr = {};
				pr.level = level;
				pr.no_segments = variant == 1;
				pr.env_seg = variant == 2 ? 20000 : 0;
				pr.tile = variant == 3 ? 2048 : 4096;
				pr.D = (32768 - 2 * pr.tile - 272) / pr.tile * pr.tile;
				pr.small_max = level <= 9 && variant != 3 ? 4096 : 0;
				check_plan(pr, named ? &names : NULL, in_off, sizes);
			}
	/* no record at all; records that are all empty; the longest name */
	zipw_params pr = {};
	pr.level = 6;
	pr.tile = 4096;
	pr.D = 20480;
	pr.small_max = 4096;
	check_plan(pr, NULL, {}, {});
	const std::vector<std::string> none;
	check_plan(pr, &none, {}, {});
	const std::vector<std::string> two = { "a", "" }, longest = { std::string(65534, 'n'), "q" };
	check_plan(pr, &two, { 0, 0 }, { 0, 0 });
	check_plan(pr, &longest, { 0, 3 }, { 10, 0 });
	/* a record just below 4 GiB: 65 536 segments whose offsets pass 2^32 */
	const std::vector<std::string> big = { "big", "tail" };
	check_plan(pr, &big, { 5000000000ull, 1 }, { 0xFFFFFFFFull, 9 });
	check_plan(pr, NULL, { 5000000000ull, 1 }, { 0xFFFFFFFFull, 9 });
	/* ... and at level 0 the longest record that is one piece */
	pr.level = 0;
	check_plan(pr, NULL, { 17 }, { GZMW_PIECE_MAX });
}

static void bounds_and_refusals(void)
{
	const uint64_t noff[4] = { 10, 11, 11, 20 }, sz[3] = { 100, 0, 1ull << 31 };
	CHECK(gzmw_bound(0, NULL, NULL) == 0 && gzmw_bound(0, noff, sz) == 0);
	CHECK(gzmw_bound(1, NULL, sz) == 18 + 100 + 5);
	CHECK(gzmw_bound(2, NULL, sz) == 18 + 100 + 5 + 18 + 5);
	CHECK(gzmw_bound(2, noff, sz) == 18 + 100 + 5 + 2 + 18 + 5);
	CHECK(gzmw_bound(3, noff, sz) ==
	      18 + 100 + 5 + 2 + 18 + 5 + 18 + (1ull << 31) + 5 * (((1ull << 31) + 4999) / 5000) + 10);
	CHECK(gzmw_deflate_bound(0) == 5 && gzmw_deflate_bound(1) == 6 && gzmw_deflate_bound(5000) == 5005 &&
	      gzmw_deflate_bound(5001) == 5011);

	std::string err;
	const uint8_t names[70000] = { 0 };
	std::vector<uint8_t> text(70000, 'x');
	const uint64_t ioff[2] = { 0, 100 }, inn[2] = { 100, 50 };
	CHECK(gzmw_check(2, text.data(), noff, ioff, inn, 150, 0, 6, err));
	CHECK(gzmw_check(2, NULL, NULL, ioff, inn, 150, 0, 6, err));
	CHECK(gzmw_check(0, NULL, NULL, NULL, NULL, 0, 0, 6, err));
	CHECK(!gzmw_check(2, text.data(), noff, ioff, inn, 149, 0, 6, err) &&
	      err.find("record 1") != err.npos && err.find("in_avail") != err.npos);
	for (unsigned flags : { 1u, 2u, 0x80000000u })
		CHECK(!gzmw_check(2, text.data(), noff, ioff, inn, 150, flags, 6, err) &&
		      err.find("flags") != err.npos);
	CHECK(!gzmw_check((1ull << 28) + 1, text.data(), noff, ioff, inn, 150, 0, 6, err) &&
	      err.find("n_records") != err.npos);
	const uint64_t back[3] = { 5, 4, 6 }, longn[3] = { 0, 65535, 65536 }, fits[3] = { 0, 65534, 65535 };
	CHECK(!gzmw_check(2, text.data(), back, ioff, inn, 150, 0, 6, err) && err.find("decrease") != err.npos);
	CHECK(!gzmw_check(2, text.data(), longn, ioff, inn, 150, 0, 6, err) && err.find("65534") != err.npos);
	CHECK(gzmw_check(2, text.data(), fits, ioff, inn, 150, 0, 6, err));
	/* a 0 byte inside a name; outside every name it is nobody's business */
	CHECK(!gzmw_check(2, names, noff, ioff, inn, 150, 0, 6, err) && err.find("record 0") != err.npos &&
	      err.find("0 byte") != err.npos);
	text[11] = 0;
	text[9] = 0;
	CHECK(gzmw_check(2, text.data(), noff, ioff, inn, 150, 0, 6, err));	/* (record 1 has no name) */
	text[19] = 0;
	CHECK(gzmw_check(2, text.data(), noff, ioff, inn, 150, 0, 6, err));
	const uint64_t inn3[3] = { 100, 50, 0 }, ioff3[3] = { 0, 100, 150 };
	CHECK(!gzmw_check(3, text.data(), noff, ioff3, inn3, 150, 0, 6, err) &&
	      err.find("record 2") != err.npos && err.find("0 byte") != err.npos);
	const uint64_t huge[2] = { 100, 1ull << 32 };
	CHECK(!gzmw_check(2, NULL, NULL, ioff, huge, 1ull << 40, 0, 6, err) && err.find("4 GiB") != err.npos);
	const uint64_t far[2] = { 0, ~0ull - 5 };
	CHECK(!gzmw_check(2, NULL, NULL, far, inn, 150, 0, 6, err) && err.find("in_avail") != err.npos);
	/* level 0 has no segments: a record above the kernels' 32-bit positions */
	const uint64_t l0[2] = { 100, GZMW_PIECE_MAX + 1 }, l0ok[2] = { 100, GZMW_PIECE_MAX };
	CHECK(!gzmw_check(2, NULL, NULL, ioff, l0, 1ull << 40, 0, 0, err) && err.find("level-0") != err.npos);
	CHECK(gzmw_check(2, NULL, NULL, ioff, l0ok, 1ull << 40, 0, 0, err));
	CHECK(gzmw_check(2, NULL, NULL, ioff, l0, 1ull << 40, 0, 1, err));
}

int main(void)
{
	bounds_and_refusals();
	plans();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("gzip members write plan ok\n");
	return 0;
}
