/*
 * test_png_write_plan.cpp - the host arithmetic of
 * libdeflate_amd_png_encode_batch (csrc/png_write_plan.h) on the CPU: every
 * refusal with its reason, the bound, the overflowing products in 128-bit
 * arithmetic, and the plan against a serial model - rooms that never overlap,
 * the group class of every image, a work list that covers every row of every
 * image exactly once and in order in its class's range, the piece columns
 * equal to zipw_cut_pieces() called directly on the rooms.  Stand-alone:
 * tests/test_png_write_plan.py builds it with the host compiler under the
 * address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_write_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef unsigned __int128 u128;

static const unsigned COMBOS[15][2] = {
	{ 1, 0 }, { 2, 0 }, { 4, 0 }, { 8, 0 }, { 16, 0 }, { 8, 2 }, { 16, 2 }, { 1, 3 }, { 2, 3 },
	{ 4, 3 }, { 8, 3 }, { 8, 4 }, { 16, 4 }, { 8, 6 }, { 16, 6 },
};

static unsigned model_channels(unsigned colour)
{
	return colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 1;
}

static u128 model_rowbytes(u128 width, unsigned depth, unsigned colour)
{
	return (width * model_channels(colour) * depth + 7) / 8;
}

static uint64_t model_zlib_bound(uint64_t len)
{
	const uint64_t blocks = (len + 4999) / 5000;
	return 6 + len + 5 * (blocks ? blocks : 1);
}

struct Image {
	uint64_t w, h;
	unsigned depth, colour;
	uint64_t plte, trns;	/* entries, length */
};

/* the rows of images laid out one behind the other from offset 3, PLTE and
 * tRNS data behind each one's pixels; *avail_ret: the bytes they take */
static std::vector<uint64_t> rows_of(const std::vector<Image> &im, uint64_t *avail_ret)
{
	std::vector<uint64_t> rows;
	uint64_t at = 3;
	for (const Image &i : im) {
		const uint64_t rb = (uint64_t)model_rowbytes(i.w, i.depth, i.colour);
		uint64_t row[PNG_ROW_WORDS] = { at, i.h * rb, i.w | i.h << 32,
						i.depth | i.colour << 8 | 0xDEADull << 24, 123, 456, 0, 0 };
		at += i.h * rb + 1;
		if (i.plte) {
			row[6] = at | i.plte << 48;
			at += 3 * i.plte;
		}
		if (i.trns) {
			row[7] = at | i.trns << 48;
			at += i.trns;
		}
		rows.insert(rows.end(), row, row + PNG_ROW_WORDS);
	}
	*avail_ret = at;
	return rows;
}

static void check_plan(const zipw_params &pr, const std::vector<Image> &im, unsigned flags)
{
	const uint64_t n = im.size();
	uint64_t avail;
	const std::vector<uint64_t> rows = rows_of(im, &avail);
	std::string err;

	CHECK(pngw_check(n, rows.data(), avail, PNGW_FILTER_ADAPTIVE, flags, pr.level, err));
	pngw_plan p;
	pngw_plan_build(pr, n, rows.data(), flags, p);
	auto I = [&](int col, uint64_t k) { return p.icols[col * n + k]; };
	CHECK(p.n == n && p.icols.size() == PNGW_ICOLS * n && p.work.size() % PNGW_WORK_WORDS == 0);

	/* the columns, the rooms, the bound */
	std::vector<uint64_t> rooms(n), scans(n);
	uint64_t room_at = 0, bound = 0, pixels = 0;
	for (uint64_t k = 0; k < n; k++) {
		const Image &i = im[k];
		const uint64_t rb = (uint64_t)model_rowbytes(i.w, i.depth, i.colour);
		const unsigned bits = model_channels(i.colour) * i.depth, unit = bits < 8 ? 1 : bits / 8;
		const uint64_t head = 8 + 25 + (i.plte ? 12 + 3 * i.plte : 0) + (i.trns ? 12 + i.trns : 0) + 8;
		rooms[k] = room_at;
		scans[k] = i.h * (1 + rb);
		CHECK(I(PNGW_I_PIX, k) == rows[8 * k] && I(PNGW_I_ROOM, k) == room_at && room_at % 16 == 0);
		CHECK(I(PNGW_I_SCAN, k) == scans[k] && I(PNGW_I_GEOM, k) == (i.h | rb << 32));
		CHECK(I(PNGW_I_DIMS, k) == (i.w | i.h << 32));
		CHECK(I(PNGW_I_META, k) ==
		      (i.depth | i.colour << 8 | (uint64_t)unit << 24 | (uint64_t)model_channels(i.colour) << 32 |
		       ((flags & 1) && i.depth == 16 ? PNGW_META_LE16 : 0)));
		CHECK(I(PNGW_I_PLTE, k) == rows[8 * k + 6] && I(PNGW_I_TRNS, k) == rows[8 * k + 7]);
		CHECK(I(PNGW_I_HEAD, k) == head);
		room_at += (scans[k] + 15) & ~(uint64_t)15;
		bound += head + model_zlib_bound(scans[k]) + 4 + 12;
		pixels += i.h * rb;
	}
	CHECK(p.scan_bytes == room_at && p.bound == bound && p.pixels_total == pixels);
	CHECK(pngw_bound(n, rows.data(), pr.level) == bound);

	/* the work list: class by class, every row of every image once, an item
	 * never longer than its image, at most about 1024 items an image */
	std::vector<uint64_t> next_row(n, 0), items_of(n, 0);
	CHECK(p.items[0] == 0 && p.items[PNGW_CLASSES] == p.work.size() / PNGW_WORK_WORDS);
	for (unsigned c = 0; c < PNGW_CLASSES; c++) {
		CHECK(p.items[c] <= p.items[c + 1]);
		uint64_t last = 0;
		for (uint64_t it = p.items[c]; it < p.items[c + 1]; it++) {
			const uint64_t k = p.work[2 * it], first = p.work[2 * it + 1] & 0xFFFFFFFFull;
			const uint64_t cnt = p.work[2 * it + 1] >> 32;
			CHECK(k < n && k >= last);	/* the caller's order inside a class */
			if (k >= n)
				return;
			last = k;
			const uint64_t rb = I(PNGW_I_GEOM, k) >> 32;
			const unsigned G = rb <= 64 ? 4 : rb <= 256 ? 16 : 64;
			CHECK(pngw_group_lanes(c) == G && pngw_group_class(rb) == c);
			CHECK((16 * (uint64_t)G >= rb || G == 64) && (G == 4 || 16 * (uint64_t)(G / 4) < rb));
			CHECK(cnt >= 1 && first + cnt <= im[k].h);
			CHECK(cnt % (256 / G) == 0 || first + cnt == im[k].h);
			CHECK(first == next_row[k]);
			next_row[k] = first + cnt;
			items_of[k]++;
		}
	}
	for (uint64_t k = 0; k < n; k++) {
		CHECK(next_row[k] == im[k].h);
		CHECK(items_of[k] >= 1 && items_of[k] <= 1024);
	}

	/* the pieces: zipw_cut_pieces() as it is, over the rooms */
	std::vector<uint64_t> first(n), cnt(n);
	zipw_pieces q;
	zipw_cut_pieces(pr, n, rooms.data(), scans.data(), first.data(), cnt.data(), q);
	CHECK(q.np == p.np && q.slots_bytes == p.slots_bytes && q.pcols == p.pcols &&
	      q.seg_info == p.seg_info && q.groups.size() == p.groups.size());
	for (size_t g = 0; g < q.groups.size() && g < p.groups.size(); g++)
		CHECK(q.groups[g].lo == p.groups[g].lo && q.groups[g].hi == p.groups[g].hi &&
		      q.groups[g].max_in == p.groups[g].max_in && q.groups[g].S == p.groups[g].S);
	for (uint64_t k = 0; k < n; k++) {
		CHECK(I(PNGW_I_FIRST, k) == first[k] && I(PNGW_I_COUNT, k) == cnt[k] && cnt[k] >= 1);
		/* an image's pieces tile its room, in order */
		uint64_t at = rooms[k];
		for (uint64_t j = first[k]; j < first[k] + cnt[k]; j++) {
			CHECK(p.pcols[ZIPW_P_PC_OFF * p.np + j] == at);
			at += p.pcols[ZIPW_P_PC_N * p.np + j];
		}
		CHECK(at == rooms[k] + scans[k]);
	}
}

static void plans(void)
{
	std::vector<Image> all;
	for (const unsigned *c : COMBOS)
		for (uint64_t w : { 1, 2, 5, 17, 64, 65, 257 })
			for (uint64_t h : { 1, 2, 3, 67 })
				all.push_back({ w, h, c[0], c[1], c[1] == 3 ? (c[0] == 1 ? 2ull : 3ull) : 0,
						c[1] == 3 ? 1ull : c[1] == 0 ? 2ull : c[1] == 2 ? 6ull : 0 });
	/* the group classes' edges, the segment rule's, a 256 x 256 RGB, tall and wide ones */
	for (uint64_t w : { 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1040, 2100 })
		all.push_back({ w, 67, 8, 0, 0, 0 });
	all.push_back({ 131070, 1, 8, 0, 0, 0 });
	all.push_back({ 1023, 128, 8, 0, 0, 0 });
	all.push_back({ 43690, 3, 8, 0, 0, 0 });
	all.push_back({ 256, 256, 8, 2, 256, 6 });
	all.push_back({ 1024, 1025, 8, 6, 3, 0 });
	all.push_back({ 1, 300000, 1, 0, 0, 0 });	/* two bytes a row, many rows */
	all.push_back({ 3000000, 2, 8, 2, 0, 0 });
	for (int level : { 0, 1, 6, 12 })
		for (int variant = 0; variant < 3; variant++) {
			zipw_params pr = {};
			pr.level = level;
			pr.no_segments = variant == 1;
			pr.env_seg = variant == 2 ? 20000 : 0;
			pr.tile = 4096;
			pr.D = 20480;
			pr.small_max = level <= 9 ? 4096 : 0;
			check_plan(pr, all, variant & 1);
		}
	zipw_params pr = {};
	pr.level = 6;
	pr.tile = 4096;
	pr.D = 20480;
	pr.small_max = 4096;
	check_plan(pr, {}, 0);
	/* a very tall image: 10^9 rows of two bytes, near the one IDAT's limit */
	check_plan(pr, { { 1, 1000000000ull, 8, 0, 0, 0 }, { 3, 3, 8, 2, 0, 0 } }, 0);
}

static bool refused(const uint64_t *row, uint64_t avail, int level, const char *word)
{
	std::string err;
	if (pngw_check(1, row, avail, 5, 0, level, err))
		return false;
	if (err.find("image 0") == err.npos || err.find(word) == err.npos) {
		printf("reason: %s (no \"%s\")\n", err.c_str(), word);
		return false;
	}
	return pngw_bound(1, row, level) == 0 || strstr(word, "in_avail") != NULL;
}

static void refusals_and_bounds(void)
{
	std::string err;
	/* a 5 x 3 RGB8 at offset 10, a palette image behind it */
	const uint64_t good[16] = { 10, 45, 5 | 3ull << 32, 8 | 2 << 8, 0, 0, 0, 0,
				    60, 28, 13 | 4ull << 32, 4 | 3 << 8, 0, 0, 88 | 5ull << 48, 103 | 5ull << 48 };
	CHECK(pngw_check(2, good, 108, 5, 0, 6, err) && pngw_check(2, good, 108, 0, 1, 0, err));
	CHECK(pngw_check(0, NULL, 0, 5, 0, 6, err) && pngw_bound(0, NULL, 6) == 0);
	CHECK(pngw_bound(2, good, 6) == (8 + 25 + 8 + 6 + 48 + 5 + 4 + 12) +
					(8 + 25 + 12 + 15 + 12 + 5 + 8 + 6 + 32 + 5 + 4 + 12));
	CHECK(pngw_zlib_bound(0) == 11 && pngw_zlib_bound(5000) == 5011 && pngw_zlib_bound(5001) == 5017);
	CHECK(!pngw_check(2, good, 108, 6, 0, 6, err) && err.find("filter") != err.npos);
	for (unsigned flags : { 2u, 3u, 0x80000000u })
		CHECK(!pngw_check(2, good, 108, 5, flags, 6, err) && err.find("flags") != err.npos);
	CHECK(!pngw_check((1ull << 28) + 1, good, 108, 5, 0, 6, err) && err.find("n_images") != err.npos);
	CHECK(pngw_bound((1ull << 28) + 1, good, 6) == 0);
	CHECK(!pngw_check(2, good, 107, 5, 0, 6, err) && err.find("image 1") != err.npos &&
	      err.find("tRNS") != err.npos);

	struct { int col; uint64_t value; uint64_t avail; const char *word; } bad[] = {
		{ 2, 3ull << 32, 100, "width" }, { 2, 5, 100, "width" },
		{ 2, 1ull << 31 | 3ull << 32, 100, "width" }, { 2, 5 | 1ull << 63, 100, "width" },
		{ 3, 4 | 2 << 8, 100, "bit depth" }, { 3, 8 | 5 << 8, 100, "bit depth" },
		{ 3, 16 | 3 << 8, 100, "bit depth" }, { 3, 8 | 2 << 8 | 1 << 16, 100, "interlaced" },
		{ 1, 44, 100, "word 1" }, { 1, 46, 100, "word 1" },
		{ 0, 56, 100, "pixels do not lie inside in_avail" }, { 0, ~0ull, 100, "pixels do not lie inside in_avail" },
		{ 1, 45, 54, "pixels do not lie inside in_avail" },
		{ 6, 60 | 257ull << 48, 2000, "PLTE" }, { 6, 60, 2000, "PLTE" },
		{ 6, 98 | 1ull << 48, 100, "PLTE does not lie inside in_avail" },
		{ 6, 101 | 1ull << 48, 100, "PLTE does not lie inside in_avail" },
		{ 7, 60 | 5ull << 48, 100, "tRNS length" }, { 7, 60 | 2ull << 48, 100, "tRNS length" },
		{ 7, 95 | 6ull << 48, 100, "tRNS does not lie inside in_avail" },
	};
	for (const auto &b : bad) {
		uint64_t row[8];
		memcpy(row, good, sizeof(row));
		if (b.col == 1 && b.avail == 54)
			;	/* the row as it is, too little input */
		else
			row[b.col] = b.value;
		CHECK(refused(row, b.avail, 6, b.word));
	}
	/* bits 24 and up of word 3 and words 4, 5 are nobody's business */
	uint64_t row[8];
	memcpy(row, good, sizeof(row));
	row[3] |= 0xFFFFFFFFFFull << 24;
	row[4] = row[5] = ~0ull;
	CHECK(pngw_check(1, row, 100, 5, 0, 6, err) && pngw_bound(1, row, 6) == pngw_bound(1, good, 6));
	/* PLTE and tRNS by colour type */
	const uint64_t grey[8] = { 0, 15, 5 | 3ull << 32, 8, 0, 0, 0, 0 };
	uint64_t r[8];
	auto with = [&](const uint64_t *base, unsigned colour_depth, uint64_t size, uint64_t plte, uint64_t trns) {
		memcpy(r, base, sizeof(r));
		r[1] = size;
		r[3] = colour_depth;
		r[6] = plte;
		r[7] = trns;
		return r;
	};
	CHECK(refused(with(grey, 8, 15, 20 | 1ull << 48, 0), 2000, 6, "PLTE with a grey"));
	CHECK(refused(with(grey, 8 | 4 << 8, 30, 20 | 1ull << 48, 0), 2000, 6, "PLTE with a grey"));
	CHECK(refused(with(grey, 8 | 3 << 8, 15, 0, 0), 2000, 6, "without a PLTE"));
	CHECK(refused(with(grey, 2 | 3 << 8, 6, 20 | 5ull << 48, 0), 2000, 6, "1 << depth"));
	CHECK(pngw_check(1, with(grey, 2 | 3 << 8, 6, 20 | 4ull << 48, 40 | 4ull << 48), 2000, 5, 0, 6, err));
	CHECK(refused(with(grey, 2 | 3 << 8, 6, 20 | 4ull << 48, 40 | 5ull << 48), 2000, 6, "tRNS length"));
	CHECK(refused(with(grey, 8 | 4 << 8, 30, 0, 40 | 2ull << 48), 2000, 6, "tRNS with an alpha"));
	CHECK(refused(with(grey, 8 | 6 << 8, 60, 0, 40 | 6ull << 48), 2000, 6, "tRNS with an alpha"));
	CHECK(pngw_check(1, with(grey, 8 | 6 << 8, 60, 20 | 256ull << 48, 0), 2000, 5, 0, 6, err));
	CHECK(pngw_check(1, with(grey, 8, 15, 0, 40 | 2ull << 48), 2000, 5, 0, 6, err));
	CHECK(pngw_check(1, with(grey, 8 | 2 << 8, 45, 0, 40 | 6ull << 48), 2000, 5, 0, 6, err));

	/* the products that overflow 64 bits where they are formed carelessly:
	 * 128-bit arithmetic says what the row is */
	const uint64_t M = 0x7FFFFFFFull;
	for (const unsigned *c : COMBOS) {
		const u128 rb = model_rowbytes(M, c[0], c[1]);
		CHECK((u128)png_rowbytes(M, c[0], c[1]) == rb);
		const u128 scan = (u128)M * (1 + rb);
		CHECK(scan >= (u128)1 << 32);
		uint64_t big[8] = { 0, (uint64_t)((u128)M * rb), M | M << 32, c[0] | c[1] << 8, 0, 0,
				    c[1] == 3 ? 1 | 1ull << 48 : 0, 0 };
		CHECK(refused(big, ~0ull, 6, "2^32"));
	}
	/* the largest scanlines there are, 2^32 - 1 bytes and just below: refused
	 * for the one IDAT, at level 0 for the compress call first */
	const uint64_t w1 = 0xFFFFFFFFull / 3 - 1;	/* 3 rows of 1 + w1: 2^32 - 1 */
	const uint64_t wide[8] = { 0, 3 * w1, w1 | 3ull << 32, 8, 0, 0, 0, 0 };
	CHECK(3 * (1 + w1) == 0xFFFFFFFFull);
	CHECK(refused(wide, ~0ull, 6, "2^31 - 1") && refused(wide, ~0ull, 0, "level-0"));
	/* the edge of the IDAT limit: the bound 2^31 - 1 passes, 2^31 does not */
	uint64_t lo = 1, hi = 1ull << 31;
	while (lo + 1 < hi) {
		const uint64_t mid = (lo + hi) / 2;
		(model_zlib_bound(mid + 1) <= 0x7FFFFFFFull ? lo : hi) = mid;
	}
	const uint64_t fits[8] = { 0, lo, lo | 1ull << 32, 8, 0, 0, 0, 0 };
	const uint64_t over[8] = { 0, lo + 1, (lo + 1) | 1ull << 32, 8, 0, 0, 0, 0 };
	CHECK(model_zlib_bound(lo + 1) <= 0x7FFFFFFFull && model_zlib_bound(lo + 2) > 0x7FFFFFFFull);
	CHECK(pngw_check(1, fits, ~0ull, 5, 0, 6, err) && pngw_check(1, fits, ~0ull, 5, 0, 0, err));
	CHECK(pngw_bound(1, fits, 6) == 8 + 25 + 8 + model_zlib_bound(lo + 1) + 4 + 12);
	CHECK(refused(over, ~0ull, 6, "2^31 - 1"));
	/* CRC-32("IDAT" + 78 9C): the check value of the bit-by-bit routine */
	uint32_t crc = ~0u;
	for (unsigned b : { 0x49u, 0x44u, 0x41u, 0x54u, 0x78u, 0x9Cu }) {
		crc ^= b;
		for (int k = 0; k < 8; k++)
			crc = crc >> 1 ^ (crc & 1 ? 0xEDB88320u : 0);
	}
	CHECK(pngw_idat_head_crc(6) == ~crc && pngw_idat_head_crc(1) != ~crc);
}

int main(void)
{
	refusals_and_bounds();
	plans();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("png write plan ok\n");
	return 0;
}
