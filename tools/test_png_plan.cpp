/*
 * test_png_plan.cpp - the host arithmetic of libdeflate_amd_png_out_sizes and
 * libdeflate_amd_png_decode_batch (csrc/png_plan.h) on the CPU: what an IHDR
 * means for all 15 depth and colour pairs, every refusal of a row and of a
 * selection, overflowing products, and the rooms and descriptor columns of
 * selections with duplicates against a serial model, for every out_align.
 * Stand-alone; tests/test_png_plan.py builds it under the address and
 * undefined-behaviour sanitizers and runs it:
 *   c++ -std=c++17 -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_png_plan tools/test_png_plan.cpp && ./test_png_plan
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
	rnd_state ^= rnd_state << 13;
	rnd_state ^= rnd_state >> 7;
	rnd_state ^= rnd_state << 17;
	return rnd_state;
}

static const unsigned combos[15][2] = {	/* depth, colour */
	{ 1, 0 }, { 2, 0 }, { 4, 0 }, { 8, 0 }, { 16, 0 }, { 8, 2 }, { 16, 2 }, { 1, 3 },
	{ 2, 3 }, { 4, 3 }, { 8, 3 }, { 8, 4 }, { 16, 4 }, { 8, 6 }, { 16, 6 },
};

/* the serial model: bits counted one pixel at a time would be too slow, so in
 * 128-bit arithmetic, which cannot overflow here */
static uint64_t model_rowbytes(uint64_t width, unsigned depth, unsigned colour)
{
	static const unsigned ch[7] = { 1, 0, 3, 1, 2, 0, 4 };
	const unsigned __int128 bits = (unsigned __int128)width * ch[colour] * depth;
	return (uint64_t)((bits + 7) / 8);
}

static unsigned model_bpp(unsigned depth, unsigned colour)
{
	static const unsigned ch[7] = { 1, 0, 3, 1, 2, 0, 4 };
	const unsigned bits = ch[colour] * depth;
	return bits >= 8 ? bits / 8 : 1;
}

/* a good row of a file at `off`: signature, IHDR, [PLTE], one IDAT of zsum, IEND */
static void make_row(uint64_t *r, uint64_t off, uint64_t w, uint64_t h, unsigned depth,
		     unsigned colour, uint64_t zsum, uint64_t *n_ret)
{
	static const unsigned ch[7] = { 1, 0, 3, 1, 2, 0, 4 };
	uint64_t pos = off + 33;
	r[6] = r[7] = 0;
	if (colour == 3) {
		r[6] = (pos + 8) | (uint64_t)4 << 48;
		pos += 12 + 12;
	}
	r[2] = w | h << 32;
	r[3] = depth | colour << 8 | (uint64_t)model_bpp(depth, colour) << 24 |
	       (uint64_t)ch[colour] << 32;
	r[4] = pos;
	r[5] = zsum;
	pos += 12 + zsum + 12;
	r[0] = off;
	r[1] = pos - off;
	*n_ret = pos;
}

static void test_shapes(void)
{
	static const uint64_t widths[] = { 1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 65, 67, 4096,
					   0x7FFFFFFFull };
	unsigned seen_bpp = 0;
	for (const auto &c : combos) {
		CHECK(png_depth_ok(c[0], c[1]));
		CHECK(png_bpp(c[0], c[1]) == model_bpp(c[0], c[1]));
		seen_bpp |= 1u << png_bpp(c[0], c[1]);
		for (uint64_t w : widths)
			CHECK(png_rowbytes(w, c[0], c[1]) == model_rowbytes(w, c[0], c[1]));
	}
	CHECK(seen_bpp == (1u << 1 | 1u << 2 | 1u << 3 | 1u << 4 | 1u << 6 | 1u << 8));
	unsigned valid = 0;
	for (unsigned depth = 0; depth < 40; depth++)
		for (unsigned colour = 0; colour < 10; colour++)
			valid += png_depth_ok(depth, colour);
	CHECK(valid == 15);
	CHECK(png_channels(1) == 0 && png_channels(5) == 0 && png_channels(7) == 0);
	/* the largest image there is: 16-bit RGBA, both sides 2^31 - 1 */
	const uint64_t big = 0x7FFFFFFFull;
	CHECK(png_rowbytes(big, 16, 6) == big * 8);
	CHECK(png_too_large(big, big * 8));
	CHECK(png_too_large(1, 0xFFFFFFFFull) && !png_too_large(1, 0xFFFFFFFEull));
	CHECK(png_too_large(16384, 262144) && !png_too_large(16384, 262140));
	CHECK(!png_too_large(65536, 65534) && png_too_large(65536, 65535));
	for (int i = 0; i < 20000; i++) {
		const uint64_t h = 1 + rnd() % big, rb = 1 + rnd() % (big * 8);
		const unsigned __int128 raw = (unsigned __int128)h * (rb + 1);
		CHECK(png_too_large(h, rb) == (raw >= ((unsigned __int128)1 << 32)));
	}
}

static void test_refusals(void)
{
	uint64_t row[8], n, offs[2];
	const uint64_t sel0 = 0;
	std::vector<uint64_t> cols;
	std::string err;
	uint64_t scratch;
	PngShape s;

	make_row(row, 100, 65, 67, 8, 2, 500, &n);
	CHECK(png_row_check(row, n, &s) == NULL);
	CHECK(s.rowbytes == 195 && s.bpp == 3 && s.channels == 3 && s.height == 67);
	CHECK(png_row_check(row, n - 1, &s) != NULL);	/* the file passes in_nbytes */
#define REFUSED(change) do { uint64_t t[8]; memcpy(t, row, sizeof(t)); change; \
		CHECK(png_row_check(t, n, &s) != NULL); \
		CHECK(!png_plan_decode(t, 1, 1, &sel0, n, ~(uint64_t)0, 0, 0, cols, offs, &scratch, err)); \
		CHECK(!err.empty()); } while (0)
	REFUSED(t[0] = n + 1);
	REFUSED(t[1] = n);
	REFUSED(t[2] = 67ull << 32);			/* width 0 */
	REFUSED(t[2] = 65);				/* height 0 */
	REFUSED(t[2] = 0x80000000ull | 67ull << 32);
	REFUSED(t[2] = 65 | 0x80000000ull << 32);
	REFUSED(t[3] = (t[3] & ~0xFFull) | 4);		/* RGB of depth 4 */
	REFUSED(t[3] = (t[3] & ~0xFF00ull) | 5 << 8);	/* colour 5 */
	REFUSED(t[3] |= 1 << 16);			/* interlaced */
	REFUSED(t[3] = (t[3] & ~(0xFFull << 24)) | 4ull << 24);	/* a wrong filter unit */
	REFUSED(t[3] = (t[3] & 0xFFFFFFFFull) | 4ull << 32);	/* wrong channels */
	REFUSED(t[3] |= 1ull << 40);
	REFUSED(t[2] = 65536 | 65536ull << 32);		/* 2^32 raw bytes and more */
	REFUSED(t[4] = 100 + 32);			/* inside the IHDR */
	REFUSED(t[4] = n - 11);
	REFUSED(t[5] = n - 12 - t[4] + 1);		/* the sum passes the file */
	REFUSED(t[6] = (100 + 33 + 8) | 257ull << 48);
	REFUSED(t[6] = (n - 3) | 1ull << 48);
	REFUSED(t[6] = 100 | 1ull << 48);		/* in front of the first chunk */
	REFUSED(t[7] = (n - 3) | 1ull << 48);
	REFUSED(t[7] = (n + 5) | 0ull << 48);
	/* the sum may be anything up to the file's end */
	{
		uint64_t t[8];
		memcpy(t, row, sizeof(t));
		t[5] = n - 12 - t[4];
		CHECK(png_row_check(t, n, &s) == NULL);
		t[5] = 0;
		CHECK(png_row_check(t, n, &s) == NULL);
	}
	/* a palette image needs its PLTE */
	make_row(row, 0, 9, 9, 4, 3, 60, &n);
	CHECK(png_row_check(row, n, &s) == NULL && s.rowbytes == 5 && s.bpp == 1);
	REFUSED(t[6] = 0);
	/* selections */
	make_row(row, 0, 3, 2, 8, 0, 20, &n);
	const uint64_t bad_sel = 1;
	CHECK(!png_plan_decode(row, 1, 1, &bad_sel, n, 100, 0, 0, cols, offs, &scratch, err));
	CHECK(err.find("sel[0]") != std::string::npos);
	CHECK(!png_plan_out_sizes(row, 1, 1, &bad_sel, 0, offs, NULL, err));
	CHECK(png_plan_decode(row, 1, 1, &sel0, n, 6, 0, 0, cols, offs, &scratch, err));
	CHECK(!png_plan_decode(row, 1, 1, &sel0, n, 5, 0, 0, cols, offs, &scratch, err));
	CHECK(err.find("out_avail") != std::string::npos);
	CHECK(!png_plan_decode(row, 1, 1, &sel0, n, 7, 7, 0, cols, offs, &scratch, err));
	CHECK(png_plan_decode(row, 1, 1, &sel0, n, 8, 7, 0, cols, offs, &scratch, err));
	CHECK(offs[0] == 0 && offs[1] == 8);
	/* nothing selected */
	CHECK(png_plan_decode(NULL, 0, 0, NULL, 0, 0, 0, 0, cols, offs, &scratch, err));
	CHECK(offs[0] == 0 && scratch == 0 && cols.empty());
	/* out_sizes refuses words 2 and 3 alone */
	{
		uint64_t t[8];
		memcpy(t, row, sizeof(t));
		t[0] = ~(uint64_t)0;	/* (not read) */
		CHECK(png_plan_out_sizes(t, 1, 1, &sel0, 0, offs, NULL, err) && offs[1] == 6);
		t[3] |= 1 << 16;
		CHECK(!png_plan_out_sizes(t, 1, 1, &sel0, 0, offs, NULL, err));
	}
}

static void test_selections(void)
{
	static const uint64_t dims[] = { 1, 2, 15, 16, 17, 33, 63, 64, 65, 130, 500 };
	const size_t entries = 200;
	std::vector<uint64_t> rows(PNG_ROW_WORDS * entries);
	std::vector<PngShape> shapes(entries);
	std::vector<bool> zero(entries);
	uint64_t pos = 0;
	for (size_t k = 0; k < entries; k++) {
		uint64_t *r = &rows[PNG_ROW_WORDS * k];
		const unsigned *c = combos[rnd() % 15];
		const uint64_t w = dims[rnd() % 11], h = dims[rnd() % 11];
		pos += rnd() % 7;	/* unaligned files */
		make_row(r, pos, w, h, c[0], c[1], rnd() % 3000, &pos);
		zero[k] = rnd() % 5 == 0;
		if (zero[k])
			memset(r + 2, 0, 6 * sizeof(uint64_t));
		shapes[k].height = h;
		shapes[k].rowbytes = model_rowbytes(w, c[0], c[1]);
		shapes[k].bpp = model_bpp(c[0], c[1]);
		shapes[k].depth = c[0];
	}
	for (uint64_t align = 1; align <= 256; align *= 2) {
		for (unsigned flags = 0; flags < 2; flags++) {
			const size_t n_sel = 1 + rnd() % 300;
			std::vector<uint64_t> sel(n_sel), offs(n_sel + 1), offs2(n_sel + 1), cols;
			for (auto &v : sel)
				v = rnd() % entries;	/* duplicates among them */
			sel[n_sel / 2] = sel[0];
			std::string err;
			uint64_t scratch = 0, total = 0;
			/* the model: one selection behind the other */
			uint64_t at = 0, z_total = 0;
			std::vector<uint64_t> m_out(n_sel), m_z(n_sel), m_raw(n_sel);
			uint64_t raw_at = 0;
			for (size_t r = 0; r < n_sel; r++) {
				const size_t k = sel[r];
				m_out[r] = at;
				m_z[r] = z_total;
				m_raw[r] = raw_at;
				if (zero[k])
					continue;
				const uint64_t px = shapes[k].height * shapes[k].rowbytes;
				at += (px + align - 1) / align * align;
				z_total += (rows[PNG_ROW_WORDS * k + 5] + 15) / 16 * 16;
				raw_at += (px + shapes[k].height + 15) / 16 * 16;
			}
			CHECK(png_plan_out_sizes(rows.data(), entries, n_sel, sel.data(), align - 1,
						 offs2.data(), &total, err));
			CHECK(total == at && offs2[n_sel] == at);
			CHECK(!png_plan_decode(rows.data(), entries, n_sel, sel.data(), pos, at ? at - 1 : 0,
					       align - 1, flags, cols, offs.data(), &scratch, err) || at == 0);
			CHECK(png_plan_decode(rows.data(), entries, n_sel, sel.data(), pos, at, align - 1,
					      flags, cols, offs.data(), &scratch, err));
			CHECK(offs == offs2 && scratch == z_total + raw_at);
			CHECK(cols.size() == PNG_COLS * n_sel);
			for (size_t r = 0; r < n_sel; r++) {
				const size_t k = sel[r];
				const uint64_t *row = &rows[PNG_ROW_WORDS * k];
				auto col = [&](int c) { return cols[c * n_sel + r]; };
				CHECK(offs[r] == m_out[r] && col(PNG_COL_OUT_OFF) == m_out[r]);
				CHECK(offs[r] % align == 0);
				if (zero[k]) {
					CHECK(col(PNG_COL_META) == (uint64_t)PNG_UNSUPPORTED << 16);
					CHECK(col(PNG_COL_RAW_N) == 0 && col(PNG_COL_ZSUM) == 0 &&
					      col(PNG_COL_END) == 0 && col(PNG_COL_GEOM) == 0);
					continue;
				}
				const uint64_t px = shapes[k].height * shapes[k].rowbytes;
				CHECK(col(PNG_COL_IDAT) == row[4] && col(PNG_COL_END) == row[0] + row[1]);
				CHECK(col(PNG_COL_ZSUM) == row[5] && col(PNG_COL_Z_OFF) == m_z[r]);
				CHECK(col(PNG_COL_RAW_OFF) == z_total + m_raw[r]);
				CHECK(col(PNG_COL_RAW_N) == px + shapes[k].height);
				CHECK(col(PNG_COL_GEOM) == (shapes[k].height | shapes[k].rowbytes << 32));
				CHECK(col(PNG_COL_META) ==
				      (shapes[k].bpp | (uint64_t)(flags && shapes[k].depth == 16) << 8));
				/* the rooms end inside their areas */
				CHECK(col(PNG_COL_Z_OFF) + row[5] <= z_total);
				CHECK(col(PNG_COL_RAW_OFF) + col(PNG_COL_RAW_N) <= scratch);
				CHECK(offs[r] + px <= offs[r + 1]);
			}
		}
	}
}

int main(void)
{
	test_shapes();
	test_refusals();
	test_selections();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("png plan ok\n");
	return 0;
}
