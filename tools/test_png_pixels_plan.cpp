/*
 * test_png_pixels_plan.cpp - the host arithmetic of
 * libdeflate_amd_png_pixels_out_sizes and libdeflate_amd_png_decode_pixels_batch
 * (csrc/png_pixels_plan.h) on the CPU: the direct / converted decision of all
 * 15 depth and colour pairs x 8 formats x tRNS present or absent against a
 * table (the bit that sends the unfilter into the scratch, the columns a
 * direct batch does not upload), sizes whose products overflow 64 bits in 128-bit arithmetic, the
 * rooms, the three scratch areas, the converted selections' columns and the
 * tile prefix
 * against a serial model for every out_align with duplicates and zero rows, and
 * every refusal.  Stand-alone; tests/test_png_pixels_plan.py builds it under
 * the address and undefined-behaviour sanitizers and runs it:
 *   c++ -std=c++17 -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_png_pixels_plan tools/test_png_pixels_plan.cpp && ./test_png_pixels_plan
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_pixels_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

typedef unsigned __int128 u128;

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
static const unsigned formats[8] = { 1, 2, 3, 4, 0x11, 0x12, 0x13, 0x14 };
static const unsigned ch_of[7] = { 1, 0, 3, 1, 2, 0, 4 };

/* the table: for each pair the one format it already is (0: none) */
static const unsigned direct_format[15] = {
	0, 0, 0, 1, 0x11, 3, 0x13, 0, 0, 0, 0, 2, 0x12, 4, 0x14,
};

static uint64_t model_rowbytes(uint64_t width, unsigned depth, unsigned colour)
{
	return (uint64_t)(((u128)width * ch_of[colour] * depth + 7) / 8);
}

static unsigned model_bpp(unsigned depth, unsigned colour)
{
	const unsigned bits = ch_of[colour] * depth;
	return bits >= 8 ? bits / 8 : 1;
}

/* a good row of a file at `off`: signature, IHDR, [PLTE of 4], [tRNS of
 * trns_n bytes; trns_n < 0: none], one IDAT of zsum, IEND */
static void make_row(uint64_t *r, uint64_t off, uint64_t w, uint64_t h, unsigned depth,
		     unsigned colour, uint64_t zsum, int trns_n, uint64_t *n_ret)
{
	uint64_t pos = off + 33;
	r[6] = r[7] = 0;
	if (colour == 3) {
		r[6] = (pos + 8) | (uint64_t)4 << 48;
		pos += 12 + 12;
	}
	if (trns_n >= 0) {
		r[7] = (pos + 8) | (uint64_t)trns_n << 48;
		pos += 12 + trns_n;
	}
	r[2] = w | h << 32;
	r[3] = depth | colour << 8 | (uint64_t)model_bpp(depth, colour) << 24 |
	       (uint64_t)ch_of[colour] << 32;
	r[4] = pos;
	r[5] = zsum;
	pos += 12 + zsum + 12;
	r[0] = off;
	r[1] = pos - off;
	*n_ret = pos;
}

static void test_formats_and_routing(void)
{
	unsigned ok = 0;
	for (unsigned f = 0; f < 0x100; f++)
		ok += pngx_format_ok(f);
	CHECK(ok == 8);
	for (unsigned f : formats)
		CHECK(pngx_format_ok(f));
	CHECK(!pngx_format_ok(0) && !pngx_format_ok(5) && !pngx_format_ok(0x20) &&
	      !pngx_format_ok(0x13 | 0x40) && !pngx_format_ok(0x10) && !pngx_format_ok(0x113) &&
	      !pngx_format_ok(0x80000003u));
	const uint64_t sel0 = 0;
	for (int c = 0; c < 15; c++) {
		for (unsigned f : formats) {
			for (int trns = 0; trns < 2; trns++) {
				const unsigned depth = combos[c][0], colour = combos[c][1];
				const bool want = direct_format[c] == f;
				CHECK(pngx_direct(depth, colour, f) == want);
				/* and through the plan: which column holds the count */
				uint64_t row[8], n, offs[2];
				PngxPlan plan;
				std::vector<uint64_t> cols;
				std::string err;
				const int trns_n = !trns ? -1 : colour == 2 ? 6 : 2;
				make_row(row, 7, 21, 5, depth, colour, 40, trns_n, &n);
				CHECK(png_pixels_plan(row, 1, 1, &sel0, f, n, 1 << 20, 0, 0, cols, offs,
						      &plan, err));
				const uint64_t rb = model_rowbytes(21, depth, colour);
				const uint64_t raw_n = 5 * (rb + 1);
				const uint64_t *cc = cols.data() + plan.conv_at;
				CHECK(plan.n_conv == !want && plan.conv_at == PNG_COLS);
				/* a direct batch uploads what png_plan_decode() uploads */
				CHECK(cols.size() == PNG_COLS + (want ? 0 : PNGX_CCOLS));
				CHECK(cols[PNG_COL_RAW_N] == raw_n);
				CHECK(!!(cols[PNG_COL_META] & PNGX_META_ALT) == !want);
				CHECK(plan.tiles == (want ? 0 : 1));
				CHECK(offs[1] == 21 * 5 * (f & 0xF) * (f & 0x10 ? 2 : 1));
				const uint64_t areas = 48 + (raw_n + 15) / 16 * 16;
				CHECK(plan.scratch == areas + (want ? 0 : (5 * rb + 15) / 16 * 16));
				CHECK(cols[PNG_COL_OUT_OFF] == (want ? 0 : areas));
				if (!want) {
					const bool key = trns && (colour == 0 || colour == 2);
					CHECK(cc[PNGX_C_SEL] == 0 && cc[PNGX_C_DST] == 0 && cc[PNGX_C_TILE_END] == 1);
					CHECK(cc[PNGX_C_SHAPE] == (21 | 5ull << 32));
					CHECK(!!(cc[PNGX_C_KIND] & PNGX_KIND_KEY) == key);
					CHECK((cc[PNGX_C_KIND] & 0xFFFF) == (depth | colour << 8));
					CHECK(cc[PNGX_C_PLTE] == (colour == 3 ? row[6] : 0));
					CHECK(cc[PNGX_C_KIND] >> 32 == (colour == 3 && trns ? 2 : 0));
					CHECK(cc[PNGX_C_TRNS] == (key || (colour == 3 && trns) ? row[7] : 0));
					CHECK(cols[PNG_COL_META] == (model_bpp(depth, colour) | PNGX_META_ALT));
				}
			}
		}
	}
	/* a tRNS of another length is no key, one on colour types 4 and 6 neither */
	uint64_t row[8], n;
	for (int len : { 0, 1, 3, 6, 7 }) {
		make_row(row, 0, 3, 3, 8, 0, 10, len, &n);
		CHECK(!pngx_has_key(row, 0));
	}
	make_row(row, 0, 3, 3, 8, 2, 10, 2, &n);
	CHECK(!pngx_has_key(row, 2));
	make_row(row, 0, 3, 3, 8, 2, 10, 6, &n);
	CHECK(pngx_has_key(row, 2) && !pngx_has_key(row, 6) && !pngx_has_key(row, 4));
	make_row(row, 0, 3, 3, 8, 0, 10, 2, &n);
	CHECK(pngx_has_key(row, 0) && !pngx_has_key(row, 4));
	row[7] = 0;
	CHECK(!pngx_has_key(row, 0));
}

static void test_sizes(void)
{
	uint64_t row[8], n, offs[3], total;
	const uint64_t sel[2] = { 0, 0 };
	std::string err;

	/* 1-bit grey, 2^17 x 2^17: 2^31 + 2^17 raw bytes, 2^37 bytes of RGBA16 */
	make_row(row, 0, 1 << 17, 1 << 17, 1, 0, 10, -1, &n);
	for (unsigned f : formats) {
		const u128 want = (u128)(1 << 17) * (1 << 17) * (f & 0xF) * (f & 0x10 ? 2 : 1);
		CHECK(png_pixels_plan_out_sizes(row, 1, 2, sel, f, 0, offs, &total, err));
		CHECK(offs[0] == 0 && (u128)offs[1] == want && (u128)total == 2 * want);
	}
	CHECK(total == (uint64_t)1 << 38);
	/* the widest row there is */
	make_row(row, 0, 0x7FFFFFFF, 1, 1, 0, 10, -1, &n);
	CHECK(png_pixels_plan_out_sizes(row, 1, 1, sel, 0x14, 255, offs, &total, err));
	CHECK((u128)total == ((u128)0x7FFFFFFF * 8 + 255) / 256 * 256);
	make_row(row, 0, 0x7FFFFFFF, 1, 16, 6, 10, -1, &n);	/* 2^34 raw bytes: refused */
	CHECK(!png_pixels_plan_out_sizes(row, 1, 1, sel, 0x14, 0, offs, &total, err));
	/* the plan takes the large image where out_avail holds it, to the byte */
	make_row(row, 0, 1 << 17, 1 << 17, 1, 0, 10, -1, &n);
	std::vector<uint64_t> cols;
	PngxPlan plan;
	CHECK(png_pixels_plan(row, 1, 1, sel, 0x14, n, (uint64_t)1 << 37, 0, 0, cols, offs, &plan,
			      err));
	CHECK(plan.tiles == (uint64_t)1 << 22 && offs[1] == (uint64_t)1 << 37);
	CHECK(!png_pixels_plan(row, 1, 1, sel, 0x14, n, ((uint64_t)1 << 37) - 1, 0, 0, cols, offs,
			       &plan, err));
	CHECK(err.find("out_avail") != std::string::npos);
	/* the sum of many large rooms stays inside 64 bits or is refused */
	uint64_t at = ~(uint64_t)0 - 5;
	CHECK(pngx_advance(&at, 5, err) && at == ~(uint64_t)0);
	CHECK(!pngx_advance(&at, 1, err));
	/* random shapes in 128 bits */
	for (int i = 0; i < 20000; i++) {
		const unsigned *c = combos[rnd() % 15];
		const uint64_t w = 1 + rnd() % 0x7FFFFFFF, h = 1 + rnd() % (rnd() % 2 ? 70000 : 3);
		const unsigned f = formats[rnd() % 8];
		const uint64_t mask = ((uint64_t)1 << rnd() % 9) - 1;
		make_row(row, 0, w, h, c[0], c[1], 10, -1, &n);
		const bool big = (u128)h * (model_rowbytes(w, c[0], c[1]) + 1) >= ((u128)1 << 32);
		const bool ok = png_pixels_plan_out_sizes(row, 1, 1, sel, f, mask, offs, &total, err);
		CHECK(ok == !big);
		if (ok) {
			const u128 px = (u128)w * h * (f & 0xF) * (f & 0x10 ? 2 : 1);
			CHECK((u128)total == (px + mask) / (mask + 1) * (mask + 1));
		}
	}
}

static void test_refusals(void)
{
	uint64_t row[8], n, offs[2];
	const uint64_t sel0 = 0;
	std::vector<uint64_t> cols;
	std::string err;
	PngxPlan plan;

	make_row(row, 100, 65, 67, 8, 3, 500, 3, &n);
#define PLAN(r, fmt, in_n, avail, mask) \
	png_pixels_plan(r, 1, 1, &sel0, fmt, in_n, avail, mask, 0, cols, offs, &plan, err)
	CHECK(PLAN(row, 3, n, 65 * 67 * 3, 0));
	CHECK(!PLAN(row, 3, n, 65 * 67 * 3 - 1, 0) && err.find("out_avail") != std::string::npos);
	CHECK(PLAN(row, 3, n, 13312, 255) && !PLAN(row, 3, n, 13311, 255));
	for (unsigned f : { 0u, 5u, 0x20u, 0x13u | 0x40u, 0x10u, 0x1Fu }) {
		CHECK(!PLAN(row, f, n, 1 << 30, 0) && err.find("format") != std::string::npos);
		CHECK(cols.empty());
		CHECK(!png_pixels_plan_out_sizes(row, 1, 1, &sel0, f, 0, offs, NULL, err));
		CHECK(err.find("format") != std::string::npos);
	}
	CHECK(!PLAN(row, 3, n - 1, 1 << 30, 0));	/* the file passes in_nbytes */
#define REFUSED(change) do { uint64_t t[8]; memcpy(t, row, sizeof(t)); change; err.clear(); \
		CHECK(!PLAN(t, 3, n, ~(uint64_t)0, 0)); CHECK(!err.empty()); } while (0)
	REFUSED(t[0] = n + 1);
	REFUSED(t[1] = n);
	REFUSED(t[2] = 67ull << 32);			/* width 0 */
	REFUSED(t[2] = 65);				/* height 0 */
	REFUSED(t[2] = 0x80000000ull | 67ull << 32);
	REFUSED(t[3] = (t[3] & ~0xFFull) | 16);		/* a palette of depth 16 */
	REFUSED(t[3] = (t[3] & ~0xFF00ull) | 5 << 8);	/* colour 5 */
	REFUSED(t[3] |= 1 << 16);			/* interlaced */
	CHECK(err.find("interlaced") != std::string::npos);
	REFUSED(t[3] = (t[3] & ~(0xFFull << 24)) | 4ull << 24);	/* a wrong filter unit */
	REFUSED(t[3] = (t[3] & 0xFFFFFFFFull) | 4ull << 32);	/* wrong channels */
	REFUSED(t[2] = 65536ull | 65536ull << 32);	/* 2^32 raw bytes and more */
	REFUSED(t[4] = 100 + 32);			/* inside the IHDR */
	REFUSED(t[4] = n - 11);
	REFUSED(t[5] = n - 12 - t[4] + 1);		/* the sum passes the file */
	REFUSED(t[6] = 0);				/* a palette image without a PLTE */
	REFUSED(t[6] = (100 + 33 + 8) | 257ull << 48);
	REFUSED(t[6] = (n - 3) | 1ull << 48);
	REFUSED(t[7] = (n - 3) | 1ull << 48);
	REFUSED(t[7] = (n + 5) | 0ull << 48);
	/* selections */
	const uint64_t bad_sel = 1;
	CHECK(!png_pixels_plan(row, 1, 1, &bad_sel, 3, n, 1 << 30, 0, 0, cols, offs, &plan, err));
	CHECK(err.find("sel[0]") != std::string::npos);
	CHECK(!png_pixels_plan_out_sizes(row, 1, 1, &bad_sel, 3, 0, offs, NULL, err));
	/* nothing selected */
	CHECK(png_pixels_plan(NULL, 0, 0, NULL, 3, 0, 0, 0, 0, cols, offs, &plan, err));
	CHECK(offs[0] == 0 && plan.scratch == 0 && plan.tiles == 0 && plan.n_conv == 0 &&
	      cols.empty());
	/* out_sizes reads words 2 and 3 alone */
	{
		uint64_t t[8];
		memcpy(t, row, sizeof(t));
		t[0] = ~(uint64_t)0;
		t[6] = 0;
		CHECK(png_pixels_plan_out_sizes(t, 1, 1, &sel0, 0x14, 0, offs, NULL, err));
		CHECK(offs[1] == 65 * 67 * 8);
		t[3] |= 1 << 16;
		CHECK(!png_pixels_plan_out_sizes(t, 1, 1, &sel0, 0x14, 0, offs, NULL, err));
	}
}

static void test_selections(void)
{
	static const uint64_t dims[] = { 1, 2, 15, 16, 17, 33, 63, 64, 65, 130, 500 };
	const size_t entries = 200;
	std::vector<uint64_t> rows(PNG_ROW_WORDS * entries);
	struct Shape { uint64_t w, h, rb; unsigned depth, colour, bpp; bool zero; };
	std::vector<Shape> shapes(entries);
	uint64_t pos = 0;
	for (size_t k = 0; k < entries; k++) {
		uint64_t *r = &rows[PNG_ROW_WORDS * k];
		const unsigned *c = combos[rnd() % 15];
		const uint64_t w = dims[rnd() % 11], h = dims[rnd() % 11];
		pos += rnd() % 7;	/* unaligned files */
		make_row(r, pos, w, h, c[0], c[1], rnd() % 3000, rnd() % 2 ? (int)(rnd() % 8) : -1, &pos);
		shapes[k] = { w, h, model_rowbytes(w, c[0], c[1]), c[0], c[1], model_bpp(c[0], c[1]),
			      rnd() % 5 == 0 };
		if (shapes[k].zero)
			memset(r + 2, 0, 6 * sizeof(uint64_t));
	}
	for (uint64_t align = 1; align <= 256; align *= 2) {
		for (unsigned f : formats) {
			const unsigned flags = (unsigned)(rnd() % 2);
			const size_t n_sel = 1 + rnd() % 300;
			std::vector<uint64_t> sel(n_sel), offs(n_sel + 1), offs2(n_sel + 1), cols;
			for (auto &v : sel)
				v = rnd() % entries;	/* duplicates among them */
			sel[n_sel / 2] = sel[0];
			std::string err;
			uint64_t total = 0;
			PngxPlan plan;
			/* the model: one selection behind the other */
			const unsigned opp = (f & 0xF) * (f & 0x10 ? 2 : 1);
			uint64_t at = 0, z_at = 0, raw_at = 0, pix_at = 0, t_at = 0, n_conv = 0;
			std::vector<uint64_t> m_out(n_sel), m_z(n_sel), m_raw(n_sel), m_pix(n_sel), m_t(n_sel),
				m_c(n_sel);
			std::vector<bool> m_direct(n_sel);
			for (size_t r = 0; r < n_sel; r++) {
				const Shape &s = shapes[sel[r]];
				m_out[r] = at;
				m_z[r] = z_at;
				m_raw[r] = raw_at;
				m_pix[r] = pix_at;
				m_c[r] = n_conv;
				if (s.zero)
					continue;
				m_direct[r] = s.colour != 3 && ch_of[s.colour] * s.depth == 8 * opp &&
					      s.depth == (f & 0x10 ? 16u : 8u);
				at += (s.w * s.h * opp + align - 1) / align * align;
				z_at += (rows[PNG_ROW_WORDS * sel[r] + 5] + 15) / 16 * 16;
				raw_at += (s.h * (s.rb + 1) + 15) / 16 * 16;
				if (!m_direct[r]) {
					pix_at += (s.h * s.rb + 15) / 16 * 16;
					for (uint64_t p = 0; p < s.w * s.h; p += PNGX_TILE)
						t_at++;
					n_conv++;
				}
				m_t[r] = t_at;
			}
			CHECK(png_pixels_plan_out_sizes(rows.data(), entries, n_sel, sel.data(), f, align - 1,
							offs2.data(), &total, err));
			CHECK(total == at && offs2[n_sel] == at);
			CHECK(!png_pixels_plan(rows.data(), entries, n_sel, sel.data(), f, pos, at ? at - 1 : 0,
					       align - 1, flags, cols, offs.data(), &plan, err) || at == 0);
			CHECK(png_pixels_plan(rows.data(), entries, n_sel, sel.data(), f, pos, at, align - 1,
					      flags, cols, offs.data(), &plan, err));
			CHECK(offs == offs2 && plan.scratch == z_at + raw_at + pix_at && plan.tiles == t_at);
			CHECK(plan.n_conv == n_conv && plan.conv_at == PNG_COLS * n_sel);
			CHECK(cols.size() == plan.conv_at + PNGX_CCOLS * n_conv);
			const uint64_t scratch = plan.scratch;
			for (size_t r = 0; r < n_sel; r++) {
				const Shape &s = shapes[sel[r]];
				const uint64_t *row = &rows[PNG_ROW_WORDS * sel[r]];
				auto col = [&](int c) { return cols[c * n_sel + r]; };
				auto ccol = [&](int c) { return cols[plan.conv_at + c * n_conv + m_c[r]]; };
				CHECK(offs[r] == m_out[r]);
				CHECK(offs[r] % align == 0);
				if (s.zero) {
					CHECK(col(PNG_COL_META) == (uint64_t)PNG_UNSUPPORTED << 16);
					for (int c = 0; c < PNG_COLS; c++)
						CHECK(c == PNG_COL_META || c == PNG_COL_OUT_OFF || col(c) == 0);
					continue;
				}
				const uint64_t raw_n = s.h * (s.rb + 1);
				CHECK(col(PNG_COL_IDAT) == row[4] && col(PNG_COL_END) == row[0] + row[1]);
				CHECK(col(PNG_COL_ZSUM) == row[5] && col(PNG_COL_Z_OFF) == m_z[r]);
				CHECK(col(PNG_COL_RAW_OFF) == z_at + m_raw[r] && col(PNG_COL_RAW_N) == raw_n);
				CHECK(col(PNG_COL_GEOM) == (s.h | s.rb << 32));
				if (m_direct[r]) {
					CHECK(col(PNG_COL_OUT_OFF) == m_out[r]);
					CHECK(col(PNG_COL_META) == (s.bpp | (uint64_t)(flags && s.depth == 16) << 8));
					CHECK(s.h * s.rb == s.w * s.h * opp);	/* the room is the image */
				} else {
					CHECK(col(PNG_COL_OUT_OFF) == z_at + raw_at + m_pix[r]);
					CHECK(col(PNG_COL_OUT_OFF) + s.h * s.rb <= scratch);
					CHECK(col(PNG_COL_META) == (s.bpp | PNGX_META_ALT));
					CHECK(ccol(PNGX_C_SEL) == r && ccol(PNGX_C_DST) == m_out[r]);
					CHECK(ccol(PNGX_C_SHAPE) == (s.w | s.h << 32));
					CHECK(ccol(PNGX_C_TILE_END) == m_t[r]);
					CHECK((ccol(PNGX_C_KIND) & 0xFFFF) == (s.depth | s.colour << 8));
				}
				/* the rooms end inside their areas */
				CHECK(col(PNG_COL_Z_OFF) + row[5] <= z_at);
				CHECK(col(PNG_COL_RAW_OFF) + raw_n <= z_at + raw_at);
				CHECK(offs[r] + s.w * s.h * opp <= offs[r + 1]);
			}
		}
	}
}

int main(void)
{
	test_formats_and_routing();
	test_sizes();
	test_refusals();
	test_selections();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("png pixels plan ok\n");
	return 0;
}
