/*
 * test_png_adam7_plan.cpp - the host arithmetic of
 * libdeflate_amd_png_out_sizes_ex and libdeflate_amd_png_decode_batch_ex
 * (csrc/png_adam7_plan.h) on the CPU: the geometry of the seven passes against
 * a walk over every pixel of the grid for all widths and heights in 1 .. 17
 * and all 15 depth and colour pairs, raw7 and its 2^32 edge in 128-bit
 * arithmetic, every refusal with and without the flag, and the units, the
 * rooms of the four scratch areas, the convert and the deinterlace columns
 * and both tile prefixes of mixed selections - interlaced, plain and zero rows,
 * duplicates - against a serial model for every out_align and format.
 * Stand-alone; tests/test_png_adam7_plan.py builds it under the address and
 * undefined-behaviour sanitizers and runs it:
 *   c++ -std=c++17 -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_png_adam7_plan tools/test_png_adam7_plan.cpp && ./test_png_adam7_plan
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_adam7_plan.h"

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
static const unsigned formats[9] = { 0, 1, 2, 3, 4, 0x11, 0x12, 0x13, 0x14 };
static const unsigned ch_of[7] = { 1, 0, 3, 1, 2, 0, 4 };

/* the model's pass of a pixel: the 8 x 8 pattern of the specification */
static const unsigned char pattern[8][8] = {
	{ 1, 6, 4, 6, 2, 6, 4, 6 }, { 7, 7, 7, 7, 7, 7, 7, 7 }, { 5, 6, 5, 6, 5, 6, 5, 6 },
	{ 7, 7, 7, 7, 7, 7, 7, 7 }, { 3, 6, 4, 6, 3, 6, 4, 6 }, { 7, 7, 7, 7, 7, 7, 7, 7 },
	{ 5, 6, 5, 6, 5, 6, 5, 6 }, { 7, 7, 7, 7, 7, 7, 7, 7 },
};

static unsigned model_bpp(unsigned depth, unsigned colour)
{
	const unsigned bits = ch_of[colour] * depth;
	return bits >= 8 ? bits / 8 : 1;
}

static u128 model_rowbytes(u128 width, unsigned depth, unsigned colour)
{
	return (width * ch_of[colour] * depth + 7) / 8;
}

/* w_p, h_p in closed form, 128 bits wide */
static void model_pass(u128 w, u128 h, unsigned p, u128 *wp, u128 *hp)
{
	static const unsigned x0[7] = { 0, 4, 0, 2, 0, 1, 0 }, y0[7] = { 0, 0, 4, 0, 2, 0, 1 };
	static const unsigned dx[7] = { 8, 8, 4, 4, 2, 2, 1 }, dy[7] = { 8, 8, 8, 4, 4, 2, 2 };
	*wp = w > x0[p] ? (w - x0[p] + dx[p] - 1) / dx[p] : 0;
	*hp = h > y0[p] ? (h - y0[p] + dy[p] - 1) / dy[p] : 0;
	if (!*wp || !*hp)
		*wp = *hp = 0;
}

static u128 model_raw7(u128 w, u128 h, unsigned depth, unsigned colour)
{
	u128 sum = 0;
	for (unsigned p = 0; p < 7; p++) {
		u128 wp, hp;
		model_pass(w, h, p, &wp, &hp);
		if (hp)
			sum += hp * (1 + model_rowbytes(wp, depth, colour));
	}
	return sum;
}

/* a good row of a file at `off` (test_png_pixels_plan.cpp's), interlaced or not */
static void make_row(uint64_t *r, uint64_t off, uint64_t w, uint64_t h, unsigned depth,
		     unsigned colour, uint64_t zsum, int trns_n, bool il, uint64_t *n_ret)
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
	r[3] = depth | colour << 8 | (uint64_t)il << 16 | (uint64_t)model_bpp(depth, colour) << 24 |
	       (uint64_t)ch_of[colour] << 32;
	r[4] = pos;
	r[5] = zsum;
	pos += 12 + zsum + 12;
	r[0] = off;
	r[1] = pos - off;
	*n_ret = pos;
}

static void test_geometry(void)
{
	for (uint64_t w = 1; w <= 17; w++) {
		for (uint64_t h = 1; h <= 17; h++) {
			/* the walk: count every pass's columns and rows */
			uint64_t cols[8][17] = { { 0 } }, rows[8][17] = { { 0 } };
			for (uint64_t y = 0; y < h; y++)
				for (uint64_t x = 0; x < w; x++) {
					const unsigned p = pattern[y % 8][x % 8];
					cols[p][x] = 1;
					rows[p][y] = 1;
				}
			for (int c = 0; c < 15; c++) {
				const unsigned depth = combos[c][0], colour = combos[c][1];
				Png7Pass pass[7];
				uint64_t raw7 = 0, want = 0;
				png7_passes(w, h, depth, colour, pass);
				for (unsigned p = 0; p < 7; p++) {
					uint64_t wp = 0, hp = 0;
					for (unsigned i = 0; i < 17; i++) {
						wp += cols[p + 1][i];
						hp += rows[p + 1][i];
					}
					CHECK(pass[p].w == wp && pass[p].h == hp);
					CHECK(pass[p].rb == (wp * ch_of[colour] * depth + 7) / 8);
					u128 mw, mh;
					model_pass(w, h, p, &mw, &mh);
					CHECK((u128)wp == mw && (u128)hp == mh);
					want += hp * (1 + pass[p].rb);
				}
				CHECK(png7_raw_bytes(pass, &raw7) && raw7 == want);
				CHECK((u128)raw7 == model_raw7(w, h, depth, colour));
			}
		}
	}
	/* the first pixel of pass p, and the pixel in front of it */
	CHECK(pattern[0][4] == 2 && pattern[4][0] == 3 && pattern[0][2] == 4 && pattern[2][0] == 5);
}

static void test_sizes(void)
{
	uint64_t row[8], n, offs[3], total;
	const uint64_t sel[2] = { 0, 0 };
	std::string err;

	/* raw7 passes 2^32 where the image does not: width 2, 3.5 against 3 bytes a row */
	int taken = 0, refused = 0;
	for (uint64_t h = 1227133500ull; h <= 1431655764ull; h += h < 1227133530ull ? 1 : 20452223ull) {
		make_row(row, 0, 2, h, 8, 0, 10, -1, true, &n);
		const bool big = model_raw7(2, h, 8, 0) >= ((u128)1 << 32);
		CHECK((u128)h * 3 < ((u128)1 << 32));
		CHECK(png7_plan_out_sizes(row, 1, 1, sel, 0, 0, PNG_ADAM7, offs, &total, err) == !big);
		if (big)
			CHECK(err.find("2^32") != std::string::npos);
		else
			CHECK(total == 2 * h);
		taken += !big;
		refused += big;
		/* its twin is taken either way */
		row[3] &= ~(1ull << 16);
		CHECK(png7_plan_out_sizes(row, 1, 1, sel, 0, 0, PNG_ADAM7, offs, &total, err));
	}
	CHECK(taken > 5 && refused > 10);	/* the edge lies inside the heights walked */
	/* the image itself at 2^32, and sizes whose products pass 2^64 */
	make_row(row, 0, 65536, 16384, 8, 6, 10, -1, true, &n);
	CHECK(!png7_plan_out_sizes(row, 1, 1, sel, 0, 0, PNG_ADAM7, offs, &total, err));
	make_row(row, 0, 0x7FFFFFFF, 0x7FFFFFFF, 16, 6, 10, -1, true, &n);
	CHECK(!png7_plan_out_sizes(row, 1, 1, sel, 0x14, 0, PNG_ADAM7, offs, &total, err));
	{
		Png7Pass pass[7];
		uint64_t raw7;
		png7_passes(0x7FFFFFFF, 0x7FFFFFFF, 16, 6, pass);
		CHECK(!png7_raw_bytes(pass, &raw7));
	}
	/* 1-bit grey, 2^17 x 2^17 interlaced: 2^37 bytes of RGBA16, twice */
	make_row(row, 0, 1 << 17, 1 << 17, 1, 0, 10, -1, true, &n);
	CHECK(png7_plan_out_sizes(row, 1, 2, sel, 0x14, 0, PNG_ADAM7, offs, &total, err));
	CHECK(total == (uint64_t)1 << 38 && offs[1] == (uint64_t)1 << 37);
	CHECK(png7_plan_out_sizes(row, 1, 2, sel, 0, 0, PNG_ADAM7, offs, &total, err));
	CHECK(total == (uint64_t)1 << 32);
	/* random shapes in 128 bits */
	for (int i = 0; i < 20000; i++) {
		const unsigned *c = combos[rnd() % 15];
		const uint64_t w = 1 + rnd() % (rnd() % 2 ? 0x7FFFFFFF : 9);
		const uint64_t h = 1 + rnd() % (rnd() % 3 == 0 ? 0x7FFFFFFF : rnd() % 2 ? 70000 : 9);
		const unsigned f = formats[rnd() % 9];
		const uint64_t mask = ((uint64_t)1 << rnd() % 9) - 1;
		const bool il = rnd() % 2;
		make_row(row, 0, w, h, c[0], c[1], 10, -1, il, &n);
		const u128 rb = model_rowbytes(w, c[0], c[1]);
		const bool big = (u128)h * (rb + 1) >= ((u128)1 << 32) ||
				 (il && model_raw7(w, h, c[0], c[1]) >= ((u128)1 << 32));
		const bool ok = png7_plan_out_sizes(row, 1, 1, sel, f, mask, PNG_ADAM7, offs, &total, err);
		CHECK(ok == !big);
		if (ok) {
			const u128 px = f ? (u128)w * h * (f & 0xF) * (f & 0x10 ? 2 : 1) : (u128)h * rb;
			CHECK((u128)total == (px + mask) / (mask + 1) * (mask + 1));
		}
		/* without the flag: the older functions' answer */
		uint64_t total2 = 0, offs2[3];
		std::string err2;
		const bool ok0 = png7_plan_out_sizes(row, 1, 1, sel, f, mask, 0, offs, &total, err);
		const bool old = f ? png_pixels_plan_out_sizes(row, 1, 1, sel, f, mask, offs2, &total2, err2) :
				     png_plan_out_sizes(row, 1, 1, sel, mask, offs2, &total2, err2);
		CHECK(ok0 == old && (!old || total == total2) && (old || err == err2));
		CHECK(!il || !ok0);
	}
}

static void test_refusals(void)
{
	uint64_t row[8], n, offs[2];
	const uint64_t sel0 = 0;
	std::vector<uint64_t> cols;
	std::string err;
	Png7Plan plan;

	make_row(row, 100, 65, 67, 8, 3, 500, 3, true, &n);
#define PLAN(r, fmt, in_n, avail, mask, fl) \
	png7_plan(r, 1, 1, &sel0, fmt, in_n, avail, mask, fl, cols, offs, &plan, err)
	CHECK(PLAN(row, 3, n, 65 * 67 * 3, 0, PNG_ADAM7));
	CHECK(PLAN(row, 0, n, 65 * 67, 0, PNG_ADAM7 | PNG_LE16));
	CHECK(!PLAN(row, 0, n, 65 * 67 - 1, 0, PNG_ADAM7) && err.find("out_avail") != std::string::npos);
	CHECK(!PLAN(row, 3, n, 65 * 67 * 3 - 1, 0, PNG_ADAM7) && err.find("out_avail") != std::string::npos);
	CHECK(PLAN(row, 3, n, 13312, 255, PNG_ADAM7) && !PLAN(row, 3, n, 13311, 255, PNG_ADAM7));
	/* interlaced without the flag: the existing word */
	for (unsigned fl : { 0u, (unsigned)PNG_LE16 }) {
		CHECK(!PLAN(row, 3, n, 1 << 30, 0, fl) && err.find("interlaced") != std::string::npos);
		CHECK(err.find("row 0") != std::string::npos);
		CHECK(!png7_plan_out_sizes(row, 1, 1, &sel0, 0, 0, fl, offs, NULL, err));
		CHECK(err.find("interlaced") != std::string::npos);
	}
	for (unsigned f : { 5u, 0x20u, 0x13u | 0x40u, 0x10u, 0x1Fu }) {
		CHECK(!PLAN(row, f, n, 1 << 30, 0, PNG_ADAM7) && err.find("format") != std::string::npos);
		CHECK(cols.empty());
		CHECK(!png7_plan_out_sizes(row, 1, 1, &sel0, f, 0, PNG_ADAM7, offs, NULL, err));
		CHECK(err.find("format") != std::string::npos);
	}
	CHECK(!PLAN(row, 3, n - 1, 1 << 30, 0, PNG_ADAM7));	/* the file passes in_nbytes */
	CHECK(err.find("in_nbytes") != std::string::npos);
#define REFUSED(change, word) do { uint64_t t[8]; memcpy(t, row, sizeof(t)); change; err.clear(); \
		CHECK(!PLAN(t, 3, n, ~(uint64_t)0, 0, PNG_ADAM7)); \
		CHECK(err.find(word) != std::string::npos); } while (0)
	REFUSED(t[0] = n + 1, "file");
	REFUSED(t[1] = n, "file");
	REFUSED(t[2] = 67ull << 32, "width");
	REFUSED(t[2] = 65, "width");
	REFUSED(t[2] = 0x80000000ull | 67ull << 32, "width");
	REFUSED(t[3] = (t[3] & ~0xFFull) | 16, "bit depth");
	REFUSED(t[3] = (t[3] & ~0xFF00ull) | 5 << 8, "bit depth");
	REFUSED(t[3] = (t[3] & ~(0xFFull << 16)) | 2 << 16, "interlace");
	REFUSED(t[3] = (t[3] & ~(0xFFull << 24)) | 4ull << 24, "filter unit");
	REFUSED(t[3] = (t[3] & 0xFFFFFFFFull) | 4ull << 32, "channel");
	REFUSED(t[2] = 65536ull | 65536ull << 32, "2^32");
	REFUSED(t[4] = 100 + 32, "IDAT");
	REFUSED(t[4] = n - 11, "IDAT");
	REFUSED(t[5] = n - 12 - t[4] + 1, "IDAT");
	REFUSED(t[6] = 0, "PLTE");
	REFUSED(t[6] = (100 + 33 + 8) | 257ull << 48, "PLTE");
	REFUSED(t[6] = (n - 3) | 1ull << 48, "PLTE");
	REFUSED(t[7] = (n - 3) | 1ull << 48, "tRNS");
	REFUSED(t[7] = (n + 5) | 0ull << 48, "tRNS");
	/* raw7 at 2^32 where the image is below it */
	{
		uint64_t t[8], m;
		make_row(t, 0, 2, 1300000000ull, 8, 0, 10, -1, true, &m);
		CHECK(!PLAN(t, 0, m, ~(uint64_t)0, 0, PNG_ADAM7) && err.find("2^32") != std::string::npos);
		t[3] &= ~(1ull << 16);
		CHECK(PLAN(t, 0, m, ~(uint64_t)0, 0, PNG_ADAM7));
	}
	/* selections */
	const uint64_t bad_sel = 1;
	CHECK(!png7_plan(row, 1, 1, &bad_sel, 3, n, 1 << 30, 0, PNG_ADAM7, cols, offs, &plan, err));
	CHECK(err.find("sel[0]") != std::string::npos);
	CHECK(!png7_plan_out_sizes(row, 1, 1, &bad_sel, 3, 0, PNG_ADAM7, offs, NULL, err));
	/* nothing selected */
	CHECK(png7_plan(NULL, 0, 0, NULL, 0, 0, 0, 0, PNG_ADAM7, cols, offs, &plan, err));
	CHECK(offs[0] == 0 && plan.scratch == 0 && plan.n_units == 0 && plan.n_il == 0 &&
	      plan.n_conv == 0 && plan.il_tiles == 0 && cols.empty());
	/* the 2^48 limit of the scratch: many copies of a large interlaced image */
	{
		uint64_t t[8], m;
		make_row(t, 0, 1 << 17, 1 << 17, 1, 0, 10, -1, true, &m);
		const size_t many = (size_t)1 << 18;	/* x 2^31 bytes of pass images: 2^49 */
		std::vector<uint64_t> sel(many, 0), o(many + 1);
		CHECK(!png7_plan(t, 1, many, sel.data(), 0, m, ~(uint64_t)0, 0, PNG_ADAM7, cols, o.data(),
				 &plan, err));
		CHECK(err.find("2^48") != std::string::npos);
	}
}

static void test_selections(void)
{
	static const uint64_t dims[] = { 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 130, 500 };
	const size_t entries = 200, ndims = sizeof(dims) / sizeof(dims[0]);
	std::vector<uint64_t> rows(PNG_ROW_WORDS * entries);
	struct Shape { uint64_t w, h, rb; unsigned depth, colour, bpp; bool zero, il; };
	std::vector<Shape> shapes(entries);
	uint64_t pos = 0;
	for (size_t k = 0; k < entries; k++) {
		uint64_t *r = &rows[PNG_ROW_WORDS * k];
		const unsigned *c = combos[rnd() % 15];
		const uint64_t w = dims[rnd() % ndims], h = dims[rnd() % ndims];
		const bool il = rnd() % 2;
		pos += rnd() % 7;	/* unaligned files */
		make_row(r, pos, w, h, c[0], c[1], rnd() % 3000, rnd() % 2 ? (int)(rnd() % 8) : -1, il, &pos);
		shapes[k] = { w, h, (uint64_t)model_rowbytes(w, c[0], c[1]), c[0], c[1], model_bpp(c[0], c[1]),
			      rnd() % 5 == 0, il };
		if (shapes[k].zero)
			memset(r + 2, 0, 6 * sizeof(uint64_t));
	}
	for (uint64_t align = 1; align <= 256; align *= 2) {
		for (unsigned f : formats) {
			const unsigned flags = (unsigned)(rnd() % 2) | PNG_ADAM7;
			const size_t n_sel = 1 + rnd() % 300;
			std::vector<uint64_t> sel(n_sel), offs(n_sel + 1), offs2(n_sel + 1), cols;
			for (auto &v : sel)
				v = rnd() % entries;	/* duplicates among them */
			sel[n_sel / 2] = sel[0];
			std::string err;
			uint64_t total = 0;
			Png7Plan plan;
			/* the model: one selection behind the other, one area behind the other */
			const unsigned opp = (f & 0xF) * (f & 0x10 ? 2 : 1);
			struct Unit { uint64_t raw, raw_n, out, geom, meta; int area; };
			struct Conv { uint64_t sel, dst, tiles; };
			struct Il { uint64_t pass[7], dst, tiles; size_t sel; bool alt; };
			std::vector<Unit> m_units;
			std::vector<Conv> m_conv;
			std::vector<Il> m_il;
			std::vector<uint64_t> m_out(n_sel), m_z(n_sel), m_raw(n_sel), m_pix(n_sel),
				m_u0(n_sel), m_un(n_sel);
			std::vector<bool> m_direct(n_sel);
			uint64_t at = 0, z_at = 0, raw_at = 0, pass_at = 0, pix_at = 0, ct = 0, dt = 0;
			for (size_t r = 0; r < n_sel; r++) {
				const Shape &s = shapes[sel[r]];
				m_out[r] = at;
				m_z[r] = z_at;
				m_raw[r] = raw_at;
				m_pix[r] = pix_at;
				m_u0[r] = m_units.size();
				if (s.zero)
					continue;
				const bool direct = !f || (s.colour != 3 && ch_of[s.colour] * s.depth == 8 * opp &&
							   s.depth == (f & 0x10 ? 16u : 8u));
				const uint64_t le = (uint64_t)(direct && (flags & 1) && s.depth == 16) << 8;
				const uint64_t alt = direct ? 0 : PNGX_META_ALT;
				m_direct[r] = direct;
				uint64_t raw_n;
				if (!s.il) {
					raw_n = s.h * (s.rb + 1);
					m_units.push_back({ raw_at, raw_n, direct ? at : pix_at, s.h | s.rb << 32,
							    s.bpp | le | alt, direct ? 0 : 2 });
				} else {
					Il d;
					uint64_t in_raw = 0;
					for (unsigned p = 0; p < 7; p++) {
						u128 wp, hp;
						model_pass(s.w, s.h, p, &wp, &hp);
						const uint64_t rb = (uint64_t)model_rowbytes(wp, s.depth, s.colour);
						d.pass[p] = pass_at;
						if (!hp)
							continue;
						m_units.push_back({ raw_at + in_raw, (uint64_t)hp * (1 + rb), pass_at,
								    (uint64_t)hp | rb << 32, s.bpp | le | PNGX_META_ALT, 1 });
						in_raw += (uint64_t)hp * (1 + rb);
						pass_at += ((uint64_t)hp * rb + 15) / 16 * 16;
					}
					raw_n = in_raw;
					CHECK((u128)raw_n == model_raw7(s.w, s.h, s.depth, s.colour));
					for (uint64_t p = 0; p < s.h * ((s.rb + 15) / 16); p += PNG7_TILE)
						dt++;
					d.dst = direct ? at : pix_at;
					d.alt = !direct;
					d.tiles = dt;
					d.sel = r;
					m_il.push_back(d);
				}
				m_un[r] = m_units.size() - m_u0[r];
				if (!direct) {
					for (uint64_t p = 0; p < s.w * s.h; p += PNGX_TILE)
						ct++;
					m_conv.push_back({ r, at, ct });
					pix_at += (s.h * s.rb + 15) / 16 * 16;
				}
				at += ((f ? s.w * s.h * opp : s.h * s.rb) + align - 1) / align * align;
				z_at += (rows[PNG_ROW_WORDS * sel[r] + 5] + 15) / 16 * 16;
				raw_at += (raw_n + 15) / 16 * 16;
			}
			const uint64_t base[3] = { 0, z_at + raw_at, z_at + raw_at + pass_at };
			CHECK(png7_plan_out_sizes(rows.data(), entries, n_sel, sel.data(), f, align - 1, PNG_ADAM7,
						  offs2.data(), &total, err));
			CHECK(total == at && offs2[n_sel] == at);
			CHECK(!png7_plan(rows.data(), entries, n_sel, sel.data(), f, pos, at ? at - 1 : 0,
					 align - 1, flags, cols, offs.data(), &plan, err) || at == 0);
			CHECK(png7_plan(rows.data(), entries, n_sel, sel.data(), f, pos, at, align - 1, flags,
					cols, offs.data(), &plan, err));
			const size_t nu = m_units.size(), nc = m_conv.size(), ni = m_il.size();
			CHECK(offs == offs2 && plan.scratch == z_at + raw_at + pass_at + pix_at);
			CHECK(plan.n_units == nu && plan.n_conv == nc && plan.n_il == ni);
			CHECK(plan.conv_tiles == ct && plan.il_tiles == dt);
			CHECK(plan.units_at == PNG7_SCOLS * n_sel && plan.conv_at == plan.units_at + PNG7_UCOLS * nu);
			CHECK(plan.il_at == plan.conv_at + PNGX_CCOLS * nc);
			CHECK(cols.size() == plan.il_at + PNG7_DCOLS * ni);
			if (cols.size() != plan.il_at + PNG7_DCOLS * ni || plan.n_units != nu)
				continue;
			const uint64_t scratch = plan.scratch;
			for (size_t r = 0; r < n_sel; r++) {
				const Shape &s = shapes[sel[r]];
				const uint64_t *row = &rows[PNG_ROW_WORDS * sel[r]];
				auto col = [&](int c) { return cols[c * n_sel + r]; };
				CHECK(offs[r] == m_out[r] && offs[r] % align == 0);
				CHECK(col(PNG7_COL_UNITS) == (m_u0[r] | m_un[r] << 32));
				if (s.zero) {
					CHECK(col(PNG_COL_META) == (uint64_t)PNG_UNSUPPORTED << 16);
					for (int c = 0; c < PNG_COLS; c++)
						CHECK(c == PNG_COL_META || c == PNG_COL_OUT_OFF || col(c) == 0);
					continue;
				}
				CHECK(col(PNG_COL_IDAT) == row[4] && col(PNG_COL_END) == row[0] + row[1]);
				CHECK(col(PNG_COL_ZSUM) == row[5] && col(PNG_COL_Z_OFF) == m_z[r]);
				CHECK(col(PNG_COL_RAW_OFF) == z_at + m_raw[r]);
				CHECK(col(PNG_COL_RAW_N) ==
				      (s.il ? (uint64_t)model_raw7(s.w, s.h, s.depth, s.colour) : s.h * (s.rb + 1)));
				CHECK(col(PNG_COL_OUT_OFF) == (m_direct[r] ? m_out[r] : base[2] + m_pix[r]));
				CHECK(!(col(PNG_COL_META) >> 16));
				CHECK(col(PNG_COL_Z_OFF) + row[5] <= z_at);
				CHECK(col(PNG_COL_RAW_OFF) + col(PNG_COL_RAW_N) <= z_at + raw_at);
				CHECK(offs[r] + (f ? s.w * s.h * opp : s.h * s.rb) <= offs[r + 1]);
			}
			for (size_t u = 0; u < nu; u++) {
				auto ucol = [&](int c) { return cols[plan.units_at + c * nu + u]; };
				const Unit &m = m_units[u];
				CHECK(ucol(PNG7_U_RAW_OFF) == z_at + m.raw && ucol(PNG7_U_RAW_N) == m.raw_n);
				CHECK(ucol(PNG7_U_OUT_OFF) == base[m.area] + m.out);
				CHECK(ucol(PNG7_U_GEOM) == m.geom && ucol(PNG7_U_META) == m.meta);
				const uint64_t bytes = (m.geom & 0xFFFFFFFFull) * (m.geom >> 32);
				if (m.area)	/* inside the scratch, on a 16-byte boundary */
					CHECK(ucol(PNG7_U_OUT_OFF) + bytes <= scratch && ucol(PNG7_U_OUT_OFF) % 16 == 0);
				else
					CHECK(ucol(PNG7_U_OUT_OFF) + bytes <= at);
				CHECK(ucol(PNG7_U_RAW_OFF) + m.raw_n <= z_at + raw_at);
			}
			for (size_t c = 0; c < nc; c++) {
				auto ccol = [&](int a) { return cols[plan.conv_at + a * nc + c]; };
				const Shape &s = shapes[sel[m_conv[c].sel]];
				CHECK(ccol(PNGX_C_SEL) == m_conv[c].sel && ccol(PNGX_C_DST) == m_conv[c].dst);
				CHECK(ccol(PNGX_C_TILE_END) == m_conv[c].tiles);
				CHECK(ccol(PNGX_C_SHAPE) == (s.w | s.h << 32));
				CHECK((ccol(PNGX_C_KIND) & 0xFFFF) == (s.depth | s.colour << 8));
			}
			for (size_t i = 0; i < ni; i++) {
				auto dcol = [&](int a) { return cols[plan.il_at + a * ni + i]; };
				const Il &m = m_il[i];
				const Shape &s = shapes[sel[m.sel]];
				for (unsigned p = 0; p < 7; p++)
					CHECK(cols[plan.il_at + 7 * i + p] == base[1] + m.pass[p]);
				CHECK(dcol(PNG7_D_SHAPE) == (s.w | s.h << 32));
				CHECK(dcol(PNG7_D_KIND) == ((uint64_t)(s.depth * ch_of[s.colour]) |
							    (m.alt ? PNG7_KIND_ALT : 0) | s.rb << 16));
				CHECK(dcol(PNG7_D_DST) == (m.alt ? base[2] : 0) + m.dst);
				CHECK(dcol(PNG7_D_TILE_END) == m.tiles);
				/* the convert kernel reads where the deinterlace wrote */
				if (m.alt)
					CHECK(dcol(PNG7_D_DST) == cols[PNG_COL_OUT_OFF * n_sel + m.sel]);
			}
		}
	}
}

/* a batch without an interlaced row: the units are the older plan's columns */
static void test_plain_batches(void)
{
	uint64_t rows[3 * 8], n = 0;
	make_row(rows, 0, 21, 5, 16, 2, 40, -1, false, &n);
	make_row(rows + 8, n, 9, 70, 2, 3, 40, 2, false, &n);
	memset(rows + 16, 0, 8 * sizeof(uint64_t));
	const uint64_t sel[4] = { 1, 2, 0, 1 };
	for (unsigned f : formats) {
		std::vector<uint64_t> cols, old;
		uint64_t offs[5], offs2[5], scratch = 0;
		std::string err;
		Png7Plan plan;
		PngxPlan xplan;
		CHECK(png7_plan(rows, 3, 4, sel, f, n, 1 << 20, 15, PNG_LE16, cols, offs, &plan, err));
		if (f) {
			CHECK(png_pixels_plan(rows, 3, 4, sel, f, n, 1 << 20, 15, PNG_LE16, old, offs2, &xplan, err));
			scratch = xplan.scratch;
		} else {
			CHECK(png_plan_decode(rows, 3, 4, sel, n, 1 << 20, 15, PNG_LE16, old, offs2, &scratch, err));
		}
		CHECK(!memcmp(offs, offs2, sizeof(offs)) && plan.scratch == scratch && plan.n_il == 0);
		CHECK(plan.n_units == 3);
		for (int c = 0; c < PNG_COLS; c++)
			for (int r = 0; r < 4; r++)
				CHECK(cols[c * 4 + r] == old[c * 4 + r]);
	}
}

int main(void)
{
	test_geometry();
	test_sizes();
	test_refusals();
	test_selections();
	test_plain_batches();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("png adam7 plan ok\n");
	return 0;
}
