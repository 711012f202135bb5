/*
 * test_tar_plan.cpp - the host arithmetic of libdeflate_amd_tar_read_batch and
 * libdeflate_amd_tar_ranges (csrc/tar_plan.h) on the CPU: every refusal of a
 * row and of a selection, and the offsets, copy columns, tile counts and
 * ranges of random selections against a plain model, for every out_align.
 * Stand-alone; tests/test_tar_plan.py builds it under the address and
 * undefined-behaviour sanitizers and runs it:
 *   c++ -std=c++17 -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_tar_plan tools/test_tar_plan.cpp && ./test_tar_plan
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tar_plan.h"

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

/* rows of an archive of entries one behind the other; *n_ret its size */
static std::vector<uint64_t> make_rows(size_t entries, uint64_t *n_ret)
{
	static const char types[] = { '0', 0, '7', '5', '2', 'S', 'Z', 'M', 'D', '1' };
	static const uint64_t sizes[] = { 0, 1, 511, 512, 513, 65535, 65536, 65537, 196607, 300 };
	std::vector<uint64_t> rows(TAR_ROW_WORDS * entries);
	uint64_t pos = 0;
	for (size_t k = 0; k < entries; k++) {
		uint64_t *r = &rows[TAR_ROW_WORDS * k];
		const char t = types[rnd() % 10];
		const bool data = t == '0' || t == 0 || t == '7' || t == 'Z';
		r[0] = pos;
		r[1] = pos;
		r[2] = 1 + rnd() % 100;
		if (rnd() % 4 == 0)
			r[2] |= (1 + rnd() % 155) << 32;
		r[3] = (uint8_t)t;
		r[4] = pos + TAR_BLOCK;
		r[5] = data ? sizes[rnd() % 10] : 0;
		r[6] = rnd() % 100000;
		r[7] = rnd();	/* (not read) */
		pos += TAR_BLOCK + (r[5] + TAR_BLOCK - 1) / TAR_BLOCK * TAR_BLOCK;
	}
	*n_ret = pos;
	return rows;
}

static void test_selections(void)
{
	for (uint64_t align = 1; align <= 256; align *= 2) {
		uint64_t n;
		const size_t entries = 40;
		std::vector<uint64_t> rows = make_rows(entries, &n);
		for (int round = 0; round < 20; round++) {
			const size_t n_sel = rnd() % 60;
			std::vector<uint64_t> sel(n_sel), offs(n_sel + 1, 77), cols, rg(2 * n_sel + 1, 5);
			std::vector<int32_t> res;
			std::string err;
			for (auto &s : sel)
				s = rnd() % entries;
			/* the plain model */
			uint64_t at = 0, tiles = 0, sum = 0;
			std::vector<uint64_t> w_off, w_tile;
			for (size_t r = 0; r < n_sel; r++) {
				const uint64_t *row = &rows[TAR_ROW_WORDS * sel[r]];
				const char t = (char)row[3];
				const bool refused = t == 'S' || t == 'M' || t == 'D';
				w_off.push_back(at);
				w_tile.push_back(tiles);
				if (!refused) {
					at += (row[5] + align - 1) / align * align;
					tiles += (row[5] + 65535) / 65536;
					sum += row[5];
				}
			}
			uint64_t total = 0;
			CHECK(tar_plan_read(rows.data(), entries, n_sel, sel.data(), n, at, align - 1, cols,
					    res, offs.data(), &total, err));
			CHECK(total == at && offs[n_sel] == at && cols.size() == TAR_COLS * n_sel + 1);
			CHECK(cols[TAR_COLS * n_sel] == tiles);
			for (size_t r = 0; r < n_sel; r++) {
				const uint64_t *row = &rows[TAR_ROW_WORDS * sel[r]];
				const char t = (char)row[3];
				const bool refused = t == 'S' || t == 'M' || t == 'D';
				CHECK(offs[r] == w_off[r]);
				CHECK(res[r] == (refused ? TAR_UNSUPPORTED : 0));
				CHECK(cols[TAR_COL_TILE * n_sel + r] == w_tile[r]);
				CHECK(cols[TAR_COL_LEN * n_sel + r] == (refused ? 0 : row[5]));
				CHECK(cols[TAR_COL_SRC * n_sel + r] == (refused ? 0 : row[4]));
				CHECK(cols[TAR_COL_DST * n_sel + r] == (refused ? 0 : w_off[r]));
				CHECK(refused || w_off[r] % align == 0);
			}
			const std::vector<uint64_t> kept = cols;
			/* one byte less room */
			if (at) {
				CHECK(!tar_plan_read(rows.data(), entries, n_sel, sel.data(), n, at - 1,
						     align - 1, cols, res, NULL, NULL, err));
				CHECK(err.find("out_avail") != std::string::npos);
			}
			/* the ranges of the same selection */
			uint64_t rtotal = 1;
			CHECK(tar_plan_ranges(rows.data(), entries, n_sel, sel.data(), rg.data(), &rtotal,
					      err));
			CHECK(rtotal == sum && rg[2 * n_sel] == 5);
			for (size_t r = 0; r < n_sel; r++) {
				const uint64_t *row = &rows[TAR_ROW_WORDS * sel[r]];
				CHECK(rg[2 * r] == row[4]);
				CHECK(rg[2 * r + 1] == kept[TAR_COL_LEN * n_sel + r]);
			}
		}
	}
}

static bool refused_with(const std::vector<uint64_t> &rows, uint64_t entries, uint64_t s,
			 uint64_t n, const char *word, bool ranges_too)
{
	std::vector<uint64_t> cols, rg(2);
	std::vector<int32_t> res;
	std::string err;
	bool ok = !tar_plan_read(rows.data(), entries, 1, &s, n, ~(uint64_t)0, 0, cols, res, NULL,
				 NULL, err) &&
		  err.find(word) != std::string::npos;
	if (ranges_too) {
		err.clear();
		ok = ok && !tar_plan_ranges(rows.data(), entries, 1, &s, rg.data(), NULL, err) &&
		     err.find(word) != std::string::npos;
	}
	return ok;
}

static void test_refusals(void)
{
	uint64_t n;
	std::vector<uint64_t> rows = make_rows(4, &n);
	uint64_t *r = &rows[TAR_ROW_WORDS * 2];
	r[3] = '0';
	r[5] = 700;
	rows[TAR_ROW_WORDS * 3 + 0] = r[0] + 512 + 1024;
	n = r[0] + 512 + 1024;
	const std::vector<uint64_t> good = rows;
	std::vector<uint64_t> cols;
	std::vector<int32_t> res;
	std::string err;
	uint64_t s = 2;

	CHECK(tar_plan_read(good.data(), 4, 1, &s, n, 700, 0, cols, res, NULL, NULL, err));
	CHECK(tar_plan_read(good.data(), 4, 1, &s, r[4] + 700, 700, 0, cols, res, NULL, NULL, err));
	/* the entry numbers */
	CHECK(refused_with(good, 4, 4, n, "sel[0] = 4 of 4", true));
	CHECK(refused_with(good, 2, 2, n, "sel[0] = 2 of 2", true));
	/* the file's size (a device call's alone) */
	CHECK(refused_with(good, 4, 2, r[4] + 699, "data", false));
	CHECK(refused_with(good, 4, 2, r[0] + 511, "header", false));
	CHECK(refused_with(good, 4, 2, r[0], "header", false));
	/* the row itself */
	rows = good; rows[16 + 0] += 1;
	CHECK(refused_with(rows, 4, 2, n, "header", true));
	rows = good; rows[16 + 0] = ((uint64_t)1 << 36);
	CHECK(refused_with(rows, 4, 2, n, "header", true));
	rows = good; rows[16 + 1] = n;
	CHECK(refused_with(rows, 4, 2, n, "name", false));
	rows = good; rows[16 + 1] = ((uint64_t)1 << 36) + 1;
	CHECK(refused_with(rows, 4, 2, n, "name", true));
	rows = good; rows[16 + 2] = 0xFFFFFFFFull;
	CHECK(refused_with(rows, 4, 2, n, "name", false));
	rows = good; rows[16 + 2] = 5 | (uint64_t)156 << 32;
	CHECK(refused_with(rows, 4, 2, n, "name", true));
	rows = good; rows[16 + 3] = 0x10000;
	CHECK(refused_with(rows, 4, 2, n, "typeflag", true));
	rows = good; rows[16 + 4] += 512;
	CHECK(refused_with(rows, 4, 2, n, "data", true));
	rows = good; rows[16 + 4] = 0;
	CHECK(refused_with(rows, 4, 2, n, "data", true));
	rows = good; rows[16 + 5] = (uint64_t)1 << 36;
	CHECK(refused_with(rows, 4, 2, n, "2^36", true));
	rows = good; rows[16 + 5] = ~(uint64_t)0;
	CHECK(refused_with(rows, 4, 2, n, "2^36", true));
	rows = good; rows[16 + 5] = 1025;
	CHECK(refused_with(rows, 4, 2, n, "data", false));
	/* a row that is not selected is not looked at */
	rows = good; rows[0] = 3;
	CHECK(tar_plan_read(rows.data(), 4, 1, &s, n, 700, 0, cols, res, NULL, NULL, err));
	/* room: with the alignment's padding */
	CHECK(!tar_plan_read(good.data(), 4, 1, &s, n, 703, 7, cols, res, NULL, NULL, err));
	CHECK(tar_plan_read(good.data(), 4, 1, &s, n, 704, 7, cols, res, NULL, NULL, err));
	/* nothing selected */
	uint64_t offs = 9, total = 9;
	CHECK(tar_plan_read(NULL, 0, 0, NULL, 0, 0, 0, cols, res, &offs, &total, err));
	CHECK(offs == 0 && total == 0 && cols.size() == 1 && cols[0] == 0);
	CHECK(tar_plan_ranges(NULL, 0, 0, NULL, NULL, &total, err) && total == 0);
}

int main(void)
{
	test_selections();
	test_refusals();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("tar plan ok\n");
	return 0;
}
