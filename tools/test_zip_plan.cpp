/*
 * test_zip_plan.cpp - the host arithmetic of libdeflate_amd_zip_read_batch
 * (csrc/zip_plan.h) on the CPU: every refusal of a row and of a selection,
 * and the offsets and descriptor columns of selections against a plain model.
 * Stand-alone: tests/test_zip_plan.py builds it with the host compiler under
 * the address and undefined-behaviour sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zip_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Row { uint64_t w[8]; };

static Row row(uint64_t rec, uint64_t name, uint64_t method, uint64_t flags, uint64_t crc,
	       uint64_t data_off, uint64_t csize, uint64_t usize)
{
	return Row{ { rec, name, method | flags << 16, crc, data_off, csize, usize, 12345 } };
}

static bool plan(const std::vector<Row> &rows, const std::vector<uint64_t> &sel, uint64_t n,
		 uint64_t avail, uint64_t align, std::vector<uint64_t> &cols,
		 std::vector<uint64_t> &offs, std::string &err)
{
	offs.assign(sel.size() + 1, ~0ull);
	return zip_plan_read(rows.empty() ? NULL : rows[0].w, rows.size(), sel.size(),
			     sel.empty() ? NULL : sel.data(), n, avail, align - 1, cols,
			     offs.data(), NULL, err);
}

int main(void)
{
	const uint64_t n = 100000;
	std::vector<Row> rows = {
		row(90000, 5, 8, 0, 0x11111111, 30, 100, 1000),		/* 0 deflate */
		row(90051, 1, 0, 0, 0x22222222, 200, 17, 17),		/* 1 stored */
		row(90098, 0, 8, 0x808, 0, 300, 2, 0),			/* 2 empty, descriptor + UTF-8 */
		row(90144, 3, 12, 0, 0x33333333, 400, 10, 10),		/* 3 method 12 */
		row(90193, 3, 8, 1, 0x44444444, 500, 10, 10),		/* 4 encrypted */
		row(90242, 3, 0, 0, 0x55555555, 600, 10, 11),		/* 5 stored, sizes differ */
		row(90291, 3, 8, 0, 0x66666666, 99990, 10, 4096),	/* 6 ends at n */
	};
	std::vector<uint64_t> cols, offs;
	std::string err;

	/* rows */
	CHECK(zip_row_check(rows[0].w, n) == NULL);
	CHECK(zip_row_check(rows[6].w, n) == NULL);
	CHECK(zip_row_check(rows[6].w, n - 1) != NULL);
	CHECK(zip_row_check(row(n - 46, 0, 8, 0, 0, 0, 0, 0).w, n) == NULL);
	CHECK(zip_row_check(row(n - 46, 1, 8, 0, 0, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(n + 1, 0, 8, 0, 0, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(~0ull, 0, 8, 0, 0, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0x10000, 8, 0, 0, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 1ull << 32, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0x10000, 0, 0, 0, 0).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 0, 0, 1ull << 32, 0).w, ~0ull) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 0, 0, 0, 1ull << 32).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 0, ~0ull, 2, 0).w, n) != NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 0, n, 0, 0).w, n) == NULL);
	CHECK(zip_row_check(row(0, 0, 8, 0, 0, n, 1, 0).w, n) != NULL);
	CHECK(zip_row_result(rows[0].w) == 0 && zip_row_result(rows[1].w) == 0);
	CHECK(zip_row_result(rows[2].w) == 0);
	CHECK(zip_row_result(rows[3].w) == ZIP_UNSUPPORTED);
	CHECK(zip_row_result(rows[4].w) == ZIP_UNSUPPORTED);
	CHECK(zip_row_result(rows[5].w) == ZIP_BAD_DATA);
	for (uint64_t bit : { 5, 6, 13 })
		CHECK(zip_row_result(row(0, 0, 8, 1ull << bit, 0, 0, 0, 0).w) == ZIP_UNSUPPORTED);
	for (uint64_t bit : { 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 14, 15 })
		CHECK(zip_row_result(row(0, 0, 8, 1ull << bit, 0, 0, 0, 0).w) == 0);

	/* selections against a plain model, for every alignment */
	const std::vector<std::vector<uint64_t>> sels = {
		{}, { 0 }, { 6, 5, 4, 3, 2, 1, 0 }, { 1, 1, 0, 1 }, { 2 }, { 2, 2, 6 }, { 3, 4, 5 },
	};
	for (uint64_t align = 1; align <= 256; align *= 2)
		for (const auto &sel : sels) {
			const size_t S = sel.size();
			CHECK(plan(rows, sel, n, 1 << 20, align, cols, offs, err));
			CHECK(cols.size() == ZIP_COLS * S);
			uint64_t at = 0;
			for (size_t r = 0; r < S; r++) {
				const uint64_t *w = rows[sel[r]].w;
				const int pre = zip_row_result(w);
				const bool live = pre == 0, defl = live && (w[2] & 0xFFFF) == 8;
				const uint64_t kind = !live ? ZIP_KIND_NONE :
						      defl ? ZIP_KIND_DEFLATE : ZIP_KIND_STORED;
				CHECK(offs[r] == at);
				CHECK(cols[ZIP_COL_OUT_OFF * S + r] == (live ? at : 0));
				CHECK(cols[ZIP_COL_IN_OFF * S + r] == (defl ? w[4] : 0));
				CHECK(cols[ZIP_COL_IN_N * S + r] == (defl ? w[5] : 0));
				CHECK(cols[ZIP_COL_OUT_AV * S + r] == (defl ? w[6] : 0));
				CHECK(cols[ZIP_COL_CP_SRC * S + r] == (live && !defl ? w[4] : 0));
				CHECK(cols[ZIP_COL_CP_LEN * S + r] == (live && !defl ? w[6] : 0));
				CHECK(cols[ZIP_COL_CRC_N * S + r] == (live ? w[6] : 0));
				CHECK(cols[ZIP_COL_META * S + r] ==
				      (w[3] | (uint64_t)pre << 32 | kind << 40));
				if (live)
					at += (w[6] + align - 1) / align * align;
			}
			CHECK(offs[S] == at);
			/* exactly that much room is enough, one byte less is not */
			CHECK(plan(rows, sel, n, at, align, cols, offs, err));
			if (at) {
				CHECK(!plan(rows, sel, n, at - 1, align, cols, offs, err));
				CHECK(err.find("out_avail") != std::string::npos);
			}
		}

	/* refusals of a selection */
	CHECK(!plan(rows, { 0, 7 }, n, 1 << 20, 1, cols, offs, err));
	CHECK(err.find("sel[1] = 7") != std::string::npos);
	CHECK(!plan(rows, { 6 }, n - 1, 1 << 20, 1, cols, offs, err));
	CHECK(err.find("row 6") != std::string::npos && err.find("in_nbytes") != std::string::npos);
	CHECK(plan(rows, { 0 }, n - 1, 1 << 20, 1, cols, offs, err));	/* only selected rows count */
	rows[1].w[6] = rows[1].w[5] = 1ull << 32;
	CHECK(!plan(rows, { 1 }, ~0ull, ~0ull, 1, cols, offs, err));
	CHECK(err.find("4 GiB") != std::string::npos);
	/* offsets near 2^64 do not wrap */
	rows[1] = row(0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF);
	CHECK(plan(rows, { 1, 1, 1 }, 1ull << 36, ~0ull, 256, cols, offs, err));
	CHECK(offs[3] == 3 * (1ull << 32));
	CHECK(!plan(rows, { 1, 1, 1 }, 1ull << 36, 3 * (1ull << 32) - 1, 256, cols, offs, err));

	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("zip plan ok\n");
	return 0;
}
