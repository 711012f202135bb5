/*
 * test_exr_plan.cpp - the host arithmetic of libdeflate_amd_exr_decode_batch
 * and libdeflate_amd_exr_encode_batch (csrc/exr_plan.h) on the CPU: every
 * refusal with its row and reason, the bound, and both plans against a serial
 * model - the class of every row, the rooms on 16-byte boundaries and disjoint,
 * the decode batch's, the copy kernel's and the undo kernels' columns, the
 * tiles' stretches and slots (the stretches of a chunk partition its bytes in
 * slot order, so every slot carries from the slots in front of it in its own
 * chunk and from no other), the layout rows with their items, tiles and
 * channel places, the verdict words; the writer's rooms, tile counts and the
 * pieces that tile every room.  Stand-alone: tests/test_exr_plan.py builds it
 * with the host compiler under the address and undefined-behaviour sanitizers
 * and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "exr_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<uint64_t> Rows;

static void row(Rows &r, uint64_t doff, uint64_t dn, uint64_t poff, uint64_t pitch, uint64_t w,
		uint64_t lines, uint64_t c, uint64_t mask, uint64_t layout, uint64_t slots,
		uint64_t head = 8, uint64_t h0 = 0, uint64_t h1 = 0)
{
	const uint64_t x[EXR_WORDS] = { doff, dn, poff, pitch, w | lines << 32, c | mask << 8 | layout << 32,
					slots, head, h0, h1 };
	r.insert(r.end(), x, x + EXR_WORDS);
}

/* the serial model of a row's sizes */
static uint64_t model_px(uint64_t c, uint64_t mask)
{
	uint64_t px = 0;
	for (uint64_t k = 0; k < c; k++)
		px += (mask >> k & 1) ? 4 : 2;
	return px;
}

static bool refused(const Rows &r, bool reader, uint64_t stored_avail, uint64_t pix_avail, int level,
		    const char *word, long long at_row)
{
	std::string err;
	if (exr_check(r.size() / EXR_WORDS, r.data(), reader, stored_avail, pix_avail, level, err))
		return false;
	char want[40];
	snprintf(want, sizeof(want), "row %lld:", at_row);
	return err.find(word) != std::string::npos && (at_row < 0 || err.find(want) != std::string::npos);
}

static void refusals_and_bound(void)
{
	std::string err;
	Rows ok;
	/* in_nbytes 30, out_avail 200 */
	row(ok, 3, 10, 0, 30, 5, 4, 3, 0, EXR_LINES, 0);		/* 4 lines of 30 at 0 */
	row(ok, 13, 7, 120, 50, 1, 2, 2, 2, EXR_PIXELS, 0x01, 20);	/* 2 lines of 6 at pitch 50: ends at 176 */
	row(ok, 20, 10, 180, 0, 5, 1, 1, 1, EXR_PIXELS, 0, 0);		/* one line of 20: ends at 200 */
	CHECK(exr_check(3, ok.data(), true, 30, 200, -1, err));
	CHECK(exr_check(0, NULL, true, 0, 0, -1, err) && exr_check(0, NULL, false, 0, 0, 6, err));
	CHECK(!exr_check(EXR_MAX_CHUNKS + 1, ok.data(), true, 30, 200, -1, err) &&
	      err.find("n_chunks") != std::string::npos);
	CHECK(refused(ok, true, 29, 200, -1, "in_nbytes", 2) && refused(ok, true, 30, 199, -1, "out_avail", 2));
	CHECK(refused(ok, true, 30, 175, -1, "out_avail", 1));
	CHECK(refused(ok, false, 0, 199, 6, "in_avail", 2));
	CHECK(exr_check(3, ok.data(), false, 0, 200, 6, err));	/* the writer ignores words 0 and 1 */
	struct { size_t r, word; uint64_t value; const char *why; } bad[] = {
		{ 0, EXR_W_FMT, 0, "channels" },
		{ 0, EXR_W_FMT, 17, "channels" },
		{ 0, EXR_W_FMT, 3 | (uint64_t)8 << 8, "wide-mask" },
		{ 0, EXR_W_FMT, 3 | (uint64_t)1 << 24, "unknown bits" },
		{ 0, EXR_W_FMT, 3 | (uint64_t)2 << 32, "unknown bits" },
		{ 0, EXR_W_FMT, 3 | (uint64_t)1 << 63, "unknown bits" },
		{ 0, EXR_W_GEOM, 0 | (uint64_t)4 << 32, "zero width" },
		{ 0, EXR_W_GEOM, 5, "zero width" },
		{ 0, EXR_W_SLOTS, 1, "word 6" },
		{ 1, EXR_W_SLOTS, 0x00, "permutation" },
		{ 1, EXR_W_SLOTS, 0x21, "permutation" },
		{ 1, EXR_W_SLOTS, 0x110, "permutation" },
		{ 2, EXR_W_SLOTS, 1, "permutation" },
		{ 0, EXR_W_HEAD, 4, "head length" },
		{ 1, EXR_W_HEAD, 21, "head length" },
		{ 0, EXR_W_PITCH, 29, "pitch below" },
		{ 1, EXR_W_PITCH, 5, "pitch below" },
		{ 0, EXR_W_GEOM, 0x40000000ull | (uint64_t)4 << 32, "2^32" },
		{ 0, EXR_W_GEOM, 5 | (uint64_t)0xFFFFFFFF << 32, "2^32" },
		{ 1, EXR_W_DATA_OFF, 31, "in_nbytes" },
		{ 1, EXR_W_DATA_N, 18, "in_nbytes" },
		{ 1, EXR_W_DATA_OFF, ~(uint64_t)0, "in_nbytes" },
		{ 1, EXR_W_PIX_OFF, 145, "out_avail" },
		{ 1, EXR_W_PIX_OFF, ~(uint64_t)0 - 2, "out_avail" },
		{ 1, EXR_W_PITCH, ~(uint64_t)0, "out_avail" },
	};
	for (const auto &b : bad) {
		Rows r = ok;
		r[EXR_WORDS * b.r + b.word] = b.value;
		CHECK(refused(r, true, 30, 200, -1, b.why, (long long)b.r));
		if (b.word > EXR_W_DATA_N && strcmp(b.why, "out_avail"))
			CHECK(exr_bound(3, r.data()) == 0);
	}
	/* one line: the pitch is not looked at */
	{
		Rows r = ok;
		r[EXR_WORDS * 2 + EXR_W_PITCH] = 1;
		CHECK(exr_check(3, r.data(), true, 30, 200, -1, err));
	}
	/* 16 channels: every slot field is in use */
	{
		Rows r;
		row(r, 0, 0, 0, 0, 1, 1, 16, 0xFFFF, EXR_PIXELS, 0x0123456789ABCDEFull);
		CHECK(exr_check(1, r.data(), true, 0, 64, -1, err));
		r[EXR_W_SLOTS] = 0x1123456789ABCDEFull;
		CHECK(refused(r, true, 0, 64, -1, "permutation", 0));
	}
	/* the writer at level 0 */
	{
		Rows r;
		row(r, 0, 0, 0, 0, 0x3FFFFFE1, 1, 1, 1, EXR_LINES, 0);	/* 0xFFFFFF84 bytes */
		CHECK(exr_check(1, r.data(), false, 0, ~(uint64_t)0, 6, err));
		CHECK(refused(r, false, 0, ~(uint64_t)0, 0, "level-0", 0));
		CHECK(exr_bound(1, r.data()) == 0xFFFFFF84ull + 8);
	}
	/* the bound: the sum of head + n, whatever words 0 and 1 hold */
	CHECK(exr_bound(3, ok.data()) == (8 + 120) + (20 + 12) + (0 + 20));
	CHECK(exr_bound(0, NULL) == 0 && exr_bound(EXR_MAX_CHUNKS + 1, ok.data()) == 0);
}

/* the stretches of a chunk of n bytes: in slot order they partition [0, n) */
static void stretches_of(uint64_t n)
{
	const uint64_t nt = exr_tiles(n), h = (n + 1) / 2;
	uint64_t at = 0;
	CHECK(nt == (n + EXR_TILE - 1) / EXR_TILE && nt >= 1);
	for (uint64_t slot = 0; slot < 2 * nt; slot++) {
		const bool second = slot >= nt;
		const uint64_t j = second ? slot - nt : slot;
		uint64_t start;
		const uint64_t len = exr_stretch(n, j, second, &start);
		CHECK(len <= EXR_TILE / 2);
		if (slot == nt)
			CHECK(at == h);	/* the second half's first stretch carries the whole first half */
		if (len) {
			CHECK(start == at);	/* the carry of a slot: all bytes in front of `at` */
			at += len;
		}
		/* tile j writes raw [j * TILE, ...): 2 * len bytes of A, or one less where B is shorter */
		if (!second) {
			uint64_t sb;
			const uint64_t lb = exr_stretch(n, j, true, &sb);
			const uint64_t out = n - j * EXR_TILE < EXR_TILE ? n - j * EXR_TILE : EXR_TILE;
			CHECK(len + lb == out && (len == lb || len == lb + 1));
			CHECK(sb == h + j * (EXR_TILE / 2));
		}
	}
	CHECK(at == n);
}

static void tiles_and_constants(void)
{
	CHECK(EXR_WORDS == 10 && EXR_CHANNELS_MAX == 16 && EXR_RESULT_WORDS == 4);
	CHECK(EXR_TILE == 64 * EXR_LANE && EXR_LANE == 32 && EXR_WG_TILES == 4 && EXR_CTILE == 4096);
	const uint64_t sizes[] = { 1, 2, 3, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 3000,
				   4095, 4096, 4097, 8191, 8192, 8193, 6150, 2 << 20, (2 << 20) + 1,
				   0xFFFFFFFFull };
	for (uint64_t n : sizes)
		if (n <= (4 << 20))
			stretches_of(n);
	CHECK(exr_tiles(0xFFFFFFFFull) == (1 << 21));
}

static void read_plan(void)
{
	Rows r;
	/* 0: zlib, direct (LINES at its own pitch): 3000 bytes -> 2 tiles, straight into d_out */
	row(r, 0, 100, 1000, 3000, 750, 1, 1, 1, EXR_LINES, 0);
	/* 1: raw, direct */
	row(r, 100, 96, 5000, 48, 8, 2, 2, 2, EXR_LINES, 0);
	/* 2: oversize */
	row(r, 200, 97, 6000, 48, 8, 2, 2, 2, EXR_LINES, 0);
	/* 3: raw through the layout kernel: A B G R half to R G B A, 9 x 3 */
	row(r, 300, 216, 7000, 100, 9, 3, 4, 0, EXR_PIXELS, 0x0123);
	/* 4: zlib, LINES at a larger pitch: through the raw room; 5 tiles */
	row(r, 600, 50, 8000, 5000, 1025, 2, 1, 1, EXR_LINES, 0);
	/* 5: zlib, mixed sizes (half half float), slots 2 0 1: the generic path */
	row(r, 700, 20, 30000, 80, 10, 2, 3, 4, EXR_PIXELS, 0x102);
	/* 6: zlib, one line of PIXELS: not direct */
	row(r, 800, 9, 40000, 0, 4, 1, 2, 0, EXR_PIXELS, 0x01);
	const uint64_t n = r.size() / EXR_WORDS;
	std::string err;
	CHECK(exr_check(n, r.data(), true, 1000, 50000, -1, err));
	const int want_class[] = { EXR_C_ZLIB, EXR_C_RAW_DIRECT, EXR_C_BAD, EXR_C_RAW_LAYOUT, EXR_C_ZLIB,
				   EXR_C_ZLIB, EXR_C_ZLIB };
	for (uint64_t k = 0; k < n; k++)
		CHECK(exr_class(r.data() + EXR_WORDS * k) == want_class[k]);

	exr_read_plan p;
	exr_read_plan_build(n, r.data(), p);
	CHECK(p.n == n && p.n_z == 4 && p.n_copy == 1 && p.n_l == 4);
	CHECK(p.utiles == 2 + 5 + 1 + 1);
	CHECK(p.coded_bytes == 3008 + 8208 + 160 + 16 && p.raw_bytes == 8208 + 160 + 16);
	CHECK(p.u_at == CHUNK_DCOLS * 4 && p.p_at == p.u_at + EXR_UCOLS * 4 && p.l_at == p.p_at + EXR_PCOLS);
	CHECK(p.verd_at == p.l_at + EXR_LCOLS * 4 && p.cols.size() == p.verd_at + n);
	const uint64_t *d = p.cols.data(), *u = d + p.u_at, *c = d + p.p_at, *l = d + p.l_at,
		       *v = d + p.verd_at;
	/* the decode batch, in row order; rooms on 16-byte boundaries, disjoint */
	const uint64_t zrows[] = { 0, 4, 5, 6 }, zn[] = { 3000, 8200, 160, 16 };
	uint64_t room = 0, tiles = 0, raw_room = 0;
	for (size_t i = 0; i < 4; i++) {
		const uint64_t *w = r.data() + EXR_WORDS * zrows[i];
		CHECK(d[CHUNK_D_IN_OFF * 4 + i] == w[0] && d[CHUNK_D_IN_N * 4 + i] == w[1]);
		CHECK(d[CHUNK_D_OUT_OFF * 4 + i] == room && d[CHUNK_D_OUT_N * 4 + i] == zn[i] && room % 16 == 0);
		tiles += (zn[i] + EXR_TILE - 1) / EXR_TILE;
		CHECK(u[EXR_U_TILE_END * 4 + i] == tiles && u[EXR_U_SRC * 4 + i] == room &&
		      u[EXR_U_N * 4 + i] == zn[i]);
		if (i == 0) {
			CHECK(u[EXR_U_DST * 4 + i] == (1000 | EXR_DST_OUT));
		} else {
			CHECK(u[EXR_U_DST * 4 + i] == raw_room && raw_room % 16 == 0);
			raw_room += chunk_align16(zn[i]);
		}
		room += chunk_align16(zn[i]);
		CHECK(v[zrows[i]] == i);
	}
	CHECK(v[1] == (EXR_VERD_OWN | 0) && v[2] == (EXR_VERD_OWN | 1) && v[3] == (EXR_VERD_OWN | 0));
	CHECK(c[EXR_P_SRC] == 100 && c[EXR_P_DST] == 5000 && c[EXR_P_LEN] == 96);
	/* the layout rows: 3 (from d_in), 4, 5, 6 (from their raw rooms) */
	/* items: 3: ceil(9 / 8) * 3 = 6; 4: ceil(4100 / 16) * 2 = 514; 5: 10 * 2; 6: ceil(4 / 8) */
	const uint64_t items[] = { 6, 514, 20, 1 };
	const uint64_t lraw[] = { 300 | EXR_RAW_IN, 0, 8208, 8368 };
	const uint64_t lrow[] = { 3, 4, 5, 6 };
	uint64_t lt = 0;
	for (size_t i = 0; i < 4; i++) {
		const uint64_t *w = r.data() + EXR_WORDS * lrow[i];
		lt += (items[i] + EXR_LTILE - 1) / EXR_LTILE;
		CHECK(l[EXR_L_TILE_END * 4 + i] == lt && l[EXR_L_RAW * 4 + i] == lraw[i]);
		CHECK(l[EXR_L_PIX * 4 + i] == w[2] && l[EXR_L_GEOM * 4 + i] == w[4] && l[EXR_L_FMT * 4 + i] == w[5]);
		CHECK(l[EXR_L_PITCH * 4 + i] == ((w[4] >> 32) > 1 ? w[3] : 0));
	}
	CHECK(p.ltiles == lt && lt == 1 + 3 + 1 + 1);
	/* where the channels stand: A B G R -> slots 3 2 1 0 of 2 bytes; half half float at 2 0 1 ->
	 * slot 0 is channel 1 (2 bytes), slot 1 channel 2 (4 bytes), slot 2 channel 0 */
	CHECK(l[EXR_L_DOFF0 * 4 + 0] == (6 | 4 << 8 | 2 << 16 | 0 << 24) && l[EXR_L_DOFF1 * 4 + 0] == 0);
	CHECK(l[EXR_L_DOFF0 * 4 + 1] == 0);
	CHECK(l[EXR_L_DOFF0 * 4 + 2] == (6 | 0 << 8 | 2 << 16));
	CHECK(l[EXR_L_DOFF0 * 4 + 3] == (2 | 0 << 8));
	/* 16 channels: the places of channels 8 .. 15 go into the second word */
	{
		Rows b;
		row(b, 0, 0, 0, 0, 3, 1, 16, 0xFF00, EXR_PIXELS, 0xFEDCBA9876543210ull);
		exr_layout_rows lr;
		lr.add(b.data(), 0);
		uint64_t d0 = 0, d1 = 0;
		for (uint64_t k = 0; k < 8; k++) {
			d0 |= (2 * k) << (8 * k);
			d1 |= (16 + 4 * k) << (8 * k);
		}
		CHECK(lr.col[EXR_L_DOFF0][0] == d0 && lr.col[EXR_L_DOFF1][0] == d1 && lr.tiles == 1);
		CHECK(model_px(16, 0xFF00) == 48 && exr_chunk_of(b.data()).px == 48);
	}
	/* nothing but direct raw rows: no room, no tile */
	{
		Rows b;
		row(b, 0, 96, 0, 48, 8, 2, 2, 2, EXR_LINES, 0);
		row(b, 96, 48, 96, 7, 8, 1, 2, 2, EXR_LINES, 0);
		exr_read_plan q;
		exr_read_plan_build(2, b.data(), q);
		CHECK(q.n_copy == 2 && q.n_z == 0 && q.n_l == 0 && q.utiles == 0 && q.ltiles == 0 &&
		      q.coded_bytes == 0 && q.raw_bytes == 0);
	}
}

static void write_plan(void)
{
	Rows r;
	row(r, 0, 0, 10, 100, 9, 3, 4, 0, EXR_PIXELS, 0x0123, 8, 7);
	row(r, 0, 0, 1000, 8200, 1025, 40, 2, 3, EXR_LINES, 0, 20, 1 | (uint64_t)2 << 32, 0);	/* 328 000 bytes */
	row(r, 0, 0, 400000, 0, 1, 1, 1, 0, EXR_LINES, 0, 0);
	const uint64_t n = 3, sizes[] = { 216, 328000, 2 };
	std::string err;
	CHECK(exr_check(n, r.data(), false, 0, 500000, 6, err));
	zipw_params pr = { 6, false, false, 0, 32768, 4096, 1024 };
	exr_write_plan p;
	exr_write_plan_build(pr, n, r.data(), p);
	CHECK(p.n == n && p.raw_total == 216 + 328000 + 2);
	const uint64_t *e = p.ecols.data();
	uint64_t room = 0, ct = 0;
	for (uint64_t k = 0; k < n; k++) {
		ct += (sizes[k] + EXR_CTILE - 1) / EXR_CTILE;
		CHECK(e[CHUNKW_E_USIZE * n + k] == sizes[k] && e[EXRW_E_ROOM * n + k] == room && room % 16 == 0);
		CHECK(e[EXRW_E_CTILE_END * n + k] == ct);
		for (uint64_t a = 0; a < 8; a++)
			CHECK(e[(EXRW_E_WORDS + a) * n + k] == r[EXR_WORDS * k + 2 + a]);
		/* the pieces tile the room */
		const uint64_t first = e[CHUNKW_E_FIRST * n + k], cnt = e[CHUNKW_E_COUNT * n + k];
		uint64_t at = room;
		CHECK(cnt >= 1);
		for (uint64_t j = first; j < first + cnt; j++) {
			CHECK(p.pcols[ZIPW_P_PC_OFF * p.np + j] == at);
			at += p.pcols[ZIPW_P_PC_N * p.np + j];
		}
		CHECK(at == room + sizes[k]);
		room += chunk_align16(sizes[k]);
	}
	CHECK(e[CHUNKW_E_COUNT * n + 1] > 1);	/* above 128 KiB: primed segments */
	CHECK(p.rooms_bytes == room && p.ctiles == ct && p.l_at == EXRW_ECOLS * n);
	CHECK(p.ecols.size() == p.l_at + EXR_LCOLS * n);
	const uint64_t *l = e + p.l_at;
	/* items: ceil(9 / 8) * 3 = 6; ceil(8200 / 16) * 40 = 20520; 1 */
	CHECK(l[EXR_L_TILE_END * n + 0] == 1 && l[EXR_L_TILE_END * n + 1] == 1 + 81 &&
	      l[EXR_L_TILE_END * n + 2] == 83 && p.ltiles == 83);
	for (uint64_t k = 0; k < n; k++)
		CHECK(l[EXR_L_RAW * n + k] == e[EXRW_E_ROOM * n + k] && l[EXR_L_PIX * n + k] == r[EXR_WORDS * k + 2]);
}

int main(void)
{
	tiles_and_constants();
	refusals_and_bound();
	read_plan();
	write_plan();
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("exr plan ok\n");
	return 0;
}
