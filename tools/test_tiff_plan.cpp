/*
 * test_tiff_plan.cpp - the host arithmetic of libdeflate_amd_tiff_decode_batch
 * and libdeflate_amd_tiff_encode_batch (csrc/tiff_plan.h) on the CPU: every
 * refusal with its row and reason, the bound, and both plans against a serial
 * model - the class of every row, the scratch rooms on 16-byte boundaries and
 * disjoint, the decode batches' columns, the unpredict kernel's scans ordered
 * by group size with their running quad counts, the gather kernel's rows, the
 * verdict words; the writer's rooms, its tile counts and the pieces that tile
 * every room.  A walk over the kernel's passes (every group, every lane's
 * piece) checks that the lanes cover every byte of a row once, stay inside it,
 * and that a group never straddles a wave.  Stand-alone: tests/test_tiff_plan.py
 * builds it with the host compiler under the address and undefined-behaviour
 * sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tiff_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<uint64_t> Rows;

static void row(Rows &r, uint64_t so, uint64_t sn, uint64_t ro, uint64_t pitch, uint64_t cw,
		uint64_t cr, uint64_t kw, uint64_t kr, uint64_t spp, uint64_t bps, uint64_t pred)
{
	const uint64_t w[TIFF_WORDS] = { so, sn, ro, pitch, cw | cr << 32, kw | kr << 32,
					 spp | bps << 8 | pred << 16, 0 };
	r.insert(r.end(), w, w + TIFF_WORDS);
}

/* the serial model of a lane's bytes and of the group */
static uint64_t model_lane(uint64_t st)
{
	switch (st) {
	case 0: return 16;
	case 1: case 2: case 4: case 8: case 16: return 64;
	case 3: case 6: case 12: case 24: case 48: return 48;
	}
	return st;
}

static uint64_t model_group(uint64_t rb, uint64_t st)
{
	const uint64_t L = model_lane(st);
	return rb <= 4 * L ? 4 : rb <= 16 * L ? 16 : 64;
}

static void groups_and_constants(void)
{
	CHECK(TIFF_WORDS == 8 && TIFF_SPP_MAX == 16 && TIFF_RESULT_WORDS == 4 && TIFF_PTILE == 4096);
	for (uint64_t st = 0; st <= 128; st++) {
		const uint64_t L = tiff_lane_bytes(st);
		CHECK(L == model_lane(st) && (st == 0 || L % st == 0));
		for (uint64_t px = 1; px <= 70; px++) {
			/* rows of whole pixels around the groups' edges */
			const uint64_t unit = st ? st : 1, rb = px * unit, G = tiff_group(rb, st);
			CHECK(G == model_group(rb, st));
			/* the passes: lane l of pass p owns [(p * G + l) * L, + L) of the row */
			uint64_t met = 0;
			for (uint64_t base = 0; base < rb; base += G * L)
				for (uint64_t l = 0; l < G; l++) {
					const uint64_t off = base + l * L;
					const uint64_t have = off >= rb ? 0 : rb - off >= L ? L : rb - off;
					CHECK(have % unit == 0);
					met += have;
				}
			CHECK(met == rb);
			CHECK(G == 64 || rb <= G * L);	/* 4 and 16 lanes: one pass */
		}
	}
}

static bool refused(const Rows &r, bool reader, uint64_t stored_avail, uint64_t raw_avail, int level,
		    const char *word, long long at_row)
{
	std::string err;
	if (tiff_check(r.size() / TIFF_WORDS, r.data(), reader, stored_avail, raw_avail, level, err))
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
	row(ok, 3, 10, 0, 30, 10, 4, 10, 4, 3, 1, 2);		/* 4 rows of 30 at 0 */
	row(ok, 13, 7, 120, 50, 8, 2, 5, 2, 1, 2, 3);		/* 2 rows of 10 at pitch 50: ends at 180 */
	row(ok, 20, 10, 180, 0, 5, 1, 5, 1, 1, 4, 1);		/* one row of 20: ends at 200 */
	CHECK(tiff_check(3, ok.data(), true, 30, 200, -1, err));
	CHECK(tiff_check(0, NULL, true, 0, 0, -1, err) && tiff_check(0, NULL, false, 0, 0, 6, err));
	{
		std::string e;
		CHECK(!tiff_check(TIFF_MAX_SEGMENTS + 1, ok.data(), true, 30, 200, -1, e) &&
		      e.find("n_segments") != std::string::npos);
	}
	CHECK(refused(ok, true, 29, 200, -1, "in_nbytes", 2) && refused(ok, true, 30, 199, -1, "out_avail", 2));
	CHECK(refused(ok, true, 30, 179, -1, "out_avail", 1));
	struct { size_t word; uint64_t value; const char *why; } bad[] = {
		{ TIFF_W_FMT, 0 | 1 << 8 | 2 << 16, "samples per pixel" },
		{ TIFF_W_FMT, 17 | 1 << 8 | 2 << 16, "samples per pixel" },
		{ TIFF_W_FMT, 1 | 3 << 8 | 2 << 16, "bytes per sample" },
		{ TIFF_W_FMT, 1 | 0 << 8 | 2 << 16, "bytes per sample" },
		{ TIFF_W_FMT, 1 | 16 << 8 | 2 << 16, "bytes per sample" },
		{ TIFF_W_FMT, 1 | 1 << 8 | 0 << 16, "predictor" },
		{ TIFF_W_FMT, 1 | 1 << 8 | 4 << 16, "predictor" },
		{ TIFF_W_FMT, 1 | 1 << 8 | 3 << 16, "floating-point" },
		{ TIFF_W_FMT, 1 | 1 << 8 | 1 << 16 | 1 << 24, "word 6" },
		{ TIFF_W_FMT, 1 | 1 << 8 | 1 << 16 | (uint64_t)1 << 63, "word 6" },
		{ TIFF_W_RESERVED, 1, "word 7" },
		{ TIFF_W_CODED, 0 | (uint64_t)4 << 32, "zero" },
		{ TIFF_W_CODED, 10, "zero" },
		{ TIFF_W_KEPT, 0 | (uint64_t)1 << 32, "zero" },
		{ TIFF_W_KEPT, 1, "zero" },
		{ TIFF_W_KEPT, 11 | (uint64_t)1 << 32, "kept above coded" },
		{ TIFF_W_KEPT, 1 | (uint64_t)5 << 32, "kept above coded" },
		{ TIFF_W_STORED_OFF, 31, "in_nbytes" },
		{ TIFF_W_STORED_OFF, ~(uint64_t)0, "in_nbytes" },
		{ TIFF_W_STORED_N, 28, "in_nbytes" },
		{ TIFF_W_RAW_OFF, 201, "out_avail" },
		{ TIFF_W_RAW_OFF, ~(uint64_t)0 - 3, "out_avail" },
	};
	for (size_t r = 0; r < 3; r++)
		for (const auto &b : bad) {
			Rows v = ok;
			v[r * TIFF_WORDS + b.word] = b.value;
			if (b.word == TIFF_W_KEPT || b.word == TIFF_W_CODED) {
				/* (keep the other one consistent with "zero" and "kept above coded" alone) */
				if (!strcmp(b.why, "kept above coded"))
					v[r * TIFF_WORDS + TIFF_W_CODED] = 10 | (uint64_t)4 << 32;
			}
			CHECK(refused(v, true, 30, 200, -1, b.why, (long long)r));
		}
	{
		/* the size: 2^16 x 2^16 x 1 x 1 is 2^32; a product that wraps 2^64 */
		Rows v = ok;
		v[TIFF_W_CODED] = 65536 | (uint64_t)65536 << 32;
		CHECK(refused(v, true, 30, ~(uint64_t)0, -1, "2^32", 0));
		v[TIFF_W_CODED] = 0xFFFFFFFFull | (uint64_t)0xFFFFFFFFull << 32;
		v[TIFF_W_FMT] = 16 | 8 << 8 | 2 << 16;
		CHECK(refused(v, true, 30, ~(uint64_t)0, -1, "2^32", 0));
		v = ok;
		v[TIFF_W_CODED] = 65535 | (uint64_t)65537 << 32;	/* 2^32 - 1 */
		v[TIFF_W_KEPT] = 1 | (uint64_t)1 << 32;
		v[TIFF_W_FMT] = 1 | 1 << 8 | 1 << 16;
		CHECK(tiff_check(1, v.data(), true, 30, 200, -1, err));
		CHECK(refused(v, false, 0, 200, 0, "level-0", 0) && tiff_check(1, v.data(), false, 0, 200, 1, err));
		/* the pitch: below the kept row's bytes, and a last row that wraps around */
		v = ok;
		v[TIFF_W_PITCH] = 29;
		CHECK(refused(v, true, 30, 200, -1, "pitch", 0));
		v[TIFF_W_PITCH] = 57;		/* 3 * 57 + 30 = 201 */
		CHECK(refused(v, true, 30, 200, -1, "out_avail", 0));
		v[TIFF_W_PITCH] = (~(uint64_t)0) / 3 + 1;
		CHECK(refused(v, true, 30, 200, -1, "out_avail", 0));
		v[TIFF_W_PITCH] = ~(uint64_t)0;
		CHECK(refused(v, true, 30, ~(uint64_t)0, -1, "out_avail", 0));
		v = ok;					/* a single row: the pitch is not looked at */
		v[2 * TIFF_WORDS + TIFF_W_PITCH] = ~(uint64_t)0;
		CHECK(tiff_check(3, v.data(), true, 30, 200, -1, err));
	}
	/* the writer: words 0 and 1 are not looked at, in_avail in the place of out_avail */
	Rows w = ok;
	w[TIFF_W_STORED_OFF] = ~(uint64_t)0;
	w[TIFF_W_STORED_N] = ~(uint64_t)0;
	CHECK(tiff_check(3, w.data(), false, 0, 200, 6, err));
	CHECK(refused(w, false, 0, 199, 6, "in_avail", 2));
	/* the bound: the sum of libdeflate_zlib_compress_bound(coded size) */
	CHECK(chunk_stream_bound(1, 0) == 11 && chunk_stream_bound(1, 5000) == 5011 && chunk_stream_bound(1, 5001) == 5017);
	CHECK(tiff_bound(3, w.data()) == (120 + 11) + (32 + 11) + (20 + 11) && tiff_bound(0, NULL) == 0);
	w[TIFF_WORDS + TIFF_W_RESERVED] = 5;
	CHECK(tiff_bound(3, w.data()) == 0);
}

/* the reader's plan of these rows against a serial walk */
static void check_read_plan(const Rows &r)
{
	const uint64_t n = r.size() / TIFF_WORDS;
	tiff_read_plan p;
	tiff_read_plan_build(n, r.data(), p);
	uint64_t n_ws = 0, n_direct = 0, n_g = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * TIFF_WORDS];
		const uint64_t cw = w[4] & 0xFFFFFFFF, cr = w[4] >> 32, kw = w[5] & 0xFFFFFFFF, kr = w[5] >> 32;
		const uint64_t px = (w[6] & 0xFF) * ((w[6] >> 8) & 0xFF), pred = w[6] >> 16;
		const bool direct = pred == 1 && cw == kw && cr == kr && (cr == 1 || w[3] == cw * px);
		CHECK(direct == tiff_direct(w));
		n_direct += direct;
		n_ws += !direct;
		n_g += pred == 3;
	}
	CHECK(p.n == n && p.n_ws == n_ws && p.n_direct == n_direct && p.n_k == n_ws && p.n_g == n_g);
	CHECK(p.k_at == CHUNK_DCOLS * n && p.g_at == p.k_at + TIFF_KCOLS * n_ws);
	CHECK(p.verd_at == p.g_at + TIFF_GCOLS * n_g && p.cols.size() == p.verd_at + n);
	if (p.cols.size() != p.verd_at + n)
		return;
	const uint64_t *dc = p.cols.data(), *kc = dc + p.k_at, *gc = dc + p.g_at, *verd = dc + p.verd_at;
	uint64_t ws = 0, di = n_ws, g = 0, scratch = 0, gtiles = 0;
	std::vector<char> scan_seen((size_t)n_ws);
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * TIFF_WORDS];
		const uint64_t cw = w[4] & 0xFFFFFFFF, cr = w[4] >> 32, kw = w[5] & 0xFFFFFFFF, kr = w[5] >> 32;
		const uint64_t spp = w[6] & 0xFF, bps = (w[6] >> 8) & 0xFF, px = spp * bps, pred = w[6] >> 16;
		const uint64_t coded = cw * cr * px, pitch = kr > 1 ? w[3] : 0;
		const bool direct = tiff_direct(w);
		const uint64_t at = direct ? di++ : ws++;
		CHECK(verd[k] == at);
		CHECK(dc[CHUNK_D_IN_OFF * n + at] == w[0] && dc[CHUNK_D_IN_N * n + at] == w[1]);
		CHECK(dc[CHUNK_D_OUT_N * n + at] == coded);
		if (direct) {
			CHECK(dc[CHUNK_D_OUT_OFF * n + at] == w[2]);
			continue;
		}
		/* a room of its own on a 16-byte boundary, behind the one before */
		CHECK(dc[CHUNK_D_OUT_OFF * n + at] == scratch && scratch % 16 == 0);
		/* its scan: somewhere in the kernel's rows, once */
		const uint64_t rb = pred == 3 ? cw * px : kw * px, sb = pred == 3 ? 1 : bps;
		const uint64_t st = pred == 3 ? spp : pred == 2 ? px : 0, G = model_group(rb, st);
		const uint64_t dst = pred == 3 ? (scratch | TIFF_DST_WS) : w[2];
		uint64_t found = n_ws;
		for (uint64_t j = 0; j < n_ws; j++)
			if (kc[TIFF_K_SRC * n_ws + j] == scratch)
				found = j;
		CHECK(found < n_ws);
		if (found < n_ws) {
			const uint64_t j = found;
			CHECK(!scan_seen[(size_t)j]);
			scan_seen[(size_t)j] = 1;
			CHECK(kc[TIFF_K_DST * n_ws + j] == dst);
			CHECK(kc[TIFF_K_SPITCH * n_ws + j] == cw * px);
			CHECK(kc[TIFF_K_DPITCH * n_ws + j] == (pred == 3 ? cw * px : pitch));
			CHECK(kc[TIFF_K_GEOM * n_ws + j] == (rb | sb << 32 | st << 40 | G << 48));
			const uint64_t before = j ? kc[TIFF_K_QUAD_END * n_ws + j - 1] : 0;
			CHECK(kc[TIFF_K_QUAD_END * n_ws + j] == before + kr * (G / 4));
			/* a group never straddles a wave: its first quad is a multiple of G / 4 */
			CHECK(before % (G / 4) == 0);
			/* the scan stays inside the room and, written to d_out, inside the kept rectangle */
			CHECK((kr - 1) * cw * px + rb <= coded);
		}
		if (pred == 3) {
			const uint64_t ns = kw * spp;
			const uint64_t items = kr * ((ns + 3) / 4);
			gtiles += (items + 255) / 256;
			CHECK(items > 0 && items <= 0xFFFFFFFFull);
			CHECK(g < n_g && gc[TIFF_G_TILE_END * n_g + g] == gtiles);
			CHECK(gc[TIFF_G_SRC * n_g + g] == scratch && gc[TIFF_G_DST * n_g + g] == w[2]);
			CHECK(gc[TIFF_G_DPITCH * n_g + g] == pitch);
			CHECK(gc[TIFF_G_GEOM * n_g + g] == (ns | bps << 32));
			CHECK(gc[TIFF_G_PLANE * n_g + g] == (cw * spp | items << 32));
			g++;
		}
		scratch += (coded + 15) / 16 * 16;
	}
	/* the scans are ordered by group size, 64 first */
	for (uint64_t j = 1; j < n_ws; j++)
		CHECK((kc[TIFF_K_GEOM * n_ws + j] >> 48) <= (kc[TIFF_K_GEOM * n_ws + j - 1] >> 48));
	CHECK(ws == n_ws && di == n && g == n_g && p.scratch == scratch && p.gtiles == gtiles);
	CHECK(p.quads == (n_ws ? kc[TIFF_K_QUAD_END * n_ws + n_ws - 1] : 0));
}

static uint64_t model_S(const zipw_params &pr, uint64_t usize)
{
	if (usize < 131072 || pr.level == 0 || (pr.no_segments && usize < 0xFFFF0000ull))
		return 0;
	if (pr.env_seg)
		return pr.env_seg;
	return usize <= (4u << 20) ? 16384 : usize <= (8u << 20) ? 32768 : 65536;
}

/* the writer's plan of these rows against a serial walk */
static void check_write_plan(const zipw_params &pr, const Rows &r)
{
	const uint64_t n = r.size() / TIFF_WORDS;
	tiff_write_plan p;
	tiff_write_plan_build(pr, n, r.data(), p);
	CHECK(p.n == n && p.ecols.size() == TIFFW_ECOLS * n);
	if (p.ecols.size() != TIFFW_ECOLS * n)
		return;
	const uint64_t *ec = p.ecols.data(), np = p.np;
	uint64_t room = 0, total = 0, tiles = 0, pieces = 0;
	std::vector<char> seen((size_t)np);
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * TIFF_WORDS];
		const uint64_t cw = w[4] & 0xFFFFFFFF, cr = w[4] >> 32, kw = w[5] & 0xFFFFFFFF, kr = w[5] >> 32;
		const uint64_t px = (w[6] & 0xFF) * ((w[6] >> 8) & 0xFF), coded = cw * cr * px;
		const uint64_t S = model_S(pr, coded);
		const uint64_t f = ec[CHUNKW_E_FIRST * n + k], cnt = ec[CHUNKW_E_COUNT * n + k];
		CHECK(ec[CHUNKW_E_USIZE * n + k] == coded && ec[TIFFW_E_RAW_OFF * n + k] == w[2]);
		CHECK(ec[TIFFW_E_PITCH * n + k] == w[3] && ec[TIFFW_E_CODED * n + k] == w[4]);
		CHECK(ec[TIFFW_E_KEPT * n + k] == w[5] && ec[TIFFW_E_FMT * n + k] == w[6]);
		CHECK(ec[TIFFW_E_ROOM * n + k] == room && room % 16 == 0);
		CHECK(cnt == (S ? (coded + S - 1) / S : 1));
		uint64_t at = room;
		for (uint64_t i = 0; i < cnt && f + cnt <= np; i++) {
			const uint64_t j = f + i;
			CHECK(!seen[(size_t)j]);
			seen[(size_t)j] = 1;
			CHECK(p.pcols[ZIPW_P_PC_OFF * np + j] == at);
			CHECK(p.pcols[ZIPW_P_IN_OFF * np + j] >= room && p.pcols[ZIPW_P_IN_OFF * np + j] <= at);
			CHECK(p.pcols[ZIPW_P_IN_OFF * np + j] + p.pcols[ZIPW_P_IN_N * np + j] ==
			      at + p.pcols[ZIPW_P_PC_N * np + j]);
			at += p.pcols[ZIPW_P_PC_N * np + j];
		}
		CHECK(f + cnt <= np && at == room + coded);
		pieces += cnt;
		tiles += (coded + 4095) / 4096;
		CHECK(ec[TIFFW_E_TILE_END * n + k] == tiles);
		/* every segment has a tile: the binary search relies on it */
		CHECK(k == 0 ? tiles > 0 : tiles > ec[TIFFW_E_TILE_END * n + k - 1]);
		room += (coded + 15) / 16 * 16;
		total += kw * px * kr;
	}
	CHECK(pieces == np && p.tiles == tiles && p.rooms_bytes == room && p.raw_total == total);
	uint64_t covered = 0;
	for (const zipw_launch &l : zipw_launches(p)) {
		CHECK(l.lo == covered && l.count > 0);
		covered += l.count;
	}
	CHECK(covered == np);
}

static void plans(void)
{
	/* every class of row, formats of both kernel paths, widths around the groups' edges */
	Rows r;
	uint64_t so = 5, ro = 3, k = 0;
	const uint64_t fmts[][2] = { { 1, 1 }, { 3, 1 }, { 4, 1 }, { 1, 2 }, { 3, 2 }, { 1, 4 }, { 2, 8 },
				     { 5, 1 }, { 7, 2 }, { 16, 8 }, { 12, 4 } };
	for (const auto &f : fmts) {
		const uint64_t spp = f[0], bps = f[1], px = spp * bps;
		for (uint64_t pred = 1; pred <= 3; pred++) {
			if (pred == 3 && bps == 1)
				continue;
			const uint64_t L = model_lane(pred == 3 ? spp : pred == 2 ? px : 0);
			const uint64_t ws[] = { 1, 2, (4 * L) / px, (4 * L) / px + 1, (16 * L) / px,
						(16 * L) / px + 1, (64 * L) / px + 1, (130 * L) / px + 1 };
			for (uint64_t cw : ws) {
				if (!cw)
					continue;
				const uint64_t cr = 1 + k % 5, crop = k % 4;
				const uint64_t kw = (crop & 1) && cw > 1 ? cw - 1 : cw;
				const uint64_t kr = (crop & 2) && cr > 1 ? cr - 1 : cr;
				const uint64_t pitch = kw * px + (k % 3 == 0 ? 0 : 7);
				row(r, so, 11 + k % 9, ro, pitch, cw, cr, kw, kr, spp, bps, pred);
				so += 12 + k % 9;
				ro += (kr - 1) * pitch + kw * px + (k & 3);
				k++;
			}
		}
	}
	std::string err;
	CHECK(tiff_check(r.size() / TIFF_WORDS, r.data(), true, so, ro, -1, err));
	check_read_plan(r);
	check_read_plan(Rows());
	/* all direct: no kernel row, no scratch */
	Rows d;
	row(d, 0, 9, 0, 30, 10, 4, 10, 4, 3, 1, 1);
	row(d, 9, 9, 120, 999, 7, 1, 7, 1, 1, 2, 1);
	check_read_plan(d);
	{
		tiff_read_plan p;
		tiff_read_plan_build(2, d.data(), p);
		CHECK(p.n_ws == 0 && p.n_direct == 2 && p.n_k == 0 && p.quads == 0 && p.gtiles == 0 && p.scratch == 0);
	}
	/* the writer: the same rows, and segments that are cut */
	Rows w = r;
	row(w, 0, 0, 0, 512 * 3, 512, 256, 512, 256, 3, 1, 2);		/* 384 KiB */
	row(w, 0, 0, 0, 131072, 32768, 1, 32768, 1, 1, 4, 3);		/* 128 KiB: cut */
	row(w, 0, 0, 0, 131071, 131071, 1, 131071, 1, 1, 1, 2);	/* one byte less: whole */
	row(w, 0, 0, 0, 4096, 1024, 1300, 1000, 1300, 1, 4, 2);	/* 5.07 MiB */
	for (int level : { 0, 1, 6, 12 })
		for (int variant = 0; variant < 3; variant++) {
			zipw_params pr = {};
			pr.level = level;
			pr.no_segments = variant == 1;
			pr.env_seg = variant == 2 ? 20000 : 0;
			pr.tile = 4096;
			pr.D = (32768 - 2 * pr.tile - 272) / pr.tile * pr.tile;
			pr.small_max = level <= 9 ? 4096 : 0;
			check_write_plan(pr, w);
			check_write_plan(pr, Rows());
		}
}

int main(void)
{
	groups_and_constants();
	refusals_and_bound();
	plans();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("tiff plan ok\n");
	return 0;
}
