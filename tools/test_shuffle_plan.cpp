/*
 * test_shuffle_plan.cpp - the host arithmetic of
 * libdeflate_amd_shuffle_decompress_batch and
 * libdeflate_amd_shuffle_compress_batch (csrc/shuffle_plan.h) on the CPU: every
 * refusal with its row and reason, the bound, and both plans against a serial
 * model - the class of every row, the scratch rooms on 16-byte boundaries and
 * disjoint, the decode batches' columns, the transpose kernels' rows, the
 * running tile count, the verdict words; the writer's rooms, its kernel rows and
 * the pieces that tile every room.  A byte-level walk over the kernels' tiling
 * (every tile, every thread's range) checks that the tiles cover every element
 * once and stay inside the chunk.  Stand-alone: tests/test_shuffle_plan.py
 * builds it with the host compiler under the address and undefined-behaviour
 * sanitizers and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "shuffle_plan.h"

using namespace lda;

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<uint64_t> Rows;

static void row(Rows &r, uint64_t so, uint64_t sn, uint64_t ro, uint64_t rn, uint64_t es,
		uint64_t mask)
{
	const uint64_t w[SHUF_WORDS] = { so, sn, ro, rn, es, mask };
	r.insert(r.end(), w, w + SHUF_WORDS);
}

/* the serial model of a tile's size */
static uint64_t model_tile(uint64_t es)
{
	if (es == 1 || es == 2 || es == 4 || es == 8)
		return 4096;
	return 16384 / es / 16 * 16;
}

static void tiles_and_constants(void)
{
	CHECK(SHUF_WORDS == 6 && SHUF_ELEM_MAX == 256 && SHUF_NO_DEFLATE == 1 && SHUF_NO_SHUFFLE == 2);
	for (uint64_t es = 1; es <= 256; es++) {
		const uint64_t T = shuf_tile_elems(es);
		CHECK(T == model_tile(es) && T % 16 == 0 && T >= 64);
		/* the kernels' staging area: es planes of T + 16 bytes in 20480 */
		CHECK(shuf_reg_es(es) || es * (T + 16) <= 20480);
		CHECK(shuf_tiles(0, es) == 0 && shuf_tiles(es - 1, es) == 0 && shuf_tiles(es, es) == 1);
		CHECK(shuf_tiles(T * es + es - 1, es) == 1 && shuf_tiles(T * es + es, es) == 2);
		/* a walk over the tiles: every element met once, none past ne */
		for (uint64_t ne : { (uint64_t)1, (uint64_t)17, T - 1, T, T + 1, 2 * T + 1 }) {
			const uint64_t n = ne * es + (es - 1), tiles = shuf_tiles(n, es);
			uint64_t met = 0;
			for (uint64_t t = 0; t < tiles; t++) {
				const uint64_t e0 = t * T, c = ne - e0 < T ? ne - e0 : T;
				CHECK(e0 < ne && c >= 1);
				met += c;
			}
			CHECK(met == ne);
		}
	}
	CHECK(shuf_identity(0, 4, 0) && shuf_identity(7, 4, 0) && !shuf_identity(8, 4, 0));
	CHECK(shuf_identity(8, 1, 0) && shuf_identity(8, 4, SHUF_NO_SHUFFLE) && !shuf_identity(512, 256, 0));
}

static bool refused(int format, const Rows &r, bool reader, uint64_t stored_avail, uint64_t raw_avail,
		    int level, const char *word, long long at_row)
{
	std::string err;
	if (shuf_check(format, r.size() / SHUF_WORDS, r.data(), reader, stored_avail, raw_avail, level, err))
		return false;
	char want[40];
	snprintf(want, sizeof(want), "row %lld:", at_row);
	return err.find(word) != std::string::npos && (at_row < 0 || err.find(want) != std::string::npos);
}

static void refusals_and_bound(void)
{
	std::string err;
	Rows ok;
	row(ok, 3, 10, 0, 40, 4, 0);
	row(ok, 13, 7, 40, 7, 3, SHUF_NO_DEFLATE);
	row(ok, 20, 0, 47, 0, 256, SHUF_NO_DEFLATE | SHUF_NO_SHUFFLE);
	CHECK(shuf_check(1, 3, ok.data(), true, 20, 47, -1, err));
	CHECK(shuf_check(0, 0, NULL, true, 0, 0, -1, err) && shuf_check(2, 0, NULL, false, 0, 0, 6, err));
	CHECK(refused(3, ok, true, 20, 47, -1, "format", -1) && refused(-1, ok, true, 20, 47, -1, "format", -1));
	{
		std::string e;
		CHECK(!shuf_check(1, SHUF_MAX_CHUNKS + 1, ok.data(), true, 20, 47, -1, e) &&
		      e.find("n_chunks") != std::string::npos);
	}
	for (size_t r = 0; r < 3; r++) {
		Rows bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_ES] = 0;
		CHECK(refused(1, bad, true, 20, 47, -1, "element size", (long long)r));
		bad[r * SHUF_WORDS + SHUF_W_ES] = 257;
		CHECK(refused(1, bad, true, 20, 47, -1, "element size", (long long)r));
		bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_MASK] |= 4;
		CHECK(refused(1, bad, true, 20, 47, -1, "mask", (long long)r));
		bad[r * SHUF_WORDS + SHUF_W_MASK] = (uint64_t)1 << 63;
		CHECK(refused(1, bad, true, 20, 47, -1, "mask", (long long)r));
		bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_RAW_N] = (uint64_t)1 << 32;
		CHECK(refused(1, bad, true, 20, ~(uint64_t)0, -1, "2^32", (long long)r));
		bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_STORED_N] += 1 + (r == 0 ? 7 : r == 1 ? 0 : 0);
		CHECK(refused(1, bad, true, 20, 47, -1, "in_nbytes", (long long)r));
		bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_STORED_OFF] = ~(uint64_t)0;	/* no wrap-around */
		CHECK(refused(1, bad, true, 20, 47, -1, "in_nbytes", (long long)r));
		bad = ok;
		bad[r * SHUF_WORDS + SHUF_W_RAW_OFF] += 1 + (r == 0 ? 7 : 0);
		CHECK(refused(1, bad, true, 20, 47, -1, "out_avail", (long long)r));
		bad[r * SHUF_WORDS + SHUF_W_RAW_OFF] = ~(uint64_t)0 - 3;
		CHECK(refused(1, bad, true, 20, 47, -1, "out_avail", (long long)r));
	}
	CHECK(refused(1, ok, true, 19, 47, -1, "in_nbytes", 1) && refused(1, ok, true, 20, 46, -1, "out_avail", 1));
	/* the writer: NO_DEFLATE is no mask of its, words 0 and 1 are not looked at */
	CHECK(refused(1, ok, false, 0, 47, 6, "mask", 1));
	Rows w = ok;
	w[1 * SHUF_WORDS + SHUF_W_MASK] = 0;
	w[2 * SHUF_WORDS + SHUF_W_MASK] = SHUF_NO_SHUFFLE;
	w[SHUF_W_STORED_OFF] = ~(uint64_t)0;
	CHECK(shuf_check(1, 3, w.data(), false, 0, 47, 6, err));
	CHECK(refused(1, w, false, 0, 46, 6, "in_avail", 1));
	Rows big;
	row(big, 0, 0, 0, 0xFFFFFF01ull, 4, 0);
	CHECK(shuf_check(0, 1, big.data(), false, 0, ~(uint64_t)0, 1, err));
	CHECK(refused(0, big, false, 0, ~(uint64_t)0, 0, "level-0", 0));
	/* the bound: the sum of libdeflate_<format>_compress_bound() */
	CHECK(shuf_bound(0, 3, w.data()) == 45 + 12 + 5 && shuf_bound(1, 3, w.data()) == 45 + 12 + 5 + 18);
	CHECK(shuf_bound(2, 3, w.data()) == 45 + 12 + 5 + 54 && shuf_bound(2, 0, NULL) == 0);
	CHECK(shuf_bound(1, 3, ok.data()) == 0 && shuf_bound(3, 3, w.data()) == 0);
	CHECK(chunk_stream_bound(0, 5000) == 5005 && chunk_stream_bound(0, 5001) == 5011);
	CHECK(shuf_bound(2, 1, big.data()) == 0xFFFFFF01ull + 5 * ((0xFFFFFF01ull + 4999) / 5000) + 18);
}

/* the reader's plan of these rows against a serial walk */
static void check_read_plan(const Rows &r)
{
	const uint64_t n = r.size() / SHUF_WORDS;
	shuf_read_plan p;
	shuf_read_plan_build(n, r.data(), p);
	uint64_t n_sd = 0, n_id = 0, n_u = 0, tiles = 0, scratch = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * SHUF_WORDS];
		const bool ident = w[4] == 1 || w[3] / w[4] <= 1 || (w[5] & 2);
		if (w[5] & 1)
			n_u += w[1] == w[3] && w[3];
		else if (ident)
			n_id++;
		else
			n_sd++, n_u++;
	}
	CHECK(p.n == n && p.n_sd == n_sd && p.n_id == n_id && p.n_u == n_u);
	const uint64_t n_dec = n_sd + n_id;
	CHECK(p.u_at == CHUNK_DCOLS * n_dec && p.verd_at == p.u_at + SHUF_UCOLS * n_u);
	CHECK(p.cols.size() == p.verd_at + n);
	if (p.cols.size() != p.verd_at + n)
		return;
	const uint64_t *dc = p.cols.data(), *uc = p.cols.data() + p.u_at, *verd = p.cols.data() + p.verd_at;
	uint64_t sd = 0, id = n_sd, u = 0;
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * SHUF_WORDS];
		const bool ident = w[4] == 1 || w[3] / w[4] <= 1 || (w[5] & 2);
		uint64_t ues = ident ? 1 : w[4];
		if (w[5] & 1) {
			CHECK(verd[k] == (SHUF_VERD_OWN | (uint64_t)(w[1] != w[3])));
			if (w[1] != w[3] || !w[3])
				continue;
			CHECK(uc[SHUF_U_SRC * n_u + u] == (w[0] | SHUF_SRC_ALT));
		} else {
			const uint64_t at = ident ? id++ : sd++;
			CHECK(verd[k] == at);
			CHECK(dc[CHUNK_D_IN_OFF * n_dec + at] == w[0] && dc[CHUNK_D_IN_N * n_dec + at] == w[1]);
			CHECK(dc[CHUNK_D_OUT_N * n_dec + at] == w[3]);
			if (ident) {
				CHECK(dc[CHUNK_D_OUT_OFF * n_dec + at] == w[2]);
				continue;
			}
			/* a room of its own on a 16-byte boundary, behind the one before */
			CHECK(dc[CHUNK_D_OUT_OFF * n_dec + at] == scratch && scratch % 16 == 0);
			CHECK(uc[SHUF_U_SRC * n_u + u] == scratch);
			scratch += (w[3] + 15) / 16 * 16;
		}
		const uint64_t T = model_tile(ues);
		tiles += (w[3] / ues + T - 1) / T;
		CHECK(uc[SHUF_U_TILE_END * n_u + u] == tiles);
		CHECK(uc[SHUF_U_DST * n_u + u] == w[2]);
		CHECK(uc[SHUF_U_GEOM * n_u + u] == (w[3] | ues << 32));
		/* a kernel row always has a tile: the binary search relies on it */
		CHECK(u == 0 ? tiles > 0 : tiles > uc[SHUF_U_TILE_END * n_u + u - 1]);
		u++;
	}
	CHECK(sd == n_sd && id == n_dec && u == n_u && p.tiles == tiles && p.scratch == scratch);
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
	const uint64_t n = r.size() / SHUF_WORDS;
	shuf_write_plan p;
	shuf_write_plan_build(pr, n, r.data(), p);
	uint64_t n_u = 0;
	for (uint64_t k = 0; k < n; k++)
		n_u += r[k * SHUF_WORDS + 3] != 0;
	CHECK(p.n == n && p.n_u == n_u && p.ecols.size() == SHUFW_ECOLS * n + SHUF_UCOLS * n_u);
	if (p.ecols.size() != SHUFW_ECOLS * n + SHUF_UCOLS * n_u)
		return;
	const uint64_t *ec = p.ecols.data(), *uc = ec + SHUFW_ECOLS * n, np = p.np;
	uint64_t room = 0, total = 0, tiles = 0, u = 0, pieces = 0;
	std::vector<char> seen((size_t)np);
	for (uint64_t k = 0; k < n; k++) {
		const uint64_t *w = &r[k * SHUF_WORDS];
		const bool ident = w[4] == 1 || w[3] / w[4] <= 1 || (w[5] & 2);
		const uint64_t ues = ident ? 1 : w[4], S = model_S(pr, w[3]);
		const uint64_t f = ec[CHUNKW_E_FIRST * n + k], cnt = ec[CHUNKW_E_COUNT * n + k];
		CHECK(ec[CHUNKW_E_USIZE * n + k] == w[3] && ec[SHUFW_E_ES * n + k] == w[4]);
		CHECK(ec[SHUFW_E_MASK * n + k] == w[5] && ec[SHUFW_E_RAW_OFF * n + k] == w[2]);
		CHECK(cnt == (S ? (w[3] + S - 1) / S : w[3] ? 1 : 0));
		CHECK(room % 16 == 0);
		/* the pieces tile the room in order; a prime never reaches in front of it */
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
		CHECK(f + cnt <= np && at == room + w[3]);
		pieces += cnt;
		if (w[3]) {
			const uint64_t T = model_tile(ues);
			tiles += (w[3] / ues + T - 1) / T;
			CHECK(uc[SHUF_U_TILE_END * n_u + u] == tiles);
			CHECK(uc[SHUF_U_SRC * n_u + u] == w[2] && uc[SHUF_U_DST * n_u + u] == room);
			CHECK(uc[SHUF_U_GEOM * n_u + u] == (w[3] | ues << 32));
			CHECK(u == 0 ? tiles > 0 : tiles > uc[SHUF_U_TILE_END * n_u + u - 1]);
			u++;
		}
		room += (w[3] + 15) / 16 * 16;
		total += w[3];
	}
	CHECK(pieces == np && u == n_u && p.tiles == tiles && p.rooms_bytes == room && p.raw_total == total);
	/* the launches cover every piece once */
	uint64_t covered = 0;
	for (const zipw_launch &l : zipw_launches(p)) {
		CHECK(l.lo == covered && l.count > 0);
		covered += l.count;
	}
	CHECK(covered == np);
}

static void plans(void)
{
	/* every class of row, every element size of the tests, sizes around a tile */
	Rows r;
	uint64_t so = 5, ro = 3;
	const uint64_t ess[] = { 1, 2, 3, 4, 5, 8, 16, 255, 256 };
	for (uint64_t es : ess) {
		const uint64_t T = model_tile(es);
		const uint64_t nes[] = { 0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1 };
		for (uint64_t ne : nes)
			for (uint64_t left : { (uint64_t)0, (uint64_t)1, es - 1 })
				for (uint64_t mask = 0; mask < 4; mask++) {
					const uint64_t n = ne * es + (left < es ? left : 0);
					/* a NO_DEFLATE row now and then with unequal sizes */
					const uint64_t sn = (mask & 1) ? n + (ne == 15 && left == 1) : n / 2 + 11;
					row(r, so, sn, ro, n, es, mask);
					so += sn + 1;
					ro += n + (es & 3);
				}
	}
	std::string err;
	CHECK(shuf_check(1, r.size() / SHUF_WORDS, r.data(), true, so, ro, -1, err));
	check_read_plan(r);
	check_read_plan(Rows());
	/* all identity: no kernel row, no scratch */
	Rows idn;
	row(idn, 0, 9, 0, 100, 1, 0);
	row(idn, 9, 9, 100, 7, 4, 0);
	row(idn, 18, 9, 107, 800, 8, SHUF_NO_SHUFFLE);
	check_read_plan(idn);
	{
		shuf_read_plan p;
		shuf_read_plan_build(3, idn.data(), p);
		CHECK(p.n_sd == 0 && p.n_id == 3 && p.n_u == 0 && p.tiles == 0 && p.scratch == 0);
	}
	/* the writer: the same rows without NO_DEFLATE, and chunks that are cut */
	Rows w;
	for (size_t k = 0; k < r.size() / SHUF_WORDS; k++)
		if (!(r[k * SHUF_WORDS + 5] & 1))
			w.insert(w.end(), r.begin() + k * SHUF_WORDS, r.begin() + (k + 1) * SHUF_WORDS);
	row(w, 0, 0, ro, 131072, 4, 0);
	row(w, 0, 0, ro + 131072, 131071, 8, 0);
	row(w, 0, 0, ro + 300000, (5u << 20) + 3, 3, 0);
	row(w, 0, 0, ro, 0xFFFFFFFFull, 2, SHUF_NO_SHUFFLE);
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
	tiles_and_constants();
	refusals_and_bound();
	plans();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("shuffle plan ok\n");
	return 0;
}
