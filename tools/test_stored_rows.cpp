/*
 * test_stored_rows.cpp - the walk over a run of stored blocks
 * (libdeflate_amd/csrc/stored_rows.h) reads the same chunks, results and stop
 * position out of the ROWS a stream in device memory is described by as out of
 * the stream's bytes.  Host only; tests/test_stored_rows.py builds it with
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I libdeflate_amd/csrc -o test_stored_rows tools/test_stored_rows.cpp
 *
 * and runs it.  The rows are made here by a plain restatement of the rule of
 * lda_stream_find_stored_kernel: every bp in [bp0, in_n - 4] whose LEN equals
 * ~NLEN, with the two bytes in front of it (zero before the stream).
 */
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <tuple>
#include <vector>

#include "stored_rows.h"

typedef std::vector<uint8_t> bytes;
typedef std::tuple<uint64_t, uint64_t, uint64_t, bool> chunk_t;	/* from, to, nout, final */

static int failures;
static std::mt19937_64 rng(0x510EED);

#define CHECK(cond, ...)                                           \
	do {                                                       \
		if (!(cond)) {                                     \
			printf("FAILED %s:%d: ", __FILE__, __LINE__); \
			printf(__VA_ARGS__);                       \
			printf("\n");                              \
			failures++;                                \
		}                                                  \
	} while (0)

static std::vector<lda_stored_row> rows_of(const bytes &raw, uint64_t in_n, uint64_t bp0)
{
	std::vector<lda_stored_row> rows;
	for (uint64_t bp = bp0; bp + 4 <= in_n; bp++) {
		const uint32_t len = raw[bp] | ((uint32_t)raw[bp + 1] << 8);
		const uint32_t nlen = raw[bp + 2] | ((uint32_t)raw[bp + 3] << 8);
		if (len != (nlen ^ 0xFFFFu))
			continue;
		lda_stored_row r = { bp, len, 0 };
		if (bp >= 2)
			r.front |= raw[bp - 2];
		if (bp >= 1)
			r.front |= (uint32_t)raw[bp - 1] << 8;
		rows.push_back(r);
	}
	/* (the kernel appends in any order) */
	std::shuffle(rows.begin(), rows.end(), rng);
	return rows;
}

struct walked {
	std::vector<chunk_t> chunks;
	uint64_t stop;
	bool fin;
	bool operator==(const walked &o) const { return chunks == o.chunks && stop == o.stop && fin == o.fin; }
};

template <typename Probe>
static walked walk(const Probe &probe, uint64_t p, uint64_t raw_n, uint64_t dev_bytes, uint64_t group)
{
	walked w;
	w.stop = lda::walk_stored_run(p, raw_n, dev_bytes, group, probe,
				      [&](uint64_t from, uint64_t to, uint64_t nout, bool fin) {
					      w.chunks.push_back(chunk_t(from, to, nout, fin));
				      },
				      &w.fin);
	return w;
}

/* a stream under construction: bits, then whole stored blocks */
struct writer {
	bytes b;
	unsigned nbits = 0;	/* bits used of the last byte (0: none open) */
	void put(uint32_t v, unsigned n)
	{
		for (unsigned i = 0; i < n; i++) {
			if (!nbits)
				b.push_back(0);
			b.back() |= ((v >> i) & 1) << nbits;
			nbits = (nbits + 1) & 7;
		}
	}
	uint64_t bit() const { return 8 * b.size() - (nbits ? 8 - nbits : 0); }
	void stored(const bytes &payload, bool fin, uint32_t len_field, bool good_nlen = true)
	{
		put(fin, 1);
		put(0, 2);
		/* (the padding bits are not checked by anybody: make them junk) */
		while (nbits)
			put((uint32_t)rng() & 1, 1);
		const uint32_t nlen = good_nlen ? len_field ^ 0xFFFFu : len_field;
		b.push_back(len_field & 0xFF);
		b.push_back(len_field >> 8);
		b.push_back(nlen & 0xFF);
		b.push_back(nlen >> 8);
		b.insert(b.end(), payload.begin(), payload.end());
	}
};

static bytes random_payload(size_t n)
{
	bytes p(n);
	for (uint8_t &x : p)
		x = (uint8_t)rng();
	return p;
}

static bytes pattern_payload(size_t n)
{
	static const uint8_t pat[4] = { 0x00, 0x00, 0xFF, 0xFF };
	bytes p(n);
	for (size_t i = 0; i < n; i++)
		p[i] = pat[i & 3];
	return p;
}

/*
 * One stream, walked from `p` by bytes and by rows for several windows
 * (in_n: what the kernel searched; dev_bytes <= in_n: what the walk may use)
 * and groups; then with half of the rows dropped.
 */
static void compare(const char *what, const bytes &raw, uint64_t raw_n, uint64_t p)
{
	const lda::stored_probe_bytes by_bytes = { raw.data(), raw_n };
	const uint64_t windows[] = { raw_n, raw_n > 7 ? raw_n - 7 : raw_n, raw_n / 2 + 3, raw_n / 3 };
	const uint64_t groups[] = { 1, 8 * 16384, 8 * 4096, ~(uint64_t)0 };
	for (uint64_t in_n : windows) {
		if (in_n > raw_n)
			continue;
		std::vector<lda_stored_row> rows = rows_of(raw, in_n, (p + 10) >> 3);
		lda::sort_stored_rows(rows.data(), rows.size());
		const lda::stored_probe_rows by_rows = { rows.data(), rows.size() };
		for (uint64_t dev_bytes : { in_n, in_n > 100 ? in_n - 100 : in_n })
			for (uint64_t group : groups) {
				const walked a = walk(by_bytes, p, raw_n, dev_bytes, group);
				const walked b = walk(by_rows, p, raw_n, dev_bytes, group);
				CHECK(a == b, "%s: p %llu in_n %llu dev_bytes %llu group %llu: bytes %zu chunks stop %llu "
				      "fin %d, rows %zu chunks stop %llu fin %d", what, (unsigned long long)p,
				      (unsigned long long)in_n, (unsigned long long)dev_bytes,
				      (unsigned long long)group, a.chunks.size(), (unsigned long long)a.stop, a.fin,
				      b.chunks.size(), (unsigned long long)b.stop, b.fin);
			}
		/* rows a full queue lost: the walk stops earlier, never elsewhere -
		 * block by block (group 1) it is a prefix of the whole walk */
		for (int round = 0; round < 4; round++) {
			std::vector<lda_stored_row> kept;
			for (const lda_stored_row &r : rows)
				if (rng() & 1)
					kept.push_back(r);
			const lda::stored_probe_rows by_kept = { kept.data(), kept.size() };
			const walked a = walk(by_bytes, p, raw_n, in_n, 1);
			const walked b = walk(by_kept, p, raw_n, in_n, 1);
			bool prefix = b.chunks.size() <= a.chunks.size();
			for (size_t i = 0; prefix && i < b.chunks.size(); i++)
				prefix = a.chunks[i] == b.chunks[i];
			const uint64_t end = b.chunks.empty() ? p : std::get<1>(b.chunks.back());
			CHECK(prefix && b.stop == end && (!b.fin || (a.fin && b.stop == a.stop)),
			      "%s: p %llu in_n %llu, rows dropped: %zu of %zu chunks, stop %llu", what,
			      (unsigned long long)p, (unsigned long long)in_n, b.chunks.size(), a.chunks.size(),
			      (unsigned long long)b.stop);
			/* (and with grouping it never passes the whole walk's stop) */
			const walked c = walk(by_kept, p, raw_n, in_n, 8 * 16384);
			CHECK(c.stop <= a.stop, "%s: dropped rows walked past the stop", what);
		}
	}
}

int main(void)
{
	size_t cases = 0;
	/* level-0 streams of random payload, from every bit a header can start at */
	for (unsigned lead = 0; lead < 16; lead++) {
		writer w;
		for (unsigned i = 0; i < lead; i++)
			w.put((uint32_t)rng() & 1, 1);
		const uint64_t p = w.bit();
		const int nblocks = 3 + (int)(rng() % 6);
		for (int i = 0; i < nblocks; i++) {
			const size_t n = i % 3 == 0 ? 65535 : (size_t)(rng() % 70000) % 65536;
			w.stored(random_payload(n), i == nblocks - 1, (uint32_t)n);
		}
		for (int k = 0; k < 11; k++)	/* (a footer and trailing bytes behind the stream) */
			w.b.push_back((uint8_t)rng());
		compare("random payload", w.b, w.b.size() - 11, p);
		compare("random payload, the buffer's end", w.b, w.b.size(), p);
		cases += 2;
	}
	/* empty stored blocks (what a full flush leaves), many small ones */
	for (unsigned lead = 0; lead < 8; lead++) {
		writer v;
		v.put(0x5A, lead);
		const uint64_t p = v.bit();
		for (int i = 0; i < 3000; i++) {
			const size_t n = i % 7 == 0 ? (size_t)(rng() % 40) : 0;
			v.stored(random_payload(n), i == 2999, (uint32_t)n);
		}
		compare("empty and tiny blocks", v.b, v.b.size(), p);
		cases++;
	}
	/* 00 00 FF FF repeated: every fourth offset of the payload is a false row */
	for (unsigned lead = 0; lead < 4; lead++) {
		writer w;
		w.put(0x3, lead);
		const uint64_t p = w.bit();
		for (int i = 0; i < 6; i++)
			w.stored(pattern_payload(i == 2 ? 17 : 65532 + (size_t)(i & 3)), i == 5,
				 i == 2 ? 17u : 65532u + (uint32_t)(i & 3));
		compare("00 00 FF FF payload", w.b, w.b.size(), p);
		cases++;
	}
	/* a final block whose LEN passes the stream's end (raw_n) or the window */
	for (uint32_t over : { 1u, 2u, 8u, 1000u }) {
		writer w;
		const uint64_t p = w.bit();
		w.stored(random_payload(5000), false, 5000);
		w.stored(random_payload(3000), true, 3000 + over);
		compare("LEN past the end", w.b, w.b.size(), p);
		for (uint32_t k = 0; k < over + 4 && k < 16; k++)
			w.b.push_back((uint8_t)rng());
		compare("LEN into the footer", w.b, w.b.size() - std::min<uint32_t>(over + 4, 16), p);
		cases += 2;
	}
	/* a damaged NLEN in the middle of a run */
	{
		writer w;
		w.stored(random_payload(4000), false, 4000);
		w.stored(random_payload(4000), false, 4000);
		w.stored(random_payload(4000), false, 4000, false);
		w.stored(random_payload(4000), true, 4000);
		compare("damaged NLEN", w.b, w.b.size(), 0);
		cases++;
	}
	/* a run that stops at a Huffman block: a static and a dynamic header, the
	 * reserved type, at every bit position */
	for (uint32_t type : { 1u, 2u, 3u })
		for (unsigned lead = 0; lead < 8; lead++) {
			writer w;
			w.put(0x77, lead);
			const uint64_t p = w.bit();
			for (int i = 0; i < 5; i++)
				w.stored(random_payload(1 + (size_t)(rng() % 3000)), false, 0);
			/* (LEN 0 with payload behind it: the payload is read as headers) */
			writer v;
			v.put(0x77, lead);
			for (int i = 0; i < 5; i++) {
				const size_t n = (size_t)(rng() % 30000);
				v.stored(random_payload(n), false, (uint32_t)n);
			}
			v.put(rng() & 1, 1);
			v.put(type, 2);
			for (int i = 0; i < 200; i++)
				v.put((uint32_t)rng(), 8);
			compare("stops at a Huffman block", v.b, v.b.size(), p);
			compare("payload read as headers", w.b, w.b.size(), p);
			cases += 2;
		}
	/* a walk that begins where no stored block is, and at the very end */
	{
		bytes junk = random_payload(5000);
		for (uint64_t p : { (uint64_t)0, (uint64_t)1, (uint64_t)77, (uint64_t)8 * 4999, (uint64_t)8 * 5000 - 3,
				    (uint64_t)8 * 5000 })
			compare("junk", junk, junk.size(), p);
		cases += 6;
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("stored rows ok: %zu streams\n", cases);
	return 0;
}
