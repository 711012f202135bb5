/*
 * test_tar_write_plan.cpp - the host arithmetic of libdeflate_amd_tar_write_batch
 * and libdeflate_amd_targz_compress_batch (csrc/tar_write_plan.h) on the CPU:
 * every refusal, one case per cause, the UTF-8 check, the self-counting length
 * of the pax record, and the entries' offsets, the archive's size and the
 * index rows against a plain serial model, for entry sizes from 0 to 8^11 - 1
 * and for archives whose two end blocks just fit a 10 240-byte record or just
 * spill into another.  Stand-alone; tests/test_tar_write_plan.py builds it under
 * the address and undefined-behaviour sanitizers and runs it:
 *   c++ -std=c++17 -fsanitize=address,undefined -I libdeflate_amd/csrc \
 *       -o test_tar_write_plan tools/test_tar_write_plan.cpp && ./test_tar_write_plan
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tar_write_plan.h"

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

struct Entry {
	std::string name;
	uint64_t src, size;
};

/* the arrays the calls take, each exactly as long as it has to be (the
 * sanitizer sees a read past any of them); the names begin at `lead` */
struct Args {
	std::vector<uint8_t> names;
	std::vector<uint64_t> name_offsets, in_offsets, in_nbytes;
	Args(const std::vector<Entry> &e, uint64_t lead = 0)
	{
		names.assign((size_t)lead, 'x');
		name_offsets.push_back(lead);
		for (const Entry &x : e) {
			names.insert(names.end(), x.name.begin(), x.name.end());
			name_offsets.push_back(names.size());
			in_offsets.push_back(x.src);
			in_nbytes.push_back(x.size);
		}
	}
};

static bool build(const std::vector<Entry> &e, uint64_t in_avail, const uint64_t *out_avail,
		  uint64_t mtime, unsigned flags, tarw_plan &p, std::string &err, uint64_t lead = 0)
{
	Args a(e, lead);
	return tarw_plan_build(e.size(), a.names.data(), a.name_offsets.data(), a.in_offsets.data(),
			       a.in_nbytes.data(), in_avail, out_avail, mtime, flags, p, err);
}

/* ---- the serial model: an archive written entry by entry ---- */

static uint64_t round_up(uint64_t v, uint64_t to)
{
	return (v + to - 1) / to * to;
}

struct Model {
	std::vector<uint64_t> off, pax, rows;
	uint64_t size;
};

static Model model(const std::vector<Entry> &e, uint64_t mtime)
{
	Model m;
	uint64_t pos = 0, out_off = 0;

	for (const Entry &x : e) {
		size_t chars = 0;
		bool high = false;
		for (unsigned char c : x.name) {
			chars += (c & 0xC0) != 0x80;
			high = high || c >= 0x80;
		}
		uint64_t name_at, n = 0, src = 0;
		m.off.push_back(pos);
		if (high || chars > 100) {
			/* the record whose printed length is its own */
			char head[32];
			int d = 0;
			for (n = x.name.size() + 8;; n++) {
				d = snprintf(head, sizeof(head), "%llu path=", (unsigned long long)n);
				if ((uint64_t)d + x.name.size() + 1 == n)
					break;
			}
			pos += 512;			/* the pax header */
			name_at = pos + (uint64_t)d;
			pos += round_up(n, 512);	/* the pax data */
			src = 2;
		} else {
			name_at = pos;
		}
		m.pax.push_back(n);
		const uint64_t hdr = pos;
		pos += 512;
		const uint64_t row[8] = { hdr, name_at, x.name.size(), '0' | src << 8, pos, x.size, mtime,
					  out_off };
		m.rows.insert(m.rows.end(), row, row + 8);
		pos += round_up(x.size, 512);
		out_off += x.size;
	}
	m.size = round_up(pos + 1024, 10240);
	return m;
}

static void check_against_model(const std::vector<Entry> &e, uint64_t mtime, uint64_t lead)
{
	tarw_plan p;
	std::string err;
	uint64_t in_avail = 0;
	for (const Entry &x : e)
		if (x.src + x.size > in_avail)
			in_avail = x.src + x.size;
	const Model m = model(e, mtime);
	CHECK(build(e, in_avail, &m.size, mtime, 0, p, err, lead));
	if (!err.empty())
		printf("  %s\n", err.c_str());
	CHECK(p.n == e.size() && p.size == m.size && p.end + 1024 <= p.size &&
	      p.size - p.end < 1024 + 10240 && p.size % 10240 == 0);
	uint64_t name_at = 0;
	for (size_t k = 0; k < e.size(); k++) {
		const uint64_t *r = &p.erows[TARW_ECOLS * k];
		CHECK(r[TARW_E_OFF] == m.off[k] && r[TARW_E_PAX] == m.pax[k]);
		CHECK(r[TARW_E_NAME_OFF] == name_at && r[TARW_E_NAME_LEN] == e[k].name.size());
		CHECK(r[TARW_E_SRC] == e[k].src && r[TARW_E_SIZE] == e[k].size);
		name_at += e[k].name.size();
	}
	std::vector<uint64_t> rows(TARW_ROW_WORDS * e.size() + 1, 0x55);
	tarw_rows(p, mtime, rows.data());
	CHECK(rows.back() == 0x55);
	rows.pop_back();
	CHECK(rows == m.rows);
	/* the size query agrees */
	Args a(e, lead);
	CHECK(tarw_size(e.size(), a.name_offsets.data(), a.names.data(), a.in_nbytes.data()) == m.size);
	/* one byte short is refused, no limit at all is not */
	const uint64_t less = m.size - 1;
	CHECK(!build(e, in_avail, &less, mtime, 0, p, err, lead) &&
	      err.find("out_avail") != std::string::npos);
	CHECK(build(e, in_avail, NULL, mtime, 0, p, err, lead));
}

static std::string utf8_name(size_t chars, unsigned step)
{
	/* 1-, 2-, 3- and 4-byte characters in turn */
	static const char *const c[] = { "a", "\xC3\xA9", "\xE2\x82\xAC", "\xF0\x9F\x98\x80" };
	std::string s;
	for (size_t i = 0; i < chars; i++)
		s += c[(i * step) % 4];
	return s;
}

static void test_layout(void)
{
	const uint64_t top = ((uint64_t)1 << 33) - 1;	/* 8^11 - 1 */
	/* sizes and names at every edge, each alone and then all together */
	std::vector<Entry> all;
	const uint64_t sizes[] = { 0, 1, 511, 512, 513, 65024, 65535, 65536, 65537, 200000, top };
	for (uint64_t s : sizes)
		all.push_back({ "f" + std::to_string(s), 3, s });
	const size_t ascii[] = { 1, 99, 100, 101, 600, 65535 };
	for (size_t l : ascii)
		all.push_back({ std::string(l, 'n'), 0, 7 });
	all.push_back({ std::string(98, 'n') + "\xC3\xA9", 1, 513 });	/* 100 bytes, 99 characters */
	all.push_back({ utf8_name(100, 1), 0, 0 });
	all.push_back({ utf8_name(101, 3), 0, 1 });
	all.push_back({ utf8_name(300, 1), 0, 512 });
	/* the record's length on each side of the steps of its decimal: with
	 * d digits it is name + 7 + d, so 99 is 90 + 9, the next name gives
	 * 101, and 999 -> 1001 likewise (100 and 1000 are never a length) */
	for (size_t l : { 90, 91, 92, 989, 990, 991, 9988, 9989, 9990 })
		all.push_back({ std::string(l - 2, 'p') + "\xC3\xA9", 0, 5 });
	for (const Entry &x : all)
		check_against_model({ x }, 1234567, 0);
	check_against_model(all, top, 5);
	check_against_model({}, 0, 0);
	{	/* the steps themselves, by the rule */
		CHECK(tarw_pax_len(90) == 99 && tarw_pax_len(91) == 101 && tarw_pax_len(92) == 102);
		CHECK(tarw_pax_len(989) == 999 && tarw_pax_len(990) == 1001);
		CHECK(tarw_pax_len(9988) == 9999 && tarw_pax_len(9989) == 10001);
		CHECK(tarw_pax_len(1) == 9 && tarw_pax_len(2) == 11 && tarw_pax_len(65535) == 65547);
	}
	/* the two end blocks just fit the record, or just spill into another:
	 * one entry of s bytes is 512 + round_up(s) + 1024 before the rounding */
	for (uint64_t records = 1; records <= 3; records++) {
		const uint64_t fits = records * 10240 - 1536;	/* the largest data that fits */
		struct { uint64_t size, want; } cases[] = {
			{ fits, records * 10240 }, { fits - 511, records * 10240 },
			{ fits + 1, (records + 1) * 10240 }, { fits - 512, records * 10240 },
			{ fits + 512, (records + 1) * 10240 },
		};
		for (auto &c : cases) {
			tarw_plan p;
			std::string err;
			CHECK(build({ { "e", 0, c.size } }, c.size, NULL, 0, 0, p, err) && p.size == c.want);
			check_against_model({ { "e", 0, c.size } }, 0, 0);
		}
	}
	/* random archives */
	for (int round = 0; round < 200; round++) {
		std::vector<Entry> e(rnd() % 30);
		for (Entry &x : e) {
			const unsigned kind = rnd() % 4;
			x.name = kind == 0 ? std::string(1 + rnd() % 100, 'a') :
				 kind == 1 ? std::string(101 + rnd() % 1500, 'b') :
					     utf8_name(1 + rnd() % 300, 1 + rnd() % 3);
			x.src = rnd() % 1000;
			x.size = rnd() % 3 ? rnd() % 3000 : rnd() % 200000;
		}
		check_against_model(e, rnd() % ((uint64_t)1 << 33), rnd() % 3);
	}
}

static void refused(int line, const char *word, uint64_t in_avail, uint64_t mtime, unsigned flags,
		    const std::vector<Entry> &e)
{
	tarw_plan p;
	std::string err;
	if (build(e, in_avail, NULL, mtime, flags, p, err) || err.find(word) == std::string::npos) {
		printf("FAILED line %d: not refused with \"%s\" (%s)\n", line, word, err.c_str());
		failures++;
	}
}
/* (the entries last: their braces hold commas) */
#define REFUSED(word, avail, mtime, flags, ...) refused(__LINE__, word, avail, mtime, flags, __VA_ARGS__)

static void test_refusals(void)
{
	typedef std::vector<Entry> E;
	const uint64_t lim = (uint64_t)1 << 33;
	tarw_plan p;
	std::string err;

	CHECK(build(E{ { "a", 0, 4 } }, 4, NULL, lim - 1, 0, p, err));
	REFUSED("flags", 4, 0, 1, E{ { "a", 0, 4 } });
	REFUSED("mtime", 4, lim, 0, E{ { "a", 0, 4 } });
	REFUSED("empty name", 4, 0, 0, E{ { "", 0, 4 } });
	REFUSED("65535", 4, 0, 0, E{ { std::string(65536, 'n'), 0, 4 } });
	CHECK(build(E{ { std::string(65535, 'n'), 0, 4 } }, 4, NULL, 0, 0, p, err));
	REFUSED("0 byte", 4, 0, 0, E{ { std::string("a\0b", 3), 0, 4 } });
	/* a lone continuation byte, a lead byte at the end, a cut sequence, an
	 * overlong form, a surrogate, above U+10FFFF, a byte that is never UTF-8 */
	for (const char *bad : { "a\x80", "a\xC3", "a\xE2\x82", "\xC0\xAF", "\xE0\x80\xAF", "\xED\xA0\x80",
				 "\xF4\x90\x80\x80", "\xF8\x88\x80\x80\x80", "\xFF", "\xC3\x28" })
		REFUSED("UTF-8", 4, 0, 0, E{ { bad, 0, 4 } });
	for (const char *good : { "\xC2\x80", "\xED\x9F\xBF", "\xEE\x80\x80", "\xF4\x8F\xBF\xBF", "\xE0\xA0\x80" })
		CHECK(build(E{ { good, 0, 4 } }, 4, NULL, 0, 0, p, err));
	REFUSED("8 GiB", lim, 0, 0, E{ { "a", 0, lim } });
	CHECK(build(E{ { "a", 0, lim - 1 } }, lim - 1, NULL, 0, 0, p, err));
	REFUSED("in_avail", 4, 0, 0, E{ { "a", 1, 4 } });
	REFUSED("in_avail", 4, 0, 0, E{ { "a", 5, 0 } });
	CHECK(build(E{ { "a", 4, 0 } }, 4, NULL, 0, 0, p, err));
	REFUSED("in_avail", 4, 0, 0, E{ { "a", ~(uint64_t)0, 2 } });
	/* the second entry's fault is found */
	REFUSED("entry 1", 4, 0, 0, (E{ { "a", 0, 4 }, { "b", 3, 2 } }));
	{	/* decreasing offsets: the arrays by hand */
		const uint8_t names[4] = { 'a', 'b', 'c', 'd' };
		const uint64_t no[3] = { 2, 4, 3 }, io[2] = { 0, 0 }, in[2] = { 1, 1 };
		CHECK(!tarw_plan_build(2, names, no, io, in, 1, NULL, 0, 0, p, err) &&
		      err.find("decrease") != std::string::npos);
		CHECK(tarw_size(2, no, names, in) == 0);
	}
	{	/* a count above 2^28 is refused before any array is walked */
		const uint64_t one[2] = { 0, 1 };
		const uint8_t name[1] = { 'a' };
		CHECK(!tarw_plan_build(TARW_MAX_ENTRIES + 1, name, one, one, one, 1, NULL, 0, 0, p, err) &&
		      err.find("2^28") != std::string::npos);
		CHECK(tarw_size(TARW_MAX_ENTRIES + 1, one, name, one) == 0);
		const uint64_t big[1] = { (uint64_t)1 << 33 };
		CHECK(tarw_size(1, one, name, big) == 0);
	}
	{	/* the size query refuses what the plan refuses of names */
		const uint8_t bad[2] = { 'a', 0x80 };
		const uint64_t no[2] = { 0, 2 }, none[2] = { 0, 0 }, in[1] = { 1 };
		CHECK(tarw_size(1, no, bad, in) == 0 && tarw_size(1, none, bad, in) == 0);
	}
	{	/* 127 entries of 8 GiB - 1 stay below 1 TiB, 128 do not */
		E e(127, Entry{ "big", 0, lim - 1 });
		CHECK(build(e, lim, NULL, 0, 0, p, err) && p.size <= TARW_MAX_ARCHIVE);
		e.push_back(Entry{ "big", 0, lim - 1 });
		REFUSED("1 TiB", lim, 0, 0, e);
		Args a(e);
		CHECK(tarw_size(e.size(), a.name_offsets.data(), a.names.data(), a.in_nbytes.data()) == 0);
	}
	/* no entries: ten kilobytes of zeros, and no room less */
	const uint64_t room[2] = { 10239, 10240 };
	CHECK(!build(E{}, 0, &room[0], 0, 0, p, err) && err.find("out_avail") != std::string::npos);
	CHECK(build(E{}, 0, &room[1], 0, 0, p, err) && p.size == 10240 && p.end == 0 && p.n == 0);
	CHECK(tarw_size(0, NULL, NULL, NULL) == 10240);
}

/*
 * `rows FILE`: the plan of the entries in FILE - u64 n, mtime, n + 1 name
 * offsets, n sizes, then the names' bytes - printed as the archive's size and
 * n index rows of 8 words: tests/test_tar_write_abi.py compares them with what
 * Python's tarfile wrote for the same entries.
 */
static int print_rows(const char *path)
{
	FILE *f = fopen(path, "rb");
	uint64_t head[2];
	if (!f || fread(head, 8, 2, f) != 2)
		return 2;
	const size_t n = (size_t)head[0];
	std::vector<uint64_t> no(n + 1), sizes(n), offs(n, 0), rows(TARW_ROW_WORDS * n);
	if (fread(no.data(), 8, n + 1, f) != n + 1 || fread(sizes.data(), 8, n, f) != n)
		return 2;
	std::vector<uint8_t> names((size_t)no[n]);
	if (fread(names.data(), 1, names.size(), f) != names.size())
		return 2;
	fclose(f);
	tarw_plan p;
	std::string err;
	if (!tarw_plan_build(n, names.data(), no.data(), offs.data(), sizes.data(), ~(uint64_t)0, NULL,
			     head[1], 0, p, err)) {
		printf("refused: %s\n", err.c_str());
		return 1;
	}
	tarw_rows(p, head[1], rows.data());
	printf("%llu\n", (unsigned long long)p.size);
	for (size_t k = 0; k < n; k++) {
		for (size_t w = 0; w < TARW_ROW_WORDS; w++)
			printf("%llu ", (unsigned long long)rows[TARW_ROW_WORDS * k + w]);
		printf("\n");
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "rows"))
		return print_rows(argv[2]);
	test_refusals();
	test_layout();
	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("tar write plan ok\n");
	return 0;
}
