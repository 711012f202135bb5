"""What a size query must answer, and the streams it is asked about: shared by
tests/test_sizes_gpu.py and tools/fuzz_inflate.py --sizes.

The expectation comes from a CPU decoder `cpu` (the reference through
tests/oracle_util.Ref in the tests), never from the library's own decode:
  - cpu.decompress_ex(fmt, stream, limit) returns SUCCESS or
    INSUFFICIENT_SPACE: that, with its actual_in / actual_out;
  - it returns BAD_DATA and the format is zlib / gzip: the container header is
    parsed HERE (its rules are the reference's, lib/zlib_decompress.c:45-72 and
    lib/gzip_decompress.c:45-107), the raw stream behind it is decoded, and
    when that succeeds, the footer is present and (gzip) ISIZE equals the
    count modulo 2^32, the size query has nothing left to object to - the
    checksum of bytes nobody produced is the one thing it does not check:
    SUCCESS with header + raw + footer bytes ("checksum-only");
  - anything else: BAD_DATA.
"""
import random
import struct
import zlib

from tests import datagen, deflate_synth, streams

SUCCESS, BAD_DATA, INSUFFICIENT_SPACE = 0, 1, 3
FOOTER = {"deflate": 0, "zlib": 4, "gzip": 8}
LIMIT_MAX = 0xFFFFFFFF
# a case's limit None: the call's "no limit" (NULL, or LIMIT_MAX).  The CPU
# decoder gets CPU_NOLIMIT of room instead of 4 GiB: no stream here is longer
NOLIMIT = None
CPU_NOLIMIT = 8 << 20


def header_len(fmt, s):
    """bytes of a VALID container header, None for an invalid one"""
    if fmt == "deflate":
        return 0
    if fmt == "zlib":
        if len(s) < 6:
            return None
        h = (s[0] << 8) | s[1]
        if h % 31 or (s[0] & 15) != 8 or (s[0] >> 4) > 7 or (s[1] & 0x20):
            return None
        return 2
    if len(s) < 18 or s[0] != 0x1F or s[1] != 0x8B or s[2] != 8 or (s[3] & 0xE0):
        return None
    flg, p, end = s[3], 10, len(s)
    if flg & 4:
        xlen = s[p] | (s[p + 1] << 8)
        p += 2
        if end - p < xlen + 8:
            return None
        p += xlen
    for bit in (8, 16):
        if flg & bit:
            while True:
                c = s[p]
                p += 1
                if c == 0 or p == end:
                    break
            if end - p < 8:
                return None
    if flg & 2:
        p += 2
        if end - p < 8:
            return None
    return p


def expect(cpu, fmt, s, limit):
    """-> (result, actual_in, size, class); class: success / space / checksum / bad"""
    if limit is None:
        limit = CPU_NOLIMIT
    r, ain, aout, _ = cpu.decompress_ex(fmt, s, limit)
    if r == SUCCESS:
        return (SUCCESS, ain, aout, "success")
    if r == INSUFFICIENT_SPACE:
        return (INSUFFICIENT_SPACE, 0, 0, "space")
    if fmt != "deflate":
        h = header_len(fmt, s)
        if h is not None:
            r2, ain2, aout2, _ = cpu.decompress_ex("deflate", s[h:], limit)
            foot = FOOTER[fmt]
            if r2 == SUCCESS and len(s) >= h + ain2 + foot:
                at = h + ain2
                if fmt == "zlib" or \
                        struct.unpack("<I", s[at + 4:at + 8])[0] == aout2 & 0xFFFFFFFF:
                    return (SUCCESS, at + foot, aout2, "checksum")
    return (BAD_DATA, 0, 0, "bad")


def one_codeword_length_streams():
    """the streams of test_codes_of_one_codeword_length (tests/test_inflate_gpu.py)"""
    import numpy as np
    rng = np.random.default_rng(0xC0DE)
    out = []
    for vals, n in ((128, 70000), (64, 30000), (16, 9000), (2, 5000), (200, 66000), (256, 40000)):
        data = rng.integers(0, vals, n, dtype=np.uint8).tobytes()
        data = data[:n // 2] + data[100:400] + data[n // 2:]
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9,
                              zlib.Z_HUFFMAN_ONLY if vals != 200 else zlib.Z_DEFAULT_STRATEGY)
        out.append((f"onelen{vals}", co.compress(data) + co.flush(), data))
    return out


def _wrap(raw, data):
    """a raw stream as (fmt, stream) in the three containers"""
    return [("deflate", raw),
            ("zlib", b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))),
            ("gzip", b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw +
             struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF))]


def verdict_corpus():
    """-> list of (fmt, stream, limit, tag)"""
    cases = [(f, s, a, t) for f, s, a, want, t in streams.random_cases(11, 400) if want]
    cases += [(f, s, a, t) for f, s, a, want, t in streams.garbage_cases(22, 600)]
    rng = random.Random(0x512E5)

    def valid(tag, raw, data):
        """exact limit, one short, none; truncated; and inside zlib / gzip with
        a wrong checksum, a wrong ISIZE, a missing footer byte"""
        n = len(data)
        for fmt, s in _wrap(raw, data):
            cases.append((fmt, s, n, f"{tag}/{fmt}"))
            if fmt == "deflate":
                cases.append((fmt, s, NOLIMIT, f"{tag}/nolimit"))
                if n:
                    cases.append((fmt, s, n - 1, f"{tag}/short1"))
                    cases.append((fmt, s, n // 2, f"{tag}/half"))
                cases.append((fmt, s[:len(s) * 2 // 3], n, f"{tag}/cut"))
                cases.append((fmt, s[:-1], n, f"{tag}/cut1"))
            else:
                bad = bytearray(s)
                bad[-FOOTER[fmt]] ^= 0x40            # the checksum's first byte
                cases.append((fmt, bytes(bad), n, f"{tag}/{fmt}/sum"))
                cases.append((fmt, s[:-1], n, f"{tag}/{fmt}/footcut"))
                if fmt == "gzip":
                    bad = bytearray(s)
                    bad[-4] ^= 1                     # ISIZE
                    cases.append((fmt, bytes(bad), n, f"{tag}/gzip/isize"))

    for i, (s, want) in enumerate([streams.incomplete_empty_offset_code(),
                                   streams.incomplete_singleton_litlen(),
                                   streams.incomplete_singleton_offset(False),
                                   streams.incomplete_singleton_offset(True)]):
        valid(f"incomplete{i}", s, want)
    cases.append(("deflate", streams.too_many_codeword_lengths(), 1000, "toomany"))
    cases.append(("deflate", streams.overread_stream(), 128, "overread"))
    cases.append(("deflate", streams.overread_stream(), NOLIMIT, "overread/nolimit"))
    for i, s in enumerate(streams.bad_distance_streams()):
        cases.append(("deflate", s, 400000, f"baddist{i}"))
        cases.append(("deflate", s, NOLIMIT, f"baddist{i}/nolimit"))
        cases.append(("deflate", s, 100, f"baddist{i}/limit100"))
    for name, s, want in streams.parallel_round_streams():
        valid(name, s, want)
        for _ in range(3):
            bad = bytearray(s)
            bad[rng.randrange(20, len(s) - 10)] ^= 1 << rng.randrange(8)
            cases.append(("deflate", bytes(bad), len(want), f"{name}/flip"))
    for i, (s, want) in enumerate(streams.stored_then_match_streams()):
        valid(f"stored{i}", s, want)
    for i, (s, want) in enumerate(streams.static_dynamic_static_streams()):
        valid(f"sds{i}", s, want)
    for i, (s, want) in enumerate(streams.gzip_optional_field_streams()):
        cases.append(("gzip", s, len(want), f"gzopt{i}"))
        cases.append(("gzip", s, len(want) - 1, f"gzopt{i}/short"))
        bad = bytearray(s)
        bad[-6] ^= 0x10                              # CRC-32
        cases.append(("gzip", bytes(bad), len(want), f"gzopt{i}/sum"))
        cases.append(("gzip", s[:len(s) // 3], len(want), f"gzopt{i}/cut"))
    for name, s in (("emptystatic", streams.empty_static_blocks()),
                    ("emptydynamic", streams.empty_dynamic_blocks())):
        cases.append(("deflate", s, 0, name))
        cases.append(("deflate", s, 1000, name + "/room"))
    for name, s, want in one_codeword_length_streams():
        valid(name, s, want)
    for c in deflate_synth.corpus():
        cases.append((c.fmt, c.data, c.avail, "synth:" + c.name))
        if c.valid and len(c.out):
            cases.append((c.fmt, c.data, len(c.out) - 1, "synth:" + c.name + "/short"))
    return cases


def valid_streams(ref):
    """-> list of (fmt, stream, data, tag): every format, levels 0 / 1 / 6 / 9 /
    12 of the reference and zlib's (Z_FIXED and Huffman-only included), the
    sizes of the issue, the datagen kinds"""
    out = []
    sizes = [0, 1, 31, 4096, 65536, 70000, 1 << 20]
    for i, n in enumerate(sizes):
        for kind in range(8) if n in (4096, 65536) else (i % 8,):
            d = datagen.chunk(kind, n, 0x0E115120 + i)
            for fmt in ("deflate", "zlib", "gzip"):
                for lvl in (0, 1, 6, 9, 12):
                    if n == 1 << 20 and lvl in (9, 12) and fmt != "gzip":
                        continue
                    out.append((fmt, ref.compress(fmt, lvl, d), d, f"ref/n{n}/k{kind}/l{lvl}"))
                    if lvl <= 9 and kind == i % 8:
                        out.append((fmt, streams._zcompress(fmt, lvl, d), d,
                                    f"zlib/n{n}/k{kind}/l{lvl}"))
                if kind == i % 8:
                    wbits = {"deflate": -15, "zlib": 15, "gzip": 31}[fmt]
                    for name, strat in (("fixed", zlib.Z_FIXED), ("huff", zlib.Z_HUFFMAN_ONLY)):
                        co = zlib.compressobj(6, zlib.DEFLATED, wbits, 9, strat)
                        out.append((fmt, co.compress(d) + co.flush(), d, f"zlib/n{n}/{name}"))
    return out
