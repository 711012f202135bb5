"""What a prefix decompress must answer, and the streams it is asked about:
shared by tests/test_prefix_abi.py (CPU) and tests/test_prefix_gpu.py.

The expectation comes from a CPU decoder `cpu` (the reference through
tests/oracle_util.Ref in the tests) and from the known plaintext, never from
the library's own decode:
  - cpu.decompress_ex(fmt, stream, out_avail=limit) returns SUCCESS: that,
    with its actual_out and bytes;
  - it returns INSUFFICIENT_SPACE: PREFIX, actual_out = limit, and the bytes
    are plain[:limit] - of a stream without known plaintext (a damaged one)
    what zlib's inflate() gives with avail_out = limit, where it gives exactly
    that many bytes; where it does not, the cut may have fallen on a match
    whose offset is bad and nothing says what the answer is: bytes None;
  - anything else: that result, nothing more.

A case is a Case below; `want`, `aout` and `data` set by hand mark the few
places where the call has a rule of its own (include/libdeflate_amd.h).
"""
import random
import zlib

import numpy as np

from tests import datagen, deflate_synth, streams
from tests.streams import BitWriter, _dyn_header, _static_lit, _static_match

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, PREFIX = 0, 1, 2, 3, 19
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}
GUARD = 64      # bytes behind every case's limit that must stay as they were


def zlib_prefix(fmt, s, limit, dictionary=None):
    """zlib's inflate() with avail_out = limit -> bytes, or None where zlib
    objects to the stream before it has them"""
    if limit == 0:
        return b""      # (max_length = 0 means "no limit" to zlib)
    try:
        d = zlib.decompressobj(WBITS[fmt], dictionary) if dictionary else \
            zlib.decompressobj(WBITS[fmt])
        return d.decompress(bytes(s), limit)
    except zlib.error:
        return None


class Case:
    def __init__(self, fmt, s, limit, tag, plain=None, dictionary=None, want=None, aout=None,
                 data=None):
        self.fmt, self.s, self.limit, self.tag = fmt, bytes(s), limit, tag
        self.plain, self.dictionary = plain, dictionary
        # the expectation: filled in by expect() unless set by hand
        self.want, self.aout, self.data = want, aout, data
        self.ain = None         # the reference's actual_in of a SUCCESS (no dictionary)
        self.by_hand = want is not None

    def __repr__(self):
        return f"Case({self.tag}, {self.fmt}, limit {self.limit})"


def expect(cpu, c):
    """fill in c.want / c.aout / c.data (data None: not to be compared)"""
    if c.by_hand:
        return c
    if c.dictionary:
        # the reference has no dictionary call: a stored block holding the
        # window in front of the raw stream is the same decode
        raw = c.s if c.fmt == "deflate" else c.s[6:-4]
        pre, n = deflate_synth.stored_prefix(c.dictionary)
        r, _, aout, out = cpu.decompress_ex("deflate", pre + raw, n + c.limit)
        aout, out = aout - n, out[n:]
    else:
        r, ain, aout, out = cpu.decompress_ex(c.fmt, c.s, c.limit)
        c.ain = ain if r == SUCCESS else None
    if r == SUCCESS:
        c.want, c.aout, c.data = SUCCESS, aout, out
        if c.plain is not None:
            assert out == c.plain, c
    elif r == INSUFFICIENT_SPACE:
        c.want, c.aout = PREFIX, c.limit
        if c.plain is not None:
            c.data = c.plain[:c.limit]
            assert len(c.data) == c.limit, c
        else:
            z = zlib_prefix(c.fmt, c.s, c.limit)
            c.data = z if z is not None and len(z) == c.limit else None
            if c.data is None:
                c.want = None       # PREFIX, or BAD_DATA for a cut match's offset
    else:
        c.want, c.aout, c.data = r, None, None
    return c


def wrap3(raw, plain):
    return [("deflate", raw), ("zlib", deflate_synth.zlib_wrap(raw, plain)),
            ("gzip", deflate_synth.gzip_wrap(raw, plain))]


# ---- hand-built static blocks ----

def static_block(w, tokens, hist, final=1, eob=True):
    """tokens: an int (literal) or (length, distance); hist grows"""
    w.put(final, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            _static_match(w, *t)
            for _ in range(t[0]):
                hist.append(hist[-t[1]])
        else:
            _static_lit(w, t)
            hist.append(t)
    if eob:
        _static_lit(w, 256)


def static_stream(tokens, dictionary=b""):
    w, hist = BitWriter(), bytearray(dictionary)
    static_block(w, tokens, hist)
    return w.finish(), bytes(hist[len(dictionary):])


def _lits(n, seed):
    return list(random.Random(seed).randbytes(n))


def site_cases():
    """each of the three cut sites at its smallest shape, in the three formats"""
    out = []

    def sweep(tag, raw, plain, limits):
        for fmt, s in wrap3(raw, plain):
            for lim in limits:
                out.append(Case(fmt, s, lim, f"{tag}/{fmt}/{lim}", plain))

    raw, plain = static_stream(_lits(40, 1))
    sweep("litrun", raw, plain, [1, 2, 7, 20, 39])
    raw, plain = static_stream(_lits(8, 2) + [(3, 4)] + _lits(3, 3))
    sweep("match3", raw, plain, [8, 9, 10, 11, 12])
    raw, plain = static_stream(_lits(10, 4) + [(258, 10)] + _lits(2, 5))
    sweep("match258", raw, plain, range(10, 270))
    raw, plain = static_stream([65, (100, 1), 66, (258, 1)])
    sweep("dist1", raw, plain, [1, 2, 3, 9, 50, 100, 101, 102, 103, 110, 359])
    raw, plain = static_stream(_lits(5, 6) + [(50, 3)] + _lits(9, 7) + [(30, 7), (17, 16)])
    sweep("overlap", raw, plain, [5, 6, 7, 8, 9, 30, 54, 55, 64, 65, 70, 93, 94, 95, 110])
    raw, plain = static_stream(_lits(32768, 8) + [(20, 32768), 1, 2, (258, 32768)])
    sweep("dist32768", raw, plain, [32768, 32769, 32778, 32787, 32788, 32790, 32791, 32800,
                                    33047])
    # a stored block behind a Huffman block, cut at its first, middle and last byte
    w, hist = BitWriter(), bytearray()
    static_block(w, _lits(5, 9), hist, final=0)
    body = bytes(_lits(100, 10))
    w.put(1, 1)
    w.put(0, 2)
    stored = w.finish() + bytes([100, 0, 155, 255]) + body
    plain = bytes(hist) + body
    sweep("stored", stored, plain, [0, 4, 5, 6, 55, 104])
    # ... and a stored block alone, longer than a wave's step of 512 bytes
    body = bytes(_lits(3000, 11))
    raw = b"\x01" + bytes([3000 & 255, 3000 >> 8, ~3000 & 255, (~3000 >> 8) & 255]) + body
    sweep("stored3000", raw, body, [0, 1, 7, 8, 9, 511, 512, 513, 1500, 2999])
    return out


def stored_past_input_cases():
    """LEN says 100, 50 bytes follow: the limit cuts the block, and the block
    is checked against the input all the same.  The reference tests the room
    first and says INSUFFICIENT_SPACE; this call's rule is BAD_DATA, not PREFIX
    (the header states it): the expectation is set by hand."""
    raw = b"\x01" + bytes([100, 0, 155, 255]) + bytes(50)
    return [Case("deflate", raw, lim, f"storedpast/{lim}", want=BAD_DATA, aout=0)
            for lim in (0, 10, 50, 99)] + \
           [Case("deflate", raw, 100, "storedpast/100")]      # the reference: BAD_DATA


def dict_cases():
    """matches that begin in the preset dictionary: raw and zlib"""
    dictionary = bytes(_lits(1000, 12))
    out = []
    for name, toks, limits in (
            ("first", [(20, 10), 7], [0, 1, 9, 10, 11, 19, 20, 21]),
            ("after3", _lits(3, 13) + [(20, 10), 9, (258, 900)], [3, 4, 5, 9, 10, 11, 22, 23, 24,
                                                                 100, 281]),
            ("dist1", [(9, 1)], [1, 8]),
            ("whole", [(258, 1000), (258, 1000)], [1, 257, 258, 259, 515])):
        raw, plain = static_stream(toks, dictionary)
        for fmt, s in (("deflate", raw), ("zlib", deflate_synth.zlib_wrap(raw, plain, dictionary))):
            for lim in limits:
                out.append(Case(fmt, s, lim, f"dict/{name}/{fmt}/{lim}", plain, dictionary))
            out.append(Case(fmt, s, len(plain), f"dict/{name}/{fmt}/all", plain, dictionary))
    return dictionary, out


def edge_cases():
    out = []
    plain = datagen.text_chunk(5000, 0x9E0)
    n = len(plain)
    for fmt in ("deflate", "zlib", "gzip"):
        s = streams._zcompress(fmt, 6, plain)
        for lim in (0, 1, n - 1, n, n + 1, n + 8):
            out.append(Case(fmt, s, lim, f"edge/{fmt}/{lim}", plain))
        e = streams._zcompress(fmt, 6, b"")
        out.append(Case(fmt, e, 0, f"edge/{fmt}/empty0", b""))
        out.append(Case(fmt, e, 5, f"edge/{fmt}/empty5", b""))
        if fmt != "deflate":
            bad = bytearray(s)
            bad[-4 if fmt == "zlib" else -8] ^= 0x40        # the checksum
            out.append(Case(fmt, bad, n, f"edge/{fmt}/sum", None))
            out.append(Case(fmt, bad, n + 1, f"edge/{fmt}/sum+1", None))
            # cut: the footer is not looked at
            out.append(Case(fmt, bad, n - 1, f"edge/{fmt}/sum-1", plain))
    # a limit exactly at a block boundary; an empty non-final block, then data
    w, hist = BitWriter(), bytearray()
    static_block(w, _lits(10, 14), hist, final=0)
    at = (len(w.out), w.n)
    static_block(w, [], hist, final=0)
    static_block(w, _lits(5, 15), hist, final=1)
    raw, plain = w.finish(), bytes(hist)
    for fmt, s in wrap3(raw, plain):
        for lim in (9, 10, 11, 15):
            out.append(Case(fmt, s, lim, f"boundary/{fmt}/{lim}", plain))
    # the same boundary, then a block of the reserved type
    w, hist = BitWriter(), bytearray()
    static_block(w, _lits(10, 14), hist, final=0)
    assert (len(w.out), w.n) == at
    w.put(1, 1)
    w.put(3, 2)
    raw = w.finish() + bytes(8)
    for lim in (9, 10, 11):     # 9: the literal is cut before the header is seen
        out.append(Case("deflate", raw, lim, f"boundary/broken/{lim}", bytes(hist) if lim < 10
                        else None))
    return out


def empty_offset_code_stream(tokens):
    """a dynamic block whose litlen code is {A: 1 bit, end of block: 2, length
    3: 2} and whose offset code has no codeword at all (the incomplete code of
    programs/test_incomplete_codes.c:75-147); tokens: "A", "M" (a match of
    length 3; its offset codeword is one bit, as the reference reads it)"""
    w = BitWriter()
    code = {0: 0, 1: 1, 2: 2, 18: 3}
    _dyn_header(w, 1, 258, 1, {0: 2, 1: 2, 2: 2, 18: 2})

    def zeros(n):
        while n:
            r = min(n, 138)
            assert r >= 11
            w.put_code(code[18], 2)
            w.put(r - 11, 7)
            n -= r
    zeros(65)
    w.put_code(code[1], 2)          # 'A': 1 bit
    zeros(190)                      # 66 .. 255
    w.put_code(code[2], 2)          # 256: 2 bits
    w.put_code(code[2], 2)          # 257 (length 3): 2 bits
    w.put_code(code[0], 2)          # the one offset length: 0
    for t in tokens:
        if t == "A":
            w.put_code(0, 1)
        else:
            w.put_code(3, 2)
            w.put(0, 1)
    w.put_code(2, 2)
    return w.finish()


def bad_offset_cases():
    """The cut match with a bad offset.  THE ONLY PLACE WITHOUT A REFERENCE
    VERDICT: the reference stops at a match without room before it reads the
    offset and says INSUFFICIENT_SPACE for all of these; this call decodes the
    offset by the rules of a match that fits, and its rule (the header's) is
    BAD_DATA with actual_out = 0.  Set by hand."""
    out = []
    # the distance reaches before the stream
    w, hist = BitWriter(), bytearray(_lits(4, 16))
    w.put(1, 1)
    w.put(1, 2)
    for b in hist:
        _static_lit(w, b)
    _static_match(w, 10, 8)
    _static_lit(w, 256)
    raw = w.finish()
    for lim in (4, 5, 13):
        out.append(Case("deflate", raw, lim, f"badoff/before/{lim}", want=BAD_DATA, aout=0))
    out.append(Case("deflate", raw, 3, "badoff/before/3", bytes(hist)))     # cut in the literals
    # the offset symbol is unused: the block's offset code is empty.  A match
    # that fits reads one bit and takes symbol 0, distance 1, as the reference
    # does with an incomplete code - so the offset is bad only where distance 1
    # reaches before the stream, and a prefix like any other behind a byte
    s = empty_offset_code_stream(["M"])
    for lim in (0, 1, 2):
        out.append(Case("deflate", s, lim, f"badoff/unused/first/{lim}", want=BAD_DATA, aout=0))
    s = empty_offset_code_stream(["A", "M", "A"])
    for lim in (1, 2, 3, 4):
        out.append(Case("deflate", s, lim, f"badoff/unused/behindA/{lim}", b"AAAAA"))
    out.append(Case("deflate", s, 5, "badoff/unused/behindA/5", b"AAAAA"))
    # the input ends inside the offset's bits (the distance itself would do:
    # 16400 bytes stand in front of it)
    lits = _lits(16400, 17)
    w = BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    for b in lits:
        _static_lit(w, b)
    _static_lit(w, 285)             # length 258, no extra bits
    keep = len(w.out) + (1 if w.n else 0)
    w.put_code(28, 5)               # distance 16385 + 13 extra bits
    w.put(0, 13)
    _static_lit(w, 256)
    whole = w.finish()
    assert len(whole) > keep + 1
    for cut in (keep, keep + 1):
        for lim in (16400, 16401, 16500, 16657):
            out.append(Case("deflate", whole[:cut], lim, f"badoff/inputends/{cut - keep}/{lim}",
                            want=BAD_DATA, aout=0))
    out.append(Case("deflate", whole, 16500, "badoff/inputends/whole", bytes(lits) + bytes(lits[15:273])))
    return out


# ---- the hand-over from the parallel rounds ----

def handover_streams(ref):
    """(tag, raw, plain): 24 to 64 KiB of text and mixed data at levels 1 / 6 /
    12, static codes only, codes of one codeword length"""
    out = []
    for i, (kind, n) in enumerate(((0, 24 << 10), (1, 40000), (5, 65536))):
        plain = datagen.chunk(kind, n, 0x9A0 + i)
        for lvl in (1, 6, 12):
            out.append((f"k{kind}/l{lvl}", ref.compress("deflate", lvl, plain), plain))
    plain = datagen.text_chunk(30000, 0x9A7)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    out.append(("fixed", co.compress(plain) + co.flush(), plain))
    plain = np.random.default_rng(0x9A8).integers(0, 256, 40000, dtype=np.uint8).tobytes()
    plain = plain[:20000] + plain[100:400] + plain[20000:]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    out.append(("onelen", co.compress(plain) + co.flush(), plain))
    return out


ROUND_IN = 64 * 384 // 8        # input bytes of one parallel round


def handover_cases(ref):
    out = []
    for tag, raw, plain in handover_streams(ref):
        n = len(plain)
        # about where the first round's output ends: what the round's input
        # span decodes to (zlib gives what it can of a truncated input); the
        # block header in front moves it a little, so the limits bracket it
        first = len(zlib_prefix("deflate", raw[:ROUND_IN], n) or b"")
        second = len(zlib_prefix("deflate", raw[:2 * ROUND_IN], n) or b"")
        limits = {first // 2, first - 300, first - 64, first - 1, first, first + 1, first + 64,
                  first + 300, second - 1, second + 1, 8191, 8192, 8193, n - 1}
        limits |= {k * 2048 + d for k in range(1, 9) for d in (-1, 0, 1)}
        for j, (fmt, s) in enumerate(wrap3(raw, plain)):
            for lim in sorted(limits):
                if 0 < lim < n and (fmt == "deflate" or lim % 3 == j % 3 or lim == n - 1):
                    out.append(Case(fmt, s, lim, f"handover/{tag}/{fmt}/{lim}", plain))
    return out


# ---- a seeded fuzz ----

FUZZ_SEED = 0x9F17


def fuzz_cases(seed=FUZZ_SEED, count=512):
    rng = random.Random(seed)
    out = []
    for it in range(count):
        n = rng.choice([0, 1, 40, 300, 3000]) if rng.randrange(4) == 0 else rng.randrange(48 << 10)
        plain = datagen.chunk(rng.randrange(8), n, seed * 31 + it)
        fmt = rng.choice(["deflate", "zlib", "gzip"])
        s = streams._zcompress(fmt, rng.choice([0, 1, 6, 9]), plain)
        lim = rng.randrange(n + 9)
        damaged = it % 4 == 3
        if damaged:
            b = bytearray(s)
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            s = bytes(b)
        out.append(Case(fmt, s, lim, f"fuzz{it}/{fmt}/{'damaged' if damaged else 'ok'}",
                        None if damaged else plain))
    return out
