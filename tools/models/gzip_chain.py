"""CPU model of the finder of concatenated gzip members of
gzip_members_kernels.hip (design aid and test subject, not product code):
file bytes -> the five result words, the index and the bytes, by the steps the
kernels take, with the same bounds and the precedence include/libdeflate_amd.h
states.

  candidates   every offset p with 1f 8b 08, FLG & 0xE0 == 0 and p + 18 <= n,
               in file order; more than max_members + SLACK of them is the
               verdict MORE_CANDIDATES;
  count        per candidate (verdict, actual_in, size) with the rest of the
               file as its input, as the count mode of the decoder answers:
               the header by libdeflate's rules (FEXTRA, FNAME, FCOMMENT,
               FHCRC skipped, not verified) and the reader's own limit of
               NAME_MAX bytes of FNAME + FCOMMENT, the DEFLATE stream by
               zlib.decompressobj(wbits=-15) and its unused_data, the footer
               present and its ISIZE the counted size modulo 2^32.  The CRC-32
               is NOT part of the count - nobody produced the bytes - which is
               why this is not zlib's wbits=31: that one stops at a wrong
               CRC-32 and verifies FHCRC, and the decoder does neither here;
  successor    the candidate at p + actual_in (END when that is n, NONE when
               no candidate stands there or the count failed), and the chain
               from candidate 0 through blocks of BLOCK candidates, which is
               bgzf_chain.parallel() on (p, actual_in) pairs;
  break        where a broken chain stopped: the verdict of the candidate
               there, BAD_DATA when none stands there;
  verdict      MORE_CANDIDATES, broken chain, MORE_MEMBERS, INSUFFICIENT_SPACE
               - and then nothing is decoded -, else the first member in file
               order whose CRC-32 is wrong (BAD_DATA), else SUCCESS.

read(data, max_members, out_avail=None, decode=True) -> Result(words, rows,
plain): rows is None where the index is not written, plain is None where
nothing is decoded (a member whose CRC-32 is wrong still leaves its bytes).

  python tools/models/gzip_chain.py FILE [max_members]
"""
import collections
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tools.models import bgzf_chain  # noqa: E402

SUCCESS, BAD_DATA, INSUFFICIENT_SPACE = 0, 1, 3
MORE_MEMBERS, MORE_CANDIDATES, SLACK = 16, 17, 1024
BLOCK = bgzf_chain.BLOCK
SIZE_LIMIT = 0xFFFFFFFF     # LIBDEFLATE_AMD_SIZE_LIMIT_MAX
MIN_MEMBER = 18
NAME_MAX = 65536            # LIBDEFLATE_AMD_GZM_NAME_MAX

Result = collections.namedtuple("Result", "words rows plain")


def candidates(data):
    n, out, p = len(data), [], data.find(b"\x1f\x8b\x08")
    while p >= 0 and p + MIN_MEMBER <= n:
        if not data[p + 3] & 0xE0:
            out.append(p)
        p = data.find(b"\x1f\x8b\x08", p + 1)
    return out


def header_len(data, p):
    """bytes of gzip header at p with [p, n) as the input, or 0: lib/gzip_decompress.c"""
    end = len(data)
    if end - p < MIN_MEMBER or data[p:p + 3] != b"\x1f\x8b\x08" or data[p + 3] & 0xE0:
        return 0
    flg, q = data[p + 3], p + 10
    if flg & 4:
        xlen = data[q] | data[q + 1] << 8
        q += 2
        if end - q < xlen + 8:
            return 0
        q += xlen
    budget = NAME_MAX            # FNAME + FCOMMENT, terminators included
    for bit in (8, 16):
        if flg & bit:
            z = data.find(b"\0", q, min(end, q + budget))
            if z < 0 and end - q > budget:
                return 0
            used = (end if z < 0 else z + 1) - q
            q, budget = q + used, budget - used
            if end - q < 8:
                return 0
    if flg & 2:
        q += 2
        if end - q < 8:
            return 0
    return q - p


def count(data, p, payload=False):
    """(verdict, actual_in, size) of the member that starts at p; with
    payload=True also its bytes and whether its CRC-32 is right"""
    fail = (BAD_DATA, 0, 0) + ((b"", False) if payload else ())
    hdr = header_len(data, p)
    if not hdr:
        return fail
    d = zlib.decompressobj(wbits=-15)
    try:
        out = d.decompress(data[p + hdr:])
    except zlib.error:
        return fail
    if not d.eof or len(d.unused_data) < 8:
        return fail
    foot = len(data) - len(d.unused_data)
    if len(out) > SIZE_LIMIT:
        return (INSUFFICIENT_SPACE,) + fail[1:]
    if int.from_bytes(data[foot + 4:foot + 8], "little") != len(out) & 0xFFFFFFFF:
        return fail
    ain = foot + 8 - p
    if ain > 0xFFFFFFFF:        # the chain's sizes are 32 bits
        return (INSUFFICIENT_SPACE,) + fail[1:]
    if payload:
        good = int.from_bytes(data[foot:foot + 4], "little") == zlib.crc32(out)
        return SUCCESS, ain, len(out), out, good
    return SUCCESS, ain, len(out)


def _break_verdict(cands, counts, n):
    """the chain from offset 0 hop by hop to where it stops"""
    at = {p: i for i, p in enumerate(cands)}
    q = 0
    for _ in range(len(cands) + 1):     # a bound that does not come from the file
        i = at.get(q)
        if i is None:
            return BAD_DATA
        if counts[i][0] != SUCCESS:
            return counts[i][0]
        q += counts[i][1]
        assert q < n, "not a broken chain"
    raise AssertionError("a successor stands behind its candidate")


def read(data, max_members, out_avail=None, decode=True, block=BLOCK):
    data = bytes(data)
    n = len(data)
    if out_avail is None or not decode:
        out_avail = 1 << 64
    if n == 0:
        return Result([BAD_DATA, 0, 0, 0, 0], None, None)
    cands = candidates(data)
    K, cap = len(cands), min(max_members + SLACK, n // 3 + 1)
    if K > cap:
        return Result([MORE_CANDIDATES, K, 0, 0, 0], None, None)
    counts = [count(data, p) for p in cands]
    pairs = [(p, c[1] if c[0] == SUCCESS else 0) for p, c in zip(cands, counts)]
    ok, m, members = bgzf_chain.parallel(data, max_members, pairs, block)
    if not ok:
        return Result([_break_verdict(cands, counts, n), 0, 0, 0, 0], None, None)
    if m > max_members:
        return Result([MORE_MEMBERS, m, 0, 0, 0], None, None)
    size = {p: c[2] for p, c in zip(cands, counts)}
    rows, u = [], 0
    for p, _ in members:
        rows.append((p, u))
        u += size[p]
    rows.append((n, u))
    if u > out_avail:
        return Result([INSUFFICIENT_SPACE, m, n, u, 0], rows, None)
    if not decode:
        return Result([SUCCESS, m, n, u, 0], rows, None)
    verdict, plain = SUCCESS, bytearray()
    for p, _ in members:
        _, _, _, out, good = count(data, p, payload=True)
        plain += out
        if not good and verdict == SUCCESS:
            verdict = BAD_DATA
    return Result([verdict, m, n, u, 0], rows, bytes(plain))


if __name__ == "__main__":
    blob = open(sys.argv[1], "rb").read()
    mm = int(sys.argv[2]) if len(sys.argv) > 2 else len(blob) // MIN_MEMBER + 1
    r = read(blob, mm)
    print(f"words={r.words} candidates={len(candidates(blob))}")
