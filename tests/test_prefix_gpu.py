"""The prefix decompress (libdeflate_amd_decompress_prefix_batch, _dict, the
host call, libdeflate_amd_gzip_members_peek_batch) against the reference and
the known plaintext: results, actual_out and the bytes must be EQUAL, and the
64 bytes behind every limit must stay as they were.  What a call must answer
is in tests/prefix_expect.py; it comes from the reference (the `ref` fixture)
with out_avail = the limit, and from the plaintext, never from the library's
own decode."""
import collections
import os
import subprocess
import sys

import pytest

from tests import gzip_members_files as G, prefix_expect as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
CANARY64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def run_prefix(dec, fmt, cases, dictionary=None, gap=E.GUARD, want_ain=True):
    """the cases (one format) as ONE device batch -> [(result, actual_in,
    actual_out, the limit's bytes, the bytes behind the limit)].  Rows of the
    same stream share its input; row i's output starts `gap` bytes behind row
    i - 1's limit (gap 0: back to back)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(cases)
    at, blob, in_off = {}, bytearray(), []
    for c in cases:
        if c.s not in at:
            at[c.s] = len(blob)
            blob += c.s
            blob += bytes(-len(blob) % 16)
        in_off.append(at[c.s])
    data = torch.frombuffer(blob + bytearray(64), dtype=torch.uint8).to(dev)
    out_off, pos = [], 0
    for c in cases:
        out_off.append(pos)
        pos += c.limit + gap
    out = torch.full((pos + E.GUARD,), FILL, dtype=torch.uint8, device=dev)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)    # noqa: E731
    res = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ain = torch.full((n,), CANARY64, dtype=torch.int64, device=dev)
    aout = torch.full((n,), CANARY64, dtype=torch.int64, device=dev)
    args = (data, t(in_off), t([len(c.s) for c in cases]), out, t(out_off),
            t([c.limit for c in cases]), res, aout)
    kw = dict(actual_in=ain if want_ain else None, stream=torch.cuda.current_stream())
    if dictionary is None:
        dec.decompress_prefix_batch(fmt, *args, **kw)
    else:
        dd = torch.frombuffer(bytearray(dictionary) + bytearray(16), dtype=torch.uint8).to(dev)
        dec.decompress_prefix_batch_dict(fmt, dd[:len(dictionary)], *args, **kw)
    torch.cuda.synchronize()
    if not want_ain:
        assert ain.cpu().tolist() == [CANARY64] * n, "a NULL actual_in was written"
    ob = out.cpu().numpy().tobytes()
    return [(r, i, o, ob[off:off + c.limit], ob[off + c.limit:off + c.limit + gap])
            for r, i, o, off, c in zip(res.cpu().tolist(), ain.cpu().tolist(), aout.cpu().tolist(),
                                       out_off, cases)]


def problems(cases, got, gap=E.GUARD, want_ain=True):
    """-> (mismatches, skipped): every row against its expectation; actual_in
    only where the call was given the array (run_prefix() checks that a NULL
    one stays unwritten)"""
    bad, skipped = [], 0
    for c, (r, ain, aout, data, guard) in zip(cases, got):
        why = None
        if guard != bytes([FILL]) * gap:
            why = "bytes behind the limit were written"
        elif c.want is None:
            skipped += 1        # a damaged stream cut where nothing says what is right
            if r not in (E.PREFIX, E.BAD_DATA):
                why = "neither PREFIX nor BAD_DATA"
        elif r != c.want:
            why = "result"
        elif r in (E.SUCCESS, E.PREFIX):
            if aout != c.aout:
                why = "actual_out"
            elif c.data is not None and data[:aout] != c.data:
                why = "bytes"
            elif want_ain and r == E.PREFIX and ain != 0:
                why = "actual_in of a cut stream"
            elif want_ain and r == E.SUCCESS and c.ain is not None and ain != c.ain:
                why = "actual_in"
        elif c.by_hand and aout != c.aout:
            why = "actual_out of a by-hand case"
        if why:
            bad.append((c.tag, why, (r, ain, aout), (c.want, c.aout)))
    return bad, skipped


def run_and_check(dec, cases, dictionary=None, max_skipped=0, **kw):
    fmts = collections.Counter()
    skipped = 0
    for fmt in ("deflate", "zlib", "gzip"):
        grp = [c for c in cases if c.fmt == fmt]
        if not grp:
            continue
        fmts[fmt] = len(grp)
        bad, sk = problems(grp, run_prefix(dec, fmt, grp, dictionary, **kw),
                           want_ain=kw.get("want_ain", True))
        assert not bad, (len(bad), bad[:8])
        skipped += sk
    assert skipped <= max_skipped, skipped
    return fmts, skipped


def test_each_cut_site_at_its_smallest_shape(dec, ref):
    """a limit inside a literal run, on every byte of a match of length 3 and
    of length 258, inside matches with dist == 1, dist < length and dist ==
    32768, and in a stored block at its first, middle and last byte - in raw
    DEFLATE, zlib and gzip; a stored block whose LEN runs past the input is
    BAD_DATA, not PREFIX"""
    cases = [E.expect(ref, c) for c in E.site_cases() + E.stored_past_input_cases()]
    assert all(c.want == E.PREFIX for c in cases if "storedpast" not in c.tag)
    fmts, _ = run_and_check(dec, cases)
    assert len(fmts) == 3


def test_matches_that_begin_in_the_dictionary(dec, ref):
    dictionary, cases = E.dict_cases()
    cases = [E.expect(ref, c) for c in cases]
    kinds = collections.Counter((c.fmt, c.want) for c in cases)
    assert all(kinds[(f, w)] >= 4 for f in ("deflate", "zlib") for w in (E.SUCCESS, E.PREFIX))
    run_and_check(dec, cases, dictionary)
    # without its dictionary the first match of every stream dangles
    raw = [E.Case(c.fmt, c.s, c.limit, c.tag, want=E.BAD_DATA, aout=0) for c in cases
           if c.fmt == "deflate" and "/first/" in c.tag and c.limit]
    run_and_check(dec, raw)


def test_edges(dec, ref):
    """limit 0 on a non-empty and on an empty stream; limit == size: SUCCESS
    with the footer checked, BAD_DATA with a wrong checksum; size - 1: PREFIX
    even with a wrong checksum; size + 1: SUCCESS with actual_out = size; a
    limit exactly at a block boundary in front of an empty non-final block and
    data (PREFIX) or of a broken header (BAD_DATA, as the reference)"""
    cases = [E.expect(ref, c) for c in E.edge_cases()]
    by = {c.tag: c for c in cases}
    for fmt in ("zlib", "gzip"):
        assert by[f"edge/{fmt}/sum"].want == E.BAD_DATA
        assert by[f"edge/{fmt}/sum-1"].want == E.PREFIX
        assert by[f"edge/{fmt}/5001"].want == E.SUCCESS and by[f"edge/{fmt}/5001"].aout == 5000
        assert by[f"edge/{fmt}/0"].want == E.PREFIX and by[f"edge/{fmt}/empty0"].want == E.SUCCESS
    assert by["boundary/deflate/10"].want == E.PREFIX
    assert by["boundary/broken/10"].want == E.BAD_DATA and by["boundary/broken/9"].want == E.PREFIX
    run_and_check(dec, cases)
    run_and_check(dec, cases, want_ain=False)


def test_the_cut_match_with_a_bad_offset(dec, ref):
    """THE ONLY PLACE WITHOUT A REFERENCE VERDICT.  The reference stops at a
    match without room before it reads the offset (INSUFFICIENT_SPACE for all
    of these, tests/test_prefix_abi.py checks that); this call decodes the
    offset by the rules of a match that fits.  A distance that reaches before
    the stream, the distance 1 that an empty offset code stands for at the
    stream's first byte, and an offset whose bits the input does not hold:
    BAD_DATA with actual_out = 0, by the header's rule and by hand here."""
    cases = [E.expect(ref, c) for c in E.bad_offset_cases()]
    assert sum(c.by_hand for c in cases) >= 14
    run_and_check(dec, cases)


@pytest.fixture(scope="module")
def handover(ref):
    cases = [E.expect(ref, c) for c in E.handover_cases(ref)]
    assert all(c.want == E.PREFIX for c in cases) and len(cases) > 400
    return cases


def test_hand_over_from_the_parallel_rounds(dec, handover):
    """24 to 64 KiB of text and mixed data at levels 1 / 6 / 12, static codes
    only, one codeword length; limits around the first round's output, at
    8 KiB - 1 / 8 KiB / 8 KiB + 1 and at the multiples of the 2 KiB mirror
    +- 1: the round that would cross the limit is abandoned and lane 0 walks
    to the cut"""
    fmts, _ = run_and_check(dec, handover)
    assert len(fmts) == 3


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from libdeflate_amd import api
from tests import oracle_util, prefix_expect as E, test_prefix_gpu as T
ref = oracle_util.load_ref()
assert ref is not None
dec = api.Decompressor()
cases = [E.expect(ref, c) for c in E.handover_cases(ref) + E.site_cases() + E.bad_offset_cases()
         + E.edge_cases()]
fmts, _ = T.run_and_check(dec, cases)
d, dc = E.dict_cases()
T.run_and_check(dec, [E.expect(ref, c) for c in dc], d)
print("checked", sum(fmts.values()))
"""


def test_the_same_cases_with_the_sequential_decoder_alone(ref):
    """LDA_INFLATE_PAR=0 in a fresh process: lane 0 decodes everything"""
    env = dict(os.environ, LDA_INFLATE_PAR="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "checked" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split("checked")[1]) > 1500


def test_seeded_fuzz(dec, ref):
    """512 streams of 0 to 48 KiB, random format, level and limit in [0, size
    + 8], one batch per format; a quarter damaged by one flipped byte, where
    the reference's verdict decides (INSUFFICIENT_SPACE -> PREFIX, the bytes
    zlib's inflate() gives with that avail_out).  A damaged stream that zlib
    cannot follow to the limit may be cut on a match with a bad offset: such
    cases are skipped and counted, at most 5 % of the batch."""
    cases = [E.expect(ref, c) for c in E.fuzz_cases()]
    assert len(cases) == 512
    _, skipped = run_and_check(dec, cases, max_skipped=len(cases) // 20)
    print("fuzz: skipped", skipped, "of", len(cases))


def test_neighbours_back_to_back(dec, ref):
    """cut, complete and broken streams alternate, their outputs back to back
    with no gap: every row exact, so no row wrote into the next one"""
    pool = {E.PREFIX: [], E.SUCCESS: [], E.BAD_DATA: []}
    for c in E.fuzz_cases(0x9F18, 300):
        if c.fmt != "gzip":
            continue
        if E.expect(ref, c).want in pool:
            pool[c.want].append(c)
        if c.plain and len(pool[E.BAD_DATA]) < 24:
            # broken where it shows last: everything decodes, the CRC-32 is wrong
            bad = bytearray(c.s)
            bad[-8] ^= 0x40
            pool[E.BAD_DATA].append(E.expect(ref, E.Case("gzip", bad, len(c.plain) + len(bad) % 3,
                                                         c.tag + "/sum")))
    assert all(c.want == E.BAD_DATA for c in pool[E.BAD_DATA])
    n = min(len(v) for v in pool.values())
    assert n >= 8, {k: len(v) for k, v in pool.items()}
    cases = [pool[k][i] for i in range(n) for k in (E.PREFIX, E.SUCCESS, E.BAD_DATA)]
    bad, _ = problems(cases, run_prefix(dec, "gzip", cases, gap=0), gap=0)
    assert not bad, bad[:8]


def test_host_call(dec, ref):
    """libdeflate_amd_decompress_prefix on a cut, a complete and a broken stream"""
    by = {c.tag: E.expect(ref, c) for c in E.edge_cases() + E.site_cases()}
    for tag in ("edge/gzip/4999", "edge/gzip/5001", "edge/zlib/sum", "match258/deflate/100",
                "edge/gzip/0"):
        c = by[tag]
        r, aout, data = dec.decompress_prefix(c.fmt, c.s, c.limit)
        assert r == c.want, (tag, r)
        if r in (E.SUCCESS, E.PREFIX):
            assert (aout, data) == (c.aout, c.data), tag
        else:
            assert (aout, data) == (0, b""), tag


def _peek(dec, blob, max_members, head):
    import torch
    dev = torch.device("cuda:0")
    data = torch.frombuffer(bytearray(blob) + bytearray(64), dtype=torch.uint8).to(dev)
    result = torch.zeros(5, dtype=torch.int64, device=dev)
    index = torch.full((2 * (max_members + 1),), -1, dtype=torch.int64, device=dev)
    heads = torch.full((max_members * head + E.GUARD,), FILL, dtype=torch.uint8, device=dev)
    sizes = torch.full((max_members,), CANARY64, dtype=torch.int64, device=dev)
    res = torch.full((max_members,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    # index, then the heads: one stream, nothing crosses to the host in between
    dec.index_gzip_members_batch(data, max_members, result, index, stream=st, in_nbytes=len(blob))
    dec.peek_gzip_members_batch(data, result, index, max_members, head, heads, sizes, res,
                                stream=st, in_nbytes=len(blob))
    torch.cuda.synchronize()
    return (result.cpu().tolist(), heads.cpu().numpy().tobytes(), sizes.cpu().tolist(),
            res.cpu().tolist())


@pytest.mark.parametrize("head", [256, 1, 4096])
def test_peek_gzip_members(dec, head):
    """empty members, members shorter and longer than head_nbytes and a 1 MiB
    member: row r is record[:head_nbytes], d_head_nbytes exact, the rows
    beyond the member count empty and untouched"""
    recs = [b"", G.text(100, 70), G.text(5000, 71), b"", G.text(1 << 20, 72), G.text(head, 73),
            G.text(head + 1, 74), G.text(max(head - 1, 0), 75), b"x", b""]
    f = G.File([G.piece(r, (1, 6, 9)[k % 3]) for k, r in enumerate(recs)], "peek")
    M = len(recs) + 5
    result, heads, sizes, res = _peek(dec, f.data, M, head)
    assert result[:2] == [0, len(recs)]
    for k, r in enumerate(recs):
        want = E.SUCCESS if len(r) <= head else E.PREFIX
        assert (res[k], sizes[k]) == (want, min(len(r), head)), (k, res[k], sizes[k])
        assert heads[k * head:k * head + sizes[k]] == r[:head], k
    assert res[len(recs):] == [0] * 5 and sizes[len(recs):] == [0] * 5
    assert heads[len(recs) * head:] == bytes([FILL]) * (5 * head + E.GUARD)


def test_peek_of_a_broken_chain_is_empty(dec):
    """the index call's verdict is not SUCCESS and the index not written:
    every row is empty and d_heads untouched"""
    f = G.defect_base()
    blob = dict(G.defects())["truncated"]
    M, head = f.m + 2, 64
    result, heads, sizes, res = _peek(dec, blob, M, head)
    assert result[0] != 0
    assert res == [0] * M and sizes == [0] * M
    assert heads == bytes([FILL]) * (M * head + E.GUARD)
    # ... an empty file (no member at offset 0; its data pointer may be NULL)
    result, heads, sizes, res = _peek(dec, b"", 3, head)
    assert result[0] == E.BAD_DATA and res == [0] * 3 and sizes == [0] * 3
    assert heads == bytes([FILL]) * (3 * head + E.GUARD)
    # ... and with too few rows for the file's members
    result, heads, sizes, res = _peek(dec, f.data, f.m - 1, head)
    assert result[0] == 16
    assert res == [0] * (f.m - 1) and heads == bytes([FILL]) * ((f.m - 1) * head + E.GUARD)
