"""The size query (libdeflate_amd_decompress_sizes_batch, _dict, _host) and
the packed decompress on top of it (libdeflate_amd_decompress_batch_packed)
against the reference: verdicts, sizes and actual_in are integers and must be
EQUAL.  What a size query must answer is in tests/sizes_expect.py; it comes
from the reference (the `ref` fixture), never from the library's own decode."""
import collections
import os
import struct
import zlib

import pytest

from libdeflate_amd import binding
from tests import datagen, deflate_synth, sizes_expect as E, streams

pytestmark = pytest.mark.gpu

PAD = 16                        # canary entries in front of and behind a result array
CANARY32 = 0x5A5A5A5A
CANARY64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def _pack(chunks, dev):
    import torch
    offs, blob = [], bytearray()
    for c in chunks:
        offs.append(len(blob))
        blob += c
        blob += bytes(-len(blob) % 16)
    data = torch.frombuffer(blob + bytearray(64), dtype=torch.uint8).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_n = torch.tensor([len(c) for c in chunks], dtype=torch.int64, device=dev)
    return data, in_off, in_n


def _guarded(n, dtype, canary, dev):
    """(the whole tensor, its n entries in the middle)"""
    import torch
    full = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=dev)
    return full, full[PAD:PAD + n]


def _canaries_intact(full, n, canary):
    v = full.cpu().tolist()
    return v[:PAD] == [canary] * PAD and v[PAD + n:] == [canary] * PAD


def device_sizes(dec, fmt, chunks, limits=None, dictionary=None, want_ain=True):
    """the chunks as one device batch -> [(result, actual_in, size)]; limits:
    None (a NULL d_out_limit) or a list whose None entries are LIMIT_MAX.
    Canaries around the three result arrays are checked on every call."""
    import torch
    dev = torch.device("cuda:0")
    n = len(chunks)
    data, in_off, in_n = _pack(chunks, dev)
    lim = None
    if limits is not None:
        lim = torch.tensor([E.LIMIT_MAX if x is None else x for x in limits],
                           dtype=torch.int64, device=dev)
    res_f, res = _guarded(n, torch.int32, CANARY32, dev)
    ain_f, ain = _guarded(n, torch.int64, CANARY64, dev)
    size_f, size = _guarded(n, torch.int64, CANARY64, dev)
    if dictionary is None:
        dec.decompress_sizes_batch(fmt, data, in_off, in_n, res, size, limits=lim,
                                   actual_in=ain if want_ain else None,
                                   stream=torch.cuda.current_stream())
    else:
        dd = torch.frombuffer(bytearray(dictionary) + bytearray(16), dtype=torch.uint8).to(dev)
        dec.decompress_sizes_batch_dict(fmt, dd[:len(dictionary)], data, in_off, in_n, res,
                                        size, limits=lim, actual_in=ain if want_ain else None,
                                        stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert _canaries_intact(res_f, n, CANARY32), "results[] canary"
    assert _canaries_intact(ain_f, n, CANARY64), "actual_in[] canary"
    assert _canaries_intact(size_f, n, CANARY64), "out_nbytes[] canary"
    if not want_ain:
        assert ain.cpu().tolist() == [CANARY64] * n, "a NULL actual_in was written"
    return list(zip(res.cpu().tolist(), ain.cpu().tolist(), size.cpu().tolist()))


def run_cases(dec, cases, **kw):
    """cases (fmt, stream, limit, tag) -> results in the cases' order, one
    device batch per format"""
    got = [None] * len(cases)
    for fmt in ("deflate", "zlib", "gzip"):
        idx = [i for i, c in enumerate(cases) if c[0] == fmt]
        if not idx:
            continue
        r = device_sizes(dec, fmt, [cases[i][1] for i in idx], [cases[i][2] for i in idx], **kw)
        for i, g in zip(idx, r):
            got[i] = g
    return got


def check(cases, got, want):
    bad = [(c[3], c[0], c[2], g, w) for c, g, w in zip(cases, got, want) if tuple(g) != tuple(w[:3])]
    assert not bad, (len(bad), bad[:8])


@pytest.fixture(scope="module")
def corpus(ref):
    """the verdict corpus with the reference's expectations; every class of
    expectation must be there (a corpus that lost one would hide a failure)"""
    cases = E.verdict_corpus()
    want = [E.expect(ref, f, s, lim) for f, s, lim, _ in cases]
    classes = collections.Counter(w[3] for w in want)
    print("verdict corpus:", len(cases), "cases", dict(classes))
    for k in ("success", "bad", "space", "checksum"):
        assert classes[k] >= 10, classes
    return cases, want


def test_valid_streams_no_limit_exact_limit_one_short(dec, ref):
    """every format, producer, level and size: a NULL d_out_limit and a limit
    equal to the size give SUCCESS with the reference's actual_in / actual_out,
    the size minus 1 gives INSUFFICIENT_SPACE"""
    vs = E.valid_streams(ref)
    assert len({v[0] for v in vs}) == 3
    for fmt in ("deflate", "zlib", "gzip"):
        grp = [v for v in vs if v[0] == fmt]
        chunks = [v[1] for v in grp]
        want = []
        for _, s, d, tag in grp:
            r = ref.decompress_ex(fmt, s, len(d))
            assert r[0] == 0 and r[3] == d, tag
            want.append((0, r[1], r[2]))
        got = device_sizes(dec, fmt, chunks)                       # NULL limits
        assert got == want, [(g, w, v[3]) for g, w, v in zip(got, want, grp) if g != w][:8]
        got = device_sizes(dec, fmt, chunks, [len(v[2]) for v in grp], want_ain=False)
        assert [(g[0], g[2]) for g in got] == [(0, w[2]) for w in want]
        short = [v for v in grp if len(v[2])]
        exp = [E.expect(ref, fmt, v[1], len(v[2]) - 1)[:3] for v in short]
        assert all(e == (3, 0, 0) for e in exp)
        got = device_sizes(dec, fmt, [v[1] for v in short], [len(v[2]) - 1 for v in short])
        assert got == exp, [(g, v[3]) for g, v in zip(got, short) if g != (3, 0, 0)][:8]


def test_batch_larger_than_the_grid(dec, ref):
    """5200 streams of mixed size and kind, a few of them damaged: the streams
    beyond the first grid-full are handed out as waves become free"""
    distinct = []
    for i in range(130):
        n = (0, 1, 31, 300, 4096, 20000, 65536, 70000)[i % 8] + 3 * i
        d = datagen.chunk(i // 8, n, 0x0E115200 + i)
        s = ref.compress("gzip", (1, 6, 9, 12, 0)[i % 5], d)
        if i % 13 == 5:
            s = s[:len(s) // 2]
        if i % 17 == 3:
            s = s[:-3] + bytes([s[-3] ^ 1]) + s[-2:]       # ISIZE
        distinct.append(s)
    want1 = [E.expect(ref, "gzip", s, None)[:3] for s in distinct]
    assert len({w[0] for w in want1}) >= 2
    n = 5200
    got = device_sizes(dec, "gzip", [distinct[(7 * i) % 130] for i in range(n)])
    want = [want1[(7 * i) % 130] for i in range(n)]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]


def test_verdicts_against_the_reference(dec, corpus):
    cases, want = corpus
    check(cases, run_cases(dec, cases), want)


@pytest.mark.parametrize("switch", ["LDA_INFLATE_PAR=0", "LDA_INFLATE_WAVES_PER_CU=4",
                                    "LDA_SIZES_WAVES_PER_CU=4"])
def test_answers_do_not_depend_on_the_tuning_switches(dec, corpus, monkeypatch, switch):
    cases, want = corpus
    base = run_cases(dec, cases)
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    binding.reload_env()
    try:
        got = run_cases(dec, cases)
    finally:
        monkeypatch.delenv(name)
        binding.reload_env()
    assert got == base
    check(cases, got, want)


def test_a_failing_stream_between_two_good_ones(dec, ref):
    """... leaves theirs right, whatever way it fails; and nothing is written
    outside the three result arrays (device_sizes checks the canaries)"""
    d = datagen.text_chunk(65536, 77)
    good = ref.compress("zlib", 6, d)
    fails = [good[:len(good) // 2], good[:5], b"", bytes([good[0], good[1] ^ 1]) + good[2:],
             good[:40] + bytes([good[40] ^ 0x10]) + good[41:], bytes(3000)]
    chunks, limits = [], []
    for f in fails:
        chunks += [good, f, good]
        limits += [None, None, len(d)]
    chunks += [good, good, good]
    limits += [len(d), len(d) - 1, None]
    got = device_sizes(dec, "zlib", chunks, limits)
    want = [E.expect(ref, "zlib", s, lim)[:3] for s, lim in zip(chunks, limits)]
    assert got == want
    ok = (0, len(good), len(d))
    assert got[0::3] == [ok] * 7 and got[2::3][:6] == [ok] * 6 and got[-2] == (3, 0, 0)
    # (the stream with one flipped bit may decode: the reference decides, above)
    assert all(got[1 + 3 * k][0] != 0 for k in (0, 1, 2, 3, 5))


def test_dictionary(dec, ref):
    """a raw stream whose first match reaches into the dictionary: SUCCESS
    with the reference's size through _dict, BAD_DATA through the plain call;
    zlib with FDICT: the right DICTID, a wrong one, and no dictionary given"""
    zdict = datagen.text_chunk(20000, 5)
    body = zdict[7000:7400] + datagen.text_chunk(30000, 6) + zdict[100:900]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=zdict)
    raw = co.compress(body) + co.flush()
    pre, npre = deflate_synth.stored_prefix(zdict)
    r = ref.decompress_ex("deflate", pre + raw, npre + len(body))
    assert r[0] == 0 and r[3][npre:] == body
    want = (0, r[1] - len(pre), r[2] - npre)
    assert ref.decompress_ex("deflate", raw, len(body))[0] == 1
    assert device_sizes(dec, "deflate", [raw, raw], [None, len(body)], dictionary=zdict) == [want, want]
    assert ref.decompress_ex("deflate", pre + raw, npre + len(body) - 1)[0] == 3
    assert device_sizes(dec, "deflate", [raw], [len(body) - 1], dictionary=zdict) == [(3, 0, 0)]
    assert device_sizes(dec, "deflate", [raw]) == [(1, 0, 0)]
    # a dictionary too short for the first match's distance
    pre5, n5 = deflate_synth.stored_prefix(zdict[-5000:])
    assert ref.decompress_ex("deflate", pre5 + raw, n5 + len(body))[0] == 1
    assert device_sizes(dec, "deflate", [raw], dictionary=zdict[-5000:]) == [(1, 0, 0)]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=zdict)
    z = co.compress(body) + co.flush()
    assert z[1] & 0x20 and ref.decompress_ex("zlib", z, len(body))[0] == 1      # FDICT: refused
    zc = deflate_synth.Case("fdict", "zlib", z, body, (), dictionary=zdict)
    wantz = deflate_synth.dict_verdict(ref, zc, len(body))[:3]
    assert wantz == (0, len(z), len(body))
    assert device_sizes(dec, "zlib", [z], dictionary=zdict) == [wantz]
    assert device_sizes(dec, "zlib", [z], dictionary=zdict[:-1] + b"#") == [(1, 0, 0)]
    assert device_sizes(dec, "zlib", [z]) == [(1, 0, 0)]
    # a stream without FDICT decodes as if no dictionary were given
    plain = zlib.compress(body, 6)
    wantp = ref.decompress_ex("zlib", plain, len(body))[:3]
    assert wantp[0] == 0
    assert device_sizes(dec, "zlib", [plain], dictionary=zdict) == [wantp]
    # the hand-built dictionary streams, against the reference behind a stored
    # block that holds the dictionary; a wrong footer is the checksum-only case
    cases = deflate_synth.dict_cases()
    good = {c.name: c for c in cases if c.valid}
    for c in cases:
        w = deflate_synth.dict_verdict(ref, c, c.avail)[:3]
        if c.name == "bad:footer":
            g = good["dict1000/zlib"]
            w = (0, len(g.data), len(g.out))
        assert device_sizes(dec, c.fmt, [c.data], [c.avail], dictionary=c.dictionary) == [w], c.name


def _packed(dec, fmt, chunks, capacity, align, actual_in=True, fill=0xA5, pre=None):
    """-> (results, actual_in, actual_out, offsets (n + 1), the output buffer's bytes)"""
    import torch
    dev = torch.device("cuda:0")
    n = len(chunks)
    data, in_off, in_n = _pack(chunks, dev)
    out = torch.full((capacity + 256,), fill, dtype=torch.uint8, device=dev)
    res_f, res = _guarded(n, torch.int32, CANARY32, dev)
    ain_f, ain = _guarded(n, torch.int64, CANARY64, dev)
    aout_f, aout = _guarded(n, torch.int64, CANARY64, dev)
    off_f, off = _guarded(n + 1, torch.int64, CANARY64, dev)
    st = torch.cuda.current_stream()
    if pre is not None:
        pre()
    dec.decompress_batch_packed(fmt, data, in_off, in_n, out, off, res, aout,
                                actual_in=ain if actual_in else None, out_align=align,
                                out_capacity=capacity, stream=st)
    busy = not st.query() if pre is not None else None
    torch.cuda.synchronize()
    assert _canaries_intact(res_f, n, CANARY32) and _canaries_intact(ain_f, n, CANARY64)
    assert _canaries_intact(aout_f, n, CANARY64) and _canaries_intact(off_f, n + 1, CANARY64)
    r = (res.cpu().tolist(), ain.cpu().tolist(), aout.cpu().tolist(), off.cpu().tolist(),
         out.cpu().numpy().tobytes())
    return r + (busy,) if pre is not None else r


def _mixed_batch(ref, fmt, n, seed):
    datas, comp = [], []
    for i in range(n):
        size = (0, 1, 31, 777, 4096, 30000, 65536, 70001)[i % 8] + i
        d = datagen.chunk(i % 8 + 3 * (i // 8), size, seed + i)
        datas.append(d)
        comp.append(ref.compress(fmt, (6, 1, 12, 0, 9)[i % 5], d))
    return datas, comp


def _slots(sizes, align):
    off, at = [], 0
    for s in sizes:
        off.append(at)
        at += (s + align - 1) // align * align
    return off + [at]


@pytest.mark.parametrize("fmt,align", [("gzip", 1), ("gzip", 16), ("zlib", 16), ("deflate", 256)])
def test_packed_mixed_batch(dec, ref, fmt, align):
    """bytes equal the reference's, offsets are exactly the aligned prefix
    sums, the last offset is the total"""
    datas, comp = _mixed_batch(ref, fmt, 300, 0x0E115300)
    want_off = _slots([len(d) for d in datas], align)
    res, ain, aout, off, out = _packed(dec, fmt, comp, want_off[-1], align)
    assert res == [0] * len(comp)
    assert off == want_off
    for i, (d, z) in enumerate(zip(datas, comp)):
        r = ref.decompress_ex(fmt, z, len(d))
        assert (ain[i], aout[i]) == (r[1], r[2]), i
        assert out[off[i]:off[i] + len(d)] == r[3] == d, i
    assert out[want_off[-1]:] == b"\xA5" * 256


def test_packed_capacity_cut_in_the_middle(dec, ref):
    """the streams in front are intact, the ones that do not fit report
    INSUFFICIENT_SPACE, nothing is written from the first unfitting offset on,
    and the last offset still names the full need"""
    datas, comp = _mixed_batch(ref, "gzip", 200, 0x0E115400)
    want_off = _slots([len(d) for d in datas], 16)
    cap = want_off[100] + len(datas[100]) - 1          # stream 100 misses by one byte
    res, ain, aout, off, out = _packed(dec, "gzip", comp, cap, 16)
    assert off == want_off
    first_bad = None
    for i, d in enumerate(datas):
        fits = want_off[i] + len(d) <= cap
        if fits:
            assert res[i] == 0 and aout[i] == len(d) and ain[i] == len(comp[i]), i
            assert out[off[i]:off[i] + len(d)] == d, i
        else:
            first_bad = i if first_bad is None else first_bad
            assert (res[i], ain[i], aout[i]) == (3, 0, 0), i
    assert first_bad == 100
    # (empty streams behind the cut still "fit": they take no bytes)
    assert out[want_off[100]:] == b"\xA5" * (len(out) - want_off[100])
    # no room at all
    res, ain, aout, off, out = _packed(dec, "gzip", comp, 0, 16)
    assert off == want_off and out == b"\xA5" * 256
    assert res == [0 if not len(d) else 3 for d in datas]


def test_packed_corrupt_streams_keep_their_verdict_and_their_neighbours(dec, ref):
    datas, comp = _mixed_batch(ref, "gzip", 120, 0x0E115500)
    comp[40] = comp[40][:len(comp[40]) // 2]                           # structural
    comp[41] = comp[41][:30] + bytes([comp[41][30] ^ 0x20]) + comp[41][31:]
    z = bytearray(comp[70])
    z[-8] ^= 1                                                         # CRC-32 only
    comp[70] = bytes(z)
    exp = [E.expect(ref, "gzip", s, None) for s in comp]
    sizes = [e[2] if e[0] == 0 else 0 for e in exp]
    assert exp[40][3] == "bad" and exp[70][3] == "checksum" and sizes[70] == len(datas[70]) > 0
    want_off = _slots(sizes, 16)
    res, ain, aout, off, out = _packed(dec, "gzip", comp, want_off[-1], 16)
    assert off == want_off
    for i, s in enumerate(comp):
        # the size query's verdict where it fails, else the decode's with
        # exactly the size as room
        r = ref.decompress_ex("gzip", s, sizes[i]) if exp[i][0] == 0 else (exp[i][0],)
        if r[0] != 0:
            assert (res[i], ain[i], aout[i]) == (r[0], 0, 0), i
        else:
            assert (res[i], ain[i], aout[i]) == (0, r[1], r[2]), i
            assert out[off[i]:off[i] + aout[i]] == r[3], i
    assert (res[40], res[70]) == (1, 1) and res[39] == res[42] == res[69] == res[71] == 0
    assert off[71] - off[70] == (len(datas[70]) + 15) // 16 * 16       # slot still reserved
    assert off[41] == off[40]                                          # a failed stream counts 0


def test_packed_only_enqueues(dec, ref):
    """the call returns while the stream is still busy with work queued in
    front of it: it does not synchronise (nor does the size query)"""
    import torch
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("no torch.cuda._sleep to keep the stream busy")
    datas, comp = _mixed_batch(ref, "gzip", 64, 0x0E115600)
    want_off = _slots([len(d) for d in datas], 16)
    _packed(dec, "gzip", comp, want_off[-1], 16)                       # buffers exist now
    r = _packed(dec, "gzip", comp, want_off[-1], 16,
                pre=lambda: torch.cuda._sleep(200_000_000))
    assert r[5] is True, "the stream had drained when the call returned"
    assert r[0] == [0] * 64 and r[3] == want_off
    for i, d in enumerate(datas):
        assert r[4][want_off[i]:want_off[i] + len(d)] == d


def test_host_form_equals_the_device_form(dec, corpus):
    cases, want = corpus
    for fmt in ("deflate", "zlib", "gzip"):
        grp = [(c, w) for c, w in zip(cases, want) if c[0] == fmt]
        got = dec.decompress_sizes_batch_host(
            fmt, [c[1] for c, _ in grp], [E.LIMIT_MAX if c[2] is None else c[2] for c, _ in grp])
        bad = [(c[3], g, w) for (c, w), g in zip(grp, got) if tuple(g) != tuple(w[:3])]
        assert not bad, bad[:8]
    # NULL limits
    ok = [(c, w) for c, w in zip(cases, want) if c[0] == "gzip" and w[3] == "success"][:50]
    got = dec.decompress_sizes_batch_host("gzip", [c[1] for c, _ in ok])
    assert got == [tuple(w[:3]) for _, w in ok] and len(ok) == 50


def test_host_form_over_several_slices(dec, ref):
    """2176 gzip streams of 64 KiB, every eighth incompressible: more than two
    slices' worth of input; one damaged stream in each half"""
    n, size, distinct = 2176, 65536, 136
    chunks = datagen.batch(distinct, size, 0x0E115700)
    comp = [streams._zcompress("gzip", 6, x) for x in chunks]
    assert sum(len(comp[i % distinct]) for i in range(n)) > (32 << 20)
    data = [comp[i % distinct] for i in range(n)]
    data[300] = data[300][:len(data[300]) // 2]
    data[n - 300] = data[n - 300][:-4] + bytes(4)                  # ISIZE
    got = dec.decompress_sizes_batch_host("gzip", data)
    for i, g in enumerate(got):
        if i in (300, n - 300):
            assert E.expect(ref, "gzip", data[i], None)[:3] == (1, 0, 0) == g, i
        else:
            assert g == (0, len(data[i]), size), (i, g)


def test_host_form_over_the_devices(dec, ref, monkeypatch):
    """LDA_DEVICES=all: one shard per visible device (2 MiB of input each, a
    shard is at least 1 MiB); and two shards that share a device"""
    import torch
    ndev = torch.cuda.device_count()
    chunks = [datagen.random_chunk(65536, 0xD5 + i) for i in range(32 * max(2, ndev))]
    comp = [streams._zcompress("zlib", 1, x) for x in chunks]
    comp[7] = comp[7][:1000]
    mib = sum(map(len, comp)) >> 20
    want = [E.expect(ref, "zlib", s, None)[:3] for s in comp]
    monkeypatch.setenv("LDA_DEVICES", "all")
    binding.reload_env()
    assert dec.decompress_sizes_batch_host("zlib", comp) == want
    assert binding.last_fanout() == min(ndev, 16, mib)
    monkeypatch.setenv("LDA_DEVICES", "2")
    monkeypatch.setenv("LDA_FANOUT_OVERSUB", "1")
    binding.reload_env()
    assert dec.decompress_sizes_batch_host("zlib", comp) == want
    assert binding.last_fanout() == 2


def test_fuzz_sizes():
    """tools/fuzz_inflate.py --sizes: the decompress fuzzer's mutations, the
    verdict by the rule of tests/sizes_expect.py; a fixed seed"""
    from tools import fuzz_inflate
    msgs = []
    n, bad = fuzz_inflate.run_sizes([9101, 9102], log=lambda *a, **k: msgs.append(a))
    assert n >= 400 and bad == 0, msgs[-5:]
