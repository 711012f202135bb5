"""The hand-built corpus of tests/deflate_synth.py through every decode path:
device batches in both mappings (with canaries around every output slot), the
single-buffer many-wave path, preset dictionaries and multi-member gzip.  The
oracle is the arbiter (tests/test_deflate_synth.py holds it to the real
reference on the same corpus)."""
import random

import numpy as np
import pytest

from libdeflate_amd import binding

from tests import deflate_synth as S

pytestmark = pytest.mark.gpu

CANARY = 13
# share of the ordinary streams of 64 KiB or more (trimmed headers, complete
# codes) that the parallel single-buffer path must answer itself: it answered
# 30 of 30 at both chunk sizes on an MI355X when the corpus was written
PAR_SHARE_MIN = 0.9


@pytest.fixture(scope="module")
def corpus():
    return S.corpus()


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def _set(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    binding.reload_env()


def _device_batch(dec, fmt, datas, avails, want, dictionary=None):
    """one device batch; output slots back to back at odd offsets with CANARY
    random bytes after each, the whole buffer pre-filled with random bytes.
    -> [(result, actual_in, actual_out, bytes)] and whether every byte
    outside the slots came back unchanged (the offending position if not)"""
    import torch
    dev = torch.device("cuda:0")
    offs, blob = [], bytearray()
    for d in datas:
        offs.append(len(blob))
        blob += d
        blob += bytes(-len(blob) % 16)
    data = torch.frombuffer(bytearray(blob) + bytearray(64), dtype=torch.uint8).to(dev)
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_n = torch.tensor([len(d) for d in datas], dtype=torch.int64, device=dev)
    ooffs, pos = [], 1
    for a in avails:
        ooffs.append(pos)
        pos += a + CANARY
    fill = np.frombuffer(random.Random(len(datas)).randbytes(pos + 64), dtype=np.uint8)
    out = torch.from_numpy(fill.copy()).to(dev)
    n = len(datas)
    res = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ain = torch.zeros(n, dtype=torch.int64, device=dev)
    aout = torch.zeros(n, dtype=torch.int64, device=dev) if want else None
    args = (data, in_off, in_n, out, torch.tensor(ooffs, dtype=torch.int64, device=dev),
            torch.tensor(avails, dtype=torch.int64, device=dev), res, ain, aout)
    if dictionary is None:
        dec.decompress_batch(fmt, *args)
    else:
        dt = torch.frombuffer(bytearray(dictionary) + bytearray(1),
                              dtype=torch.uint8)[:len(dictionary)].to(dev)
        dec.decompress_batch_dict(fmt, dt, *args)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    res, ain = res.cpu().tolist(), ain.cpu().tolist()
    aout = aout.cpu().tolist() if want else list(avails)
    got = [(r, i, o if want else 0, host[s:s + o].tobytes() if r == 0 else b"")
           for r, i, o, s in zip(res, ain, aout, ooffs)]
    keep = np.ones(len(host), dtype=bool)
    for s, a in zip(ooffs, avails):
        keep[s:s + a] = False
    bad = np.nonzero((host != fill) & keep)[0]
    return got, (int(bad[0]) if len(bad) else None)


def _compare(tag, got, exp, want):
    assert got[0] == exp[0], (tag, "gpu", got[:3], "oracle", exp[:3])
    if exp[0] == 0:
        assert got[1] == exp[1], (tag, "actual_in", got[1], exp[1])
        if want:
            assert got[2] == exp[2], (tag, "actual_out", got[2], exp[2])
        assert got[3] == exp[3], (tag, "bytes differ")


def _batches(dec, oracle, cases, delta, want, dictionary=None):
    groups = {}
    for c in cases:
        groups.setdefault(c.fmt, []).append(c)
    for fmt, grp in groups.items():
        avails = [max(c.avail + delta, 0) for c in grp]
        got, spill = _device_batch(dec, fmt, [c.data for c in grp], avails, want, dictionary)
        assert spill is None, (fmt, delta, want, "byte outside every slot changed at", spill)
        for c, a, g in zip(grp, avails, got):
            if dictionary is None:
                exp = oracle.decompress_ex(fmt, c.data, a, want)
            else:
                exp = S.dict_verdict(oracle, c, a, want)
            _compare((c.name, delta, want), g, exp, want)
            if c.valid and a == c.avail:
                assert g[3] == c.out, c.name


@pytest.mark.parametrize("mode", ["1", "0"])
def test_device_batch_both_mappings(dec, oracle, corpus, monkeypatch, mode):
    """wave mapping (1, the default) and lane mapping (0): exact, one byte
    short and 100 bytes spare output space, with and without actual_out"""
    _set(monkeypatch, LDA_INFLATE_PAR=mode)
    for want in (True, False):
        for delta in (0, -1, 100):
            _batches(dec, oracle, corpus, delta, want)


@pytest.mark.parametrize("mode", ["1", "0"])
def test_canaries_around_failing_streams(dec, oracle, corpus, monkeypatch, mode):
    """short-output and bad-data streams between valid ones, slots back to
    back: the valid neighbours come back exact and nothing outside
    [off, off + out_avail) changes"""
    _set(monkeypatch, LDA_INFLATE_PAR=mode)
    good = [c for c in corpus if c.valid and c.fmt == "deflate" and len(c.out) < 70000]
    bad = [c for c in corpus if not c.valid and c.fmt == "deflate"]
    short = [S.Case(c.name + "-short", c.fmt, c.data, None, c.tags, avail=max(len(c.out) - 1, 0))
             for c in good[::3] if len(c.out)]
    mixed = []
    for i, g in enumerate(good):
        mixed.append(g)
        pool = bad if i % 2 else short
        mixed.append(pool[i // 2 % len(pool)])
    for want in (True, False):
        _batches(dec, oracle, mixed, 0, want)


@pytest.mark.parametrize("chunk", [4096, 32768])
def test_single_buffer_many_wave_path(dec, oracle, corpus, monkeypatch, chunk):
    """every case of 64 KiB or more through the single-buffer path forced on;
    the streams the block finder cannot enter (untrimmed headers, incomplete
    litlen codes, no EOB) are checked on their bytes only"""
    _set(monkeypatch, LDA_STREAM_PAR_MIN=0, LDA_STREAM_CHUNK=chunk)
    big = [c for c in corpus if c.avail >= 65536]
    assert len(big) >= 20
    npar = nord = 0
    for c in big:
        for want in (True, False):
            got = dec.decompress_ex(c.fmt, c.data, c.avail, want)
            par = binding.stream_stats()["parallel"]
            exp = oracle.decompress_ex(c.fmt, c.data, c.avail, want)
            _compare((c.name, chunk, want, binding.stream_stats()), got, exp, want)
            if c.ordinary and want:
                nord += 1
                npar += par
    print(f"\nchunk {chunk}: parallel path answered {npar} of {nord} ordinary streams")
    assert nord >= 10 and npar >= PAR_SHARE_MIN * nord, (npar, nord)


@pytest.mark.parametrize("mode", ["1", "0"])
def test_dictionaries(dec, oracle, monkeypatch, mode):
    """decompress_batch_dict in both mappings and decompress_dict_ex against
    the stored-prefix verdict"""
    _set(monkeypatch, LDA_INFLATE_PAR=mode)
    cases = S.dict_cases()
    by_dict = {}
    for c in cases:
        by_dict.setdefault(c.dictionary, []).append(c)
    for d, grp in by_dict.items():
        for want in (True, False):
            for delta in (0, -1, 100):
                _batches(dec, oracle, grp, delta, want, dictionary=d)
    for c in cases:
        for want in (True, False):
            got = dec.decompress_dict_ex(c.fmt, c.dictionary, c.data, c.avail, want)
            _compare((c.name, want), got, S.dict_verdict(oracle, c, c.avail, want), want)


def test_multi_member_gzip(dec, corpus, ref):
    """the reference decoding member after member is the expectation"""
    def ref_loop(buf, avail):
        pos, out = 0, b""
        while pos < len(buf):
            r, ain, aout, o = ref.decompress_ex("gzip", buf[pos:], avail - len(out))
            if r != 0:
                return r, out
            pos += ain
            out += o
        return 0, out
    for m in S.gzip_members(corpus):
        k = int(m.name[len("members"):])
        assert ref_loop(m.data, m.avail) == (0, m.out)
        r, ain, aout, nm, out = dec.gzip_decompress_members(m.data, m.avail + 10)
        assert (r, ain, aout, nm) == (0, len(m.data), len(m.out), k) and out == m.out, m.name
        assert dec.gzip_decompress_members(m.data, m.avail - 1)[0] == \
            ref_loop(m.data, m.avail - 1)[0] == 3, m.name
        cut = m.data[:-5]
        assert dec.gzip_decompress_members(cut, m.avail)[0] == ref_loop(cut, m.avail)[0], m.name
