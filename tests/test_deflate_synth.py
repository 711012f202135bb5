"""The hand-built corpus of tests/deflate_synth.py against three decoders on
the CPU: the oracle (the arbiter of the GPU tests), the real reference and
zlib.  The oracle and the reference must agree on every case; zlib must agree
on every case not marked ref_only and refuse every case that is."""
import zlib

import pytest

from tests import deflate_synth as S

FORMAT_WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}


@pytest.fixture(scope="module")
def corpus():
    return S.corpus()


@pytest.fixture(scope="module")
def dict_corpus():
    return S.dict_cases()


def _zlib_verdict(case):
    """(accepted, actual_in, out) of zlib on a case with its output space"""
    kw = {"zdict": case.dictionary} if case.dictionary else {}
    d = zlib.decompressobj(FORMAT_WBITS[case.fmt], **kw)
    try:
        out = d.decompress(case.data, case.avail + 1)
    except zlib.error:
        return False, 0, b""
    if not d.eof or len(out) > case.avail:
        return False, 0, b""
    return True, len(case.data) - len(d.unused_data), out


def test_composer_is_deterministic(corpus):
    again = S.corpus()
    assert [(c.name, c.data, c.out) for c in again] == [(c.name, c.data, c.out) for c in corpus]


@pytest.mark.parametrize("want", [True, False])
def test_oracle_builds_what_was_composed(corpus, oracle, want):
    for c in corpus:
        r, ain, aout, out = oracle.decompress_ex(c.fmt, c.data, c.avail, want)
        if c.valid:
            assert r == 0, (c.name, r)
            assert out == c.out, c.name
            assert not want or aout == len(c.out), c.name
        else:
            assert r != 0, c.name


@pytest.mark.parametrize("want", [True, False])
def test_oracle_agrees_with_reference(corpus, oracle, ref, want):
    for c in corpus:
        for avail in (c.avail, c.avail + 100):
            o = oracle.decompress_ex(c.fmt, c.data, avail, want)
            g = ref.decompress_ex(c.fmt, c.data, avail, want)
            assert o[0] == g[0], (c.name, avail, "oracle", o[:3], "ref", g[:3])
            if o[0] == 0:
                assert o[1:] == g[1:], (c.name, avail)
            if c.valid and avail == c.avail:
                assert g[0] == 0 and g[3] == c.out, c.name


def test_zlib_agrees_except_on_reference_only_cases(corpus):
    for c in corpus:
        ok, ain, out = _zlib_verdict(c)
        if c.ref_only:
            assert not ok, (c.name, "zlib accepted a reference-only case")
        elif c.valid:
            assert ok and out == c.out, c.name
        else:
            assert not ok, (c.name, "zlib accepted an invalid case")


def test_actual_in_matches_zlib(corpus, oracle):
    for c in corpus:
        if c.valid and not c.ref_only:
            ok, ain, out = _zlib_verdict(c)
            assert oracle.decompress_ex(c.fmt, c.data, c.avail)[1] == ain, c.name


def test_dictionary_cases(dict_corpus, oracle, ref):
    """the stored-prefix verdict of the oracle and the reference, and zlib
    with zdict, on streams that reach into a preset dictionary"""
    for c in dict_corpus:
        for want in (True, False):
            o = S.dict_verdict(oracle, c, c.avail, want)
            g = S.dict_verdict(ref, c, c.avail, want)
            assert o == g, (c.name, want, o[:3], g[:3])
            if c.valid:
                assert o[0] == 0 and o[3] == c.out, (c.name, o[:3])
                if want:
                    assert o[1] == len(c.data) and o[2] == len(c.out), c.name
            else:
                assert o[0] != 0, c.name
        ok, ain, out = _zlib_verdict(c)
        assert ok == (c.valid and not c.ref_only), c.name
        if ok:
            assert out == c.out and ain == len(c.data), c.name


def test_gzip_members(corpus, ref):
    for m in S.gzip_members(corpus):
        pos, out = 0, b""
        while pos < len(m.data):
            r, ain, aout, o = ref.decompress_ex("gzip", m.data[pos:], m.avail - len(out))
            assert r == 0, m.name
            pos += ain
            out += o
        assert out == m.out, m.name


def test_every_tag_was_reached(corpus, dict_corpus):
    seen = S.tally(corpus, dict_corpus + S.gzip_members(corpus))
    print("\nsynthetic corpus:", len(corpus), "cases,",
          sum(c.ref_only for c in corpus), "reference-only")
    print(" ".join(f"{t}={seen.get(t, 0)}" for t in S.TAGS))
    missing = [t for t in S.TAGS if t not in seen]
    assert not missing, missing
    ref_only = {t for c in corpus if c.ref_only for t in c.tags}
    for t in ("lit:sym286", "lit:sym287", "off:sym30", "off:sym31", "hlit:288",
              "hdist:32", "single-cw-bit1", "empty-off-match"):
        assert t in ref_only, t
