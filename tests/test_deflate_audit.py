"""CPU self-tests of the block auditor (tests/deflate_audit.py): the walker
against zlib, the real reference and oracle.block_map(), the exact
references against brute force, and one hand-built stream per invariant that
breaks exactly that invariant - a check that never fires guards nothing."""
import itertools
import random
import zlib

import pytest

from tests import datagen
from tests import deflate_audit as A
from tests.streams import BitWriter

WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}


def _zlib(fmt, level, data, zdict=None):
    co = (zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], zdict=zdict) if zdict
          else zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt]))
    return co.compress(data) + co.flush()


def _inputs():
    return [datagen.chunk(i, n, 0x0E1100D0) for i, n in
            enumerate((0, 1, 100, 5000, 65536, 70000, 40000, 65536))]


# ------------------------------------------------------------ the walker

@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_walker_reproduces_zlib_streams(fmt):
    for level in (0, 1, 6, 9):
        for d in _inputs():
            out, blocks = A.walk(_zlib(fmt, level, d), fmt)
            assert out == d, (fmt, level, len(d))
            assert blocks[-1].final and not any(b.final for b in blocks[:-1])
            assert sum(b.out_len for b in blocks) == len(d)


@pytest.mark.parametrize("fmt", ["deflate", "zlib"])
def test_walker_resolves_dictionary_distances(fmt):
    zdict = datagen.text_chunk(32768, 0x0E1100D1)
    body = zdict[1000:9000] + datagen.text_chunk(20000, 0x0E1100D2)
    z = _zlib(fmt, 6, body, zdict)
    out, blocks = A.walk(z, fmt, zdict)
    assert out == body
    assert max(m[1] for b in blocks for m in b.matches) > 20000   # into the dictionary
    with pytest.raises(A.StreamError):
        A.walk(z, fmt)


def test_walker_agrees_with_reference_and_block_map(oracle, ref):
    """streams of the real reference at every level: decoded bytes, block
    starts (bit, output position, type, final) as oracle.block_map() sees
    them; the reference's run-length coding and header trims are exactly
    precode_items_ref / trimmed_counts / trimmed_hclen"""
    for level in range(1, 13):
        for d in _inputs()[1:]:
            z = ref.compress("deflate", level, d)
            out, blocks = A.walk(z)
            assert out == d, level
            bm, res = oracle.block_map(z, len(d))
            assert res == 0
            assert [(b.start_bit, b.out_start, b.type, b.final) for b in blocks] == \
                [tuple(x) for x in bm], level
            for b in blocks:
                if b.type != 2:
                    continue
                assert (b.hlit, b.hdist) == A.trimmed_counts(b.ll_lens, b.d_lens)
                assert b.hclen == A.trimmed_hclen(b.pre_lens)
                assert b.pre_items == A.precode_items_ref(b.ll_lens[:b.hlit] +
                                                          b.d_lens[:b.hdist])


def test_walker_on_oracle_streams(oracle):
    for level in (1, 6, 9, 12):
        for d in _inputs():
            out, blocks = A.walk(oracle.compress("zlib", level, d), "zlib")
            assert out == d
            bm, _ = oracle.block_map(A.strip_container(oracle.compress("zlib", level, d),
                                                       "zlib"), len(d))
            assert [b.start_bit for b in blocks] == [x[0] for x in bm]


# ------------------------------------------------------------ the references

def _brute(freq, limit):
    """cheapest complete prefix code within the limit, by enumeration"""
    used = [f for f in freq if f]
    if len(used) < 2:
        return sum(used)
    best = None
    for lens in itertools.product(range(1, limit + 1), repeat=len(used)):
        if sum(2.0 ** -x for x in lens) <= 1.0:
            c = sum(f * x for f, x in zip(used, lens))
            best = c if best is None else min(best, c)
    return best


def test_package_merge_and_huffman_against_brute_force():
    rng = random.Random(0x0E1100D3)
    for _ in range(150):
        m = rng.randint(1, 6)
        freq = [rng.choice([1, 1, 2, 3, 5, 8, 13, 100, rng.randint(1, 1000)])
                for _ in range(m)] + [0] * rng.randint(1, 3)
        rng.shuffle(freq)
        for limit in range(max(1, (m - 1).bit_length()), 6):
            assert A.package_merge(freq, limit) == _brute(freq, limit), (freq, limit)
        assert A.huffman_cost(freq) == _brute(freq, 6), freq
        lens = A.restated_make_code(freq, 15)
        assert A.code_cost(freq, lens) == A.huffman_cost(freq)


def test_package_merge_equals_huffman_when_the_tree_fits():
    rng = random.Random(0x0E1100D4)
    for _ in range(100):
        freq = [rng.randint(0, 5000) for _ in range(rng.randint(2, 288))]
        info = {}
        lens = A.restated_make_code(freq, 15, info)
        if not info["clamped"]:
            assert A.package_merge(freq, 15) == A.huffman_cost(freq) == \
                A.code_cost(freq, lens)
        assert A.kraft_sum(lens) == 1 << 15 or info["m"] < 2


@pytest.mark.parametrize("k,limit", [(20, 15), (22, 15), (30, 15), (12, 7), (19, 7)])
def test_package_merge_beats_the_repair_on_fibonacci(k, limit):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    info = {}
    lens = A.restated_make_code(f, limit, info)
    assert info["clamped"] and max(lens) == limit
    assert A.kraft_sum(lens) == 1 << 15
    assert A.package_merge(f, limit) < A.code_cost(f, lens)


def test_restated_make_code_small_alphabets():
    assert A.restated_make_code([0] * 30, 15)[:2] == [1, 1]
    lens = A.restated_make_code([0] * 5 + [7] + [0] * 24, 15)
    assert {s for s, x in enumerate(lens) if x} == {0, 5} and lens[0] == lens[5] == 1
    lens = A.restated_make_code([9] + [0] * 29, 15)
    assert {s for s, x in enumerate(lens) if x} == {0, 1}
    # ties: equal frequencies, the lower symbol ranks lower -> longer code
    lens = A.restated_make_code([5, 5, 5], 15)
    assert lens == [2, 2, 1]


def test_precode_items_ref_runs():
    assert A.precode_items_ref([0] * 139) == [(18, 138), (0, None)]
    assert A.precode_items_ref([0] * 148) == [(18, 138), (17, 10)]
    assert A.precode_items_ref([0] * 10) == [(17, 10)]
    assert A.precode_items_ref([0, 0]) == [(0, None)] * 2
    assert A.precode_items_ref([5] * 4) == [(5, None), (16, 3)]
    assert A.precode_items_ref([5] * 8) == [(5, None), (16, 6), (5, None)]
    assert A.precode_items_ref([5] * 10) == [(5, None), (16, 6), (16, 3)]
    assert A.precode_items_ref([5] * 3) == [(5, None)] * 3


def test_cost_formulas():
    assert A.stored_cost(0, 0) == 40
    assert A.stored_cost(5, 10) == 3 + 0 + 32 + 80
    assert A.stored_cost(0, 65535) == 40 + 8 * 65535
    assert A.stored_cost(0, 65536) == 80 + 8 * 65536
    h = [0] * 288
    h[65], h[256] = 3, 1
    assert A.static_cost(h, [0] * 32) == 3 + 3 * 8 + 7


# ------------------------------------------------------------ negative cases

def _hist(tokens):
    ll, dd = [0] * 288, [0] * 32
    for t in tokens:
        if len(t) == 1:
            ll[t[0]] += 1
        else:
            ll[t[2]] += 1
            dd[A.dist_sym(t[1])] += 1
    ll[256] += 1
    return ll, dd


def _emit_dynamic(tokens, ll_lens=None, d_lens=None, hlit_extra=0, pre_lens=None,
                  extra_pre=None):
    """one final dynamic block: tokens are (byte,) or (length, dist, lsym,
    lextra); the code lengths default to restated_make_code of the tokens'
    histogram, the header to what the block end derives from them"""
    ll, dd = _hist(tokens)
    ll_lens = ll_lens or A.restated_make_code(ll, 15)
    d_lens = d_lens or A.restated_make_code(dd, 15)
    hlit, hdist = A.trimmed_counts(ll_lens, d_lens)
    hlit += hlit_extra
    items = A.precode_items_ref(ll_lens[:hlit] + d_lens[:hdist])
    ph = [0] * 19
    for s, _ in items:
        ph[s] += 1
    pre_lens = pre_lens or A.restated_make_code(ph, 7)
    if extra_pre is not None:
        pre_lens = list(pre_lens)
        pre_lens[extra_pre[0]] = extra_pre[1]
    hclen = A.trimmed_hclen(pre_lens)
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(pre_lens[A.PERM[i]], 3)
    pc = A.canonical_codes(pre_lens)
    for s, r in items:
        w.put_code(pc[s], pre_lens[s])
        if s == 16:
            w.put(r - 3, 2)
        elif s == 17:
            w.put(r - 3, 3)
        elif s == 18:
            w.put(r - 11, 7)
    lc, dc = A.canonical_codes(ll_lens), A.canonical_codes(d_lens)
    for t in tokens:
        if len(t) == 1:
            w.put_code(lc[t[0]], ll_lens[t[0]])
            continue
        length, dist, ls, le = t
        w.put_code(lc[ls], ll_lens[ls])
        w.put(le, A.ll_extra(ls))
        ds = A.dist_sym(dist)
        w.put_code(dc[ds], d_lens[ds])
        w.put(dist - A.DIST_BASE[ds], A.d_extra(ds))
    w.put_code(lc[256], ll_lens[256])
    return w.finish(), ll, dd


def _base_tokens(longest=258):
    """text-like literals and matches, one of length `longest` among them"""
    rng = random.Random(0x0E1100D5)
    toks, out = [], bytearray()
    for _ in range(400):
        if len(out) > 300 and rng.random() < 0.3:
            length = rng.choice([3, 4, 5, 8, 13, 30, longest])
            dist = rng.randint(1, len(out))
            toks.append((length, dist, A.len_sym(length), length - A.LEN_BASE[A.len_sym(length) - 257]))
            for _ in range(length):
                out.append(out[-dist])
        else:
            c = rng.choice(b"etaoinshrdlu  ")
            toks.append((c,))
            out.append(c)
    return toks, bytes(out)


def _fired(stream, data):
    blocks, bad = A.audit_stream(stream, expect=data)
    return {c for c, _, _ in bad}


def test_hand_built_base_stream_is_clean():
    toks, data = _base_tokens()
    z, _, _ = _emit_dynamic(toks)
    assert zlib.decompress(z, -15) == data
    assert _fired(z, data) == set()


def _case_hlit_plus_one():
    toks, data = _base_tokens(longest=200)     # HLIT 286 has no room for one more
    return _emit_dynamic(toks, hlit_extra=1)[0], data


def _case_not_optimal():
    toks, data = _base_tokens()
    ll, _ = _hist(toks)
    lens = A.restated_make_code(ll, 15)
    common = max(range(288), key=lambda s: ll[s])
    rare = min((s for s in range(288) if ll[s]), key=lambda s: (ll[s], -lens[s]))
    assert lens[common] < lens[rare]
    lens[common], lens[rare] = lens[rare], lens[common]
    return _emit_dynamic(toks, ll_lens=lens)[0], data


def _case_oversubscribed_precode():
    toks, data = _base_tokens()
    # an unused precode symbol gets a 7-bit codeword on top of a complete code
    return _emit_dynamic(toks, extra_pre=(15, 7))[0], data


def _case_258_as_284():
    toks, data = _base_tokens()
    toks = [(258, t[1], 284, 31) if len(t) == 4 and t[0] == 258 else t for t in toks]
    assert any(len(t) == 4 and t[2] == 284 for t in toks)
    return _emit_dynamic(toks)[0], data


def _case_static_over_stored():
    data = bytes(random.Random(0x0E1100D6).randrange(144, 256) for _ in range(300))
    w = BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    lc = A.canonical_codes(A.STATIC_LL)
    for c in data:
        w.put_code(lc[c], 9)
    w.put_code(lc[256], 7)
    return w.finish(), data


def _case_unused_codeword():
    toks, data = _base_tokens()
    ll, _ = _hist(toks)
    lens = A.restated_make_code(ll, 15)
    # split the rarest used symbol's leaf with an unused symbol: still complete
    rare = min((s for s in range(288) if ll[s]), key=lambda s: (ll[s], -lens[s]))
    unused = next(s for s in range(1, 256) if not ll[s])
    lens[rare] += 1
    lens[unused] = lens[rare]
    assert A.kraft_sum(lens) == 1 << 15
    return _emit_dynamic(toks, ll_lens=lens)[0], data


# case -> (the check it is built to break, checks that follow from the same
# defect and may fire beside it)
NEGATIVE = {
    _case_hlit_plus_one: ("header_trim", set()),
    _case_not_optimal: ("optimal", {"restated_lens"}),
    _case_oversubscribed_precode: ("kraft", {"used_iff_coded", "restated_lens",
                                            "header_trim"}),
    _case_258_as_284: ("symbols", set()),
    _case_static_over_stored: ("choice", set()),
    _case_unused_codeword: ("used_iff_coded", {"optimal", "restated_lens"}),
}


@pytest.mark.parametrize("case", list(NEGATIVE), ids=lambda f: f.__name__[6:])
def test_each_invariant_has_a_stream_that_breaks_it(case):
    z, data = case()
    if case is not _case_oversubscribed_precode:        # no decoder takes that one
        assert zlib.decompress(z, -15) == data
    target, companions = NEGATIVE[case]
    fired = _fired(z, data)
    assert target in fired, (case.__name__, fired)
    assert fired - {target} <= companions, (case.__name__, fired)


def test_negative_cases_hit_different_checks():
    targets = [t for t, _ in NEGATIVE.values()]
    assert len(set(targets)) == len(targets)
