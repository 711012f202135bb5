"""Preset dictionaries on the GPU (libdeflate_amd_*_dict), with Python's zlib
(`zdict=`) as the oracle throughout: zlib -> GPU, GPU -> zlib, GPU round
trips, the negative cases, the empty dictionary and the compression ratio."""
import random
import zlib

import pytest

from libdeflate_amd import binding
from tests import datagen, streams

pytestmark = pytest.mark.gpu

MODES = ("1", "0")      # LDA_INFLATE_PAR: wave per stream, lane per stream


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def _records(count, lo, hi, seed):
    rng = random.Random(seed)
    return [datagen.text_chunk(rng.randrange(lo, hi + 1), seed + i) for i in range(count)]


def _dictionary(n, seed):
    """n bytes of text records of seeds no test record uses"""
    out = b""
    k = 0
    while len(out) < n:
        out += datagen.text_chunk(4096, seed + k)
        k += 1
    return out[:n]


def _pack(chunks, dev):
    import torch
    offs, blob = [], bytearray()
    for c in chunks:
        offs.append(len(blob))
        blob += c
        blob += bytes(-len(blob) % 16)
    data = torch.frombuffer(bytearray(blob) + bytearray(64), dtype=torch.uint8).to(dev)
    return (data, torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor([len(c) for c in chunks], dtype=torch.int64, device=dev))


def _slots(avail, dev):
    import torch
    offs, pos = [], 0
    for a in avail:
        offs.append(pos)
        pos += (a + 15) // 16 * 16 + 16
    return (torch.zeros(pos + 64, dtype=torch.uint8, device=dev),
            torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor(avail, dtype=torch.int64, device=dev))


def _dict_tensor(d, dev):
    import torch
    return torch.frombuffer(bytearray(d) + bytearray(1), dtype=torch.uint8)[:len(d)].to(dev)


def gpu_compress(c, fmt, d, chunks, dict_call=True):
    """-> compressed bytes per chunk (None where it did not fit)"""
    import torch
    dev = torch.device("cuda:0")
    data, off, n = _pack(chunks, dev)
    avail = [c.bound(fmt, len(x)) + 4 for x in chunks]
    out, ooff, oav = _slots(avail, dev)
    on = torch.zeros(len(chunks), dtype=torch.int64, device=dev)
    if dict_call:
        c.compress_batch_dict(fmt, _dict_tensor(d, dev), data, off, n, out, ooff, oav, on)
    else:
        c.compress_batch(fmt, data, off, n, out, ooff, oav, on)
    torch.cuda.synchronize()
    host, ooff, on = out.cpu().numpy(), ooff.cpu().tolist(), on.cpu().tolist()
    return [host[o:o + k].tobytes() if k else None for o, k in zip(ooff, on)]


def gpu_decompress(dec, fmt, d, comp, avail, dict_call=True, want_actual_out=True):
    """-> (result, actual_in, actual_out, bytes) per stream"""
    import torch
    dev = torch.device("cuda:0")
    data, off, n = _pack(comp, dev)
    out, ooff, oav = _slots(avail, dev)
    k = len(comp)
    res = torch.full((k,), -1, dtype=torch.int32, device=dev)
    ain = torch.zeros(k, dtype=torch.int64, device=dev)
    aout = torch.zeros(k, dtype=torch.int64, device=dev) if want_actual_out else None
    if dict_call:
        dec.decompress_batch_dict(fmt, _dict_tensor(d, dev), data, off, n, out, ooff, oav,
                                  res, ain, aout)
    else:
        dec.decompress_batch(fmt, data, off, n, out, ooff, oav, res, ain, aout)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    res, ain = res.cpu().tolist(), ain.cpu().tolist()
    aout = aout.cpu().tolist() if want_actual_out else list(avail)
    return [(r, i, o if want_actual_out else 0,
             host[s:s + o].tobytes() if r == 0 else b"")
            for r, i, o, s in zip(res, ain, aout, ooff.cpu().tolist())]


def zlib_compress(fmt, level, d, data):
    co = zlib.compressobj(level, zlib.DEFLATED, 15 if fmt == "zlib" else -15, zdict=d)
    return co.compress(data) + co.flush()


def zlib_decompress(fmt, d, z):
    do = zlib.decompressobj(15 if fmt == "zlib" else -15, zdict=d)
    return do.decompress(z) + do.flush()


def _bad_distance_dicts():
    """The dictionaries streams.bad_distance_streams() compressed with (the
    same random sequence) -> list of (stream, zdict, original)"""
    rng = random.Random(0x0E110032)
    out = []
    for at in (0, 700, 5000):
        words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(3, 9)))
                 for _ in range(300)]
        text = b" ".join(rng.choice(words) for _ in range(12000))
        zdict = text[20000:52768] if at == 0 else bytes(rng.randrange(256) for _ in range(32768))
        body = text[:at] + zdict[1000:1400] + text[at:]
        out.append((zlib_compress("deflate", 6, zdict, body), zdict, body))
    return out


def _set_mode(monkeypatch, mode):
    monkeypatch.setenv("LDA_INFLATE_PAR", mode)
    binding.reload_env()


@pytest.mark.parametrize("mode", MODES)
def test_bad_distance_streams_decode_with_their_dictionary(dec, monkeypatch, mode):
    _set_mode(monkeypatch, mode)
    cases = _bad_distance_dicts()
    assert [c[0] for c in cases] == streams.bad_distance_streams()
    bad = 0
    for z, zd, body in cases:
        got = gpu_decompress(dec, "deflate", zd, [z], [len(body) + 100])[0]
        assert got == (0, len(z), len(body), body)
        # without the dictionary: invalid where zlib says so (the call
        # without a dictionary is unchanged)
        try:
            plain = zlib.decompress(z, -15)
        except zlib.error:
            plain = None
        got = gpu_decompress(dec, "deflate", b"", [z], [len(body) + 100], dict_call=False)[0]
        assert got[0] == (binding.BAD_DATA if plain is None else 0)
        bad += plain is None
        r, ain, aout, out = dec.decompress_dict_ex("deflate", zd, z, len(body) + 100)
        assert (r, ain, aout, out) == (0, len(z), len(body), body)
    assert bad >= 2


DICT_SIZES = (1, 100, 4095, 4096, 20480, 32768, 102400)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("level", (1, 6, 9))
def test_zlib_to_gpu(dec, monkeypatch, mode, level):
    _set_mode(monkeypatch, mode)
    sizes = [0, 1, 17, 300, 4095, 4096, 5000, 20000, 40000, 65536]
    for fmt in ("deflate", "zlib"):
        for dn in DICT_SIZES:
            d = _dictionary(dn, 0xD1C7 + dn)
            recs = [datagen.text_chunk(n, 0x5EED + n) if n else b"" for n in sizes]
            comp = [zlib_compress(fmt, level, d, r) for r in recs]
            got = gpu_decompress(dec, fmt, d, comp, [len(r) + 16 for r in recs])
            for r, z, g in zip(recs, comp, got):
                assert g == (0, len(z), len(r), r), (fmt, dn, len(r), g[:3])
    # a 1 MiB record, batch and single buffer
    big = datagen.text_chunk(1 << 20, 0xB16)
    d = _dictionary(32768, 0xD1C7)
    for fmt in ("deflate", "zlib"):
        z = zlib_compress(fmt, level, d, big)
        assert gpu_decompress(dec, fmt, d, [z], [len(big)])[0] == (0, len(z), len(big), big)
        assert dec.decompress_dict_ex(fmt, d, z, len(big)) == (0, len(z), len(big), big)


def test_zlib_to_gpu_single_buffer(dec):
    for fmt in ("deflate", "zlib"):
        for dn in DICT_SIZES:
            d = _dictionary(dn, 0xD1C7 + dn)
            for n in (0, 100, 5000, 65536):
                r = datagen.text_chunk(n, 0xA11 + n) if n else b""
                z = zlib_compress(fmt, 6, d, r)
                assert dec.decompress_dict_ex(fmt, d, z, n + 8) == (0, len(z), n, r)
                # exact fill
                got = dec.decompress_dict_ex(fmt, d, z, n, want_actual_out=False)
                assert got[0] == 0 and got[3] == r


def _check_zlib_header(z, d):
    cmf, flg = z[0], z[1]
    assert (cmf * 256 + flg) % 31 == 0
    assert flg & 0x20
    assert int.from_bytes(z[2:6], "big") == zlib.adler32(d)


@pytest.mark.parametrize("level", (0, 1, 6, 9, 10, 12))
def test_gpu_to_zlib(level):
    from libdeflate_amd import api
    c = api.Compressor(level)
    sizes = [0, 1, 5, 60, 300, 1000, 4096, 4097, 9000, 30000, 65536]
    for fmt in ("deflate", "zlib"):
        for dn in (1, 100, 4095, 4096, 20480, 102400):
            d = _dictionary(dn, 0xD1C7 + dn)
            recs = [datagen.text_chunk(n, 0x7E57 + n) if n else b"" for n in sizes]
            comp = gpu_compress(c, fmt, d, recs)
            for r, z in zip(recs, comp):
                assert z is not None
                assert zlib_decompress(fmt, d, z) == r, (fmt, dn, len(r))
                if fmt == "zlib":
                    _check_zlib_header(z, d)
        # single buffer, including one that takes the segmented path
        d = _dictionary(20480, 0xD1C7)
        for n in (0, 3000, 70000, 300000):
            r = datagen.text_chunk(n, 0x51 + n) if n else b""
            z = c.compress_dict(fmt, d, r)
            assert z is not None and zlib_decompress(fmt, d, z) == r, (fmt, n)
            if fmt == "zlib":
                _check_zlib_header(z, d)
    c.close()


def test_dictionary_is_used_by_the_compressor():
    """A record that repeats the dictionary's tail compresses to far less than
    the record alone, down to dictionaries of a few bytes and past a tile"""
    from libdeflate_amd import api
    c = api.Compressor(6)
    for dn in (40, 4095, 4097, 20480):
        d = _dictionary(dn, 0xFEED + dn)
        rec = d[-min(dn, 20000):]
        z = gpu_compress(c, "deflate", d, [rec])[0]
        assert zlib_decompress("deflate", d, z) == rec
        assert len(z) < len(rec) // 4 + 20, (dn, len(z))
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_round_trip(dec, monkeypatch, mode):
    from libdeflate_amd import api
    _set_mode(monkeypatch, mode)
    recs = _records(300, 0, 9000, 0x4077)
    recs += [datagen.chunk(i, 65536, 0x0E1100AA) for i in range(6)]
    d = _dictionary(16384, 0xD1C7)
    for level in (1, 6, 11):
        c = api.Compressor(level)
        for fmt in ("deflate", "zlib"):
            comp = gpu_compress(c, fmt, d, recs)
            got = gpu_decompress(dec, fmt, d, comp, [len(r) for r in recs])
            for r, z, g in zip(recs, comp, got):
                assert g == (0, len(z), len(r), r)
        c.close()


def test_negative_cases(dec):
    from libdeflate_amd import api
    d = _dictionary(8192, 0xD1C7)
    rec = datagen.text_chunk(20000, 0x0BAD)
    z = zlib_compress("zlib", 6, d, rec)
    good = (0, len(z), len(rec), rec)
    # a wrong dictionary, no dictionary
    wrong = d[:-1] + bytes([d[-1] ^ 1])
    got = gpu_decompress(dec, "zlib", wrong, [z, z], [30000, 30000])
    assert [g[0] for g in got] == [binding.BAD_DATA] * 2
    assert dec.decompress_dict_ex("zlib", wrong, z, 30000)[0] == binding.BAD_DATA
    assert dec.decompress_dict_ex("zlib", b"", z, 30000)[0] == binding.BAD_DATA
    got = gpu_decompress(dec, "zlib", b"", [z], [30000])
    assert got[0][0] == binding.BAD_DATA
    # the calls without a dictionary still refuse FDICT
    assert dec.decompress_ex("zlib", z, 30000)[0] == binding.BAD_DATA
    # a zlib stream without FDICT decodes as if no dictionary were given
    plain = zlib.compress(rec, 6)
    assert gpu_decompress(dec, "zlib", d, [plain], [30000])[0] == (0, len(plain), len(rec), rec)
    # a distance one byte beyond dictionary + output
    w = streams.BitWriter()
    w.put(1, 1)
    w.put(1, 2)                     # final, static
    streams._static_lit(w, 65)
    streams._static_match(w, 3, len(d) + 2)
    streams._static_lit(w, 256)
    raw = w.finish()
    assert gpu_decompress(dec, "deflate", d, [raw], [100])[0][0] == binding.BAD_DATA
    w = streams.BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    streams._static_lit(w, 65)
    streams._static_match(w, 3, len(d) + 1)
    streams._static_lit(w, 256)
    raw_ok = w.finish()
    assert zlib_decompress("deflate", d, raw_ok) == b"A" + d[:3]
    assert gpu_decompress(dec, "deflate", d, [raw_ok], [100])[0] == (0, len(raw_ok), 4, b"A" + d[:3])
    # gzip takes no dictionary
    import torch
    dev = torch.device("cuda:0")
    data, off, n = _pack([rec], dev)
    out, ooff, oav = _slots([30000], dev)
    res = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="status -2"):
        dec.decompress_batch_dict("gzip", _dict_tensor(d, dev), data, off, n, out, ooff,
                                  oav, res)
    c = api.Compressor(6)
    with pytest.raises(RuntimeError, match="status -2"):
        c.compress_batch_dict("gzip", _dict_tensor(d, dev), data, off, n, out, ooff, oav,
                              torch.zeros(1, dtype=torch.int64, device=dev))
    assert c.compress_dict("gzip", d, rec, 40000) is None
    assert dec.decompress_dict_ex("gzip", d, z, 30000)[0] == binding.BAD_DATA
    c.close()
    # truncated streams: never SUCCESS unless zlib decodes the same bytes;
    # a failed stream leaves its neighbours alone
    for fmt in ("deflate", "zlib"):
        z = zlib_compress(fmt, 6, d, rec)
        cuts = sorted(set([0, 1, 2, 5, 6, 7, 10] + list(range(11, len(z), max(1, len(z) // 40)))))
        batch = []
        for k in cuts:
            batch += [z[:k], z]
        got = gpu_decompress(dec, fmt, d, batch, [30000] * len(batch))
        for k, (gt, gf) in zip(cuts, zip(got[0::2], got[1::2])):
            assert gf == (0, len(z), len(rec), rec), (fmt, k)
            if gt[0] == 0:
                do = zlib.decompressobj(15 if fmt == "zlib" else -15, zdict=d)
                assert do.decompress(z[:k]) == gt[3] and do.eof, (fmt, k)


def test_empty_dictionary_is_the_plain_call(dec):
    from libdeflate_amd import api
    recs = _records(64, 0, 20000, 0xE3)
    for level in (1, 6, 12):
        c = api.Compressor(level)
        for fmt in ("deflate", "zlib"):
            a = gpu_compress(c, fmt, b"", recs, dict_call=True)
            b = gpu_compress(c, fmt, b"", recs, dict_call=False)
            assert a == b
            for want in (True, False):
                avail = [len(r) for r in recs]
                x = gpu_decompress(dec, fmt, b"", b, avail, True, want)
                y = gpu_decompress(dec, fmt, b"", b, avail, False, want)
                assert x == y
            assert c.compress_dict(fmt, b"", recs[3]) == c.compress(fmt, recs[3])
        c.close()


@pytest.mark.parametrize("level", (6, 9))
def test_ratio_against_zlib(level):
    from libdeflate_amd import api
    recs = _records(2048, 256, 4096, 0x2A71)
    d = _dictionary(16384, 0x90000)
    def zco(r, zd):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, **({"zdict": zd} if zd else {}))
        return co.compress(r) + co.flush()

    z_plain = sum(len(zco(r, None)) for r in recs)
    z_dict = sum(len(zco(r, d)) for r in recs)
    c = api.Compressor(level)
    g_dict = gpu_compress(c, "deflate", d, recs)
    g_plain = gpu_compress(c, "deflate", b"", recs, dict_call=False)
    c.close()
    for r, z in zip(recs, g_dict):
        assert zlib_decompress("deflate", d, z) == r
    gd, gp = sum(map(len, g_dict)), sum(map(len, g_plain))
    assert gd <= 1.03 * z_dict, (gd, z_dict)
    assert abs(gd / gp - z_dict / z_plain) <= 0.03, (gd / gp, z_dict / z_plain)
