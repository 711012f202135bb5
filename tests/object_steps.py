"""A catalogue of *steps* for the tests that queue calls of different families
on ONE Compressor or Decompressor (tests/test_object_sequences_gpu.py).

A step is one library call (or the two or three calls that belong together,
such as index + extract) with everything around it:

    prepare(torch, obj)   uploads the inputs to staging tensors, allocates the
                          call's own input tensors (zeros) and its outputs
                          (0xA5 with guard bytes on both sides) -> a handle
    launch(obj, h, s)     copies staging -> input on the stream `s` and makes
                          the call behind it; no synchronisation
    check(h)              after the final synchronise: every output byte, every
                          result word and index row, and the guards, against
                          `expected`; returns the bytes a compressor wrote
    validate()            (CPU) holds `expected` against a second CPU source; a
                          compressor step, whose expectation is its own input,
                          shows instead that the CPU decoder of its check()
                          reads zlib's stream of that input

`expected` never comes from the library: the oracle, zlib, gzip, zipfile,
tarfile, and the models and builders the suite already has (tools/models,
tests/*_files.py, *_expect.py, deflate_synth.py).  Compressed output has no
CPU reference for its bytes, so a compressor step checks that a CPU decoder
gives the input back; the sequence tests add a byte comparison with what a
fresh object returns for the same call made alone.

Which step touches which field of the object (csrc/host_objects.h):

    step                      family          blocking  fields
    ------------------------  --------------  --------  -----------------------------
    batch*                    batch           no        d->tokens, d->scratch
    dict                      batch-dict      no        d->tokens, d->scratch
    prefix                    prefix          no        d->tokens, d->scratch
    sizes                     sizes           no        d->scratch
    packed                    packed          no        d->tokens, d->scratch
    zip*                      zip             no        d->bgzf, d->bgzf_up, d->tokens
    zip-read                  zip             no        d->bgzf, d->bgzf_up, d->tokens
    zip-large                 zip-large       yes       d->bgzf, d->bgzf_up, d->tokens, s_copy, s_run
    tar*, tar-read            tar             no        d->bgzf, d->bgzf_up
    bgzf*, bgzf-read          bgzf            no        d->bgzf, d->bgzf_up, d->tokens
    gzm*, gzm-peek            gzip-members    no        d->bgzf, d->bgzf_up, d->tokens
    large, large-damaged      stream          yes       d->tokens, d->scratch, s_copy, s_run
    large-index, seek-read    stream / seek   yes / no  d->tokens, d->scratch, s_copy, s_run
    batch-host, ex-host       host            yes       d->tokens, d->scratch, pinned slices
    refused-*                 refused         no        - (the call returns before any device work)

    (reader_steps(): the readers that joined the shared host pipeline later)
    png, png-zero             png             no        d->bgzf, d->bgzf_up, d->tokens
    png-pixels                png-pixels      no        d->bgzf, d->bgzf_up, d->tokens
    png-ex, png-ex-raw        png-adam7       no        d->bgzf, d->bgzf_up, d->tokens
    shuffle                   shuffle         no        d->bgzf, d->bgzf_up, d->tokens
    refused-png*, -shuffle    refused         no        -

    c-batch-large/-small      compress        no        c->scratch
    c-dict                    compress-dict   no        c->scratch
    c-zip                     zip-write       no        c->zipw, c->zipw_up, c->scratch
    c-gzm                     gzm-write       no        c->zipw, c->zipw_up, c->scratch
    c-png                     png-write       no        c->zipw, c->zipw_up, c->scratch
    c-tar                     tar-write       no        c->zipw, c->zipw_up
    c-targz                   tar-write       no        c->zipw, c->zipw_up, c->large, c->scratch
    c-large                   compress-large  no        c->large, c->scratch
    c-bgzf                    bgzf-write      no        c->scratch
    c-batch-host, c-one,      host            yes       c->scratch, pinned slices
    c-bgzf-host
"""
import gzip
import io
import random
import tarfile
import zipfile
import zlib

import numpy as np

from tests import bgzf_files, bgzf_walk, datagen
from tests import deflate_synth as S
from tests import gzip_members_files as gf
from tests import png_adam7_files as p7
from tests import png_files as pf
from tests import prefix_expect, shuffle_chunks, sizes_expect
from tests import tar_files as tf
from tests import tar_write_cases as tw
from tests import zip_files as zf
from tests import zip_large_files as zl
from tools.models import png_adam7 as p7m
from tools.models import png_model as pm
from tools.models import png_pixels_model as px
from tools.models import png_write as pw
from tools.models import shuffle_model as sm
from tools.models import tar_walk, zip_walk

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
PREFIX = 19
HAS_EOF = 1
CANARY = 0xA5
GUARD = 64          # bytes on both sides of every byte output
WGUARD = 8          # entries on both sides of every word output
UNSET = -7          # result words and rows where nothing was written
DEVICE = "cuda"     # (tests/test_object_steps.py looks at the checks themselves on "cpu")
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}
B = bgzf_walk.BLOCK


class Handle:
    """what prepare() made: tensors, and whatever a blocking call returned"""

    def __init__(self):
        self.copies = []        # (input tensor, staging tensor)


class Guarded:
    """a device tensor with guard entries on both sides of the part a call gets"""

    def __init__(self, torch, n, dtype=None, fill=CANARY):
        dtype = torch.uint8 if dtype is None else dtype
        self.guard = GUARD if dtype == torch.uint8 else WGUARD
        self.n, self.fill = n, fill
        self.whole = torch.full((n + 2 * self.guard,), fill, dtype=dtype, device=DEVICE)
        self.t = self.whole[self.guard:self.guard + n]

    def host(self, what):
        """the n entries as numpy, after looking at the guards"""
        h = self.whole.cpu().numpy()
        g = self.guard
        assert (h[:g] == self.fill).all(), f"{what}: written in front of the tensor"
        assert (h[g + self.n:] == self.fill).all(), f"{what}: written behind the tensor"
        return h[g:g + self.n]


def _stage(torch, h, data, behind=b""):
    """the bytes on the device twice: a staging copy, and the (still zero)
    tensor the call reads, which launch() fills on the call's stream"""
    src = torch.frombuffer(bytearray(data) + bytearray(behind) + bytearray(16),
                           dtype=torch.uint8).to(DEVICE)
    dst = torch.zeros_like(src)
    h.copies.append((dst, src))
    return dst


def _i64(torch, v):
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=DEVICE)


def _pack(chunks, align=16):
    """-> (blob, offsets): the chunks one behind the other at aligned offsets"""
    offs, blob = [], bytearray()
    for c in chunks:
        offs.append(len(blob))
        blob += c
        blob += bytes(-len(blob) % align)
    return bytes(blob), offs


def _image(n, pieces):
    """n bytes of CANARY with (offset, bytes) laid over them"""
    want = np.full(n, CANARY, dtype=np.uint8)
    for off, b in pieces:
        if b:
            want[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return want


def _same(got, want, what, free=()):
    """numpy byte images equal but for the `free` (offset, length) regions"""
    ne = got != want
    for off, n in free:
        ne[off:off + n] = False
    assert not ne.any(), \
        f"{what}: {int(ne.sum())} bytes differ, the first at {int(np.flatnonzero(ne)[0])}"


class Step:
    name = family = fields = ""
    blocking = False

    def prepare(self, torch, obj=None):
        raise NotImplementedError

    def enqueue(self, obj, h, stream):
        raise NotImplementedError

    def launch(self, obj, h, stream):
        """the inputs on `stream`, then the call behind them"""
        import torch
        with torch.cuda.stream(stream):
            for dst, src in h.copies:
                dst.copy_(src, non_blocking=True)
        self.enqueue(obj, h, stream)

    def check(self, h):
        raise NotImplementedError

    def validate(self):
        raise NotImplementedError

    def __repr__(self):
        return self.name


# ===================================================================== inflate

_zcache = {}


def zcases(fmt, count, lo, hi, seed):
    """`count` S.Case of zlib's streams, sizes log-uniform in lo..hi bytes,
    levels 1 / 6 / 9; built once, a shorter list is a prefix of a longer one"""
    key = (fmt, lo, hi, seed)
    have = _zcache.setdefault(key, [])
    rng = random.Random(seed)
    sizes = [max(lo, min(hi, int(lo * (hi / lo) ** rng.random()))) for _ in range(max(count, len(have)))]
    for i in range(len(have), count):
        data = datagen.chunk(i, sizes[i], seed)
        co = zlib.compressobj((1, 6, 9)[i % 3], zlib.DEFLATED, WBITS[fmt])
        have.append(S.Case(f"z{i}", fmt, co.compress(data) + co.flush(), data, ()))
    return have[:count]


class Batch(Step):
    """decompress_batch / decompress_batch_dict: slots back to back at odd
    offsets with 13 bytes between them"""
    family, fields = "batch", "d->tokens, d->scratch"
    GAP = 13

    def __init__(self, name, fmt, cases, oracle, dictionary=None):
        self.name, self.fmt, self.cases, self.dictionary = name, fmt, cases, dictionary
        if dictionary is not None:
            self.family = "batch-dict"
            self.expected = [S.dict_verdict(oracle, c, c.avail) for c in cases]
        else:
            self.expected = [oracle.decompress_ex(fmt, c.data, c.avail) for c in cases]

    def validate(self):
        for c, e in zip(self.cases, self.expected):
            if c.valid and c.avail >= len(c.out):
                assert e[0] == SUCCESS and e[2] == len(c.out) and e[3] == c.out, c.name
                try:
                    d = zlib.decompressobj(WBITS[self.fmt], zdict=self.dictionary) \
                        if self.dictionary is not None else zlib.decompressobj(WBITS[self.fmt])
                    z = d.decompress(c.data)
                except zlib.error:
                    assert c.ref_only or c.tags, c.name     # (what zlib refuses: hand-built only)
                else:
                    assert z == c.out, c.name
            else:
                assert e[0] != SUCCESS, c.name

    def prepare(self, torch, obj=None):
        h = Handle()
        n = len(self.cases)
        blob, offs = _pack([c.data for c in self.cases])
        h.data = _stage(torch, h, blob)
        h.in_off, h.in_n = _i64(torch, offs), _i64(torch, [len(c.data) for c in self.cases])
        h.ooffs, pos = [], 1
        for c in self.cases:
            h.ooffs.append(pos)
            pos += c.avail + self.GAP
        h.out = Guarded(torch, pos)
        h.out_off, h.avail = _i64(torch, h.ooffs), _i64(torch, [c.avail for c in self.cases])
        h.res = Guarded(torch, n, torch.int32, UNSET)
        h.ain = Guarded(torch, n, torch.int64, UNSET)
        h.aout = Guarded(torch, n, torch.int64, UNSET)
        if self.dictionary is not None:
            h.dict = _stage(torch, h, self.dictionary)[:len(self.dictionary)]
        return h

    def enqueue(self, obj, h, stream):
        args = (h.data, h.in_off, h.in_n, h.out.t, h.out_off, h.avail, h.res.t, h.ain.t, h.aout.t)
        if self.dictionary is None:
            obj.decompress_batch(self.fmt, *args, stream=stream)
        else:
            obj.decompress_batch_dict(self.fmt, h.dict, *args, stream=stream)

    def check(self, h):
        res, ain, aout = (x.host(self.name).tolist() for x in (h.res, h.ain, h.aout))
        host = h.out.host(self.name)
        keep = np.ones(len(host), dtype=bool)
        for k, (c, e) in enumerate(zip(self.cases, self.expected)):
            at = h.ooffs[k]
            keep[at:at + c.avail] = False
            assert res[k] == e[0], (self.name, c.name, "result", res[k], e[0])
            if e[0] == SUCCESS:
                assert (ain[k], aout[k]) == (e[1], e[2]), (self.name, c.name, ain[k], aout[k], e[1:3])
                assert host[at:at + e[2]].tobytes() == e[3], (self.name, c.name, "bytes differ")
        assert (host[keep] == CANARY).all(), (self.name, "a byte outside every slot was written")


class Prefix(Step):
    """decompress_prefix_batch: cut, complete and broken streams"""
    family, fields = "prefix", "d->tokens, d->scratch"

    def __init__(self, name, fmt, cases, oracle):
        self.name, self.fmt = name, fmt
        self.cases = self.expected = [prefix_expect.expect(oracle, c) for c in cases]

    def validate(self):
        kinds = set()
        for c in self.cases:
            kinds.add(c.want)
            if c.want == PREFIX:
                assert c.data == prefix_expect.zlib_prefix(c.fmt, c.s, c.limit) == c.plain[:c.limit]
            elif c.want == SUCCESS:
                assert c.data == zlib.decompress(c.s, WBITS[c.fmt]) and c.aout == len(c.data)
            else:
                assert prefix_expect.zlib_prefix(c.fmt, c.s, c.limit) is None, c.tag
        assert {SUCCESS, PREFIX, BAD_DATA} <= kinds, kinds

    def prepare(self, torch, obj=None):
        h = Handle()
        n = len(self.cases)
        blob, offs = _pack([c.s for c in self.cases])
        h.data = _stage(torch, h, blob)
        h.in_off, h.in_n = _i64(torch, offs), _i64(torch, [len(c.s) for c in self.cases])
        h.ooffs, pos = [], 0
        for c in self.cases:
            h.ooffs.append(pos)
            pos += c.limit + prefix_expect.GUARD
        h.out = Guarded(torch, pos)
        h.out_off, h.limits = _i64(torch, h.ooffs), _i64(torch, [c.limit for c in self.cases])
        h.res = Guarded(torch, n, torch.int32, UNSET)
        h.ain = Guarded(torch, n, torch.int64, UNSET)
        h.aout = Guarded(torch, n, torch.int64, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.decompress_prefix_batch(self.fmt, h.data, h.in_off, h.in_n, h.out.t, h.out_off,
                                    h.limits, h.res.t, h.aout.t, actual_in=h.ain.t, stream=stream)

    def check(self, h):
        res, ain, aout = (x.host(self.name).tolist() for x in (h.res, h.ain, h.aout))
        host = h.out.host(self.name)
        for k, c in enumerate(self.cases):
            at = h.ooffs[k]
            behind = host[at + c.limit:at + c.limit + prefix_expect.GUARD]
            assert (behind == CANARY).all(), (self.name, c.tag, "bytes behind the limit")
            assert c.want is not None and res[k] == c.want, (self.name, c.tag, res[k], c.want)
            if c.want in (SUCCESS, PREFIX):
                assert aout[k] == c.aout, (self.name, c.tag, aout[k], c.aout)
                assert host[at:at + c.aout].tobytes() == c.data, (self.name, c.tag, "bytes")
                assert ain[k] == (0 if c.want == PREFIX else c.ain), (self.name, c.tag, ain[k])


class Sizes(Step):
    """decompress_sizes_batch with a NULL limit array"""
    family, fields = "sizes", "d->scratch"

    def __init__(self, name, fmt, streams, oracle):
        """streams: (stream, plain or None for a damaged one)"""
        self.name, self.fmt, self.streams = name, fmt, streams
        self.expected = [sizes_expect.expect(oracle, fmt, s, None)[:3] for s, _ in streams]

    def validate(self):
        for (s, plain), e in zip(self.streams, self.expected):
            if plain is not None:
                assert e == (SUCCESS, len(s), len(plain))
                assert zlib.decompress(s, WBITS[self.fmt]) == plain
            else:   # (a size query checks no checksum: the model may say SUCCESS where zlib objects)
                try:
                    zlib.decompress(s, WBITS[self.fmt])
                except zlib.error:
                    continue
                raise AssertionError("zlib reads a damaged stream")
        assert any(p is None for _, p in self.streams)

    def prepare(self, torch, obj=None):
        h = Handle()
        n = len(self.streams)
        blob, offs = _pack([s for s, _ in self.streams])
        h.data = _stage(torch, h, blob)
        h.in_off, h.in_n = _i64(torch, offs), _i64(torch, [len(s) for s, _ in self.streams])
        h.res = Guarded(torch, n, torch.int32, UNSET)
        h.ain = Guarded(torch, n, torch.int64, UNSET)
        h.size = Guarded(torch, n, torch.int64, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.decompress_sizes_batch(self.fmt, h.data, h.in_off, h.in_n, h.res.t, h.size.t,
                                   actual_in=h.ain.t, stream=stream)

    def check(self, h):
        got = list(zip(*(x.host(self.name).tolist() for x in (h.res, h.ain, h.size))))
        bad = [(k, g, e) for k, (g, e) in enumerate(zip(got, self.expected)) if tuple(g) != tuple(e)]
        assert not bad, (self.name, bad[:6])


class Packed(Step):
    """decompress_batch_packed of valid streams: offsets are the aligned
    prefix sums of the sizes"""
    family, fields = "packed", "d->tokens, d->scratch"
    ALIGN = 16

    def __init__(self, name, fmt, cases, oracle):
        self.name, self.fmt, self.cases = name, fmt, cases
        self.expected = [oracle.decompress_ex(fmt, c.data, len(c.out)) for c in cases]
        self.offs, at = [], 0
        for c in cases:
            self.offs.append(at)
            at += -(-len(c.out) // self.ALIGN) * self.ALIGN
        self.offs.append(at)

    def validate(self):
        for c, e in zip(self.cases, self.expected):
            assert e == (SUCCESS, len(c.data), len(c.out), c.out), c.name
            assert zlib.decompress(c.data, WBITS[self.fmt]) == c.out, c.name

    def prepare(self, torch, obj=None):
        h = Handle()
        n = len(self.cases)
        blob, offs = _pack([c.data for c in self.cases])
        h.data = _stage(torch, h, blob)
        h.in_off, h.in_n = _i64(torch, offs), _i64(torch, [len(c.data) for c in self.cases])
        h.out = Guarded(torch, self.offs[-1])
        h.off = Guarded(torch, n + 1, torch.int64, UNSET)
        h.res = Guarded(torch, n, torch.int32, UNSET)
        h.ain = Guarded(torch, n, torch.int64, UNSET)
        h.aout = Guarded(torch, n, torch.int64, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.decompress_batch_packed(self.fmt, h.data, h.in_off, h.in_n, h.out.t, h.off.t, h.res.t,
                                    h.aout.t, actual_in=h.ain.t, out_align=self.ALIGN,
                                    out_capacity=self.offs[-1], stream=stream)

    def check(self, h):
        assert h.off.host(self.name).tolist() == self.offs, self.name
        assert not h.res.host(self.name).any(), self.name
        assert h.ain.host(self.name).tolist() == [e[1] for e in self.expected], self.name
        assert h.aout.host(self.name).tolist() == [e[2] for e in self.expected], self.name
        want = _image(self.offs[-1], [(o, c.out) for o, c in zip(self.offs, self.cases)])
        _same(h.out.host(self.name), want, self.name)


# ============================================================ archives: readers

class _Archive(Step):
    """what the ZIP and the tar reader share: five words, index rows, per-entry
    results and the output image against the model's Result"""
    BEHIND = b""
    free_failed = False     # a failed entry's slot may hold anything (ZIP: its decode ran)

    def _tensors(self, torch, h, avail):
        m = self.max
        h.d_in = _stage(torch, h, self.data, self.BEHIND)
        h.out = Guarded(torch, avail)
        h.res = Guarded(torch, 5, torch.int64, UNSET)
        h.idx = Guarded(torch, 8 * m, torch.int64, -1)
        h.per = Guarded(torch, m, torch.int32, UNSET)
        h.ires = Guarded(torch, 5, torch.int64, UNSET)
        h.iidx = Guarded(torch, 8 * m, torch.int64, -1)
        h.iper = Guarded(torch, m, torch.int32, UNSET)

    def _against(self, model, res, idx, per, out, pre=None):
        name = self.name
        words = [int(x) for x in res.host(name)]
        assert words == model.words, (name, words, model.words)
        rows, results = idx.host(name).reshape(-1, 8), per.host(name)
        if model.rows is None:
            assert (rows == -1).all() and (results == UNSET).all(), (name, "rows of a refused archive")
            m = 0
        else:
            m = len(model.rows)
            assert rows[:m].tolist() == model.rows and (rows[m:] == -1).all(), (name, "rows")
            assert results[:m].tolist() == model.results, (name, "results")
            assert (results[m:] == UNSET).all(), (name, "results past the entries")
        if out is None:
            return
        host = out.host(name)
        pieces, free = [], []
        for k in range(m if model.plain is not None else 0):
            row = model.rows[k]
            if model.plain[k] is not None:
                pieces.append((row[7], model.plain[k]))
            elif self.free_failed and pre.results[k] == SUCCESS:
                free.append((row[7], row[6]))
        _same(host, _image(len(host), pieces), name, free)


class Zip(_Archive):
    """index_zip_batch, then decompress_zip_batch, into exactly the room"""
    family, fields = "zip", "d->bgzf, d->bgzf_up, d->tokens"
    BEHIND = b"PK\5\6" + b"\0" * 18
    free_failed = True

    def __init__(self, name, data, max_entries, twin=None, room=None):
        """twin: (infolist, datas) of zipfile for a good archive"""
        self.name, self.data, self.max, self.twin = name, data, max_entries, twin
        self.expected = zip_walk.read(data, max_entries, out_avail=room)
        self.index = zip_walk.read(data, max_entries, decode=False)
        self.room = self.expected.words[3] if room is None else room

    def validate(self):
        if self.twin is not None:
            infos, datas = self.twin
            assert self.expected.words[:2] == [SUCCESS, len(infos)] and self.expected.plain == datas
            for row, zi in zip(self.expected.rows, infos):
                assert (row[3], row[6]) == (zi.CRC, zi.file_size)
        else:
            assert self.expected.words[0] != SUCCESS, self.name

    def prepare(self, torch, obj=None):
        h = Handle()
        self._tensors(torch, h, self.room)
        return h

    def enqueue(self, obj, h, stream):
        n = len(self.data)
        obj.index_zip_batch(h.d_in, self.max, h.ires.t, h.iper.t, index=h.iidx.t, stream=stream,
                            in_nbytes=n)
        obj.decompress_zip_batch(h.d_in, self.max, h.out.t, h.res.t, h.per.t, index=h.idx.t,
                                 stream=stream, in_nbytes=n, out_avail=self.room)

    def check(self, h):
        self._against(self.index, h.ires, h.iidx, h.iper, None)
        self._against(self.expected, h.res, h.idx, h.per, h.out, self.index)


class _Selection(Step):
    """read_zip_batch / read_zip_large / read_tar_batch through host rows that
    come from the model, not from an earlier call"""
    BEHIND = b""
    call = ""
    kw = {}

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.data, self.BEHIND)
        h.out = Guarded(torch, self.offs[-1])
        h.per = Guarded(torch, max(len(self.sel), 1), torch.int32, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        h.offs = getattr(obj, self.call)(h.d_in, self.rows, self.sel, h.out.t, h.per.t,
                                         stream=stream, in_nbytes=len(self.data),
                                         out_avail=self.offs[-1], **self.kw)

    def check(self, h):
        assert h.offs.tolist() == self.offs, (self.name, h.offs.tolist())
        assert h.per.host(self.name)[:len(self.sel)].tolist() == self.results, self.name
        pieces = [(o, b) for o, b in zip(self.offs, self.plain) if b is not None]
        free = [(o, int(self.rows[k][6])) for o, b, k, r in
                zip(self.offs, self.plain, self.sel, self.results) if b is None and self.free_failed]
        _same(h.out.host(self.name), _image(self.offs[-1], pieces), self.name, free)


class ZipRead(_Selection):
    family, fields, call = "zip", "d->bgzf, d->bgzf_up, d->tokens", "read_zip_batch"
    BEHIND = Zip.BEHIND
    free_failed = True

    def __init__(self, name, data, rows, sel, datas):
        """datas: zipfile's bytes per entry (None for an entry the archive's
        defect is in)"""
        self.name, self.data, self.rows, self.sel, self.datas = name, data, rows, list(sel), datas
        self.offs, self.results, self.plain = zip_walk.read_selection(data, rows, self.sel)
        self.expected = (self.offs, self.results, self.plain)

    def validate(self):
        for k, r, b in zip(self.sel, self.results, self.plain):
            if self.datas[k] is not None:
                assert r == SUCCESS and b == self.datas[k], (self.name, k)
            else:
                assert r != SUCCESS, (self.name, k)


class ZipLarge(ZipRead):
    """read_zip_large: one deflated entry above large_min goes many-wave, one
    stored entry above binding.ZIP_PIECE is copied and checksummed in pieces"""
    family, call, blocking = "zip-large", "read_zip_large", True
    fields = "d->bgzf, d->bgzf_up, d->tokens, s_copy, s_run"

    def __init__(self, name, data, rows, sel, datas, large_min):
        ZipRead.__init__(self, name, data, rows, sel, datas)
        self.kw = {"large_min": large_min}
        self.large_min = large_min

    def validate(self):
        ZipRead.validate(self)
        rows = [self.rows[k] for k in self.sel]
        assert any(r[2] & 0xFFFF == 8 and r[5] >= self.large_min for r in rows), "no many-wave entry"
        assert any(r[2] & 0xFFFF == 8 and 0 < r[5] < self.large_min for r in rows), "no batch entry"
        assert any(r[2] & 0xFFFF == 0 and r[6] > zl.PIECE for r in rows), "no pieced entry"


class Tar(_Archive):
    """index_tar_batch, then extract_tar_batch, into exactly the room"""
    family, fields = "tar", "d->bgzf, d->bgzf_up"
    BEHIND = tf.member(b"behind", b"never read")

    def __init__(self, name, data, max_records, twin=None, room=None):
        """twin: tar_files.expected() of a file tarfile reads"""
        self.name, self.data, self.max, self.twin = name, data, max_records, twin
        self.expected = tar_walk.read(data, max_records, out_avail=room)
        self.index = tar_walk.read(data, max_records, extract=False)
        self.room = self.expected.words[3] if room is None else room

    def validate(self):
        if self.twin is not None:
            assert self.expected.words[:2] == [SUCCESS, len(self.twin)]
            for (ti, data), row, b in zip(self.twin, self.expected.rows, self.expected.plain):
                assert row[4] == ti.offset_data
                assert data is None or b == data, ti.name
        else:
            assert self.expected.words[0] != SUCCESS, self.name

    def prepare(self, torch, obj=None):
        h = Handle()
        self._tensors(torch, h, self.room)
        return h

    def enqueue(self, obj, h, stream):
        n = len(self.data)
        obj.index_tar_batch(h.d_in, self.max, h.ires.t, h.iper.t, index=h.iidx.t, stream=stream,
                            in_nbytes=n)
        obj.extract_tar_batch(h.d_in, self.max, h.out.t, h.res.t, h.per.t, index=h.idx.t,
                              stream=stream, in_nbytes=n, out_avail=self.room)

    def check(self, h):
        self._against(self.index, h.ires, h.iidx, h.iper, None)
        self._against(self.expected, h.res, h.idx, h.per, h.out)


class TarRead(_Selection):
    family, fields, call = "tar", "d->bgzf, d->bgzf_up", "read_tar_batch"
    BEHIND = Tar.BEHIND
    free_failed = False

    def __init__(self, name, data, rows, sel, twin):
        self.name, self.data, self.rows, self.sel, self.twin = name, data, rows, list(sel), twin
        self.offs, self.results, self.plain = tar_walk.read_selection(data, rows, self.sel)
        self.expected = (self.offs, self.results, self.plain)

    def validate(self):
        for k, r, b in zip(self.sel, self.results, self.plain):
            assert r == SUCCESS and (self.twin[k][1] is None or b == self.twin[k][1]), (self.name, k)


class _Members(Step):
    """decompress_bgzf_batch / decompress_gzip_members_batch with an index"""
    BEHIND = b""
    call = ""

    def __init__(self, name, f, max_members, flags=0):
        self.name, self.f, self.max = name, f, max_members
        self.expected = ([SUCCESS, f.m, len(f.data), len(f.plain), flags], f.plain, f.rows())

    def validate(self):
        f = self.f
        assert gzip.decompress(f.data) == f.plain and f.m <= self.max
        at = 0
        for (off, size, n), row in zip(f.members, f.rows()):
            assert (int(row[0]), int(row[1])) == (off, at) and \
                gzip.decompress(f.data[off:off + size]) == f.plain[at:at + n]
            at += n

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.f.data, self.BEHIND)
        h.out = Guarded(torch, len(self.f.plain))
        h.res = Guarded(torch, 5, torch.int64, UNSET)
        h.idx = Guarded(torch, 2 * (self.max + 1), torch.int64, -1)
        return h

    def enqueue(self, obj, h, stream):
        getattr(obj, self.call)(h.d_in, self.max, h.out.t, h.res.t, index=h.idx.t, stream=stream,
                                in_nbytes=len(self.f.data), out_avail=len(self.f.plain))

    def check(self, h):
        words, plain, rows = self.expected
        assert [int(x) for x in h.res.host(self.name)] == words, (self.name, h.res.host(self.name))
        assert h.out.host(self.name).tobytes() == plain, (self.name, "bytes differ")
        got = h.idx.host(self.name).reshape(-1, 2)
        assert np.array_equal(got[:len(rows)].astype(np.uint64), rows), (self.name, "index")


class Bgzf(_Members):
    family, fields, call = "bgzf", "d->bgzf, d->bgzf_up, d->tokens", "decompress_bgzf_batch"

    def __init__(self, name, f, max_members):
        _Members.__init__(self, name, f, max_members, HAS_EOF if f.has_eof else 0)


class GzipMembers(_Members):
    family, fields = "gzip-members", "d->bgzf, d->bgzf_up, d->tokens"
    call = "decompress_gzip_members_batch"
    BEHIND = b"\x1f\x8b\x08\x00" * 8

    def check(self, h):
        _Members.check(self, h)
        got = h.idx.host(self.name).reshape(-1, 2)
        assert (got[self.f.m + 1:] == -1).all(), (self.name, "index rows past the members")


class BgzfRead(Step):
    """read_bgzf_batch through the rows recorded while the file was built"""
    family, fields = "bgzf", "d->bgzf, d->bgzf_up, d->tokens"

    def __init__(self, name, f, ranges):
        self.name, self.f, self.ranges = name, f, [(int(b), int(n)) for b, n in ranges]
        self.expected = [f.plain[b:b + n] for b, n in self.ranges]

    def validate(self):
        plain = gzip.decompress(self.f.data)
        assert [plain[b:b + n] for b, n in self.ranges] == self.expected
        assert all(len(e) == n for e, (_, n) in zip(self.expected, self.ranges))

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.f.data)
        h.out = Guarded(torch, sum(n for _, n in self.ranges))
        h.res = Guarded(torch, len(self.ranges), torch.int32, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.read_bgzf_batch(h.d_in, self.f.rows(), np.array(self.ranges, dtype=np.uint64), h.out.t,
                            h.res.t, stream=stream, in_nbytes=len(self.f.data), out_avail=h.out.n)

    def check(self, h):
        assert not h.res.host(self.name).any(), (self.name, h.res.host(self.name))
        assert h.out.host(self.name).tobytes() == b"".join(self.expected), (self.name, "bytes differ")


class GzipMembersPeek(Step):
    """index_gzip_members_batch, then peek_gzip_members_batch through its
    device result and index"""
    family, fields = "gzip-members", "d->bgzf, d->bgzf_up, d->tokens"
    SPARE = 3       # rows beyond the member count: empty and untouched

    def __init__(self, name, f, head):
        self.name, self.f, self.head, self.max = name, f, head, f.m + self.SPARE
        sizes = [n for _, _, n in f.members]
        starts = f.rows()[:, 1].astype(int).tolist()
        self.expected = [(SUCCESS if n <= head else PREFIX, min(n, head), f.plain[u:u + min(n, head)])
                         for n, u in zip(sizes, starts)]

    def validate(self):
        f = self.f
        for (off, size, _), e in zip(f.members, self.expected):
            plain = gzip.decompress(f.data[off:off + size])
            assert e == (SUCCESS if len(plain) <= self.head else PREFIX, len(plain[:self.head]),
                         plain[:self.head])
        assert {e[0] for e in self.expected} == {SUCCESS, PREFIX}

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.f.data, GzipMembers.BEHIND)
        h.result = Guarded(torch, 5, torch.int64, UNSET)
        h.idx = Guarded(torch, 2 * (self.max + 1), torch.int64, -1)
        h.heads = Guarded(torch, self.max * self.head)
        h.sizes = Guarded(torch, self.max, torch.int64, UNSET)
        h.res = Guarded(torch, self.max, torch.int32, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        n = len(self.f.data)
        obj.index_gzip_members_batch(h.d_in, self.max, h.result.t, h.idx.t, stream=stream, in_nbytes=n)
        obj.peek_gzip_members_batch(h.d_in, h.result.t, h.idx.t, self.max, self.head, h.heads.t,
                                    h.sizes.t, h.res.t, stream=stream, in_nbytes=n)

    def check(self, h):
        f, m = self.f, self.f.m
        assert [int(x) for x in h.result.host(self.name)] == [SUCCESS, m, len(f.data), len(f.plain), 0]
        res, sizes = h.res.host(self.name).tolist(), h.sizes.host(self.name).tolist()
        assert list(zip(res[:m], sizes[:m])) == [e[:2] for e in self.expected], self.name
        assert res[m:] == [0] * self.SPARE and sizes[m:] == [0] * self.SPARE, self.name
        want = _image(self.max * self.head, [(k * self.head, e[2]) for k, e in enumerate(self.expected)])
        _same(h.heads.host(self.name), want, self.name)


# ============================================== one large stream, host calls

class Large(Step):
    """decompress_large: BLOCKS; the oracle's result, and its bytes where it
    succeeds"""
    family, blocking = "stream", True
    fields = "d->tokens, d->scratch, s_copy, s_run"

    def __init__(self, name, fmt, z, avail, oracle, plain=None, parallel=None):
        self.name, self.fmt, self.z, self.avail = name, fmt, z, avail
        self.plain, self.parallel = plain, parallel
        self.expected = oracle.decompress_ex(fmt, z, avail)

    def validate(self):
        if self.plain is not None:
            assert self.expected == (SUCCESS, len(self.z), len(self.plain), self.plain)
            assert zlib.decompress(self.z, WBITS[self.fmt]) == self.plain
        else:
            assert self.expected[0] != SUCCESS
            try:
                zlib.decompress(self.z, WBITS[self.fmt])
            except zlib.error:
                pass
            else:
                raise AssertionError("zlib reads the damaged stream")

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.z, b"\xee\xdd\xcc")
        h.out = Guarded(torch, self.avail)
        return h

    def enqueue(self, obj, h, stream):
        from libdeflate_amd import binding
        h.got = obj.decompress_large(self.fmt, h.d_in, h.out.t, in_nbytes=len(self.z),
                                     out_avail=self.avail, stream=stream)
        h.stats = binding.stream_stats()

    def check(self, h):
        e = self.expected
        host = h.out.host(self.name)
        assert h.got[0] == e[0], (self.name, h.got, e[:3], h.stats)
        if e[0] == SUCCESS:
            assert h.got == e[:3], (self.name, h.got, e[:3])
            assert host[:e[2]].tobytes() == e[3], (self.name, "bytes differ")
        if self.parallel is not None:
            assert h.stats["parallel"] == self.parallel, (self.name, h.stats)


class LargeIndex(Large):
    """decompress_large_index: decompress_large's answer, and every window of
    the index against the plain bytes"""
    SPACING, POINTS = 262144, 16

    def enqueue(self, obj, h, stream):
        r = obj.decompress_large_index(self.fmt, h.d_in, h.out.t, self.SPACING, self.POINTS,
                                       in_nbytes=len(self.z), out_avail=self.avail, stream=stream)
        h.got, h.rows, h.windows, h.stats = r[:3], r[3], r[4], None

    def check(self, h):
        from libdeflate_amd import binding
        Large.check(self, h)
        rows, win, n = h.rows, binding.SEEK_WINDOW, len(self.plain)
        npts = len(rows) - 2
        assert int(rows[0, 3]) == npts >= 2 and int(rows[-1, 0]) == n, (self.name, rows)
        assert h.windows.numel() == npts * win
        wins = h.windows.cpu().numpy().tobytes()
        for k, off in enumerate(int(v) for v in rows[1:-1, 0]):
            have = min(off, win)
            assert wins[k * win:(k + 1) * win] == bytes(win - have) + self.plain[off - have:off], \
                (self.name, "window", k, off)


class SeekRead(LargeIndex):
    """seek_read_batch through the index decompress_large_index has just
    made on the same object (the index is the call's input, not its
    expectation: that is the plain bytes' slices)"""
    family = "seek"

    def __init__(self, name, fmt, z, plain, ranges, oracle):
        LargeIndex.__init__(self, name, fmt, z, len(plain), oracle, plain)
        self.ranges = list(ranges)
        self.slices = [plain[b:b + n] for b, n in self.ranges]

    def validate(self):
        LargeIndex.validate(self)
        assert all(len(s) == n for s, (_, n) in zip(self.slices, self.ranges))

    def prepare(self, torch, obj=None):
        h = LargeIndex.prepare(self, torch, obj)
        h.sub = Guarded(torch, sum(n for _, n in self.ranges))
        h.sres = Guarded(torch, len(self.ranges), torch.int32, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        LargeIndex.enqueue(self, obj, h, stream)
        assert h.got[0] == SUCCESS, (self.name, h.got)
        obj.seek_read_batch(h.d_in, h.rows, h.windows, self.ranges, h.sub.t, h.sres.t, stream=stream,
                            in_nbytes=len(self.z), out_avail=h.sub.n)

    def check(self, h):
        LargeIndex.check(self, h)
        assert not h.sres.host(self.name).any(), (self.name, h.sres.host(self.name))
        assert h.sub.host(self.name).tobytes() == b"".join(self.slices), (self.name, "bytes differ")


class BatchHost(Step):
    """decompress_batch_host: BLOCKS"""
    family, blocking, fields = "host", True, "d->tokens, d->scratch, pinned slices"

    def __init__(self, name, fmt, cases, oracle):
        self.name, self.fmt, self.cases = name, fmt, cases
        self.expected = [oracle.decompress_ex(fmt, c.data, len(c.out)) for c in cases]

    validate = Packed.validate

    def prepare(self, torch, obj=None):
        return Handle()

    def enqueue(self, obj, h, stream):
        h.got = obj.decompress_batch_host(self.fmt, [c.data for c in self.cases],
                                          [len(c.out) for c in self.cases])

    def check(self, h):
        bad = [k for k, (g, e) in enumerate(zip(h.got, self.expected)) if tuple(g) != tuple(e)]
        assert not bad, (self.name, bad[:8])


class ExHost(Step):
    """decompress_ex on one host buffer: BLOCKS"""
    family, blocking, fields = "host", True, "d->tokens, d->scratch, pinned slices"

    def __init__(self, name, fmt, z, plain, oracle):
        self.name, self.fmt, self.z, self.plain = name, fmt, z, plain
        self.expected = oracle.decompress_ex(fmt, z, len(plain))

    def validate(self):
        assert self.expected == (SUCCESS, len(self.z), len(self.plain), self.plain)
        assert zlib.decompress(self.z, WBITS[self.fmt]) == self.plain

    def prepare(self, torch, obj=None):
        return Handle()

    def enqueue(self, obj, h, stream):
        h.got = obj.decompress_ex(self.fmt, self.z, len(self.plain))

    def check(self, h):
        assert h.got[:3] == self.expected[:3] and h.got[3] == self.expected[3], (self.name, h.got[:3])


class Refused(Step):
    """a call that is refused before any device work: it raises with the
    call's name, and its outputs stay as they were"""
    family, fields = "refused", "-"

    def __init__(self, name, base, call, **kw):
        """base: a _Selection step; kw overrides its arguments (sel included)"""
        self.name, self.base, self.call, self.kw = name, base, call, kw
        self.expected = "RuntimeError"

    def validate(self):
        rows, kw = self.base.rows, self.kw
        sel = kw.get("sel", self.base.sel)
        assert any(k >= len(rows) for k in sel) or "out_avail" in kw or "in_nbytes" in kw

    def prepare(self, torch, obj=None):
        return self.base.prepare(torch, obj)

    def enqueue(self, obj, h, stream):
        b, kw = self.base, dict(self.kw)
        sel = kw.pop("sel", b.sel)
        args = {"in_nbytes": len(b.data), "out_avail": b.offs[-1], **b.kw, **kw}
        h.error = None
        try:
            getattr(obj, self.call)(h.d_in, b.rows, sel, h.out.t, h.per.t, stream=stream, **args)
        except RuntimeError as e:
            h.error = str(e)

    def check(self, h):
        call = {"read_zip_batch": "zip_read_batch", "read_tar_batch": "tar_read_batch",
                "read_zip_large": "zip_read_large"}[self.call]
        assert h.error is not None and call in h.error, (self.name, h.error)
        assert (h.out.host(self.name) == CANARY).all(), (self.name, "d_out was written")
        assert (h.per.host(self.name) == UNSET).all(), (self.name, "d_results was written")


# ============================================================ the decompressor

def text_stream(fmt, n, seed, level=6):
    data = datagen.text_chunk(n, seed)
    co = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    return co.compress(data) + co.flush(), data


def damaged(z, seed):
    """64 bytes in the middle overwritten"""
    b = bytearray(z)
    at = len(b) // 2
    b[at:at + 64] = random.Random(seed).randbytes(64)
    return bytes(b)


def synth_cases():
    """the short, invalid and damaged raw cases of deflate_synth.corpus() that
    decode in under 70 000 bytes, and every third valid one a byte short"""
    small = [c for c in S.corpus() if c.fmt == "deflate" and c.avail < 70000]
    short = [S.Case(c.name + "-short", c.fmt, c.data, None, c.tags, avail=len(c.out) - 1)
             for c in small[::3] if c.valid and len(c.out)]
    out = []
    for i, c in enumerate(small):
        out.append(c)
        if i % 3 == 0 and short:
            out.append(short.pop())
    return out


def _prefix_cases():
    out = []
    for k, n in enumerate((5000, 70000, 300)):
        z, plain = text_stream("gzip", n, 0x9F00 + k)
        out.append(prefix_expect.Case("gzip", z, n // 3 + k, f"cut{k}", plain=plain))
        out.append(prefix_expect.Case("gzip", z, n + 7 * k, f"whole{k}", plain=plain))
    z, plain = text_stream("gzip", 20000, 0x9F10)
    b = bytearray(z)
    b[10] |= 6      # BTYPE 3 in the first block header
    out.append(prefix_expect.Case("gzip", bytes(b), 100, "broken"))
    return out


def _sizes_streams():
    out = [(c.data, c.out) for c in zcases("zlib", 36, 1, 100000, 0x512E)]
    z = out[5][0]
    out += [(z[:len(z) // 2], None), (z[:-1], None), (damaged(out[20][0], 3), None),
            (b"\x78\x9c", None)]
    return out


_steps = {}


def decompressor_steps(oracle):
    """name -> Step; built once per process"""
    if "d" in _steps:
        return _steps["d"]
    st = {}

    def add(s):
        assert s.name not in st
        st[s.name] = s
    add(Batch("batch300", "gzip", zcases("gzip", 300, 1024, 65536, 0xB300), oracle))
    add(Batch("batch2", "zlib", zcases("zlib", 2, 1024, 65536, 0xB002), oracle))
    add(Batch("batch1", "deflate", zcases("deflate", 1, 1024, 65536, 0xB001), oracle))
    add(Batch("batch-synth", "deflate", synth_cases(), oracle))
    shorts = [S.Case(c.name + "-short", c.fmt, c.data, None, (), avail=len(c.out) - 1 - k)
              for k, c in enumerate(zcases("gzip", 12, 1024, 65536, 0xB300))]
    add(Batch("batch-short", "gzip", shorts[:6] + zcases("gzip", 6, 1024, 65536, 0xB300) + shorts[6:],
              oracle))
    for n in (1, 4, 600, 2500):    # (D4: each larger than what the object has seen)
        add(Batch(f"batch-small{n}", "zlib", zcases("zlib", n, 1024, 4096, 0xB400), oracle))
    dicts = S.dict_cases()
    d = next(c.dictionary for c in dicts if len(c.dictionary) == 1000)
    for fmt in ("deflate", "zlib"):
        add(Batch(f"dict-{fmt}", fmt, [c for c in dicts if c.dictionary == d and c.fmt == fmt],
                  oracle, dictionary=d))
    add(Prefix("prefix", "gzip", _prefix_cases(), oracle))
    add(Sizes("sizes", "zlib", _sizes_streams(), oracle))
    add(Packed("packed", "gzip", zcases("gzip", 30, 1, 40000, 0xBAC0), oracle))

    g = zf.good("zip64")
    infos, datas = zf.expected(g)
    add(Zip("zip", g.data, len(infos), (infos, datas)))
    rows = zip_walk.read(g.data, len(infos), decode=False).rows
    zread = ZipRead("zip-read", g.data, rows, [3, 0, 3, 6, 1, 2], datas)
    add(zread)
    g = zf.good("false")
    add(Zip("zip-false", g.data, len(zf.expected(g)[0]), zf.expected(g)))
    d = {x.name: x for x in zf.defects()}["deflate_byte"]
    infos, datas = zf.expected(d.base)
    add(Zip("zip-defect", d.data, len(infos) + 1))
    rows = zip_walk.read(d.data, len(infos), decode=False).rows
    add(ZipRead("zip-read-defect", d.data, rows, [0, d.entry, 5, 4],
                [None if k == d.entry else b for k, b in enumerate(datas)]))
    add(Zip("zip-overflow", zf.lookalikes().data, 1))
    g = zf.good("zip64")
    add(Zip("zip-space", g.data, 7, room=zip_walk.read(g.data, 7).words[3] - 1))    # a byte short
    for n in (8, 3000):     # (D4: index_zip_batch's scratch follows max_entries)
        g = zf.good("zip64")
        add(Zip(f"zip-max{n}", g.data, n, zf.expected(g)))
    a = zl.archive()
    # (large_min is the call's argument; the piece size is the library's constant
    # binding.ZIP_PIECE = 1 MiB, so the pieced path is reached by choosing an
    # entry above it - stored2m+1 - and validate() asserts that one is there)
    sel = [zl.entry(x) for x in ("small0", "text1m", "small1", "stored2m+1", "small3")]
    zlarge = ZipLarge("zip-large", a.data, zl.rows_of(a), sel, a.datas, large_min=200000)
    add(zlarge)

    g = tf.tiles()
    m = len(tar_walk.walk(g.data).records)
    add(Tar("tar", g.data, m, tf.expected(g)))
    rows = tar_walk.read(g.data, m, extract=False).rows
    tread = TarRead("tar-read", g.data, rows, [5, 2, 7, 1, 1, 0], tf.expected(g))
    add(tread)
    g = tf.good("mixed_pax")
    add(Tar("tar-pax", g.data, len(tar_walk.walk(g.data).records), tf.expected(g)))
    add(Tar("tar-defect", tf.defects()[0].data, 64, room=1 << 16))
    add(Tar("tar-overflow", tf.nested_big().data, 2, room=100))

    f = bgzf_files.cut_file(300000, 0xB62F)
    add(Bgzf("bgzf", f, f.m + 1))
    u = f.rows()[:, 1].astype(int).tolist()
    add(BgzfRead("bgzf-read", f, [(u[2] + 10, 100), (u[3], u[4] - u[3]), (u[1] + 1, u[5] - u[1]),
                                   (len(f.plain) - 1, 1), (7, 0), (0, 70000)]))
    e, false = bgzf_files.adversarial("e")
    assert e.m + false > 4 * (e.m + 1) + 1024       # the walk runs inside the call
    add(Bgzf("bgzf-walk", e, e.m + 1))
    f4 = bgzf_files.plain_file(2 * B + 100, 0xB630)
    assert f4.m == 4
    for n in (4, 4000):     # (D4)
        add(Bgzf(f"bgzf-max{n}", f4, n))

    add(GzipMembers("gzm", gf.flagged(), gf.flagged().m))
    add(GzipMembers("gzm-mixed", gf.mixed(40), 40))
    add(GzipMembers("gzm-false", gf.false_candidates("pair"), gf.false_candidates("pair").m))
    add(GzipMembersPeek("gzm-peek", gf.empties(), 1000))

    z, plain = text_stream("gzip", 2 << 20, 0x1A26E)
    add(Large("large", "gzip", z, len(plain), oracle, plain, parallel=1))
    add(Large("large-damaged", "gzip", damaged(z, 5), len(plain), oracle))
    z1, plain1 = text_stream("zlib", 1 << 20, 0x1A26F)
    add(LargeIndex("large-index", "zlib", z1, len(plain1), oracle, plain1))
    n = len(plain1)
    add(SeekRead("seek-read", "zlib", z1, plain1,
                 [(5, 1000), (n // 2 - 3, 70000), (n - 10, 10), (7, 0), (300000, 1)], oracle))
    add(BatchHost("batch-host", "gzip", zcases("gzip", 64, 4096, 4096, 0xB064), oracle))
    add(ExHost("ex-host", "gzip", *text_stream("gzip", 1 << 20, 0x1A270), oracle))

    # refused before any device work, with the arguments of the existing
    # test_read_refuses_before_any_device_work tests
    zr = zread.rows
    add(Refused("refused-zip-space", zread, "read_zip_batch", sel=[1], out_avail=int(zr[1][6]) - 1))
    add(Refused("refused-zip-input", zread, "read_zip_batch", sel=[1], in_nbytes=int(zr[1][4])))
    add(Refused("refused-zip-row", zread, "read_zip_batch", sel=[len(zr)]))
    tr = tread.rows
    add(Refused("refused-tar-space", tread, "read_tar_batch", sel=[7], out_avail=16))
    add(Refused("refused-tar-input", tread, "read_tar_batch", sel=[7], in_nbytes=int(tr[7][4]) + 16))
    add(Refused("refused-tar-row", tread, "read_tar_batch", sel=[8]))
    add(Refused("refused-zip-large-row", zlarge, "read_zip_large", sel=[len(zlarge.rows)]))
    _steps["d"] = st
    return st


# ===================================== the PNG decodes and the shuffled chunks

UNSUPPORTED = 18


class PngDecode(_Selection):
    """decode_png_batch / decode_png_pixels_batch / decode_png_batch_ex through
    host rows that come from the models' index, not from an index call.  The
    plain calls' rows are indexed without PNG_ADAM7: an interlaced file is a
    zero row to them, UNSUPPORTED and without a room"""
    fields = "d->bgzf, d->bgzf_up, d->tokens"
    free_failed = False
    ALIGN = 16

    def __init__(self, name, family, call, files, sel, fmt=0, flags=0):
        self.name, self.family, self.call, self.files, self.sel = name, family, call, files, list(sel)
        self.fmt, self.flags = fmt, flags
        self.data, at = _pack([f.data for f in files])
        self.rows = [p7m.index(self.data, o, len(f.data), flags & p7m.ADAM7)[1]
                     for o, f in zip(at, files)]
        self.kw = {"out_align": self.ALIGN, "flags": flags}
        if call != "decode_png_batch":
            self.kw["fmt"] = fmt
        self.offs = p7m.out_sizes(self.rows, self.sel, fmt, self.ALIGN)
        got = [p7m.decode(self.data, self.rows[k], flags, fmt) for k in self.sel]
        self.results, self.plain = [r for r, _ in got], [b for _, b in got]
        self.expected = (self.offs, self.results, self.plain)

    def validate(self):
        """against the pixels the files were built from, through the model of
        the call's own layout"""
        for k, r, b in zip(self.sel, self.results, self.plain):
            f, row = self.files[k], self.rows[k]
            if pm.is_zero(row):
                assert (r, b) == (UNSUPPORTED, None), (self.name, k)
                continue
            assert r == SUCCESS, (self.name, k, r)
            if not self.fmt:
                le = self.flags & pm.LE16 and f.depth == 16
                assert b == (pm.swap16(f.pixels) if le else f.pixels), (self.name, k)
            else:
                plte, trns = px.chunks_of(self.data, row)
                want = px.convert(f.pixels, f.width, f.height, f.depth, f.colour, self.fmt, plte,
                                  trns, self.flags & pm.LE16)
                assert want == (SUCCESS, b), (self.name, k)
            if not p7m.is_interlaced(row):     # the older models say the same
                older = px.decode(self.data, row, self.fmt, self.flags & pm.LE16) if self.fmt else \
                    pm.decode(self.data, row, self.flags & pm.LE16)
                assert older == (r, b), (self.name, k)


class ShuffleRead(Step):
    """decompress_shuffle_batch: the stored chunks at odd offsets with junk
    between them, the rooms at odd offsets with gaps between them"""
    family, fields = "shuffle", "d->bgzf, d->bgzf_up, d->tokens"

    def __init__(self, name, fmt, chunks):
        """chunks: (element size, raw bytes, mask)"""
        self.name, self.fmt, self.chunks = name, fmt, chunks
        buf, rows, at = bytearray(), [], 0
        for k, (es, n, mask) in enumerate(chunks):
            raw = shuffle_chunks.raw_bytes(es, n)
            stored = sm.stored(raw, es, mask, lambda b: _deflate(fmt, b))
            buf += bytes([0x78, 0x9C, k][:1 + k % 3])
            at += k % 4
            rows.append([len(buf), len(stored), at, n, es, mask])
            buf += stored
            at += n
        self.data, self.rows, self.total = bytes(buf), rows, at
        self.expected = [(r[2], shuffle_chunks.raw_bytes(r[4], r[3])) for r in rows]

    def validate(self):
        """zlib and the model's inverse transform give the rooms' bytes"""
        for r, (off, raw) in zip(self.rows, self.expected):
            body = self.data[r[0]:r[0] + r[1]]
            if not r[5] & sm.NO_DEFLATE:
                body = _inflate(self.fmt, body)
            if not sm.identity(r[3], r[4], r[5]):
                body = sm.unshuffle(body, r[4])
            assert bytes(body) == raw and len(raw) == r[3], (self.name, r)

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.data, b"\x78\x9c" * 5)
        h.out = Guarded(torch, self.total)
        h.per = Guarded(torch, len(self.rows), torch.int32, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.decompress_shuffle_batch(self.fmt, self.rows, h.d_in, h.out.t, h.per.t, stream=stream,
                                     in_nbytes=len(self.data), out_avail=self.total)

    def check(self, h):
        assert not h.per.host(self.name).any(), (self.name, h.per.host(self.name))
        _same(h.out.host(self.name), _image(self.total, self.expected), self.name)


class RefusedReader(Refused):
    """Refused for the PNG decodes (an unknown flag bit) and the shuffle read
    (an element size of 0)"""

    def __init__(self, name, base, **kw):
        self.name, self.base, self.kw = name, base, kw
        self.expected = "RuntimeError"

    def validate(self):
        if isinstance(self.base, ShuffleRead):
            assert sm.row_why(self.rows()[self.kw["row"]], True, len(self.base.data),
                              self.base.total) == "element size"
        else:
            assert self.kw["flags"] & ~(pm.LE16 | p7m.ADAM7)

    def rows(self):
        rows = [list(r) for r in self.base.rows]
        rows[self.kw["row"]][4] = 0
        return rows

    def enqueue(self, obj, h, stream):
        b = self.base
        h.error = None
        try:
            if isinstance(b, ShuffleRead):
                obj.decompress_shuffle_batch(b.fmt, self.rows(), h.d_in, h.out.t, h.per.t,
                                             stream=stream, in_nbytes=len(b.data), out_avail=b.total)
            else:
                getattr(obj, b.call)(h.d_in, b.rows, b.sel, h.out.t, h.per.t, stream=stream,
                                     in_nbytes=len(b.data), out_avail=b.offs[-1],
                                     **{**b.kw, **self.kw})
        except RuntimeError as e:
            h.error = str(e)

    def check(self, h):
        call = "shuffle_decompress_batch" if isinstance(self.base, ShuffleRead) else \
            {"decode_png_batch": "png_decode_batch", "decode_png_pixels_batch": "png_decode_pixels_batch",
             "decode_png_batch_ex": "png_decode_batch_ex"}[self.base.call]
        assert h.error is not None and call in h.error, (self.name, h.error)
        assert (h.out.host(self.name) == CANARY).all(), (self.name, "d_out was written")
        assert (h.per.host(self.name) == UNSET).all(), (self.name, "d_results was written")


def png_files():
    """seven files of at most 64 x 64: a palette with tRNS, 16-bit RGBA, one
    pixel wide, interlaced and three pixels wide (passes 2, 4 and 6 absent), the
    largest, 8-bit RGBA (what the pixel format of the steps is), interlaced
    16-bit grey"""
    return [pf.make(33, 17, depth=4, colour=3, trns=bytes(range(0, 160, 10)), seed=0x91),
            pf.make(20, 9, depth=16, colour=6, seed=0x92),
            pf.make(1, 40, depth=8, colour=2, seed=0x93),
            p7.make7(3, 5, depth=8, colour=2, seed=0x94),
            pf.make(64, 64, depth=8, colour=2, seed=0x95),
            pf.make(7, 5, depth=8, colour=6, seed=0x96),
            p7.make7(19, 10, depth=16, colour=0, seed=0x97)]


def shuffle_shapes():
    """(element size, raw bytes, mask): a full tile and a part of one, bytes
    behind the last element, element sizes that do not divide the tile (3,
    255), every class of the reader's plan"""
    return [(4, 4 * 4096 + 4 * 17, 0), (8, 2059, 0), (3, 3001, 0), (2, 1000, sm.NO_SHUFFLE),
            (4, 2048, sm.NO_DEFLATE), (1, 500, 0), (5, 0, 0), (255, 255 * 20 + 7, 0),
            (16, 700, sm.NO_DEFLATE | sm.NO_SHUFFLE)]


def reader_steps():
    """name -> Step of the PNG decodes and the shuffle read; a catalogue of its
    own, so that the seeded shuffles of the older one draw what they always
    drew.  Built once per process"""
    if "r" in _steps:
        return _steps["r"]
    st = {}

    def add(s):
        assert s.name not in st
        st[s.name] = s
    files = png_files()
    png = PngDecode("png", "png", "decode_png_batch", files, [4, 0, 2, 3, 1, 5, 0], flags=pm.LE16)
    add(png)
    add(PngDecode("png-zero", "png", "decode_png_batch", files, [3, 6]))
    pixels = PngDecode("png-pixels", "png-pixels", "decode_png_pixels_batch", files,
                       [0, 5, 1, 4, 6, 2, 5], fmt=px.RGBA)
    add(pixels)
    ex = PngDecode("png-ex", "png-adam7", "decode_png_batch_ex", files, [3, 0, 6, 1, 3, 5, 2],
                   fmt=px.RGBA, flags=p7m.ADAM7)
    add(ex)
    add(PngDecode("png-ex-raw", "png-adam7", "decode_png_batch_ex", files, [6, 2, 3, 1],
                  flags=p7m.ADAM7 | pm.LE16))
    shuf = ShuffleRead("shuffle", "zlib", shuffle_shapes())
    add(shuf)
    add(RefusedReader("refused-png", png, flags=0x80))
    add(RefusedReader("refused-png-pixels", pixels, flags=0x80))
    add(RefusedReader("refused-png-ex", ex, flags=0x80 | p7m.ADAM7))
    add(RefusedReader("refused-shuffle", shuf, row=2))
    _steps["r"] = st
    return st


# ================================================================== compressor

class CStep(Step):
    """a compressor step: check() returns the bytes the call wrote, which the
    sequence tests hold against a fresh object's"""


def _inflate(fmt, z, dictionary=None):
    d = zlib.decompressobj(WBITS[fmt], zdict=dictionary) if dictionary else \
        zlib.decompressobj(WBITS[fmt])
    out = d.decompress(z) + d.flush()
    assert d.eof and not d.unused_data, "the stream does not end where its bytes end"
    return out


def _deflate(fmt, data, dictionary=None):
    """zlib's stream of the data: what validate() feeds the CPU decoder of a
    step's check() with, so that the decoder is known to read this input in
    this format (the library's own bytes have no CPU reference)"""
    co = zlib.compressobj(1, zlib.DEFLATED, WBITS[fmt], zdict=dictionary) if dictionary else \
        zlib.compressobj(1, zlib.DEFLATED, WBITS[fmt])
    return co.compress(data) + co.flush()


def _bgzf_by_zlib(data):
    """-> (a BGZF file of the data by zlib, its index rows)"""
    rows, at = [], 0
    for k in range(0, len(data), B):
        rows.append([at, k])
        at += len(bgzf_walk.member(data[k:k + B]))
    return bgzf_walk.build(data), rows + [[at, len(data)]]


def _place(records):
    """the records in one buffer at offsets of their own, with gaps of other
    bytes between them"""
    buf, offs = bytearray(b"\xEE" * 5), []
    for k, r in enumerate(records):
        offs.append(len(buf))
        buf += r + b"\xEE" * (1 + 3 * k % 16)
    return bytes(buf), offs


class CBatch(CStep):
    """compress_batch / compress_batch_dict: every chunk into a slot of its
    bound, 16 guard bytes between the slots"""
    family, fields = "compress", "c->scratch"

    def __init__(self, name, fmt, chunks, max_chunk=None, dictionary=None):
        self.name, self.fmt, self.chunks = name, fmt, chunks
        self.max_chunk, self.dictionary = max_chunk, dictionary
        self.expected = chunks      # what a CPU decoder has to give back
        if dictionary is not None:
            self.family = "compress-dict"

    def validate(self):
        assert self.chunks and all(isinstance(c, bytes) for c in self.chunks)
        assert self.max_chunk is None or max(map(len, self.chunks)) <= self.max_chunk
        for c in self.chunks:
            assert _inflate(self.fmt, _deflate(self.fmt, c, self.dictionary), self.dictionary) == c

    def prepare(self, torch, obj=None):
        h = Handle()
        n = len(self.chunks)
        blob, offs = _pack(self.chunks)
        h.data = _stage(torch, h, blob)
        h.in_off, h.in_n = _i64(torch, offs), _i64(torch, [len(c) for c in self.chunks])
        extra = 4 if self.dictionary is not None else 0
        h.bounds = [obj.bound(self.fmt, len(c)) + extra for c in self.chunks]
        h.ooffs, pos = [], 0
        for b in h.bounds:
            h.ooffs.append(pos)
            pos += b + 16
        h.out = Guarded(torch, pos)
        h.out_off, h.avail = _i64(torch, h.ooffs), _i64(torch, h.bounds)
        h.nb = Guarded(torch, n, torch.int64, UNSET)
        if self.dictionary is not None:
            h.dict = _stage(torch, h, self.dictionary)[:len(self.dictionary)]
        return h

    def enqueue(self, obj, h, stream):
        args = (h.data, h.in_off, h.in_n, h.out.t, h.out_off, h.avail, h.nb.t)
        if self.dictionary is not None:
            obj.compress_batch_dict(self.fmt, h.dict, *args, stream=stream)
        else:
            obj.compress_batch(self.fmt, *args, stream=stream, max_chunk=self.max_chunk)

    def check(self, h):
        nb, host = h.nb.host(self.name).tolist(), h.out.host(self.name)
        got = []
        for k, c in enumerate(self.chunks):
            at = h.ooffs[k]
            assert 0 < nb[k] <= h.bounds[k], (self.name, k, nb[k])
            got.append(host[at:at + nb[k]].tobytes())
            assert _inflate(self.fmt, got[-1], self.dictionary) == c, (self.name, k, "round trip")
            assert (host[at + h.bounds[k]:at + h.bounds[k] + 16] == CANARY).all(), (self.name, k, "gap")
        return got


class _Entries(CStep):
    """what the three writers share: names, entries at offsets of their own"""

    def __init__(self, name, names, entries):
        self.name, self.names, self.entries = name, names, entries
        self.sizes = [len(e) for e in entries]
        self.buf, self.offs = _place(entries)
        self.expected = (names, entries)

    def validate(self):
        assert len(self.names) == len(self.entries) <= 8
        assert None in self.names or len(set(self.names)) == len(self.names)
        for o, e in zip(self.offs, self.entries):
            assert self.buf[o:o + len(e)] == e


class CZip(_Entries):
    family, fields = "zip-write", "c->zipw, c->zipw_up, c->scratch"
    DATETIME = (2024 - 1980) << 25 | 2 << 21 | 29 << 16 | 13 << 11 | 7 << 5 | 9

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.buf)
        h.bound = obj.zip_bound(self.names, self.sizes)
        h.out = Guarded(torch, h.bound)
        h.res = Guarded(torch, 4, torch.int64, UNSET)
        h.idx = Guarded(torch, 8 * len(self.names), torch.int64, -1)
        return h

    def enqueue(self, obj, h, stream):
        obj.compress_zip_batch(self.names, h.d_in, self.offs, self.sizes, h.out.t, h.res.t,
                               index=h.idx.t, dos_datetime=self.DATETIME, stream=stream,
                               in_avail=len(self.buf), out_avail=h.bound)

    def check(self, h):
        words = [int(x) for x in h.res.host(self.name)]
        host = h.out.host(self.name)
        assert words[0] == SUCCESS and 0 < words[1] <= h.bound, (self.name, words)
        got = host[:words[1]].tobytes()
        assert (host[words[1]:] == CANARY).all(), (self.name, "bytes written behind the archive")
        with zipfile.ZipFile(io.BytesIO(got)) as z:
            assert z.testzip() is None
            infos = z.infolist()
            assert [zi.filename.encode("utf-8") for zi in infos] == list(self.names), self.name
            datas = [z.read(zi) for zi in infos]
        assert datas == self.entries, (self.name, "round trip")
        assert all(zi.date_time == (2024, 2, 29, 13, 7, 18) for zi in infos)
        assert words[3] == sum(zi.compress_type == 8 for zi in infos), (self.name, words)
        want = zl.rows_of(zl.Archive(got, infos, datas))
        assert words[2] == want[0][0], (self.name, "cd_off")
        assert h.idx.host(self.name).reshape(-1, 8).tolist() == want, (self.name, "index rows")
        return got


class CGzm(_Entries):
    family, fields = "gzm-write", "c->zipw, c->zipw_up, c->scratch"

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.buf)
        h.bound = obj.gzip_members_compress_bound(self.sizes, self.names)
        h.out = Guarded(torch, h.bound)
        h.res = Guarded(torch, 4, torch.int64, UNSET)
        h.idx = Guarded(torch, 2 * (len(self.names) + 1), torch.int64, -1)
        return h

    def enqueue(self, obj, h, stream):
        obj.gzip_members_compress((h.d_in, self.offs, self.sizes), self.names, 1700000000,
                                  out=h.out.t, result=h.res.t, index=h.idx.t, stream=stream,
                                  in_avail=len(self.buf), out_avail=h.bound)

    def check(self, h):
        n = len(self.entries)
        words = [int(x) for x in h.res.host(self.name)]
        host = h.out.host(self.name)
        assert words[0] == SUCCESS and 0 < words[1] <= h.bound, (self.name, words)
        assert words[2:] == [sum(self.sizes), n], (self.name, words)
        got = host[:words[1]].tobytes()
        assert (host[words[1]:] == CANARY).all(), (self.name, "bytes written behind the file")
        assert gzip.decompress(got) == b"".join(self.entries), (self.name, "round trip")
        # a member walk by zlib: where every member starts, and what it holds
        rows, at, u = [], 0, 0
        for e in self.entries:
            rows.append([at, u])
            d = zlib.decompressobj(31)
            assert d.decompress(got[at:]) + d.flush() == e and d.eof, (self.name, "member")
            at, u = len(got) - len(d.unused_data), u + len(e)
        rows.append([at, u])
        assert at == len(got)
        assert h.idx.host(self.name).reshape(-1, 2).tolist() == rows, (self.name, "index pairs")
        return got


_png_streams = {}


def _png_zlib(level, raws):
    """a fresh object's own libdeflate_zlib_compress() of every image's
    scanlines, the streams the CPU model assembles the files around (as
    tests/test_png_write_gpu.py takes them); once per level"""
    from libdeflate_amd import api
    if level not in _png_streams:
        c = api.Compressor(level)
        _png_streams[level] = [c.compress("zlib", raw) for raw in raws]
        c.close()
    return _png_streams[level]


class CPng(CStep):
    """encode_png_batch: byte for byte the files of the CPU model
    (tools/models/png_write.py) around the object's own zlib streams of the
    model's filtered scanlines, with its result words and index rows"""
    family, fields = "png-write", "c->zipw, c->zipw_up, c->scratch"

    def __init__(self, name, images):
        """images: (width, height, depth, colour, pixels); in one buffer at
        offsets of their own, with other bytes between them"""
        self.name, self.images = name, images
        buf, self.rows = bytearray(b"\xEE" * 3), []
        for k, (w, h, d, c, px) in enumerate(images):
            self.rows.append([len(buf), len(px), w | h << 32, d | c << 8, 0, 0, 0, 0])
            buf += px + b"\xEE" * (1 + 5 * k % 16)
        self.buf = bytes(buf)
        self.raws = [pw.image_scanlines(r, self.buf)[0] for r in self.rows]
        self.expected = self.raws       # what a CPU inflate of every IDAT has to give back

    def validate(self):
        assert [pw.geometry(r)[:4] for r in self.rows] == \
            [(1, 1, 8, 0), (7, 5, 8, 2), (33, 17, 16, 6), (43690, 3, 8, 0)]
        # one call with a whole-entry group and a segmented one: the last
        # image is the first size above the segment rule's edge
        assert [len(raw) for raw in self.raws] == [2, 110, 4505, 131073]
        assert pw.bound(self.rows) > 0
        # the model's scanlines unfilter to the pixels, and its files around
        # zlib's streams are files the reader's model decodes to them
        files = pw.encode(self.rows, self.buf, [zlib.compress(raw) for raw in self.raws])[0]
        for (w, h, d, c, px), row, raw, f in zip(self.images, self.rows, self.raws, files):
            rb, unit = pw.geometry(row)[4:]
            assert pm.unfilter(raw, h, rb, unit) == (True, px), self.name
            assert pm.read(f)[2:] == (SUCCESS, px), self.name

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.buf)
        h.level = obj.level
        h.bound = obj.png_encode_bound(self.rows)
        h.out = Guarded(torch, h.bound)
        h.res = Guarded(torch, 4, torch.int64, UNSET)
        h.idx = Guarded(torch, 8 * len(self.rows), torch.int64, -1)
        return h

    def enqueue(self, obj, h, stream):
        obj.encode_png_batch(self.rows, h.d_in, h.out.t, h.res.t, h.idx.t, stream=stream,
                             in_avail=len(self.buf), out_avail=h.bound)

    def check(self, h):
        words = [int(x) for x in h.res.host(self.name)]
        host = h.out.host(self.name)
        assert words[0] == SUCCESS and 0 < words[1] <= h.bound, (self.name, words)
        got = host[:words[1]].tobytes()
        assert (host[words[1]:] == CANARY).all(), (self.name, "bytes written behind the files")
        rows = h.idx.host(self.name).view(np.uint64).reshape(-1, 8).tolist()
        # a CPU inflate of every IDAT payload: the model's filtered scanlines
        for k, (r, raw) in enumerate(zip(rows, self.raws)):
            assert 0 < r[5] and r[4] + 8 + r[5] <= len(got), (self.name, k, r)
            assert _inflate("zlib", got[r[4] + 8:r[4] + 8 + r[5]]) == raw, (self.name, k, "round trip")
        files, want_words, want_rows = pw.encode(self.rows, self.buf, _png_zlib(h.level, self.raws))
        assert words == want_words, (self.name, words, want_words)
        assert got == b"".join(files), (self.name, "files differ from the model's")
        assert rows == want_rows, (self.name, "index rows")
        return got


class CTar(_Entries):
    """write_tar_batch: byte for byte tarfile's archive"""
    family, fields = "tar-write", "c->zipw, c->zipw_up"

    def __init__(self, name, names, entries):
        _Entries.__init__(self, name, names, entries)
        self.archive = self.expected = tw.tarfile_bytes(names, entries)

    def validate(self):
        _Entries.validate(self)
        with tarfile.open(fileobj=io.BytesIO(self.archive), mode="r:") as t:
            ms = t.getmembers()
            assert [m.name for m in ms] == list(self.names)
            assert [t.extractfile(m).read() for m in ms] == self.entries

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.buf)
        h.size = obj.tar_write_size(self.names, self.sizes)
        h.out = Guarded(torch, h.size)
        return h

    def enqueue(self, obj, h, stream):
        h.rows = obj.write_tar_batch(self.names, h.d_in, self.offs, self.sizes, h.out.t,
                                     mtime=tw.MTIME, stream=stream, in_avail=len(self.buf),
                                     out_avail=h.size)

    def check(self, h):
        assert h.size == len(self.archive), (self.name, h.size, len(self.archive))
        _same(h.out.host(self.name), np.frombuffer(self.archive, dtype=np.uint8), self.name)
        model = tar_walk.read(self.archive, 64, extract=False)
        assert h.rows.tolist() == model.rows, (self.name, "index rows")
        return self.archive


class CTarGz(CTar):
    family, fields = "tar-write", "c->zipw, c->zipw_up, c->large, c->scratch"

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.buf)
        h.bound = obj.bound("gzip", obj.tar_write_size(self.names, self.sizes))
        h.out = Guarded(torch, h.bound)
        h.nb = Guarded(torch, 1, torch.int64, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        h.rows = obj.compress_targz_batch("gzip", self.names, h.d_in, self.offs, self.sizes, h.out.t,
                                          h.nb.t, mtime=tw.MTIME, stream=stream,
                                          in_avail=len(self.buf), out_avail=h.bound)

    def check(self, h):
        nb, host = int(h.nb.host(self.name)[0]), h.out.host(self.name)
        assert 0 < nb <= h.bound, (self.name, nb)
        got = host[:nb].tobytes()
        assert (host[nb:] == CANARY).all(), (self.name, "bytes written behind the stream")
        assert _inflate("gzip", got) == self.archive, (self.name, "round trip")
        assert h.rows.tolist() == tar_walk.read(self.archive, 64, extract=False).rows
        return got


class CLarge(CStep):
    """compress_large_batch: ONE stream of the whole buffer"""
    family, fields = "compress-large", "c->large, c->scratch"

    def __init__(self, name, fmt, data):
        self.name, self.fmt, self.data = name, fmt, data
        self.expected = data

    def validate(self):
        assert len(self.data) > 131072      # (segmented: above the segment rule's edge)
        assert _inflate(self.fmt, _deflate(self.fmt, self.data)) == self.data

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.data)
        h.bound = obj.bound(self.fmt, len(self.data))
        h.out = Guarded(torch, h.bound)
        h.nb = Guarded(torch, 1, torch.int64, UNSET)
        return h

    def enqueue(self, obj, h, stream):
        obj.compress_large_batch(self.fmt, h.d_in, h.out.t, h.nb.t, stream=stream,
                                 in_nbytes=len(self.data), out_avail=h.bound)

    def check(self, h):
        nb, host = int(h.nb.host(self.name)[0]), h.out.host(self.name)
        assert 0 < nb <= h.bound, (self.name, nb)
        got = host[:nb].tobytes()
        assert (host[nb:] == CANARY).all(), (self.name, "bytes written behind the stream")
        assert _inflate(self.fmt, got) == self.data, (self.name, "round trip")
        return got


def _bgzf_checked(name, got, data, rows):
    """a BGZF file of ours: the spec's layout (bgzf_walk), the bytes, the index"""
    members, has_eof = bgzf_walk.walk(got)
    assert has_eof and b"".join(m.data for m in members) == data, (name, "round trip")
    assert [m.isize for m in members] == [min(B, len(data) - k) for k in range(0, len(data), B)]
    want, u = [], 0
    for m in members:
        want.append([m.offset, u])
        u += m.isize
    want.append([len(got) - len(bgzf_walk.EOF_MEMBER), u])
    assert np.asarray(rows).astype(np.int64).reshape(-1, 2).tolist() == want, (name, "index")
    assert gzip.decompress(got) == data


class CBgzf(CLarge):
    family, fields = "bgzf-write", "c->scratch"

    def validate(self):
        assert len(self.data) == 3 * B + 17
        got, rows = _bgzf_by_zlib(self.data)
        _bgzf_checked(self.name, got, self.data, rows)

    def prepare(self, torch, obj=None):
        h = Handle()
        h.d_in = _stage(torch, h, self.data)
        h.bound = obj.bgzf_bound(len(self.data))
        h.out = Guarded(torch, h.bound)
        h.nb = Guarded(torch, 1, torch.int64, UNSET)
        h.idx = Guarded(torch, 2 * (-(-len(self.data) // B) + 1), torch.int64, -1)
        return h

    def enqueue(self, obj, h, stream):
        obj.compress_bgzf_batch(h.d_in, h.out.t, h.nb.t, index=h.idx.t, stream=stream,
                                in_nbytes=len(self.data), out_avail=h.bound)

    def check(self, h):
        nb, host = int(h.nb.host(self.name)[0]), h.out.host(self.name)
        assert 0 < nb <= h.bound, (self.name, nb)
        got = host[:nb].tobytes()
        assert (host[nb:] == CANARY).all(), (self.name, "bytes written behind the file")
        _bgzf_checked(self.name, got, self.data, h.idx.host(self.name))
        return got


class CHost(CStep):
    """compress_batch_host, compress, compress_bgzf on host buffers: BLOCK"""
    family, blocking, fields = "host", True, "c->scratch, pinned slices"

    def __init__(self, name, how, fmt, chunks):
        self.name, self.how, self.fmt, self.chunks = name, how, fmt, chunks
        self.expected = chunks

    def validate(self):
        assert self.how in ("batch", "one", "bgzf") and self.chunks
        assert self.how == "batch" or len(self.chunks) == 1
        for c in self.chunks:
            if self.how == "bgzf":
                got, rows = _bgzf_by_zlib(c)
                _bgzf_checked(self.name, got, c, rows)
            else:
                assert _inflate(self.fmt, _deflate(self.fmt, c)) == c

    def prepare(self, torch, obj=None):
        return Handle()

    def enqueue(self, obj, h, stream):
        if self.how == "batch":
            h.got = obj.compress_batch_host(self.fmt, self.chunks)
        elif self.how == "one":
            h.got = [obj.compress(self.fmt, self.chunks[0])]
        else:
            h.got = obj.compress_bgzf(self.chunks[0], index=True)

    def check(self, h):
        if self.how == "bgzf":
            assert h.got is not None, self.name
            _bgzf_checked(self.name, h.got[0], self.chunks[0], h.got[1])
            return h.got[0]
        for k, (z, c) in enumerate(zip(h.got, self.chunks)):
            assert z is not None and _inflate(self.fmt, z) == c, (self.name, k, "round trip")
        return h.got


def _entries(seed, sizes):
    text = datagen.text_chunk(sum(sizes), seed)
    out, at = [], 0
    for n in sizes:
        out.append(text[at:at + n])
        at += n
    return out


def compressor_steps():
    """name -> CStep; built once per process"""
    if "c" in _steps:
        return _steps["c"]
    st = {}

    def add(s):
        assert s.name not in st
        st[s.name] = s
    add(CBatch("c-batch-large", "gzip", [datagen.chunk(i, 65536, 0xC640) for i in range(40)]))
    rng = random.Random(0xC4096)
    small = [datagen.chunk(i, rng.choice((1, 31, 32, 500, 4095, 4096)), 0xC200, datagen.MIX4K)
             for i in range(200)]
    add(CBatch("c-batch-small", "zlib", small, max_chunk=4096))
    for n in (3, 500):      # (C2: ascending and descending chunk counts)
        add(CBatch(f"c-batch-small{n}", "deflate", (small * 3)[:n], max_chunk=4096))
    dictionary = datagen.text_chunk(5000, 0xD1C7)
    chunks = [dictionary[100 * i:100 * i + 700] + datagen.text_chunk(3000, 0xD1C8 + i)
              for i in range(12)]
    add(CBatch("c-dict", "zlib", chunks, dictionary=dictionary))
    names = [b"a", "déjà vu/漢字.txt".encode("utf-8"), b"dir/e2", b"n" * 255, b"e4", b"e5",
             b"e6", b"noise"]
    entries = _entries(0x21D, (0, 1, 100, 4096, 4097, 65537, 131073)) + [datagen.random_chunk(1000, 1)]
    add(CZip("c-zip", names, entries))
    add(CZip("c-zip2", names[:2], entries[5:7]))
    gnames = [None, b"a", b"", "w/漢字.warc".encode("utf-8"), b"b", None, b"big.bin", b"noise"]
    add(CGzm("c-gzm", gnames, _entries(0x2B1, (0, 1, 31, 32, 4096, 4097, 131073)) +
             [datagen.random_chunk(7000, 7)]))
    add(CPng("c-png", [(w, h, d, c, build(w, h, d, c, 0x9C + w)) for w, h, d, c, build in
                       ((1, 1, 8, 0, pf.pixels_random), (7, 5, 8, 2, pf.pixels_random),
                        (33, 17, 16, 6, pf.pixels_smooth), (43690, 3, 8, 0, pf.pixels_smooth))]))
    tnames = ["a", "dir/file01.txt", "d" * 101, "é€" * 60, "g" * 600, "dir/file05.txt", "e6", "e7"]
    tsizes = (0, 1, 511, 512, 513, 65536, 65537, 17)
    tdatas = [tw.payload(k, s) for k, s in enumerate(tsizes)]
    add(CTar("c-tar", tnames, tdatas))
    add(CTar("c-tar2", tnames[:2], tdatas[6:8]))
    add(CTarGz("c-targz", tnames, tdatas))
    add(CLarge("c-large", "gzip", datagen.text_chunk(300 << 10, 0xC1A6)))
    add(CBgzf("c-bgzf", "bgzf", datagen.text_chunk(3 * B + 17, 0xCB62)))
    add(CHost("c-batch-host", "batch", "gzip", [datagen.chunk(i, 20000 + i, 0xC805) for i in range(16)]))
    add(CHost("c-one", "one", "zlib", [datagen.text_chunk(200000, 0xC806)]))
    add(CHost("c-bgzf-host", "bgzf", "bgzf", [datagen.text_chunk(2 * B + 5, 0xC807)]))
    _steps["c"] = st
    return st
