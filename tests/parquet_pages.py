"""Hand-built Parquet pages for the tests of libdeflate_amd_parquet_decode_batch:
a small RLE / bit-packed hybrid *encoder* over explicit run structures, page
bodies in both data page versions, and the rows that describe them.  Nothing
here is a Parquet writer: there is no Thrift and no file, only what the call
reads."""
import os
import zlib

import numpy as np

from tools.models import parquet_model as pm

WBITS = pm.WBITS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet")


def fixture_files():
    """the names of tests/golden/parquet's Parquet files"""
    return sorted(n for n in os.listdir(GOLDEN) if n.endswith(".parquet"))


def fixture(name):
    """(the file's bytes, {column: (uint8 [rows, width] values, uint8 [rows]
    validity)} as pyarrow read them back)"""
    buf = open(os.path.join(GOLDEN, name), "rb").read()
    group, want = name.split("_")[0], {}
    for n in sorted(os.listdir(GOLDEN)):
        if n.startswith(group + ".") and n.endswith(".values.npy"):
            col = n[len(group) + 1:-len(".values.npy")]
            want[col] = (np.load(os.path.join(GOLDEN, n)),
                         np.load(os.path.join(GOLDEN, n.replace(".values.", ".valid."))))
        elif n.startswith(group + ".") and n.endswith(".npz"):
            z = np.load(os.path.join(GOLDEN, n))
            want[n[len(group) + 1:-len(".npz")]] = (z["values"], z["valid"])
    return buf, want


def expected(pg, want, fill):
    """the d_out and d_valid bytes of parquet.pages()'s layout pg from the
    fixture's columns, `fill` everywhere else"""
    out = np.full(pg.out_nbytes, fill, dtype=np.uint8)
    valid = np.full(pg.valid_nbytes, fill, dtype=np.uint8)
    for name, c in pg.columns.items():
        out[c.offset:c.offset + c.rows * c.width] = want[name][0].reshape(-1)
        if c.valid_offset is not None:
            valid[c.valid_offset:c.valid_offset + c.rows] = want[name][1]
    return out, valid


CANARY, UNSET, GUARD = 0xA5, -7, 64


def run_gpu(torch, dec, buf, rows, fmt, out_nbytes, valid_nbytes, want_results=None):
    """One call on the GPU against the model: every result, every slot byte and
    every validity byte of the pages that succeed equal the model's, and the
    canary bytes in front of d_out and d_valid, between the pages' slots and
    behind out_avail and valid_avail stay untouched.  -> (results, out, valid)
    as numpy arrays"""
    res, out, valid, out_def, valid_def = pm.decode(rows, buf, fmt, out_nbytes, valid_nbytes, CANARY)
    if want_results is not None:
        assert res == list(want_results), res
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    g_out = torch.full((GUARD + out_nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    g_valid = torch.full((GUARD + valid_nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    got_rows = dec.parquet_decode_batch(fmt, rows, d_in, g_out[GUARD:], g_valid[GUARD:], per,
                                        out_avail=out_nbytes, valid_avail=valid_nbytes)
    torch.cuda.synchronize()
    assert d_in.numel() == len(buf)
    assert (got_rows == np.asarray(rows, dtype=np.uint64).reshape(-1, pm.WORDS)).all()
    got = per.cpu().numpy()
    assert got[len(rows)] == UNSET
    assert got[:len(rows)].tolist() == res
    for name, g, n, want, defined in (("d_out", g_out, out_nbytes, out, out_def),
                                      ("d_valid", g_valid, valid_nbytes, valid, valid_def)):
        host = g.cpu().numpy()
        assert not (host[:GUARD] != CANARY).any(), "bytes written in front of " + name
        assert not (host[GUARD + n:] != CANARY).any(), "bytes written behind the end of " + name
        bad = np.nonzero((host[GUARD:GUARD + n] != want) & defined)[0]
        if bad.size:
            word = 5 if name == "d_out" else 6
            k = max((i for i, r in enumerate(rows) if int(r[3]) & 15 != pm.DICT and
                     int(r[word]) <= bad[0]), key=lambda i: int(rows[i][word]), default=-1)
            raise AssertionError("%s: first wrong byte at %d (got %d, want %d), page row %d %r; %d "
                                 "wrong in all" % (name, bad[0], host[GUARD + bad[0]], want[bad[0]], k,
                                                   pm.unpack(rows[k]) if k >= 0 else None, bad.size))
    return got[:len(rows)], g_out.cpu().numpy()[GUARD:GUARD + out_nbytes], \
        g_valid.cpu().numpy()[GUARD:GUARD + valid_nbytes]


def uleb(v, nbytes=None):
    """v as ULEB128, in exactly nbytes bytes if given (padded with continuation
    bytes, as the format allows)"""
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        more = v or (nbytes is not None and len(out) + 1 < nbytes)
        out.append(b | (0x80 if more else 0))
        if not more:
            return bytes(out)


def encode_runs(runs, w, hdr=None):
    """runs: [("rle", value, count)] and [("bp", [values])] (a multiple of 8
    values) -> the hybrid stream of bit width w; hdr: the bytes of every run
    header"""
    out = bytearray()
    for run in runs:
        if run[0] == "rle":
            out += uleb(run[2] << 1, hdr) + int(run[1]).to_bytes((w + 7) // 8, "little")
        else:
            vals = [int(v) for v in run[1]]
            assert len(vals) % 8 == 0
            out += uleb(len(vals) // 8 << 1 | 1, hdr)
            acc = 0
            for k, v in enumerate(vals):
                assert v < 1 << w or w == 0
                acc |= v << (k * w)
            out += acc.to_bytes(len(vals) * w // 8, "little")
    return bytes(out)


def runs_of(values, w, shape, rng, group_max=63):
    """a run structure that codes `values` (ints below 2^w).  shape: "rle" -
    maximal runs of equal values; "rle1" - RLE runs of one value; "bp" -
    bit-packed runs of at most group_max groups, the last padded past the end
    with junk; "alt" - RLE and bit-packed runs alternating"""
    vals, n, runs, p = [int(v) for v in values], len(values), [], 0

    def junk(k):
        return [rng.randrange(1 << w) if w else 0 for _ in range(k)]

    def equal_from(p):
        q = p
        while q < n and vals[q] == vals[p]:
            q += 1
        return q - p
    turn = 0
    while p < n:
        if shape == "rle1" or (shape == "rle") or (shape == "alt" and turn % 2 == 0):
            c = 1 if shape == "rle1" else equal_from(p)
            runs.append(("rle", vals[p], c))
            p += c
        else:
            g = group_max if shape == "bp" else rng.randrange(1, 4)
            take = min(8 * g, n - p)
            pad = -take % 8
            runs.append(("bp", vals[p:p + take] + junk(pad)))
            p += take
        turn += 1
    return runs


def pack(fmt, data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    return c.compress(bytes(data)) + c.flush()


class Page:
    """one page as the call sees it.  stored: its body in the file; f: the
    fields of its row (tools/models/parquet_model.py: unpack) without the
    offsets"""

    def __init__(self, kind, width, count, section, levels=None, enc=pm.PLAIN, max_def=0,
                 compress=True, fmt="gzip", usize_delta=0, level_len=None):
        self.kind, self.width, self.count, self.enc, self.max_def = kind, width, count, enc, max_def
        self.compressed, self.def_len = bool(compress), 0
        if kind == pm.DATA_V2:
            lev = levels if max_def else b""
            self.def_len = len(lev)
            self.stored = lev + (pack(fmt, section) if compress else section)
            self.usize = len(lev) + len(section)
        else:
            body = section
            if kind == pm.DATA_V1 and max_def:
                # (level_len: a wrong length prefix, for the failure tests)
                body = (len(levels) if level_len is None else level_len).to_bytes(4, "little") + \
                    levels + section
            self.stored = pack(fmt, body) if compress else body
            self.usize = len(body)
        self.usize += usize_delta          # (a lie in the header, for the failure tests)
        self.dict_page = None              # a dictionary-coded page: its dictionary's Page

    def row(self, off, out=0, valid=0, dict_row=0):
        return [off, len(self.stored), self.usize if self.compressed else len(self.stored),
                self.kind | self.enc << 4 | int(self.compressed) << 12 | self.max_def << 13 |
                (self.width - 1) << 16, self.count | self.def_len << 32, out, valid, dict_row]


def dict_page(entries, compress=True, fmt="gzip"):
    """entries: uint8 [n, width]"""
    e = np.ascontiguousarray(entries, dtype=np.uint8)
    return Page(pm.DICT, e.shape[1], e.shape[0], e.tobytes(), compress=compress, fmt=fmt)


def data_page(rng, version, width, mask=None, dictionary=None, entries=None, w=None, shape="bp",
              level_shape="bp", hdr=None, compress=True, fmt="gzip", n=None, level_runs=None,
              index_runs=None, indices=None):
    """A data page of n slots.  mask: None (max_def 0) or n 0/1 levels;
    dictionary: None (PLAIN, random values) or the dictionary's Page with
    `entries` uint8 [E, width]; w: the index bit width (None: the least that
    holds E - 1); shape / level_shape: runs_of()'s, or level_runs / index_runs
    given outright.  -> (Page, uint8 [n, width] expected slots)"""
    if mask is not None:
        mask = np.asarray(mask, dtype=np.uint8)
        n = len(mask)
    nv = n if mask is None else int(mask.sum())
    levels = None
    if mask is not None:
        levels = encode_runs(level_runs or runs_of(mask, 1, level_shape, rng), 1, hdr)
    if dictionary is None:
        vals = np.frombuffer(bytes(rng.randrange(256) for _ in range(nv * width)),
                             dtype=np.uint8).reshape(nv, width)
        section, enc = vals.tobytes(), pm.PLAIN
    else:
        e = len(entries)
        if w is None:
            w = max(e - 1, 0).bit_length()
        if indices is None:
            indices = [rng.randrange(e) for _ in range(nv)]
        # (an index past the dictionary, for the failure tests: the page fails anyway)
        vals = entries[np.minimum(np.asarray(indices, dtype=np.int64), e - 1)] if nv else \
            np.zeros((0, width), np.uint8)
        section = b"" if nv == 0 and index_runs is None else \
            bytes([w]) + encode_runs(index_runs or runs_of(indices, w, shape, rng), w, hdr)
        enc = pm.RLE_DICTIONARY
    page = Page(pm.DATA_V1 if version == 1 else pm.DATA_V2, width, n, section, levels, enc,
                int(mask is not None), compress, fmt)
    page.dict_page = dictionary
    want = np.zeros((n, width), dtype=np.uint8)
    want[(mask if mask is not None else np.ones(n, np.uint8)) == 1] = vals
    return page, want


def lay_out(pages, rng, junk=True):
    """the pages packed at unaligned offsets with junk between them, every data
    page's slots and validity bytes behind the previous one's with a gap ->
    (buf, rows, out_nbytes, valid_nbytes)"""
    buf, rows, out_at, valid_at, where = bytearray(), [], 0, 0, {}
    for k, p in enumerate(pages):
        if junk:
            buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        where[id(p)] = k
        if p.kind == pm.DICT:
            rows.append(p.row(len(buf)))
        else:
            out_at += rng.randrange(0, 4) if junk else 0
            valid_at += rng.randrange(0, 4) if junk else 0
            rows.append(p.row(len(buf), out_at, valid_at if p.max_def else 0,
                              where[id(p.dict_page)] if p.dict_page is not None else 0))
            out_at += p.count * p.width
            valid_at += p.count if p.max_def else 0
        buf += p.stored
    buf += b"\x1f\x8b" * 3      # behind the last page: never read as part of it
    return bytes(buf), np.array(rows, dtype=np.uint64).reshape(-1, pm.WORDS), out_at, valid_at
