"""Hand-built BYTE_ARRAY pages for the tests of
libdeflate_amd_parquet_decode_batch_ex, on top of tests/parquet_pages.py's hybrid
encoder and Page: sections of length-prefixed values, dictionary and data pages
in both versions, a layout with gaps, and one call on the GPU against
tools/models/parquet_strings_model.py with canaries around everything."""
import os

import numpy as np

from tests import parquet_pages as pp
from tools.models import parquet_model as pm
from tools.models import parquet_strings_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_strings")
CANARY, UNSET, GUARD = pp.CANARY, pp.UNSET, pp.GUARD


def fixture_files():
    return sorted(n for n in os.listdir(GOLDEN) if n.endswith(".parquet"))


def fixture(name):
    """(the file's bytes, {column: (offsets int64 from 0, bytes uint8, valid
    uint8)} as pyarrow read them back)"""
    buf = open(os.path.join(GOLDEN, name), "rb").read()
    group, want = name.split("_")[0], {}
    for n in sorted(os.listdir(GOLDEN)):
        if n.startswith(group + ".") and n.endswith(".npz"):
            z = np.load(os.path.join(GOLDEN, n))
            want[n[len(group) + 1:-len(".npz")]] = (z["offsets"], z["bytes"], z["valid"])
    return buf, want


def section_of(vals):
    """the values, each behind its 4-byte length"""
    return b"".join(len(v).to_bytes(4, "little") + bytes(v) for v in vals)


def dict_page(entries, compress=True, fmt="gzip", section=None, count=None):
    """entries: a list of bytes; section / count: what the page holds and
    states instead, for the failure tests"""
    p = pp.Page(pm.DICT, 1, len(entries) if count is None else count,
                section_of(entries) if section is None else section, compress=compress, fmt=fmt)
    p.byte_array, p.entries = True, list(entries)
    return p


def data_page(rng, version, vals, dictionary=None, indices=None, w=None, shape="bp",
              level_shape="bp", compress=True, fmt="gzip", required=False, section=None):
    """A data page of len(vals) slots: bytes, or None for a null (required: no
    levels, and no None).  dictionary: None (PLAIN) or dict_page()'s Page,
    whose entries must hold the values - or `indices` given outright, one per
    valid slot.  section: the values section instead of the right one."""
    mask = None if required else np.array([v is not None for v in vals], dtype=np.uint8)
    present = [v for v in vals if v is not None]
    levels = None if required else pp.encode_runs(pp.runs_of(mask, 1, level_shape, rng), 1)
    if dictionary is None:
        sec, enc = section_of(present), pm.PLAIN
    else:
        e = len(dictionary.entries)
        if w is None:
            w = max(e - 1, 0).bit_length()
        if indices is None:
            indices = [dictionary.entries.index(v) for v in present]
        sec = b"" if not present else bytes([w]) + pp.encode_runs(pp.runs_of(indices, w, shape, rng), w)
        enc = pm.RLE_DICTIONARY
    page = pp.Page(pm.DATA_V1 if version == 1 else pm.DATA_V2, 1, len(vals),
                   sec if section is None else section, levels, enc, int(not required), compress, fmt)
    page.dict_page, page.byte_array = dictionary, True
    return page


def lay_out(pages, rng):
    """the pages packed at unaligned offsets with junk between them; every
    data page's slots - a string page's count + 1 offsets at a multiple of 8 -
    and validity bytes behind the previous one's with a gap -> (buf, rows,
    out_nbytes, valid_nbytes)"""
    buf, rows, out_at, valid_at, where = bytearray(), [], 0, 0, {}
    for k, p in enumerate(pages):
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        where[id(p)] = k
        is_str = getattr(p, "byte_array", False)
        if p.kind == pm.DICT:
            row = p.row(len(buf))
        else:
            out_at += rng.randrange(0, 4)
            valid_at += rng.randrange(0, 4)
            if is_str:
                out_at = (out_at + 7) // 8 * 8 + 8 * rng.randrange(0, 2)
            row = p.row(len(buf), out_at, valid_at if p.max_def else 0,
                        where[id(p.dict_page)] if p.dict_page is not None else 0)
            out_at += (p.count + 1) * 8 if is_str else p.count * p.width
            valid_at += p.count if p.max_def else 0
        if is_str:
            row[3] |= sm.BYTE_ARRAY
        rows.append(row)
        buf += p.stored
    buf += b"\x1f\x8b" * 3
    return bytes(buf), np.array(rows, dtype=np.uint64).reshape(-1, pm.WORDS), out_at, valid_at


def run_gpu(torch, dec, buf, rows, fmt, out_nbytes, valid_nbytes, bytes_avail=None,
            want_results=None, sizing=False):
    """One call on the GPU against the model: every result, the total, every
    offset, string byte and validity byte that the model defines, and the
    canaries in front of, between and behind them.  bytes_avail None: what
    the model's total asks for; sizing: d_bytes NULL.  -> the model's dict"""
    if bytes_avail is None:
        bytes_avail = sm.decode(rows, buf, fmt, out_nbytes, valid_nbytes, 0)["total"]
    m = sm.decode(rows, buf, fmt, out_nbytes, valid_nbytes, bytes_avail, CANARY)
    if want_results is not None:
        assert m["results"] == list(want_results), m["results"]
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    # (d_out stays 8-byte aligned behind its guard)
    g_out = torch.full((GUARD + out_nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    g_valid = torch.full((GUARD + valid_nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    g_data = torch.full((GUARD + bytes_avail + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    total = torch.full((3,), UNSET, dtype=torch.int64, device="cuda")
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.parquet_decode_batch_ex(fmt, rows, d_in, g_out[GUARD:], g_valid[GUARD:],
                                None if sizing else g_data[GUARD:], total[1:2], per,
                                out_avail=out_nbytes, valid_avail=valid_nbytes,
                                bytes_avail=bytes_avail)
    torch.cuda.synchronize()
    got = per.cpu().numpy()
    assert got[len(rows)] == UNSET
    assert got[:len(rows)].tolist() == m["results"], (got[:len(rows)].tolist(), m["results"])
    assert total.cpu().tolist() == [UNSET, m["total"], UNSET], (total.cpu().tolist(), m["total"])
    for name, g, n, want, defined in (("d_out", g_out, out_nbytes, m["out"], m["out_defined"]),
                                      ("d_valid", g_valid, valid_nbytes, m["valid"], m["valid_defined"]),
                                      ("d_bytes", g_data, bytes_avail, m["data"], m["data_defined"])):
        host = g.cpu().numpy()
        assert not (host[:GUARD] != CANARY).any(), "bytes written in front of " + name
        assert not (host[GUARD + n:] != CANARY).any(), "bytes written behind the end of " + name
        bad = np.nonzero((host[GUARD:GUARD + n] != want) & defined)[0]
        assert not bad.size, "%s: first wrong byte at %d (got %d, want %d); %d wrong in all" % (
            name, bad[0], host[GUARD + bad[0]], want[bad[0]], bad.size)
    return m


def strings_of(m, row, count):
    """the slots of the data page `row` (its word 5, count) out of a model's or
    a run's dict -> a list of bytes"""
    o = m["out"][int(row[5]):int(row[5]) + (count + 1) * 8].view("<i8")
    return [bytes(m["data"][o[k]:o[k + 1]]) for k in range(count)]
