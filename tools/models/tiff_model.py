"""CPU model of the predictor-coded deflate strips and tiles of TIFF and GeoTIFF
(include/libdeflate_amd.h: libdeflate_amd_tiff_decode_batch and
libdeflate_amd_tiff_encode_batch; csrc/tiff_plan.h): the two predictors and
their inverses in numpy, the rows, the reasons a row is refused with, the
writer's bound, the reader's classification of a row and the kernels' group
sizes.  The tests' oracle, with Python's zlib.

A segment is `rows` rows of `width` pixels, a pixel spp samples of bps bytes,
little-endian, pixel-interleaved.
  predictor 2  every sample minus the sample of its channel one pixel to the
               left, modulo 2^(8 bps); undone by a cumsum per row and channel.
  predictor 3  the row's samples as bps byte planes, the most significant
               first, then every byte of the row minus the byte spp places
               earlier; undone by a byte cumsum at stride spp over the row,
               the planes reversed and transposed."""
import numpy as np

WORDS, SPP_MAX, RESULT_WORDS = 8, 16, 4
PTILE = 4096                        # csrc/kernels.h: LDA_TIFF_PTILE
MAX_SEGMENTS = 1 << 28
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
DIRECT, SCAN, SCAN_GATHER = range(3)        # what a row is to the reader
_DTYPE = {1: np.uint8, 2: "<u2", 4: "<u4", 8: "<u8"}


def _bytes(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def undo(buf, rows, width, spp, bps, predictor):
    """the decoded bytes of a segment -> its pixels' bytes"""
    a = _bytes(buf)
    assert a.size == rows * width * spp * bps
    if predictor == 1:
        return a.tobytes()
    if predictor == 2:
        s = a.view(_DTYPE[bps]).reshape(rows, width, spp)
        return np.cumsum(s, axis=1, dtype=s.dtype).astype(s.dtype).tobytes()
    assert predictor == 3 and bps > 1
    ns = width * spp
    b = a.reshape(rows, bps * width, spp)
    b = np.cumsum(b, axis=1, dtype=np.uint8).reshape(rows, bps, ns)
    # plane 0 is the most significant byte: byte bps - 1 of a little-endian sample
    return np.ascontiguousarray(b[:, ::-1, :].transpose(0, 2, 1)).tobytes()


def apply(buf, rows, width, spp, bps, predictor):
    """a segment's pixels' bytes -> the bytes that are deflated"""
    a = _bytes(buf)
    assert a.size == rows * width * spp * bps
    if predictor == 1:
        return a.tobytes()
    if predictor == 2:
        s = a.view(_DTYPE[bps]).reshape(rows, width, spp).copy()
        s[:, 1:, :] = s[:, 1:, :] - s[:, :-1, :]
        return s.tobytes()
    assert predictor == 3 and bps > 1
    ns = width * spp
    planes = a.reshape(rows, ns, bps).transpose(0, 2, 1)[:, ::-1, :]
    b = np.ascontiguousarray(planes).reshape(rows, bps * width, spp).copy()
    b[:, 1:, :] = b[:, 1:, :] - b[:, :-1, :]
    return b.tobytes()


def pad(pixels, kept, coded, spp, bps):
    """the kept rectangle's bytes (kept = (width, rows)) -> the coded segment's:
    zero samples on the right and at the bottom"""
    (kw, kr), (cw, cr) = kept, coded
    px = spp * bps
    out = np.zeros((cr, cw * px), dtype=np.uint8)
    out[:kr, :kw * px] = _bytes(pixels).reshape(kr, kw * px)
    return out.tobytes()


def crop(seg, kept, coded, spp, bps):
    """the coded segment's pixels -> the kept rectangle's"""
    (kw, kr), (cw, cr) = kept, coded
    px = spp * bps
    return _bytes(seg).reshape(cr, cw * px)[:kr, :kw * px].tobytes()


def row(stored_off, stored_n, raw_off, pitch, coded, kept, spp, bps, predictor):
    """one segment's words"""
    return [int(stored_off), int(stored_n), int(raw_off), int(pitch),
            int(coded[0]) | int(coded[1]) << 32, int(kept[0]) | int(kept[1]) << 32,
            int(spp) | int(bps) << 8 | int(predictor) << 16, 0]


def rows(raw_offsets, pitches, coded, kept, spp, bps, predictor, stored_offsets=None,
         stored_sizes=None):
    """lists or single values -> numpy uint64 (segments, WORDS); api.tiff_rows()"""
    n = len(raw_offsets)

    def per(v):
        return list(v) if isinstance(v, (list, np.ndarray)) else [v] * n
    so, sn = per(0 if stored_offsets is None else stored_offsets), \
        per(0 if stored_sizes is None else stored_sizes)
    pi, cd, sp, bp, pr = per(pitches), per(coded), per(spp), per(bps), per(predictor)
    kp = cd if kept is None else per(kept)
    out = np.zeros((n, WORDS), dtype=np.uint64)
    for k in range(n):
        for w, v in enumerate(row(so[k], sn[k], raw_offsets[k], pi[k], cd[k], kp[k], sp[k], bp[k],
                                  pr[k])):
            out[k, w] = v
    return out


def unpack(r):
    """a row -> dict of its fields"""
    r = [int(x) for x in r]
    d = dict(stored_off=r[0], stored_n=r[1], raw_off=r[2], pitch=r[3],
             cw=r[4] & 0xFFFFFFFF, cr=r[4] >> 32, kw=r[5] & 0xFFFFFFFF, kr=r[5] >> 32,
             spp=r[6] & 0xFF, bps=(r[6] >> 8) & 0xFF, pred=(r[6] >> 16) & 0xFF,
             other=r[6] >> 24, reserved=r[7])
    d["px"] = d["spp"] * d["bps"]
    d["coded"] = d["cw"] * d["cr"] * d["px"]
    d["kept_rb"] = d["kw"] * d["px"]
    return d


def row_why(r, reader, stored_avail, raw_avail, level=-1):
    """the word of the reason a call refuses the row with, or None"""
    d = unpack(r)
    if d["other"]:
        return "word 6"
    if d["reserved"]:
        return "word 7"
    if d["spp"] == 0 or d["spp"] > SPP_MAX:
        return "samples per pixel"
    if d["bps"] not in (1, 2, 4, 8):
        return "bytes per sample"
    if d["pred"] not in (1, 2, 3):
        return "predictor"
    if d["pred"] == 3 and d["bps"] == 1:
        return "floating-point"
    if 0 in (d["cw"], d["cr"], d["kw"], d["kr"]):
        return "zero"
    if d["kw"] > d["cw"] or d["kr"] > d["cr"]:
        return "kept above coded"
    if d["coded"] >= 1 << 32:
        return "2^32"
    if reader and (d["stored_off"] > stored_avail or stored_avail - d["stored_off"] < d["stored_n"]):
        return "in_nbytes"
    if d["kr"] > 1 and d["pitch"] < d["kept_rb"]:
        return "pitch"
    if d["raw_off"] + (d["kr"] - 1) * (d["pitch"] if d["kr"] > 1 else 0) + d["kept_rb"] > raw_avail:
        return "out_avail" if reader else "in_avail"
    if not reader and level == 0 and d["coded"] > 0xFFFFFF00:
        return "level-0"
    return None


def stream_bound(n):
    """libdeflate_zlib_compress_bound(n)"""
    return 5 * max(1, (n + 4999) // 5000) + n + 6


def bound(rws):
    """libdeflate_amd_tiff_encode_bound; 0 for rows the writer refuses"""
    if any(row_why(r, False, 0, (1 << 64) - 1) for r in rws):
        return 0
    return sum(stream_bound(unpack(r)["coded"]) for r in rws)


def classify(r):
    """what the reader's plan does with a row that passed the checks"""
    d = unpack(r)
    if d["pred"] == 1 and d["kw"] == d["cw"] and d["kr"] == d["cr"] and \
            (d["cr"] == 1 or d["pitch"] == d["cw"] * d["px"]):
        return DIRECT
    return SCAN_GATHER if d["pred"] == 3 else SCAN


REG_STRIDES = (1, 2, 4, 8, 16, 3, 6, 12, 24, 48)


def lane_bytes(st):
    """the bytes of a row a lane of the unpredict kernel owns in a pass"""
    if st == 0:
        return 16
    if st not in REG_STRIDES:
        return st
    return 48 if st % 3 == 0 else 64


def group(rb, st):
    """the lanes of the group that walks a row of rb bytes at stride st"""
    lb = lane_bytes(st)
    return 4 if rb <= 4 * lb else 16 if rb <= 16 * lb else 64


def expected(r, seg_pixels):
    """the bytes the reader leaves in the kept rectangle, row by row (a list of
    kept_rows byte strings), from the coded segment's pixels"""
    d = unpack(r)
    a = _bytes(seg_pixels).reshape(d["cr"], d["cw"] * d["px"])
    return [a[y, :d["kept_rb"]].tobytes() for y in range(d["kr"])]
