"""CPU model of the byte-shuffled deflate chunks of HDF5, NetCDF-4 and Zarr
(include/libdeflate_amd.h: libdeflate_amd_shuffle_decompress_batch and
libdeflate_amd_shuffle_compress_batch; csrc/shuffle_plan.h): the transform and
its inverse in numpy, the rows, the writer's bound, the tile sizes and the
reader's classification of a row.  The tests' oracle, with Python's zlib.

A chunk of n bytes and element size es has ne = n // es elements and n % es
bytes behind them:
    shuffled[j * ne + k]  = raw[k * es + j]
    shuffled[es * ne + t] = raw[es * ne + t]
(H5Z_FILTER_SHUFFLE)."""
import numpy as np

WORDS, ELEM_MAX, NO_DEFLATE, NO_SHUFFLE, RESULT_WORDS = 6, 256, 1, 2, 4
TILE, GEN_BYTES = 4096, 16384       # csrc/kernels.h: LDA_SHUF_TILE, LDA_SHUF_GEN_BYTES
MAX_CHUNKS = 1 << 28
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
FORMATS = {"deflate": 0, "zlib": 1, "gzip": 2}
# what a row is to the reader
DECODE_DIRECT, DECODE_UNSHUFFLE, STORED_UNSHUFFLE, STORED_COPY, STORED_BAD, STORED_EMPTY = range(6)


def _bytes(raw):
    return np.frombuffer(bytes(raw), dtype=np.uint8)


def shuffle(raw, es):
    """raw bytes -> shuffled bytes"""
    a = _bytes(raw)
    ne = len(a) // es
    body = a[:ne * es].reshape(ne, es).T
    return body.tobytes() + a[ne * es:].tobytes()


def unshuffle(sh, es):
    """shuffled bytes -> raw bytes"""
    a = _bytes(sh)
    ne = len(a) // es
    body = a[:ne * es].reshape(es, ne).T
    return body.tobytes() + a[ne * es:].tobytes()


def identity(n, es, mask=0):
    return es == 1 or n // es <= 1 or bool(mask & NO_SHUFFLE)


def tile_elems(es):
    """the elements of one tile of the transpose kernels"""
    return TILE if es in (1, 2, 4, 8) else (GEN_BYTES // es) & ~15


def tiles(n, es):
    t = tile_elems(es)
    return (n // es + t - 1) // t


def rows(raw_offsets, raw_sizes, es, stored_offsets=None, stored_sizes=None, mask=0):
    """lists or single values -> numpy uint64 (chunks, WORDS)"""
    n = len(raw_offsets)

    def per(v):
        return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
    out = np.zeros((n, WORDS), dtype=np.uint64)
    for w, col in enumerate((per(0 if stored_offsets is None else stored_offsets),
                             per(0 if stored_sizes is None else stored_sizes), raw_offsets,
                             raw_sizes, per(es), per(mask))):
        for k in range(n):
            out[k, w] = int(col[k])
    return out


def row_why(row, reader, stored_avail, raw_avail):
    """the word of the reason a call refuses the row with, or None"""
    so, sn, ro, rn, es, mask = (int(x) for x in row)
    if es == 0 or es > ELEM_MAX:
        return "element size"
    if mask & ~((NO_DEFLATE | NO_SHUFFLE) if reader else NO_SHUFFLE):
        return "mask"
    if rn >= 1 << 32:
        return "2^32"
    if reader and (so > stored_avail or stored_avail - so < sn):
        return "in_nbytes"
    if ro > raw_avail or raw_avail - ro < rn:
        return "out_avail" if reader else "in_avail"
    return None


def stream_bound(fmt, n):
    """libdeflate_<format>_compress_bound(n)"""
    return 5 * max(1, (n + 4999) // 5000) + n + {0: 0, 1: 6, 2: 18}[FORMATS.get(fmt, fmt)]


def bound(fmt, rws):
    """libdeflate_amd_shuffle_compress_bound; 0 for rows the writer refuses"""
    if any(row_why(r, False, 0, (1 << 64) - 1) for r in rws):
        return 0
    return sum(stream_bound(fmt, int(r[3])) for r in rws)


def classify(row):
    """what the reader's plan does with a row that passed the checks"""
    so, sn, ro, rn, es, mask = (int(x) for x in row)
    ident = identity(rn, es, mask)
    if mask & NO_DEFLATE:
        if sn != rn:
            return STORED_BAD
        if rn == 0:
            return STORED_EMPTY
        return STORED_COPY if ident else STORED_UNSHUFFLE
    return DECODE_DIRECT if ident else DECODE_UNSHUFFLE


def stored(raw, es, mask, compress):
    """the bytes a file stores for a chunk: compress(shuffled) unless the mask
    says which steps were skipped"""
    body = bytes(raw) if identity(len(raw), es, mask) else shuffle(raw, es)
    return body if mask & NO_DEFLATE else compress(body)
