"""The chunks the shuffle tests share (tests/test_shuffle_read_gpu.py,
tests/test_shuffle_write_gpu.py): the shapes that aim at the transpose kernels'
tiles, and every shape's bytes, made once."""
import numpy as np

from tools.models import shuffle_model as sm

ELEM_SIZES = (1, 2, 3, 4, 5, 8, 16, 255, 256)


def shapes(elem_sizes=ELEM_SIZES):
    """(es, raw size): for every element size es and its tile of T =
    sm.tile_elems(es) elements, the element counts 0, 1, 2, 15, 16, 17, T - 1,
    T, T + 1 and 2 T + 1 with 0, 1 and es - 1 bytes behind the elements"""
    out = []
    for es in elem_sizes:
        t = sm.tile_elems(es)
        for ne in (0, 1, 2, 15, 16, 17, t - 1, t, t + 1, 2 * t + 1):
            for left in sorted({0, 1, es - 1}):
                if left < es:
                    out.append((es, ne * es + left))
    assert (elem_sizes[0], 0) in out    # the raw size 0
    return out


_RAW = {}


def raw_bytes(es, n):
    """n bytes, compressible and different in every plane; once per shape"""
    if (es, n) not in _RAW:
        rng = np.random.RandomState(es * 1000003 + n)
        a = rng.randint(0, 7, size=n, dtype=np.uint8) * 9
        _RAW[es, n] = (a + (np.arange(n, dtype=np.int64) % es).astype(np.uint8)).tobytes()
    return _RAW[es, n]
