"""One ZIP archive with huge entries among small ones, for the tests of
libdeflate_amd_zip_read_large: built with Python's zipfile from tests/datagen
bytes, deterministic, about 14 MiB, once per process.  The damaged copies are
patched by hand, one defect per file, on the file or on its index rows."""
import io
import struct
import zipfile
from collections import namedtuple

from tests import datagen

MIB = 1 << 20
PIECE = MIB     # LIBDEFLATE_AMD_ZIP_PIECE

# name -> (method, level, bytes); directory order, small entries in between
_SPEC = (
    ("text3m", zipfile.ZIP_DEFLATED, 6, lambda: datagen.text_chunk(3 * MIB + 17, 0x5A01)),
    ("small0", zipfile.ZIP_DEFLATED, 6, lambda: datagen.text_chunk(100, 0x5A02)),
    ("text1m", zipfile.ZIP_DEFLATED, 1, lambda: datagen.text_chunk(MIB, 0x5A03)),
    ("small1", zipfile.ZIP_STORED, None, lambda: datagen.binary_chunk(4097, 0x5A04)),
    ("text1m+1", zipfile.ZIP_DEFLATED, 6, lambda: datagen.text_chunk(MIB + 1, 0x5A05)),
    ("random", zipfile.ZIP_DEFLATED, 6, lambda: datagen.random_chunk(3 * MIB // 2, 0x5A06)),
    ("small2", zipfile.ZIP_DEFLATED, 9, lambda: datagen.lowentropy_chunk(60000, 0x5A07)),
    ("zeros", zipfile.ZIP_DEFLATED, 9, lambda: bytes(4 * MIB)),
    ("stored2m+1", zipfile.ZIP_STORED, None, lambda: datagen.text_chunk(2 * MIB + 1, 0x5A08)),
    ("small3", zipfile.ZIP_DEFLATED, 1, lambda: datagen.text_chunk(20000, 0x5A09)),
    ("stored2m", zipfile.ZIP_STORED, None, lambda: datagen.binary_chunk(2 * MIB, 0x5A0A)),
    ("empty", zipfile.ZIP_DEFLATED, 6, lambda: b""),
    ("small4", zipfile.ZIP_STORED, None, lambda: datagen.random_chunk(777, 0x5A0B)),
)
NAMES = tuple(s[0] for s in _SPEC)
SMALL = tuple(k for k, n in enumerate(NAMES) if n.startswith("small") or n == "empty")
LARGE = tuple(k for k in range(len(NAMES)) if k not in SMALL)

# data: the archive; datas: every entry's bytes as zipfile reads them back;
# infos: zipfile's infolist
Archive = namedtuple("Archive", "data infos datas")
_cache = {}


def archive():
    if "a" not in _cache:
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            for name, method, level, make in _SPEC:
                zi = zipfile.ZipInfo(name, date_time=(2024, 1, 2, 3, 4, 6))
                zi.compress_type = method
                zi._compresslevel = level
                zf.writestr(zi, make())
        data = b.getvalue()
        with zipfile.ZipFile(io.BytesIO(data)) as zf:
            infos = zf.infolist()
            datas = [zf.read(zi) for zi in infos]   # (read() checks every CRC-32)
        assert [zi.filename for zi in infos] == list(NAMES)
        _cache["a"] = Archive(data, infos, datas)
    return _cache["a"]


def entry(name):
    return NAMES.index(name)


def rows_of(a):
    """the index rows of the archive as libdeflate_amd_zip_index_batch states
    them for out_align 1, from zipfile's own fields"""
    p = a.data.rfind(b"PK\5\6")
    at = struct.unpack_from("<I", a.data, p + 16)[0]
    rows, out_off = [], 0
    for zi in a.infos:
        assert a.data[at:at + 4] == b"PK\1\2"
        n, x, c = struct.unpack_from("<HHH", a.data, at + 28)
        ln, lx = struct.unpack_from("<HH", a.data, zi.header_offset + 26)
        rows.append([at, n, zi.compress_type | zi.flag_bits << 16, zi.CRC,
                     zi.header_offset + 30 + ln + lx, zi.compress_size, zi.file_size, out_off])
        out_off += zi.file_size
        at += 46 + n + x + c
    return rows
