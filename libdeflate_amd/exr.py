"""The host side of the OpenEXR calls (libdeflate_amd_exr_decode_batch,
libdeflate_amd_exr_encode_batch): parse() reads the header, the offset table
and the chunk heads of a host copy of a single-part scanline or tiled OpenEXR
file with the NONE, ZIPS or ZIP compression and makes the chunk rows the decode
call takes; build() makes the header and the offset table that go in front of
what the encode call wrote, from its index.

    im = exr.parse(buf)
    rows = im.rows(layout=binding.EXR_PIXELS, order="RGBA")   # H x W x 4 half
    dec.decode_exr_batch(rows, d_file, d_pixels, d_results)

Everything here is host arithmetic on a few hundred bytes; no pixel is touched.
The format facts are those of include/libdeflate_amd.h; no file written by the
OpenEXR library has been read yet."""
import struct

import numpy as np

from . import binding

MAGIC = b"\x76\x2f\x31\x01"
TILED, LONG_NAMES, DEEP, MULTIPART = 0x200, 0x400, 0x800, 0x1000
NONE, RLE, ZIPS, ZIP = 0, 1, 2, 3
COMPRESSIONS = ["NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"]
UINT, HALF, FLOAT = 0, 1, 2
TYPE_BYTES = {UINT: 4, HALF: 2, FLOAT: 4}
LINES_PER_CHUNK = {NONE: 1, ZIPS: 1, ZIP: 16}
# the chunk table's columns
T_HEAD_OFF, T_DATA_OFF, T_DATA_N, T_X0, T_Y0, T_W, T_LINES = range(7)


class Image:
    """one parsed file.  width, height: of the data window; channels: [(name,
    pixel type)] in the file's order; compression: 0, 2 or 3; tile: None or
    (xSize, ySize); chunks: int64 (n, 7) - the offset of the chunk's head, of
    its data, dataSize, and the chunk's x0, y0 (from the data window's corner),
    width and lines"""

    def __init__(self, width, height, channels, compression, tile, chunks, attributes):
        self.width, self.height, self.channels = width, height, channels
        self.compression, self.tile, self.chunks = compression, tile, chunks
        self.attributes = attributes

    @property
    def wide(self):
        return [TYPE_BYTES[t] == 4 for _, t in self.channels]

    @property
    def pixel_bytes(self):
        return sum(TYPE_BYTES[t] for _, t in self.channels)

    @property
    def nbytes(self):
        return self.width * self.height * self.pixel_bytes

    def slots(self, order):
        """the slot of every channel of the file for pixels whose channels
        stand in `order`: a string of one-letter names ("RGBA") or a list of
        names; None: the file's order"""
        names = [n for n, _ in self.channels]
        if order is None:
            return list(range(len(names)))
        order = list(order)
        if sorted(order) != sorted(names):
            raise ValueError("exr: order %r is not the file's channels %r" % (order, names))
        return [order.index(n) for n in names]

    def rows(self, offset=0, layout=binding.EXR_LINES, order=None, pitch=None):
        """the rows of libdeflate_amd_exr_decode_batch for a height x (width x
        pixel bytes) buffer at `offset`, lines `pitch` bytes apart (None: the
        line's bytes): every chunk at its place.  layout EXR_PIXELS gives
        height x width x channels, the channels in `order`; EXR_LINES keeps
        every chunk's line as the file has it, channel plane behind channel
        plane, at the chunk's place in the image's line."""
        from . import api
        px = self.pixel_bytes
        pitch = self.width * px if pitch is None else int(pitch)
        if layout == binding.EXR_LINES and order is not None:
            raise ValueError("exr: an order needs the PIXELS layout")
        t = self.chunks
        heads = []
        for k in range(len(t)):
            if self.tile:
                heads.append((int(t[k, T_X0]) // self.tile[0], int(t[k, T_Y0]) // self.tile[1], 0, 0))
            else:
                heads.append((int(t[k, T_Y0]) + self.attributes["dataWindow"][1],))
        return api.exr_rows(
            [offset + int(t[k, T_Y0]) * pitch + int(t[k, T_X0]) * px for k in range(len(t))],
            pitch, [(int(t[k, T_W]), int(t[k, T_LINES])) for k in range(len(t))], self.wide,
            layout, self.slots(order) if layout == binding.EXR_PIXELS else None,
            t[:, T_DATA_OFF].tolist(), t[:, T_DATA_N].tolist(), heads)


def _cstr(buf, at, limit):
    end = buf.find(b"\0", at, at + limit + 1)
    if end < 0:
        raise ValueError("exr: a name without its end at %d" % at)
    return bytes(buf[at:end]), end + 1


def _chlist(v):
    out, at = [], 0
    while True:
        if at >= len(v):
            raise ValueError("exr: the channel list has no end")
        if v[at] == 0:
            return out
        name, at = _cstr(v, at, 255)
        if at + 16 > len(v):
            raise ValueError("exr: the channel list is cut short")
        ptype, _lin, xs, ys = struct.unpack_from("<iB3xii", v, at)
        at += 16
        if ptype not in TYPE_BYTES:
            raise ValueError("exr: channel %r has pixel type %d" % (name.decode("latin-1"), ptype))
        if xs != 1 or ys != 1:
            raise ValueError("exr: channel %r is subsampled (%d x %d)" %
                             (name.decode("latin-1"), xs, ys))
        out.append((name.decode("latin-1"), ptype))


def parse(buf):
    """a single-part OpenEXR file (bytes-like, on the host) -> Image.
    ValueError names what is not covered: compressions other than NONE, ZIPS
    and ZIP, deep data, multi-part files, MIPMAP and RIPMAP tiles, subsampled
    channels - and what is broken: offsets or sizes outside the file."""
    buf = bytes(buf)
    if len(buf) < 8 or buf[:4] != MAGIC:
        raise ValueError("exr: no OpenEXR magic number")
    (version,) = struct.unpack_from("<i", buf, 4)
    if version & 0xFF != 2:
        raise ValueError("exr: version %d, not 2" % (version & 0xFF))
    if version & DEEP:
        raise ValueError("exr: deep data is not covered")
    if version & MULTIPART:
        raise ValueError("exr: multi-part files are not covered")
    if version & ~(0xFF | TILED | LONG_NAMES | DEEP | MULTIPART):
        raise ValueError("exr: unknown version flags 0x%x" % version)
    limit = 255 if version & LONG_NAMES else 31
    attrs, at = {}, 8
    while True:
        if at >= len(buf):
            raise ValueError("exr: the header has no end")
        if buf[at] == 0:
            at += 1
            break
        name, at = _cstr(buf, at, limit)
        atype, at = _cstr(buf, at, limit)
        if at + 4 > len(buf):
            raise ValueError("exr: attribute %r outside the file" % name.decode("latin-1"))
        (size,) = struct.unpack_from("<i", buf, at)
        at += 4
        if size < 0 or at + size > len(buf):
            raise ValueError("exr: attribute %r outside the file" % name.decode("latin-1"))
        attrs[name.decode("latin-1")] = (atype.decode("latin-1"), buf[at:at + size])
        at += size
    for need in ("channels", "compression", "dataWindow"):
        if need not in attrs:
            raise ValueError("exr: attribute %r is missing" % need)
    comp = attrs["compression"][1][0]
    if comp not in LINES_PER_CHUNK:
        raise ValueError("exr: compression %s is not covered (NONE, ZIPS, ZIP)" %
                         (COMPRESSIONS[comp] if comp < len(COMPRESSIONS) else comp))
    channels = _chlist(attrs["channels"][1])
    if not 1 <= len(channels) <= binding.EXR_CHANNELS_MAX:
        raise ValueError("exr: %d channels (1 .. 16)" % len(channels))
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1][:16])
    width, height = x1 - x0 + 1, y1 - y0 + 1
    if width < 1 or height < 1:
        raise ValueError("exr: an empty data window")
    px = sum(TYPE_BYTES[t] for _, t in channels)
    tile = None
    if version & TILED:
        if "tiles" not in attrs:
            raise ValueError("exr: attribute 'tiles' is missing")
        xs, ys, mode = struct.unpack("<IIB", attrs["tiles"][1][:9])
        if mode & 15:
            raise ValueError("exr: %s tiles are not covered (ONE_LEVEL)" %
                             ("MIPMAP" if mode & 15 == 1 else "RIPMAP"))
        if xs < 1 or ys < 1:
            raise ValueError("exr: an empty tile size")
        tile = (xs, ys)
        across, down = -(-width // xs), -(-height // ys)
        n = across * down
    else:
        per = LINES_PER_CHUNK[comp]
        n = -(-height // per)
    if at + 8 * n > len(buf):
        raise ValueError("exr: the offset table lies outside the file")
    offsets = struct.unpack_from("<%dQ" % n, buf, at)
    head = 20 if tile else 8
    table = np.zeros((n, 7), dtype=np.int64)
    for k, off in enumerate(offsets):
        if off + head > len(buf):
            raise ValueError("exr: chunk %d's offset %d lies outside the file" % (k, off))
        ints = struct.unpack_from("<%di" % (head // 4), buf, off)
        size = ints[-1]
        if size < 0 or off + head + size > len(buf):
            raise ValueError("exr: chunk %d's size %d lies outside the file" % (k, size))
        if tile:
            tx, ty, lx, ly = ints[:4]
            if lx or ly or not (0 <= tx < across and 0 <= ty < down):
                raise ValueError("exr: chunk %d is tile (%d, %d) of level (%d, %d)" %
                                 (k, tx, ty, lx, ly))
            cx, cy = tx * tile[0], ty * tile[1]
            cw, cl = min(tile[0], width - cx), min(tile[1], height - cy)
        else:
            cy = ints[0] - y0
            if not 0 <= cy < height or cy % per:
                raise ValueError("exr: chunk %d starts at line %d" % (k, ints[0]))
            cx, cw, cl = 0, width, min(per, height - cy)
        table[k] = (off, off + head, size, cx, cy, cw, cl)
    values = {"dataWindow": (x0, y0, x1, y1)}
    return Image(width, height, channels, comp, tile, table, values)


def _attr(name, atype, value):
    return name.encode() + b"\0" + atype.encode() + b"\0" + struct.pack("<i", len(value)) + value


def header(width, height, channels, compression, tile=None, line_order=0):
    """the bytes in front of the offset table: magic, version and attributes.
    channels: [(name, pixel type)] in the order the chunks hold them (a
    conforming file has them sorted by name)"""
    if compression not in LINES_PER_CHUNK:
        raise ValueError("exr.build: compression %r (NONE, ZIPS, ZIP)" % (compression,))
    long_names = any(len(n) > 31 for n, _ in channels)
    version = 2 | (TILED if tile else 0) | (LONG_NAMES if long_names else 0)
    chl = b"".join(n.encode("latin-1") + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1)
                   for n, t in channels) + b"\0"
    box = struct.pack("<4i", 0, 0, width - 1, height - 1)
    out = MAGIC + struct.pack("<i", version)
    out += _attr("channels", "chlist", chl)
    out += _attr("compression", "compression", bytes([compression]))
    out += _attr("dataWindow", "box2i", box)
    out += _attr("displayWindow", "box2i", box)
    out += _attr("lineOrder", "lineOrder", bytes([line_order]))
    out += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    out += _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    out += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    if tile:
        out += _attr("tiles", "tiledesc", struct.pack("<IIB", tile[0], tile[1], 0))
    return out + b"\0"


def build(width, height, channels, compression, index, tile=None):
    """the header and the offset table of a file whose chunks are what
    libdeflate_amd_exr_encode_batch wrote: index is its d_index on the host
    (chunks x EXR_WORDS; word 0 the data's offset in d_out, word 7 the head's
    length), the chunks in the file's order - scanline blocks top down, tiles
    by tile row, then tile column.  The file is build(...) + d_out[:written].
    -> bytes"""
    idx = np.asarray(index).astype(np.uint64).reshape(-1, binding.EXR_WORDS)
    per = LINES_PER_CHUNK.get(compression)
    head = header(width, height, channels, compression, tile)
    n = -(-width // tile[0]) * -(-height // tile[1]) if tile else -(-height // per)
    if len(idx) != n:
        raise ValueError("exr.build: %d index rows for %d chunks" % (len(idx), n))
    want = 20 if tile else 8
    base = len(head) + 8 * n
    table = b""
    for r in idx:
        if int(r[7]) != want:
            raise ValueError("exr.build: a chunk head of %d bytes, not %d" % (int(r[7]), want))
        table += struct.pack("<Q", base + int(r[0]) - want)
    return head + table


def assemble(width, height, channels, compression, datas, tile=None):
    """a whole file on the host from every chunk's finished data (zlib stream
    or raw chunk), in the file's order: what the tests and the fixture
    generator write with Python's zlib.  -> bytes"""
    body, idx, k = b"", [], 0
    per = LINES_PER_CHUNK[compression]
    if tile:
        coords = [(tx, ty, 0, 0) for ty in range(-(-height // tile[1]))
                  for tx in range(-(-width // tile[0]))]
    else:
        coords = [(y,) for y in range(0, height, per)]
    if len(datas) != len(coords):
        raise ValueError("exr.assemble: %d chunks of data for %d chunks" % (len(datas), len(coords)))
    for ints, data in zip(coords, datas):
        head = struct.pack("<%di" % (len(ints) + 1), *ints, len(data))
        row = [0] * binding.EXR_WORDS
        row[0], row[1], row[7] = len(body) + len(head), len(data), len(head)
        idx.append(row)
        body += head + bytes(data)
        k += 1
    return build(width, height, channels, compression, np.array(idx, dtype=np.uint64), tile) + body
