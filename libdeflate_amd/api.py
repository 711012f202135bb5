"""Host-side mirror of the reference interface, on top of the C-ABI.

`Compressor` / `Decompressor` follow libdeflate.h's object model (alloc with a
level, call `<format>_compress` / `<format>_decompress[_ex]`, free) with the
same argument meaning and result conventions, so parity tests read like the
reference's own (programs/test_trailing_bytes.c etc.).  The `*_batch`
functions take torch CUDA tensors that already live in HBM and only pass
their device pointers through; torch is plumbing (memory, streams), never
compute.
"""
import collections
import ctypes
import functools
from ctypes import c_size_t, c_void_p

import numpy as np

from . import binding
from .binding import FORMATS, PREFIX, check  # noqa: F401  (PREFIX: a per-stream result)


def _buf(b):
    """ctypes pointer + length for bytes / bytearray / numpy uint8."""
    if isinstance(b, np.ndarray):
        assert b.dtype == np.uint8 and b.flags["C_CONTIGUOUS"]
        return b.ctypes.data_as(c_void_p), b.size
    if isinstance(b, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(b, dtype=np.uint8)
        return arr.ctypes.data_as(c_void_p), arr.size
    raise TypeError(type(b))


# what Decompressor.read_targz returns
TarGz = collections.namedtuple("TarGz", "result nbytes seek_index windows words rows results")


class Compressor:
    """libdeflate_alloc_compressor / _free_compressor (libdeflate.h:59-160)."""

    def __init__(self, level=6):
        self._lib = binding.load()
        self.level = level
        self._h = self._lib.libdeflate_alloc_compressor(level)
        if not self._h:
            raise RuntimeError(
                f"libdeflate_alloc_compressor({level}) returned NULL: "
                f"{binding.last_error()}")

    def close(self):
        if self._h:
            self._lib.libdeflate_free_compressor(self._h)
            self._h = None

    __del__ = close

    def bound(self, fmt, n):
        if fmt == "bgzf":   # one member: gzip's bound with 8 more header bytes
            return self._lib.libdeflate_gzip_compress_bound(self._h, n) + 8
        return getattr(self._lib, f"libdeflate_{fmt}_compress_bound")(self._h, n)

    def bgzf_bound(self, n):
        """libdeflate_amd_bgzf_compress_bound: the most bytes a BGZF file of n
        input bytes takes (64 KiB per member and the EOF member)."""
        return self._lib.libdeflate_amd_bgzf_compress_bound(self._h, n)

    def compress_bgzf(self, data, index=False, eof=True, out_avail=None):
        """libdeflate_amd_bgzf_compress: host bytes -> a BGZF file (one member
        per 65280 bytes, then the EOF member unless eof=False).  Returns the
        bytes, or (bytes, index) with index=True: a numpy uint64 array of
        m + 1 rows (compressed offset, uncompressed offset), the last row the
        EOF member's (or the end's).  None when the call returns 0."""
        p, n = _buf(data)
        m = -(-n // binding.BGZF_BLOCK)
        if out_avail is None:
            out_avail = self.bgzf_bound(n)
        out = np.empty(max(out_avail, 1), dtype=np.uint8)
        idx = np.zeros(2 * (m + 1), dtype=np.uint64) if index else None
        r = self._lib.libdeflate_amd_bgzf_compress(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail,
            idx.ctypes.data_as(c_void_p) if index else None, idx.size if index else 0,
            0 if eof else binding.BGZF_NO_EOF)
        if r == 0 and (eof or n):
            return None
        if index:
            return out[:r].tobytes(), idx.reshape(m + 1, 2)
        return out[:r].tobytes()

    def compress_bgzf_batch(self, data, out, out_nbytes, index=None, eof=True,
                            stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_bgzf_compress_batch: a BGZF file of the uint8 torch
        CUDA tensor `data` (its first in_nbytes bytes) into `out` (out_avail
        bytes of it, default all); out_nbytes: int64 CUDA tensor, [0] gets the
        file's size (0: does not fit).  index: None or an int64 CUDA tensor of
        2 (m + 1) entries.  Only enqueues on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_bgzf_compress_batch(
            self._h, data.data_ptr(), n, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), out_nbytes.data_ptr(),
            index.data_ptr() if index is not None else None,
            0 if eof else binding.BGZF_NO_EOF, _stream_ptr(stream)), "bgzf_compress_batch")

    def compress_large_batch(self, fmt, data, out, out_nbytes, stream=None, in_nbytes=None,
                             out_avail=None):
        """libdeflate_amd_compress_large_batch: ONE "deflate", "zlib" or "gzip"
        stream of the uint8 torch CUDA tensor `data` (its first in_nbytes
        bytes) into `out` (out_avail bytes of it, default all), byte for byte
        what compress(fmt, ...) returns for the same bytes; bound(fmt, n) is
        room enough.  out_nbytes: int64 CUDA tensor, [0] gets the stream's
        size (0: does not fit).  Only enqueues on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_compress_large_batch(
            self._h, FORMATS[fmt], data.data_ptr() if n else None, n, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), out_nbytes.data_ptr(),
            _stream_ptr(stream)), "compress_large_batch")

    @staticmethod
    def _zip_names(names):
        """names (str -> UTF-8, or bytes) -> (blob, uint64 offsets (n + 1));
        a caller that makes many archives of the same names passes that pair
        itself and skips the encoding"""
        if isinstance(names, tuple):
            blob, offs = names
            assert blob.dtype == np.uint8 and offs.dtype == np.uint64
            return blob, offs
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
        offs = np.zeros(len(raw) + 1, dtype=np.uint64)
        if raw:
            offs[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
        return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8), offs

    def zip_bound(self, names, sizes, flags=0):
        """libdeflate_amd_zip_compress_bound: the exact upper bound of the
        archive compress_zip_batch writes for entries of these names (str or
        bytes) and sizes."""
        _, offs = self._zip_names(names)
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        assert sz.size == offs.size - 1
        return self._lib.libdeflate_amd_zip_compress_bound(
            sz.size, offs.ctypes.data_as(c_void_p), sz.ctypes.data_as(c_void_p), int(flags))

    def compress_zip_batch(self, names, data, in_offsets, in_nbytes, out, result, index=None,
                           dos_datetime=0, flags=0, stream=None, in_avail=None, out_avail=None):
        """libdeflate_amd_zip_compress_batch: a ZIP archive of the entries
        data[in_offsets[k] : + in_nbytes[k]] (data: uint8 torch CUDA tensor, its
        first in_avail bytes; names, offsets and sizes: host lists or arrays,
        names also as the (blob, offsets) pair of _zip_names())
        into `out` (out_avail bytes of it, default all; zip_bound() is room
        enough).  result: int64 CUDA tensor of ZIPW_RESULT_WORDS - [0] 0 or
        INSUFFICIENT_SPACE, [1] the archive's size, [2] cd_off, [3] entries
        deflated; index: None or an int64 CUDA tensor of ZIP_WORDS per entry,
        the rows index_zip_batch returns for the archive.  flags: ZIP_STORE,
        ZIP_FORCE_ZIP64.  Only enqueues on `stream`."""
        blob, offs = self._zip_names(names)
        ino = np.ascontiguousarray(in_offsets, dtype=np.uint64)
        inn = np.ascontiguousarray(in_nbytes, dtype=np.uint64)
        n = offs.size - 1
        assert ino.size == n and inn.size == n
        assert result.numel() >= binding.ZIPW_RESULT_WORDS
        assert index is None or index.numel() >= binding.ZIP_WORDS * n
        avail = data.numel() if in_avail is None else int(in_avail)
        check(self._lib.libdeflate_amd_zip_compress_batch(
            self._h, n, blob.ctypes.data_as(c_void_p), offs.ctypes.data_as(c_void_p),
            data.data_ptr() if avail else None, avail, ino.ctypes.data_as(c_void_p),
            inn.ctypes.data_as(c_void_p), out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), result.data_ptr(),
            index.data_ptr() if index is not None else None, int(dos_datetime), int(flags),
            _stream_ptr(stream)), "zip_compress_batch")

    @staticmethod
    def _gzm_names(names, n):
        """None, or names (str -> UTF-8, bytes, None / empty for no name) ->
        (blob, uint64 offsets (n + 1)), or that pair itself"""
        if names is None:
            return None, None
        if isinstance(names, tuple):
            return Compressor._zip_names(names)
        assert len(names) == n
        return Compressor._zip_names([b"" if x is None else x for x in names])

    def gzip_members_compress_bound(self, sizes, names=None):
        """libdeflate_amd_gzip_members_compress_bound: room enough for the file
        gzip_members_compress writes for records of these sizes and names."""
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        _, offs = self._gzm_names(names, sz.size)
        return self._lib.libdeflate_amd_gzip_members_compress_bound(
            self._h, sz.size, offs.ctypes.data_as(c_void_p) if offs is not None else None,
            sz.ctypes.data_as(c_void_p))

    def gzip_members_compress(self, records, names=None, mtime=0, out=None, result=None,
                              index=True, flags=0, stream=None, in_avail=None, out_avail=None):
        """libdeflate_amd_gzip_members_compress_batch: a file of gzip members,
        one per record.  records: (data, in_offsets, in_nbytes) - a uint8 torch
        CUDA tensor (its first in_avail bytes) and host lists or arrays; record
        k is data[in_offsets[k] : + in_nbytes[k]].  names: None, or per record
        a str, bytes or None (also the (blob, offsets) pair of _zip_names()).
        out: a uint8 CUDA tensor (out_avail bytes of it, default all), or None
        for a new one of gzip_members_compress_bound() bytes.  Returns (out,
        result, index): result an int64 CUDA tensor of GZMW_RESULT_WORDS - [0]
        0 or INSUFFICIENT_SPACE, [1] the file's size, [2] the records' bytes,
        [3] the members; index an int64 CUDA tensor of n + 1 pairs (compressed
        offset, uncompressed offset), what index_gzip_members_batch returns
        for the file, or None with index=False.  result and index may be the
        caller's tensors.  Only enqueues on `stream`: the tensors are valid in
        stream order."""
        import torch
        data, in_offsets, in_nbytes = records
        ino = np.ascontiguousarray(in_offsets, dtype=np.uint64)
        inn = np.ascontiguousarray(in_nbytes, dtype=np.uint64)
        n = inn.size
        assert ino.size == n
        blob, offs = self._gzm_names(names, n)
        assert offs is None or offs.size == n + 1
        dev = data.device
        if out is None:
            out = torch.empty(max(1, self.gzip_members_compress_bound(
                inn, (blob, offs) if offs is not None else None)), dtype=torch.uint8, device=dev)
        if result is None:
            result = torch.zeros(binding.GZMW_RESULT_WORDS, dtype=torch.int64, device=dev)
        idx = index if isinstance(index, torch.Tensor) else \
            torch.zeros((n + 1, 2), dtype=torch.int64, device=dev) if index else None
        assert result.numel() >= binding.GZMW_RESULT_WORDS
        assert idx is None or idx.numel() >= 2 * (n + 1)
        avail = data.numel() if in_avail is None else int(in_avail)
        check(self._lib.libdeflate_amd_gzip_members_compress_batch(
            self._h, n, blob.ctypes.data_as(c_void_p) if blob is not None else None,
            offs.ctypes.data_as(c_void_p) if offs is not None else None,
            data.data_ptr() if avail else None, avail, ino.ctypes.data_as(c_void_p),
            inn.ctypes.data_as(c_void_p), out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), result.data_ptr(),
            idx.data_ptr() if idx is not None else None, int(mtime), int(flags),
            _stream_ptr(stream)), "gzip_members_compress_batch")
        return out, result, idx

    def png_encode_bound(self, images):
        """libdeflate_amd_png_encode_bound: room enough for the files
        encode_png_batch writes for these image rows (png_image_rows()).  No
        device is touched; ValueError for rows the call would refuse."""
        rows = np.ascontiguousarray(images, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
        size = self._lib.libdeflate_amd_png_encode_bound(
            self._h, len(rows), rows.ctypes.data_as(c_void_p))
        if len(rows) and not size:
            raise ValueError("png_encode_bound: a row the encode call refuses")
        return size

    def encode_png_batch(self, images, data, out, result, index=None,
                         filter=binding.PNG_FILTER_ADAPTIVE, flags=0, stream=None,
                         in_avail=None, out_avail=None):
        """libdeflate_amd_png_encode_batch: one PNG file per image row, back to
        back from out[0].  images: host rows of PNG_WORDS u64 (png_image_rows(),
        or the rows of index_png_batch with words 0 and 1 replaced); data: the
        uint8 torch CUDA tensor the rows' offsets point into (its first in_avail
        bytes) - pixels as decode_png_batch writes them, PLTE and tRNS data;
        out: uint8 CUDA tensor (out_avail bytes of it, default all;
        png_encode_bound() is room enough); result: int64 CUDA tensor of
        PNGW_RESULT_WORDS - [0] 0 or INSUFFICIENT_SPACE, [1] the files' bytes,
        [2] the pixels' bytes, [3] the images; index: None or an int64 CUDA
        tensor of images x PNG_WORDS, the rows index_png_batch returns for the
        files.  filter: 0..4 or PNG_FILTER_ADAPTIVE; flags: 0 or PNG_LE16 (the
        16-bit samples in `data` are little-endian).  Only enqueues on
        `stream`."""
        rows = np.ascontiguousarray(images, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
        n = len(rows)
        assert result.numel() >= binding.PNGW_RESULT_WORDS
        assert index is None or index.numel() >= binding.PNG_WORDS * n
        avail = data.numel() if in_avail is None else int(in_avail)
        check(self._lib.libdeflate_amd_png_encode_batch(
            self._h, n, rows.ctypes.data_as(c_void_p), data.data_ptr() if avail else None,
            avail, out.data_ptr(), out.numel() if out_avail is None else int(out_avail),
            result.data_ptr(), index.data_ptr() if index is not None else None, int(filter),
            int(flags), _stream_ptr(stream)), "png_encode_batch")

    def _chunk_bound(self, call, words, rows, refuses, *fmt):
        """The body of the chunk codecs' *_bound wrappers: libdeflate_amd_<call>
        (handle, [format,] rows) over rows of `words` u64."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words)
        size = getattr(self._lib, "libdeflate_amd_" + call)(
            self._h, *fmt, len(r), r.ctypes.data_as(c_void_p))
        if len(r) and not size:
            raise ValueError(f"{call}: a row the {refuses} call refuses")
        return size

    def _chunk_encode(self, call, words, result_words, rows, data, out, result, index, stream,
                      in_avail, out_avail, *fmt):
        """The body of the chunk codecs' compress / encode wrappers:
        libdeflate_amd_<call>(handle, [format,] rows, data, out, result, index,
        stream).  An empty `data` goes as NULL."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words)
        assert result.numel() >= result_words
        assert index is None or index.numel() >= words * len(r)
        avail = data.numel() if in_avail is None else int(in_avail)
        check(getattr(self._lib, "libdeflate_amd_" + call)(
            self._h, *fmt, len(r), r.ctypes.data_as(c_void_p),
            data.data_ptr() if avail else None, avail, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), result.data_ptr(),
            index.data_ptr() if index is not None else None, _stream_ptr(stream)), call)
        return r

    def shuffle_compress_bound(self, fmt, rows):
        """libdeflate_amd_shuffle_compress_bound: room enough for the streams
        compress_shuffle_batch writes for these rows (shuffle_rows()).  No
        device is touched; ValueError for rows the call would refuse."""
        return self._chunk_bound("shuffle_compress_bound", binding.SHUF_WORDS, rows, "compress",
                                 FORMATS[fmt])

    def compress_shuffle_batch(self, fmt, rows, data, out, result, index=None, stream=None,
                               in_avail=None, out_avail=None):
        """libdeflate_amd_shuffle_compress_batch: every chunk of `data` (uint8
        CUDA tensor; rows: shuffle_rows(), words 2 to 5) byte-shuffled and
        compressed into one stream of `fmt`, the streams back to back from
        out[0].  result: int64 CUDA tensor of SHUFW_RESULT_WORDS - [0] 0 or
        INSUFFICIENT_SPACE, [1] the streams' bytes, [2] the raw bytes, [3] the
        chunks; index: None or an int64 CUDA tensor of chunks x SHUF_WORDS, the
        rows decompress_shuffle_batch takes for `out`.  Returns the rows as
        passed (numpy uint64).  Only enqueues on `stream`."""
        return self._chunk_encode("shuffle_compress_batch", binding.SHUF_WORDS,
                                  binding.SHUFW_RESULT_WORDS, rows, data, out, result, index,
                                  stream, in_avail, out_avail, FORMATS[fmt])

    def tiff_encode_bound(self, rows):
        """libdeflate_amd_tiff_encode_bound: room enough for the streams
        encode_tiff_batch writes for these rows (tiff_rows()).  No device is
        touched; ValueError for rows the call would refuse."""
        return self._chunk_bound("tiff_encode_bound", binding.TIFF_WORDS, rows, "encode")

    def encode_tiff_batch(self, rows, data, out, result, index=None, stream=None,
                          in_avail=None, out_avail=None):
        """libdeflate_amd_tiff_encode_batch: every segment (strip or tile) of
        the pixels in `data` (uint8 CUDA tensor; rows: tiff_rows(), words 2 to
        7) padded to its coded size, predicted and compressed into one zlib
        stream, the streams back to back from out[0].  result: int64 CUDA
        tensor of TIFFW_RESULT_WORDS - [0] 0 or INSUFFICIENT_SPACE, [1] the
        streams' bytes, [2] the kept bytes, [3] the segments; index: None or
        an int64 CUDA tensor of segments x TIFF_WORDS, the rows
        decode_tiff_batch takes for `out`.  Returns the rows as passed (numpy
        uint64).  Only enqueues on `stream`."""
        return self._chunk_encode("tiff_encode_batch", binding.TIFF_WORDS,
                                  binding.TIFFW_RESULT_WORDS, rows, data, out, result, index,
                                  stream, in_avail, out_avail)

    def exr_encode_bound(self, rows):
        """libdeflate_amd_exr_encode_bound: the sum of head + raw size over the
        rows (exr_rows()), which nothing encode_exr_batch writes exceeds.  No
        device is touched; ValueError for rows the call would refuse."""
        return self._chunk_bound("exr_encode_bound", binding.EXR_WORDS, rows, "encode")

    def encode_exr_batch(self, rows, data, out, result, index=None, stream=None,
                         in_avail=None, out_avail=None):
        """libdeflate_amd_exr_encode_batch: every chunk (scanline block or
        tile) of the pixels in `data` (uint8 CUDA tensor; rows: exr_rows(),
        words 2 to 9) gathered, coded and compressed, and written as head,
        dataSize and data - the zlib stream where it is shorter than the raw
        chunk, else the raw chunk - back to back from out[0].  result: int64
        CUDA tensor of EXRW_RESULT_WORDS - [0] 0 or INSUFFICIENT_SPACE, [1]
        the bytes written, [2] the raw bytes, [3] the chunks; index: None or
        an int64 CUDA tensor of chunks x EXR_WORDS, the rows decode_exr_batch
        takes for `out`.  Returns the rows as passed (numpy uint64).  Only
        enqueues on `stream`."""
        return self._chunk_encode("exr_encode_batch", binding.EXR_WORDS,
                                  binding.EXRW_RESULT_WORDS, rows, data, out, result, index,
                                  stream, in_avail, out_avail)

    def tar_write_size(self, names, sizes):
        """libdeflate_amd_tar_write_size: the exact size of the tar archive
        write_tar_batch writes for entries of these names (str or bytes, or
        the (blob, offsets) pair of _zip_names()) and sizes.  No device is
        touched."""
        blob, offs = self._zip_names(names)
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        assert sz.size == offs.size - 1
        size = self._lib.libdeflate_amd_tar_write_size(
            sz.size, offs.ctypes.data_as(c_void_p), blob.ctypes.data_as(c_void_p),
            sz.ctypes.data_as(c_void_p))
        if not size:
            raise ValueError(binding.last_error())
        return size

    def _tar_entries(self, names, data, in_offsets, in_nbytes, index, in_avail):
        blob, offs = self._zip_names(names)
        ino = np.ascontiguousarray(in_offsets, dtype=np.uint64)
        inn = np.ascontiguousarray(in_nbytes, dtype=np.uint64)
        n = offs.size - 1
        assert ino.size == n and inn.size == n
        rows = np.zeros((n, binding.TAR_WORDS), dtype=np.uint64) if index else None
        avail = data.numel() if in_avail is None else int(in_avail)
        args = (n, blob.ctypes.data_as(c_void_p), offs.ctypes.data_as(c_void_p),
                data.data_ptr() if avail else None, avail, ino.ctypes.data_as(c_void_p),
                inn.ctypes.data_as(c_void_p))
        # (the arrays stay alive with the tuple until the call has returned)
        return args, (blob, offs, ino, inn), rows

    def write_tar_batch(self, names, data, in_offsets, in_nbytes, out, index=True, mtime=0,
                        flags=0, stream=None, in_avail=None, out_avail=None):
        """libdeflate_amd_tar_write_batch: a tar archive (pax format, byte for
        byte tarfile's) of the entries data[in_offsets[k] : + in_nbytes[k]]
        (data: uint8 torch CUDA tensor, its first in_avail bytes; names,
        offsets and sizes: host lists or arrays, names also as the (blob,
        offsets) pair of _zip_names()) into out[:tar_write_size()] (out_avail
        bytes of `out` are there, default all).  Returns the index rows
        (numpy uint64, entries x TAR_WORDS: what index_tar_batch returns for
        the archive, ready for read_tar_batch and tar_ranges), or None with
        index=False.  Only enqueues on `stream`."""
        args, keep, rows = self._tar_entries(names, data, in_offsets, in_nbytes, index, in_avail)
        check(self._lib.libdeflate_amd_tar_write_batch(
            self._h, *args, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail),
            rows.ctypes.data_as(c_void_p) if rows is not None else None, int(mtime),
            int(flags), _stream_ptr(stream)), "tar_write_batch")
        del keep
        return rows

    def compress_targz_batch(self, fmt, names, data, in_offsets, in_nbytes, out, out_nbytes,
                             index=True, mtime=0, flags=0, stream=None, in_avail=None,
                             out_avail=None):
        """libdeflate_amd_targz_compress_batch: the archive write_tar_batch
        writes for these entries, compressed into ONE "gzip", "zlib" or
        "deflate" stream in `out` (out_avail bytes of it, default all;
        bound(fmt, tar_write_size()) is room enough) - byte for byte what
        compress_large_batch gives for the archive.  out_nbytes: int64 CUDA
        tensor, [0] gets the stream's size (0: does not fit).  Returns the
        archive's index rows as write_tar_batch does.  Only enqueues."""
        args, keep, rows = self._tar_entries(names, data, in_offsets, in_nbytes, index, in_avail)
        check(self._lib.libdeflate_amd_targz_compress_batch(
            self._h, FORMATS[fmt], *args, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), out_nbytes.data_ptr(),
            rows.ctypes.data_as(c_void_p) if rows is not None else None, int(mtime),
            int(flags), _stream_ptr(stream)), "targz_compress_batch")
        del keep
        return rows

    def compress(self, fmt, data, out_avail=None):
        """Returns the compressed bytes, or None when the reference API would
        return 0 (does not fit in out_avail)."""
        p, n = _buf(data)
        if out_avail is None:
            out_avail = self.bound(fmt, n)
        out = np.empty(max(out_avail, 1), dtype=np.uint8)
        r = getattr(self._lib, f"libdeflate_{fmt}_compress")(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail)
        if r == 0:
            return None
        return out[:r].tobytes()

    def compress_batch(self, fmt, data, in_offsets, in_nbytes, out,
                       out_offsets, out_avail, out_nbytes, stream=None,
                       max_chunk=None):
        """Device batch: all arguments are torch CUDA tensors (uint8 data,
        int64 descriptors).  Enqueues on `stream` (torch stream or None).
        max_chunk: an upper bound of the chunk sizes, if the caller knows one
        (libdeflate_amd_compress_batch_bounded: small chunks get their own
        kernel, and at levels 0-9 large batches split the block end off into
        a kernel of its own).  Only a bound <= 4096 is enforced: a chunk above
        it reports 0; above any larger bound a chunk is still compressed."""
        if max_chunk is None:
            check(self._lib.libdeflate_amd_compress_batch(
                self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
                in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
                out_offsets.data_ptr(), out_avail.data_ptr(),
                out_nbytes.data_ptr(), _stream_ptr(stream)), "compress_batch")
        else:
            check(self._lib.libdeflate_amd_compress_batch_bounded(
                self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
                in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
                out_offsets.data_ptr(), out_avail.data_ptr(),
                out_nbytes.data_ptr(), int(max_chunk), _stream_ptr(stream)),
                "compress_batch_bounded")

    def last_schedule(self):
        """libdeflate_amd_compress_last_schedule: how the last batch call on
        this object was scheduled -> dict(split, overlapped, head, tail)."""
        return binding.compress_last_schedule(self._h)

    def last_kernel(self):
        """libdeflate_amd_compress_last_kernel: the name of the compress kernel
        the last batch call on this object launched (on the split path the
        LZ77 stage: the level's own instance or the generic kernel)."""
        return binding.compress_last_kernel(self._h)

    def compress_dict(self, fmt, dictionary, data, out_avail=None):
        """libdeflate_amd_compress_dict: one host buffer with a preset
        dictionary ("deflate" or "zlib").  Returns the compressed bytes, or
        None when the call returns 0 (does not fit, or a bad argument)."""
        p, n = _buf(data)
        dp, dn = _buf(dictionary)
        if out_avail is None:
            out_avail = self.bound(fmt, n) + 4     # + DICTID
        out = np.empty(max(out_avail, 1), dtype=np.uint8)
        r = self._lib.libdeflate_amd_compress_dict(
            self._h, FORMATS[fmt], dp, dn, p, n, out.ctypes.data_as(c_void_p), out_avail)
        if r == 0:
            return None
        return out[:r].tobytes()

    def compress_batch_dict(self, fmt, dictionary, data, in_offsets, in_nbytes, out,
                            out_offsets, out_avail, out_nbytes, stream=None):
        """Device batch with one preset dictionary for every chunk
        (libdeflate_amd_compress_batch_dict): `dictionary` is a uint8 torch
        CUDA tensor, the rest as in compress_batch."""
        check(self._lib.libdeflate_amd_compress_batch_dict(
            self._h, FORMATS[fmt], in_offsets.numel(),
            dictionary.data_ptr() if dictionary.numel() else None, dictionary.numel(),
            data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr(), out_avail.data_ptr(), out_nbytes.data_ptr(),
            _stream_ptr(stream)), "compress_batch_dict")

    def compress_batch_host(self, fmt, chunks, out_avail=None):
        """List of bytes -> list of compressed bytes (None where it did not
        fit), through libdeflate_amd_compress_batch_host."""
        n = len(chunks)
        arrs = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
        avail = [self.bound(fmt, a.size) if out_avail is None else out_avail[i]
                 for i, a in enumerate(arrs)]
        outs = [np.empty(max(a, 1), dtype=np.uint8) for a in avail]
        inp = (c_void_p * n)(*[a.ctypes.data for a in arrs])
        inn = (c_size_t * n)(*[a.size for a in arrs])
        outp = (c_void_p * n)(*[o.ctypes.data for o in outs])
        outa = (c_size_t * n)(*avail)
        outn = (c_size_t * n)()
        check(self._lib.libdeflate_amd_compress_batch_host(
            self._h, FORMATS[fmt], n, inp, inn, outp, outa, outn),
            "compress_batch_host")
        return [outs[i][:outn[i]].tobytes() if outn[i] else None
                for i in range(n)]


class Decompressor:
    """libdeflate_alloc_decompressor / _free (libdeflate.h:181-323)."""

    def __init__(self):
        self._lib = binding.load()
        self._h = self._lib.libdeflate_alloc_decompressor()
        if not self._h:
            raise RuntimeError("libdeflate_alloc_decompressor returned NULL: "
                               + binding.last_error())

    def close(self):
        if self._h:
            self._lib.libdeflate_free_decompressor(self._h)
            self._h = None

    __del__ = close

    def decompress_ex(self, fmt, data, out_avail, want_actual_out=True):
        """-> (result, actual_in, actual_out, out_bytes) with the semantics of
        libdeflate_<fmt>_decompress_ex; want_actual_out=False passes NULL for
        actual_out_nbytes_ret (exact-fill mode)."""
        p, n = _buf(data)
        out = np.zeros(max(out_avail, 1), dtype=np.uint8)
        ai, ao = c_size_t(0), c_size_t(0)
        r = getattr(self._lib, f"libdeflate_{fmt}_decompress_ex")(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail,
            ctypes.byref(ai), ctypes.byref(ao) if want_actual_out else None)
        nout = ao.value if want_actual_out else out_avail
        return r, ai.value, ao.value, out[:nout].tobytes()

    def decompress_dict_ex(self, fmt, dictionary, data, out_avail, want_actual_out=True):
        """libdeflate_amd_decompress_dict_ex -> (result, actual_in,
        actual_out, out_bytes), like decompress_ex."""
        p, n = _buf(data)
        dp, dn = _buf(dictionary)
        out = np.zeros(max(out_avail, 1), dtype=np.uint8)
        ai, ao = c_size_t(0), c_size_t(0)
        r = self._lib.libdeflate_amd_decompress_dict_ex(
            self._h, FORMATS[fmt], dp, dn, p, n, out.ctypes.data_as(c_void_p), out_avail,
            ctypes.byref(ai), ctypes.byref(ao) if want_actual_out else None)
        nout = ao.value if want_actual_out else out_avail
        return r, ai.value, ao.value, out[:nout].tobytes()

    def decompress(self, fmt, data, out_avail, want_actual_out=True):
        p, n = _buf(data)
        out = np.zeros(max(out_avail, 1), dtype=np.uint8)
        ao = c_size_t(0)
        r = getattr(self._lib, f"libdeflate_{fmt}_decompress")(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail,
            ctypes.byref(ao) if want_actual_out else None)
        nout = ao.value if want_actual_out else out_avail
        return r, ao.value, out[:nout].tobytes()

    def gzip_decompress_members(self, data, out_avail):
        """All members of a multi-member gzip buffer (the loop of
        programs/gzip.c:236-299 in one call) -> (result, actual_in,
        actual_out, members, bytes)."""
        p, n = _buf(data)
        out = np.zeros(max(out_avail, 1), dtype=np.uint8)
        ai, ao, nm = c_size_t(0), c_size_t(0), c_size_t(0)
        r = self._lib.libdeflate_amd_gzip_decompress_members(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail,
            ctypes.byref(ai), ctypes.byref(ao), ctypes.byref(nm))
        return r, ai.value, ao.value, nm.value, out[:ao.value].tobytes()

    def decompress_bgzf_batch(self, data, max_members, out, result, index=None, stream=None,
                              in_nbytes=None, out_avail=None):
        """libdeflate_amd_bgzf_decompress_batch: the BGZF file in the uint8
        torch CUDA tensor `data` (its first in_nbytes bytes) into `out`
        (out_avail bytes of it, default all).  result: int64 CUDA tensor of 5
        (verdict, members, compressed bytes, uncompressed bytes, flags);
        index: None or an int64 CUDA tensor of 2 (max_members + 1).  Only
        enqueues on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_bgzf_decompress_batch(
            self._h, data.data_ptr(), n, int(max_members), out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), result.data_ptr(),
            index.data_ptr() if index is not None else None, _stream_ptr(stream)),
            "bgzf_decompress_batch")

    def index_bgzf_batch(self, data, max_members, result, index=None, stream=None,
                         in_nbytes=None):
        """libdeflate_amd_bgzf_index_batch: result and index as in
        decompress_bgzf_batch; nothing is decoded."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_bgzf_index_batch(
            self._h, data.data_ptr(), n, int(max_members), result.data_ptr(),
            index.data_ptr() if index is not None else None, _stream_ptr(stream)),
            "bgzf_index_batch")

    def decompress_gzip_members_batch(self, data, max_members, out, result, index=None,
                                      stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_gzip_members_decompress_batch: the file of
        concatenated gzip members in the uint8 torch CUDA tensor `data` (its
        first in_nbytes bytes) into `out` (out_avail bytes of it, default
        all).  result: int64 CUDA tensor of 5 (verdict, members, compressed
        bytes, uncompressed bytes, 0); index: None or an int64 CUDA tensor of
        2 (max_members + 1).  Only enqueues on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_gzip_members_decompress_batch(
            self._h, data.data_ptr() if n else None, n, int(max_members),
            out.data_ptr() if avail else None, avail, result.data_ptr(),
            index.data_ptr() if index is not None else None, _stream_ptr(stream)),
            "gzip_members_decompress_batch")

    def index_gzip_members_batch(self, data, max_members, result, index=None, stream=None,
                                 in_nbytes=None):
        """libdeflate_amd_gzip_members_index_batch: result and index as in
        decompress_gzip_members_batch; nothing is decoded."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_gzip_members_index_batch(
            self._h, data.data_ptr() if n else None, n, int(max_members), result.data_ptr(),
            index.data_ptr() if index is not None else None, _stream_ptr(stream)),
            "gzip_members_index_batch")

    def index_zip_batch(self, data, max_entries, result, results, index=None, out_align=1,
                        stream=None, in_nbytes=None):
        """libdeflate_amd_zip_index_batch: the ZIP archive in the uint8 torch
        CUDA tensor `data` (its first in_nbytes bytes) -> result: int64 CUDA
        tensor of 5 (verdict, entries, cd_off, bytes of output needed, flags);
        results: int32 CUDA tensor of max_entries (per-entry pre-decode
        results); index: None or an int64 CUDA tensor of 8 max_entries (rows
        of central record, name_len, method | flags << 16, CRC-32, data_off,
        csize, usize, out_off).  Nothing is decoded.  Only enqueues."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_zip_index_batch(
            self._h, data.data_ptr() if n else None, n, int(max_entries), int(out_align),
            result.data_ptr(), index.data_ptr() if index is not None else None,
            results.data_ptr(), _stream_ptr(stream)), "zip_index_batch")

    def decompress_zip_batch(self, data, max_entries, out, result, results, index=None,
                             out_align=1, stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_zip_decompress_batch: every entry of the ZIP archive
        in `data` into `out` (out_avail bytes of it, default all), entry k at
        out_off of row k; result, results and index as in index_zip_batch,
        results with the decode's and the CRC-32's verdicts.  Only enqueues
        on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_zip_decompress_batch(
            self._h, data.data_ptr() if n else None, n, int(max_entries),
            out.data_ptr() if avail else None, avail, int(out_align), result.data_ptr(),
            index.data_ptr() if index is not None else None, results.data_ptr(),
            _stream_ptr(stream)), "zip_decompress_batch")

    def read_zip_batch(self, data, index, sel, out, results, out_align=1, stream=None,
                       in_nbytes=None, out_avail=None):
        """libdeflate_amd_zip_read_batch: the entries `sel` (host, any order,
        duplicates allowed) of the archive in the CUDA tensor `data`, back to
        back into `out` with out_align; index: host rows as index_zip_batch
        wrote them; results: int32 CUDA tensor, one per selection.  Returns
        the numpy uint64 offsets (len(sel) + 1) of the selections in `out`.
        Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.ZIP_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_zip_read_batch(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), out.data_ptr() if avail else None, avail,
            int(out_align), offs.ctypes.data_as(c_void_p), results.data_ptr(),
            _stream_ptr(stream)), "zip_read_batch")
        return offs

    def read_zip_large(self, data, index, sel, out, results, out_align=1, large_min=0,
                       stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_zip_read_large: read_zip_batch for archives with a
        few huge entries - the same arguments, offsets, results and bytes.  A
        deflated entry of large_min compressed bytes and more (0: the
        library's default, LDA_ZIP_LARGE_MIN) is decoded on many waves, an
        entry above binding.ZIP_PIECE bytes is copied and checksummed in
        pieces.  BLOCKS while the many-wave entries decode; everything else
        is enqueued on `stream`."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.ZIP_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_zip_read_large(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), out.data_ptr() if avail else None, avail,
            int(out_align), int(large_min), offs.ctypes.data_as(c_void_p), results.data_ptr(),
            _stream_ptr(stream)), "zip_read_large")
        return offs

    def index_tar_batch(self, data, max_records, result, results, index=None, out_align=1,
                        stream=None, in_nbytes=None):
        """libdeflate_amd_tar_index_batch: the tar archive in the uint8 torch
        CUDA tensor `data` (its first in_nbytes bytes) -> result: int64 CUDA
        tensor of 5 (verdict, entries, the offset where the walk ended, bytes
        of output needed, flags); results: int32 CUDA tensor of max_records
        (per-entry results); index: None or an int64 CUDA tensor of 8
        max_records (rows of header, name_off, name_len | prefix_len << 32,
        typeflag | name source << 8, data_off, usize, mtime, out_off).
        max_records bounds entries and extension records together.  Nothing
        is copied.  Only enqueues."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_tar_index_batch(
            self._h, data.data_ptr() if n else None, n, int(max_records), int(out_align),
            result.data_ptr(), index.data_ptr() if index is not None else None,
            results.data_ptr(), _stream_ptr(stream)), "tar_index_batch")

    def extract_tar_batch(self, data, max_records, out, result, results, index=None,
                          out_align=1, stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_tar_extract_batch: every entry of the tar archive in
        `data` into `out` (out_avail bytes of it, default all), entry k at
        out_off of row k; result, results and index as in index_tar_batch.
        Only enqueues on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_tar_extract_batch(
            self._h, data.data_ptr() if n else None, n, int(max_records),
            out.data_ptr() if avail else None, avail, int(out_align), result.data_ptr(),
            index.data_ptr() if index is not None else None, results.data_ptr(),
            _stream_ptr(stream)), "tar_extract_batch")

    def read_tar_batch(self, data, index, sel, out, results, out_align=1, stream=None,
                       in_nbytes=None, out_avail=None):
        """libdeflate_amd_tar_read_batch: the entries `sel` (host, any order,
        duplicates allowed) of the archive in the CUDA tensor `data`, back to
        back into `out` with out_align; index: host rows as index_tar_batch
        wrote them; results: int32 CUDA tensor, one per selection.  Returns
        the numpy uint64 offsets (len(sel) + 1) of the selections in `out`.
        Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.TAR_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_tar_read_batch(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), out.data_ptr() if avail else None, avail,
            int(out_align), offs.ctypes.data_as(c_void_p), results.data_ptr(),
            _stream_ptr(stream)), "tar_read_batch")
        return offs

    def index_png_batch(self, data, in_offsets, in_nbytes, index, results, stream=None):
        """libdeflate_amd_png_index_batch: the PNG files data[in_offsets[k] :
        + in_nbytes[k]] (uint8 CUDA tensor; int64 CUDA tensors) -> index: int64
        CUDA tensor of 8 per file (rows of file offset, file nbytes, width |
        height << 32, depth | colour << 8 | interlace << 16 | filter unit << 24
        | channels << 32, first IDAT, IDAT bytes, PLTE, tRNS; zero beyond the
        first two words for a refused file); results: int32 CUDA tensor, one
        per file (0, BAD_DATA, PNG_UNSUPPORTED).  Only enqueues."""
        n = in_offsets.numel()
        check(self._lib.libdeflate_amd_png_index_batch(
            self._h, n, data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(),
            index.data_ptr(), results.data_ptr(), _stream_ptr(stream)), "png_index_batch")

    def decode_png_batch(self, data, index, sel, out, results, out_align=1, flags=0,
                         stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_png_decode_batch: the images `sel` (host, any order,
        duplicates allowed) of the files in the CUDA tensor `data`, back to
        back into `out` with out_align: height rows of rowbytes bytes each, no
        filter bytes; index: host rows as index_png_batch wrote them; results:
        int32 CUDA tensor, one per selection; flags: 0 or binding.PNG_LE16
        (16-bit samples little-endian).  Returns the numpy uint64 offsets
        (len(sel) + 1) of the selections in `out`; png_shapes(index) gives the
        shapes to view them with.  Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_png_decode_batch(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), out.data_ptr() if avail else None, avail,
            int(out_align), int(flags), offs.ctypes.data_as(c_void_p), results.data_ptr(),
            _stream_ptr(stream)), "png_decode_batch")
        return offs

    def decode_png_pixels_batch(self, data, index, sel, out, results, fmt, out_align=1, flags=0,
                                stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_png_decode_pixels_batch: decode_png_batch, and every
        image expanded to ONE pixel format whatever its file stores: fmt is
        binding.PNG_GRAY, PNG_GRAY_ALPHA, PNG_RGB or PNG_RGBA, alone (uint8
        samples) or with PNG_OUT16 (16-bit, big-endian unless flags has
        PNG_LE16).  Palette and tRNS are applied, depths scaled, grey
        replicated or RGB weighted to grey, alpha dropped where fmt has none.
        Selection r is height x width x channels interleaved at out[offsets[r]];
        png_pixels_shapes(index, fmt) gives the shapes and the dtype.  Returns
        the numpy uint64 offsets (len(sel) + 1).  Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_png_decode_pixels_batch(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), int(fmt), out.data_ptr() if avail else None,
            avail, int(out_align), int(flags), offs.ctypes.data_as(c_void_p),
            results.data_ptr(), _stream_ptr(stream)), "png_decode_pixels_batch")
        return offs

    def index_png_batch_ex(self, data, in_offsets, in_nbytes, index, results, flags=0,
                           stream=None):
        """libdeflate_amd_png_index_batch_ex: index_png_batch with flags.  0:
        its rows and results exactly; binding.PNG_ADAM7: an Adam7-interlaced
        file that passes every other rule is a full row (bit 16 of word 3 set)
        and result 0, PNG_UNSUPPORTED only where the image or the bytes its
        stream inflates to reach 2^32.  Only enqueues."""
        n = in_offsets.numel()
        check(self._lib.libdeflate_amd_png_index_batch_ex(
            self._h, n, data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(), int(flags),
            index.data_ptr(), results.data_ptr(), _stream_ptr(stream)), "png_index_batch_ex")

    def decode_png_batch_ex(self, data, index, sel, out, results, fmt=0, out_align=1, flags=0,
                            stream=None, in_nbytes=None, out_avail=None):
        """libdeflate_amd_png_decode_batch_ex: fmt 0 is decode_png_batch's
        layout (height rows of rowbytes bytes as PNG stores them), any other
        fmt decode_png_pixels_batch's; flags: binding.PNG_LE16 |
        binding.PNG_ADAM7.  With PNG_ADAM7 the selection may hold interlaced
        rows of index_png_batch_ex among plain ones, zero rows and duplicates;
        an interlaced image's bytes are those of its non-interlaced twin.
        Returns the numpy uint64 offsets (len(sel) + 1); png_shapes(index) or
        png_pixels_shapes(index, fmt) gives the shapes.  Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
        s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
        offs = np.zeros(len(s) + 1, dtype=np.uint64)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_png_decode_batch_ex(
            self._h, data.data_ptr() if n else None, n, idx.ctypes.data_as(c_void_p), len(idx),
            len(s), s.ctypes.data_as(c_void_p), int(fmt), out.data_ptr() if avail else None,
            avail, int(out_align), int(flags), offs.ctypes.data_as(c_void_p),
            results.data_ptr(), _stream_ptr(stream)), "png_decode_batch_ex")
        return offs

    def read_targz(self, data, out, max_records, spacing=1 << 20, max_points=1024,
                   in_nbytes=None, out_avail=None, stream=None):
        """A .tar.gz in the CUDA tensor `data`: decompress_large_index("gzip")
        into `out`, then index_tar_batch on the decoded bytes -> TarGz(result,
        nbytes, seek_index, windows, words, rows, results): the gzip result
        and the archive's size, the seek index and its windows, and on the
        host the five words, the index rows (numpy uint64, entries x 8) and
        the per-entry results of the tar index (None unless result is 0).
        Any selection is then read from the compressed bytes with
        read_targz_entries.  Blocks."""
        import torch
        r, _, nbytes, seek_index, windows = self.decompress_large_index(
            "gzip", data, out, spacing, max_points, in_nbytes=in_nbytes, out_avail=out_avail,
            stream=stream)
        if r != 0:
            return TarGz(r, nbytes, None, None, None, None, None)
        m = int(max_records)
        res = torch.zeros(binding.TAR_RESULT_WORDS, dtype=torch.int64, device=data.device)
        idx = torch.zeros(binding.TAR_WORDS * m, dtype=torch.int64, device=data.device)
        per = torch.zeros(m, dtype=torch.int32, device=data.device)
        self.index_tar_batch(out, m, res, per, index=idx, stream=stream, in_nbytes=nbytes)
        words = [int(x) for x in res.cpu().tolist()]    # (waits for the stream's work)
        known = words[0] not in (binding.BAD_DATA, binding.TAR_MORE_RECORDS,
                                 binding.TAR_MORE_CANDIDATES)
        entries = words[1] if known else 0
        rows = idx.cpu().numpy().astype(np.uint64).reshape(-1, binding.TAR_WORDS)[:entries]
        return TarGz(r, nbytes, seek_index, windows, words, rows, per.cpu().numpy()[:entries])

    def read_targz_entries(self, data, targz, sel, out, results, stream=None, in_nbytes=None,
                           out_avail=None):
        """The entries `sel` of the .tar.gz in `data` out of its compressed
        bytes: tar_ranges of the rows read_targz returned, then
        seek_read_batch through its seek index, back to back into `out`;
        results: int32 CUDA tensor, one per selection.  Returns the numpy
        uint64 offsets (len(sel) + 1) in `out`.  Only enqueues."""
        rng, _ = tar_ranges(targz.rows, sel)
        self.seek_read_batch(data, targz.seek_index, targz.windows, rng, out, results,
                             stream=stream, in_nbytes=in_nbytes, out_avail=out_avail)
        return np.concatenate(([0], np.cumsum(rng[:, 1]))).astype(np.uint64)

    def read_bgzf_batch(self, data, index, ranges, out, results, voffsets=False, stream=None,
                        in_nbytes=None, out_avail=None):
        """libdeflate_amd_bgzf_read_batch: `ranges` (host, rows of (begin,
        nbytes), or of (v_begin, v_end) with voffsets=True) of the file in the
        CUDA tensor `data`, back to back into `out`; index: host rows
        (compressed, uncompressed offset) of every member and the closing
        row; results: int32 CUDA tensor, one per range.  Only enqueues."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, 2)
        rng = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_bgzf_read_batch(
            self._h, data.data_ptr(), n, idx.ctypes.data_as(c_void_p), len(idx) - 1,
            len(rng), rng.ctypes.data_as(c_void_p),
            binding.BGZF_VOFFSETS if voffsets else 0, out.data_ptr(),
            out.numel() if out_avail is None else int(out_avail), results.data_ptr(),
            _stream_ptr(stream)), "bgzf_read_batch")

    def decompress_bgzf(self, data, out_avail, index=False, index_avail=None):
        """libdeflate_amd_bgzf_decompress: a BGZF file in host memory ->
        (result, bytes, members, flags), or with index=True (result, bytes,
        members, flags, rows): numpy uint64 rows (compressed, uncompressed
        offset) of every member and the closing row."""
        p, n = _buf(data)
        out = np.zeros(max(out_avail, 1), dtype=np.uint8)
        ao, nm, fl = c_size_t(0), c_size_t(0), ctypes.c_uint32(0)
        if index and index_avail is None:
            index_avail = 2 * (n // 28 + 2)
        idx = np.zeros(max(index_avail, 1), dtype=np.uint64) if index else None
        r = self._lib.libdeflate_amd_bgzf_decompress(
            self._h, p, n, out.ctypes.data_as(c_void_p), out_avail, ctypes.byref(ao),
            ctypes.byref(nm), idx.ctypes.data_as(c_void_p) if index else None,
            index_avail if index else 0, ctypes.byref(fl))
        got = out[:ao.value].tobytes() if r == 0 else b""
        if index:
            rows = idx[:2 * (nm.value + 1)].reshape(-1, 2) if r == 0 else None
            return r, got, nm.value, fl.value, rows
        return r, got, nm.value, fl.value

    def decompress_large(self, fmt, data, out, in_nbytes=None, out_avail=None,
                         want_actual_out=True, stream=None):
        """libdeflate_amd_decompress_large: ONE "deflate", "zlib" or "gzip"
        stream in the uint8 torch CUDA tensor `data` (its first in_nbytes
        bytes) into the uint8 CUDA tensor `out` (out_avail bytes of it,
        default all), on many waves, with the results of decompress_ex ->
        (result, actual_in, actual_out); want_actual_out=False asks for an
        exact fill.  Blocks; ordered behind what is queued on `stream`."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        ai, ao = c_size_t(0), c_size_t(0)
        r = self._lib.libdeflate_amd_decompress_large(
            self._h, FORMATS[fmt], data.data_ptr() if n else None, n,
            out.data_ptr() if avail else None, avail, ctypes.byref(ai),
            ctypes.byref(ao) if want_actual_out else None, _stream_ptr(stream))
        return r, ai.value, ao.value

    def decompress_large_index(self, fmt, data, out, spacing, max_points, in_nbytes=None,
                               out_avail=None, want_actual_out=True, stream=None):
        """libdeflate_amd_decompress_large_index: decompress_large, and a
        seek index over the stream with a point about every `spacing` bytes
        of output, at most max_points of them (the spacing is doubled until
        they fit) -> (result, actual_in, actual_out, index, windows): index
        is a numpy uint64 array of rows of 4 (header row, the points, closing
        row; None unless result is 0), windows the uint8 CUDA tensor of
        32768 bytes per point that read through it.  Blocks."""
        import torch
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        max_points = int(max_points)
        idx = np.zeros(binding.SEEK_WORDS * (max(max_points, 0) + 2), dtype=np.uint64)
        win = torch.empty(max(max_points, 0) * binding.SEEK_WINDOW, dtype=torch.uint8,
                          device=data.device)
        ai, ao, npts = c_size_t(0), c_size_t(0), c_size_t(0)
        r = self._lib.libdeflate_amd_decompress_large_index(
            self._h, FORMATS[fmt], data.data_ptr() if n else None, n,
            out.data_ptr() if avail else None, avail, ctypes.byref(ai),
            ctypes.byref(ao) if want_actual_out else None, int(spacing),
            idx.ctypes.data_as(c_void_p), idx.size, ctypes.byref(npts),
            win.data_ptr() if max_points > 0 else None, win.numel(), _stream_ptr(stream))
        if r != 0:
            return r, ai.value, ao.value, None, None
        rows = idx[:binding.SEEK_WORDS * (npts.value + 2)].reshape(-1, binding.SEEK_WORDS).copy()
        return r, ai.value, ao.value, rows, win[:npts.value * binding.SEEK_WINDOW]

    def seek_read_batch(self, data, index, windows, ranges, out, results, stream=None,
                        in_nbytes=None, out_avail=None):
        """libdeflate_amd_seek_read_batch: `ranges` (host, rows of (offset,
        nbytes) of the uncompressed data) of the stream in the CUDA tensor
        `data`, through the index and windows of decompress_large_index,
        back to back into `out`; results: int32 CUDA tensor, one per range (0
        or BAD_DATA).  Only enqueues on `stream`."""
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
        rng = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        check(self._lib.libdeflate_amd_seek_read_batch(
            self._h, data.data_ptr(), n, idx.ctypes.data_as(c_void_p), idx.size,
            windows.data_ptr(), len(rng), rng.ctypes.data_as(c_void_p),
            out.data_ptr() if out.numel() else None, avail,
            results.data_ptr() if len(rng) else None, _stream_ptr(stream)), "seek_read_batch")

    def decompress_batch(self, fmt, data, in_offsets, in_nbytes, out,
                         out_offsets, out_avail, results, actual_in=None,
                         actual_out=None, stream=None):
        check(self._lib.libdeflate_amd_decompress_batch(
            self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
            in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr(), out_avail.data_ptr(), results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            actual_out.data_ptr() if actual_out is not None else None,
            _stream_ptr(stream)), "decompress_batch")

    def _chunk_decode(self, call, words, rows, data, out, results, stream, in_nbytes, out_avail,
                      fmt=None, more=()):
        """The body of the chunk codecs' decompress / decode wrappers:
        libdeflate_amd_<call>(handle, [format,] rows, data, out, [more,]
        results, stream).  An empty `data` or `out` goes as NULL, and so does
        `results` of no rows."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, words)
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        avail = out.numel() if out_avail is None else int(out_avail)
        assert results.numel() >= len(r)
        check(getattr(self._lib, "libdeflate_amd_" + call)(
            self._h, *(() if fmt is None else (fmt,)), len(r), r.ctypes.data_as(c_void_p),
            data.data_ptr() if n else None, n, out.data_ptr() if avail else None, avail, *more,
            results.data_ptr() if len(r) else None, _stream_ptr(stream)), call)
        return r

    def decompress_shuffle_batch(self, fmt, rows, data, out, results, stream=None,
                                 in_nbytes=None, out_avail=None):
        """libdeflate_amd_shuffle_decompress_batch: byte-shuffled deflate chunks
        (HDF5, NetCDF-4, Zarr) of `data` decoded and unshuffled into their rooms
        of `out`.  rows: host rows of SHUF_WORDS u64 (shuffle_rows(), or the
        index compress_shuffle_batch wrote); data, out: uint8 CUDA tensors;
        results: int32 CUDA tensor, one enum libdeflate_result per chunk.
        Returns the rows as passed (numpy uint64).  Only enqueues."""
        return self._chunk_decode("shuffle_decompress_batch", binding.SHUF_WORDS, rows, data, out,
                                  results, stream, in_nbytes, out_avail, fmt=FORMATS[fmt])

    def decode_tiff_batch(self, rows, data, out, results, stream=None, in_nbytes=None,
                          out_avail=None):
        """libdeflate_amd_tiff_decode_batch: the deflate strips or tiles of a
        TIFF in `data` decoded, their predictor undone and their kept
        rectangles written into `out` at the rows' offsets and pitch.  rows:
        host rows of TIFF_WORDS u64 (tiff_rows(), libdeflate_amd.tiff.parse(),
        or the index encode_tiff_batch wrote); data, out: uint8 CUDA tensors;
        results: int32 CUDA tensor, one enum libdeflate_result per segment.
        Returns the rows as passed (numpy uint64).  Only enqueues."""
        return self._chunk_decode("tiff_decode_batch", binding.TIFF_WORDS, rows, data, out, results,
                                  stream, in_nbytes, out_avail)

    def decode_exr_batch(self, rows, data, out, results, stream=None, in_nbytes=None,
                         out_avail=None):
        """libdeflate_amd_exr_decode_batch: the ZIP / ZIPS chunks of an OpenEXR
        file in `data` - zlib streams or raw, by their dataSize - decoded,
        their coding undone and their lines written into `out` at the rows'
        offsets and pitch, as the file's planes (LINES) or as interleaved
        pixels (PIXELS).  rows: host rows of EXR_WORDS u64 (exr_rows(),
        libdeflate_amd.exr.parse(), or the index encode_exr_batch wrote);
        data, out: uint8 CUDA tensors; results: int32 CUDA tensor, one enum
        libdeflate_result per chunk.  Returns the rows as passed (numpy
        uint64).  Only enqueues."""
        return self._chunk_decode("exr_decode_batch", binding.EXR_WORDS, rows, data, out, results,
                                  stream, in_nbytes, out_avail)

    def parquet_decode_batch(self, fmt, rows, data, out, valid, results, stream=None,
                             in_nbytes=None, out_avail=None, valid_avail=None):
        """libdeflate_amd_parquet_decode_batch: the pages of flat Parquet column
        chunks in `data` - gzip members (fmt "gzip"; "zlib" and "deflate" are
        taken too) or uncompressed - decoded, their definition levels and
        dictionary indices expanded and every slot written into `out` at the
        rows' offsets, a null as zeros, with one validity byte per slot of a
        nullable column in `valid`.  rows: host rows of PARQUET_WORDS u64
        (parquet_rows(), or libdeflate_amd.parquet.pages()); data, out: uint8
        CUDA tensors; valid: uint8 or bool CUDA tensor, or None while no row
        has max_def 1; results: int32 CUDA tensor, one enum libdeflate_result
        per page.  Returns the rows as passed (numpy uint64).  Only
        enqueues."""
        v_avail = (0 if valid is None else valid.numel()) if valid_avail is None \
            else int(valid_avail)
        return self._chunk_decode("parquet_decode_batch", binding.PARQUET_WORDS, rows, data, out,
                                  results, stream, in_nbytes, out_avail, fmt=FORMATS[fmt],
                                  more=(valid.data_ptr() if valid is not None else None, v_avail))

    def parquet_decode_batch_ex(self, fmt, rows, data, out, valid, strings, total, results,
                                stream=None, in_nbytes=None, out_avail=None, valid_avail=None,
                                bytes_avail=None, flags=0):
        """libdeflate_amd_parquet_decode_batch_ex: parquet_decode_batch with
        BYTE_ARRAY rows (parquet_rows(byte_array=1),
        libdeflate_amd.parquet.pages(strings=True)).  Such a data page writes
        count + 1 int64 offsets into `out` at its word 5 and its bytes into
        `strings`, where the bytes of all such pages of the call lie back to
        back; the offsets are positions in `strings`.  strings: uint8 CUDA
        tensor, or None for the sizing call; total: uint64 or int64 CUDA
        tensor of one element, which receives the room the strings need - a
        page that does not fit ends as INSUFFICIENT_SPACE -, or None while no
        row is BYTE_ARRAY.  The rest as parquet_decode_batch.  Only
        enqueues."""
        v_avail = (0 if valid is None else valid.numel()) if valid_avail is None \
            else int(valid_avail)
        b_avail = (0 if strings is None else strings.numel()) if bytes_avail is None \
            else int(bytes_avail)
        return self._chunk_decode(
            "parquet_decode_batch_ex", binding.PARQUET_WORDS, rows, data, out, results, stream,
            in_nbytes, out_avail, fmt=FORMATS[fmt],
            more=(valid.data_ptr() if valid is not None else None, v_avail,
                  strings.data_ptr() if strings is not None and strings.numel() else None, b_avail,
                  total.data_ptr() if total is not None else None, int(flags)))

    def decompress_batch_dict(self, fmt, dictionary, data, in_offsets, in_nbytes, out,
                              out_offsets, out_avail, results, actual_in=None,
                              actual_out=None, stream=None):
        """Device batch with one preset dictionary for every stream
        (libdeflate_amd_decompress_batch_dict); `dictionary` is a uint8
        torch CUDA tensor, the rest as in decompress_batch."""
        check(self._lib.libdeflate_amd_decompress_batch_dict(
            self._h, FORMATS[fmt], in_offsets.numel(),
            dictionary.data_ptr() if dictionary.numel() else None, dictionary.numel(),
            data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr(), out_avail.data_ptr(), results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            actual_out.data_ptr() if actual_out is not None else None,
            _stream_ptr(stream)), "decompress_batch_dict")

    def decompress_prefix_batch(self, fmt, data, in_offsets, in_nbytes, out, out_offsets,
                                limits, results, actual_out, actual_in=None, stream=None):
        """libdeflate_amd_decompress_prefix_batch: the first limits[i] bytes
        of every stream.  results[i] is SUCCESS (the stream ended within its
        limit and was checked in full), PREFIX (cut: exactly limits[i] bytes
        written, actual_out[i] = limits[i]) or the stream's failure.  Tensors
        as in decompress_batch; limits and actual_out int64.  Only enqueues."""
        check(self._lib.libdeflate_amd_decompress_prefix_batch(
            self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
            in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr(), limits.data_ptr(), results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            actual_out.data_ptr(), _stream_ptr(stream)), "decompress_prefix_batch")

    def decompress_prefix_batch_dict(self, fmt, dictionary, data, in_offsets, in_nbytes, out,
                                     out_offsets, limits, results, actual_out, actual_in=None,
                                     stream=None):
        """libdeflate_amd_decompress_prefix_batch_dict: the same with the
        preset dictionary (a uint8 torch CUDA tensor) of decompress_batch_dict."""
        check(self._lib.libdeflate_amd_decompress_prefix_batch_dict(
            self._h, FORMATS[fmt], in_offsets.numel(),
            dictionary.data_ptr() if dictionary.numel() else None, dictionary.numel(),
            data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out_offsets.data_ptr(), limits.data_ptr(), results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            actual_out.data_ptr(), _stream_ptr(stream)), "decompress_prefix_batch_dict")

    def decompress_prefix(self, fmt, data, limit):
        """libdeflate_amd_decompress_prefix: host bytes -> (result,
        actual_out, bytes); result is SUCCESS, PREFIX (bytes are the first
        `limit` of the stream) or the stream's failure (no bytes)."""
        p, n = _buf(data)
        out = np.zeros(max(limit, 1), dtype=np.uint8)
        ao = c_size_t(0)
        r = self._lib.libdeflate_amd_decompress_prefix(
            self._h, FORMATS[fmt], p, n, out.ctypes.data_as(c_void_p), limit, ctypes.byref(ao))
        return r, ao.value, out[:ao.value].tobytes()

    def peek_gzip_members_batch(self, data, result, index, max_members, head_nbytes, heads,
                                head_sizes, results, stream=None, in_nbytes=None):
        """libdeflate_amd_gzip_members_peek_batch: the first head_nbytes bytes
        of every member of the file in `data`, from `result` and `index` as
        index_gzip_members_batch wrote them (CUDA tensors, nothing crosses to
        the host).  heads: uint8 CUDA tensor of max_members * head_nbytes;
        head_sizes: int64, results: int32, max_members each.  Only enqueues."""
        n = data.numel() if in_nbytes is None else int(in_nbytes)
        check(self._lib.libdeflate_amd_gzip_members_peek_batch(
            self._h, data.data_ptr() if n else None, n, result.data_ptr(), index.data_ptr(),
            int(max_members), int(head_nbytes),
            heads.data_ptr() if heads is not None and heads.numel() else None,
            head_sizes.data_ptr(), results.data_ptr(), _stream_ptr(stream)),
            "gzip_members_peek_batch")

    def decompress_sizes_batch(self, fmt, data, in_offsets, in_nbytes, results, out_nbytes,
                               limits=None, actual_in=None, stream=None):
        """libdeflate_amd_decompress_sizes_batch: the uncompressed size of
        every stream, nothing decoded.  results: int32 CUDA tensor, out_nbytes
        (and limits, actual_in when given): int64.  Only enqueues."""
        check(self._lib.libdeflate_amd_decompress_sizes_batch(
            self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
            in_offsets.data_ptr(), in_nbytes.data_ptr(),
            limits.data_ptr() if limits is not None else None, results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            out_nbytes.data_ptr(), _stream_ptr(stream)), "decompress_sizes_batch")

    def decompress_sizes_batch_dict(self, fmt, dictionary, data, in_offsets, in_nbytes,
                                    results, out_nbytes, limits=None, actual_in=None,
                                    stream=None):
        """libdeflate_amd_decompress_sizes_batch_dict: the same with the
        preset dictionary (a uint8 torch CUDA tensor) of decompress_batch_dict."""
        check(self._lib.libdeflate_amd_decompress_sizes_batch_dict(
            self._h, FORMATS[fmt], in_offsets.numel(),
            dictionary.data_ptr() if dictionary.numel() else None, dictionary.numel(),
            data.data_ptr(), in_offsets.data_ptr(), in_nbytes.data_ptr(),
            limits.data_ptr() if limits is not None else None, results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            out_nbytes.data_ptr(), _stream_ptr(stream)), "decompress_sizes_batch_dict")

    def decompress_sizes_batch_host(self, fmt, chunks, limits=None):
        """libdeflate_amd_decompress_sizes_batch_host: list of bytes -> list
        of (result, actual_in, size)."""
        n = len(chunks)
        arrs = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
        inp = (c_void_p * n)(*[a.ctypes.data for a in arrs])
        inn = (c_size_t * n)(*[a.size for a in arrs])
        lim = (c_size_t * n)(*limits) if limits is not None else None
        res = (ctypes.c_int32 * n)()
        ain = (c_size_t * n)()
        size = (c_size_t * n)()
        check(self._lib.libdeflate_amd_decompress_sizes_batch_host(
            self._h, FORMATS[fmt], n, inp, inn, lim, res, ain, size),
            "decompress_sizes_batch_host")
        return [(res[i], ain[i], size[i]) for i in range(n)]

    def decompress_batch_packed(self, fmt, data, in_offsets, in_nbytes, out, out_offsets,
                                results, actual_out, actual_in=None, out_align=16,
                                out_capacity=None, stream=None):
        """libdeflate_amd_decompress_batch_packed: streams of unknown size
        into `out` back to back (slots aligned to out_align).  out_offsets:
        int64 CUDA tensor of n + 1 entries, written; the last one is the total
        the batch needs.  Only enqueues."""
        check(self._lib.libdeflate_amd_decompress_batch_packed(
            self._h, FORMATS[fmt], in_offsets.numel(), data.data_ptr(),
            in_offsets.data_ptr(), in_nbytes.data_ptr(), out.data_ptr(),
            out.numel() if out_capacity is None else int(out_capacity), int(out_align),
            out_offsets.data_ptr(), results.data_ptr(),
            actual_in.data_ptr() if actual_in is not None else None,
            actual_out.data_ptr(), _stream_ptr(stream)), "decompress_batch_packed")

    def decompress_batch_host(self, fmt, chunks, out_avail,
                              want_actual_out=True):
        """-> list of (result, actual_in, actual_out, bytes)."""
        n = len(chunks)
        arrs = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
        outs = [np.zeros(max(a, 1), dtype=np.uint8) for a in out_avail]
        inp = (c_void_p * n)(*[a.ctypes.data for a in arrs])
        inn = (c_size_t * n)(*[a.size for a in arrs])
        outp = (c_void_p * n)(*[o.ctypes.data for o in outs])
        outa = (c_size_t * n)(*out_avail)
        res = (ctypes.c_int32 * n)()
        ain = (c_size_t * n)()
        aout = (c_size_t * n)()
        check(self._lib.libdeflate_amd_decompress_batch_host(
            self._h, FORMATS[fmt], n, inp, inn, outp, outa, res, ain,
            aout if want_actual_out else None), "decompress_batch_host")
        r = []
        for i in range(n):
            nout = aout[i] if want_actual_out else out_avail[i]
            r.append((res[i], ain[i], aout[i],
                      outs[i][:nout].tobytes() if res[i] == 0 else b""))
        return r


def bgzf_gzi(index):
    """The index of a BGZF file (rows of compressed / uncompressed offsets of
    every member start, as compress_bgzf(index=True) returns them, the EOF row
    last) as the bytes of bgzip's .gzi: u64 LE count, then the pairs of the
    member starts after the first.  Follows htslib's description of the
    format; not compared with bgzip -i itself."""
    rows = np.asarray(index, dtype=np.uint64).reshape(-1, 2)[1:-1]
    return (np.array([len(rows)], dtype="<u8").tobytes() +
            rows.astype("<u8").tobytes())


def bgzf_index_gzi(index, members=None):
    """.gzi bytes from what the BGZF reader returns: the index tensor or
    array of decompress_bgzf_batch / index_bgzf_batch (`members` = result[1])
    or the rows of decompress_bgzf.  bgzip's .gzi lists the starts of the
    data members; a trailing EOF member's row closes the list as
    bgzf_gzi() expects it."""
    if hasattr(index, "cpu"):
        index = index.cpu().numpy()
    rows = np.asarray(index).astype(np.uint64).reshape(-1, 2)
    if members is not None:
        rows = rows[:int(members) + 1]
    # an empty last member (the EOF member) stands where the closing row
    # would: drop the closing row and let its row close the list
    if len(rows) >= 2 and rows[-1][1] == rows[-2][1]:
        rows = rows[:-1]
    return bgzf_gzi(rows)


def bgzf_gzi_parse(blob):
    """bgzf_gzi()'s bytes back to rows (compressed, uncompressed) of the member
    starts after the first."""
    count = int(np.frombuffer(blob[:8], dtype="<u8")[0])
    assert len(blob) == 8 + 16 * count, "truncated .gzi"
    return np.frombuffer(blob[8:], dtype="<u8").reshape(count, 2)


def zip_entry_names(data, result, index):
    """The entries' names of the archive in the CUDA tensor `data`, from the
    result words and index rows of index_zip_batch / decompress_zip_batch
    (CUDA tensors or host arrays): the directory region is fetched once.
    Bytes that are no UTF-8 decode as CP437, as zipfile reads them."""
    words = [int(x) for x in (result.cpu().tolist() if hasattr(result, "cpu") else result)]
    rows = index.cpu().numpy() if hasattr(index, "cpu") else np.asarray(index)
    entries, cd_off = words[1], words[2]
    rows = rows.reshape(-1, binding.ZIP_WORDS)[:entries].astype(np.uint64)
    if not entries:
        return []
    cd_end = int((rows[:, 0] + np.uint64(46) + rows[:, 1]).max())
    cd = data[cd_off:cd_end].cpu().numpy().tobytes()
    names = []
    for rec, name_len, mf in zip(rows[:, 0].tolist(), rows[:, 1].tolist(), rows[:, 2].tolist()):
        raw = cd[rec + 46 - cd_off:rec + 46 - cd_off + name_len]
        names.append(raw.decode("utf-8" if (mf >> 16) & 0x800 else "cp437"))
    return names


def tar_entry_names(data, result, index):
    """The entries' names of the tar archive in the CUDA tensor `data`, from
    the result words and index rows of index_tar_batch / extract_tar_batch
    (CUDA tensors or host arrays): a ustar prefix, '/' and the name joined,
    the pax value or the L data as they stand.  The name bytes are gathered on
    the device and fetched once; they decode as UTF-8 with surrogateescape, as
    tarfile reads them."""
    import torch
    words = [int(x) for x in (result.cpu().tolist() if hasattr(result, "cpu") else result)]
    rows = index.cpu().numpy() if hasattr(index, "cpu") else np.asarray(index)
    rows = rows.reshape(-1, binding.TAR_WORDS)[:words[1]].astype(np.int64)
    if not len(rows):
        return []
    name_len, prefix_len = rows[:, 2] & 0xFFFFFFFF, rows[:, 2] >> 32
    starts = np.stack([rows[:, 0] + 345, rows[:, 1]], axis=1).reshape(-1)
    lens = np.stack([prefix_len, name_len], axis=1).reshape(-1)
    ends = np.cumsum(lens)
    where = np.repeat(starts - (ends - lens), lens) + np.arange(ends[-1])
    raw = data[torch.from_numpy(where).to(data.device)].cpu().numpy().tobytes() if ends[-1] else b""
    names = []
    for k in range(len(rows)):
        p0 = int(ends[2 * k] - lens[2 * k])
        prefix, name = raw[p0:int(ends[2 * k])], raw[int(ends[2 * k]):int(ends[2 * k + 1])]
        names.append(((prefix + b"/" if prefix else b"") + name).decode("utf-8", "surrogateescape"))
    return names


def tar_ranges(index, sel):
    """libdeflate_amd_tar_ranges: (data_off, usize) of the entries `sel` of
    the host index rows `index` -> (numpy uint64 rows of 2, total bytes): what
    seek_read_batch takes as `ranges` for the .gz the archive came out of.  No
    device is touched."""
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.TAR_WORDS)
    s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
    rng = np.zeros((len(s), 2), dtype=np.uint64)
    total = ctypes.c_uint64(0)
    check(binding.load().libdeflate_amd_tar_ranges(
        idx.ctypes.data_as(c_void_p), len(idx), len(s), s.ctypes.data_as(c_void_p),
        rng.ctypes.data_as(c_void_p), ctypes.byref(total)), "tar_ranges")
    return rng, total.value


def png_out_sizes(index, sel, out_align=1):
    """libdeflate_amd_png_out_sizes: where decode_png_batch puts the images
    `sel` of the host index rows `index` -> (numpy uint64 offsets, len(sel) + 1,
    total bytes).  An image takes height * rowbytes bytes rounded up to
    out_align, a zero row (a refused file) none.  No device is touched."""
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
    s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
    offs = np.zeros(len(s) + 1, dtype=np.uint64)
    total = ctypes.c_uint64(0)
    check(binding.load().libdeflate_amd_png_out_sizes(
        idx.ctypes.data_as(c_void_p), len(idx), len(s), s.ctypes.data_as(c_void_p),
        int(out_align), offs.ctypes.data_as(c_void_p), ctypes.byref(total)), "png_out_sizes")
    return offs, total.value


def png_out_sizes_ex(index, sel, fmt=0, out_align=1, flags=0):
    """libdeflate_amd_png_out_sizes_ex: where decode_png_batch_ex puts the
    images `sel` of the host index rows `index` -> (numpy uint64 offsets,
    len(sel) + 1, total bytes): png_out_sizes for fmt 0, png_pixels_out_sizes
    for any other.  An interlaced row is taken only with binding.PNG_ADAM7 in
    flags, and takes the room of its non-interlaced twin.  No device is
    touched."""
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
    s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
    offs = np.zeros(len(s) + 1, dtype=np.uint64)
    total = ctypes.c_uint64(0)
    check(binding.load().libdeflate_amd_png_out_sizes_ex(
        idx.ctypes.data_as(c_void_p), len(idx), len(s), s.ctypes.data_as(c_void_p), int(fmt),
        int(out_align), int(flags), offs.ctypes.data_as(c_void_p), ctypes.byref(total)),
        "png_out_sizes_ex")
    return offs, total.value


def png_shapes(index):
    """(height, width, channels, bit_depth, colour_type) of every host index
    row of index_png_batch, all zero for a refused file: an 8-bit image's bytes
    view as a uint8 tensor of height x width x channels, a 16-bit image's
    (decoded with PNG_LE16) as uint16 of the same shape; below 8 bits a row is
    ceil(width * bit_depth / 8) packed bytes."""
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
    return [(int(r[2] >> 32), int(r[2] & 0xFFFFFFFF), int(r[3] >> 32), int(r[3] & 0xFF),
             int(r[3] >> 8 & 0xFF)) for r in idx.tolist()]


def png_pixels_out_sizes(index, sel, fmt, out_align=1):
    """libdeflate_amd_png_pixels_out_sizes: where decode_png_pixels_batch puts
    the images `sel` of the host index rows `index` in the format fmt ->
    (numpy uint64 offsets, len(sel) + 1, total bytes).  An image takes height *
    width * channels * (1 or 2) bytes rounded up to out_align, a zero row none.
    No device is touched."""
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
    s = np.ascontiguousarray(sel, dtype=np.uint64).reshape(-1)
    offs = np.zeros(len(s) + 1, dtype=np.uint64)
    total = ctypes.c_uint64(0)
    check(binding.load().libdeflate_amd_png_pixels_out_sizes(
        idx.ctypes.data_as(c_void_p), len(idx), len(s), s.ctypes.data_as(c_void_p), int(fmt),
        int(out_align), offs.ctypes.data_as(c_void_p), ctypes.byref(total)),
        "png_pixels_out_sizes")
    return offs, total.value


def png_pixels_shapes(index, fmt):
    """([(height, width, channels) per host index row, zeros for a refused
    file], the numpy dtype) of what decode_png_pixels_batch writes in the
    format fmt (uint16 wants PNG_LE16 in the call's flags)."""
    ch = int(fmt) & 0xF
    if not 1 <= ch <= 4 or int(fmt) & ~(0xF | binding.PNG_OUT16):
        raise ValueError("png_pixels_shapes: format 0x%x" % int(fmt))
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1, binding.PNG_WORDS)
    shapes = [(int(r[2] >> 32), int(r[2] & 0xFFFFFFFF), ch) if any(r[2:]) else (0, 0, 0)
              for r in idx.tolist()]
    return shapes, np.dtype(np.uint16 if int(fmt) & binding.PNG_OUT16 else np.uint8)


_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_PNG_COLOUR_OF = {1: 0, 2: 4, 3: 2, 4: 6}


def png_image_rows(shapes, offsets, depth=8, colour=None, plte=None, trns=None):
    """The host rows encode_png_batch takes.  shapes: (H, W) or (H, W, C) per
    image; offsets: where each image's pixels start in the data tensor, in
    bytes; depth and colour: one value or one per image - colour None takes the
    colour type from C (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA; (H, W) is grey);
    plte / trns: None, or per image None or (offset in the data tensor, entries
    / length).  -> numpy uint64 (images, PNG_WORDS)."""
    n = len(shapes)

    def per_image(v):
        return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
    depths, colours = per_image(depth), per_image(colour)
    pl, tr = per_image(plte) if plte is not None else [None] * n, \
        per_image(trns) if trns is not None else [None] * n
    assert len(offsets) == n and len(depths) == n and len(colours) == n
    rows = np.zeros((n, binding.PNG_WORDS), dtype=np.uint64)
    for k, shp in enumerate(shapes):
        h, w = int(shp[0]), int(shp[1])
        c = int(shp[2]) if len(shp) > 2 else 1
        col = _PNG_COLOUR_OF[c] if colours[k] is None else int(colours[k])
        if _PNG_CHANNELS.get(col) != c:
            raise ValueError(f"image {k}: colour type {col} has not {c} channels")
        rb = (w * c * int(depths[k]) + 7) // 8
        rows[k, 0], rows[k, 1] = int(offsets[k]), h * rb
        rows[k, 2] = w | h << 32
        rows[k, 3] = int(depths[k]) | col << 8
        if pl[k] is not None:
            rows[k, 6] = int(pl[k][0]) | int(pl[k][1]) << 48
        if tr[k] is not None:
            rows[k, 7] = int(tr[k][0]) | int(tr[k][1]) << 48
    return rows


def _per_row(v, n, pair=False):
    """One value for all n rows, or a sequence of one per row.  pair: a tuple
    is ONE value - a (width, rows) pair -, not a sequence of per-row values."""
    return list(v) if isinstance(v, (list, np.ndarray) if pair else (list, tuple, np.ndarray)) \
        else [v] * n


def shuffle_rows(raw_offsets, raw_sizes, itemsize, stored_offsets=None, stored_sizes=None,
                 mask=0):
    """The host rows of the shuffle calls.  raw_offsets / raw_sizes: where each
    chunk's raw bytes lie (the writer's input, the reader's rooms), in bytes;
    itemsize: the element size (numpy's dtype.itemsize), one value or one per
    chunk; stored_offsets / stored_sizes: the stored chunks in the compressed
    buffer (the reader; None: zeros, which the writer ignores); mask: 0 or
    SHUF_NO_DEFLATE | SHUF_NO_SHUFFLE, one value or one per chunk.
    -> numpy uint64 (chunks, SHUF_WORDS)."""
    n = len(raw_offsets)
    per = functools.partial(_per_row, n=n)
    rows = np.zeros((n, binding.SHUF_WORDS), dtype=np.uint64)
    cols = (per(0 if stored_offsets is None else stored_offsets),
            per(0 if stored_sizes is None else stored_sizes),
            raw_offsets, raw_sizes, per(itemsize), per(mask))
    for w, col in enumerate(cols):
        assert len(col) == n
        for k in range(n):
            rows[k, w] = int(col[k])
    return rows


def tiff_rows(raw_offsets, pitches, coded, kept, spp, bps, predictor, stored_offsets=None,
              stored_sizes=None):
    """The host rows of the TIFF calls, one per segment (strip or tile).
    raw_offsets: where each segment's kept pixel (0, 0) lies in the raw
    buffer; pitches: bytes between kept rows there; coded / kept: (width,
    rows) of the coded segment and of the rectangle that is kept, one pair or
    one per segment (kept None: the coded size); spp, bps, predictor: samples
    per pixel, bytes per sample, 1 / 2 / 3, one value or one per segment;
    stored_offsets / stored_sizes: the zlib streams in the compressed buffer
    (the reader; None: zeros, which the writer ignores).
    -> numpy uint64 (segments, TIFF_WORDS)."""
    n = len(raw_offsets)
    per = functools.partial(_per_row, n=n, pair=True)
    so, sn = per(0 if stored_offsets is None else stored_offsets), \
        per(0 if stored_sizes is None else stored_sizes)
    pi, cd, sp, bp, pr = per(pitches), per(coded), per(spp), per(bps), per(predictor)
    kp = cd if kept is None else per(kept)
    rows = np.zeros((n, binding.TIFF_WORDS), dtype=np.uint64)
    for k in range(n):
        rows[k, 0], rows[k, 1], rows[k, 2], rows[k, 3] = int(so[k]), int(sn[k]), \
            int(raw_offsets[k]), int(pi[k])
        rows[k, 4] = int(cd[k][0]) | int(cd[k][1]) << 32
        rows[k, 5] = int(kp[k][0]) | int(kp[k][1]) << 32
        rows[k, 6] = int(sp[k]) | int(bp[k]) << 8 | int(pr[k]) << 16
    return rows


def exr_rows(pix_offsets, pitches, sizes, wide, layout=0, slots=None, data_offsets=None,
             data_sizes=None, heads=None):
    """The host rows of the OpenEXR calls, one per chunk (scanline block or
    tile).  pix_offsets: where each chunk's line 0, pixel 0 lies in the pixel
    buffer; pitches: bytes between lines there; sizes: (width, lines), one
    pair or one per chunk; wide: per channel of the file, in its order, True
    for 4-byte samples (FLOAT, UINT) and False for HALF - one list for all
    chunks; layout: binding.EXR_LINES or EXR_PIXELS; slots: PIXELS only, the
    place of the file's channel k in the pixel (None: the file's order);
    data_offsets / data_sizes: the chunks' data in the compressed buffer (the
    reader; None: zeros, which the writer ignores); heads: None (no head) or
    per chunk a tuple of the int32 values in front of dataSize - (y,) or
    (tileX, tileY, levelX, levelY).
    -> numpy uint64 (chunks, EXR_WORDS)."""
    n = len(pix_offsets)
    per = functools.partial(_per_row, n=n, pair=True)
    do, dn = per(0 if data_offsets is None else data_offsets), \
        per(0 if data_sizes is None else data_sizes)
    pi = per(pitches)
    sz = [tuple(sizes)] * n if np.ndim(sizes) == 1 else [tuple(s) for s in sizes]
    wide = [bool(w) for w in wide]
    c = len(wide)
    fmt = c | sum(1 << (8 + k) for k in range(c) if wide[k]) | int(layout) << 32
    slot_word = 0
    if int(layout) == binding.EXR_PIXELS:
        for k, s in enumerate(range(c) if slots is None else slots):
            slot_word |= int(s) << (4 * k)
    rows = np.zeros((n, binding.EXR_WORDS), dtype=np.uint64)
    for k in range(n):
        rows[k, 0], rows[k, 1], rows[k, 2], rows[k, 3] = int(do[k]), int(dn[k]), \
            int(pix_offsets[k]), int(pi[k])
        rows[k, 4] = int(sz[k][0]) | int(sz[k][1]) << 32
        rows[k, 5], rows[k, 6] = fmt, slot_word
        head = () if heads is None else tuple(heads[k])
        assert len(head) in (0, 1, 4), "a head of one or four ints, or none"
        rows[k, 7] = 4 * len(head) + 4 if head else 0
        v = [int(x) & 0xFFFFFFFF for x in head] + [0, 0, 0, 0]
        rows[k, 8], rows[k, 9] = v[0] | v[1] << 32, v[2] | v[3] << 32
    return rows


def parquet_rows(offsets, csizes, usizes, kinds, counts, widths, encodings=0, compressed=True,
                 max_def=0, def_lens=0, out_offsets=0, valid_offsets=0, dict_rows=0, byte_array=0):
    """The host rows of the Parquet call, one per page, in the call's order.
    offsets, csizes, usizes: the page bodies in the compressed buffer and
    their two sizes; kinds: binding.PARQUET_DATA_V1, _DICT or _DATA_V2;
    counts: num_values (a dictionary page: its entries); widths: bytes of a
    value; encodings: 0, 2 or 8; compressed: is the body (V2: the values
    section) a stream; max_def: 0 or 1; def_lens: V2's
    definition_levels_byte_length; out_offsets / valid_offsets: slot 0 in the
    output and in the validity bytes; dict_rows: the row of a dictionary-coded
    page's dictionary; byte_array: 1 for a BYTE_ARRAY page of
    parquet_decode_batch_ex, whose width is 1 (the field 0) and whose
    out_offset is that of its int64 offsets.  All but offsets: one value or
    one per page.  -> numpy uint64 (pages, PARQUET_WORDS)."""
    n = len(offsets)
    per = functools.partial(_per_row, n=n)
    cs, us, kd, ct, wd, en, cp, md, dl, oo, vo, dr, ba = (per(v) for v in (
        csizes, usizes, kinds, counts, widths, encodings, compressed, max_def, def_lens,
        out_offsets, valid_offsets, dict_rows, byte_array))
    rows = np.zeros((n, binding.PARQUET_WORDS), dtype=np.uint64)
    for k in range(n):
        rows[k, 0], rows[k, 1], rows[k, 2] = int(offsets[k]), int(cs[k]), int(us[k])
        rows[k, 3] = int(kd[k]) | int(en[k]) << 4 | int(bool(cp[k])) << 12 | int(md[k]) << 13 | \
            (int(wd[k]) - 1) << 16 | (binding.PARQUET_BYTE_ARRAY if ba[k] else 0)
        rows[k, 4] = int(ct[k]) | int(dl[k]) << 32
        rows[k, 5], rows[k, 6], rows[k, 7] = int(oo[k]), int(vo[k]), int(dr[k])
    return rows


def _stream_ptr(stream):
    if stream is None:
        return None
    return c_void_p(getattr(stream, "cuda_stream", stream))


def crc32(data, init=0):
    """libdeflate_crc32 (libdeflate.h:345-346) on a host buffer."""
    p, n = _buf(data)
    return binding.load().libdeflate_crc32(init, p, n)


def adler32(data, init=1):
    """libdeflate_adler32 (libdeflate.h:335-336) on a host buffer."""
    p, n = _buf(data)
    return binding.load().libdeflate_adler32(init, p, n)


def checksum_batch(kind, data, offsets, nbytes, out, init=None, stream=None):
    """Device batch CRC-32 / Adler-32; torch CUDA tensors (uint8 data, int64
    offsets/nbytes, int32 out/init holding the u32 bit patterns)."""
    lib = binding.load()
    fn = (lib.libdeflate_amd_crc32_batch if kind == "crc32"
          else lib.libdeflate_amd_adler32_batch)
    check(fn(offsets.numel(), data.data_ptr(), offsets.data_ptr(),
             nbytes.data_ptr(), init.data_ptr() if init is not None else None,
             out.data_ptr(), _stream_ptr(stream)), kind + "_batch")


def compact_batch(data, offsets, nbytes, stream=None):
    """Device-side compaction (libdeflate_amd_compact_batch): the used part of
    every slot back to back.  torch CUDA tensors in; returns (packed uint8
    tensor sized for the worst case, int64 offsets[n + 1] - exclusive prefix
    sums of nbytes, offsets[n] = total).  Only enqueues; slice `packed` with
    int(offsets[n]) after synchronising."""
    import torch
    lib = binding.load()
    n = offsets.numel()
    cap = int(lib.libdeflate_amd_compact_offsets_len(n))
    out_off = torch.zeros(cap, dtype=torch.int64, device=data.device)
    packed = torch.empty(data.numel(), dtype=torch.uint8, device=data.device)
    check(lib.libdeflate_amd_compact_batch(
        n, data.data_ptr(), offsets.data_ptr(), nbytes.data_ptr(),
        packed.data_ptr(), out_off.data_ptr(), _stream_ptr(stream)),
        "compact_batch")
    return packed, out_off[:n + 1]
