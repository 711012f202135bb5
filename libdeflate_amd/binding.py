"""ctypes binding of libdeflate_amd.so (the C-ABI in include/libdeflate_amd.h).

This is the stub a Python caller of the reference would add (the reference's
own bindings list, README.md:146-157, are all thin FFI layers over
libdeflate.h).  It only declares signatures; all work happens in the HIP
library.  There is no fallback: if the shared object is missing the import
fails with instructions to build it.
"""
import ctypes
import os
from ctypes import (POINTER, c_char_p, c_int, c_int32, c_size_t, c_uint32,
                    c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
# LIBDEFLATE_AMD_LIB selects another build of the same library (e.g. the
# phase-profiling build libdeflate_amd_prof.so); never a different backend.
LIB_PATH = os.environ.get("LIBDEFLATE_AMD_LIB",
                          os.path.join(_HERE, "libdeflate_amd.so"))

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
FMT_DEFLATE, FMT_ZLIB, FMT_GZIP, FMT_BGZF = 0, 1, 2, 3
FORMATS = {"deflate": FMT_DEFLATE, "zlib": FMT_ZLIB, "gzip": FMT_GZIP, "bgzf": FMT_BGZF}
# BGZF (include/libdeflate_amd.h): input bytes per member, largest member, the
# EOF member's size, the flag that leaves it out
BGZF_BLOCK, BGZF_MEMBER_MAX, BGZF_EOF_BYTES, BGZF_NO_EOF = 65280, 65536, 28, 1
# the BGZF reader: result[0] beyond enum libdeflate_result, the flag bit of
# result[4], the words of a result, the read flag for virtual offsets
BGZF_MORE_MEMBERS, BGZF_HAS_EOF, BGZF_RESULT_WORDS, BGZF_VOFFSETS = 16, 1, 5, 2
# the reader of concatenated gzip members: result[0] beyond enum
# libdeflate_result, the words of a result, candidate room beyond max_members
GZM_MORE_MEMBERS, GZM_MORE_CANDIDATES, GZM_RESULT_WORDS, GZM_SLACK = 16, 17, 5, 1024
GZM_NAME_MAX = 65536    # bytes of FNAME + FCOMMENT the member reader accepts
# the ZIP reader: result[0] beyond enum libdeflate_result, a per-entry result,
# the words of a result, u64 per index row, candidate room beyond max_entries,
# the flag bit of result[4]
ZIP_MORE_ENTRIES, ZIP_MORE_CANDIDATES, ZIP_UNSUPPORTED = 16, 17, 18
ZIP_RESULT_WORDS, ZIP_WORDS, ZIP_SLACK, ZIP_ZIP64 = 5, 8, 1024, 1
# ... and bytes per copy / CRC piece of libdeflate_amd_zip_read_large
ZIP_PIECE = 1 << 20
# the tar reader: result[0] beyond enum libdeflate_result, a per-entry result,
# the words of a result, u64 per index row, candidate room beyond max_records,
# the flag bits of result[4]
TAR_MORE_RECORDS, TAR_MORE_CANDIDATES, TAR_UNSUPPORTED = 16, 17, 18
TAR_RESULT_WORDS, TAR_WORDS, TAR_SLACK = 5, 8, 1024
TAR_EOF, TAR_HAS_L, TAR_HAS_PAX = 1, 2, 4
# the PNG reader: a per-file result (the ZIP and tar readers' value), u64 per
# index row, the one flag of a decode
PNG_UNSUPPORTED, PNG_WORDS, PNG_LE16 = 18, 8, 1
# the flag of the _ex calls that lets Adam7-interlaced files through
PNG_ADAM7 = 2
# the pixel format of decode_png_pixels_batch: the channels, alone (8-bit
# samples) or with PNG_OUT16
PNG_GRAY, PNG_GRAY_ALPHA, PNG_RGB, PNG_RGBA, PNG_OUT16 = 1, 2, 3, 4, 0x10
# the PNG writer: the filter mode beyond the five types, the words of its result
PNG_FILTER_ADAPTIVE, PNGW_RESULT_WORDS = 5, 4
# the ZIP writer: the two flags, the words of its result
ZIP_STORE, ZIP_FORCE_ZIP64, ZIPW_RESULT_WORDS = 1, 2, 4
# the writer of concatenated gzip members: the words of its result, the longest
# name (GZM_NAME_MAX with its terminator and one byte to spare)
GZMW_RESULT_WORDS, GZMW_NAME_MAX = 4, 65534
# the seek index: bytes of window per point, u64 per row
SEEK_WINDOW, SEEK_WORDS = 32768, 4
# the size query: the limit a NULL d_out_limit stands for
SIZE_LIMIT_MAX = 0xFFFFFFFF
# the prefix decompress: the per-stream result of a stream cut at its limit
PREFIX = 19
# byte-shuffled deflate chunks: u64 per row, the largest element size, the two
# mask bits, the words of the writer's result
SHUF_WORDS, SHUF_ELEM_MAX, SHUF_NO_DEFLATE, SHUF_NO_SHUFFLE = 6, 256, 1, 2
SHUFW_RESULT_WORDS = 4
# predictor-coded deflate strips and tiles (TIFF): u64 per row, the most
# samples per pixel, the words of the writer's result
TIFF_WORDS, TIFF_SPP_MAX, TIFFW_RESULT_WORDS = 8, 16, 4
# OpenEXR ZIP / ZIPS chunks: u64 per row, the most channels, the words of the
# writer's result, the two layouts
EXR_WORDS, EXR_CHANNELS_MAX, EXRW_RESULT_WORDS = 10, 16, 4
EXR_LINES, EXR_PIXELS = 0, 1
# Parquet pages: u64 per row, the page kinds of a row's word 3
PARQUET_WORDS = 8
PARQUET_DATA_V1, PARQUET_DICT, PARQUET_DATA_V2 = 0, 2, 3
PARQUET_BYTE_ARRAY = 1 << 14      # word 3 of a row of the _ex call: a BYTE_ARRAY page

# every symbol include/libdeflate_amd.h declares
DROPIN_SYMBOLS = [
    "libdeflate_alloc_compressor", "libdeflate_alloc_compressor_ex",
    "libdeflate_deflate_compress", "libdeflate_deflate_compress_bound",
    "libdeflate_zlib_compress", "libdeflate_zlib_compress_bound",
    "libdeflate_gzip_compress", "libdeflate_gzip_compress_bound",
    "libdeflate_free_compressor",
    "libdeflate_alloc_decompressor", "libdeflate_alloc_decompressor_ex",
    "libdeflate_deflate_decompress", "libdeflate_deflate_decompress_ex",
    "libdeflate_zlib_decompress", "libdeflate_zlib_decompress_ex",
    "libdeflate_gzip_decompress", "libdeflate_gzip_decompress_ex",
    "libdeflate_free_decompressor",
    "libdeflate_adler32", "libdeflate_crc32",
    "libdeflate_set_memory_allocator",
]
BATCH_SYMBOLS = [
    "libdeflate_amd_device_ready", "libdeflate_amd_last_error",
    "libdeflate_amd_reload_env",
    "libdeflate_amd_compress_batch", "libdeflate_amd_decompress_batch",
    "libdeflate_amd_compress_batch_bounded", "libdeflate_amd_compress_last_schedule",
    "libdeflate_amd_compress_last_kernel",
    "libdeflate_amd_crc32_batch", "libdeflate_amd_adler32_batch",
    "libdeflate_amd_compress_batch_host",
    "libdeflate_amd_decompress_batch_host",
    "libdeflate_amd_compact_offsets_len", "libdeflate_amd_compact_batch",
    "libdeflate_amd_gzip_decompress_members",
    "libdeflate_amd_stream_stats", "libdeflate_amd_last_fanout",
    "libdeflate_amd_selfcheck",
    "libdeflate_amd_compress_batch_dict", "libdeflate_amd_decompress_batch_dict",
    "libdeflate_amd_compress_dict", "libdeflate_amd_decompress_dict_ex",
    "libdeflate_amd_bgzf_compress_bound", "libdeflate_amd_bgzf_compress_batch",
    "libdeflate_amd_bgzf_compress",
    "libdeflate_amd_bgzf_decompress_batch", "libdeflate_amd_bgzf_index_batch",
    "libdeflate_amd_bgzf_read_batch", "libdeflate_amd_bgzf_decompress",
    "libdeflate_amd_decompress_sizes_batch", "libdeflate_amd_decompress_sizes_batch_dict",
    "libdeflate_amd_decompress_sizes_batch_host", "libdeflate_amd_decompress_batch_packed",
    "libdeflate_amd_compress_large_batch", "libdeflate_amd_decompress_large",
    "libdeflate_amd_decompress_large_index", "libdeflate_amd_seek_read_batch",
    "libdeflate_amd_gzip_members_decompress_batch", "libdeflate_amd_gzip_members_index_batch",
    "libdeflate_amd_zip_index_batch", "libdeflate_amd_zip_decompress_batch",
    "libdeflate_amd_zip_read_batch", "libdeflate_amd_zip_read_large",
    "libdeflate_amd_zip_compress_bound", "libdeflate_amd_zip_compress_batch",
    "libdeflate_amd_gzip_members_compress_bound", "libdeflate_amd_gzip_members_compress_batch",
    "libdeflate_amd_decompress_prefix_batch", "libdeflate_amd_decompress_prefix_batch_dict",
    "libdeflate_amd_decompress_prefix", "libdeflate_amd_gzip_members_peek_batch",
    "libdeflate_amd_tar_index_batch", "libdeflate_amd_tar_extract_batch",
    "libdeflate_amd_tar_read_batch", "libdeflate_amd_tar_ranges",
    "libdeflate_amd_tar_write_size", "libdeflate_amd_tar_write_batch",
    "libdeflate_amd_targz_compress_batch",
    "libdeflate_amd_png_index_batch", "libdeflate_amd_png_out_sizes",
    "libdeflate_amd_png_decode_batch",
    "libdeflate_amd_png_pixels_out_sizes", "libdeflate_amd_png_decode_pixels_batch",
    "libdeflate_amd_png_encode_bound", "libdeflate_amd_png_encode_batch",
    "libdeflate_amd_png_index_batch_ex", "libdeflate_amd_png_out_sizes_ex",
    "libdeflate_amd_png_decode_batch_ex",
    "libdeflate_amd_shuffle_decompress_batch", "libdeflate_amd_shuffle_compress_bound",
    "libdeflate_amd_shuffle_compress_batch",
    "libdeflate_amd_tiff_decode_batch", "libdeflate_amd_tiff_encode_bound",
    "libdeflate_amd_tiff_encode_batch",
    "libdeflate_amd_exr_decode_batch", "libdeflate_amd_exr_encode_bound",
    "libdeflate_amd_exr_encode_batch",
    "libdeflate_amd_parquet_decode_batch", "libdeflate_amd_parquet_decode_batch_ex",
]

_lib = None
MISSING = []


def load():
    """dlopen the HIP library (RTLD_LOCAL) and declare the signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C libdeflate_amd/csrc -j` (hipcc, gfx950). "
            "libdeflate_amd has no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same
    # SONAME as /opt/rocm's).  Importing torch first makes the dynamic loader
    # bind our DT_NEEDED libamdhip64.so.7 to the copy torch already mapped;
    # the other order would map two runtimes and the second one sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    P, SZ = c_void_p, c_size_t
    psz = POINTER(c_size_t)

    def sig(name, restype, *argtypes):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            MISSING.append(name)    # tests/test_abi.py asserts this stays empty
            return
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("libdeflate_alloc_compressor", P, c_int)
    sig("libdeflate_alloc_compressor_ex", P, c_int, P)
    sig("libdeflate_free_compressor", None, P)
    sig("libdeflate_alloc_decompressor", P)
    sig("libdeflate_alloc_decompressor_ex", P, P)
    sig("libdeflate_free_decompressor", None, P)
    for f in ("deflate", "zlib", "gzip"):
        sig(f"libdeflate_{f}_compress", SZ, P, P, SZ, P, SZ)
        sig(f"libdeflate_{f}_compress_bound", SZ, P, SZ)
        sig(f"libdeflate_{f}_decompress", c_int, P, P, SZ, P, SZ, psz)
        sig(f"libdeflate_{f}_decompress_ex", c_int, P, P, SZ, P, SZ, psz, psz)
    sig("libdeflate_crc32", c_uint32, c_uint32, P, SZ)
    sig("libdeflate_adler32", c_uint32, c_uint32, P, SZ)
    sig("libdeflate_set_memory_allocator", None, P, P)
    sig("libdeflate_amd_device_ready", c_int)
    sig("libdeflate_amd_last_error", c_char_p)
    sig("libdeflate_amd_reload_env", None)
    sig("libdeflate_amd_crc32_batch", c_int, SZ, P, P, P, P, P, P)
    sig("libdeflate_amd_adler32_batch", c_int, SZ, P, P, P, P, P, P)
    sig("libdeflate_amd_compress_batch", c_int, P, c_int, SZ, P, P, P, P, P,
        P, P, P)
    sig("libdeflate_amd_compress_batch_bounded", c_int, P, c_int, SZ, P, P, P, P, P,
        P, P, SZ, P)
    sig("libdeflate_amd_compress_last_schedule", None, P, POINTER(c_uint32))
    sig("libdeflate_amd_compress_last_kernel", c_char_p, P)
    sig("libdeflate_amd_decompress_batch", c_int, P, c_int, SZ, P, P, P, P, P,
        P, P, P, P, P)
    sig("libdeflate_amd_compress_batch_host", c_int, P, c_int, SZ, P, P, P, P,
        P)
    sig("libdeflate_amd_decompress_batch_host", c_int, P, c_int, SZ, P, P, P,
        P, P, P, P)
    sig("libdeflate_amd_gzip_decompress_members", c_int, P, P, SZ, P, SZ, psz, psz, psz)
    sig("libdeflate_amd_stream_stats", None, POINTER(c_uint64))
    sig("libdeflate_amd_last_fanout", c_size_t)
    sig("libdeflate_amd_selfcheck", c_int, POINTER(c_uint64))
    sig("libdeflate_amd_compact_offsets_len", SZ, SZ)
    sig("libdeflate_amd_compact_batch", c_int, SZ, P, P, P, P, P, P)
    # preset dictionaries: the batch arguments with (dict, dict_nbytes) after
    # n_chunks, the single-buffer ones with them after the format
    sig("libdeflate_amd_compress_batch_dict", c_int, P, c_int, SZ, P, SZ, P, P, P, P,
        P, P, P, P)
    sig("libdeflate_amd_decompress_batch_dict", c_int, P, c_int, SZ, P, SZ, P, P, P, P,
        P, P, P, P, P, P)
    sig("libdeflate_amd_compress_dict", SZ, P, c_int, P, SZ, P, SZ, P, SZ)
    sig("libdeflate_amd_decompress_dict_ex", c_int, P, c_int, P, SZ, P, SZ, P, SZ,
        psz, psz)
    # BGZF files from one buffer: bound, device (enqueue only), host (blocking)
    sig("libdeflate_amd_bgzf_compress_bound", SZ, P, SZ)
    sig("libdeflate_amd_bgzf_compress_batch", c_int, P, P, SZ, P, SZ, P, P, c_uint32, P)
    sig("libdeflate_amd_bgzf_compress", SZ, P, P, SZ, P, SZ, P, SZ, c_uint32)
    # BGZF files read: device file -> device bytes, the index alone, ranged
    # reads (index and ranges on the host), host memory (blocking)
    sig("libdeflate_amd_bgzf_decompress_batch", c_int, P, P, SZ, SZ, P, SZ, P, P, P)
    sig("libdeflate_amd_bgzf_index_batch", c_int, P, P, SZ, SZ, P, P, P)
    sig("libdeflate_amd_bgzf_read_batch", c_int, P, P, SZ, P, SZ, SZ, P, c_uint32, P, SZ, P, P)
    sig("libdeflate_amd_bgzf_decompress", c_int, P, P, SZ, P, SZ, psz, psz, P, SZ,
        POINTER(c_uint32))
    # sizes without decoding (device, with a dictionary, host pointers), and
    # the packed decompress on top: sizes -> offsets -> decode, enqueue only
    sig("libdeflate_amd_decompress_sizes_batch", c_int, P, c_int, SZ, P, P, P, P, P, P, P, P)
    sig("libdeflate_amd_decompress_sizes_batch_dict", c_int, P, c_int, SZ, P, SZ, P, P, P, P,
        P, P, P, P)
    sig("libdeflate_amd_decompress_sizes_batch_host", c_int, P, c_int, SZ, P, P, P, P, P, P)
    sig("libdeflate_amd_decompress_batch_packed", c_int, P, c_int, SZ, P, P, P, P, SZ, SZ, P,
        P, P, P, P)
    # one raw DEFLATE / zlib / gzip stream from one device buffer, enqueue only
    sig("libdeflate_amd_compress_large_batch", c_int, P, c_int, P, SZ, P, SZ, P, P)
    # ... and one such stream from device memory to device memory (blocking)
    sig("libdeflate_amd_decompress_large", c_int, P, c_int, P, SZ, P, SZ, psz, psz, P)
    # ... the same with a seek index (host rows, device windows), and ranged
    # reads through such an index (index and ranges on the host, enqueue only)
    sig("libdeflate_amd_decompress_large_index", c_int, P, c_int, P, SZ, P, SZ, psz, psz,
        SZ, P, SZ, psz, P, SZ, P)
    sig("libdeflate_amd_seek_read_batch", c_int, P, P, SZ, P, SZ, P, SZ, P, P, SZ, P, P)
    # a file of concatenated gzip members: device file -> device bytes, the
    # index alone (enqueue only)
    sig("libdeflate_amd_gzip_members_decompress_batch", c_int, P, P, SZ, SZ, P, SZ, P, P, P)
    sig("libdeflate_amd_gzip_members_index_batch", c_int, P, P, SZ, SZ, P, P, P)
    # a ZIP archive: the index alone, device file -> every entry's bytes, a
    # selection of entries (index rows and entry numbers on the host)
    sig("libdeflate_amd_zip_index_batch", c_int, P, P, SZ, SZ, SZ, P, P, P, P)
    sig("libdeflate_amd_zip_decompress_batch", c_int, P, P, SZ, SZ, P, SZ, SZ, P, P, P, P)
    sig("libdeflate_amd_zip_read_batch", c_int, P, P, SZ, P, SZ, SZ, P, P, SZ, SZ, P, P, P)
    # ... the same selection with huge entries on many waves and in pieces
    # (blocking while those decode; large_min before out_offsets)
    sig("libdeflate_amd_zip_read_large", c_int, P, P, SZ, P, SZ, SZ, P, P, SZ, SZ, SZ, P, P, P)
    # a tar archive: the index alone, device file -> every entry's bytes, a
    # selection through host index rows, and the ranges of a selection (host)
    sig("libdeflate_amd_tar_index_batch", c_int, P, P, SZ, SZ, SZ, P, P, P, P)
    sig("libdeflate_amd_tar_extract_batch", c_int, P, P, SZ, SZ, P, SZ, SZ, P, P, P, P)
    sig("libdeflate_amd_tar_read_batch", c_int, P, P, SZ, P, SZ, SZ, P, P, SZ, SZ, P, P, P)
    sig("libdeflate_amd_tar_ranges", c_int, P, SZ, SZ, P, P, P)
    # PNG files: the index of a batch of files, the output offsets of a
    # selection (host arithmetic), and a selection through host index rows ->
    # pixels (flags before out_offsets)
    sig("libdeflate_amd_png_index_batch", c_int, P, SZ, P, P, P, P, P, P)
    sig("libdeflate_amd_png_out_sizes", c_int, P, SZ, SZ, P, SZ, P, P)
    sig("libdeflate_amd_png_decode_batch", c_int, P, P, SZ, P, SZ, SZ, P, P, SZ, SZ, c_uint32,
        P, P, P)
    # the same to one pixel format (format behind sel)
    sig("libdeflate_amd_png_pixels_out_sizes", c_int, P, SZ, SZ, P, c_uint32, SZ, P, P)
    sig("libdeflate_amd_png_decode_pixels_batch", c_int, P, P, SZ, P, SZ, SZ, P, c_uint32, P, SZ,
        SZ, c_uint32, P, P, P)
    # the same three with Adam7: flags behind the sizes of the index call,
    # format behind sel and flags behind out_align in the other two
    sig("libdeflate_amd_png_index_batch_ex", c_int, P, SZ, P, P, P, c_uint32, P, P, P)
    sig("libdeflate_amd_png_out_sizes_ex", c_int, P, SZ, SZ, P, c_uint32, SZ, c_uint32, P, P)
    sig("libdeflate_amd_png_decode_batch_ex", c_int, P, P, SZ, P, SZ, SZ, P, c_uint32, P, SZ,
        SZ, c_uint32, P, P, P)
    # byte-shuffled deflate chunks (HDF5, NetCDF-4, Zarr): host rows of
    # SHUF_WORDS u64, streams in a device buffer -> raw bytes and back
    sig("libdeflate_amd_shuffle_decompress_batch", c_int, P, c_int, SZ, P, P, SZ, P, SZ, P, P)
    sig("libdeflate_amd_shuffle_compress_bound", SZ, P, c_int, SZ, P)
    sig("libdeflate_amd_shuffle_compress_batch", c_int, P, c_int, SZ, P, P, SZ, P, SZ, P, P, P)
    # predictor-coded deflate strips and tiles (TIFF, GeoTIFF): host rows of
    # TIFF_WORDS u64, zlib streams in a device buffer -> pixels and back
    sig("libdeflate_amd_tiff_decode_batch", c_int, P, SZ, P, P, SZ, P, SZ, P, P)
    sig("libdeflate_amd_tiff_encode_bound", SZ, P, SZ, P)
    sig("libdeflate_amd_tiff_encode_batch", c_int, P, SZ, P, P, SZ, P, SZ, P, P, P)
    # OpenEXR ZIP / ZIPS chunks: host rows of EXR_WORDS u64, chunk data in a
    # device buffer -> lines or interleaved pixels and back
    sig("libdeflate_amd_exr_decode_batch", c_int, P, SZ, P, P, SZ, P, SZ, P, P)
    sig("libdeflate_amd_exr_encode_bound", SZ, P, SZ, P)
    sig("libdeflate_amd_exr_encode_batch", c_int, P, SZ, P, P, SZ, P, SZ, P, P, P)
    # Parquet pages: host rows of PARQUET_WORDS u64, the file in a device
    # buffer -> column slots and validity bytes
    sig("libdeflate_amd_parquet_decode_batch", c_int, P, c_int, SZ, P, P, SZ, P, SZ, P, SZ, P, P)
    # ... with BYTE_ARRAY rows: d_bytes, bytes_avail, d_bytes_total, flags
    sig("libdeflate_amd_parquet_decode_batch_ex", c_int, P, c_int, SZ, P, P, SZ, P, SZ, P, SZ,
        P, SZ, P, ctypes.c_uint64, P, P)
    # PNG files written: the bound (host arithmetic), and pixel arrays of a
    # device buffer -> files (the image rows on the host)
    sig("libdeflate_amd_png_encode_bound", SZ, P, SZ, P)
    sig("libdeflate_amd_png_encode_batch", c_int, P, SZ, P, P, SZ, P, SZ, P, P, c_uint32,
        c_uint32, P)
    # a ZIP archive written: the exact bound (host arithmetic), and named ranges
    # of a device buffer -> archive (names, offsets and sizes on the host)
    sig("libdeflate_amd_zip_compress_bound", SZ, SZ, P, P, c_uint32)
    sig("libdeflate_amd_zip_compress_batch", c_int, P, SZ, P, P, P, SZ, P, P, P, SZ, P, P,
        c_uint32, c_uint32, P)
    # a tar archive written: the exact size (host arithmetic), named ranges of a
    # device buffer -> archive, and -> one compressed stream of that archive
    # (names, offsets and sizes on the host; the index rows come back on the host)
    sig("libdeflate_amd_tar_write_size", SZ, SZ, P, P, P)
    sig("libdeflate_amd_tar_write_batch", c_int, P, SZ, P, P, P, SZ, P, P, P, SZ, P,
        c_uint64, c_uint32, P)
    sig("libdeflate_amd_targz_compress_batch", c_int, P, c_int, SZ, P, P, P, SZ, P, P, P, SZ,
        P, P, c_uint64, c_uint32, P)
    # a file of gzip members written: the bound (host arithmetic), and ranges of
    # a device buffer -> file (names, offsets and sizes on the host)
    sig("libdeflate_amd_gzip_members_compress_bound", SZ, P, SZ, P, P)
    sig("libdeflate_amd_gzip_members_compress_batch", c_int, P, SZ, P, P, P, SZ, P, P, P, SZ,
        P, P, c_uint32, c_uint32, P)
    # the first bytes of every stream: device batch (with a dictionary), one
    # host buffer (blocking), the heads of an indexed gzip-members file
    sig("libdeflate_amd_decompress_prefix_batch", c_int, P, c_int, SZ, P, P, P, P, P, P, P, P,
        P, P)
    sig("libdeflate_amd_decompress_prefix_batch_dict", c_int, P, c_int, SZ, P, SZ, P, P, P, P,
        P, P, P, P, P, P)
    sig("libdeflate_amd_decompress_prefix", c_int, P, c_int, P, SZ, P, SZ, psz)
    sig("libdeflate_amd_gzip_members_peek_batch", c_int, P, P, SZ, P, P, SZ, SZ, P, P, P, P)
    _lib = lib
    return lib


def reload_env():
    """Have the library read its LDA_* tuning switches again (it reads them
    once, at load)."""
    load().libdeflate_amd_reload_env()


def last_fanout():
    """shards (devices) the calling thread's last host-pointer batch used"""
    return int(load().libdeflate_amd_last_fanout())


def selfcheck():
    """the per-device hardware self-check again -> (status, dict of counters)"""
    out = (c_uint64 * 5)()
    rc = load().libdeflate_amd_selfcheck(out)
    keys = ("lds_lanes", "lds_out_of_order", "lds_conflicts", "loads", "stale_loads")
    return rc, dict(zip(keys, (int(x) for x in out)))


def stream_stats():
    """libdeflate_amd_stream_stats: what the last single-buffer decompress
    call of this thread did (see include/libdeflate_amd.h)."""
    out = (c_uint64 * 16)()
    load().libdeflate_amd_stream_stats(out)
    keys = ("parallel", "why_not", "filter_a", "blocks_found", "chunks_planned",
            "repairs", "chunks_decoded", "bytes", "us_in", "us_find", "us_count",
            "us_decode", "us_sum", "us_out", "windows", "host_chunks")
    return dict(zip(keys, [int(v) for v in out]))


def compress_last_schedule(compressor):
    """libdeflate_amd_compress_last_schedule of a compressor handle: how its
    last batch call was scheduled (see include/libdeflate_amd.h)."""
    out = (c_uint32 * 4)()
    load().libdeflate_amd_compress_last_schedule(compressor, out)
    return {"split": int(out[0]), "overlapped": int(out[1]), "head": int(out[2]),
            "tail": int(out[3])}


def compress_last_kernel(compressor):
    """libdeflate_amd_compress_last_kernel of a compressor handle: the name of
    the compress kernel its last batch call launched."""
    return load().libdeflate_amd_compress_last_kernel(compressor).decode()


def last_error():
    return load().libdeflate_amd_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (status {rc}): {last_error()}")
