"""The far-offset checker (tests/far_buffers.py) bites: a fake call written in
numpy over SparseMem stand-ins - dicts of windows, no 6 GiB array - makes each
mistake the GPU tests are there to catch, and check_windows reports each with
the row and the byte.  With the correct fake call it passes.

The fake call is the shape of the chunk decoders: row k copies `lines` lines of
`width` bytes from in_off to out_off + line * pitch.
"""
import re

import numpy as np
import pytest

from tests import far_buffers as fb

M32 = fb.S32 - 1
SHAPES = [(8, 5, 3), (7, 1, 0), (10, 10, 2), (33, 2, 0)]      # width, lines, gap behind a line
BIG_PITCH = fb.S31 + 3
BIG_AT = fb.S31 // 2        # the out offset of the segment of three lines BIG_PITCH apart
BIG_WIDTH = 22       # three lines of it are row 3


def fake_call(rows, d_in, d_out, bug=None):
    for in_off, width, lines, out_off, pitch in rows:
        if bug == "in32":
            in_off &= M32
        if bug == "out32":
            out_off &= M32
        if bug == "out_sext":       # the low word taken for an int
            out_off = ((out_off & M32) ^ fb.S31) - fb.S31
        for y in range(lines):
            step = y * pitch
            if bug == "pitch32":
                step &= M32
            d_out.put(out_off + step, d_in.get(in_off + y * width, in_off + (y + 1) * width))


def layout():
    rng = np.random.default_rng(31)
    buf, rows, at = bytearray(), [], 0
    for width, lines, gap in SHAPES:
        buf += bytes(3)
        at += 2
        rows.append((len(buf), width, lines, at, width + gap))
        buf += rng.integers(1, 255, width * lines, dtype=np.uint8).tobytes()
        at += lines * (width + gap) - gap
    want = np.full(at, fb.CANARY, dtype=np.uint8)
    for in_off, width, lines, out_off, pitch in rows:
        for y in range(lines):
            want[out_off + y * pitch:out_off + y * pitch + width] = np.frombuffer(
                bytes(buf[in_off + y * width:in_off + (y + 1) * width]), dtype=np.uint8)
    return bytes(buf), rows, want


def run(bug):
    buf, rows, want = layout()
    inp = fb.Side("in", len(buf), [(r[0], r[1] * r[2]) for r in rows], "ABC", ("mid", "access"))
    out = fb.Side("out", len(want), [(r[3], r[4] * (r[2] - 1) + r[1]) for r in rows], "CAB",
                  ("access", "mid"))
    fb.assert_placed(inp, out)
    d_in, d_out = fb.SparseMem(inp.nbytes, fb.FILL), fb.SparseMem(out.nbytes, fb.CANARY)
    for s in inp.shifts:
        d_in.put(s, buf)
    far = [(inp.at(c, r[0]), r[1], r[2], out.at(c, r[3]), r[4]) for c in range(3) for r in rows]
    # the segment whose line * pitch crosses 2^32: its input is row 3 of copy 2
    far.append((inp.at(2, rows[3][0]), BIG_WIDTH, 3, BIG_AT, BIG_PITCH))
    fake_call(far, d_in, d_out, bug)
    windows = out.windows(want)
    src = buf[rows[3][0]:]
    for y in range(3):
        windows.append(fb.Window(BIG_AT + y * BIG_PITCH, src[y * BIG_WIDTH:(y + 1) * BIG_WIDTH],
                                 None, "big pitch line %d" % y, [(0, BIG_WIDTH)]))
    assert BIG_AT + 2 * BIG_PITCH > fb.S32 and windows[-1].end <= out.nbytes
    fb.check_windows(d_out, windows)


def test_fill_is_no_stream():
    assert fb.fill_is_no_stream()
    assert fb.FAR > fb.S32 and fb.FAR & fb.S31 and fb.FAR & 1


def test_correct_call_passes():
    run(None)


@pytest.mark.parametrize("bug, said", [
    # copies 0 and 2 lie beyond 4 GiB on the output side ("CAB"): their windows
    # stay canary from row 0 byte 0 on, and the bytes land outside every window
    ("out32", r"out copy 0 \(C\): row 0 byte 0 .* is 0xa5.*stray write: offset 0x"),
    ("out_sext", r"out copy 0 \(C\): row 0 byte 0 .* is 0xa5.*stray write: offset -0x"),
    # copy 2's input lies at FAR: it reads the fill
    ("in32", r"out copy 2 \(B\): row 0 byte 0 .* is 0xff"),
    # line 2 of the wide segment lands at line 0 + 6
    ("pitch32", r"big pitch line 2: row 0 byte 0 .* is 0xa5.*stray write"),
])
def test_each_mistake_is_reported_with_row_and_byte(bug, said):
    with pytest.raises(AssertionError) as e:
        run(bug)
    assert re.search(said, str(e.value)), str(e.value)


def test_a_wrapped_write_is_caught_by_the_scan_alone():
    """a write that wraps to a low address and leaves every window as it
    should be - the row is written at both places - is found by the scan of
    the bytes outside the windows, and by nothing else"""
    mem = fb.SparseMem(fb.FAR + 100, fb.CANARY)
    w = fb.Window(fb.FAR, b"\x01\x02\x03", None, "w", [(0, 3)])
    mem.put(fb.FAR, b"\x01\x02\x03")
    fb.check_windows(mem, [w])
    mem.put(fb.FAR & M32, b"\x01")
    with pytest.raises(AssertionError, match="stray write: offset 0x80000005"):
        fb.check_windows(mem, [w])


def test_sparse_mem_is_a_memory():
    mem = fb.SparseMem(1000, 7)
    mem.put(10, b"abc")
    mem.put(12, b"xyz")
    mem.put(500, b"q")
    assert bytes(mem.get(8, 17)) == b"\x07\x07abxyz\x07\x07" and bytes(mem.get(499, 502)) == b"\x07q\x07"
    assert mem.stray([(10, 15)], 7) == 500 and mem.stray([(10, 15), (500, 501)], 7) is None
    assert mem.stray([(11, 15), (500, 501)], 7) == 10


def test_the_device_scan_finds_every_byte_outside_the_windows(monkeypatch):
    """DeviceMem's scan - heads and tails by bytes, the body as int64 words in
    slices - on a CPU tensor, with slices of four words: a byte changed at
    every position outside the windows is found, and is the first found"""
    import torch
    monkeypatch.setattr(fb, "SCAN_WORDS", 4)
    n, windows = 203, [(13, 30), (30, 41), (97, 98), (150, 203)]
    mem = fb.DeviceMem(torch, n, fb.CANARY, device="cpu")
    assert mem.stray(windows, fb.CANARY) is None and mem.stray([], fb.CANARY) is None
    inside = set()
    for a, b in windows:
        inside |= set(range(a, b))
        mem.put(a, bytes(b - a))
    assert mem.stray(windows, fb.CANARY) is None
    for at in range(n):
        if at in inside:
            continue
        mem.put(at, b"\x00")
        assert mem.stray(windows, fb.CANARY) == at
        later = min(n - 1, at + 9)
        if later not in inside:
            mem.put(later, b"\x01")
            assert mem.stray(windows, fb.CANARY) == at
            mem.put(later, bytes([fb.CANARY]))
        mem.put(at, bytes([fb.CANARY]))
    assert bytes(mem.get(12, 14)) == bytes([fb.CANARY, 0])
    mem.free()
