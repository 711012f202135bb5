"""One small batch layout relocated to device offsets at and beyond 4 GiB.

A test builds its small case as the near-offset tests do - the stored bytes and
rows whose offsets start near 0 - and a Side per address space of the call (the
input, the output, the validity bytes) places that layout three times:

  A  shifted so that one row's bytes contain the byte at offset S31,
  B  shifted so that one row's bytes contain the byte at offset S32,
  C  shifted by FAR (beyond 4 GiB, bit 31 set in the low word, odd).

The three copies go into ONE call, and the sides take different orders (the
input "ABC", the written sides "CAB"), so that a row's input and output offsets
differ from bit 31 upwards and offsets within one batch lie more than 2^32
apart.  The straddled row is the largest one (common_row: the same row on
every side of a call), and the boundary is put into it twice: "mid" puts it in
the middle of the row, "access" at the row's byte ACCESS_BYTE, inside its
first 16-byte access.  A side uses one choice at S31 and the other at S32, and
the written sides swap them.

What is checked, without a tolerance (check_windows): every byte of every
window equals the expectation, and every other byte of the whole written tensor
- the 6 GiB outside the windows too - still is CANARY.  A truncated offset
writes inside the tensor at a low address, which guard bands would miss.

The memory is a DeviceMem (a torch CUDA tensor) in the GPU tests, and a
SparseMem (numpy windows over a fill) where tests/test_far_buffers.py proves on
the CPU that the checks bite.  Nothing here knows more of the GPU than torch's
tensor operations.
"""
import numpy as np

S31 = 1 << 31
S32 = 1 << 32
FAR = S32 + S31 + 5
CANARY = 0xA5       # tensors that are written
FILL = 0xFF         # input tensors: decodes as nothing valid (fill_is_no_stream)
SLACK = 64          # bytes of every tensor behind FAR + the layout
ACCESS_BYTE = 5     # "access": the boundary is this byte of the row (1..15)
SCAN_WORDS = 1 << 27    # int64 words per slice of the canary scan: 1 GiB read, 128 MiB of flags


def fill_is_no_stream():
    """FILL's first three bits are BFINAL with the reserved block type 3; two
    FILL bytes are no gzip magic and fail zlib's header check"""
    two = bytes([FILL, FILL])
    assert FILL & 1 and (FILL >> 1) & 3 == 3
    assert two != b"\x1f\x8b"
    assert two[0] & 15 != 8 and (two[0] * 256 + two[1]) % 31 != 0
    return True


def pick_row(spans, kind, pick=None):
    """(row, byte of it that the boundary falls on), the boundary strictly
    inside the row; pick: the row, where the caller chooses it"""
    need = 32 if kind == "access" else 2
    ok = [k for k, s in enumerate(spans) if s is not None and s[1] >= need]
    assert ok, "no row of %d bytes or more to straddle a boundary" % need
    k = max(ok, key=lambda k: spans[k][1]) if pick is None else pick
    assert k in ok
    return k, ACCESS_BYTE if kind == "access" else spans[k][1] // 2


def common_row(*sides_spans):
    """the row that is largest on its smallest side: straddled on every side
    of a call, it keeps a row's offsets on two sides apart from bit 31
    upwards in every copy (assert_placed)"""
    n = len(sides_spans[0])
    size = [min(s[k][1] if s[k] is not None else 0 for s in sides_spans) for k in range(n)]
    return max(range(n), key=lambda k: size[k])


class Side:
    """One address space of a call.  length: the bytes of the small layout;
    spans: (offset, size) of every row in it, None for a row that has nothing
    on this side; order: the placement of copies 0, 1, 2, a permutation of
    "ABC"; kinds: how the straddled row is chosen at S31 and at S32; pick:
    that row, where the sides of a call share it (common_row); align: what
    the call asks of this side's offsets (FAR itself is odd)."""

    def __init__(self, name, length, spans, order="ABC", kinds=("mid", "access"), pick=None,
                 align=1):
        self.name, self.length, self.order = name, int(length), order
        self.spans = [None if s is None else (int(s[0]), int(s[1])) for s in spans]
        assert sorted(order) == ["A", "B", "C"] and 0 < self.length < S31 // 4
        real = [s for s in self.spans if s is not None]
        assert all(0 <= o and o + n <= self.length for o, n in real)
        shift = {"C": FAR}
        for place, at, kind in (("A", S31, kinds[0]), ("B", S32, kinds[1])):
            k, byte = pick_row(self.spans, kind, pick)
            shift[place] = at - (self.spans[k][0] + byte)
            shift[place] -= shift[place] % align        # the boundary moves up in its row
            assert byte + align <= self.spans[k][1] and (kind != "access" or byte + align <= 16)
        shift["C"] += -shift["C"] % align
        self.shifts = [shift[p] for p in order]
        self.end = max(self.shifts) + self.length       # in_nbytes / out_avail / valid_avail
        self.nbytes = self.end + SLACK

    def at(self, copy, offset):
        return int(offset) + self.shifts[copy]

    def column(self, offsets):
        """the small layout's offsets of all rows -> those of the three copies"""
        return [self.at(c, o) for c in range(3) for o in offsets]

    def rows(self):
        """(copy, row, offset, size) of every row of every copy"""
        return [(c, k, self.at(c, s[0]), s[1]) for c in range(3)
                for k, s in enumerate(self.spans) if s is not None]

    def windows(self, want, defined=None):
        """the copies' windows for check_windows; want (and defined): the
        small layout's expectation, one for all copies or one per copy"""
        per = (lambda v, c: v[c] if isinstance(v, (list, tuple)) else v)
        return [Window(self.shifts[c], per(want, c), per(defined, c), "%s copy %d (%s)" % (
            self.name, c, self.order[c]), self.spans) for c in range(3)]


def assert_placed(inp, *outs):
    """What the placements were asked to be, on the rows themselves: on every
    side one row contains S31, one contains S32 and one starts at or beyond
    FAR, and no row's input and output offsets agree from bit 31 upwards (a
    copy at S32 has rows on both sides of it, so the words above bit 32 alone
    cannot differ for every row: they do for every row of the copy whose
    input is placed A)"""
    for side in (inp,) + outs:
        rows = side.rows()
        for at in (S31, S32):
            assert any(o < at < o + n for _, _, o, n in rows), (side.name, "no row across", at)
        assert any(o >= FAR for _, _, o, _ in rows), (side.name, "no row at FAR")
        assert side.end <= side.nbytes
    for out in outs:
        assert len(out.spans) == len(inp.spans)
        high = 0
        for c in range(3):
            for k, (a, b) in enumerate(zip(inp.spans, out.spans)):
                if a is None or b is None:
                    continue
                i, o = inp.at(c, a[0]), out.at(c, b[0])
                assert i >> 31 != o >> 31, (inp.name, out.name, c, k, hex(i), hex(o))
                high += i >> 32 != o >> 32
        assert high >= sum(a is not None and b is not None for a, b in zip(inp.spans, out.spans))


class Window:
    """want: the bytes [start, start + len(want)) must hold; defined: a bool
    array, False where nothing is said; spans: (offset, size) of the rows in
    it, for the message"""

    def __init__(self, start, want, defined=None, label="", spans=()):
        self.start = int(start)
        self.want = np.frombuffer(bytes(want), dtype=np.uint8) if isinstance(
            want, (bytes, bytearray)) else np.asarray(want, dtype=np.uint8)
        self.defined, self.label = defined, label
        self.spans = list(spans)
        self.end = self.start + self.want.size

    def where(self, i):
        for k, s in enumerate(self.spans):
            if s is not None and s[0] <= i < s[0] + s[1]:
                return "row %d byte %d" % (k, i - s[0])
        return "byte %d, in no row" % i


def check_windows(mem, windows, fill=CANARY):
    """every window holds what it should, and every other byte of `mem` still
    is `fill`; the message names the row and byte of the first wrong byte of
    every wrong window, and the position of the first byte written outside"""
    windows = sorted(windows, key=lambda w: w.start)
    said = []
    for a, b in zip(windows, windows[1:]):
        assert a.end <= b.start, ("windows overlap", a.label, b.label)
    for w in windows:
        got = mem.get(w.start, w.end)
        bad = got != w.want
        if w.defined is not None:
            bad &= w.defined
        bad = np.nonzero(bad)[0]
        if bad.size:
            i = int(bad[0])
            said.append("%s: %s (offset 0x%x) is 0x%02x, not 0x%02x" % (
                w.label, w.where(i), w.start + i, got[i], w.want[i]))
    stray = mem.stray([(w.start, w.end) for w in windows], fill)
    if stray is not None:
        said.append("stray write: offset %s, outside every window, is 0x%02x, not 0x%02x" % (
            hex(stray), int(mem.get(stray, stray + 1)[0]), fill))
    assert not said, "; ".join(said)


def _outside(windows, nbytes, start=0):
    at = start
    for a, b in sorted(windows):
        if at < a:
            yield at, a
        at = max(at, b)
    if at < nbytes:
        yield at, nbytes


class SparseMem:
    """The CPU stand-in for a tensor of nbytes: `fill` everywhere but in the
    windows that were written, a dict start -> numpy bytes."""

    def __init__(self, nbytes, fill):
        self.nbytes, self.fill, self.win = int(nbytes), fill, {}

    def put(self, at, data):
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        at = int(at)
        lo, hi = at, at + data.size       # (out of bounds is kept too, and found by stray())
        near = [s for s, v in self.win.items() if s <= hi and lo <= s + v.size]
        for s in near:
            lo, hi = min(lo, s), max(hi, s + self.win[s].size)
        merged = np.full(hi - lo, self.fill, dtype=np.uint8)
        for s in near:
            v = self.win.pop(s)
            merged[s - lo:s - lo + v.size] = v
        merged[at - lo:at - lo + data.size] = data
        self.win[lo] = merged

    def get(self, a, b):
        a, b = int(a), int(b)
        out = np.full(b - a, self.fill, dtype=np.uint8)
        for s, v in self.win.items():
            lo, hi = max(a, s), min(b, s + v.size)
            if lo < hi:
                out[lo - a:hi - a] = v[lo - s:hi - s]
        return out

    def stray(self, windows, fill):
        first = None
        lo = min([0] + list(self.win))
        hi = max([self.nbytes] + [s + v.size for s, v in self.win.items()])
        for a, b in _outside(windows, hi, lo):
            for s, v in self.win.items():
                lo, hi = max(a, s), min(b, s + v.size)
                bad = np.nonzero(v[lo - s:hi - s] != fill)[0] if lo < hi else ()
                if len(bad) and (first is None or lo + bad[0] < first):
                    first = int(lo + bad[0])
        return first


class DeviceMem:
    """A uint8 tensor of nbytes filled on the device (the CPU only where
    tests/test_far_buffers.py checks the scan itself)."""

    def __init__(self, torch, nbytes, fill, device="cuda"):
        self.torch, self.nbytes, self.fill, self.device = torch, int(nbytes), fill, device
        self.t = torch.full((self.nbytes,), fill, dtype=torch.uint8, device=device)

    def put(self, at, data):
        src = self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8)
        self.t[at:at + src.numel()] = src.to(self.device)

    def get(self, a, b):
        return self.t[a:b].cpu().numpy()

    def _first(self, a, b, fill):
        """the first byte of [a, b) that is not fill, by bytes (short ranges)"""
        bad = self.torch.nonzero(self.t[a:b] != fill)
        return a + int(bad[0]) if bad.numel() else None

    def stray(self, windows, fill):
        word = int.from_bytes(bytes([fill]) * 8, "little", signed=True)
        for a, b in _outside(windows, self.nbytes):
            a8, b8 = min(b, -(-a // 8) * 8), max(a, b // 8 * 8)
            if a8 >= b8:
                a8 = b8 = b
            for s, e in [(a, a8)] + [(s, min(b8, s + 8 * SCAN_WORDS)) for s in
                                     range(a8, b8, 8 * SCAN_WORDS)] + [(b8, b)]:
                if s >= e:
                    continue
                if e - s < 8:
                    at = self._first(s, e, fill)
                    if at is not None:
                        return at
                elif bool((self.t[s:e].view(self.torch.int64) != word).any()):
                    w = int(self.torch.nonzero(self.t[s:e].view(self.torch.int64) != word)[0])
                    return self._first(s + 8 * w, s + 8 * w + 8, fill)
        return None

    def free(self):
        self.t = None
        if self.device == "cuda":
            self.torch.cuda.empty_cache()


def device_input(torch, side, buf):
    """a tensor of FILL with the small layout's bytes in each copy's slice"""
    assert len(buf) == side.length
    mem = DeviceMem(torch, side.nbytes, FILL)
    for s in side.shifts:
        mem.put(s, buf)
    return mem


def device_output(torch, side):
    return DeviceMem(torch, side.nbytes, CANARY)


def free_memory(torch, tensors, room=2 << 30):
    """-> (free bytes, needed bytes) for `tensors` far tensors and what the
    scan and the call itself take"""
    free = torch.cuda.mem_get_info()[0]
    return free, tensors * (FAR + (64 << 20)) + room
