"""The entropy kernel's own token encode (deflate_blockend.h under LDA_ENTROPY:
packed code tables in LDS, four consecutive tokens per thread, one workgroup
scan per window of 1024 tokens, a run of staging words per thread) and its
stored path (16-byte units copied from the input straight to the output)
against the fused kernels, which keep the one-token-per-thread loop and the
byte-by-byte stored path: for every input here the split path's bytes
(compress_batch with a bound and at least four buffers per CU) must equal the
fused path's (no bound), and every stream must decode to its input with the
reference library (the oracle where it is not built) and with zlib.

What cannot be reached through the API: a window of worst-case tokens (48 bits
each: a 15-bit length code with 5 extra bits and a 15-bit offset code with 13)
- a block with such codes has few such tokens.  The capacity of the staging
area for that window is held by the static_assert next to the encode loop;
the long-match input below gets the widths near the top, not the worst
window."""
import zlib

import numpy as np
import pytest
import torch

from libdeflate_amd import api
from tests import datagen, deflate_audit, oracle_util

pytestmark = pytest.mark.gpu

WB = {"deflate": -15, "zlib": 15, "gzip": 31, "bgzf": 31}   # a BGZF member is a gzip member
KIND = {"bgzf": "gzip"}
WINDOW = 4 * 256          # tokens per window of the encode loop: ENC_K x NT
GUARD = 0xA5


def _decoder():
    return oracle_util.load_ref() or oracle_util.load_oracle()


def _min_buffers():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _fill(chunks):
    """the chunks repeated to four buffers per CU (what takes the split path)"""
    return chunks * -(-_min_buffers() // len(chunks))


def _run(fmt, level, chunks, bound, avail=None):
    """One device batch; bound None = the unbounded (fused) call.  -> (streams,
    None where size 0 was reported; True when every byte outside the slots'
    out_avail - the guard - is untouched)"""
    c = api.Compressor(level)
    n = len(chunks)
    offs, pos = [], 0
    for x in chunks:
        offs.append(pos)
        pos += (len(x) + 15) // 16 * 16
    blob = bytearray(pos + 64)
    for o, x in zip(offs, chunks):
        blob[o:o + len(x)] = x
    data = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    in_off = torch.tensor(offs, dtype=torch.int64).cuda()
    in_n = torch.tensor([len(x) for x in chunks], dtype=torch.int64).cuda()
    av = [c.bound(fmt, len(x)) if avail is None else avail(x) for x in chunks]
    # slots start at odd alignments too: the staging base and the stored
    # copy's head depend on the slot's address mod 16
    slot = [a + 16 + (i * 7) % 16 for i, a in enumerate(av)]
    offv = np.cumsum([0] + slot[:-1]).tolist()
    out = torch.full((sum(slot) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor(offv, dtype=torch.int64).cuda()
    out_av = torch.tensor(av, dtype=torch.int64).cuda()
    out_n = torch.zeros(n, dtype=torch.int64, device="cuda")
    c.compress_batch(fmt, data, in_off, in_n, out, out_off, out_av, out_n, max_chunk=bound)
    torch.cuda.synchronize()
    host, sizes = out.cpu().numpy(), out_n.cpu().tolist()
    c.close()
    guard_ok = True
    for o, a, w in zip(offv, av, slot):
        guard_ok = guard_ok and bool((host[o + a:o + w] == GUARD).all())
    guard_ok = guard_ok and bool((host[sum(slot):] == GUARD).all())
    return [bytes(host[o:o + s]) if s else None for o, s in zip(offv, sizes)], guard_ok


def _check(fmt, chunks, comps):
    """every distinct input's stream decodes to it, with both decoders; every
    copy of an input came out the same"""
    ref = _decoder()
    first = {}
    for x, z in zip(chunks, comps):
        assert first.setdefault(bytes(x), z) == z
    for x, z in first.items():
        assert z is not None, len(x)
        assert zlib.decompress(z, WB[fmt]) == x
        r, ain, _, got = ref.decompress_ex(KIND.get(fmt, fmt), z, len(x))
        assert (r, ain, got) == (0, len(z), x)


def _split_and_fused(fmt, level, chunks):
    assert len(chunks) >= _min_buffers()
    # (a bound of 4 KiB or less selects the small-buffer kernel, which is
    # neither of the two paths compared here)
    bound = max(8192, max(len(x) for x in chunks))
    split, guard_ok = _run(fmt, level, chunks, bound)
    assert guard_ok
    _check(fmt, chunks, split)
    fused, guard_ok = _run(fmt, level, chunks, None)
    assert guard_ok
    assert split == fused
    return split


def _sweep():
    """2 x WINDOW prefixes at consecutive lengths of a text and of a 16-symbol
    source: a block's token count cannot be set through the API, so it is
    swept - it grows by at most one per byte, so it takes every value it
    passes, and here it passes the first two multiples of the window (text at
    two to three bytes per token, the 16-symbol source at under two)"""
    rng = np.random.default_rng(0xE7C0DE)
    text = datagen.text_chunk(16384, 97)
    sym = rng.integers(0x61, 0x71, 16384, dtype=np.uint8).tobytes()
    n = 2 * WINDOW
    return [text[:1200 + i] for i in range(n)] + [sym[:1200 + i] for i in range(n)]


def _token_counts(z):
    """tokens (literals and matches, without the end-of-block symbol) of every
    Huffman-coded block of a raw DEFLATE stream"""
    _, blocks = deflate_audit.walk(z, "deflate")
    return [sum(b.ll_hist[:256]) + len(b.matches) for b in blocks if b.type != 0]


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip", "bgzf"])
def test_token_counts_at_every_residue_of_the_window(fmt, level):
    chunks = _sweep()
    k = -(-_min_buffers() // len(chunks))
    comps = _split_and_fused(fmt, level, chunks * k)
    if fmt == "deflate":
        # the sweep did what it is for: the blocks' token counts take every
        # residue of the window, below one window and above two
        counts = [n for z in comps[:len(chunks)] for n in _token_counts(z)]
        print("token counts %d..%d, %d residues of %d" %
              (min(counts), max(counts), len({n % WINDOW for n in counts}), WINDOW))
        assert min(counts) < WINDOW and max(counts) > 2 * WINDOW
        assert {n % WINDOW for n in counts} == set(range(WINDOW))


def _shaped():
    """inputs chosen for what the encode loop and the stored copy have new"""
    rng = np.random.default_rng(0x5E1176)
    text = datagen.text_chunk(1 << 18, 33)
    rnd = rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()
    out = []
    # content switches: retro splits, so later blocks whose first token is at
    # any index mod 4 of the buffer's list; stored blocks between coded ones
    # at any byte phase
    for i in range(12):
        a, b = 30000 + 1237 * i, 20000 + 811 * i
        out.append(text[:a] + rnd[:b] + text[a:a + 30000 + i])
    out.append(text[:200000])                      # several blocks per buffer
    # long distances, long lengths: a 20 000-byte random period repeated, a byte
    # changed every ~200 - offsets with 13 extra bits, lengths with 5
    period = rnd[100000:120000]
    rep = bytearray((period * 4)[:65536])
    for p in range(150, len(rep), 199):
        rep[p] ^= 0x55
    out.append(bytes(rep))
    # stored blocks: random bytes at lengths around the 16-byte units and the
    # 65535-byte pieces of the stored copy
    out += [rnd[:n] for n in (15, 16, 17, 31, 33, 4096, 65535, 65536, 65537, 150001)]
    out += [text[:n] for n in (24, 40, 60)]        # the static code
    out += [b"", b"a", b"ab", b"abc"]
    return out


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_shaped_inputs(fmt, level):
    _split_and_fused(fmt, level, _fill(_shaped()))


@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
def test_slot_one_byte_short(fmt):
    """an output slot one byte smaller than the stream: size 0 is reported and
    nothing behind the slot is written (the stored copy writes whole 16-byte
    units: the check in front of it is what keeps them inside)"""
    chunks = _fill(_shaped())
    bound = max(len(x) for x in chunks)
    exact, guard_ok = _run(fmt, 6, chunks, bound)
    assert guard_ok
    _check(fmt, chunks, exact)
    sizes = {bytes(x): len(z) for x, z in zip(chunks, exact)}
    fit, guard_ok = _run(fmt, 6, chunks, bound, avail=lambda x: sizes[bytes(x)])
    assert guard_ok and fit == exact
    short, guard_ok = _run(fmt, 6, chunks, bound, avail=lambda x: sizes[bytes(x)] - 1)
    assert guard_ok
    assert short == [None] * len(chunks)
