"""Calls of DIFFERENT families queued back to back on ONE Compressor or
Decompressor, with no synchronisation between them.

The two passages of include/libdeflate_amd.h this module tests:

  :529-535  "the batch calls only ENQUEUE work on `stream`.  A compressor /
            decompressor owns device scratch ... that a batch uses until it
            completes, so an object may have batches in flight on ONE stream
            at a time (they are ordered by the stream)"
  :1511-1515 "nothing comes back to the host and the device is not waited
            for, with two exceptions: scratch of the object grows on the
            host ... and the plan goes up through one pinned block per object,
            so a call waits until the previous call on the same object has had
            its plan uploaded (its stream has reached that copy, not its
            kernels)"

One object's scratch is shared by families that lay it out differently (the
table in tests/object_steps.py says which step touches which field), so a
sequence checks what no single-family test can: a stale candidate table read
by the next reader, a counter or descriptor block overwritten under queued
kernels, a plan upload overtaking the call before, a buffer freed by growth
under queued work, an internal stream not drained on an error return.

`expected` never comes from the library (tests/test_object_steps.py holds every
step's expectation against a second CPU source), with one exception: the bytes
a compressor step wrote are also compared with what a FRESH object returns for
the same call made alone and synchronised - which sits beside a CPU decode of
the same bytes in the step's own check.

The blocking calls run on the object's own two streams.  Those that take a
stream (decompress_large, _large_index, read_zip_large) make them wait for it
with an event; the host-pointer calls take none, so they wait on the host until
the device has nothing in flight before they reserve and reuse the scratch
(StreamPair::enter(), csrc/host_context.hip).  The test synchronises in front
of neither: D3, C3 and the shuffles make them right behind enqueued calls.

Every sequence runs plainly first (which grows the scratch and is the plain
answer) and then piled up behind torch.cuda._sleep on the same object, where
most calls return with the stream still busy; the count is printed, not
asserted: plan-uploading calls wait for the previous plan's upload."""
import random

import pytest

from libdeflate_amd import binding
from tests import object_steps as O

pytestmark = pytest.mark.gpu

SLEEP = 200_000_000     # cycles; tests/test_tar_gpu.py::test_calls_only_enqueue uses the same


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def steps(oracle):
    return O.decompressor_steps(oracle)


@pytest.fixture(scope="module")
def rsteps(steps):
    """the older catalogue and the PNG and shuffle readers' beside it (the
    seeded shuffles draw from `steps` alone, as they always have)"""
    return {**steps, **O.reader_steps()}


@pytest.fixture(params=["current", "side"])
def stream(request, torch):
    """the current stream, and a side stream as tests/test_seek_gpu.py::
    test_a_side_stream passes one; every step's inputs are copied on it"""
    return torch.cuda.current_stream() if request.param == "current" else torch.cuda.Stream()


@pytest.fixture
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def run_sequence(obj, steps, stream, pile_up, fresh=None, label=""):
    """prepare all, one synchronise, [sleep on the stream,] every call in
    order with no synchronisation, one synchronise, check all.  -> what the
    compressor steps wrote"""
    import torch
    with torch.cuda.stream(stream):
        handles = [s.prepare(torch, obj) for s in steps]
    torch.cuda.synchronize()
    if pile_up:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(SLEEP)
    early = 0
    for s, h in zip(steps, handles):
        s.launch(obj, h, stream)
        early += not s.blocking and not stream.query()
    torch.cuda.synchronize()
    print(f"\n[{label}{' piled up' if pile_up else ''}] {early} of "
          f"{sum(not s.blocking for s in steps)} enqueue-only calls ({len(steps)} calls) returned "
          f"with the stream still busy")
    outs = []
    for k, (s, h) in enumerate(zip(steps, handles)):
        try:
            got = s.check(h)
        except AssertionError as e:
            names = [x.name for x in steps]
            raise AssertionError(f"step {k} ({s.name}) of {names}"
                                 f"{' piled up' if pile_up else ''}: {e}") from None
        if fresh is not None and isinstance(s, O.CStep):
            assert got == fresh[s.name], (s.name, "differs from a fresh object's bytes",
                                          [x.name for x in steps])
        outs.append(got)
    return outs


def both(obj, seq, stream, label, fresh=None):
    """plainly first, then piled up on the same object"""
    a = run_sequence(obj, seq, stream, False, fresh, label)
    b = run_sequence(obj, seq, stream, True, fresh, label)
    return a, b


# ---------------------------------------------------------------- decompressor

def test_five_readers_share_one_scratch(dec, rsteps, stream):
    """D1: ZIP, tar, BGZF, gzip members through d->bgzf and d->bgzf_up, the
    false-candidate and overflow files between the good ones, then the ranged
    and selected reads through the four indices in reverse order; the PNG
    decodes and the shuffle read, which stage their plans through the same
    pipeline on the host, between them - the first in front of every step that
    grows d->bgzf (a fresh object: "zip" is the first to reserve more than a
    few KiB, "bgzf" and "zip-large" grow it again), the others behind"""
    names = ["png", "zip", "shuffle", "zip-false", "tar", "png-pixels", "zip-overflow", "bgzf",
             "png-ex", "tar-overflow", "gzm", "bgzf-walk", "png-zero", "zip-defect", "tar-pax",
             "gzm-false", "shuffle",
             "bgzf-read", "png-ex-raw", "tar-read", "png", "zip-read", "png-ex", "zip-large",
             "png-pixels", "gzm-peek", "shuffle"]
    both(dec, [rsteps[n] for n in names], stream, "D1")


@pytest.mark.parametrize("mode", ["1", "0"])
def test_three_decoders_share_the_token_scratch(dec, steps, stream, monkeypatch, mode):
    """D2: wave mapping (1) and lane mapping (0); the first and the last step
    are the same batch and give the same bytes (both checked against the
    oracle's)"""
    monkeypatch.setenv("LDA_INFLATE_PAR", mode)
    binding.reload_env()
    names = ["batch300", "prefix", "sizes", "packed", "dict-zlib", "dict-deflate", "batch2",
             "batch-synth", "batch300"]
    both(dec, [steps[n] for n in names], stream, f"D2 par={mode}")


def test_blocking_calls_between_enqueued_ones(dec, steps, stream):
    """D3: the batch right behind the damaged large stream queues on an object
    whose many-wave attempt has just been refused or has failed"""
    names = ["batch300", "large", "batch2", "large-damaged", "batch300", "large-index", "seek-read",
             "batch-host", "ex-host", "zip-large", "batch-synth"]
    both(dec, [steps[n] for n in names], stream, "D3")


def test_scratch_grows_under_queued_work(dec, steps, stream):
    """D4: a fresh object and no warm-up pass: every larger call grows the
    scratch (hipFree + hipMalloc) with the smaller call still queued"""
    names = ["batch-small4", "zip-max8", "bgzf-max4", "batch-small600", "zip-max3000",
             "bgzf-max4000", "batch-small1", "zip-max8", "bgzf-max4", "batch-small2500"]
    run_sequence(dec, [steps[n] for n in names], stream, True, label="D4")


def test_failing_and_refused_calls_leave_the_object_whole(dec, rsteps, stream):
    """D5: refusals before any device work, defect archives and short-output
    batches between good steps on a busy stream; then one more good sequence.
    The PNG decodes' and the shuffle read's refusals stand between good calls
    of the same kind: the refusal path is the readers' shared one, and it
    leaves d->bgzf_up as it found it"""
    names = ["zip", "refused-zip-space", "tar", "refused-tar-row", "batch-short", "refused-zip-input",
             "png", "refused-png", "png-pixels", "refused-png-pixels", "png",
             "zip-defect", "batch2", "refused-tar-space", "tar-defect", "zip-read-defect",
             "png-ex", "refused-png-ex", "png-ex-raw", "shuffle", "refused-shuffle", "shuffle",
             "refused-zip-large-row", "bgzf", "zip-space", "refused-zip-row", "refused-tar-input",
             "gzm", "batch-synth"]
    both(dec, [rsteps[n] for n in names], stream, "D5")
    both(dec, [rsteps[n] for n in ("zip", "tar", "bgzf", "gzm", "batch2", "tar-read", "zip-read",
                                    "png", "shuffle")],
         stream, "D5 after")


@pytest.mark.parametrize("seed", range(6))
def test_seeded_shuffles(dec, steps, stream, seed):
    """D6: ten steps drawn with repeats from the whole catalogue"""
    pool = sorted(steps)
    seq = random.Random(0xD6000 + seed).choices(pool, k=10)
    try:
        both(dec, [steps[n] for n in seq], stream, f"D6 seed {seed}")
    except AssertionError as e:
        raise AssertionError(f"seed {seed}, steps {seq}: {e}") from None


# ------------------------------------------------------------------ compressor

_fresh = {}


def fresh_bytes(level):
    """what a fresh Compressor returns for every step made alone and
    synchronised; once per level"""
    import torch
    from libdeflate_amd import api
    if level not in _fresh:
        out = {}
        for name, s in O.compressor_steps().items():
            c = api.Compressor(level)
            out[name] = run_sequence(c, [s], torch.cuda.current_stream(), False,
                                     label=f"fresh {name}")[0]
            c.close()
        _fresh[level] = out
    return _fresh[level]


@pytest.fixture
def comp(request):
    from libdeflate_amd import api
    c = api.Compressor(getattr(request, "param", 6))
    yield c
    c.close()


@pytest.mark.parametrize("comp", [1, 6, 12], indirect=True, ids=lambda v: f"level{v}")
def test_the_writers_share_one_compressor(comp, stream):
    """C1: c->zipw, c->zipw_up, c->large and c->scratch through every writer;
    the first and the last step are the same batch and give the same bytes"""
    cs = O.compressor_steps()
    names = ["c-batch-large", "c-batch-small", "c-zip", "c-gzm", "c-png", "c-tar", "c-targz",
             "c-large", "c-bgzf", "c-dict", "c-batch-large"]
    for outs in both(comp, [cs[n] for n in names], stream, f"C1 level {comp.level}",
                     fresh_bytes(comp.level)):
        assert outs[0] == outs[-1]


def test_compressor_scratch_grows_under_queued_work(comp, stream):
    """C2: a fresh object, ascending and descending chunk and entry counts,
    piled up from the first call"""
    cs = O.compressor_steps()
    names = ["c-batch-small3", "c-zip2", "c-png", "c-tar2", "c-batch-small500", "c-zip", "c-png",
             "c-tar", "c-gzm", "c-batch-small3", "c-zip2", "c-targz", "c-tar2", "c-batch-large",
             "c-batch-small3"]
    run_sequence(comp, [cs[n] for n in names], stream, True, fresh_bytes(6), "C2")


def test_host_calls_between_enqueued_compress_calls(comp, stream):
    """C3"""
    cs = O.compressor_steps()
    names = ["c-batch-large", "c-batch-host", "c-zip", "c-one", "c-tar", "c-bgzf-host", "c-large",
             "c-batch-small", "c-batch-host", "c-gzm"]
    both(comp, [cs[n] for n in names], stream, "C3", fresh_bytes(6))


@pytest.mark.parametrize("seed", range(9))
def test_seeded_compressor_shuffles(comp, stream, seed):
    """C4: as D6; seeds 0 to 5 draw from the catalogue as it was before the PNG
    writer's step joined it (the sequences they have always run), 6 to 8 from
    all of it"""
    cs = O.compressor_steps()
    pool = sorted(n for n in cs if seed >= 6 or n != "c-png")
    seq = random.Random(0xC4000 + seed).choices(pool, k=10)
    try:
        both(comp, [cs[n] for n in seq], stream, f"C4 seed {seed}", fresh_bytes(6))
    except AssertionError as e:
        raise AssertionError(f"seed {seed}, steps {seq}: {e}") from None
