"""Escape-prefix literal blocks counted one lane per block (inflate_wave.hpp count_flat_group):
incompressible data, whose blocks' literal/length code is 255 (254, 252) literals of 8 bits with the
longer codes under the remaining all-ones prefix.  The decode must equal the oracle's -- output,
consumed bits, Reason of the first error -- with the flat groups on (the default) and off
(NDFL_FLAT=0: every block in wave form), one wave per chain (NDFL_COUNT_W=1), and the flat
groups must actually have counted chains.
Streams: random bytes; random bytes with sparse byte runs (length codes under the escape prefix,
decoded through the global table record); with dense runs (more than NDFL_FLAT_OTHER_MAX such
tokens per block: the chain goes back to the wave decode); random blocks between text blocks;
truncated and corrupted random streams (errors inside a flat block go back to the wave decode,
which reports them).  Every decode also passes the emit passes' check of each count-pass segment
record (NDFL_E_INTERNAL otherwise).  The flat groups' records are also replayed by decodes that do
not run from bit 0 to the stream's end: ranges between block seams (window given or deferred), a
range that ends inside the flat region, and a partial input cut inside a block.
Reference semantics: D/decomp/Open.java:83-618."""
import os

import numpy as np
import pytest

import corpus
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _ctx(flat):
    """A context with the flat groups on or off and one wave per chain (NDFL_COUNT_W=1: streams this
    small would otherwise be counted four waves per chain, a kernel without flat groups), flat groups
    at any stream size (NDFL_FLAT_MIN=0)."""
    import ndfl
    env = {"NDFL_FLAT": str(flat), "NDFL_COUNT_W": "1", "NDFL_FLAT_MIN": "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ndfl.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    return {1: _ctx(1), 0: _ctx(0)}


def _runs(data, every, ln, rng):
    b = bytearray(data)
    for p in range(int(rng.integers(0, every)), len(b) - ln, every):
        b[p:p + ln] = bytes([b[p]]) * ln
    return bytes(b)


STREAMS = {}
RND = {}                                        # the "random" stream's data and block seams (bits)


def _streams():
    if not STREAMS:
        rng = np.random.default_rng(61)
        rnd = rng.integers(0, 256, 3 << 20, dtype=np.uint8).tobytes()
        text = corpus.c3_text(1 << 20).numpy().tobytes()
        mixed = b"".join(rnd[i:i + 65536] + text[i // 3:i // 3 + 65536] for i in range(0, 1 << 20, 65536))
        seams = [0]
        for b in O.block_bits(rnd):
            seams.append(seams[-1] + b)
        RND.update({"data": rnd, "seams": seams})
        STREAMS.update({
            "random": O.deflate(rnd),
            "random_sparse_runs": O.deflate(_runs(rnd, 2500, 7, rng)),
            "random_dense_runs": O.deflate(_runs(rnd, 400, 5, rng)),
            "random_text": O.deflate(mixed),
            "random_dynamic_stream": O.deflate(rnd[:1 << 20], "FULL_DYNAMIC"),
        })
    return STREAMS


def _same(ctx, comp):
    r, out, bits = ctx.inflate(comp)
    oreason, oout, obits = O.inflate(comp)
    assert (None if r is None else r.name) == oreason
    assert out == oout
    if oreason is None:
        assert bits == obits
    return ctx.timings()["inflate_flat_chains"]


@pytest.mark.parametrize("name", ["random", "random_sparse_runs", "random_dense_runs", "random_text",
                                  "random_dynamic_stream"])
def test_flat_groups_match_oracle(ctxs, name):
    comp = _streams()[name]
    nflat = _same(ctxs[1], comp)
    assert _same(ctxs[0], comp) == 0
    if name in ("random", "random_text"):
        assert nflat > 0                        # (the path under test ran)


def test_flat_truncated_and_corrupted(ctxs):
    comp = _streams()["random"]
    rng = np.random.default_rng(5)
    cases = [comp[:len(comp) // 2], comp[:len(comp) // 3 + 17]]
    for _ in range(4):
        bad = bytearray(comp)
        k = int(rng.integers(len(bad) // 8, len(bad)))
        bad[k] ^= 0x5A
        cases.append(bytes(bad))
    for c in cases:
        _same(ctxs[1], c)


# ---- the flat group's records replayed by range and partial-input decodes ----------------------------
# (the "random" stream: 48 blocks of 64 KiB, every one an escape-prefix literal block)

def _rnd():
    comp = _streams()["random"]
    return comp, RND["data"], RND["seams"]


def _range(ctx, comp, s_bit, e_bit, window, ref, deferred=False):
    """ndfl_inflate_range on device memory; returns the decoded bytes after checking code, length, bits."""
    import torch
    import ndfl
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dev_in = torch.frombuffer(bytearray(comp), dtype=torch.uint8).cuda()
        dl, n = len(window), len(ref[1])
        out = torch.full((dl + n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        wt = torch.frombuffer(bytearray(window), dtype=torch.uint8).cuda() if dl else None
        flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
        if deferred:
            flags |= ndfl.DICT_DEFERRED
        elif dl:
            out[:dl] = wt
        r, olen, bits = ctx.inflate_range_raw(dev_in.data_ptr(), len(comp), s_bit, e_bit, out.data_ptr(), dl, n + 64,
                                              flags)
        assert (r, olen, bits) == (0, n, ref[2])
        nflat = ctx.timings()["inflate_flat_chains"]
        if deferred:
            out[:dl] = wt
            ctx.inflate_resolve()
        return bytes(out[dl:dl + n].cpu().numpy()), nflat
    finally:
        ctx.set_stream(None)


@pytest.mark.parametrize("deferred", [False, True])
def test_flat_range_between_seams(ctxs, deferred):
    """A range that starts and ends on block seams inside the flat region, with the 32 KiB window
    before it (given, or deferred and resolved afterwards)."""
    comp, data, seams = _rnd()
    window = data[5 * 65536 - 32768:5 * 65536]
    ref = O.inflate_range(comp, seams[5], seams[20], window)
    assert ref[0] is None and ref[1] == data[5 * 65536:20 * 65536]
    out, nflat = _range(ctxs[1], comp, seams[5], seams[20], window, ref, deferred)
    assert out == ref[1]
    assert nflat > 0                            # (the path under test ran)
    out, nflat = _range(ctxs[0], comp, seams[5], seams[20], window, ref, deferred)
    assert out == ref[1] and nflat == 0


def test_flat_range_end_inside_flat_region(ctxs):
    """From bit 0 to a seam: the group's stop lies inside the flat region."""
    comp, data, seams = _rnd()
    ref = O.inflate_range(comp, 0, seams[7], b"")
    assert ref[0] is None and ref[1] == data[:7 * 65536]
    out, nflat = _range(ctxs[1], comp, 0, seams[7], b"", ref)
    assert out == ref[1]
    assert nflat > 0
    out, nflat = _range(ctxs[0], comp, 0, seams[7], b"", ref)
    assert out == ref[1] and nflat == 0


def test_flat_partial_input_cut_inside_block(ctxs):
    """NDFL_IN_PARTIAL with the input cut in the middle of the tenth block: NEED_INPUT, the first
    nine blocks' output, consumed bits at the tenth block's start."""
    import ctypes
    import ndfl
    comp, data, seams = _rnd()
    cut = comp[:(seams[9] + seams[10]) // 16]
    assert seams[9] < 8 * len(cut) < seams[10]
    for flat in (1, 0):
        ctx = ctxs[flat]
        cin = ctypes.create_string_buffer(cut, len(cut))
        cap = 10 * 65536 + 64
        cout = ctypes.create_string_buffer(cap)
        r, olen, bits = ctx.inflate_range_raw(ctypes.addressof(cin), len(cut), 0, None, ctypes.addressof(cout), 0, cap,
                                              ndfl.IN_PARTIAL)
        assert (r, olen, bits) == (ndfl.NEED_INPUT, 9 * 65536, seams[9])
        assert cout.raw[:olen] == data[:9 * 65536]
        assert (ctx.timings()["inflate_flat_chains"] > 0) == (flat == 1)
