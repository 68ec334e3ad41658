"""ndfl_inflate / ndfl_inflate_range on hand-built LZ77 token streams (token_stream.py): the copy a
lane executes itself (wr_copy's five width classes, after wr_flush_word and the held literal words),
the decision to defer (src < dst0, the lane's own pend bits in 32-byte groups), the dist-1 anchor
(lsp / lastsrc), the resolve rounds (ndfl_inflate_resolve_kernel: six queued on the device, the rest
in the host-checked resolve_rounds loop) and the dictionary bound -- in both emit kernels
(ndfl_inflate_emit_fast_kernel by default, ndfl_inflate_emit_wave_kernel alone with NDFL_EMIT_FAST=0,
after a hand-over with NDFL_NO_BT=1) and with the count pass's fixed segment width (NDFL_COUNT_W=1).

Every decode goes into a device buffer pre-filled with 0xEE: a copy that wrongly runs from a byte
that is still pending reads 0xEE, not a stale correct value.  The reference is token_stream.expand
(byte-at-a-time, sharing nothing with the library or the oracle); the CPU oracle must agree as well.
The same streams then go through ndfl_inflate_batch and ndfl_inflate_members."""
import functools
import zlib

import numpy as np
import pytest

import knobs
import oracle_lib as O
import token_stream as T

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 64
E_CAPACITY = -3
COPY_BEFORE_CODE = O.REASONS.index(T.COPY_BEFORE) + 1

MODES = {"default": {}, "full_only": {"NDFL_EMIT_FAST": "0"}, "no_bt": {"NDFL_NO_BT": "1"},
         "count_w": {"NDFL_COUNT_W": "1"}}

# Family D, distance 7: measured on an MI355X at 64 KiB, 128 KiB, ... 8 MiB of output, 128 KiB is the
# smallest size after which the six device-queued resolve rounds leave pending groups (64 KiB: 0;
# 128 KiB: 73..261; 1 MiB: 28,5xx..28,8xx; 8 MiB: ~250,000 -- in all four modes).  The hops race
# benignly within a launch, so that size cannot be derived from the code; the test uses 8 times it.
D7_SMALLEST_ENGAGING = 128 << 10
D7_OUT_LEN = 8 * D7_SMALLEST_ENGAGING


@pytest.fixture(scope="module", params=list(MODES))
def ctx(request):
    """A context per mode: the library reads its switches when a context is created."""
    import torch
    c = knobs.context(**MODES[request.param])
    c.set_stream(torch.cuda.current_stream().cuda_stream)      # ordered with torch's fills and copies
    c.mode = request.param
    return c


@pytest.fixture(scope="module")
def plain():
    import torch
    import ndfl
    c = ndfl.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@functools.lru_cache(maxsize=None)
def oracle(comp):
    return O.inflate(comp)


def to_dev(data):
    import torch
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def first_diff(got, want):
    a = np.frombuffer(got, dtype=np.uint8)
    b = np.frombuffer(want, dtype=np.uint8)
    return int(np.flatnonzero(a != b)[0])


def decode_checked(ctx, s, want_reason, want, capacity=True):
    """One stream through ndfl_inflate on device buffers: Reason, out_len, consumed bits and bytes
    against `want` (expand's) and the oracle's, the guard bytes, and the two capacity edges.  A valid
    stream gets GUARD bytes of room after its length and must leave them untouched.  A stream that ends
    with a Reason gets room for the tokens behind the error as well (include/ndfl.h promises the bytes
    before the error, and says nothing of out[out_len, out_cap)); its guard lies after out_cap."""
    import torch
    import ndfl
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
    oreason, oout, obits = oracle(s.comp)
    assert (oreason, oout) == (want_reason, want), s.name
    n = len(want)
    cap = n + GUARD if want_reason is None else n + 1024
    src = to_dev(s.comp)
    out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    r, olen, bits = ctx.inflate_raw(src.data_ptr(), len(s.comp), out.data_ptr(), cap, flags)
    got = out.cpu().numpy().tobytes()
    where = (ctx.mode, s.name)
    assert r == (0 if want_reason is None else O.REASONS.index(want_reason) + 1), (where, r)
    assert olen == n, (where, olen, n)
    if got[:n] != want:
        at = first_diff(got[:n], want)
        raise AssertionError((where, "first wrong byte at output offset", at, "case", T.case_at(s, at),
                              "got", got[at], "want", want[at]))
    guard_from = n if want_reason is None else cap
    assert got[guard_from:] == bytes([FILL]) * (len(got) - guard_from), (where, "guard bytes written")
    if want_reason is None:
        assert bits == obits, (where, bits, obits)
    if want_reason is None and capacity:
        out.fill_(FILL)
        r, olen, bits = ctx.inflate_raw(src.data_ptr(), len(s.comp), out.data_ptr(), n, flags)
        assert (r, olen, bits) == (0, n, obits), (where, "exact capacity", r, olen)
        got = out.cpu().numpy().tobytes()
        assert got[:n] == want and got[n:] == bytes([FILL]) * (2 * GUARD), (where, "exact capacity")
        if n:
            out.fill_(FILL)
            r, olen, _ = ctx.inflate_raw(src.data_ptr(), len(s.comp), out.data_ptr(), n - 1, flags)
            assert (r, olen) == (E_CAPACITY, n), (where, "one byte short", r, olen)
            assert out[n - 1:].cpu().numpy().tobytes() == bytes([FILL]) * (2 * GUARD + 1), (where, "one byte short")


@pytest.mark.parametrize("fam", ["A", "B", "C", "E"])
def test_copy_families(ctx, fam):
    """A: wr_copy's width classes at every flushed-word remainder and held-word count, the second copy
    reading the first one's bytes; B: the defer decision with the source wholly final, straddling the
    final / pending edge by one byte either way, wholly pending, or reaching before the pending run, at
    every bit of a pend word; C: dist-1 runs that span lanes, follow a deferred copy or precede one;
    E: distances up to 32,768 and copies of copies."""
    for s in T.family(fam):
        assert s.reason is None
        decode_checked(ctx, s, None, s.out)


def test_dictionary_bound_whole_stream(ctx):
    """F: a copy whose distance equals its output position reaches byte 0 and is valid; one byte more is
    COPY_FROM_BEFORE_DICTIONARY_START with out_len == the position and the bytes before it -- in the
    first block, after dynamic blocks, and ahead of a later block's reserved length symbol (the first
    error in stream order wins)."""
    streams = T.family("F")
    assert sum(1 for s in streams if s.reason) == 30 and sum(1 for s in streams if s.reason is None) == 33
    for s in streams:
        decode_checked(ctx, s, s.reason, s.out)


@pytest.mark.parametrize("distance", [1, 32768])
def test_depth_runs_and_far_chains(ctx, distance):
    """D with distance 1 (every byte the previous one, 1 MiB deep) and 32,768 (each block's bytes the
    previous 32 KiB's)."""
    s, want = T.family_d(distance)
    decode_checked(ctx, s, None, want, capacity=False)


def test_depth_engages_the_host_rounds(ctx):
    """D with (258, 7) copies only: every byte depends on the previous block's, so the reference chains
    are as deep as the output is long and pointer jumping (four hops per launch, six launches queued on
    the device) leaves work for the host-checked resolve_rounds loop; ndfl_ctx_timings [9] says so.
    Measured: the smallest output size that reports > 0 is 128 KiB (D7_SMALLEST_ENGAGING); this test
    runs at 8 times that, 1 MiB (D7_OUT_LEN)."""
    assert D7_OUT_LEN == 1 << 20
    s, want = T.family_d(7, D7_OUT_LEN)
    decode_checked(ctx, s, None, want, capacity=False)
    assert ctx.timings()["inflate_pending_after_dev_rounds"] > 0, ctx.mode


def test_pending_count_is_zero_when_six_rounds_suffice(ctx):
    s = T.by_name("F_258_exact_first")
    decode_checked(ctx, s, None, s.out, capacity=False)
    assert ctx.timings()["inflate_pending_after_dev_rounds"] == 0


def test_dictionary_bound_range_decode(ctx):
    """ndfl_inflate_range from a block seam with dict_len window bytes: a first-block copy that reaches
    exactly dict_len + n bytes back reads the window's first byte; one byte further is
    COPY_FROM_BEFORE_DICTIONARY_START with out_len == n.  With NDFL_DICT_DEFERRED the valid streams give
    the same bytes once the window is written and ndfl_inflate_resolve has run."""
    import torch
    import ndfl
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
    for c in T.family_f_ranges():
        where = (ctx.mode, c.name)
        oreason, oout, obits = O.inflate_range(c.comp, c.seams[c.k], None, c.window)
        assert (oreason, oout) == (c.reason, c.out), where
        src = to_dev(c.comp)
        n, dl = len(c.out), c.dict_len
        cap = n + GUARD if c.reason is None else n + 400
        out = torch.full((dl + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if dl:
            out[:dl] = to_dev(c.window)
        r, olen, bits = ctx.inflate_range_raw(src.data_ptr(), len(c.comp), c.seams[c.k], None, out.data_ptr(), dl, cap,
                                              flags)
        assert r == (0 if c.reason is None else COPY_BEFORE_CODE), (where, r)
        assert olen == n, (where, olen, n)
        got = out.cpu().numpy().tobytes()
        assert got[:dl] == c.window and got[dl:dl + n] == c.out, where
        if c.reason is None:
            assert bits == obits, where
            assert got[dl + n:] == bytes([FILL]) * (len(got) - dl - n), where
            out.fill_(FILL)                                  # (the window too: it arrives later)
            r, olen, bits = ctx.inflate_range_raw(src.data_ptr(), len(c.comp), c.seams[c.k], None, out.data_ptr(), dl,
                                                  cap, flags | ndfl.DICT_DEFERRED)
            assert (r, olen, bits) == (0, n, obits), (where, "deferred", r, olen)
            if dl:
                out[:dl] = to_dev(c.window)
            ctx.inflate_resolve()
            got = out.cpu().numpy().tobytes()
            assert got[:dl] == c.window and got[dl:dl + n] == c.out, (where, "deferred")
            assert got[dl + n:] == bytes([FILL]) * (len(got) - dl - n), (where, "deferred")


# ---- the same streams through the batch decoders ---------------------------------------------

@functools.lru_cache(maxsize=None)
def batch_streams():
    """Every valid family stream of at most 1 MiB of output and family F's error streams."""
    streams = [s for f in T.FAMILIES for s in T.family(f)]
    streams += [T.family_d(d, 65536)[0]._replace(out=T.family_d(d, 65536)[1]) for d in (7, 1, 32768)]
    return [s for s in streams if s.reason is not None or len(s.out) <= 1 << 20]


def test_batch_decoder(plain):
    from test_gpu_inflate_batch import oracle as batch_oracle, run_check
    streams = batch_streams()
    for s in streams:
        assert batch_oracle(s.comp)[:2] == (s.reason, s.out), s.name       # (run_check compares with this)
    res = run_check(plain, [s.comp for s in streams], "token streams")
    for s, (code, _, olen, _) in zip(streams, res):
        assert code == (0 if s.reason is None else COPY_BEFORE_CODE), s.name
        assert olen == len(s.out), s.name


def test_members_decoder_with_crc32(plain):
    import test_gpu_inflate_members as M
    streams = batch_streams()
    items = [(s.comp, M.RAW, M.CRC32) for s in streams]
    for s in streams:
        assert M.oracle(M.RAW, M.CRC32, s.comp)[:2] == (s.reason, s.out), s.name
    res = M.run_check(plain, items, "token streams")
    for s, r in zip(streams, res):
        assert r[0] == (0 if s.reason is None else COPY_BEFORE_CODE), s.name
        assert r[2] == len(s.out), s.name
        assert r[4] == (zlib.crc32(s.out) if s.reason is None else 0), s.name
