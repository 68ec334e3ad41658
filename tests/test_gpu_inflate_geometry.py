"""GPU decode of the count pass's limit cases: the hand-placed streams of tests/inflate_geometry.py (a token k bits
before a round end, a 48-bit token on the last bit of a lane segment, a literal pair split at a checkpoint, a round
that is the end-of-block code alone, a round cut inside a token by a false header candidate, ...; what each case
hits is pinned on the CPU by tests/test_inflate_geometry_cpu.py) against token_stream.expand: Reason, bytes and
consumed bits (the bits only where the Reason is not UNEXPECTED_END_OF_STREAM, as everywhere), through

    w1, w4            NDFL_COUNT_W = 1 and 4: the widths the cases' geometry is built for
    w2, w8, default   the same streams, no position aimed at
    emit_full, no_bt  NDFL_EMIT_FAST=0, NDFL_NO_BT=1: the full emit kernel, its own tables
    flat_off, flat_on the escape-prefix blocks (family K, P_escape) in wave form and one lane per block
    batch             ctx.inflate_batch over every case in one call (the serial wave decoder, its own staging); it
                      reports consumed bits with status 0 only (ndfl.h), so there they are compared on success
    padded            family T's truncations as NDFL_IN_PADDED device input
    range             one case of R and of K through inflate_range_raw from the tested block's seam with its window

A decode whose emit pass disagrees with the count pass's records returns NDFL_E_INTERNAL, which ctx.inflate raises.
Under NDFL_STATS=1 the library's "count pass: ... rounds N" equals the host model's round count for families R and S
(and its "width W" line names the W asked for), and its "slow-verify lanes" equals the model's count for family C.
"""
import collections
import functools
import re

import pytest

import inflate_geometry as G
import knobs
import token_stream as TS

pytestmark = pytest.mark.gpu

WAYS = collections.OrderedDict([
    ("w1", {"NDFL_COUNT_W": 1}), ("w4", {"NDFL_COUNT_W": 4}), ("w2", {"NDFL_COUNT_W": 2}), ("w8", {"NDFL_COUNT_W": 8}),
    ("default", {}), ("emit_full", {"NDFL_EMIT_FAST": 0}), ("no_bt", {"NDFL_NO_BT": 1}),
    ("flat_off", {"NDFL_FLAT": 0}), ("flat_on", {"NDFL_FLAT": 1, "NDFL_FLAT_MIN": 0})])
MAIN_WAYS = [w for w in WAYS if not w.startswith("flat")]


@pytest.fixture(scope="module")
def ndfl():
    import torch  # noqa: F401 (before libndfl.so: the device tests share torch's stream)
    import ndfl as N
    return N


@pytest.fixture(scope="module")
def context(ndfl):
    made = {}

    def get(way, **more):
        key = (way,) + tuple(sorted(more.items()))
        if key not in made:
            made[key] = knobs.context(**dict(WAYS[way], **more))
        return made[key]
    return get


def check(c, got, what, bits_on_error=True):
    reason, out, bits = got
    reason = getattr(reason, "name", reason)
    assert reason == c.reason, (what, c.name, reason, c.reason)
    assert len(out) == len(c.out) and out == c.out, (what, c.name, len(out), len(c.out),
                                                     next((i for i, (x, y) in enumerate(zip(out, c.out)) if x != y), None))
    if c.reason != G.UEOS and (bits_on_error or c.reason is None):
        want = c.bits if c.bits is not None else G.O.inflate(c.comp, out_cap=len(c.out) + 1024)[2]
        assert bits == want, (what, c.name, bits, want)


def decode(ctx, c):
    return ctx.inflate(c.comp, out_cap=len(c.out) + 4096)


@pytest.mark.parametrize("way", MAIN_WAYS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_decode_matches_expand(context, family, way):
    ctx = context(way)
    for c in G.cases(family):
        check(c, decode(ctx, c), way)


def escape_cases():
    return G.cases("K")[:4] + [c for c in G.cases("P") if c.name.startswith(("P_escape", "P_short_round"))]


@pytest.mark.parametrize("way", ["flat_off", "flat_on"])
def test_escape_prefix_blocks_both_ways(context, way):
    ctx = context(way)
    for c in escape_cases():
        check(c, decode(ctx, c), way)


def test_batch_of_every_case(context):
    cs = [c for f in G.FAMILIES for c in G.cases(f)]
    got = context("default").inflate_batch([c.comp for c in cs], out_caps=[len(c.out) + 4096 for c in cs])
    assert len(got) == len(cs) == sum(G.COUNTS.values())
    for c, g in zip(cs, got):
        check(c, g, "batch", bits_on_error=False)       # (ndfl_inflate_batch reports consumed bits with status 0 only)


def test_truncations_as_padded_device_input(ndfl, context):
    import torch
    ctx = context("w1")
    D = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | ndfl.IN_PADDED
    n = 0
    for c in G.cases("T"):
        if "cut" not in c.info:
            continue
        n += 1
        buf = torch.zeros(len(c.comp) + ndfl.IN_PAD_BYTES, dtype=torch.uint8, device="cuda")
        buf[:len(c.comp)] = torch.frombuffer(bytearray(c.comp), dtype=torch.uint8).cuda()
        out = torch.zeros(len(c.out) + 4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r, olen, bits = ctx.inflate_raw(buf.data_ptr(), len(c.comp), out.data_ptr(), out.numel(), D)
        assert r >= 0, (c.name, r)
        check(c, (None if r == 0 else ndfl.Reason(r - 1), out[:olen].cpu().numpy().tobytes(), bits), "padded")
    assert n == 11


@pytest.mark.parametrize("name", ["R_token_W1_slow_w48_k47", "K_in_token"])
def test_range_decode_from_the_tested_seam(ndfl, context, name):
    import torch
    c = next(c for c in G.cases(name[0]) if c.name.startswith(name))
    before = TS.expand([b.tokens for b in c.blocks[:c.k]])[1]
    window = before[-32768:]
    reason, want = TS.expand([b.tokens for b in c.blocks[c.k:]], window)
    assert reason is None and before + want == c.out
    src = torch.frombuffer(bytearray(c.comp), dtype=torch.uint8).cuda()
    out = torch.zeros(len(window) + len(want) + 4096, dtype=torch.uint8, device="cuda")
    out[:len(window)] = torch.frombuffer(bytearray(window), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for way in ("w1", "w4"):
        r, olen, bits = context(way).inflate_range_raw(src.data_ptr(), len(c.comp), c.blocks[c.k].hdr, None, out.data_ptr(),
                                                       len(window), len(want) + 4096, ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
        assert (r, olen, bits) == (0, len(want), c.bits), (way, r, olen, bits)
        assert out[len(window):len(window) + olen].cpu().numpy().tobytes() == want, way


# ---- the count pass's own statistics against the model -----------------------------------------------------------
def count_stats(ctx, c, capfd):
    """(slow-verify lanes, rounds, width) the library prints for one decode under NDFL_STATS=1."""
    capfd.readouterr()
    got = decode(ctx, c)
    err = capfd.readouterr().err
    m = re.findall(r"count pass: slow-verify lanes (\d+) fixups \d+ rounds (\d+)", err)
    w = re.findall(r"count pass: \d+ candidates, \d+ counted, width (\d+)", err)
    assert len(m) == 1 and len(w) == 1, err
    return got, int(m[0][0]), int(m[0][1]), int(w[0])


@functools.lru_cache(maxsize=None)
def model_rounds(family, i, W):
    return G.stat_rounds(G.cases(family)[i], W)


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("family", ["R", "S"])
def test_round_counts_are_the_models(context, capfd, family, W):
    ctx = context(f"w{W}", NDFL_STATS=1)
    wrong = []
    for i, c in enumerate(G.cases(family)):
        if c.W != W:
            continue
        got, _, rounds, width = count_stats(ctx, c, capfd)
        check(c, got, "stats")
        assert width == W, (c.name, width)
        if rounds != model_rounds(family, i, W):
            wrong.append((c.name, rounds, model_rounds(family, i, W)))
    assert not wrong, wrong


def test_slow_verify_lanes_are_the_models(context, capfd):
    """Family C at W = 1 (its geometry is a one-wave round's).  The count is exact: every lane whose first verify
    -- from its predecessor's speculative exit -- meets none of its three checkpoints, up to the first lane whose
    speculation ended the block.  So C_nslow_8 stays at 8 (sweeps alone), C_nslow_9 passes NDFL_PH_FALLBACK, and
    C_nslow_49_then_9 counts 49 and not 58: its second round is phase-mapped, C_nslow_48_then_9's is not (57)."""
    ctx = context("w1", NDFL_STATS=1)
    wrong, seen = [], {}
    for c in G.cases("C"):
        got, nslow, _, width = count_stats(ctx, c, capfd)
        check(c, got, "stats")
        assert width == 1
        seen[c.name] = nslow
        if nslow != G.stat_nslow(c, 1):
            wrong.append((c.name, nslow, G.stat_nslow(c, 1)))
    assert not wrong, wrong
    assert [seen[n] for n in ("C_nslow_1", "C_nslow_8", "C_nslow_9", "C_nslow_49_then_9", "C_nslow_48_then_9")] == \
        [1, 8, 9, 49, 57], seen
