"""GPU decode of the literal-run loop's limit cases (tests/emit_litrun.py: literal runs of K-1, K, K+1 and 2K+1 steps
ended by a dist-1 run, a deferred match, a long code, the end of block; a literal or pair at every offset 0..20 before
its lane's end; a run into the input's checked tail and a stream cut inside a run; a block of matches only; the
four-literal and escape-scan blocks; the decode errors after a run; what each case hits is pinned on the CPU by
tests/test_emit_litrun_cpu.py) against the oracle, byte for byte: output, Reason and consumed bits (the bits where
the Reason is not UNEXPECTED_END_OF_STREAM, as everywhere), through

    default      the fast emit kernel with the literal-run loop
    emit_full    NDFL_EMIT_FAST=0: the full emit kernel, the in-library reference
    batch        ctx.inflate_batch over every case in one call (it reports consumed bits with status 0 only)
    range        one case through inflate_range_raw from the tested block's header with its window

A decode whose emit pass disagrees with the count pass's records returns NDFL_E_INTERNAL, which ctx.inflate raises;
with one record perturbed (NDFL_TEST_SEGFLIP) it must.
"""
import pytest

import emit_litrun as E
import inflate_geometry as G
import knobs
import oracle_lib as O
import token_stream as TS

pytestmark = pytest.mark.gpu

WAYS = {"default": {}, "emit_full": {"NDFL_EMIT_FAST": 0}}


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


_ORACLE = {}


def oracle(c):
    """The oracle's decode of the case, computed once."""
    if c.name not in _ORACLE:
        _ORACLE[c.name] = O.inflate(c.comp, out_cap=len(c.out) + 4096)
    return _ORACLE[c.name]


def check(c, got, what, bits_on_error=True):
    reason, out, bits = got
    reason = getattr(reason, "name", reason)
    oreason, oout, obits = oracle(c)
    assert reason == oreason == c.reason, (what, c.name, reason, oreason)
    assert len(out) == len(oout) and out == oout, (what, c.name, len(out), len(oout),
                                                   next((i for i, (x, y) in enumerate(zip(out, oout)) if x != y), None))
    if oreason != G.UEOS and (bits_on_error or oreason is None):
        assert bits == obits, (what, c.name, bits, obits)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("family", E.FAMILIES)
def test_decode_matches_the_oracle(context, family, way):
    ctx = context(way)
    for c in E.cases(family):
        check(c, ctx.inflate(c.comp, out_cap=len(c.out) + 4096), way)


def test_batch_of_every_case(context):
    cs = [c for f in E.FAMILIES for c in E.cases(f)]
    got = context("default").inflate_batch([c.comp for c in cs], out_caps=[len(c.out) + 4096 for c in cs])
    assert len(got) == len(cs) == sum(E.COUNTS.values())
    for c, g in zip(cs, got):
        check(c, g, "batch", bits_on_error=False)


def test_range_decode_from_the_tested_block(ndfl, context):
    import torch
    c = next(c for c in E.cases("N") if c.name == "N_dist1_pair")
    before = TS.expand([b.tokens for b in c.blocks[:c.k]])[1]
    window = before[-32768:]
    start = c.blocks[c.k].hdr
    oreason, want, obits = O.inflate_range(c.comp, start, None, window, out_cap=len(c.out) + 4096)
    assert oreason is None and before + want == c.out and obits == c.bits
    src = torch.frombuffer(bytearray(c.comp), dtype=torch.uint8).cuda()
    out = torch.zeros(len(window) + len(want) + 4096, dtype=torch.uint8, device="cuda")
    out[:len(window)] = torch.frombuffer(bytearray(window), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for way in WAYS:
        r, olen, bits = context(way).inflate_range_raw(src.data_ptr(), len(c.comp), start, None, out.data_ptr(),
                                                       len(window), len(want) + 4096, ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
        assert (r, olen, bits) == (0, len(want), obits), (way, r, olen, bits)
        assert out[len(window):len(window) + olen].cpu().numpy().tobytes() == want, way


@pytest.mark.parametrize("way", list(WAYS))
def test_count_record_check_still_fails_loudly(ndfl, context, way):
    from ndfl import _lib
    c = next(c for c in E.cases("N") if c.name == "N_lit15_single")
    with pytest.raises(_lib.NdflError) as ei:
        context(way, NDFL_TEST_SEGFLIP=1).inflate(c.comp, out_cap=len(c.out) + 4096)
    assert ei.value.code == _lib.E_INTERNAL
