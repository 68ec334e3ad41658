"""GPU parity of the per-block code construction at its limits: the inputs of tests/adversarial_hist.py
(15-bit literal/length and distance codes that need the limit, 7-bit code-length codes that need it,
long package/leaf tie chains, the single-distance-code fix-ups, HLIT = 286, HDIST = 30, code-length
runs around every length at which the run decomposition changes) through each encoder that builds
codes, byte for byte against the CPU oracle.  There is one builder (huffman_build.hpp), instantiated
at 64 and at 1024 threads:

    split   the default pipeline's codes kernel: build_block_codes at 64 threads (deflate_split.hip)
    fused   NDFL_DEFLATE_FUSED=1: build_block_codes at 1024 threads (deflate_kernels.hip)
    lz      build_block_codes at 1024 threads inside the LZ77 kernel (lz77_kernels.hip)

and the decoder on the oracle's streams of the same inputs.  The engagement condition of every case
is asserted on the oracle's stream by the CPU suite (test_oracle_deflate.test_adversarial_cases);
here it is evaluated again only where a path encodes a case another way (FULL_DYNAMIC on the
literal-limit chunks).  On a mismatch the message names the first differing block and header field.
"""
import functools
import io

import pytest

import adversarial_hist as A
import knobs
import oracle_lib as O

pytestmark = pytest.mark.gpu

NO_MATCH = (True, 258, 258, 1, 32768)     # the LZ77 kernel, but no 258-byte repeat exists: literals only
PRESET = {"LITERAL_DYNAMIC": (True, 0, 0, 0, 0), "RLE_DYNAMIC": (True, 3, 258, 1, 1)}


@pytest.fixture(scope="module")
def ndfl():
    import ndfl as N
    return N


@pytest.fixture(scope="module")
def ctx(ndfl):
    return ndfl.Context(0)


@pytest.fixture(scope="module")
def fused():
    return knobs.context(NDFL_DEFLATE_FUSED=1)


@pytest.fixture(scope="module")
def full_only():
    return knobs.context(NDFL_EMIT_FAST=0)


def ways(case):
    """How a case is encoded: preset names, or one Lz77Huffman parameter tuple."""
    mode, arg, _, _ = case.encode_args
    return list(arg) if mode == "preset" else [arg]


@functools.lru_cache(maxsize=None)
def expected(cls, i, way):
    """The oracle's stream of case i of cls encoded `way` (computed once, shared by the tests)."""
    case = A.cases(cls)[i]
    _, _, chunk_len, hist = case.encode_args
    if isinstance(way, str):
        return O.deflate(case.data, way, chunk_len, hist)
    return O.deflate_lz(case.data, *way, chunk_len, hist)


def gpu_encode(ndfl, c, case, way):
    _, _, chunk_len, hist = case.encode_args
    strat = way if isinstance(way, str) else ndfl.Lz77Huffman(*way)
    return c.deflate(case.data, strat, chunk_len=chunk_len, hist_limit=hist)


def check(got, exp, *where):
    assert got == exp, (where, A.explain(exp, got))


@pytest.mark.parametrize("cls", A.CLASSES)
def test_split_and_fused_match_oracle(ndfl, ctx, fused, cls):
    """Every case, encoded the way its generator names, on the default context and on the fused one.
    Presets (and the Lz77Huffman parameters equal to one) take the split codes kernel / the fused
    kernel; other parameters take the LZ77 kernel on both contexts."""
    for i, case in enumerate(A.cases(cls)):
        for way in ways(case):
            exp = expected(cls, i, way)
            check(gpu_encode(ndfl, ctx, case, way), exp, "default", cls, case.name, way)
            check(gpu_encode(ndfl, fused, case, way), exp, "fused", cls, case.name, way)


def test_lz_kernel_on_literal_and_code_length_limits(ndfl, ctx):
    """build_block_codes inside the LZ77 kernel with the literal alphabet at its limit: the
    lit_limit and cl_limit chunks with parameters that can match nothing (the literal histogram is
    LITERAL_DYNAMIC's, so every condition holds as on the CPU), and FULL_DYNAMIC on the cases whose
    condition still holds on the oracle's FULL_DYNAMIC stream (skewed shuffles repeat 3-byte strings,
    so the Fibonacci and power-of-two chunks drop out there; the tie and equal-frequency ones stay)."""
    kept_full = []
    for cls in ["lit_limit", "cl_limit"]:
        for i, case in enumerate(A.cases(cls)):
            exp = O.deflate_lz(case.data, *NO_MATCH)
            assert exp == expected(cls, i, "LITERAL_DYNAMIC"), (cls, case.name)
            check(ctx.deflate(case.data, ndfl.Lz77Huffman(*NO_MATCH)), exp, "lz no-match", cls, case.name)
            exp = O.deflate(case.data, "FULL_DYNAMIC")
            if A.engaged(case.kind, A.walk_blocks(exp)):
                kept_full.append(case.name)
                check(ctx.deflate(case.data, "FULL_DYNAMIC"), exp, "FULL_DYNAMIC", cls, case.name)
    assert any(n.startswith("ties") for n in kept_full), kept_full


def test_strategy_choice_rests_on_block_bits(ndfl, ctx):
    """MultiStrategy picks by the computed block size: per chunk and over the concatenated lit_limit +
    cl_limit chunks the choice equals the oracle's, and the bit lengths the plugin API reports for
    each chunk equal the oracle's block sizes."""
    L, U = ndfl.Lz77Huffman, ndfl.Uncompressed.SINGLETON
    sets = [(ndfl.MultiStrategy(L.RLE_DYNAMIC, U), [PRESET["RLE_DYNAMIC"], "UNCOMPRESSED"]),
            (ndfl.MultiStrategy(L.LITERAL_DYNAMIC, L.RLE_DYNAMIC), [PRESET["LITERAL_DYNAMIC"], PRESET["RLE_DYNAMIC"]])]
    chunks = [c for cls in ["lit_limit", "cl_limit"] for c in A.cases(cls)]
    joined = b"".join(c.data for c in chunks)
    for strat, subs in sets:
        for c in chunks:
            check(ctx.deflate(c.data, strat), O.deflate_multi(c.data, subs), "multi", c.name, subs)
        for chunk_len, hist in [(65536, 32768), (32768, 0)]:
            check(ctx.deflate(joined, strat, chunk_len=chunk_len, hist_limit=hist),
                  O.deflate_multi(joined, subs, chunk_len, hist), "multi joined", chunk_len, subs)
    for c in chunks:
        for name in ["RLE_DYNAMIC", "LITERAL_DYNAMIC"]:
            bits = getattr(L, name).decide(c.data, 0, 0, len(c.data)).getBitLengths()
            assert bits == [O.block_bits(c.data, name)[0]] * 8, (c.name, name)


@pytest.mark.parametrize("cls", A.CLASSES)
def test_decoder_on_edge_streams(ctx, full_only, cls):
    """The decoder on the oracle's streams of every case (complete 15-bit literal and distance codes,
    7-bit code-length codes, HLIT 286 / HDIST 30, 101 headers at arbitrary bit offsets): the
    oracle's (reason, output, consumed bits), with the fast emit pass and without it."""
    for i, case in enumerate(A.cases(cls)):
        for way in ways(case):
            comp = expected(cls, i, way)
            want = O.inflate(comp)
            assert want[0] is None and want[1] == case.data
            for name, c in [("default", ctx), ("NDFL_EMIT_FAST=0", full_only)]:
                reason, out, bits = c.inflate(comp)
                assert (reason, bits) == (None, want[2]) and out == case.data, (name, cls, case.name, way)


def test_sweep_stitched_at_odd_bit_positions(ndfl, ctx, fused):
    """The 512-byte chunk sweep through DeflaterOutputStream one chunk per GPU call: every block's
    header starts at the bit position the previous call ended on."""
    case = A.cases("cl_runs")[0]
    assert case.name == "sweep512"
    for c in [ctx, fused]:
        for way in ways(case):
            bout = io.BytesIO()
            d = ndfl.DeflaterOutputStream(bout, 512, 0, getattr(ndfl.Lz77Huffman, way), context=c, batch_bytes=1)
            for off in range(0, len(case.data), 512):
                d.write(case.data, off, 512)
            d.finish()
            check(bout.getvalue(), expected("cl_runs", 0, way), "stream", way)
