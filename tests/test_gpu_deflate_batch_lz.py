"""ndfl_deflate_batch_lz77 on the GPU: many independent buffers compressed in one call with an LZ77
search, each stream checked against the CPU oracle on that buffer alone -- the DEFLATE bytes are
O.deflate_lz(buffer, *params, chunk_len, hist_limit), end_bits is the bit at which the oracle's decoder
ends that stream, the checksums are Python's zlib.crc32 / zlib.adler32 -- and every byte of `out` outside
the streams' stored bytes must still hold the fill byte.

The buffers are the places where the batch kernel (csrc/hip/deflate_batch_lz.hip) can go wrong, not the
workload's sizes: a wave walks a chunk in steps of 64 positions, one lane per position, links every
position into hash chains that run on across chunk ends (a 4,096-bucket head table, a ring of links),
searches the 64 positions at once, and carries the greedy parse from step to step.  So repeats start, end
and have their sources around the step edges, at the run lengths and distances where the search's caps
and window bounds bite, in chains that are long, shared by colliding prefixes, or left behind by the
stream the wave encoded before.
"""
import functools
import gzip
import random
import zlib

import pytest

import deflate_batch_harness as H
import test_gpu_lz77 as LZ
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_UNSUPPORTED, FILL, FULL_DYNAMIC, FULL_STATIC, GZIP, NONE, RAW,
                                   ZLIB, chain_buffers, checksum, chunk_edge_buffers, ctx, edge_buffers, layout_items, mixed,
                                   one_wave, raws, reuse_items, salad, trailer)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

DEFAULT = (FULL_DYNAMIC, 65536, 32768)
STEP = 64                         # positions per step (deflate_batch_lz.hip)

oracle, raw = H.lz_oracle, H.lz_raw


def c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg):
    import ndfl
    params, chunk_len, hist_limit = cfg
    return ndfl._lib.load().ndfl_deflate_batch_lz77(ctx._h, in_addr, in_size, out_addr, out_size, items, results, n,
                                                    *map(int, params), chunk_len, hist_limit, 0)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


@pytest.mark.parametrize("params", [FULL_DYNAMIC, FULL_STATIC])
def test_step_and_lane_edges(ctx, params):
    bufs = edge_buffers()
    assert len(bufs) > 300
    res = run_check(ctx, raws(bufs), (params, 65536, 32768), "edges")
    assert all(r[0] == 0 for r in res)


@pytest.mark.parametrize("hist_limit", [0, 1, 100, 32768])
@pytest.mark.parametrize("chunk_len", [1, 7, 259, 1000, 65536])
def test_runs_cut_by_the_chunk_end(ctx, chunk_len, hist_limit):
    """A run ends at the chunk's end; the next chunk finds the rest with history and nothing without."""
    bufs = chunk_edge_buffers()
    run_check(ctx, raws(bufs), (FULL_DYNAMIC, chunk_len, hist_limit), "chunk end")
    if chunk_len == 1000:
        # the construction does what it says: history makes the later chunks smaller
        b = bufs[-4]
        assert len(oracle(b, FULL_DYNAMIC, 1000, 32768)[0]) + 200 < len(oracle(b, FULL_DYNAMIC, 1000, 0)[0])


def at_distance(d, lead=0):
    """A 60-byte pattern at `lead`, random bytes (the same ones for every d), and the pattern again d bytes
    after its first copy."""
    b = bytearray(random.Random(0xD157).randbytes(lead + d + 60 + 40))
    b[lead + d:lead + d + 60] = b[lead:lead + 60]
    return bytes(b)


def test_distances(ctx):
    ds = (1, 2, 63, 64, 65, 32767, 32768, 32769)
    bufs = [at_distance(d) for d in ds]
    # the same across a chunk end, more than one lap of the link ring into the stream
    bufs += [at_distance(d, lead=65536 + 100 - d) for d in (32767, 32768, 32769)]
    bufs += [at_distance(d, lead=40000) for d in (32768, 32769)]
    run_check(ctx, raws(bufs), DEFAULT, "distances")
    run_check(ctx, raws(bufs[:8]), ((True, 3, 258, 64, 32767), 65536, 32768), "distances 64..32767")
    # 32,768 matches and 32,769 does not: the pattern costs its literals again
    size = {d: len(oracle(b)[0]) - len(b) for d, b in zip(ds, bufs)}
    assert size[32769] > size[32768] + 40 and abs(size[32768] - size[32767]) < 8, size


def test_ties(ctx):
    rng = random.Random(0x71E5)
    P, Q = b"PATTERN8", b"PATTERN8andmore!"
    fill = lambda n: rng.randbytes(n)                           # noqa: E731
    bufs = [
        P + fill(50) + P + fill(70) + P,                           # one run length at two distances
        P + fill(50) + P + fill(70) + P + fill(30) + P,            # at three
        Q + fill(40) + P + fill(40) + Q,                           # the longer run is the farther one
        Q + fill(40) + P + fill(40) + P + fill(40) + Q + fill(40) + P,
        P + fill(56) + P + fill(56) + P,                           # sources one step apart
        b"abcd" + fill(3) + b"abce" + fill(3) + b"abcd" + fill(3) + b"abc",
    ]
    run_check(ctx, raws(bufs), DEFAULT, "ties")
    run_check(ctx, raws(bufs), (FULL_STATIC, 65536, 32768), "ties")


def test_duplicates_and_long_chains(ctx):
    bufs = chain_buffers()
    run_check(ctx, raws(bufs), DEFAULT, "chains")
    run_check(ctx, raws([b for b in bufs if len(b) < 10000]), (FULL_STATIC, 1000, 100), "chains")


PARAMETER_TUPLES = LZ.test_lz77_parameters_match_oracle.pytestmark[0].args[1]


@pytest.mark.parametrize("params", PARAMETER_TUPLES)
def test_parameters(ctx, params):
    """The thirteen tuples of test_gpu_lz77.py, all buffers of one tuple in one batch call."""
    assert len(PARAMETER_TUPLES) == 13 and (True, 0, 0, 0, 0) in PARAMETER_TUPLES
    run_check(ctx, raws(LZ.inputs(12)[::2]), (tuple(params), 65536, 32768), "parameters")


@pytest.mark.parametrize("params", [FULL_DYNAMIC, FULL_STATIC])
def test_full_presets(ctx, params):
    """Up to 200,003 bytes with repeats at distances up to 40,000: more than one lap of the link ring,
    across chunk ends."""
    bufs = LZ.inputs(11)
    assert {131072, 200003} <= {len(b) for b in bufs}
    run_check(ctx, raws(bufs), (params, 65536, 32768), "full presets")


def test_neighbours_in_the_input(ctx):
    """Buffers packed back to back, where the bytes just before in_off would supply a match and the bytes
    just after in_off + in_len would lengthen one; input regions that overlap and repeat."""
    rng = random.Random(0x9E16)
    X, Y, Z = rng.randbytes(300), rng.randbytes(200), rng.randbytes(100)
    packed = X + Y + Y + Z + X[:50] + Y
    n = len(packed)
    spans = [(0, 500),            # X + Y
             (500, 300),          # Y + Z: what precedes it is its own first 200 bytes
             (0, 510),            # X + Y + Y[:10]: the run at its end goes on in the bytes after it
             (500, 210),          # ends inside a run whose source is its own start... and goes on after it
             (300, 400), (300, 400),                       # the same region twice
             (200, n - 200), (0, n), (n - 200, 200), (n - 3, 3), (n, 0), (0, 0), (499, 2)]
    items = [(packed[o:o + l], (RAW, ZLIB, GZIP)[k % 3], (CRC32, NONE, ADLER32)[k % 3]) for k, (o, l) in enumerate(spans)]
    for cfg in (DEFAULT, (FULL_DYNAMIC, 128, 32768), (FULL_STATIC, 100, 64)):
        res, out, regions = run(ctx, items, cfg, inputs=(packed, [o for o, _ in spans]))
        check(items, cfg, res, out, regions, "neighbours")


def test_wave_reuse_one_wave(one_wave):
    items = reuse_items()
    assert len(items) == 300
    for cfg in (DEFAULT, (FULL_DYNAMIC, 259, 32768)):
        run_check(one_wave, items, cfg, "one wave")


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_capacity(ctx, fmt):
    """A stream that needs R bytes in a region of 0, 1, R - 1 and R, between neighbours whose regions touch
    it: status, out_len == R, the stored prefix, and the neighbours bit-exact."""
    rng = random.Random(9)
    left, mid, right = salad(rng, 777), mixed(rng, 4000), salad(rng, 1500)
    R = len(member(mid, fmt, DEFAULT)[0])
    H.capacity_layout(raw, oracle, ctx, DEFAULT, left, mid, right, fmt, [0, 1, R - 1, R])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_touching_regions_at_every_alignment(ctx, shift):
    """All three formats and both sums for RAW, regions that touch, `out` shifted by 0..3 bytes and the
    first region by 0..3 more."""
    H.touching_regions(raw, oracle, ctx, layout_items(), DEFAULT, range(4), shift)


def test_device_pointers_on_the_callers_stream(ctx):
    H.device_pointers_on_the_callers_stream(raw, oracle, ctx, reuse_items()[:60] + layout_items(), DEFAULT)


def test_arguments(ctx):
    import ndfl
    ok = (FULL_DYNAMIC, 65536, 32768)

    def own_cases(one):
        cases = [(E_ARG, one, (FULL_DYNAMIC, 0, 32768)), (E_UNSUPPORTED, one, (FULL_DYNAMIC, 65537, 32768)),
                 (E_ARG, one, (FULL_DYNAMIC, 65536, 32769)), (E_ARG, one, ((True, 0, 0, 0, 0), 0, 32768)),
                 (E_UNSUPPORTED, one, ((False, 3, 258, 1, 1), 65537, 32768))]
        return cases + [(E_ARG, one, (bad, 65536, 32768)) for bad in H.BAD_TUPLES]

    a = H.argument_rules(raw, c_call, ctx, ok, own_cases)
    # ndfl_deflate_batch itself still refuses the FULL_* presets
    with pytest.raises(ndfl.NdflError) as e:
        ctx.deflate_batch_raw(a.a_in, len(a.s), a.a_out, 256, a.one, "FULL_DYNAMIC", 65536, 32768, 0)
    assert e.value.code == E_UNSUPPORTED and a.out.raw == bytes([FILL]) * 256
    H.regions_that_only_touch(raw, oracle, ctx, ok, a)


def test_equals_the_one_stream_encoder(ctx):
    """GPU against GPU: the batch's bytes for a 200,000-byte buffer are ctx.deflate's."""
    import ndfl
    buf = mixed(random.Random(31), 200000)
    for chunk_len, hist_limit in ((65536, 32768), (10000, 0)):
        comp, bits, _ = ctx.deflate_batch([buf], ndfl.Lz77Huffman.FULL_DYNAMIC, chunk_len, hist_limit)[0]
        assert comp == ctx.deflate(buf, "FULL_DYNAMIC", chunk_len, hist_limit)
        assert (bits + 7) // 8 == len(comp)


def test_members_round_trip(ctx):
    """Context.deflate_members with FULL_DYNAMIC gives complete members: ctx.inflate_members reads them back
    with the same checksum, and so do Python's gzip and zlib."""
    import ndfl
    rng = random.Random(13)
    bufs = [b"", b"x", salad(rng, 3000), mixed(rng, 70000), b"\xff" * 70000, rng.randbytes(2000)]
    for fmt, unpack in ((GZIP, gzip.decompress), (ZLIB, zlib.decompress)):
        members = ctx.deflate_members(bufs, fmt, strategy=ndfl.Lz77Huffman.FULL_DYNAMIC)
        header = bytes((ndfl.ZlibMetadata.DEFAULT if fmt == ZLIB else ndfl.GzipMetadata()).header_bytes())
        for b, m in zip(bufs, members):
            assert m == header + oracle(b)[0] + trailer(b, fmt)
            assert unpack(m) == b
        back = ctx.inflate_members(members, fmt, out_caps=[len(b) for b in bufs])
        for b, m, (reason, out, bits, ck, hl) in zip(bufs, members, back):
            assert reason is None and out == b and bits == 8 * len(m) and hl == len(header)
            assert ck == checksum(b, fmt, NONE)
    # the preset names keep ndfl_deflate_batch
    assert ctx.deflate_members([bufs[2]], GZIP, strategy="RLE_DYNAMIC") == ctx.deflate_members([bufs[2]], GZIP)
