"""ndfl_deflate_batch_chunked on the GPU: many independent buffers compressed in one call by the chunk
encoders, one 1024-thread workgroup per chunk, each stream checked against the CPU oracle on that buffer
alone -- the DEFLATE bytes are O.deflate_lz(buffer, *params, chunk_len, hist_limit), end_bits is the bit at
which the oracle's decoder ends that stream, the checksums are Python's zlib.crc32 / zlib.adler32 -- and
every byte of `out` outside the streams' stored bytes must still hold the fill byte.

The buffers are the places where the segmented kernels can go wrong, not the workload's sizes.  Every
stream sits in a slot of whole chunks of the staged input, so what a chunk's index used to say comes from
a table: the length of a stream's last chunk (lengths around the multiples of chunk_len, empty streams),
where the stream starts (a neighbour's bytes lie right before a slot and must never be history: streams
that fill their slot exactly, followed by a stream that begins with their last bytes), which chunk
restarts the bit offsets (more than 64 one-chunk streams before a long one: the look-back's walk), and
the 8 KiB tiles of the parse-driven search, which know nothing of streams.
"""
import functools
import gzip
import random
import zlib

import pytest

import deflate_batch_harness as H
import knobs
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_UNSUPPORTED, FULL_DYNAMIC, FULL_STATIC, GZIP, NONE, RAW, ZLIB,
                                   chain_buffers, chunk_edge_buffers, ctx, layout_items, mixed, raws, salad,
                                   with_repeat)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

RLE_DYNAMIC, RLE_STATIC = (True, 3, 258, 1, 1), (False, 3, 258, 1, 1)
LITERAL_DYNAMIC, LITERAL_STATIC = (True, 0, 0, 0, 0), (False, 0, 0, 0, 0)
TUPLES = [FULL_DYNAMIC, FULL_STATIC, RLE_DYNAMIC, RLE_STATIC, LITERAL_DYNAMIC, LITERAL_STATIC, (True, 4, 100, 2, 5000)]
TILE = 8192                       # staged positions per workgroup of the parse-driven search (lz77_kernels.hip)

oracle = H.lz_oracle


def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_chunked; cfg: (params, chunk_len, hist_limit)."""
    params, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_chunked_raw(in_addr, in_size, out_addr, out_size, recs, *params, chunk_len, hist_limit, flags)


def c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg):
    import ndfl
    params, chunk_len, hist_limit = cfg
    return ndfl._lib.load().ndfl_deflate_batch_chunked(ctx._h, in_addr, in_size, out_addr, out_size, items, results, n,
                                                       *map(int, params), chunk_len, hist_limit, 0)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


# ---- 1. lengths against chunk lengths ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def length_items(c):
    """Streams of 0, 1, 2, c-1, c, c+1, 2c, 2c+1, 5c+7 bytes of mixed and of salad data, all three formats
    and both RAW sums, shuffled."""
    rng = random.Random(0xC0DE + c)
    items = []
    for k, n in enumerate([0, 1, 2, c - 1, c, c + 1, 2 * c, 2 * c + 1, 5 * c + 7] * 2):
        buf = mixed(rng, n) if k < 9 else salad(rng, n)
        items.append((buf, (RAW, ZLIB, GZIP, RAW)[k % 4], (NONE, CRC32, ADLER32, CRC32, ADLER32)[k % 5]))
    rng.shuffle(items)
    assert {fmt for _, fmt, _ in items} == {RAW, ZLIB, GZIP}
    assert {kind for _, fmt, kind in items if fmt == RAW} == {NONE, CRC32, ADLER32}
    return items


@pytest.mark.parametrize("hist_limit", [0, 1, 300, 32768])
@pytest.mark.parametrize("params", TUPLES)
@pytest.mark.parametrize("c", [64, 1000])
def test_lengths_around_the_chunk_length(ctx, c, params, hist_limit):
    res = run_check(ctx, length_items(c), (params, c, hist_limit), "lengths")
    assert all(r[0] == 0 for r in res)


@pytest.mark.parametrize("params", [FULL_DYNAMIC, RLE_DYNAMIC])
@pytest.mark.parametrize("c", [4096, 65536])
def test_lengths_around_the_larger_chunk_lengths(ctx, c, params):
    run_check(ctx, length_items(c), (params, c, 32768), "lengths")


# ---- 2. neighbour isolation -------------------------------------------------------------------------
@pytest.mark.parametrize("hist_limit", [32768, 0])
@pytest.mark.parametrize("params", [FULL_DYNAMIC, RLE_DYNAMIC, (False, 3, 258, 1, 400)])
@pytest.mark.parametrize("c", [1000, 4096])
def test_a_stream_never_sees_its_neighbour(ctx, c, params, hist_limit):
    """A fills its slot exactly (3c bytes), so B's slot starts at A's last byte + 1, and B begins with A's
    last 300 bytes (for the RLE form: with A's last byte, 50 times): B must not find them."""
    rng = random.Random(0xAB + c)
    A = salad(rng, 3 * c)
    lead = A[-1:] * 50 if params[3:] == (1, 1) else A[-300:]
    B = lead + salad(rng, c + 17)
    cfg = (params, c, hist_limit)
    # the construction bites: with A as history B would be shorter
    if params == FULL_DYNAMIC and hist_limit:
        assert len(oracle(A + B, *cfg)[0]) + 100 < len(oracle(A, *cfg)[0]) + len(oracle(B, *cfg)[0])
    items = [(A, RAW, CRC32), (B, ZLIB, NONE), (A, GZIP, NONE), (B, RAW, ADLER32)]
    run_check(ctx, items, cfg, "slots")
    # `in` packed back to back at odd offsets; B's region overlapping A's; one region used by two items
    if lead == A[-300:]:
        packed = b"\x00" + A + B[300:]
        offs = [1, 1 + len(A) - 300, 1, 1 + len(A) - 300]
        assert packed[offs[1]:offs[1] + len(B)] == B
    else:
        packed = b"\x00" + A + B
        offs = [1, 1 + len(A), 1, 1 + len(A)]
    assert all(o % 2 for o in offs)
    res, out, regions = run(ctx, items, cfg, inputs=(packed, offs))
    check(items, cfg, res, out, regions, "overlapping inputs")


# ---- 3. look-back past 64 predecessors and across stream starts ---------------------------------------
@pytest.mark.parametrize("params", [FULL_DYNAMIC, RLE_DYNAMIC])
def test_lookback_across_many_stream_starts(ctx, params):
    rng = random.Random(0x10CB)
    bufs = [mixed(rng, 1 + (7 * k) % 64) for k in range(130)]          # 130 one-chunk streams
    bufs.append(mixed(rng, 200 * 64 - 5))                               # 200 chunks
    bufs += [salad(rng, 64), b"", mixed(rng, 3 * 64 + 1)]
    items = [(b, (RAW, GZIP, ZLIB)[k % 3], (CRC32, ADLER32)[k % 2]) for k, b in enumerate(bufs)]
    run_check(ctx, items, (params, 64, 32768), "look-back")


# ---- 4. search-tile edges -----------------------------------------------------------------------------
def tile_edge_buffers(c):
    """Streams placed by their lengths so that, in slots of whole chunks, streams begin on a tile boundary
    and end on one, one byte before and one byte after; a repeat inside one stream across a tile edge; a
    stream that begins with the last bytes of the stream before it."""
    rng = random.Random(0x711E + c)
    bufs = [with_repeat(rng, 10000, 8100, 8150, 100)]                   # slot 0: the copy crosses staged byte 8192
    pos = -(-10000 // c) * c
    for d in (-1, 0, 1, 0, -1, 1):
        target = (pos // TILE + 1) * TILE
        if target % c == 0 and d == 0:
            target += TILE                                              # (not an empty stream)
        n = target - pos + d
        assert n >= 160
        b = bytearray(salad(rng, n))
        b[:80] = bufs[-1][-80:]                                         # its start repeats its neighbour's end
        b[n - 40:] = b[n // 2:n // 2 + 40]                              # a repeat at its own end
        bufs.append(bytes(b))
        pos += -(-n // c) * c
    return bufs


@pytest.mark.parametrize("params", [FULL_DYNAMIC, (True, 3, 258, 1, 9000)])
@pytest.mark.parametrize("c", [1000, 4096])
def test_search_tile_edges(ctx, c, params):
    bufs = tile_edge_buffers(c)
    if c == 4096:
        # streams that start on a tile boundary exist in this layout
        starts, pos = [], 0
        for b in bufs:
            starts.append(pos)
            pos += -(-len(b) // c) * c
        assert any(s and s % TILE == 0 for s in starts), starts
    run_check(ctx, raws(bufs), (params, c, 32768), "tile edges")
    run_check(ctx, raws(bufs[::-1]), (params, c, 300), "tile edges, reversed")


@pytest.mark.parametrize("c", [1000, 4096])
def test_chunk_edge_and_chain_buffers_as_one_batch(ctx, c):
    run_check(ctx, raws(chunk_edge_buffers() + chain_buffers()), (FULL_DYNAMIC, c, 32768), "edges + chains")


# ---- 5. several launch slabs --------------------------------------------------------------------------
def test_several_launch_slabs(ctx):
    import torch
    small = knobs.context(NDFL_SEG_SLAB=8192)
    small.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = random.Random(0x51AB)
    lens = [0, 9000, 1, 999, 1000, 1001, 7000, 8192, 3000, 9216, 2, 5000]           # begin, end and straddle slabs
    items = [((mixed if k % 2 else salad)(rng, n), (RAW, ZLIB, GZIP)[k % 3], (CRC32, NONE, ADLER32)[k % 3])
             for k, n in enumerate(lens)]
    for params in (FULL_DYNAMIC, (False, 3, 258, 1, 32768), RLE_DYNAMIC):
        cfg = (params, 1000, 32768)
        res_d, out_d, regions = run(ctx, items, cfg)
        check(items, cfg, res_d, out_d, regions, "default slab")
        res_s, out_s, _ = run(small, items, cfg)
        assert res_s == res_d and out_s == out_d, params


# ---- 6. the harness scenarios -------------------------------------------------------------------------
CFGS = [(FULL_DYNAMIC, 1000, 32768), (RLE_DYNAMIC, 1000, 32768)]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("shift", [0, 1])
def test_touching_regions_at_every_alignment(ctx, shift, cfg):
    seen = H.touching_regions(raw, oracle, ctx, layout_items(), cfg, range(18), shift)
    assert len(seen) == 16


@pytest.mark.parametrize("cfg", CFGS)
def test_device_pointers_on_the_callers_stream(ctx, cfg):
    H.device_pointers_on_the_callers_stream(raw, oracle, ctx, layout_items() + length_items(1000), cfg)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("fmt", [ZLIB, GZIP, RAW])
def test_capacity(ctx, fmt, cfg):
    rng = random.Random(9)
    left, mid, right = salad(rng, 777), mixed(rng, 4000), salad(rng, 1500)
    R = len(member(mid, fmt, cfg)[0])
    H.capacity_layout(raw, oracle, ctx, cfg, left, mid, right, fmt, [0, 1, R - 1, R, R + 1])


def test_arguments(ctx):
    ok = (FULL_DYNAMIC, 65536, 32768)

    def own_cases(one):
        cases = [(E_ARG, one, (FULL_DYNAMIC, 0, 32768)), (E_UNSUPPORTED, one, (FULL_DYNAMIC, 65537, 32768)),
                 (E_ARG, one, (FULL_DYNAMIC, 65536, 32769)), (E_ARG, one, (LITERAL_DYNAMIC, 0, 32768)),
                 (E_UNSUPPORTED, one, (RLE_STATIC, 65537, 32768)), (E_ARG, one, (RLE_DYNAMIC, 65536, 32769))]
        return cases + [(E_ARG, one, (bad, 65536, 32768)) for bad in H.BAD_TUPLES]

    a = H.argument_rules(raw, c_call, ctx, ok, own_cases)
    H.regions_that_only_touch(raw, oracle, ctx, ok, a)
    H.regions_that_only_touch(raw, oracle, ctx, (RLE_DYNAMIC, 65536, 32768), a)


# ---- 7. round trip and wrapper ------------------------------------------------------------------------
def test_members_round_trip(ctx):
    import ndfl
    rng = random.Random(13)
    bufs = [b"", b"x", salad(rng, 3000), mixed(rng, 70000), b"\xff" * 70000, rng.randbytes(2000)]
    for strategy in (ndfl.Lz77Huffman.FULL_DYNAMIC, "RLE_DYNAMIC"):
        for fmt, unpack in ((GZIP, gzip.decompress), (ZLIB, zlib.decompress)):
            members = ctx.deflate_members(bufs, fmt, strategy=strategy, path="chunks")
            for b, m in zip(bufs, members):
                assert unpack(m) == b
            back = ctx.inflate_members(members, fmt, out_caps=[len(b) for b in bufs])
            for b, m, (reason, out, bits, ck, hl) in zip(bufs, members, back):
                assert reason is None and out == b and bits == 8 * len(m)
                assert ck == H.checksum(b, fmt, NONE)
            assert members == ctx.deflate_members(bufs, fmt, strategy=strategy)


def test_wrapper_paths_agree_and_refuse(ctx):
    import ndfl
    rng = random.Random(14)
    bufs = [b"", salad(rng, 100), mixed(rng, 70000), salad(rng, 5000)]
    for strategy in (ndfl.Strategy.RLE_DYNAMIC, ndfl.Strategy.LITERAL_STATIC, ndfl.Lz77Huffman(True, 3, 258, 1, 32768)):
        for kind in (None, ndfl._lib.SUM_CRC32, ndfl._lib.SUM_ADLER32):
            assert ctx.deflate_batch(bufs, strategy, sum=kind, path="chunks") == ctx.deflate_batch(bufs, strategy, sum=kind)
    full = ndfl.Lz77Huffman.FULL_DYNAMIC
    for strategy in (ndfl.Uncompressed.SINGLETON, ndfl.MultiStrategy(full, ndfl.Lz77Huffman.RLE_DYNAMIC),
                     ndfl.BinarySplit(full, 1000), "UNCOMPRESSED"):
        with pytest.raises(ndfl.NdflError) as e:
            ctx.deflate_batch(bufs, strategy, path="chunks")
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(ValueError):
        ctx.deflate_batch(bufs, full, path="auto")


# ---- 8. one medium shape, the workload's grain ----------------------------------------------------------
@pytest.mark.parametrize("params", [FULL_DYNAMIC, RLE_DYNAMIC])
def test_medium_buffers(ctx, params):
    rng = random.Random(0x3ED)
    bufs = [mixed(rng, 200000) for _ in range(3)] + [b""] + [mixed(rng, 200000) for _ in range(3)] + [b"hello"]
    items = [(b, (GZIP, RAW, ZLIB)[k % 3], (CRC32, ADLER32)[k % 2]) for k, b in enumerate(bufs)]
    run_check(ctx, items, (params, 65536, 32768), "medium")
