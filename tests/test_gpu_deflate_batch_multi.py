"""ndfl_deflate_batch_multi on the GPU: many independent buffers compressed in one call under
MultiStrategy(subs...), every chunk as the block of the substrategy with the fewest bits.  Each stream is
checked byte for byte against the CPU oracle on that buffer alone -- the DEFLATE bytes are
O.deflate_multi(buffer, subs, chunk_len, hist_limit), end_bits is the bit at which the oracle's decoder
ends that stream, the checksums are Python's zlib.crc32 / zlib.adler32 -- and every byte of `out` outside
the streams' stored bytes must still hold the fill byte.

The buffers are those of test_gpu_deflate_batch_lz.py (the search's step, chunk and chain edges) and the
places where the choice itself can go wrong (csrc/hip/deflate_batch_multi.hip): a stored block after a
Huffman block that ends at each bit position, ties, a best candidate that a later one beats or does not,
stored blocks at the 65,535-byte limit and at the ends of an output region, and the state a wave could
carry from one stream into the next.

U = Uncompressed, FS = FULL_STATIC, FD = FULL_DYNAMIC, T3 = (U, FS, FD).
"""
import functools
import gzip
import itertools
import random
import zlib

import pytest

import adversarial_hist as AH
import deflate_batch_harness as H
import oracle_lib as O
import test_gpu_lz77 as LZ
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_UNSUPPORTED, FILL, GZIP, NONE, RAW, ZLIB, checksum, ctx, mixed,
                                   one_wave, raws, salad, trailer)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

U = "UNCOMPRESSED"
FS, FD = H.FULL_STATIC, H.FULL_DYNAMIC
RLE_DYNAMIC = (True, 3, 258, 1, 1)
LITERAL_STATIC, LITERAL_DYNAMIC = (False, 0, 0, 0, 0), (True, 0, 0, 0, 0)
T3 = (U, FS, FD)
DEFAULT = (T3, 65536, 32768)


@functools.lru_cache(maxsize=None)
def oracle(buf, subs=T3, chunk_len=65536, hist_limit=32768):
    """(DEFLATE bytes, end bits) of one buffer alone, computed once; the oracle's decoder gives the bits."""
    comp = O.deflate_multi(buf, subs, chunk_len, hist_limit)
    reason, back, bits = O.inflate(comp, out_cap=len(buf) + 64)
    assert reason is None and back == buf and (bits + 7) // 8 == len(comp)
    return comp, bits


def descs(subs):
    """StrategyDesc records of U / Lz77Huffman tuples (ready-made records pass through)."""
    import ndfl
    D = ndfl._lib.StrategyDesc
    return [s if isinstance(s, D) else D(1, 0, 0, 0, 0, 0) if s == U else D(0, *map(int, s)) for s in subs]


def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_multi; cfg: (subs, chunk_len, hist_limit)."""
    subs, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_multi_raw(in_addr, in_size, out_addr, out_size, recs, descs(subs), chunk_len, hist_limit,
                                       flags)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


def c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg):
    import ndfl
    subs = descs(cfg[0])
    arr = (ndfl._lib.StrategyDesc * max(1, len(subs)))(*subs)
    return ndfl._lib.load().ndfl_deflate_batch_multi(ctx._h, in_addr, in_size, out_addr, out_size, items, results, n, arr,
                                                     len(subs), cfg[1], cfg[2], 0)


def btypes(comp):
    return [b["btype"] for b in AH.walk_blocks(comp)]


def type_buffers():
    rng = random.Random(0x7E58)
    return [b"", rng.randbytes(1), rng.randbytes(64), salad(rng, 512), salad(rng, 4096), mixed(rng, 3000)]


def test_each_block_type_wins_in_one_batch(ctx):
    bufs = type_buffers()
    seen = [btypes(oracle(b)[0]) for b in bufs]
    assert seen[2] == [0] and seen[3] == [1] and seen[4] == [2], seen
    assert {0, 1, 2} <= {t for s in seen for t in s}
    res = run_check(ctx, raws(bufs), DEFAULT, "block types")
    assert all(r[0] == 0 for r in res)


def position_buffer(k, n):
    return random.Random(0x9051 + k).randbytes(n) * 40


@functools.lru_cache(maxsize=None)
def position_buffers():
    """One random chunk of n bytes 40 times over, chunk_len = n and no history: every chunk has the same
    fixed-code size and only its bit position differs.  ((n, buffer), ...) for those where the oracle has
    stored and fixed blocks in one stream, or differs between (U, FS) and (FS, U)."""
    picked, mixed_types, order = [], 0, 0
    for k in range(12):
        for n in range(50, 57):
            buf = position_buffer(k, n)
            a, b = oracle(buf, (U, FS), n, 0)[0], oracle(buf, (FS, U), n, 0)[0]
            both = {0, 1} <= set(btypes(a))
            if both or a != b:
                picked.append((n, buf))
                mixed_types += both
                order += a != b
    return tuple(picked), mixed_types, order


def test_choice_depends_on_the_bit_position_and_ties_keep_the_first(ctx):
    picked, mixed_types, order = position_buffers()
    assert mixed_types >= 1 and order >= 1, (mixed_types, order)
    # a case worked out on the CPU beforehand: seed 0x9051 + 4, n = 50 has 5 stored blocks of 40 and depends on the order
    buf = position_buffer(4, 50)
    assert (50, buf) in picked and btypes(oracle(buf, (U, FS), 50, 0)[0]).count(0) == 5
    assert oracle(buf, (U, FS), 50, 0) != oracle(buf, (FS, U), 50, 0)
    # stored blocks after Huffman blocks that end at more than one bit position (a stored block's padding is
    # shortest, so it wins most easily, at bit 5, then at bit 4)
    ends = set()
    for n, buf in picked:
        for subs in ((U, FS), (FS, U)):
            blocks = AH.walk_blocks(oracle(buf, subs, n, 0)[0])
            ends |= {p["end_bit"] & 7 for p, q in zip(blocks, blocks[1:]) if p["btype"] == 1 and q["btype"] == 0}
    assert len(ends) >= 2, ends
    for n in range(50, 57):
        bufs = [b for m, b in picked if m == n]
        if bufs:
            for subs in ((U, FS), (FS, U)):
                run_check(ctx, raws(bufs), (subs, n, 0), "bit position")


def stored_oracle(buf, subs, chunk_len, hist_limit):
    comp, bits = oracle(buf, subs, chunk_len, hist_limit)
    assert subs == (U,) and comp == O.deflate(buf, "UNCOMPRESSED", chunk_len)
    return comp, bits


def test_stored_edges(ctx):
    rng = random.Random(0x5702ED)
    big = rng.randbytes(131072)
    bufs = [big[:n] for n in (0, 1, 2, 65534, 65535, 65536, 65537, 131071, 131072)]
    for chunk_len in (65536, 65535):
        H.run_check(raw, stored_oracle, ctx, raws(bufs), ((U,), chunk_len, 32768), "stored")
    small = [big[1000:1000 + n] for n in range(301)]
    for chunk_len in (1, 7):
        H.run_check(raw, stored_oracle, ctx, raws(small), ((U,), chunk_len, 0), "stored, small chunks")
    # a 65,536-byte chunk is a 65,535-byte block and a 1-byte block; BFINAL on the last block only
    blocks = AH.walk_blocks(oracle(big[:65536], (U,), 65536, 32768)[0])
    assert [(b["btype"], len(b["stored"]), b["final"]) for b in blocks] == [(0, 65535, 0), (0, 1, 1)]
    blocks = AH.walk_blocks(oracle(big, (U,), 65536, 32768)[0])
    assert [(len(b["stored"]), b["final"]) for b in blocks] == [(65535, 0), (1, 0), (65535, 0), (1, 1)]
    assert [(len(b["stored"]), b["final"]) for b in AH.walk_blocks(oracle(b"", (U,), 65536, 32768)[0])] == [(0, 1)]


FIVE = (FD, RLE_DYNAMIC, LITERAL_STATIC, (True, 4, 32, 2, 1024), U)
EIGHT = FIVE + (FS, LITERAL_DYNAMIC, (False, 3, 258, 64, 32767))


def tuple_buffers():
    return H.edge_buffers()[::7] + [b for b in H.chain_buffers() if len(b) < 10000] + LZ.inputs(12)[::2]


# the two lists after them take the host's short cuts: equal substrategies that leave one Lz77Huffman (forwarded to
# ndfl_deflate_batch_lz77), and literal-only ones alone, for which the kernel skips its link pass
@pytest.mark.parametrize("subs", [FIVE, EIGHT, (FD, FD), (LITERAL_STATIC, U, LITERAL_DYNAMIC)],
                         ids=["five", "eight", "duplicates", "literal-only"])
def test_tuples(ctx, subs):
    run_check(ctx, raws(tuple_buffers()), (subs, 65536, 32768), "tuples")


def single_oracle(buf, subs, chunk_len, hist_limit):
    return H.lz_oracle(buf, subs[0], chunk_len, hist_limit)


@pytest.mark.parametrize("params", [s for s in EIGHT if s != U])
def test_one_substrategy_alone_is_that_strategy(ctx, params):
    H.run_check(raw, single_oracle, ctx, raws(tuple_buffers()), ((params,), 65536, 32768), "alone")


def test_best_so_far_survives_a_loser_and_loses_to_a_winner(ctx):
    rng = random.Random(0xBE57)
    trio = (FD, (True, 3, 8, 1, 64), LITERAL_DYNAMIC)
    for buf in (salad(rng, 4096), mixed(rng, 3000)):
        winners = set()
        for order in itertools.permutations(trio):
            subs = order + (U,)
            comp = oracle(buf, subs)[0]
            # one chunk from bit 0: the stream is the winner's stream
            winners.add(next(i for i, s in enumerate(subs) if oracle(buf, (s,))[0] == comp))
            run_check(ctx, raws([buf, buf[:700], buf[1:]]), (subs, 65536, 32768), "orders")
        assert len(winners) > 1, winners


@pytest.mark.parametrize("hist_limit", [0, 1, 100, 32768])
@pytest.mark.parametrize("chunk_len", [1, 7, 259, 1000, 65536])
def test_chunk_ends_and_history(ctx, chunk_len, hist_limit):
    run_check(ctx, raws(H.chunk_edge_buffers()), (T3, chunk_len, hist_limit), "chunk end")


def test_wave_reuse_one_wave(one_wave):
    """Nothing of the stream before -- its best so far, its histograms, its stored block's position -- leaks."""
    items = H.reuse_items()
    assert len(items) == 300
    for cfg in (DEFAULT, ((U, FD), 259, 32768)):
        run_check(one_wave, items, cfg, "one wave")


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_capacity(ctx, fmt):
    """test_gpu_deflate_batch_lz.py's construction, once with a Huffman member and once with a stored one in
    the region of 0, 1, R - 1 and R bytes."""
    rng = random.Random(9)
    left, right = salad(rng, 777), salad(rng, 1500)
    for mid in (mixed(rng, 4000), rng.randbytes(300)):
        R = len(member(mid, fmt, DEFAULT)[0])
        H.capacity_layout(raw, oracle, ctx, DEFAULT, left, mid, right, fmt, [0, 1, R - 1, R])
    assert btypes(oracle(mid)[0]) == [0]


def layout_items():
    rng = random.Random(78)
    items = H.layout_items()
    for k, n in enumerate((5, 64, 255, 256, 257, 300, 1025)):          # stored members between the others
        items.insert(4 * k + 1, (rng.randbytes(n), (GZIP, RAW, ZLIB)[k % 3], (CRC32, NONE, ADLER32)[k % 3]))
    return items


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_touching_regions_at_every_alignment(ctx, shift):
    items = layout_items()
    assert sum(btypes(oracle(b)[0]) == [0] for b, _, _ in items) >= 5
    H.touching_regions(raw, oracle, ctx, items, DEFAULT, range(4), shift)


def test_device_pointers_on_the_callers_stream(ctx):
    H.device_pointers_on_the_callers_stream(raw, oracle, ctx, H.reuse_items()[:60] + layout_items(), DEFAULT)


def test_arguments(ctx):
    import ndfl
    L = ndfl._lib.load()
    D = ndfl._lib.StrategyDesc
    t3 = descs(T3)
    ok = (T3, 65536, 32768)

    def own_cases(one):
        # the frame; the strategies: none, too many, another kind; the six invalid tuples of test_gpu_lz77.py
        cases = [(E_ARG, one, (t3, 0, 32768)), (E_UNSUPPORTED, one, (t3, 65537, 32768)), (E_ARG, one, (t3, 65536, 32769)),
                 (E_ARG, one, ([], 65536, 32768)), (E_UNSUPPORTED, one, (descs((FD,)) * 9, 65536, 32768)),
                 (E_ARG, one, ([D(1, 0, 0, 0, 0, 0), D(2, 1, 3, 258, 1, 32768)], 65536, 32768)),
                 (E_ARG, one, (descs((U,)), 0, 32768)), (E_UNSUPPORTED, one, (descs((U,)), 65537, 32768)),
                 (E_ARG, one, (descs((FD,)), 65536, 32769))]
        for bad in H.BAD_TUPLES:
            cases += [(E_ARG, one, (descs((U, bad)), 65536, 32768)), (E_ARG, one, (descs((bad,)), 65536, 32768)),
                      (E_ARG, one, (descs((FS, FD, bad)), 65536, 32768))]
        return cases

    a = H.argument_rules(raw, c_call, ctx, ok, own_cases)
    # n == 0 with no strategies either; a null list and a count of 0 with a list
    arr3 = (D * 3)(*t3)
    assert L.ndfl_deflate_batch_multi(ctx._h, None, 0, None, 0, None, None, 0, None, 0, 65536, 32768, 0) == 0
    res = (ndfl._lib.DeflateResult * 1)()
    arr = (ndfl._lib.MemberItem * 1)(ndfl._lib.MemberItem(*a.one[0]))
    before = bytes(res)
    good = (a.a_in, len(a.s), a.a_out, 256, arr, res, 1)
    assert L.ndfl_deflate_batch_multi(ctx._h, *good, arr3, 0, 65536, 32768, 0) == E_ARG
    assert L.ndfl_deflate_batch_multi(ctx._h, *good, None, 3, 65536, 32768, 0) == E_ARG
    nine = (D * 9)(*(descs((FD,)) * 9))
    assert L.ndfl_deflate_batch_multi(ctx._h, *good, nine, 9, 65536, 32768, 0) == E_UNSUPPORTED
    assert bytes(res) == before and a.out.raw == bytes([FILL]) * 256
    # ndfl_deflate_batch itself still refuses what this call is for
    for name in ("FULL_DYNAMIC", "UNCOMPRESSED"):
        with pytest.raises(ndfl.NdflError) as e:
            ctx.deflate_batch_raw(a.a_in, len(a.s), a.a_out, 256, a.one, name, 65536, 32768, 0)
        assert e.value.code == E_UNSUPPORTED and a.out.raw == bytes([FILL]) * 256
    H.regions_that_only_touch(raw, oracle, ctx, ok, a)


def test_equals_the_one_stream_encoder(ctx):
    """GPU against GPU: the batch's bytes for a 200,000-byte buffer are ctx.deflate's."""
    import ndfl
    buf = mixed(random.Random(31), 200000)
    strategy = ndfl.MultiStrategy(ndfl.Uncompressed.SINGLETON, ndfl.Lz77Huffman.FULL_STATIC, ndfl.Lz77Huffman.FULL_DYNAMIC,
                                  ndfl.Lz77Huffman.RLE_DYNAMIC)
    for chunk_len, hist_limit in ((65536, 32768), (10000, 0)):
        comp, bits, _ = ctx.deflate_batch([buf], strategy, chunk_len, hist_limit)[0]
        assert comp == ctx.deflate(buf, strategy, chunk_len, hist_limit)
        assert (bits + 7) // 8 == len(comp)


def test_python_routing(ctx):
    import ndfl
    LH, US = ndfl.Lz77Huffman, ndfl.Uncompressed.SINGLETON
    rng = random.Random(13)
    bufs = [b"", b"x", salad(rng, 3000), mixed(rng, 70000), b"\xff" * 70000, rng.randbytes(2000), rng.randbytes(70000)]
    t3 = ndfl.MultiStrategy(US, LH.FULL_STATIC, LH.FULL_DYNAMIC)
    for fmt, unpack in ((GZIP, gzip.decompress), (ZLIB, zlib.decompress)):
        members = ctx.deflate_members(bufs, fmt, strategy=t3)
        header = bytes((ndfl.ZlibMetadata.DEFAULT if fmt == ZLIB else ndfl.GzipMetadata()).header_bytes())
        for b, m in zip(bufs, members):
            assert m == header + oracle(b)[0] + trailer(b, fmt)
            assert unpack(m) == b
        back = ctx.inflate_members(members, fmt, out_caps=[len(b) for b in bufs])
        for b, m, (reason, out, bits, ck, hl) in zip(bufs, members, back):
            assert reason is None and out == b and bits == 8 * len(m) and hl == len(header)
            assert ck == checksum(b, fmt, NONE)
    # Uncompressed.SINGLETON goes to the new call
    for (comp, bits, ck), b in zip(ctx.deflate_batch(bufs, US, sum=ndfl.SUM_CRC32), bufs):
        assert (comp, bits) == oracle(b, (U,)) and ck == zlib.crc32(b)
    assert ctx.deflate_batch(bufs[:3], ndfl.MultiStrategy(LH.FULL_DYNAMIC)) == ctx.deflate_batch(bufs[:3], LH.FULL_DYNAMIC)
    # what is not batched stays refused
    for strategy in (ndfl.MultiStrategy(US, ndfl.MultiStrategy(LH.FULL_STATIC, LH.FULL_DYNAMIC)),
                     ndfl.MultiStrategy(*([LH.FULL_DYNAMIC] * 8 + [US])),
                     ndfl.MultiStrategy(US, ndfl.BinarySplit(LH.FULL_DYNAMIC, 1000))):
        with pytest.raises(ndfl.NdflError) as e:
            ctx.deflate_batch(bufs[:2], strategy)
        assert e.value.code == E_UNSUPPORTED
    # the preset names keep ndfl_deflate_batch
    assert ctx.deflate_members([bufs[2]], GZIP, strategy="RLE_DYNAMIC") == ctx.deflate_members([bufs[2]], GZIP)


def test_never_longer_than_a_part(ctx):
    """end_bits is the DEFLATE data alone, and every chunk takes the fewest bits at its position: by the
    reference's construction a stream is no longer than under one of its substrategies alone."""
    rng = random.Random(0x1E55)
    bufs = type_buffers()
    for k in range(100):
        n = rng.randrange(0, 3000)
        bufs.append(salad(rng, n) if k % 2 else rng.randbytes(n))
    both = run_check(ctx, raws(bufs), DEFAULT, "T3")
    for sub in (U, FS, FD):
        alone = run_check(ctx, raws(bufs), ((sub,), 65536, 32768), "alone")
        for b, r, a in zip(bufs, both, alone):
            assert r[3] <= a[3], (sub, len(b), r[3], a[3])
