"""ndfl_deflate_batch_binsplit on the GPU: many independent buffers compressed in one call under
BinarySplit(Lz77Huffman(...), minBlockLen), every chunk split into the blocks the reference's recursion
chooses.  Each stream is checked byte for byte against the CPU oracle on that buffer alone -- the DEFLATE
bytes are O.deflate_binsplit(buffer, sub, min_block_len, chunk_len, hist_limit), which handles odd halvings,
end_bits is the bit at which the oracle's decoder ends that stream, the checksums are Python's zlib.crc32 /
zlib.adler32 -- and every byte of `out` outside the streams' stored bytes must still hold the fill byte.

The inputs are built so that the split tree is deep (csrc/hip/deflate_batch_binsplit.hip: the stack, the
leaves searched again, the leaf emitted from the block in place): ladder(nseg, seglen) has 16 byte values
of its own in every segment, so a dynamic code per segment beats one code over all of them.  Every test
that is about splitting asserts on the oracle's stream that it is split (adversarial_hist.walk_blocks),
so none of them can quietly turn into the unsplit case.

cfg = (sub, min_block_len, chunk_len, hist_limit); FD = FULL_DYNAMIC, FS = FULL_STATIC.
"""
import ctypes
import functools
import gzip
import random
import zlib

import pytest

import adversarial_hist as AH
import deflate_batch_harness as H
import oracle_lib as O
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_UNSUPPORTED, GZIP, NONE, RAW, ZLIB, ctx, one_wave, raws, salad,
                                   trailer)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FS, FD = H.FULL_STATIC, H.FULL_DYNAMIC
RLE_DYNAMIC = (True, 3, 258, 1, 1)
LITERAL_DYNAMIC = (True, 0, 0, 0, 0)
ODD = (True, 4, 32, 2, 1024)
TUPLES = {"FULL_DYNAMIC": FD, "RLE_DYNAMIC": RLE_DYNAMIC, "LITERAL_DYNAMIC": LITERAL_DYNAMIC, "FULL_STATIC": FS, "odd": ODD}
DEFAULT = (FD, 100, 65536, 32768)


@functools.lru_cache(maxsize=None)
def oracle(buf, sub=FD, min_block_len=100, chunk_len=65536, hist_limit=32768):
    """(DEFLATE bytes, end bits) of one buffer alone, computed once; the oracle's decoder gives the bits."""
    comp = O.deflate_binsplit(buf, sub, min_block_len, chunk_len, hist_limit)
    reason, back, bits = O.inflate(comp, out_cap=len(buf) + 64)
    assert reason is None and back == buf and (bits + 7) // 8 == len(comp)
    return comp, bits


def desc(sub):
    """The StrategyDesc record of an Lz77Huffman tuple (None and ready-made records pass through)."""
    import ndfl
    return sub if sub is None or isinstance(sub, ndfl._lib.StrategyDesc) else ndfl._lib.StrategyDesc(0, *map(int, sub))


def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_binsplit; cfg: (sub, min_block_len, chunk_len, hist_limit)."""
    sub, min_block_len, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_binsplit_raw(in_addr, in_size, out_addr, out_size, recs, desc(sub), min_block_len,
                                          chunk_len, hist_limit, flags)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


def c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg):
    import ndfl
    sub = desc(cfg[0])
    return ndfl._lib.load().ndfl_deflate_batch_binsplit(ctx._h, in_addr, in_size, out_addr, out_size, items, results, n,
                                                        None if sub is None else ctypes.byref(sub), cfg[1], cfg[2], cfg[3], 0)


def nblocks(buf, *cfg):
    return len(AH.walk_blocks(oracle(buf, *cfg)[0]))


@functools.lru_cache(maxsize=None)
def ladder(nseg, seglen):
    """Segment s: seglen bytes drawn uniformly from the 16 byte values 16 * s .. 16 * s + 15."""
    rng = random.Random(0x1ADD)
    return b"".join(bytes(16 * s + rng.randrange(16) for _ in range(seglen)) for s in range(nseg))


def letters(rng, n, alphabet=b"abcdefghijklmnopqrstuvwxyz"):
    return bytes(rng.choice(alphabet) for _ in range(n))


EVEN, UNEVEN = (16, 256), (13, 333)      # 4,096 bytes: even halvings; 4,329: halves 2165/2164, 1083/1082, ...


def lz_end_bits(ctx, bufs, cfg):
    """end_bits of the same buffers under ndfl_deflate_batch_lz77 with cfg's tuple, chunk_len and hist_limit."""
    sub, _, chunk_len, hist_limit = cfg
    return [r[3] for r in H.run_check(H.lz_raw, H.lz_oracle, ctx, raws(bufs), (sub, chunk_len, hist_limit), "unsplit")]


@pytest.mark.parametrize("min_block_len", [1, 100, 300, 1100])
@pytest.mark.parametrize("name", list(TUPLES))
def test_depth_and_odd_halvings(ctx, name, min_block_len):
    sub = TUPLES[name]
    cfg = (sub, min_block_len, 65536, 32768)
    bufs = [ladder(*EVEN), ladder(*UNEVEN)]
    assert [len(b) for b in bufs] == [4096, 4329]
    if sub[0]:                               # (fixed codes gain nothing on these inputs: one block, searched 3 times)
        for b in bufs:
            assert nblocks(b, *cfg) >= (8 if min_block_len <= 300 else 2), (name, min_block_len, nblocks(b, *cfg))
    res = run_check(ctx, raws(bufs), cfg, "ladders")
    assert all(r[0] == 0 for r in res)
    # never longer than unsplit
    for r, unsplit in zip(res, lz_end_bits(ctx, bufs, cfg)):
        assert r[3] <= unsplit, (name, min_block_len, r[3], unsplit)


def test_depth_counts_of_the_oracle():
    """The trees the other tests rely on, FULL_DYNAMIC: depth 4 at min_block_len 1 and 100, 3 at 300, 1 at 1100."""
    a = ladder(*EVEN)
    assert [nblocks(a, FD, m) for m in (1, 100, 300, 1100)] == [16, 16, 8, 2]
    assert nblocks(ladder(*UNEVEN), FD, 100) >= 16
    assert len(oracle(a)[0]) < 0.7 * len(H.lz_oracle(a)[0])         # this is where BinarySplit pays


def static_splitters():
    """Short strings over a few letters on which two fresh greedy parses under the FIXED codes are shorter
    than one (found by search with the oracle; min_block_len 4)."""
    bufs = []
    for seed in (151, 286, 666, 671, 674, 706, 837, 881, 1366):
        r = random.Random(seed)
        n = r.randrange(20, 400)
        k = r.randrange(2, 8)
        bufs.append(bytes(r.randrange(k) + 97 for _ in range(n)))
    return bufs


def test_static_codes_split_too(ctx):
    bufs = static_splitters()
    cfg = (FS, 4, 65536, 32768)
    for b in bufs:
        assert nblocks(b, *cfg) > 1, len(b)
    res = run_check(ctx, raws(bufs), cfg, "static")
    for r, unsplit in zip(res, lz_end_bits(ctx, bufs, cfg)):
        assert r[3] <= unsplit


def test_halves_must_be_longer_than_min_block_len(ctx):
    """513 bytes, halves of 257 and 256: split at min_block_len 255, not at 256."""
    rng = random.Random(0x513)
    buf = letters(rng, 257, b"01") + letters(rng, 256)
    assert nblocks(buf, FD, 255) == 2 and nblocks(buf, FD, 256) == 1
    assert len(oracle(buf, FD, 255)[0]) < len(oracle(buf, FD, 256)[0]) == len(H.lz_oracle(buf)[0])
    for m in (255, 256):
        run_check(ctx, raws([buf]), (FD, m, 65536, 32768), "min(f, s) > min_block_len")


@functools.lru_cache(maxsize=None)
def mixed_batch():
    rng = random.Random(0xB175)
    four = letters(rng, 1024, b"0123456789") + letters(rng, 1024) + rng.randbytes(1024) + bytes(1024)
    bufs = [rng.randbytes(n) for n in (0, 1, 2, 3, 5, 7)]
    bufs += [letters(rng, 3000), ladder(*EVEN), ladder(*UNEVEN), four]
    fmts = ((RAW, CRC32), (RAW, ADLER32), (ZLIB, NONE), (GZIP, NONE))
    return tuple((b,) + fmts[k % 4] for k, b in enumerate(bufs))


def check_mixed_batch_shape():
    items = mixed_batch()
    assert nblocks(items[6][0]) == 1                                    # uniform text never splits
    assert nblocks(items[7][0]) >= 8 and nblocks(items[8][0]) >= 8
    assert nblocks(items[9][0]) >= 3                                    # depth 2


def test_mixed_batch(ctx):
    check_mixed_batch_shape()
    items = list(mixed_batch())
    res = run_check(ctx, items, DEFAULT, "mixed")
    assert all(r[0] == 0 for r in res)
    for r, unsplit in zip(res, lz_end_bits(ctx, [b for b, _, _ in items], DEFAULT)):
        assert r[3] <= unsplit


def test_wave_reuse_one_wave(one_wave):
    """The stack, the head table and the histograms start afresh for each stream: one wave encodes them all,
    the deep trees before the short buffers and after them."""
    check_mixed_batch_shape()
    items = list(mixed_batch())
    items = items[6:] + items + items[::-1]
    run_check(one_wave, items, DEFAULT, "one wave")
    run_check(one_wave, items, (RLE_DYNAMIC, 1, 1000, 100), "one wave, chunks")


@pytest.mark.parametrize("chunk_len,hist_limit", [(3000, 32768), (3000, 0), (4097, 100), (1000, 1), (65536, 32768)])
def test_chunks_and_history(ctx, chunk_len, hist_limit):
    buf = ladder(16, 512)
    cfg = (FD, 100, chunk_len, hist_limit)
    chunks = -(-len(buf) // chunk_len)
    assert nblocks(buf, *cfg) >= 8
    if chunk_len in (3000, 4097):
        assert chunks >= 2 and nblocks(buf, *cfg) >= 4 * chunks              # several chunks are split
    run_check(ctx, raws([buf, buf[:chunk_len + 1], buf[1:]]), cfg, "chunks")


def test_partial_second_chunk_with_a_window_behind_it(ctx):
    """70,000 bytes, chunk_len 65536, min_block_len 1: the second chunk is partial and its sub-blocks' windows
    reach back into the first.  The first chunk's segments double in length (256, 256, 512, ... 32,768
    bytes, 16 byte values each), so every split along the left spine wins and the right halves wait on the
    stack, eight at once."""
    rng = random.Random(0x70000)
    sizes = [256] + [256 << k for k in range(8)]
    first = b"".join(bytes(16 * s + rng.randrange(16) for _ in range(n)) for s, n in enumerate(sizes))
    buf = first + ladder(16, 512)[:70000 - 65536]
    assert len(first) == 65536 and len(buf) == 70000
    cfg = (FD, 1, 65536, 32768)
    assert nblocks(first, *cfg) >= 9 and nblocks(buf, *cfg) >= 9 + 2
    run_check(ctx, raws([buf]), cfg, "70,000 bytes")


@pytest.mark.parametrize("fmt", [RAW, ZLIB, GZIP])
def test_capacity(ctx, fmt):
    """A region one byte short, one cut inside the second block, and one of 0 bytes, between neighbours whose
    regions touch it: status, out_len == R, the stored prefix, and the neighbours bit-exact."""
    rng = random.Random(9)
    left, mid, right = salad(rng, 777), ladder(*UNEVEN), salad(rng, 1500)
    blocks = AH.walk_blocks(oracle(mid)[0])
    assert len(blocks) >= 8
    inside_second = (blocks[1]["bit"] + blocks[1]["end_bit"]) // 16
    R = len(member(mid, fmt, DEFAULT)[0])
    assert 0 < inside_second < R - 1
    H.capacity_layout(raw, oracle, ctx, DEFAULT, left, mid, right, fmt, [0, inside_second, R - 1, R])


def layout_items():
    items = H.layout_items()
    for k, b in enumerate((ladder(*EVEN), ladder(*UNEVEN), ladder(5, 100), ladder(3, 211))):
        items.insert(5 * k + 1, (b, (GZIP, RAW, ZLIB)[k % 3], (CRC32, NONE, ADLER32)[k % 3]))
    return items


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_touching_regions_at_every_alignment(ctx, shift):
    items = layout_items()
    assert sum(nblocks(b) > 1 for b, _, _ in items) >= 4
    H.touching_regions(raw, oracle, ctx, items, DEFAULT, range(4), shift)


def test_device_pointers_on_the_callers_stream(ctx):
    H.device_pointers_on_the_callers_stream(raw, oracle, ctx, list(mixed_batch()) + layout_items(), DEFAULT)


def test_arguments(ctx):
    import ndfl
    L = ndfl._lib.load()
    D = ndfl._lib.StrategyDesc
    fd = desc(FD)
    ok = (FD, 100, 65536, 32768)

    def own_cases(one):
        stored, seven = D(1, 0, 0, 0, 0, 0), D(7, 1, 3, 258, 1, 32768)
        cases = [(E_ARG, one, (None, 100, 65536, 32768)), (E_ARG, one, (fd, 0, 65536, 32768)),
                 (E_ARG, one, (fd, -1, 65536, 32768)), (E_ARG, one, (fd, 100, 0, 32768)),
                 (E_UNSUPPORTED, one, (fd, 100, 65537, 32768)), (E_ARG, one, (fd, 100, 65536, 32769)),
                 (E_UNSUPPORTED, one, (stored, 100, 65536, 32768)), (E_UNSUPPORTED, one, (seven, 100, 65536, 32768)),
                 # ndfl_deflate_chunks_binsplit's order: min_block_len before the frame, the frame before the kind,
                 # the kind before the tuple
                 (E_ARG, one, (stored, 0, 65537, 32768)), (E_UNSUPPORTED, one, (stored, 100, 65537, 32768)),
                 (E_ARG, one, (stored, 100, 0, 32768)), (E_ARG, one, (stored, 100, 65536, 32769)),
                 (E_UNSUPPORTED, one, (D(1, 1, 2, 258, 1, 32768), 100, 65536, 32768))]
        return cases + [(E_ARG, one, (desc(bad), 100, 65536, 32768)) for bad in H.BAD_TUPLES]

    a = H.argument_rules(raw, c_call, ctx, ok, own_cases)
    # n == 0: nothing is looked at, not the substrategy, min_block_len, chunk_len or hist_limit either
    assert L.ndfl_deflate_batch_binsplit(ctx._h, None, 0, None, 0, None, None, 0, None, 0, 0, 40000, 0) == 0
    H.regions_that_only_touch(raw, oracle, ctx, ok, a)


def test_against_the_chunked_encoder(ctx):
    """GPU against GPU: where ndfl_deflate_chunks_binsplit takes the input (every halving even) the streams
    are equal bit for bit; an odd halving it refuses, and the batch encodes."""
    import ndfl
    strategy = ndfl.BinarySplit(ndfl.Lz77Huffman.FULL_DYNAMIC, 100)
    even, uneven = ladder(*EVEN), ladder(*UNEVEN)
    comp, bits, _ = ctx.deflate_batch([even], strategy, 4096, 32768)[0]
    assert nblocks(even, FD, 100, 4096, 32768) >= 8
    assert comp == ctx.deflate(even, strategy, 4096, 32768) and (bits + 7) // 8 == len(comp)
    with pytest.raises(ndfl.NdflError) as e:
        ctx.deflate(uneven, strategy, len(uneven), 32768)          # (a full chunk of an odd length)
    assert e.value.code == E_UNSUPPORTED
    comp, bits, _ = ctx.deflate_batch([uneven], strategy, len(uneven), 32768)[0]
    assert (comp, bits) == oracle(uneven, FD, 100, len(uneven), 32768) and nblocks(uneven, FD, 100, len(uneven), 32768) >= 8


def test_python_routing(ctx):
    import ndfl
    LH, US = ndfl.Lz77Huffman, ndfl.Uncompressed.SINGLETON
    bufs = [b for b, _, _ in mixed_batch()]
    for lz, sub in ((LH.FULL_DYNAMIC, FD), (LH.RLE_DYNAMIC, RLE_DYNAMIC), (LH.FULL_STATIC, FS)):
        got = ctx.deflate_batch(bufs, strategy=ndfl.BinarySplit(lz, 100), sum=ndfl.SUM_CRC32)
        for (comp, bits, ck), b in zip(got, bufs):
            assert (comp, bits) == oracle(b, sub) and ck == zlib.crc32(b)
    members = ctx.deflate_members(bufs, ndfl.FMT_GZIP, strategy=ndfl.BinarySplit(LH.FULL_DYNAMIC, 100))
    header = bytes(ndfl.GzipMetadata().header_bytes())
    for b, m in zip(bufs, members):
        assert m == header + oracle(b)[0] + trailer(b, GZIP)
        assert gzip.decompress(m) == b
    # what is not batched stays refused
    for strategy in (ndfl.BinarySplit(US, 100), ndfl.BinarySplit(ndfl.MultiStrategy(LH.FULL_DYNAMIC, US), 100)):
        with pytest.raises(ndfl.NdflError) as e:
            ctx.deflate_batch(bufs[:2], strategy)
        assert e.value.code == E_UNSUPPORTED
    # the other routes are as they were
    assert ctx.deflate_batch(bufs[:7], LH.FULL_DYNAMIC)[6][:2] == H.lz_oracle(bufs[6])
