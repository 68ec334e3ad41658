"""ndfl_deflate_batch on the GPU: many independent buffers compressed in one call, each stream
checked against the CPU oracle on that buffer alone -- the DEFLATE bytes are O.deflate(buffer, strategy,
chunk_len, hist_limit), end_bits is O.deflate_chunks(b"", buffer, True, ...)'s, the checksums are
Python's zlib.crc32 / zlib.adler32 -- and every byte of `out` outside the streams' stored bytes must
still hold the fill byte.

The buffers are the places where the batch kernel (csrc/hip/deflate_batch.hip) can go wrong: a wave
walks a chunk in steps of 64 lanes x 16 bytes and carries the run piece that is open at a step's end
into the next step, so runs start and end around every boundary it has (16 bytes per lane, 1024 bytes
per step, the chunk length), at the run lengths where the closed-form parse changes shape (remainders
0..3 after whole 258s, with and without the lead literal).
"""
import concurrent.futures
import functools
import gzip
import random
import zlib

import pytest

import adversarial_hist as A
import deflate_batch_harness as H
import oracle_lib as O
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_UNSUPPORTED, GZIP, NONE, RAW, ZLIB, checksum, ctx, mixed, one_wave,
                                   pack_inputs, salad, trailer)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

STRATEGIES = ["LITERAL_STATIC", "LITERAL_DYNAMIC", "RLE_STATIC", "RLE_DYNAMIC"]
CONFIGS = [(65536, 32768), (259, 32768), (259, 0), (7, 32768), (1, 32768)]
BPL, STEP = 16, 1024              # the kernel's bytes per lane and per step (deflate_batch.hip)
BIG = 65535                       # buffers from this size on run at chunk_len 65536 only


@functools.lru_cache(maxsize=None)
def oracle(buf, strategy="RLE_DYNAMIC", chunk_len=65536, hist_limit=32768):
    """(DEFLATE bytes, end bits) of one buffer alone, computed once."""
    comp = O.deflate(buf, strategy, chunk_len, hist_limit)
    comp2, bits = O.deflate_chunks(b"", buf, True, strategy, chunk_len, hist_limit)
    assert comp2 == comp and (bits + 7) // 8 == len(comp)
    return comp, bits


def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch; cfg: (strategy, chunk_len, hist_limit)."""
    return ctx.deflate_batch_raw(in_addr, in_size, out_addr, out_size, recs, *cfg, flags)


def c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg):
    import ndfl
    strategy, chunk_len, hist_limit = cfg
    return ndfl._lib.load().ndfl_deflate_batch(ctx._h, in_addr, in_size, out_addr, out_size, items, results, n,
                                               ndfl.STRATEGIES.get(strategy, strategy), chunk_len, hist_limit, 0)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


def no_runs(rng, n):
    """n random bytes with no two equal neighbours, so that the only runs are the ones spliced in."""
    b = bytearray(rng.randbytes(n))
    for i in range(1, n):
        if b[i] == b[i - 1]:
            b[i] = (b[i] + 1 + (i + 1 < n and b[i + 1] == (b[i] + 1) & 0xFF)) & 0xFF
    return b


def with_run(rng, n, start, length):
    """no_runs bytes with bytes [start, start + length) one value that differs from both neighbours."""
    b = no_runs(rng, n)
    v = next(x for x in range(256) if x != b[start - 1 if start else 0] and (start + length >= n or x != b[start + length]))
    b[start:start + length] = bytes([v]) * length
    return bytes(b)


BOUNDARIES = [7, BPL, 2 * BPL, 259, 2 * 259, STEP, 2 * STEP, 65536]


@functools.lru_cache(maxsize=None)
def parity_buffers():
    rng = random.Random(0xDEF1A7E)
    bufs = [b"", b"a", b"ab", b"aa", b"abc", b"aaa"]
    bufs += [b"\x55" * n for n in (3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 519, 776, 4097)]
    for B in BOUNDARIES:
        pad = 700 if B < BIG else 40
        for d in range(-3, 4):
            for length in (4, 300 if B < BIG else 30):
                if B + d >= 0:
                    bufs.append(with_run(rng, B + pad, B + d, length))                      # starts at B + d
                if B + d - length >= 0:
                    bufs.append(with_run(rng, B + pad, B + d - length, length))             # ends at B + d
        bufs.append(with_run(rng, B + pad, max(0, B - 150), 300))                            # straddles B
        bufs += [bytes(no_runs(rng, n)) for n in (B - 1, B, B + 1)]
        bufs += [b"\x00" * n for n in (B - 1, B, B + 1)]
    bufs.append(b"ab" * 1500)
    bufs.append(rng.randbytes(5000))
    bufs.append(bytes(range(256)))
    bufs.append(salad(rng, 6000))
    # (the 15-bit literal/length limit and the 7-bit code-length limit: test_oracle_deflate.py asserts that
    # these inputs reach them on the oracle's streams)
    bufs += [c.data for cls in ("lit_limit", "cl_limit") for c in A.cases(cls)]
    bufs += [mixed(rng, n) for n in (65535, 65536, 65537, 131073)]
    return bufs


@pytest.mark.parametrize("chunk_len,hist_limit", CONFIGS)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_parity(ctx, strategy, chunk_len, hist_limit):
    bufs = [b for b in parity_buffers() if chunk_len == 65536 or len(b) < BIG]
    assert len(bufs) > 200
    cfg = (strategy, chunk_len, hist_limit)
    # the oracle's streams, eight buffers at a time (or_deflate keeps no state between calls once its
    # fixed-code tables exist, and ctypes releases the interpreter lock): chunk_len 1 is 500,000 blocks
    oracle(b"", *cfg)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda b: oracle(b, *cfg), bufs))
    res = run_check(ctx, [(b, RAW, NONE) for b in bufs], cfg, "parity")
    assert all(r[0] == 0 for r in res)


LAYOUT_LENGTHS = [0, 1, 2, 3, 5, 15, 16, 17, 40, 258, 700, 1023, 1024, 1025, 3000, 5000]


def layout_items():
    rng = random.Random(77)
    items = []
    for k, n in enumerate(LAYOUT_LENGTHS * 2):
        buf = mixed(rng, n) if k % 2 else salad(rng, n)
        items.append((buf, (RAW, ZLIB, GZIP)[k % 3], (NONE, CRC32, ADLER32)[k % 3]))
    return items


def test_layout_touching_regions_every_residue(ctx):
    """Regions that touch, with out_off at every residue mod 16 (the members' lengths shift them, and a
    leading pad of 0..15 bytes shifts all of them), and `out` itself at an odd address."""
    seen = H.touching_regions(raw, oracle, ctx, layout_items(), ("RLE_DYNAMIC", 65536, 32768), range(16), lambda pad: pad % 2)
    assert seen == set(range(16))


def test_layout_shuffled_regions_with_gaps_and_shared_inputs(ctx):
    """Regions in an order other than the item order, with gaps of 0..9 bytes; one input region used by
    two items and overlapped by a third."""
    cfg = ("RLE_DYNAMIC", 259, 32768)
    rng = random.Random(5)
    items = layout_items()
    base = mixed(rng, 3000)
    items += [(base, RAW, CRC32), (base, ZLIB, NONE), (base[1000:], GZIP, NONE)]
    packed, offs = pack_inputs(items[:-3])
    offs += [len(packed), len(packed), len(packed) + 1000]
    packed += base
    order = list(range(len(items)))
    rng.shuffle(order)
    regions, off = [None] * len(items), 3
    for i in order:
        n = len(member(items[i][0], items[i][1], cfg)[0])
        regions[i] = (off, n)
        off += n + rng.randrange(0, 10)
    res, out, _ = run(ctx, items, cfg, regions=regions, out_size=off + 7, out_shift=1, inputs=(packed, offs))
    check(items, cfg, res, out, regions, "shuffled")


@pytest.mark.parametrize("fmt", [RAW, ZLIB])
def test_capacity(ctx, fmt):
    """A stream that needs R bytes in a region of 0, 1, R - 1 and R (and, for a zlib member, regions that
    end inside its trailer), between neighbours whose regions touch it: status, out_len == R, the stored
    prefix, and the neighbours bit-exact."""
    cfg = ("RLE_DYNAMIC", 65536, 32768)
    rng = random.Random(9)
    left, mid, right = salad(rng, 777), mixed(rng, 4000), mixed(rng, 1500)
    R = len(member(mid, fmt, cfg)[0])
    H.capacity_layout(raw, oracle, ctx, cfg, left, mid, right, fmt,
                      [0, 1, R - 1, R] + ([R - 4, R - 3, R - 2] if fmt == ZLIB else []))


def test_checksums_and_trailers(ctx):
    rng = random.Random(11)
    bufs = [b"", b"\x00", b"\xff" * 70000, salad(rng, 5000), mixed(rng, 70001), rng.randbytes(1025), b"a" * 1024,
            bytes(range(256)) * 5]
    items = [(b, fmt, kind) for b in bufs for fmt, kind in
             ((RAW, CRC32), (RAW, ADLER32), (RAW, NONE), (ZLIB, NONE), (GZIP, NONE), (ZLIB, CRC32), (GZIP, ADLER32))]
    for cfg in (("RLE_DYNAMIC", 65536, 32768), ("LITERAL_STATIC", 259, 0)):
        run_check(ctx, items, cfg, "checksums")


@pytest.mark.parametrize("fmt", [ZLIB, GZIP])
def test_members_round_trip(ctx, fmt):
    """Context.deflate_members gives complete members: Python's zlib / gzip decode them, and so does
    ctx.inflate_members, with the same checksum."""
    import ndfl
    rng = random.Random(13)
    bufs = [b"", b"x", salad(rng, 3000), mixed(rng, 70000), b"\xff" * 70000, rng.randbytes(2000)]
    members = ctx.deflate_members(bufs, fmt)
    header = bytes((ndfl.ZlibMetadata.DEFAULT if fmt == ZLIB else ndfl.GzipMetadata()).header_bytes())
    for b, m in zip(bufs, members):
        assert m == header + oracle(b)[0] + trailer(b, fmt)
        assert (zlib.decompress(m) if fmt == ZLIB else gzip.decompress(m)) == b
    back = ctx.inflate_members(members, fmt, out_caps=[len(b) for b in bufs])
    for b, m, (reason, out, bits, ck, hl) in zip(bufs, members, back):
        assert reason is None and out == b and bits == 8 * len(m) and hl == len(header)
        assert ck == checksum(b, fmt, NONE)
    if fmt == GZIP:                         # other metadata: the header is the metadata's, the rest the same
        meta = ndfl.GzipMetadata(fileName="a.txt", hasHeaderCrc=True, modificationTimeUnixS=1234567)
        m = ctx.deflate_members([bufs[2]], GZIP, meta=meta, strategy="LITERAL_DYNAMIC", chunk_len=259)[0]
        assert gzip.decompress(m) == bufs[2] and b"a.txt\0" in m[:20]
        assert m.endswith(oracle(bufs[2], "LITERAL_DYNAMIC", 259, 32768)[0] + trailer(bufs[2], GZIP))


def test_python_deflate_batch(ctx):
    rng = random.Random(17)
    bufs = [b"", salad(rng, 100), mixed(rng, 9000), b"q" * 300]
    for sum_, ref in ((None, lambda b: 0), (CRC32, zlib.crc32), (ADLER32, zlib.adler32)):
        got = ctx.deflate_batch(bufs, strategy="RLE_STATIC", chunk_len=1000, hist_limit=0, sum=sum_)
        for b, (comp, bits, ck) in zip(bufs, got):
            assert (comp, bits) == oracle(b, "RLE_STATIC", 1000, 0) and ck == ref(b)


@functools.lru_cache(maxsize=None)
def reuse_items():
    """About 200 unlike streams in shuffled order: empty, text, long runs, random, multi-chunk."""
    rng = random.Random(21)
    items = []
    for k in range(200):
        kind = k % 6
        if kind == 0:
            buf = b""
        elif kind == 1:
            buf = salad(rng, rng.randrange(1, 3000))
        elif kind == 2:
            buf = bytes([rng.randrange(256)]) * rng.randrange(1, 5000)
        elif kind == 3:
            buf = rng.randbytes(rng.randrange(1, 1500))
        elif kind == 4:
            buf = mixed(rng, rng.randrange(1, 4000))
        else:
            buf = mixed(rng, 65536 + rng.randrange(0, 3000)) if k % 30 == 5 else bytes(rng.randrange(3) for _ in range(500))
        items.append((buf, (RAW, ZLIB, GZIP)[rng.randrange(3)], (NONE, CRC32, ADLER32)[rng.randrange(3)]))
    rng.shuffle(items)
    return items


def test_wave_reuse_one_wave(one_wave):
    for cfg in (("RLE_DYNAMIC", 65536, 32768), ("RLE_DYNAMIC", 259, 32768)):
        run_check(one_wave, reuse_items(), cfg, "one wave")


def test_more_streams_than_waves(ctx):
    rng = random.Random(23)
    items = [(bytes(rng.randrange(4) for _ in range(rng.randrange(0, 41))), RAW, CRC32) for _ in range(5000)]
    run_check(ctx, items, ("RLE_DYNAMIC", 65536, 32768), "5000 streams")


def test_device_pointers_on_the_callers_stream(ctx):
    H.device_pointers_on_the_callers_stream(raw, oracle, ctx, reuse_items()[:60] + layout_items(), ("RLE_DYNAMIC", 65536, 32768))


def test_arguments(ctx):
    ok = ("RLE_DYNAMIC", 65536, 32768)

    def own_cases(one):
        return [(E_ARG, one, ("RLE_DYNAMIC", 0, 32768)), (E_UNSUPPORTED, one, ("RLE_DYNAMIC", 65537, 32768)),
                (E_ARG, one, ("RLE_DYNAMIC", 65536, 32769)), (E_UNSUPPORTED, one, ("FULL_DYNAMIC", 65536, 32768)),
                (E_UNSUPPORTED, one, ("FULL_STATIC", 65536, 32768)), (E_UNSUPPORTED, one, ("UNCOMPRESSED", 65536, 32768)),
                (E_ARG, one, (7, 65536, 32768))]

    a = H.argument_rules(raw, c_call, ctx, ok, own_cases)
    H.regions_that_only_touch(raw, oracle, ctx, ok, a)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_equals_the_one_stream_encoder(ctx, strategy):
    """GPU against GPU: the batch's bytes for a 200,000-byte buffer are ctx.deflate's."""
    buf = mixed(random.Random(31), 200000)
    for chunk_len, hist_limit in ((65536, 32768), (10000, 0)):
        comp, bits, _ = ctx.deflate_batch([buf], strategy, chunk_len, hist_limit)[0]
        assert comp == ctx.deflate(buf, strategy, chunk_len, hist_limit)
        assert (bits + 7) // 8 == len(comp)
