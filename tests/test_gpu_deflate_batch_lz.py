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
import ctypes
import functools
import gzip
import random
import zlib

import pytest

import deflate_batch_harness as H
import oracle_lib as O
import test_gpu_lz77 as LZ
from deflate_batch_harness import (ADLER32, CRC32, E_ARG, E_CAPACITY, E_UNSUPPORTED, FILL, GZIP, NONE, RAW, ZLIB,
                                   checksum, ctx, mixed, one_wave, pack_inputs, salad, trailer)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FULL_DYNAMIC = (True, 3, 258, 1, 32768)
FULL_STATIC = (False, 3, 258, 1, 32768)
DEFAULT = (FULL_DYNAMIC, 65536, 32768)
STEP = 64                         # positions per step (deflate_batch_lz.hip)


@functools.lru_cache(maxsize=None)
def oracle(buf, params=FULL_DYNAMIC, chunk_len=65536, hist_limit=32768):
    """(DEFLATE bytes, end bits) of one buffer alone, computed once; the oracle's decoder gives the bits."""
    comp = O.deflate_lz(buf, *params, chunk_len, hist_limit)
    reason, back, bits = O.inflate(comp, out_cap=len(buf) + 64)
    assert reason is None and back == buf and (bits + 7) // 8 == len(comp)
    return comp, bits


def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_lz77; cfg: (params, chunk_len, hist_limit)."""
    params, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_lz77_raw(in_addr, in_size, out_addr, out_size, recs, *params, chunk_len, hist_limit, flags)


member = functools.partial(H.member, oracle)
run = functools.partial(H.run, raw, oracle)
check = functools.partial(H.check, oracle)
run_check = functools.partial(H.run_check, raw, oracle)


def raws(bufs):
    return [(b, RAW, NONE) for b in bufs]


def with_repeat(rng, n, src, dst, length):
    """n random bytes with bytes [dst, dst + length) a copy of the bytes from src on (dst > src; the copy
    may overlap its source), and the byte after the copy different from the one after its source."""
    b = bytearray(rng.randbytes(n))
    for k in range(length):
        b[dst + k] = b[src + k]
    if dst + length < n and b[dst + length] == b[src + length]:
        b[dst + length] ^= 0x55
    return bytes(b)


@functools.lru_cache(maxsize=None)
def edge_buffers():
    """Repeats whose source, start and end sit on and around the step edges, at the run lengths where the
    cap bites (258; 600 = 258 + 258 + 84) and the shortest ones."""
    rng = random.Random(0x17A77)
    bufs = []
    for src in (0, 1, 62, 63, 64, 65):
        for dst in (63, 64, 65, 66, 126, 127, 128, 129, 191, 192):
            if dst > src:
                for length in (3, 4, 257, 258, 259, 600):
                    bufs.append(with_repeat(rng, dst + length + rng.randrange(0, 70), src, dst, length))
    for length in (3, 4, 5, 62, 63, 64, 65):                       # the repeat ENDS at 63 / 64 / 65 / 127 / 128
        for end in (63, 64, 65, 127, 128):
            if end - length > 10:
                bufs.append(with_repeat(rng, end + 40, 5, end - length, length))
    bufs.append(with_repeat(rng, 400, 10, 60, 140))                # starts in step 0, ends in step 3
    bufs.append(with_repeat(rng, 400, 10, 63, 130))                # step 0's last lane to step 3's first
    bufs.append(with_repeat(rng, 700, 0, 64, 600))
    return bufs


@pytest.mark.parametrize("params", [FULL_DYNAMIC, FULL_STATIC])
def test_step_and_lane_edges(ctx, params):
    bufs = edge_buffers()
    assert len(bufs) > 300
    res = run_check(ctx, raws(bufs), (params, 65536, 32768), "edges")
    assert all(r[0] == 0 for r in res)


def chunk_edge_buffers():
    rng = random.Random(0xC4C4)
    bufs = [b for b in edge_buffers() if len(b) < 500][::9]
    # a 300-byte repeat that every chunk length below cuts, its source 500 before it; a long run of one byte
    bufs += [with_repeat(rng, 1300, 100, 600, 300), with_repeat(rng, 1300, 599, 600, 650),
             with_repeat(rng, 2100, 0, 1000, 1000), salad(rng, 1500), b"\x00" * 1100, b"ab" * 600]
    return bufs


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


def kernel_hash(trigram):
    """deflate_batch_lz.hip's hash3, restated: the 12 high bits of the 24-bit prefix (little-endian) times
    2654435761 mod 2^32.  A change of the kernel's hash only makes the collision case below a weaker one."""
    k = trigram[0] | trigram[1] << 8 | trigram[2] << 16
    return ((k * 2654435761) & 0xFFFFFFFF) >> 20


def colliding_trigrams():
    a = b"abc"
    for x in range(0x20, 0x7F):
        for y in range(0x20, 0x7F):
            for z in range(0x20, 0x7F):
                b = bytes((x, y, z))
                if b != a and b[0] != a[0] and kernel_hash(b) == kernel_hash(a):
                    return a, b
    raise AssertionError("no colliding pair among the printable trigrams")


def chain_buffers():
    rng = random.Random(0xC4A1)
    bufs = [b"abc" * k for k in (1, 2, 3, 21, 22, 43, 500)]
    bufs += [b"\x00" * n for n in (1, 2, 3, 4, 64, 65, 1000, 65537)]
    bufs.append(bytes(range(256)) * 30)
    # the bucket adversary, 8 KiB: 1,638 positions share the prefix "xyz" and all differ within the two
    # bytes after it, so every chain is walked to its end and no run goes past 4
    bufs.append(b"".join(b"xyz" + bytes((i & 0xFF, i >> 8)) for i in range(8192 // 5)))
    # two prefixes in one bucket of the kernel's hash, interleaved: each one's chain holds the other's positions
    a, b = colliding_trigrams()
    bufs.append(b"".join((a if i % 2 else b) + rng.randbytes(2) for i in range(400)) + a + b + a)
    bufs.append(b"".join((a, b, a + a, b + a)[rng.randrange(4)] + rng.randbytes(1) for i in range(600)))
    return bufs


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


@functools.lru_cache(maxsize=None)
def reuse_items():
    """300 streams for one wave, each kind after the one whose leftovers would change it: long and
    repetitive (head table, ring, carried parse position, histograms full), then empty, 1 byte, 2 bytes,
    random."""
    rng = random.Random(0x2E05E)
    items = []
    for k in range(60):
        words = [rng.randbytes(rng.randrange(3, 9)) for _ in range(12)]
        long_rep = b"".join(rng.choice(words) for _ in range(rng.randrange(200, 500))) + b"\x07" * rng.randrange(0, 600)
        for buf in (long_rep, b"", rng.randbytes(1), words[0][:2], rng.randbytes(rng.randrange(3, 400))):
            items.append((buf, (RAW, ZLIB, GZIP)[rng.randrange(3)], (NONE, CRC32, ADLER32)[rng.randrange(3)]))
    return items


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
    caps = [0, 1, R - 1, R]
    items, cl = [], []
    for cap in caps:
        items += [(left, GZIP, NONE), (mid, fmt, CRC32), (right, RAW, ADLER32)]
        cl += [len(member(left, GZIP, DEFAULT)[0]), cap, len(member(right, RAW, DEFAULT)[0])]
    res = run_check(ctx, items, DEFAULT, "capacity", caps=cl)
    for k, cap in enumerate(caps):
        assert res[3 * k + 1][0] == (0 if cap >= R else E_CAPACITY) and res[3 * k + 1][2] == R
        assert res[3 * k][0] == 0 and res[3 * k + 2][0] == 0


def layout_items():
    rng = random.Random(77)
    items = []
    for k, n in enumerate([0, 1, 2, 3, 5, 15, 16, 17, 40, 63, 64, 65, 258, 700, 1025, 3000] * 2):
        buf = mixed(rng, n) if k % 2 else salad(rng, n)
        items.append((buf, (RAW, ZLIB, GZIP, RAW)[k % 4], (NONE, CRC32, ADLER32, CRC32, ADLER32)[k % 5]))
    return items


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_touching_regions_at_every_alignment(ctx, shift):
    """All three formats and both sums for RAW, regions that touch, `out` shifted by 0..3 bytes and the
    first region by 0..3 more."""
    items = layout_items()
    for pad in range(4):
        regions, off = [], pad
        for buf, fmt, _ in items:
            n = len(member(buf, fmt, DEFAULT)[0])
            regions.append((off, n))
            off += n
        res, out, _ = run(ctx, items, DEFAULT, regions=regions, out_size=off + 5, out_shift=shift)
        check(items, DEFAULT, res, out, regions, f"shift {shift} pad {pad}")


def test_device_pointers_on_the_callers_stream(ctx):
    """Input and output are torch tensors; the input is produced by a torch kernel on the current stream
    immediately before the call, with no synchronize, and the output is read by torch right after."""
    import torch
    import ndfl
    items = reuse_items()[:60] + layout_items()
    host_res, host_out, regions = run(ctx, items, DEFAULT)
    check(items, DEFAULT, host_res, host_out, regions, "host")
    packed, offs = pack_inputs(items)
    recs = [(io, len(buf), o, c, fmt, kind) for (buf, fmt, kind), io, (o, c) in zip(items, offs, regions)]
    n = len(packed)
    masked = torch.frombuffer(bytearray(bytes(x ^ 0x5A for x in packed)), dtype=torch.uint8).cuda()
    for shift in (0, 1):
        d_out = torch.full((len(host_out) + shift,), FILL, dtype=torch.uint8, device="cuda")
        d_in = torch.empty(n + shift, dtype=torch.uint8, device="cuda")
        d_in[shift:] = torch.bitwise_xor(masked, 0x5A)             # queued on the current stream, not waited for
        res = ctx.deflate_batch_lz77_raw(d_in.data_ptr() + shift, n, d_out.data_ptr() + shift, len(host_out), recs,
                                         *FULL_DYNAMIC, 65536, 32768, ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
        got = bytes(d_out.cpu().numpy())
        assert res == host_res, shift
        assert got[shift:] == host_out and got[:shift] == bytes([FILL]) * shift, shift
    assert ctx.last_kernel_ms() > 0


def test_arguments(ctx):
    import ndfl
    L = ndfl._lib.load()
    s = b"abcdef" * 10
    src = ctypes.create_string_buffer(s, len(s))
    out = ctypes.create_string_buffer(bytes([FILL]) * 256, 256)
    a_in, a_out = ctypes.addressof(src), ctypes.addressof(out)
    ok = (FULL_DYNAMIC, 65536, 32768)

    def raw(items, cfg, flags=0):
        return ctx.deflate_batch_lz77_raw(a_in, len(s), a_out, 256, items, *cfg[0], cfg[1], cfg[2], flags)

    assert raw([], ok) == []
    assert L.ndfl_deflate_batch_lz77(ctx._h, None, 0, None, 0, None, None, 0, 1, 3, 258, 1, 32768, 65536, 32768, 0) == 0
    assert out.raw == bytes([FILL]) * 256
    one = [(0, len(s), 0, 100, RAW, NONE)]
    res = (ndfl._lib.DeflateResult * 1)()
    arr = (ndfl._lib.MemberItem * 1)(ndfl._lib.MemberItem(*one[0]))
    before = bytes(res)
    for args in ((None, len(s), a_out, 256, arr, res), (a_in, len(s), None, 256, arr, res),
                 (a_in, len(s), a_out, 256, None, res), (a_in, len(s), a_out, 256, arr, None)):
        assert L.ndfl_deflate_batch_lz77(ctx._h, *args, 1, 1, 3, 258, 1, 32768, 65536, 32768, 0) == E_ARG
    cases = [(E_ARG, items, ok) for items in (
        [(0, len(s) + 1, 0, 100, RAW, NONE)], [(len(s) + 1, 0, 0, 100, RAW, NONE)], [(0, len(s), 200, 57, RAW, NONE)],
        [(0, len(s), 257, 0, RAW, NONE)], [(0, len(s), 0, 100, RAW, NONE), (0, len(s), 99, 100, RAW, NONE)],
        [(0, len(s), 50, 10, RAW, NONE), (0, len(s), 0, 100, RAW, NONE)], [(0, len(s), 1 << 63, 1 << 63, RAW, NONE)],
        [(0, len(s), 0, 100, 3, NONE)], [(0, len(s), 0, 100, RAW, 3)])]
    cases += [(E_ARG, one, (FULL_DYNAMIC, 0, 32768)), (E_UNSUPPORTED, one, (FULL_DYNAMIC, 65537, 32768)),
              (E_ARG, one, (FULL_DYNAMIC, 65536, 32769)), (E_ARG, one, ((True, 0, 0, 0, 0), 0, 32768)),
              (E_UNSUPPORTED, one, ((False, 3, 258, 1, 1), 65537, 32768))]
    # the six invalid tuples of test_gpu_lz77.py::test_invalid_parameters
    cases += [(E_ARG, one, (bad, 65536, 32768)) for bad in
              [(True, 2, 258, 1, 32768), (True, 3, 259, 1, 32768), (True, 5, 4, 1, 10), (True, 3, 258, 0, 10),
               (True, 3, 258, 1, 32769), (True, 3, 258, 10, 9)]]
    for code, items, cfg in cases:
        with pytest.raises(ndfl.NdflError) as e:
            raw(items, cfg)
        assert e.value.code == code, (items, cfg)
        assert out.raw == bytes([FILL]) * 256, (items, cfg)
    # the raw call leaves `results` untouched on an error
    assert L.ndfl_deflate_batch_lz77(ctx._h, a_in, len(s), a_out, 256, arr, res, 1, 1, 2, 258, 1, 32768, 65536, 32768, 0) == E_ARG
    assert L.ndfl_deflate_batch_lz77(ctx._h, a_in, len(s), a_out, 256, arr, res, 1, 1, 3, 258, 1, 32768, 0, 32768, 0) == E_ARG
    assert L.ndfl_deflate_batch_lz77(ctx._h, a_in, len(s), a_out, 256, arr, res, 1, 1, 3, 258, 1, 32768, 65537, 32768,
                                     0) == E_UNSUPPORTED
    assert bytes(res) == before and out.raw == bytes([FILL]) * 256
    # ndfl_deflate_batch itself still refuses the FULL_* presets
    with pytest.raises(ndfl.NdflError) as e:
        ctx.deflate_batch_raw(a_in, len(s), a_out, 256, one, "FULL_DYNAMIC", 65536, 32768, 0)
    assert e.value.code == E_UNSUPPORTED and out.raw == bytes([FILL]) * 256
    # regions that only touch, and an empty region inside another, are fine
    items = [(0, len(s), 0, 60, RAW, NONE), (0, len(s), 60, 60, RAW, NONE), (0, 0, 30, 0, RAW, NONE)]
    got = raw(items, ok)
    comp, bits = oracle(s)
    empty, ebits = oracle(b"")
    assert got == [(0, 0, len(comp), bits), (0, 0, len(comp), bits), (E_CAPACITY, 0, len(empty), ebits)]
    assert out.raw[:len(comp)] == comp and out.raw[60:60 + len(comp)] == comp
    assert out.raw[len(comp):60] == bytes([FILL]) * (60 - len(comp)) and out.raw[60 + len(comp):] == bytes([FILL]) * (196 - len(comp))


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
