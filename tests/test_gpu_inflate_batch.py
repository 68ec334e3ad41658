"""ndfl_inflate_batch on the GPU: many independent raw DEFLATE streams in one call, every stream's
status, error symbol, output bytes and end position against the CPU oracle on that stream alone
(O.inflate, O.error_symbol), and every byte of `out` outside the streams' stored bytes untouched.

The batch kernel (csrc/hip/inflate_batch.hip) decodes one stream per wave, serially, out of a 32 KiB
LDS ring; a wave takes stream after stream from a ticket.  The cases below are the places where that
can go wrong: neighbours in the input (a stream's last word holds the next stream's first bytes)
and in the output (regions that touch, odd alignments, every length around the 16-byte store and
the ring size), the dictionary start, copies of every period shape and a distance that wraps the
ring, codes longer than the primary tables, one wave reused for many unlike streams
(NDFL_BATCH_WAVES=1), more streams than waves, capacity overflow, and device pointers on the
caller's stream.
"""
import ctypes
import functools
import random
import zlib

import pytest

import adversarial_hist as A
import knobs
import oracle_lib as O
from test_gpu_long_codes import dynamic_block, long_lit_lens
from test_oracle_inflate import KAT, reserved_symbol_streams

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_ARG, E_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def ctx():
    import torch
    import ndfl
    c = ndfl.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)     # ordered with torch's kernels
    return c


@pytest.fixture(scope="module")
def one_wave():
    import torch
    c = knobs.context(NDFL_BATCH_WAVES=1)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@functools.lru_cache(maxsize=None)
def oracle(data):
    """(reason name, output, consumed bits, error symbol) of one stream alone, computed once."""
    r, out, bits = O.inflate(data)
    return r, out, bits, O.error_symbol()


def zraw(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    return co.compress(data) + co.flush()


def salad(rng, n):
    words = [rng.randbytes(rng.randrange(2, 9)) for _ in range(200)]
    return b"".join(rng.choice(words) for _ in range(n // 4 + 1))[:n]


def run(ctx, streams, regions=None, caps=None, out_size=None):
    """One ndfl_inflate_batch call on host buffers: the streams packed back to back (no gaps), `out`
    pre-filled with FILL.  regions: (out_off, out_cap) per stream; default: consecutive regions of
    caps[i] (default: the oracle's length + 8) bytes.  Returns (results, out bytes, regions)."""
    packed = b"".join(streams)
    if regions is None:
        regions, off = [], 0
        for i, s in enumerate(streams):
            cap = caps[i] if caps is not None else len(oracle(s)[1]) + 8
            regions.append((off, cap))
            off += cap
    if out_size is None:
        out_size = max([o + c for o, c in regions] + [1])
    items, in_off = [], 0
    for s, (o, c) in zip(streams, regions):
        items.append((in_off, len(s), o, c))
        in_off += len(s)
    src = ctypes.create_string_buffer(packed, max(1, len(packed)))
    out = ctypes.create_string_buffer(bytes([FILL]) * out_size, out_size)
    res = ctx.inflate_batch_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_size, items, 0)
    return res, out.raw, regions


def reason_of(code):
    return O.REASONS[code - 1] if code > 0 else None


def check(streams, res, out, regions, what=""):
    """Every stream against the oracle (a Reason wins over E_CAPACITY; the first min(out_len, cap)
    bytes are stored), and every other byte of `out` still FILL."""
    expect = bytearray(bytes([FILL]) * len(out))
    for i, (s, r, (off, cap)) in enumerate(zip(streams, res, regions)):
        oreason, oout, obits, osym = oracle(s)
        code, sym, olen, bits = r
        where = (what, i, len(s), off, cap)
        if oreason is None and len(oout) > cap:
            assert code == E_CAPACITY, where
        else:
            assert code >= 0 and reason_of(code) == oreason, (where, code, oreason)
        assert olen == len(oout), (where, olen, len(oout))
        if code == 0:
            assert bits == obits, where
        assert sym == (osym if code > 0 else -1), where
        n = min(len(oout), cap)
        expect[off:off + n] = oout[:n]
    if out != bytes(expect):
        bad = next(k for k in range(len(out)) if out[k] != expect[k])
        owner = [i for i, (off, cap) in enumerate(regions) if off <= bad < off + cap]
        raise AssertionError((what, "first wrong byte", bad, "region of stream", owner, out[bad], expect[bad]))


def run_check(ctx, streams, what="", **kw):
    res, out, regions = run(ctx, streams, **kw)
    check(streams, res, out, regions, what)
    return res


def test_known_answers_in_one_call(ctx):
    """All 39 KATs x the three paddings of O.bits_to_bytes: 117 streams back to back, one batch; per item
    what test_gpu_inflate.test_known_answer asserts (and the oracle's bytes for the failing ones)."""
    streams, kats = [], []
    for kat in KAT:
        rng = random.Random(kat["line"])
        for pad in range(3):
            streams.append(O.bits_to_bytes(kat["bits"], pad, rng))
            kats.append(kat)
    assert len(streams) == 117
    res, out, regions = run(ctx, streams)
    check(streams, res, out, regions, "kat")
    for kat, s, (code, sym, olen, bits), (off, cap) in zip(kats, streams, res, regions):
        if kat["expect_reason"] is None:
            assert code == 0 and out[off:off + olen] == bytes.fromhex(kat["expect_hex"]), kat["name"]
            assert (bits + 7) // 8 == len(s), kat["name"]
        else:
            assert reason_of(code) == kat["expect_reason"], kat["name"]


def test_reserved_symbols_per_stream(ctx):
    import ndfl
    good = O.deflate(b"abc")
    streams, want = [], []
    for name, data, _, reason, sym in reserved_symbol_streams():
        streams += [data, good]
        want += [(reason, sym), (None, -1)]
    res = run_check(ctx, streams, "reserved")
    for (reason, sym), r in zip(want, res):
        assert (reason_of(r[0]), r[1]) == (reason, sym)
        if reason:
            prefix = "Reserved run length symbol" if reason == "RESERVED_LENGTH_SYMBOL" else "Reserved distance symbol"
            e = ctx.data_format_error_for(r)
            assert isinstance(e, ndfl.DataFormatException) and str(e) == f"{prefix}: {sym}"


def test_truncated_stream_never_reads_its_neighbour(ctx):
    """s[:k] packed directly in front of a valid stream: the truncated one ends as the oracle ends it on
    s[:k] alone (its Reason, out_len and bytes), the valid one is unaffected."""
    rng = random.Random(3)
    streams = []
    for level in (0, 1, 6, 9):
        for n in (0, 1, 100, 5000):
            s = zraw(salad(rng, n), level)
            ks = sorted({0, 1, 2, 3, len(s) // 2, len(s) - 1} | {rng.randrange(len(s)) for _ in range(3)})
            for k in ks:
                if 0 <= k < len(s):
                    streams += [s[:k], s]
    res = run_check(ctx, streams, "truncated")
    assert all(r[0] == 0 for r in res[1::2])
    assert all(r[0] > 0 for r in res[0::2])


LENGTHS = [0, 1, 3, 15, 16, 17, 258, 32768, 32769, 70000]


def layout_streams():
    rng = random.Random(17)
    streams = [zraw(salad(rng, n), 6) for n in LENGTHS] + [O.deflate(salad(rng, n), "FULL_DYNAMIC") for n in LENGTHS]
    return streams


def shuffled_layout(streams, caps, seed):
    """Regions in shuffled order: some adjacent, some after 1..17-byte gaps; starts forced through odd,
    4k+3 and 16k+15 alignments."""
    rng = random.Random(seed)
    order = list(range(len(streams)))
    rng.shuffle(order)
    regions = [None] * len(streams)
    off = 1
    for j, i in enumerate(order):
        if j % 3 == 1:
            off += rng.randrange(1, 18)
        if j % 5 == 2:
            off += (3 - off) % 4                   # 4k + 3
        if j % 5 == 4:
            off += (15 - off) % 16                 # 16k + 15
        regions[i] = (off, caps[i])
        off += caps[i]
    assert any(o % 2 == 1 for o, _ in regions) and any(o % 4 == 3 for o, _ in regions)
    assert any(o % 16 == 15 for o, _ in regions)
    return regions, off + 19


def test_output_regions_are_exact(ctx):
    """out pre-filled with 0xA5; regions shuffled, adjacent ones with out_cap == the exact length: every
    region holds the oracle's bytes and every byte outside them is still 0xA5."""
    streams = layout_streams()
    caps = [len(oracle(s)[1]) for s in streams]
    for seed in (1, 2):
        regions, size = shuffled_layout(streams, caps, seed)
        res = run_check(ctx, streams, f"exact{seed}", regions=regions, out_size=size)
        assert all(r[0] == 0 for r in res)


def test_output_regions_with_errors_and_overflow(ctx):
    """The same layouts with error streams and E_CAPACITY streams mixed in."""
    rng = random.Random(23)
    streams = layout_streams()
    caps = [len(oracle(s)[1]) for s in streams]
    extra = []
    for s in streams[3:]:
        extra.append(s[:rng.randrange(1, len(s))])                  # truncated: UEOS part way
    bad = bytearray(streams[8])
    bad[len(bad) // 2] ^= 0x55
    extra.append(bytes(bad))
    streams = streams + extra
    caps = caps + [len(oracle(s)[1]) for s in extra]
    for i in range(0, len(caps), 3):                                # every third: too small by 1..40 (or to 0)
        caps[i] = max(0, caps[i] - rng.randrange(1, 41))
    for seed in (3, 4):
        regions, size = shuffled_layout(streams, caps, seed)
        res = run_check(ctx, streams, f"mixed{seed}", regions=regions, out_size=size)
        assert any(r[0] == E_CAPACITY for r in res) and any(r[0] > 0 for r in res)


def test_dictionary_starts_at_the_streams_own_output(ctx):
    """Fixed block: literal 'A', then length 3 at distance 2 -- one byte before the stream's own first
    byte, where the neighbour's output lies."""
    from test_oracle_inflate import MSB_LIT
    bits = "1" + "10" + MSB_LIT[65] + "0000001" + "00001" + "0000000"
    s = O.bits_to_bytes(bits)
    assert oracle(s)[0] == "COPY_FROM_BEFORE_DICTIONARY_START" and oracle(s)[1] == b"A"
    neighbour = O.deflate(b"A" * 40)
    res = run_check(ctx, [neighbour, s, neighbour, s], "dict", caps=[40, 16, 40, 16])
    assert reason_of(res[1][0]) == "COPY_FROM_BEFORE_DICTIONARY_START" and res[1][2] == 1


def copy_inputs():
    rng = random.Random(29)
    out = [b"x" * 258, b"q" + b"r" * 258 * 5, b"", b"z"]
    for p in (2, 3, 7, 63, 64, 65):
        unit = rng.randbytes(p)
        out.append(unit * (600 // p + 3))
        out.append(rng.randbytes(10) + unit * 3 + rng.randbytes(5) + unit * (300 // p + 2))
    # a distance of exactly 32768 in a stream longer than 32 KiB of output: the ring wraps
    head = rng.randbytes(300)
    out.append(head + rng.randbytes(32768 - 300) + head + rng.randbytes(50) + head[10:200])
    out.append(salad(rng, 300000))
    return out


def test_copies(ctx):
    streams = []
    for data in copy_inputs():
        for strat in ("FULL_DYNAMIC", "FULL_STATIC", "RLE_DYNAMIC", "RLE_STATIC"):
            streams.append(O.deflate(data, strat, 65536 if len(data) < 100000 else 50000))
    wrap = A.walk_blocks(O.deflate(copy_inputs()[-2], "FULL_DYNAMIC"))
    assert any(isinstance(t, tuple) and t[-1] == 32768 for b in wrap for t in b["tokens"])
    rng = random.Random(31)
    mixed = salad(rng, 65535 * 3 + 100)
    streams.append(O.deflate_mixed(mixed, ["UNCOMPRESSED", "RLE_STATIC", "FULL_DYNAMIC"], 65535))
    streams.append(O.deflate_mixed(mixed[:70000], ["FULL_DYNAMIC", "UNCOMPRESSED"], 700))
    # stored blocks of LEN 0 and LEN 65,535 around Huffman blocks (written by hand)
    st0 = b"\x00\x00\x00\xff\xff"
    big = rng.randbytes(65535)
    st_big = b"\x00\xff\xff\x00\x00" + big
    fixed = O.deflate(b"tail tail tail tail", "FULL_STATIC")
    streams.append(st0 + st_big + st0 + fixed)
    streams.append(st_big + st_big + b"\x01\x00\x00\xff\xff")
    res = run_check(ctx, streams, "copies")
    assert all(r[0] == 0 for r in res)


def test_ring_wrap_distance_32768(ctx):
    """A hand-made fixed-Huffman stream: 32,768 literals, then copies of length 258 at distance 32,768
    (the furthest the ring reaches) and at 32,768 - 100, 200 times over -- 84 KiB of output."""
    from test_oracle_inflate import MSB_LIT
    rng = random.Random(37)
    bits = ["1", "10"]
    for _ in range(32768):
        bits.append(MSB_LIT[rng.randrange(256)])
    for k in range(200):
        bits.append("11000101")                                       # length symbol 285: 258
        d = 32768 if k % 2 == 0 else 32768 - 100
        bits.append("11101" + format(d - 24577, "013b")[::-1])        # distance code 29 + 13 extra bits, LSB first
    bits.append("0000000")
    s = O.bits_to_bytes("".join(bits))
    r, out, _, _ = oracle(s)
    assert r is None and len(out) == 32768 + 200 * 258
    res = run_check(ctx, [s, O.deflate(b"n"), s], "wrap")
    assert all(r[0] == 0 for r in res)


def test_code_edges(ctx):
    """15-bit literal codes and 7-bit code-length codes (adversarial_hist), and codes far longer than
    the primary tables: second-level tables and the canonical slow path (test_gpu_long_codes)."""
    streams = []
    for cls in ("lit_limit", "cl_limit"):
        for case in A.cases(cls):
            mode, arg, chunk_len, hist = case.encode_args
            for way in (arg if mode == "preset" else [arg]):
                streams.append(O.deflate(case.data, way, chunk_len, hist) if isinstance(way, str)
                               else O.deflate_lz(case.data, *way, chunk_len, hist))
    lit = long_lit_lens()
    for seed, dist in ((7, list(range(1, 15)) + [15, 15] + [0] * 14),
                       (11, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12] + [0] * 17)):
        rng = random.Random(seed)
        for rep in range(2):
            comp = dynamic_block(lit, dist, rng)
            streams += [comp, b"\x00\x05\x00\xfa\xffhello" + comp]
    res = run_check(ctx, streams, "edges")
    assert all(r[0] == 0 for r in res)


def reuse_streams():
    rng = random.Random(41)
    dyn = [O.deflate(salad(rng, 3000 + 500 * k), "FULL_DYNAMIC") for k in range(4)]
    dyn.append(dynamic_block(long_lit_lens(), list(range(1, 15)) + [15, 15] + [0] * 14, random.Random(5), ntok=800))
    fixed = [O.deflate(salad(rng, 200 + k), "FULL_STATIC") for k in range(3)]
    stored = [O.deflate(rng.randbytes(1000), "UNCOMPRESSED"), b"\x01\x00\x00\xff\xff"]
    empty = [b"", b"\x03\x00"]
    errors = [d for _, d, _, _, _ in reserved_symbol_streams()] + [dyn[0][:len(dyn[0]) // 2], dyn[1][:40], b"\x07",
                                                                   b"\x00\x01\x00\x00\x00", fixed[0][:-3]]
    kinds = [dyn, fixed, stored, empty, errors]
    out = []
    for k in range(80):
        group = kinds[k % 5]
        out.append(group[(k // 5) % len(group)])
    return out


def test_wave_reuse(ctx, one_wave):
    """>= 64 unlike streams on ONE wave (NDFL_BATCH_WAVES=1): nothing of a stream's tables, code lengths,
    ring or pending literals reaches the next.  The default grid gives identical results."""
    streams = reuse_streams()
    assert len(streams) >= 64 and oracle(b"")[0] == "UNEXPECTED_END_OF_STREAM" and oracle(b"")[1] == b""
    r1, out1, regions = run(one_wave, streams)
    check(streams, r1, out1, regions, "one wave")
    r2, out2, _ = run(ctx, streams)
    assert r1 == r2 and out1 == out2


def test_more_streams_than_waves(ctx):
    rng = random.Random(43)
    streams = [zraw(salad(rng, rng.randrange(0, 301)), rng.choice((1, 6, 9))) for _ in range(5000)]
    for k in range(3):
        streams.insert(1000 + 1500 * k, zraw(salad(rng, (1 << 20) + 1000 * k), 6))
    res = run_check(ctx, streams, "many")
    assert all(r[0] == 0 for r in res)
    # input regions repeated: the same stream listed twice, with two output regions
    s = streams[1000]
    n = len(oracle(s)[1])
    src = ctypes.create_string_buffer(s, len(s))
    out = ctypes.create_string_buffer(2 * n + 7)
    res = ctx.inflate_batch_raw(ctypes.addressof(src), len(s), ctypes.addressof(out), 2 * n + 7,
                                [(0, len(s), n + 7, n), (0, len(s), 0, n)], 0)
    assert [r[0] for r in res] == [0, 0] and out.raw[:n] == oracle(s)[1] == out.raw[n + 7:]


def test_capacity(ctx):
    rng = random.Random(47)
    data = salad(rng, 5000)
    s = zraw(data)
    empty = b"\x03\x00"
    # a stream that overflows its region and THEN hits an error: the Reason, with the oracle's out_len
    late = zraw(salad(rng, 40000))
    late = late[:len(late) - 50]
    assert oracle(late)[0] == "UNEXPECTED_END_OF_STREAM" and len(oracle(late)[1]) > 1000
    streams = [s, empty, late, s]
    res = run_check(ctx, streams, "capacity", caps=[len(data) - 1, 0, 100, len(data)])
    assert res[0][0] == E_CAPACITY and res[0][2] == len(data)
    assert res[1][0] == 0 and res[1][2] == 0
    assert reason_of(res[2][0]) == "UNEXPECTED_END_OF_STREAM" and res[2][2] == len(oracle(late)[1])
    assert res[3][0] == 0


def test_python_batch_recovers_from_overflow(ctx):
    """Context.inflate_batch without caps: regions of 4 * len + 65536; a stream that needs more is run
    again alone with the size it reported."""
    big = bytes(400000)                                        # ~400 bytes compressed: overflows 4 * len + 65536
    streams = [zraw(b"hello " * 50), zraw(big, 9), b"\x03\x00", zraw(b"tail")[:-2], zraw(big + b"x", 9)]
    calls = []
    raw = ctx.inflate_batch_raw

    def spy(*a):
        calls.append(len(a[4]))
        return raw(*a)
    ctx.inflate_batch_raw = spy
    try:
        got = ctx.inflate_batch(streams)
    finally:
        del ctx.inflate_batch_raw
    assert calls == [5, 2]
    for s, (reason, out, bits) in zip(streams, got):
        oreason, oout, obits, _ = oracle(s)
        assert (reason.name if reason else None) == oreason and out == oout
        assert oreason is not None or bits == obits


def test_arguments(ctx):
    s = zraw(b"abcdef" * 10)
    src = ctypes.create_string_buffer(s, len(s))
    out = ctypes.create_string_buffer(bytes([FILL]) * 256, 256)
    L = __import__("ndfl")._lib.load()
    a_in, a_out = ctypes.addressof(src), ctypes.addressof(out)
    assert ctx.inflate_batch_raw(a_in, len(s), a_out, 256, [], 0) == []
    assert L.ndfl_inflate_batch(ctx._h, None, 0, None, 0, None, None, 0, 0) == 0
    for items in ([(0, len(s) + 1, 0, 100)], [(len(s) + 1, 0, 0, 100)], [(0, len(s), 200, 57)], [(0, len(s), 257, 0)],
                  [(0, len(s), 0, 100), (0, len(s), 99, 100)], [(0, len(s), 50, 10), (0, len(s), 0, 100)],
                  [(0, len(s), 0, 100), (1 << 63, 1 << 63, 100, 100)], [(0, len(s), 1 << 63, 1 << 63)]):
        with pytest.raises(__import__("ndfl").NdflError) as e:
            ctx.inflate_batch_raw(a_in, len(s), a_out, 256, items, 0)
        assert e.value.code == E_ARG, items
        assert out.raw == bytes([FILL]) * 256, items
    # regions that only touch, and empty regions inside another, are fine
    res = ctx.inflate_batch_raw(a_in, len(s), a_out, 256, [(0, len(s), 0, 60), (0, len(s), 60, 60), (0, 0, 30, 0)], 0)
    assert [r[0] for r in res] == [0, 0, 1] and out.raw[:120] == b"abcdef" * 20 and out.raw[120:] == bytes([FILL]) * 136


def test_device_pointers_on_the_callers_stream(ctx):
    """Input and output are torch tensors; the input is written by a torch kernel on the current stream
    with no host sync before the call.  IN_DEVICE | OUT_DEVICE with and without IN_PADDED equal the
    host-pointer run."""
    import torch
    import ndfl
    streams = reuse_streams()[:40] + layout_streams()
    host_res, host_out, regions = run(ctx, streams)
    check(streams, host_res, host_out, regions, "host")
    packed = b"".join(streams)
    items, in_off = [], 0
    for s, (o, c) in zip(streams, regions):
        items.append((in_off, len(s), o, c))
        in_off += len(s)
    n = len(packed)
    staged = torch.frombuffer(bytearray(packed), dtype=torch.uint8).pin_memory()
    for padded in (False, True):
        d_in = torch.full((n + ndfl.IN_PAD_BYTES + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        d_out = torch.full((len(host_out),), FILL, dtype=torch.uint8, device="cuda")
        d_in[:n].copy_(staged, non_blocking=True)              # queued on the current stream, not waited for
        d_in[n:].zero_()
        flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | (ndfl.IN_PADDED if padded else 0)
        res = ctx.inflate_batch_raw(d_in.data_ptr(), n, d_out.data_ptr(), len(host_out), items, flags)
        assert res == host_res, padded
        assert bytes(d_out.cpu().numpy()) == host_out, padded
    assert ctx.last_kernel_ms() > 0
