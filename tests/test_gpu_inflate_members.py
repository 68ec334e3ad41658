"""ndfl_inflate_members on the GPU: many zlib members, gzip members and raw DEFLATE streams in one
call, the container header parsed, the output checksummed and the trailer compared in the launch that
decodes them.  Every stream's status, error symbol, output bytes, checksum, header length and end
position are checked against the CPU oracle on that stream alone (O.gunzip, O.zlib_decompress,
O.inflate, O.crc32, O.adler32), and every byte of `out` outside the streams' stored bytes stays
untouched.

The set-up is tests/test_gpu_inflate_batch.py's: items packed back to back with no gaps, `out`
pre-filled with 0xA5.  The cases are the places where the members kernel
(csrc/hip/inflate_batch_loop.inc with NDFL_BATCH_MEMBERS) can go wrong on top of the plain batch
kernel's: headers of every length (so the DEFLATE data starts at every byte alignment), the header
checks in the reference's order, truncation at every byte next to a neighbour's bytes, the trailer
checks and their precedence over NDFL_E_CAPACITY, the checksum over spans of every size the ring
flushes (Adler-32's worst case included), and the checksum state of one wave reused for unlike
streams.
"""
import ctypes
import functools
import gzip
import random
import zlib

import pytest

import knobs
import oracle_lib as O
from test_gpu_inflate_batch import (E_ARG, E_CAPACITY, FILL, layout_streams, reason_of, reuse_streams, salad,
                                    shuffled_layout, zraw)
from test_oracle_inflate import reserved_symbol_streams

pytestmark = pytest.mark.gpu

RAW, ZLIB, GZIP = 0, 1, 2
NONE, CRC32, ADLER32 = 0, 1, 2
HEADER_REASONS = {"GZIP_INVALID_MAGIC_NUMBER", "UNSUPPORTED_COMPRESSION_METHOD", "GZIP_RESERVED_FLAGS_SET",
                  "GZIP_UNSUPPORTED_OPERATING_SYSTEM", "HEADER_CHECKSUM_MISMATCH"}
MISMATCHES = {"DECOMPRESSED_CHECKSUM_MISMATCH", "DECOMPRESSED_SIZE_MISMATCH"}
UEOS = "UNEXPECTED_END_OF_STREAM"
ILLEGAL = "ERR-3"            # the oracle's IllegalArgumentException (zlib CINFO > 7): NDFL_E_ARG per stream


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


def gzip_header_len(m):
    """The length of a complete gzip header at the start of m, else None (layout only: no checks)."""
    try:
        flg, i = m[3], 10
        if flg & 4:
            i += 2 + (m[i] | m[i + 1] << 8)
        for bit in (8, 16):
            if flg & bit:
                i = m.index(0, i) + 1
        if flg & 2:
            i += 2
    except (IndexError, ValueError):
        return None
    return i if 10 <= i <= len(m) else None


def zlib_header_len(m):
    """The length of the zlib header ZlibMetadata.read accepts at the start of m, else None."""
    if len(m) < 2 or (m[0] << 8 | m[1]) % 31 or m[0] & 15 not in (8, 15):
        return None
    hl = 6 if m[1] & 0x20 else 2
    if len(m) < hl or (m[0] & 15 == 8 and m[0] >> 4 > 7):
        return None
    return hl


@functools.lru_cache(maxsize=None)
def oracle(fmt, kind, s, cap=None):
    """One item alone on the CPU: (reason name | None | ILLEGAL, output, consumed bits on success, checksum
    where the C ABI reports one else 0, header length, error symbol)."""
    reason, out, bits, value, hl = oracle_decode(fmt, kind, s, cap)
    # (the oracle's symbol is that of its last DEFLATE decode: read only where this item's decode set it)
    sym = O.error_symbol() if reason in ("RESERVED_LENGTH_SYMBOL", "RESERVED_DISTANCE_SYMBOL") else -1
    return reason, out, bits, value, hl, sym


def oracle_decode(fmt, kind, s, cap):
    if fmt == RAW:
        reason, out, bits = O.inflate(s, cap)
        value = {NONE: 0, CRC32: O.crc32(out), ADLER32: O.adler32(out)}[kind] if reason is None else 0
        return reason, out, bits, value, 0
    if fmt == GZIP:
        reason, out, _, end = O.gunzip(s, cap)
        hl = None if reason in HEADER_REASONS else gzip_header_len(s)
        value = O.crc32(out) if reason is None or reason in MISMATCHES else 0
        return reason, out, 8 * end, value, hl or 0
    reason, out = O.zlib_decompress(s, cap)
    hl = None if reason in HEADER_REASONS or reason == ILLEGAL else zlib_header_len(s)
    bits = 0
    if reason is None:
        bits = 8 * (hl + (O.inflate(s[hl:], cap)[2] + 7) // 8 + 4)
    value = O.adler32(out) if reason is None or reason in MISMATCHES else 0
    return reason, out, bits, value, hl or 0


def run(ctx, items, regions=None, caps=None, out_size=None, tails=None, hints=None):
    """One ndfl_inflate_members call on host buffers.  items: (stream, format, sum) packed back to back
    (tails[i]: bytes that follow item i in the buffer without belonging to it); `out` pre-filled with
    FILL.  regions: (out_off, out_cap) per item; default: consecutive regions of caps[i] (default: the
    oracle's length + 8) bytes.  hints[i]: an output capacity that is enough for the oracle.  Returns
    (results, out bytes, regions)."""
    hints = hints or [None] * len(items)
    if regions is None:
        regions, off = [], 0
        for i, (s, fmt, kind) in enumerate(items):
            cap = caps[i] if caps is not None else len(oracle(fmt, kind, s, hints[i])[1]) + 8
            regions.append((off, cap))
            off += cap
    if out_size is None:
        out_size = max([o + c for o, c in regions] + [1])
    packed, recs = bytearray(), []
    for i, ((s, fmt, kind), (o, c)) in enumerate(zip(items, regions)):
        recs.append((len(packed), len(s), o, c, fmt, kind))
        packed += s
        if tails is not None:
            packed += tails[i]
    packed = bytes(packed)
    src = ctypes.create_string_buffer(packed, max(1, len(packed)))
    out = ctypes.create_string_buffer(bytes([FILL]) * out_size, out_size)
    res = ctx.inflate_members_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_size, recs, 0)
    return res, out.raw, regions


def check(items, res, out, regions, what="", hints=None):
    """Every item against the oracle (a Reason or the per-stream E_ARG wins over E_CAPACITY; the first
    min(out_len, cap) bytes are stored), and every other byte of `out` still FILL."""
    hints = hints or [None] * len(items)
    expect = bytearray(bytes([FILL]) * len(out))
    for i, ((s, fmt, kind), r, (off, cap)) in enumerate(zip(items, res, regions)):
        oreason, oout, obits, ovalue, ohl, osym = oracle(fmt, kind, s, hints[i])
        code, sym, olen, bits, value, hl = r
        where = (what, i, fmt, kind, len(s), off, cap)
        if oreason == ILLEGAL:
            assert code == E_ARG, (where, code)
        elif oreason is None and len(oout) > cap:
            assert code == E_CAPACITY, (where, code)
        else:
            assert code >= 0 and reason_of(code) == oreason, (where, code, oreason)
        assert olen == len(oout), (where, olen, len(oout))
        if code == 0:
            assert bits == obits, (where, bits, obits)
        assert sym == (osym if code > 0 else -1), where
        assert value == ovalue, (where, hex(value), hex(ovalue))
        assert hl == ohl, (where, hl, ohl)
        n = min(len(oout), cap)
        expect[off:off + n] = oout[:n]
    if out != bytes(expect):
        bad = next(k for k in range(len(out)) if out[k] != expect[k])
        owner = [i for i, (off, cap) in enumerate(regions) if off <= bad < off + cap]
        raise AssertionError((what, "first wrong byte", bad, "region of item", owner, out[bad], expect[bad]))


def run_check(ctx, items, what="", **kw):
    res, out, regions = run(ctx, items, **kw)
    check(items, res, out, regions, what, kw.get("hints"))
    return res


def zhdr(cmf, flg_high):
    """A zlib header with FLG's upper three bits given and FCHECK made to fit."""
    flg = flg_high & 0xE0
    flg |= (31 - (cmf << 8 | flg) % 31) % 31
    return bytes([cmf, flg])


def zmember(body, data, cmf=0x78, flg_high=0x80, dictid=b""):
    return zhdr(cmf, flg_high) + dictid + body + O.adler32(data).to_bytes(4, "big")


MEMBER_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 5552, 5553, 32767, 32768, 32769, 70000]


@functools.lru_cache(maxsize=None)
def valid_members():
    """(item, data, header length) of every shape of member the issue lists."""
    rng = random.Random(53)
    out = []
    for n in MEMBER_LENGTHS:
        data = salad(rng, n)
        for level in (0, 1, 6, 9):
            out.append(((zlib.compress(data, level), ZLIB, NONE), data, 2))
        out.append(((O.zlib_compress(data), ZLIB, NONE), data, 2))
        for k in range(9):                      # no name, then names of 0..7 bytes: every alignment of the body
            name = None if k == 8 else bytes(rng.randrange(97, 123) for _ in range(k))
            crc, extra, comment = bool(k & 1), rng.randbytes(k + 1) if k & 2 else None, b"c" * (k % 3) if k & 4 else None
            g = O.gzip_compress(data, name=name, mtime=k * 1000, header_crc=crc, extra=extra, comment=comment)
            hl = (10 + (2 + len(extra) if extra is not None else 0) + (len(name) + 1 if name is not None else 0) +
                  (len(comment) + 1 if comment is not None else 0) + (2 if crc else 0))
            out.append(((g, GZIP, NONE), data, hl))
        g = gzip.compress(data, 6, mtime=0)     # Python writes OS byte 255
        assert g[9] == 255
        out.append(((g, GZIP, NONE), data, 10))
    return out


def test_valid_members_in_one_call(ctx):
    members = valid_members()
    items = [m[0] for m in members]
    hints = [len(m[1]) + 8 for m in members]
    assert {hl % 4 for _, _, hl in members} == {0, 1, 2, 3}
    caps = [len(m[1]) for m in members]
    regions, size = shuffled_layout(items, caps, 5)
    res, out, _ = run(ctx, items, regions=regions, out_size=size, hints=hints)
    check(items, res, out, regions, "valid", hints)
    for ((s, fmt, _), data, hl), r, (off, cap) in zip(members, res, regions):
        assert r[0] == 0 and r[2] == len(data) and out[off:off + cap] == data
        assert r[4] == (O.crc32(data) if fmt == GZIP else O.adler32(data))
        assert r[5] == hl and r[3] == 8 * len(s), (fmt, len(data), r, len(s))
        if fmt == GZIP:
            assert O.gunzip(s, len(data) + 8)[3] == len(s)


def test_concatenation_and_trailing_junk(ctx):
    rng = random.Random(59)
    a, b = salad(rng, 3000), salad(rng, 777)
    for fmt, first, second in ((GZIP, O.gzip_compress(a, name=b"one"), O.gzip_compress(b, header_crc=False)),
                               (ZLIB, zlib.compress(a, 6), b"junk after the member \x00\xff" * 3)):
        whole = first + second
        src = ctypes.create_string_buffer(whole, len(whole))
        out = ctypes.create_string_buffer(bytes([FILL]) * 4096, 4096)
        r = ctx.inflate_members_raw(ctypes.addressof(src), len(whole), ctypes.addressof(out), 4096,
                                    [(0, len(whole), 0, 4096, fmt, NONE)], 0)[0]
        assert r[0] == 0 and r[2] == len(a) and out.raw[:len(a)] == a and out.raw[len(a):] == bytes([FILL]) * (4096 - len(a))
        assert r[3] % 8 == 0 and r[3] // 8 == len(first)
        if fmt == GZIP:
            nxt = r[3] // 8
            r2 = ctx.inflate_members_raw(ctypes.addressof(src), len(whole), ctypes.addressof(out), 4096,
                                         [(nxt, len(whole) - nxt, 3000, 1000, fmt, NONE)], 0)[0]
            assert r2[0] == 0 and r2[2] == len(b) and out.raw[3000:3000 + len(b)] == b
            assert r2[3] // 8 == len(second) and r2[4] == O.crc32(b)


def test_truncation_never_reads_the_neighbour(ctx):
    """Every prefix m[:k] of a small gzip member and a small zlib member as an item, the bytes that would
    complete it directly behind it in the buffer: UNEXPECTED_END_OF_STREAM with the oracle's out_len."""
    gdata = b"truncate me, truncate me, truncate"
    zdata = gdata + bytes(range(40, 70))
    g = O.gzip_compress(gdata, name=b"nm", extra=b"xy", comment=b"c")
    z = zlib.compress(zdata, 9)
    assert 50 <= len(z) <= 70 and 50 <= len(g) <= 70
    items, tails = [], []
    for m, fmt in ((g, GZIP), (z, ZLIB)):
        for k in range(len(m)):
            items.append((m[:k], fmt, NONE))
            tails.append(m[k:])
    res = run_check(ctx, items, "truncated", tails=tails)
    assert all(reason_of(r[0]) == UEOS for r in res)
    assert res[len(g) - 1][2] == len(gdata) and res[-1][2] == len(zdata)    # k = len - 1: all bytes decoded


def header_cases():
    data = b"header checks " * 9
    g = bytearray(O.gzip_compress(data, name=b"name", header_crc=True))
    body = zraw(data)
    cases = []

    def gz(what, reason, **edit):
        m = bytearray(g)
        for pos, val in edit.items():
            m[int(pos[1:])] = val
        cases.append((what, (bytes(m), GZIP, NONE), reason))
    gz("magic", "GZIP_INVALID_MAGIC_NUMBER", b0=0x1E)
    gz("magic2", "GZIP_INVALID_MAGIC_NUMBER", b1=0x8C)
    gz("method 9", "UNSUPPORTED_COMPRESSION_METHOD", b2=9)
    gz("flag bit 5", "GZIP_RESERVED_FLAGS_SET", b3=g[3] | 0x20)
    gz("os 14", "GZIP_UNSUPPORTED_OPERATING_SYSTEM", b9=14)
    gz("os 255 under a header crc", "HEADER_CHECKSUM_MISMATCH", b9=255)
    gz("as written", None)
    cases.append(("zlib flg bit", (bytes([0x78, 0x9C ^ 0x40]) + body + O.adler32(data).to_bytes(4, "big"), ZLIB, NONE),
                  "HEADER_CHECKSUM_MISMATCH"))
    cases.append(("zlib method 9", (zmember(body, data, cmf=0x79), ZLIB, NONE), "UNSUPPORTED_COMPRESSION_METHOD"))
    cases.append(("zlib method 15", (zmember(body, data, cmf=0x7F), ZLIB, NONE), None))
    cases.append(("zlib fdict", (zmember(body, data, flg_high=0xA0, dictid=b"\x01\x02\x03\x04"), ZLIB, NONE), None))
    cases.append(("zlib fdict cut", (zhdr(0x78, 0xA0) + b"\x01\x02\x03", ZLIB, NONE), UEOS))
    cases.append(("zlib cinfo 8", (zmember(body, data, cmf=0x88), ZLIB, NONE), ILLEGAL))
    cases.append(("zlib cinfo 8, method 15", (zmember(body, data, cmf=0x8F), ZLIB, NONE), None))
    cases.append(("zlib 0 bytes", (b"", ZLIB, NONE), UEOS))
    cases.append(("zlib 1 byte", (b"\x78", ZLIB, NONE), UEOS))
    cases.append(("gzip 0 bytes", (b"", GZIP, NONE), UEOS))
    return cases, data


def test_header_reasons(ctx):
    cases, data = header_cases()
    items = [c[1] for c in cases]
    for what, (s, fmt, kind), reason in cases:
        assert oracle(fmt, kind, s)[0] == reason, what
    res = run_check(ctx, items, "headers")
    for (what, _, reason), r in zip(cases, res):
        if reason is None:
            assert r[0] == 0 and r[2] == len(data), what
        else:
            assert r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 0, what
            assert r[0] == (E_ARG if reason == ILLEGAL else O.REASONS.index(reason) + 1), what
    fdict = [r for (what, _, _), r in zip(cases, res) if what == "zlib fdict"][0]
    assert fdict[5] == 6


def test_trailer_reasons(ctx):
    rng = random.Random(61)
    data = salad(rng, 4000)
    g, z = O.gzip_compress(data), zlib.compress(data, 6)

    def flip(m, *at):
        m = bytearray(m)
        for k in at:
            m[k] ^= 0x10
        return bytes(m)
    cases = [((flip(g, -8), GZIP, NONE), "DECOMPRESSED_CHECKSUM_MISMATCH"),
             ((flip(g, -5), GZIP, NONE), "DECOMPRESSED_CHECKSUM_MISMATCH"),
             ((flip(g, -4), GZIP, NONE), "DECOMPRESSED_SIZE_MISMATCH"),
             ((flip(g, -1), GZIP, NONE), "DECOMPRESSED_SIZE_MISMATCH"),
             ((flip(g, -6, -2), GZIP, NONE), "DECOMPRESSED_CHECKSUM_MISMATCH"),     # both: the checksum is tested first
             ((flip(z, -4), ZLIB, NONE), "DECOMPRESSED_CHECKSUM_MISMATCH"),
             ((flip(z, -1), ZLIB, NONE), "DECOMPRESSED_CHECKSUM_MISMATCH"),
             ((g[:-1], GZIP, NONE), UEOS), ((z[:-1], ZLIB, NONE), UEOS), ((g, GZIP, NONE), None)]
    items = [c[0] for c in cases]
    res, out, regions = run(ctx, items)
    check(items, res, out, regions, "trailers")
    for (item, reason), r, (off, cap) in zip(cases, res, regions):
        assert reason_of(r[0]) == reason and r[2] == len(data) and out[off:off + len(data)] == data
        if reason in MISMATCHES:
            assert r[4] == (O.crc32(data) if item[1] == GZIP else O.adler32(data)) and r[3] == 0


def test_deflate_errors_inside_a_container(ctx):
    items, want = [], []
    for name, body, _, reason, sym in reserved_symbol_streams():
        items += [(zhdr(0x78, 0x80) + body + b"\0\0\0\1", ZLIB, NONE),
                  (O.gzip_compress(b"", header_crc=False)[:10] + body + bytes(8), GZIP, NONE)]
        want += [(reason, sym)] * 2
    rng = random.Random(67)
    data = salad(rng, 6000)
    z = bytearray(O.zlib_compress(data))
    z[len(z) // 2] ^= 0x55
    items.append((bytes(z), ZLIB, NONE))
    res = run_check(ctx, items, "deflate errors")
    for (reason, sym), r in zip(want, res):
        assert (reason_of(r[0]), r[1]) == (reason, sym) and r[4] == 0 and r[3] == 0
    assert res[-1][0] > 0 and oracle(ZLIB, NONE, bytes(z))[0] not in (None, UEOS)


def test_raw_with_a_checksum_equals_the_batch(ctx):
    streams = reuse_streams() + layout_streams()
    rng = random.Random(71)
    caps = [len(O.inflate(s)[1]) for s in streams]
    for i in range(0, len(caps), 4):                                # every fourth region too small
        caps[i] = max(0, caps[i] - rng.randrange(1, 41))
    regions, off = [], 0
    for c in caps:
        regions.append((off, c))
        off += c
    packed = b"".join(streams)
    recs, in_off = [], 0
    for s, (o, c) in zip(streams, regions):
        recs.append((in_off, len(s), o, c))
        in_off += len(s)
    src = ctypes.create_string_buffer(packed, len(packed))
    ref_out = ctypes.create_string_buffer(bytes([FILL]) * (off + 1), off + 1)
    ref = ctx.inflate_batch_raw(ctypes.addressof(src), len(packed), ctypes.addressof(ref_out), off + 1, recs, 0)
    assert any(r[0] == E_CAPACITY for r in ref) and any(r[0] > 0 for r in ref) and any(r[0] == 0 for r in ref)
    for kind in (CRC32, ADLER32, NONE):
        items = [(s, RAW, kind) for s in streams]
        res, out, _ = run(ctx, items, regions=regions, out_size=off + 1)
        check(items, res, out, regions, f"raw{kind}")
        assert [r[:4] for r in res] == ref and out == ref_out.raw
        for s, r in zip(streams, res):
            oout = O.inflate(s)[1]
            want = {NONE: 0, CRC32: O.crc32(oout), ADLER32: O.adler32(oout)}[kind] if r[0] in (0, E_CAPACITY) else 0
            assert r[4] == want and r[5] == 0


def test_capacity(ctx):
    rng = random.Random(73)
    data = salad(rng, 5000)
    g, z = O.gzip_compress(data, name=b"cap"), zlib.compress(data, 6)
    bad_g, bad_z = g[:-7] + bytes([g[-7] ^ 1]) + g[-6:], z[:-2] + bytes([z[-2] ^ 1]) + z[-1:]
    bad_size = g[:-3] + bytes([g[-3] ^ 1]) + g[-2:]
    items = [(g, GZIP, NONE), (z, ZLIB, NONE), (g, GZIP, NONE), (z, ZLIB, NONE), (zraw(data), RAW, CRC32),
             (bad_g, GZIP, NONE), (bad_z, ZLIB, NONE), (bad_size, GZIP, NONE), (g, GZIP, NONE)]
    caps = [len(data) - 1, len(data) - 1, 0, 0, 17, 100, 0, len(data) - 1, len(data)]
    res = run_check(ctx, items, "capacity", caps=caps)
    for r in res[:5]:
        assert r[0] == E_CAPACITY and r[2] == len(data)
    assert [r[4] for r in res[:5]] == [O.crc32(data), O.adler32(data), O.crc32(data), O.adler32(data), O.crc32(data)]
    # overflow AND a bad trailer: the mismatch Reason wins, the checksum is the computed one
    assert [reason_of(r[0]) for r in res[5:8]] == ["DECOMPRESSED_CHECKSUM_MISMATCH"] * 2 + ["DECOMPRESSED_SIZE_MISMATCH"]
    assert [r[4] for r in res[5:8]] == [O.crc32(data), O.adler32(data), O.crc32(data)] and all(r[2] == len(data) for r in res[5:8])
    assert res[8][0] == 0


def test_flush_spans_and_sum_overflow(ctx):
    """300,000 bytes of 0xFF (Adler-32's largest sums: every 32 KiB flush span at the maximum) and of
    text, stored (level 0) and compressed (level 9): many ring flushes per stream."""
    rng = random.Random(79)
    items, hints, datas = [], [], []
    for data in (b"\xff" * 300000, salad(rng, 300000)):
        for level in (0, 9):
            items += [(zlib.compress(data, level), ZLIB, NONE), (gzip.compress(data, level, mtime=0), GZIP, NONE),
                      (zraw(data, level), RAW, ADLER32), (zraw(data, level), RAW, CRC32)]
            hints += [len(data) + 8] * 4
            datas += [data] * 4
    res = run_check(ctx, items, "spans", hints=hints)
    for (s, fmt, kind), data, r in zip(items, datas, res):
        assert r[0] == 0 and r[2] == len(data)
        assert r[4] == (O.crc32(data) if fmt == GZIP or kind == CRC32 else O.adler32(data))


def reuse_items():
    """>= 64 unlike items for one wave: formats, sum kinds, header errors, trailer errors, DEFLATE errors
    and empty members in turn."""
    rng = random.Random(83)
    raws = reuse_streams()
    out = []
    for k in range(16):
        data = salad(rng, 50 + 700 * k)
        g = O.gzip_compress(data, name=bytes(rng.randrange(97, 123) for _ in range(k % 8)), header_crc=bool(k & 1))
        z = zlib.compress(data, (0, 1, 6, 9)[k % 4])
        out += [(g, GZIP, NONE), (raws[k], RAW, (CRC32, ADLER32, NONE)[k % 3]), (z, ZLIB, NONE),
                (raws[k + 16], RAW, (ADLER32, NONE, CRC32)[k % 3])]
        if k % 4 == 0:
            out += [(g[:3] + b"\xe0" + g[4:], GZIP, NONE), (z[:-1] + bytes([z[-1] ^ 8]), ZLIB, NONE),
                    (O.gzip_compress(b""), GZIP, NONE), (zlib.compress(b""), ZLIB, NONE)]
        if k % 4 == 1:
            out += [(g[:-8] + bytes(4) + g[-4:], GZIP, NONE), (b"\x78", ZLIB, NONE), (g[:len(g) // 2], GZIP, NONE),
                    (zhdr(0x88, 0x80) + z[2:], ZLIB, NONE)]
    return out


def test_wave_reuse(ctx, one_wave):
    """>= 64 unlike items on ONE wave (NDFL_BATCH_WAVES=1): nothing of an item's checksum state, format,
    header or tables reaches the next.  The default grid gives identical results."""
    items = reuse_items()
    assert len(items) >= 64
    r1, out1, regions = run(one_wave, items)
    check(items, r1, out1, regions, "one wave")
    codes = {r[0] for r in r1}
    assert 0 in codes and E_ARG in codes and len([c for c in codes if c > 0]) >= 4
    r2, out2, _ = run(ctx, items)
    assert r1 == r2 and out1 == out2


def test_more_streams_than_waves(ctx):
    rng = random.Random(89)
    datas = [salad(rng, rng.randrange(0, 301)) for _ in range(5000)]
    for k in range(3):
        datas.insert(1000 + 1500 * k, salad(rng, (1 << 20) + 1000 * k))
    items = [(zlib.compress(d, 6 if len(d) > 1000 else rng.choice((1, 6, 9))), ZLIB, NONE) for d in datas]
    hints = [len(d) + 8 for d in datas]
    res = run_check(ctx, items, "many", hints=hints)
    assert all(r[0] == 0 for r in res)
    assert all(r[2] == len(d) and r[3] == 8 * len(it[0]) for d, it, r in zip(datas, items, res))


def test_device_pointers_on_the_callers_stream(ctx):
    """Input and output are torch tensors; the input is written by a torch kernel on the current stream
    with no host sync before the call.  IN_DEVICE | OUT_DEVICE with and without IN_PADDED equal the
    host-pointer run."""
    import torch
    import ndfl
    items = reuse_items()[:48] + [m[0] for m in valid_members()[-40:]]
    host_res, host_out, regions = run(ctx, items)
    check(items, host_res, host_out, regions, "host")
    packed = b"".join(s for s, _, _ in items)
    recs, in_off = [], 0
    for (s, fmt, kind), (o, c) in zip(items, regions):
        recs.append((in_off, len(s), o, c, fmt, kind))
        in_off += len(s)
    n = len(packed)
    staged = torch.frombuffer(bytearray(packed), dtype=torch.uint8).pin_memory()
    for padded in (False, True):
        d_in = torch.full((n + ndfl.IN_PAD_BYTES + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        d_out = torch.full((len(host_out),), FILL, dtype=torch.uint8, device="cuda")
        d_in[:n].copy_(staged, non_blocking=True)              # queued on the current stream, not waited for
        d_in[n:].zero_()
        flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | (ndfl.IN_PADDED if padded else 0)
        res = ctx.inflate_members_raw(d_in.data_ptr(), n, d_out.data_ptr(), len(host_out), recs, flags)
        assert res == host_res, padded
        assert bytes(d_out.cpu().numpy()) == host_out, padded
    assert ctx.last_kernel_ms() > 0


def test_arguments(ctx):
    import ndfl
    s = zlib.compress(b"abcdef" * 10)
    src = ctypes.create_string_buffer(s, len(s))
    out = ctypes.create_string_buffer(bytes([FILL]) * 256, 256)
    L = ndfl._lib.load()
    a_in, a_out = ctypes.addressof(src), ctypes.addressof(out)
    assert ctx.inflate_members_raw(a_in, len(s), a_out, 256, [], 0) == []
    assert L.ndfl_inflate_members(ctx._h, None, 0, None, 0, None, None, 0, 0) == 0
    ok = (0, len(s), 0, 100, ZLIB, NONE)
    for items in ([(0, len(s), 0, 100, 3, NONE)], [(0, len(s), 0, 100, RAW, 3)], [ok, (0, len(s), 100, 100, ZLIB, 3)],
                  [ok, (0, len(s), 100, 100, 1 << 31, NONE)],
                  # the rules shared with ndfl_inflate_batch
                  [(0, len(s) + 1, 0, 100, ZLIB, NONE)], [(0, len(s), 200, 57, ZLIB, NONE)],
                  [ok, (0, len(s), 99, 100, ZLIB, NONE)], [(0, len(s), 1 << 63, 1 << 63, ZLIB, NONE)]):
        with pytest.raises(ndfl.NdflError) as e:
            ctx.inflate_members_raw(a_in, len(s), a_out, 256, items, 0)
        assert e.value.code == E_ARG, items
        assert out.raw == bytes([FILL]) * 256, items
    res = ctx.inflate_members_raw(a_in, len(s), a_out, 256, [ok, (0, len(s), 100, 60, ZLIB, ADLER32), (0, 0, 30, 0, GZIP, NONE)], 0)
    assert [r[0] for r in res] == [0, 0, 1] and out.raw[:60] == out.raw[100:160] == b"abcdef" * 10
    assert res[0][4] == res[1][4] == zlib.adler32(b"abcdef" * 10)


def test_python_members_recover_from_overflow(ctx):
    """Context.inflate_members without caps: regions of 4 * len + 65536; a member that needs more is run
    again alone with the size it reported (as test_python_batch_recovers_from_overflow checks the batch)."""
    import ndfl
    big = bytes(400000)                                        # ~400 bytes compressed: overflows 4 * len + 65536
    for fmt, pack in ((ndfl.FMT_ZLIB, lambda d: zlib.compress(d, 9)), (ndfl.FMT_GZIP, lambda d: gzip.compress(d, 9, mtime=0))):
        streams = [pack(b"hello " * 50), pack(big), pack(b""), pack(b"tail")[:-2], pack(big + b"x")]
        calls = []
        raw = ctx.inflate_members_raw

        def spy(*a):
            calls.append(len(a[4]))
            return raw(*a)
        ctx.inflate_members_raw = spy
        try:
            got = ctx.inflate_members(streams, fmt)
        finally:
            del ctx.inflate_members_raw
        assert calls == [5, 2]
        for s, (reason, out, bits, value, hl) in zip(streams, got):
            oreason, oout, obits, ovalue, ohl, _ = oracle(fmt, NONE, s, 400100)
            assert (reason.name if reason else None) == oreason and out == oout and value == ovalue and hl == ohl
            assert oreason is not None or bits == obits == 8 * len(s)
    # raw streams with a checksum, one format per stream, explicit capacities
    data = b"zip entry " * 30
    got = ctx.inflate_members([zraw(data), zlib.compress(data)], [ndfl.FMT_RAW, ndfl.FMT_ZLIB], sum=ndfl.SUM_CRC32,
                              out_caps=[300, 300])
    assert [g[0] for g in got] == [None, None] and got[0][1] == got[1][1] == data
    assert got[0][3] == zlib.crc32(data) and got[1][3] == zlib.adler32(data) and (got[0][4], got[1][4]) == (0, 2)
    with pytest.raises(ndfl.NdflError) as e:
        ctx.inflate_members([zlib.compress(data)], ndfl.FMT_ZLIB, out_caps=[299])
    assert e.value.code == E_CAPACITY
