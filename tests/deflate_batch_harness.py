"""What the GPU tests of the two batched deflate calls share (test_gpu_deflate_batch.py: ndfl_deflate_batch,
test_gpu_deflate_batch_lz.py: ndfl_deflate_batch_lz77): the constants, the fixtures, the input builders,
and one call / one check of a batch against a per-buffer oracle.

A test module gives run, check and run_check its own two functions:
    raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags) -> the entry point's results, one
        (status, checksum, out_len, end_bits) per stream;
    oracle(buf, *cfg) -> (DEFLATE bytes, end bits) of one buffer alone.
"""
import ctypes
import struct
import zlib

import pytest

import knobs

FILL = 0xA5
E_ARG, E_UNSUPPORTED, E_CAPACITY = -1, -2, -3
RAW, ZLIB, GZIP = 0, 1, 2
NONE, CRC32, ADLER32 = 0, 1, 2


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


def trailer(buf, fmt):
    if fmt == ZLIB:
        return struct.pack(">I", zlib.adler32(buf))
    if fmt == GZIP:
        return struct.pack("<II", zlib.crc32(buf), len(buf) & 0xFFFFFFFF)
    return b""


def checksum(buf, fmt, kind):
    kind = ADLER32 if fmt == ZLIB else CRC32 if fmt == GZIP else kind
    return {NONE: 0, CRC32: zlib.crc32(buf), ADLER32: zlib.adler32(buf)}[kind]


def member(oracle, buf, fmt, cfg):
    """(the member's bytes as the kernel writes them, end bits)."""
    comp, bits = oracle(buf, *cfg)
    return comp + trailer(buf, fmt), bits


def pack_inputs(items):
    """The items' buffers back to back (no gaps): (packed, [in_off])."""
    packed, offs = bytearray(), []
    for buf, _, _ in items:
        offs.append(len(packed))
        packed += buf
    return bytes(packed), offs


def run(raw, oracle, ctx, items, cfg, regions=None, caps=None, out_size=None, out_shift=0, inputs=None):
    """One batch call on host buffers.  items: (buffer, format, sum); cfg: the oracle's arguments after
    the buffer; regions: (out_off, out_cap) per item, default consecutive regions of caps[i] (default:
    the member's length) bytes, so that all regions touch.  `out` is pre-filled with FILL and starts
    out_shift bytes into its allocation.  inputs: (packed, [in_off]) instead of the items' buffers back
    to back.  Returns (results, out bytes, regions)."""
    if regions is None:
        regions, off = [], 0
        for i, (buf, fmt, _) in enumerate(items):
            cap = caps[i] if caps is not None else len(member(oracle, buf, fmt, cfg)[0])
            regions.append((off, cap))
            off += cap
    if out_size is None:
        out_size = max([o + c for o, c in regions] + [1])
    packed, offs = inputs if inputs is not None else pack_inputs(items)
    recs = [(io, len(buf), o, c, fmt, kind) for (buf, fmt, kind), io, (o, c) in zip(items, offs, regions)]
    src = ctypes.create_string_buffer(packed, max(1, len(packed)))
    out = ctypes.create_string_buffer(bytes([FILL]) * (out_size + out_shift), out_size + out_shift)
    res = raw(ctx, ctypes.addressof(src), len(packed), ctypes.addressof(out) + out_shift, out_size, recs, cfg, 0)
    assert out.raw[:out_shift] == bytes([FILL]) * out_shift
    return res, out.raw[out_shift:], regions


def check(oracle, items, cfg, res, out, regions, what=""):
    """Every stream against the oracle (the first min(out_len, cap) bytes are stored), the zero high
    bits of its last DEFLATE byte, and every other byte of `out` still FILL."""
    expect = bytearray(bytes([FILL]) * len(out))
    for i, ((buf, fmt, kind), r, (off, cap)) in enumerate(zip(items, res, regions)):
        exp, bits = member(oracle, buf, fmt, cfg)
        status, ck, olen, end_bits = r
        where = (what, cfg, i, len(buf), off, cap)
        assert status == (E_CAPACITY if len(exp) > cap else 0), (where, status)
        assert olen == len(exp), (where, olen, len(exp))
        assert end_bits == bits, (where, end_bits, bits)
        assert ck == checksum(buf, fmt, kind), (where, ck)
        last = exp[(bits + 7) // 8 - 1]
        assert bits % 8 == 0 or last >> (bits % 8) == 0, where
        n = min(len(exp), cap)
        expect[off:off + n] = exp[:n]
    if out != bytes(expect):
        bad = next(k for k in range(len(out)) if out[k] != expect[k])
        owner = [i for i, (off, cap) in enumerate(regions) if off <= bad < off + cap]
        raise AssertionError((what, cfg, "first wrong byte", bad, "region of stream", owner,
                              [len(items[i][0]) for i in owner], out[bad], expect[bad]))


def run_check(raw, oracle, ctx, items, cfg, what="", **kw):
    res, out, regions = run(raw, oracle, ctx, items, cfg, **kw)
    check(oracle, items, cfg, res, out, regions, what)
    return res


def salad(rng, n):
    words = [rng.randbytes(rng.randrange(2, 9)) for _ in range(200)]
    return b"".join(rng.choice(words) for _ in range(n // 4 + 1))[:n]


def mixed(rng, n):
    """Runs and text, with a run across every 64 KiB boundary."""
    b = bytearray()
    while len(b) < n:
        b += bytes([rng.randrange(4)]) * rng.randrange(1, 700) + salad(rng, rng.randrange(0, 400))
    b = b[:n]
    for k in range(65536, n, 65536):
        b[k - 300:min(n, k + 300)] = b"\x07" * (min(n, k + 300) - (k - 300))
    return bytes(b)
