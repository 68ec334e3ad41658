"""What the GPU tests of the four batched deflate calls share (test_gpu_deflate_batch.py: ndfl_deflate_batch,
test_gpu_deflate_batch_lz.py: ndfl_deflate_batch_lz77, test_gpu_deflate_batch_multi.py:
ndfl_deflate_batch_multi, test_gpu_deflate_batch_binsplit.py: ndfl_deflate_batch_binsplit): the constants,
the fixtures, the input builders, one call / one check of a batch against a per-buffer oracle, and the
scenarios that every call must pass in the same way (touching regions, device pointers, the argument
rules, the capacity layout).  No test module imports another for helpers: what two of them need is here.

A test module gives run, check, run_check and the scenarios its own functions:
    raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags) -> the entry point's results, one
        (status, checksum, out_len, end_bits) per stream (the Python wrapper: it raises NdflError);
    oracle(buf, *cfg) -> (DEFLATE bytes, end bits) of one buffer alone;
    c_call(ctx, in_addr, in_size, out_addr, out_size, items, results, n, cfg) -> the C entry point's
        return code, called directly with ctypes arrays (or None) -- for the argument rules only.
"""
import ctypes
import functools
import random
import struct
import types
import zlib

import pytest

import knobs
import oracle_lib as O

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


def raws(bufs):
    return [(b, RAW, NONE) for b in bufs]


# ---- the scenarios every batched deflate call passes in the same way --------------------------------
def touching_regions(raw, oracle, ctx, items, cfg, pads, shift):
    """Regions that touch, the first one `pad` bytes into `out` for every pad, `out` itself shift (or
    shift(pad)) bytes into its allocation: every stream against the oracle and every other byte still
    FILL.  Returns the residues mod 16 at which a region started."""
    seen = set()
    for pad in pads:
        regions, off = [], pad
        for buf, fmt, _ in items:
            n = len(member(oracle, buf, fmt, cfg)[0])
            regions.append((off, n))
            seen.add(off % 16)
            off += n
        s = shift(pad) if callable(shift) else shift
        res, out, _ = run(raw, oracle, ctx, items, cfg, regions=regions, out_size=off + 5, out_shift=s)
        check(oracle, items, cfg, res, out, regions, f"shift {s} pad {pad}")
    return seen


def device_pointers_on_the_callers_stream(raw, oracle, ctx, items, cfg):
    """Input and output are torch tensors; the input is produced by a torch kernel on the current stream
    immediately before the call, with no synchronize, and the output is read by torch right after."""
    import torch
    import ndfl
    host_res, host_out, regions = run(raw, oracle, ctx, items, cfg)
    check(oracle, items, cfg, host_res, host_out, regions, "host")
    packed, offs = pack_inputs(items)
    recs = [(io, len(buf), o, c, fmt, kind) for (buf, fmt, kind), io, (o, c) in zip(items, offs, regions)]
    n = len(packed)
    # the device input is computed on the GPU: the packed bytes XOR 0x5A, XORed back by a torch kernel
    masked = torch.frombuffer(bytearray(bytes(x ^ 0x5A for x in packed)), dtype=torch.uint8).cuda()
    for shift in (0, 1):                                           # `in` and `out` at an odd address too
        d_out = torch.full((len(host_out) + shift,), FILL, dtype=torch.uint8, device="cuda")
        d_in = torch.empty(n + shift, dtype=torch.uint8, device="cuda")
        d_in[shift:] = torch.bitwise_xor(masked, 0x5A)             # queued on the current stream, not waited for
        res = raw(ctx, d_in.data_ptr() + shift, n, d_out.data_ptr() + shift, len(host_out), recs, cfg,
                  ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
        got = bytes(d_out.cpu().numpy())
        assert res == host_res, shift
        assert got[shift:] == host_out and got[:shift] == bytes([FILL]) * shift, shift
    assert ctx.last_kernel_ms() > 0


def capacity_layout(raw, oracle, ctx, cfg, left, mid, right, fmt, caps):
    """left | mid (cap) | right for every cap in one call, all regions touching: mid's status, its
    out_len == the R bytes it needs whatever the cap, the stored prefix, and the neighbours bit-exact."""
    R = len(member(oracle, mid, fmt, cfg)[0])
    items, cl = [], []
    for cap in caps:
        items += [(left, GZIP, NONE), (mid, fmt, CRC32), (right, RAW, ADLER32)]
        cl += [len(member(oracle, left, GZIP, cfg)[0]), cap, len(member(oracle, right, RAW, cfg)[0])]
    res = run_check(raw, oracle, ctx, items, cfg, "capacity", caps=cl)
    for k, cap in enumerate(caps):
        assert res[3 * k + 1][0] == (0 if cap >= R else E_CAPACITY) and res[3 * k + 1][2] == R
        assert res[3 * k][0] == 0 and res[3 * k + 2][0] == 0


def argument_rules(raw, c_call, ctx, ok, own_cases):
    """The rules of the frame, with 60 input bytes and 256 output bytes: n == 0 looks at nothing; each of
    the four null pointers; the nine item rules (input and output bounds, overlapping regions, an offset
    that wraps, an unknown format, an unknown sum) under the good configuration `ok`; and the module's
    own_cases(one) -> [(code, items, cfg)], `one` a good item.  Every refused call is made twice, through
    the wrapper and directly with a result array of its own: the code, nothing written to `out`, the
    result array untouched.  Returns what the module's own checks after it need."""
    import ndfl
    s = b"abcdef" * 10
    src = ctypes.create_string_buffer(s, len(s))
    out = ctypes.create_string_buffer(bytes([FILL]) * 256, 256)
    a_in, a_out = ctypes.addressof(src), ctypes.addressof(out)
    assert raw(ctx, a_in, len(s), a_out, 256, [], ok, 0) == []
    assert c_call(ctx, None, 0, None, 0, None, None, 0, ok) == 0
    assert out.raw == bytes([FILL]) * 256
    one = [(0, len(s), 0, 100, RAW, NONE)]
    res = (ndfl._lib.DeflateResult * 1)()
    arr = (ndfl._lib.MemberItem * 1)(ndfl._lib.MemberItem(*one[0]))
    before = bytes(res)
    for args in ((None, len(s), a_out, 256, arr, res), (a_in, len(s), None, 256, arr, res),
                 (a_in, len(s), a_out, 256, None, res), (a_in, len(s), a_out, 256, arr, None)):
        assert c_call(ctx, *args, 1, ok) == E_ARG
    cases = [(E_ARG, items, ok) for items in (
        [(0, len(s) + 1, 0, 100, RAW, NONE)], [(len(s) + 1, 0, 0, 100, RAW, NONE)], [(0, len(s), 200, 57, RAW, NONE)],
        [(0, len(s), 257, 0, RAW, NONE)], [(0, len(s), 0, 100, RAW, NONE), (0, len(s), 99, 100, RAW, NONE)],
        [(0, len(s), 50, 10, RAW, NONE), (0, len(s), 0, 100, RAW, NONE)], [(0, len(s), 1 << 63, 1 << 63, RAW, NONE)],
        [(0, len(s), 0, 100, 3, NONE)], [(0, len(s), 0, 100, RAW, 3)])]
    cases += list(own_cases(one))
    for code, items, cfg in cases:
        with pytest.raises(ndfl.NdflError) as e:
            raw(ctx, a_in, len(s), a_out, 256, items, cfg, 0)
        assert e.value.code == code, (items, cfg)
        assert out.raw == bytes([FILL]) * 256, (items, cfg)
        # the same call with a result array of this test's: untouched too
        arr_k = (ndfl._lib.MemberItem * len(items))(*[ndfl._lib.MemberItem(*it) for it in items])
        res_k = (ndfl._lib.DeflateResult * len(items))()
        before_k = bytes(res_k)
        assert c_call(ctx, a_in, len(s), a_out, 256, arr_k, res_k, len(items), cfg) == code, (items, cfg)
        assert bytes(res_k) == before_k and out.raw == bytes([FILL]) * 256, (items, cfg)
    assert bytes(res) == before and out.raw == bytes([FILL]) * 256
    return types.SimpleNamespace(s=s, src=src, out=out, a_in=a_in, a_out=a_out, one=one)


def regions_that_only_touch(raw, oracle, ctx, ok, a):
    """After argument_rules (a: what it returned): regions that only touch, and an empty region inside
    another, are fine."""
    s, out = a.s, a.out
    items = [(0, len(s), 0, 60, RAW, NONE), (0, len(s), 60, 60, RAW, NONE), (0, 0, 30, 0, RAW, NONE)]
    got = raw(ctx, a.a_in, len(s), a.a_out, 256, items, ok, 0)
    comp, bits = oracle(s, *ok)
    empty, ebits = oracle(b"", *ok)
    assert got == [(0, 0, len(comp), bits), (0, 0, len(comp), bits), (E_CAPACITY, 0, len(empty), ebits)]
    assert out.raw[:len(comp)] == comp and out.raw[60:60 + len(comp)] == comp
    assert out.raw[len(comp):60] == bytes([FILL]) * (60 - len(comp)) and out.raw[60 + len(comp):] == bytes([FILL]) * (196 - len(comp))


# the six invalid Lz77Huffman tuples of test_gpu_lz77.py::test_invalid_parameters
BAD_TUPLES = [(True, 2, 258, 1, 32768), (True, 3, 259, 1, 32768), (True, 5, 4, 1, 10), (True, 3, 258, 0, 10),
              (True, 3, 258, 1, 32769), (True, 3, 258, 10, 9)]


# ---- what the three LZ modules share: ndfl_deflate_batch_lz77 itself and its inputs -------------------
FULL_DYNAMIC = (True, 3, 258, 1, 32768)
FULL_STATIC = (False, 3, 258, 1, 32768)


@functools.lru_cache(maxsize=None)
def lz_oracle(buf, params=FULL_DYNAMIC, chunk_len=65536, hist_limit=32768):
    """(DEFLATE bytes, end bits) of one buffer alone, computed once; the oracle's decoder gives the bits."""
    comp = O.deflate_lz(buf, *params, chunk_len, hist_limit)
    reason, back, bits = O.inflate(comp, out_cap=len(buf) + 64)
    assert reason is None and back == buf and (bits + 7) // 8 == len(comp)
    return comp, bits


def lz_raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_lz77; cfg: (params, chunk_len, hist_limit)."""
    params, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_lz77_raw(in_addr, in_size, out_addr, out_size, recs, *params, chunk_len, hist_limit, flags)


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


def chunk_edge_buffers():
    rng = random.Random(0xC4C4)
    bufs = [b for b in edge_buffers() if len(b) < 500][::9]
    # a 300-byte repeat that every chunk length below cuts, its source 500 before it; a long run of one byte
    bufs += [with_repeat(rng, 1300, 100, 600, 300), with_repeat(rng, 1300, 599, 600, 650),
             with_repeat(rng, 2100, 0, 1000, 1000), salad(rng, 1500), b"\x00" * 1100, b"ab" * 600]
    return bufs


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


def layout_items():
    """All three formats and both sums for RAW, at lengths around the lane, step and chunk edges."""
    rng = random.Random(77)
    items = []
    for k, n in enumerate([0, 1, 2, 3, 5, 15, 16, 17, 40, 63, 64, 65, 258, 700, 1025, 3000] * 2):
        buf = mixed(rng, n) if k % 2 else salad(rng, n)
        items.append((buf, (RAW, ZLIB, GZIP, RAW)[k % 4], (NONE, CRC32, ADLER32, CRC32, ADLER32)[k % 5]))
    return items
