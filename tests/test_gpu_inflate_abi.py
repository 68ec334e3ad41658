"""The call frame of the inflate entry points at the C ABI (include/ndfl.h): ndfl_inflate, ndfl_inflate_range,
ndfl_inflate_sync, ndfl_inflate_headers, ndfl_inflate_resolve, ndfl_inflate_tail, ndfl_inflate_tail_map and
ndfl_bits_shift -- the counterpart of test_gpu_deflate_chunks_abi.py.

What the calls share around the decoder is pinned here, call by call: the return code of every argument rule of
csrc/capi/ndfl_capi.cpp (and that a refused call writes nothing), which rule wins where two are broken at once, the
state rules of the deferred-window decode (NDFL_E_STATE with none pending, a pending one dropped by the next decode, a
second resolve), where input and output may lie (host or device; device input read in place when it is padded and
16-byte aligned, staged otherwise) and in_len = 0.  The decoder's own output is pinned by the other decoder tests;
here every result is compared with the host-to-host call's, which those cover.

One stream of 12 dynamic blocks and a final fixed block (3,6xx bytes; link_geometry.pool_stream), each block copying
from the one before it, so that a range decode needs its window.
"""
import ctypes

import pytest

import link_geometry as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

B = G.pool_stream(12)
COMP = B.w.getbytes()
OUT = bytes(B.out)
BITS = B.end
K = 5                                           # the range decodes start at block 5's seam
START, WINDOW, TAIL = B.seams[K], OUT[:B.outs[K]], OUT[B.outs[K]:]
SENT = 0x5A5A5A5A5A5A5A5A                       # what an output word holds before a call
FILL = 0xEE
UEOS_CODE = O.REASONS.index("UNEXPECTED_END_OF_STREAM") + 1


@pytest.fixture(scope="module")
def ndfl():
    import ndfl as M
    return M


@pytest.fixture(scope="module")
def torch():
    import torch as T
    T.cuda.init()
    return T


@pytest.fixture(scope="module")
def ctx(ndfl, torch):                           # (torch's runtime first, as in test_gpu_deflate_chunks_abi.py)
    return ndfl.Context(0)


@pytest.fixture(scope="module")
def L(ndfl):
    return ndfl._lib.load()


class Frame:
    """Host buffers for one call: the input, an output pre-filled with 0xEE, the two result words."""

    def __init__(self, comp=COMP, cap=len(OUT) + 64, window=b""):
        self.src = ctypes.create_string_buffer(bytes(comp), max(1, len(comp)))
        self.out = ctypes.create_string_buffer(bytes(window) + bytes([FILL]) * cap, len(window) + cap)
        self.olen, self.bits = ctypes.c_uint64(SENT), ctypes.c_uint64(SENT)
        self.n, self.cap, self.dl = len(comp), cap, len(window)

    @property
    def inp(self):
        return ctypes.addressof(self.src)

    @property
    def outp(self):
        return ctypes.addressof(self.out)

    def untouched(self):
        return (self.olen.value, self.bits.value) == (SENT, SENT) and self.out.raw[self.dl:] == bytes([FILL]) * self.cap


def dev(torch, data, pad=0, skew=0):
    """data on the device, `pad` zero bytes behind it, starting `skew` bytes into a 256-byte aligned allocation."""
    t = torch.zeros(skew + len(data) + pad, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[skew:skew + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t


# ---- argument rules -----------------------------------------------------------------------------------------------
def test_inflate_argument_rules(ndfl, ctx, L):
    ref = ctypes.byref
    E = ndfl._lib.E_ARG
    ctx._order()
    f = Frame()
    assert L.ndfl_inflate(None, f.inp, f.n, f.outp, f.cap, ref(f.olen), ref(f.bits), 0) == E and f.untouched()
    assert L.ndfl_inflate(ctx._h, f.inp, f.n, f.outp, f.cap, None, ref(f.bits), 0) == E and f.untouched()
    assert L.ndfl_inflate(ctx._h, f.inp, f.n, f.outp, f.cap, ref(f.olen), None, 0) == E and f.untouched()
    assert L.ndfl_inflate(ctx._h, None, f.n, f.outp, f.cap, ref(f.olen), ref(f.bits), 0) == E and f.untouched()


RANGE_RULES = [
    ("null context", dict(ctx=None)),
    ("null out_len", dict(olen=None)),
    ("null consumed_bits", dict(bits=None)),
    ("null in with a length", dict(inp=None)),
    ("null out with dict_len", dict(outp=None, cap=0)),
    ("null out with out_cap", dict(outp=None, dl=0)),
    ("dict_len 32769", dict(dl=32769)),
    ("start_bit > 8 in_len", dict(start=8 * len(COMP) + 1)),
    ("end_bit == start_bit", dict(end=START)),
    ("end_bit < start_bit", dict(end=START - 1)),
    ("deferred without device output", dict(flags=4)),
    ("partial with deferred", dict(flags=16 | 4 | 2, end=G.NONE)),
    ("partial with a finite end_bit", dict(flags=16, end=B.seams[8])),
    # two rules at once: every argument rule is checked before the decode starts, so all of these are E_ARG as well
    ("dict_len 32769 and deferred without device output", dict(dl=32769, flags=4)),
    ("null out_len and partial with a finite end", dict(olen=None, flags=16, end=B.seams[8])),
]


@pytest.mark.parametrize("what,kw", RANGE_RULES, ids=[r[0] for r in RANGE_RULES])
def test_inflate_range_argument_rules(ndfl, ctx, L, what, kw):
    f = Frame(window=WINDOW)
    a = dict(ctx=ctx._h, inp=f.inp, n=f.n, start=START, end=G.NONE, outp=f.outp, dl=f.dl, cap=f.cap,
             olen=ctypes.byref(f.olen), bits=ctypes.byref(f.bits), flags=0)
    a.update(kw)
    ctx._order()
    r = L.ndfl_inflate_range(a["ctx"], a["inp"], a["n"], a["start"], a["end"], a["outp"], a["dl"], a["cap"], a["olen"],
                             a["bits"], a["flags"])
    assert r == ndfl._lib.E_ARG, what
    assert f.untouched() and f.out.raw[:f.dl] == WINDOW, what


def test_sync_and_headers_argument_rules(ndfl, ctx, L):
    ref = ctypes.byref
    E = ndfl._lib.E_ARG
    f = Frame()
    v = ctypes.c_uint64(SENT)
    ctx._order()
    assert L.ndfl_inflate_sync(None, f.inp, f.n, 0, 1 << 20, ref(v), 0) == E
    assert L.ndfl_inflate_sync(ctx._h, f.inp, f.n, 0, 1 << 20, None, 0) == E
    assert L.ndfl_inflate_sync(ctx._h, None, f.n, 0, 1 << 20, ref(v), 0) == E
    assert L.ndfl_inflate_sync(ctx._h, f.inp, f.n, 8 * f.n + 1, 1 << 20, ref(v), 0) == E
    assert v.value == SENT
    hs = (ctypes.c_uint64 * 64)(*[SENT] * 64)
    n = ctypes.c_uint64(SENT)
    assert L.ndfl_inflate_headers(None, f.inp, f.n, 0, hs, 64, ref(n), None, 0, None) == E
    assert L.ndfl_inflate_headers(ctx._h, f.inp, f.n, 0, hs, 64, None, None, 0, None) == E
    assert L.ndfl_inflate_headers(ctx._h, None, f.n, 0, hs, 64, ref(n), None, 0, None) == E
    assert L.ndfl_inflate_headers(ctx._h, f.inp, f.n, 0, None, 64, ref(n), None, 0, None) == E
    assert L.ndfl_inflate_headers(ctx._h, f.inp, f.n, 0, hs, 64, ref(n), None, 8, None) == E
    assert n.value == SENT and list(hs) == [SENT] * 64
    # the calls as they are meant: the chain starts are the non-final dynamic blocks' seams; the first confirmed
    # boundary from bit 1 is block 2's (the end of block 1's chain, a candidate whose own chain links on)
    assert L.ndfl_inflate_headers(ctx._h, f.inp, f.n, 0, hs, 64, ref(n), None, 0, None) == 0
    assert list(hs[:n.value]) == list(B.seams[:12]) == O.scan_headers(COMP)
    assert L.ndfl_inflate_sync(ctx._h, f.inp, f.n, 1, 1 << 20, ref(v), 0) == 0 and v.value == B.seams[2]


def test_bits_shift_argument_rules(ndfl, ctx, L, torch):
    E, C = ndfl._lib.E_ARG, ndfl._lib.E_CAPACITY
    D = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
    src = dev(torch, COMP[:64])
    dst = torch.full((128,), FILL, dtype=torch.uint8, device="cuda")
    host = ctypes.create_string_buffer(COMP[:64], 64)
    sp, dp = src.data_ptr(), dst.data_ptr()
    ctx._order()
    calls = [
        ("null context", (None, sp, 500, 3, dp, 128, D), E),
        ("null in with bits", (ctx._h, None, 500, 3, dp, 128, D), E),
        ("null out", (ctx._h, sp, 500, 3, None, 128, D), E),
        ("shift 8", (ctx._h, sp, 500, 8, dp, 128, D), E),
        ("host input", (ctx._h, ctypes.addressof(host), 500, 3, dp, 128, ndfl.OUT_DEVICE), E),
        ("host output", (ctx._h, sp, 500, 3, ctypes.addressof(host), 128, ndfl.IN_DEVICE), E),
        ("capacity", (ctx._h, sp, 500, 3, dp, 62, D), C),                     # (500 + 3 bits: 63 bytes)
        ("overlap", (ctx._h, sp, 500, 3, sp + 8, 128, D), E),
        # two rules at once
        ("capacity before overlap", (ctx._h, sp, 500, 3, sp + 8, 62, D), C),
        ("shift 8 before capacity", (ctx._h, sp, 500, 8, dp, 1, D), E),
        ("host pointers before capacity", (ctx._h, sp, 500, 3, dp, 1, 0), E),
    ]
    for what, args, code in calls:
        assert L.ndfl_bits_shift(*args) == code, what
    assert dst.cpu().numpy().tobytes() == bytes([FILL]) * 128 and src.cpu().numpy().tobytes() == COMP[:64]
    assert L.ndfl_bits_shift(ctx._h, sp, 500, 3, dp, 63, D) == 0
    want = (int.from_bytes(COMP[:64], "little") & ((1 << 500) - 1)) << 3
    assert dst[:63].cpu().numpy().tobytes() == want.to_bytes(63, "little")
    assert dst[63:].cpu().numpy().tobytes() == bytes([FILL]) * 65


# ---- the deferred decode's state -----------------------------------------------------------------------------------
def deferred_decode(ndfl, ctx, torch, write_window=True):
    """A deferred-window range decode from block K's seam into a device buffer; returns the buffer."""
    out = torch.full((len(WINDOW) + len(TAIL) + 64,), FILL, dtype=torch.uint8, device="cuda")
    src = dev(torch, COMP)
    r = ctx.inflate_range_raw(src.data_ptr(), len(COMP), START, None, out.data_ptr(), len(WINDOW), len(TAIL) + 64,
                              ndfl.IN_DEVICE | ndfl.OUT_DEVICE | ndfl.DICT_DEFERRED)
    assert r == (0, len(TAIL), BITS)
    if write_window:
        out[:len(WINDOW)] = torch.frombuffer(bytearray(WINDOW), dtype=torch.uint8).cuda()
    return out, src


def test_state_rules(ndfl, ctx, L, torch):
    S, E = ndfl._lib.E_STATE, ndfl._lib.E_ARG
    n = ctypes.c_uint64(SENT)
    dst = torch.full((4 * 64,), FILL, dtype=torch.uint8, device="cuda")

    def none_pending(what):
        ctx._order()
        assert L.ndfl_inflate_resolve(ctx._h, ctypes.byref(n)) == S and n.value == 0, what
        assert L.ndfl_inflate_tail(ctx._h, 16, dst.data_ptr()) == S, what
        assert L.ndfl_inflate_tail_map(ctx._h, 16, dst.data_ptr()) == S, what
        assert dst.cpu().numpy().tobytes() == bytes([FILL]) * 256, what

    assert ctx.inflate(COMP)[1] == OUT
    none_pending("after a plain decode")
    # the argument rules come before the state rule
    ctx._order()
    assert L.ndfl_inflate_resolve(ctx._h, None) == E and L.ndfl_inflate_resolve(None, ctypes.byref(n)) == E
    assert L.ndfl_inflate_tail(ctx._h, 16, None) == E and L.ndfl_inflate_tail(None, 16, dst.data_ptr()) == E
    assert L.ndfl_inflate_tail_map(ctx._h, 16, None) == E and L.ndfl_inflate_tail_map(None, 16, dst.data_ptr()) == E
    # a pending decode: tail and tail_map leave it pending, resolve ends it; a second resolve is NDFL_E_STATE
    out, src = deferred_decode(ndfl, ctx, torch)
    total = len(WINDOW) + len(TAIL)
    assert L.ndfl_inflate_tail(ctx._h, total + 1, dst.data_ptr()) == E      # more than window + output
    assert L.ndfl_inflate_tail(ctx._h, 0, None) == 0 and L.ndfl_inflate_tail_map(ctx._h, 0, None) == 0
    assert ctx.inflate_tail_raw(40, dst.data_ptr()) and dst[:40].cpu().numpy().tobytes() == OUT[-40:]
    assert ctx.inflate_tail_map_raw(40, dst.data_ptr())
    m = dst[:160].cpu().numpy().view("<u4")
    assert bytes((WINDOW[v] if v < len(WINDOW) else v & 0xFF) for v in m) == OUT[-40:]
    assert all(v < len(WINDOW) or v & ndfl._lib.TAIL_LITERAL for v in m)
    ctx.inflate_resolve()
    assert out[:total].cpu().numpy().tobytes() == OUT
    assert out[total:].cpu().numpy().tobytes() == bytes([FILL]) * 64
    dst.fill_(FILL)
    none_pending("after the resolve")
    # a pending decode is dropped by the next ndfl_inflate and by the next ndfl_inflate_range
    out, src = deferred_decode(ndfl, ctx, torch)
    assert ctx.inflate(COMP)[1] == OUT
    none_pending("dropped by ndfl_inflate")
    out, src = deferred_decode(ndfl, ctx, torch)
    plain = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
    plain[:len(WINDOW)] = out[:len(WINDOW)]
    r = ctx.inflate_range_raw(src.data_ptr(), len(COMP), START, None, plain.data_ptr(), len(WINDOW), len(TAIL) + 64,
                              ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
    assert r == (0, len(TAIL), BITS) and plain[:total].cpu().numpy().tobytes() == OUT
    none_pending("dropped by ndfl_inflate_range")
    # a call refused for its arguments leaves the pending decode as it was
    out, src = deferred_decode(ndfl, ctx, torch)
    f = Frame()
    ctx._order()
    assert L.ndfl_inflate_range(ctx._h, f.inp, f.n, 8 * f.n + 1, G.NONE, f.outp, 0, f.cap, ctypes.byref(f.olen),
                                ctypes.byref(f.bits), 0) == E
    assert ctx.inflate_resolve() >= 0
    assert out[:total].cpu().numpy().tobytes() == OUT
    none_pending("after the resolve")


# ---- placement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["inflate", "range"])
def test_placements_agree(ndfl, ctx, torch, call):
    """host / device input x host / device output; device input padded and aligned (read in place) and padded but one
    byte off the alignment (staged) -- all give the host-to-host call's result, and the input bytes are left as they
    were."""
    window, want = (b"", OUT) if call == "inflate" else (WINDOW, TAIL)
    dl, cap = len(window), len(want) + 64
    bits = BITS

    def run(in_ptr, out_ptr, flags):
        if call == "inflate":
            return ctx.inflate_raw(in_ptr, len(COMP), out_ptr, cap, flags)
        return ctx.inflate_range_raw(in_ptr, len(COMP), START, None, out_ptr, dl, cap, flags)

    f = Frame(cap=cap, window=window)
    assert run(f.inp, f.outp, 0) == (0, len(want), bits)
    ref = f.out.raw
    assert ref == window + want + bytes([FILL]) * 64
    inputs = {"host": (f.inp, 0, None),
              "device": (None, ndfl.IN_DEVICE, dev(torch, COMP)),
              "device padded aligned": (None, ndfl.IN_DEVICE | ndfl.IN_PADDED, dev(torch, COMP, ndfl.IN_PAD_BYTES)),
              "device padded off by one": (None, ndfl.IN_DEVICE | ndfl.IN_PADDED, dev(torch, COMP, ndfl.IN_PAD_BYTES, 1))}
    for iname, (ptr, iflags, t) in inputs.items():
        skew = 1 if iname.endswith("off by one") else 0
        if t is not None:
            ptr = t.data_ptr() + skew
            assert (ptr % 16 == 0) == (skew == 0)
            before = t.cpu().numpy().tobytes()
        for oname in ("host", "device"):
            if oname == "host":
                g = Frame(cap=cap, window=window)
                assert run(ptr, g.outp, iflags) == (0, len(want), bits), (iname, oname)
                got = g.out.raw
            else:
                o = torch.full((dl + cap,), FILL, dtype=torch.uint8, device="cuda")
                if dl:
                    o[:dl] = torch.frombuffer(bytearray(window), dtype=torch.uint8).cuda()
                assert run(ptr, o.data_ptr(), iflags | ndfl.OUT_DEVICE) == (0, len(want), bits), (iname, oname)
                got = o.cpu().numpy().tobytes()
            assert got == ref, (iname, oname)
        if t is not None:
            assert t.cpu().numpy().tobytes() == before, (iname, "input changed")
    assert f.src.raw[:len(COMP)] == COMP


# ---- in_len = 0 --------------------------------------------------------------------------------------------------------
def test_empty_input(ndfl, ctx, L, torch):
    """An empty input is a stream that ends before its first header: UNEXPECTED_END_OF_STREAM and nothing produced
    (the oracle's answer; consumed bits are compared nowhere for this Reason); no sync point, no headers; a shift of
    no bits writes nothing."""
    ref = ctypes.byref
    assert O.inflate(b"") == ("UNEXPECTED_END_OF_STREAM", b"", 0)
    for in_ptr in (None, "host"):
        f = Frame(comp=b"")
        p = f.inp if in_ptr else None
        ctx._order()
        assert L.ndfl_inflate(ctx._h, p, 0, f.outp, f.cap, ref(f.olen), ref(f.bits), 0) == UEOS_CODE
        assert f.olen.value == 0 and f.bits.value != SENT and f.out.raw == bytes([FILL]) * f.cap
        f = Frame(comp=b"")
        assert L.ndfl_inflate_range(ctx._h, p, 0, 0, G.NONE, f.outp, 0, f.cap, ref(f.olen), ref(f.bits), 0) == UEOS_CODE
        assert f.olen.value == 0 and f.bits.value != SENT and f.out.raw == bytes([FILL]) * f.cap
        v = ctypes.c_uint64(SENT)
        assert L.ndfl_inflate_sync(ctx._h, p, 0, 0, 1 << 20, ref(v), 0) == 0 and v.value == G.NONE
        n = ctypes.c_uint64(SENT)
        assert L.ndfl_inflate_headers(ctx._h, p, 0, 0, None, 0, ref(n), None, 0, None) == 0 and n.value == 0
    dst = torch.full((16,), FILL, dtype=torch.uint8, device="cuda")
    assert L.ndfl_bits_shift(ctx._h, None, 0, 0, dst.data_ptr(), 16, ndfl.IN_DEVICE | ndfl.OUT_DEVICE) == 0
    assert dst.cpu().numpy().tobytes() == bytes([FILL]) * 16
