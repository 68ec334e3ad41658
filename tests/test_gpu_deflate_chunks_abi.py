"""The call frame of the four chunked deflate entry points at the C ABI (include/ndfl.h):
ndfl_deflate_chunks, ndfl_deflate_chunks_lz77, ndfl_deflate_chunks_multi, ndfl_deflate_chunks_binsplit.

What the calls share around their encoders is pinned here, call by call: the return code of every
argument rule and which rule wins where two are broken at once, where the output lands (written in
place in the caller's device buffer, staged and copied device to device, staged and copied to the
host) and the capacity rule, device input with history, the CRC, and BinarySplit's partial final
chunk (the node-by-node path that owns temporary device buffers).  The encoders' own output is pinned
against the oracle by test_gpu_deflate.py, test_gpu_lz77.py and test_gpu_strategies.py; here every
result is compared with the same call made with host pointers, which those tests cover.

13,000 bytes in chunks of 4,096: three full chunks and a partial one.  One strategy per entry point.
"""
import ctypes
import random
import zlib

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

N, CHUNK = 13000, 4096
CALLS = ["chunks", "lz77", "multi", "binsplit"]
SEED_CRC = 0x12345678
BAD_TUPLE = (3, 2, 1, 1)                     # minRun > maxRun


def _corpus():
    rng = random.Random(20)
    parts = []
    for k in range(20):                      # 650-byte sections: runs, noise, runs, ...
        if k % 2:
            parts.append(rng.randbytes(650))
        else:
            sec = bytearray()
            while len(sec) < 650:
                sec += bytes([rng.randrange(4)]) * rng.choice([3, 40, 258, 300])
            parts.append(bytes(sec[:650]))
    return b"".join(parts)


DATA = _corpus()
HIST = random.Random(21).randbytes(60) + DATA[:1] * 40          # 100 bytes, ending in a run that DATA continues


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
def ctx(ndfl, torch):                        # (torch's runtime first, as in deflate_batch_harness.py)
    return ndfl.Context(0)


def _strategy(ndfl, call):
    """The strategy that reaches entry point `call` through Context.deflate_chunks_raw."""
    return {"chunks": "RLE_DYNAMIC",
            "lz77": ndfl.Lz77Huffman.FULL_DYNAMIC,
            "multi": ndfl.MultiStrategy(ndfl.Lz77Huffman.RLE_DYNAMIC, ndfl.Uncompressed.SINGLETON),
            "binsplit": ndfl.BinarySplit(ndfl.Lz77Huffman.RLE_DYNAMIC, 512)}[call]


def _desc(ndfl, kind=0, dynamic=1, tup=(3, 258, 1, 1)):
    return ndfl._lib.StrategyDesc(kind, dynamic, *tup)


def _raw(ndfl, ctx, call, mid=None, *, hist=None, hist_len=0, hist_limit=32768, data=DATA, n=None, chunk_len=CHUNK,
         final=1, start=0, out_cap=None, end_bits=True, crc=None, flags=0):
    """One entry point called directly, host pointers: (code, end_bits, output buffer).  `mid`: the
    call's own arguments between chunk_len and final_flag (default: _strategy's)."""
    L = ndfl._lib.load()
    n = len(data) if n is None else n
    keep = []
    if mid is None:
        if call == "chunks":
            mid = (3,)
        elif call == "lz77":
            mid = (1, 3, 258, 1, 32768)
        elif call == "multi":
            keep.append((ndfl._lib.StrategyDesc * 2)(_desc(ndfl), _desc(ndfl, kind=1, dynamic=0, tup=(0, 0, 0, 0))))
            mid = (keep[-1], 2)
        else:
            keep.append(_desc(ndfl))
            mid = (ctypes.byref(keep[-1]), 512)
    src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
    hb = ctypes.create_string_buffer(bytes(hist), max(1, len(hist))) if hist is not None else None
    cap = L.ndfl_deflate_bound(n, min(max(chunk_len, 1), 65536)) + 64 if out_cap is None else out_cap
    out = ctypes.create_string_buffer(max(1, cap))
    eb = ctypes.c_uint64(0)
    crcv = ctypes.c_uint32(crc or 0)
    ctx._order()
    fn = getattr(L, "ndfl_deflate_chunks" + ("" if call == "chunks" else "_" + call))
    r = fn(ctx._h, ctypes.addressof(hb) if hb is not None else None, hist_len, hist_limit, ctypes.addressof(src), n,
           chunk_len, *mid, final, start, ctypes.addressof(out), cap, ctypes.byref(eb) if end_bits else None,
           ctypes.byref(crcv) if crc is not None else None, flags)
    return r, eb.value, out


def _host(ndfl, ctx, call, data=DATA, hist=None, final=True, start=0, crc=None):
    """The reference result: (bytes, end_bits, crc), host input and host output."""
    L = ndfl._lib.load()
    cap = L.ndfl_deflate_bound(len(data), CHUNK) + 64
    out = ctypes.create_string_buffer(cap)
    src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
    hb = ctypes.create_string_buffer(bytes(hist)) if hist else None
    eb, c = ctx.deflate_chunks_raw(ctypes.addressof(hb) if hb else None, len(hist) if hist else 0, 32768,
                                   ctypes.addressof(src), len(data), CHUNK, _strategy(ndfl, call), final, start,
                                   ctypes.addressof(out), cap, 0, crc=crc)
    return out.raw[:(eb + 7) // 8], eb, c


@pytest.fixture(scope="module")
def reference(ndfl, ctx):
    """Per entry point: the whole corpus, final, from bit 0, host in and out."""
    return {call: _host(ndfl, ctx, call)[:2] for call in CALLS}


# ---- return codes ------------------------------------------------------------------------------

COMMON = [
    ("null out_end_bits", dict(end_bits=False), "E_ARG"),
    ("start_bitpos 8", dict(start=8), "E_ARG"),
    ("hist_limit 32769", dict(hist_limit=32769), "E_ARG"),
    ("hist_len > hist_limit", dict(hist=HIST, hist_len=100, hist_limit=99), "E_ARG"),
    ("chunk_len 0", dict(chunk_len=0), "E_ARG"),
    ("non-final, len % chunk_len != 0", dict(final=0), "E_ARG"),
    ("non-final, len 0", dict(final=0, n=0), "E_ARG"),
    ("chunk_len 65537", dict(chunk_len=65537), "E_UNSUPPORTED"),
]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("what,kw,code", COMMON, ids=[c[0] for c in COMMON])
def test_common_argument_rules(ndfl, ctx, call, what, kw, code):
    assert _raw(ndfl, ctx, call, **kw)[0] == getattr(ndfl._lib, code), (call, what)


def _precedence(ndfl):
    """(call, case, mid, keyword arguments, code): where two rules are broken, the one each call checks first."""
    D = ndfl._lib.StrategyDesc
    nine = (D * 9)(*[_desc(ndfl)] * 9)
    unknown = (D * 1)(_desc(ndfl, kind=7))
    stored = _desc(ndfl, kind=1, dynamic=0, tup=(0, 0, 0, 0))
    bad = _desc(ndfl, tup=BAD_TUPLE)
    ok = _desc(ndfl)
    ref = ctypes.byref
    return [
        ("chunks", "unknown strategy id, chunk_len 65537", (99,), dict(chunk_len=65537), "E_ARG"),
        ("lz77", "invalid tuple, chunk_len 65537", (1,) + BAD_TUPLE, dict(chunk_len=65537), "E_ARG"),
        ("multi", "n_strats 0", (nine, 0), {}, "E_ARG"),
        ("multi", "n_strats 9, start_bitpos 8", (nine, 9), dict(start=8), "E_UNSUPPORTED"),
        ("multi", "chunk_len 65537, unknown kind", (unknown, 1), dict(chunk_len=65537), "E_UNSUPPORTED"),
        ("multi", "unknown kind", (unknown, 1), {}, "E_ARG"),
        ("binsplit", "min_block_len 0", (ref(ok), 0), {}, "E_ARG"),
        ("binsplit", "Uncompressed substrategy", (ref(stored), 512), {}, "E_UNSUPPORTED"),
        ("binsplit", "Uncompressed substrategy, chunk_len 65537", (ref(stored), 512), dict(chunk_len=65537),
         "E_UNSUPPORTED"),
        ("binsplit", "invalid tuple", (ref(bad), 512), {}, "E_ARG"),
        ("binsplit", "chunk_len 10, min_block_len 1: an odd halving level", (ref(ok), 1), dict(chunk_len=10),
         "E_UNSUPPORTED"),
    ]


def test_precedence_of_the_calls_own_rules(ndfl, ctx):
    for call, what, mid, kw, code in _precedence(ndfl):
        assert _raw(ndfl, ctx, call, mid, **kw)[0] == getattr(ndfl._lib, code), (call, what)


def test_batched_lz_calls_reject_an_invalid_tuple(ndfl, ctx):
    """The Lz77Huffman parameter rule at its two batched sites."""
    L = ndfl._lib.load()
    src = ctypes.create_string_buffer(DATA)
    cap = L.ndfl_deflate_bound(N, CHUNK) + 64
    out = ctypes.create_string_buffer(cap)
    items = [(0, N, 0, cap, ndfl._lib.FMT_RAW, ndfl._lib.SUM_NONE)]
    args = (ctypes.addressof(src), N, ctypes.addressof(out), cap, items)
    with pytest.raises(ndfl._lib.NdflError) as e:
        ctx.deflate_batch_lz77_raw(*args, 1, *BAD_TUPLE, CHUNK, 32768, 0)
    assert e.value.code == ndfl._lib.E_ARG
    with pytest.raises(ndfl._lib.NdflError) as e:
        ctx.deflate_batch_multi_raw(*args, [_desc(ndfl), _desc(ndfl, tup=BAD_TUPLE)], CHUNK, 32768, 0)
    assert e.value.code == ndfl._lib.E_ARG


# ---- output placement --------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("shape", ["aligned, bound + 64", "one byte in", "exact size"])
def test_device_output_equals_host_output(ndfl, ctx, torch, reference, call, shape):
    L = ndfl._lib.load()
    exp, exp_bits = reference[call]
    size = L.ndfl_deflate_bound(N, CHUNK) + 64
    if shape == "exact size":
        size = len(exp)
    dev = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    skip = 1 if shape == "one byte in" else 0
    assert dev.data_ptr() % 4 == 0
    src = ctypes.create_string_buffer(DATA)
    eb, _ = ctx.deflate_chunks_raw(None, 0, 32768, ctypes.addressof(src), N, CHUNK, _strategy(ndfl, call), True, 0,
                                   dev.data_ptr() + skip, size - skip, ndfl.OUT_DEVICE)
    got = bytes(dev.cpu().numpy())
    assert eb == exp_bits
    assert got[skip:skip + len(exp)] == exp
    if skip:                                 # staged: exactly the stream's bytes are copied out
        assert got[:skip] == b"\xa5" and set(got[skip + len(exp):]) == {0xA5}


@pytest.mark.parametrize("call", CALLS)
def test_capacity_one_byte_short(ndfl, ctx, reference, call):
    exp, exp_bits = reference[call]
    r, eb, _ = _raw(ndfl, ctx, call, out_cap=len(exp) - 1)
    assert r == ndfl._lib.E_CAPACITY
    assert eb == exp_bits                    # the true end, so the caller can size the next try
    r, eb, out = _raw(ndfl, ctx, call, out_cap=len(exp))
    assert r == 0 and eb == exp_bits and out.raw[:len(exp)] == exp


# ---- device input with history -----------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
def test_device_input_with_history(ndfl, ctx, torch, call):
    """Non-final, three full chunks after 100 bytes of history, starting at bit 5: the RLE path reads
    the last history byte back, the others stage [history | data]."""
    import numpy as np
    L = ndfl._lib.load()
    data = DATA[:3 * CHUNK]
    exp, exp_bits, _ = _host(ndfl, ctx, call, data, HIST, final=False, start=5)
    assert exp_bits > 5 and exp[0] & 31 == 0
    dev = torch.from_numpy(np.frombuffer(HIST + data, dtype=np.uint8).copy()).cuda()
    cap = L.ndfl_deflate_bound(len(data), CHUNK) + 64
    out = ctypes.create_string_buffer(cap)
    eb, _ = ctx.deflate_chunks_raw(dev.data_ptr(), len(HIST), 32768, dev.data_ptr() + len(HIST), len(data), CHUNK,
                                   _strategy(ndfl, call), False, 5, ctypes.addressof(out), cap, ndfl.IN_DEVICE)
    assert eb == exp_bits
    assert out.raw[:(eb + 7) // 8] == exp


# ---- CRC ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
def test_crc_is_seeded(ndfl, ctx, reference, call):
    got, eb, crc = _host(ndfl, ctx, call, crc=SEED_CRC)
    assert crc == zlib.crc32(DATA, SEED_CRC)
    assert (got, eb) == reference[call]


@pytest.mark.parametrize("call", CALLS)
def test_crc_of_an_empty_final_call(ndfl, ctx, call):
    got, eb, crc = _host(ndfl, ctx, call, b"", crc=SEED_CRC)
    assert crc == SEED_CRC
    assert zlib.decompress(got, -15) == b""


# ---- BinarySplit: the partial final chunk ------------------------------------------------------

@pytest.mark.parametrize("sub", ["RLE_DYNAMIC", "FULL_DYNAMIC"])
@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK + 1])
def test_binsplit_partial_final_chunk(ndfl, ctx, sub, n):
    lz = getattr(ndfl.Lz77Huffman, sub)
    got = ctx.deflate(DATA[:n], ndfl.BinarySplit(lz, 64), chunk_len=CHUNK)
    assert got == O.deflate_binsplit(DATA[:n], (lz.useDynamicHuffmanCodes,) + lz.params, 64, CHUNK)
    assert zlib.decompress(got, -15) == DATA[:n]
