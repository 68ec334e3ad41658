"""The emit pass's one token walk (deflate_kernels.hip, MODE_EMIT): every lane packs its codes into a slot
of 18 words (576 bits) and the slots are compacted at the scanned bit offsets; a chunk in which some lane
has more bits than its slot holds takes the two walks instead (bit counts, then codes).

Every case compares three streams byte for byte and on their end bits: the CPU oracle's, the one-walk
run's (the default) and the run of a context created with NDFL_DEFLATE_ONEWALK=0.  Both contexts have
NDFL_STATS set, and the number of chunks that took two walks is read from the line the library prints
per call: "[ndfl] deflate emit: <n> chunks, <f> took two walks".

The inputs put single lanes over, exactly at and under the 576 bits (a lane carries the codes of the
pieces that start in its 64 bytes, the literal copies past its last byte included), leave lanes without
any bit, and walk the shapes of tests/test_gpu_deflate.py::inputs through the presets, chunk lengths,
history limits and start bit positions.
"""
import ctypes
import random
import re

import numpy as np
import pytest

import deflate_batch_harness as H
import knobs
import oracle_lib as O

pytestmark = pytest.mark.gpu

PRESETS = ["RLE_DYNAMIC", "RLE_STATIC", "LITERAL_DYNAMIC", "LITERAL_STATIC"]
STATS_LINE = re.compile(r"\[ndfl\] deflate emit: (\d+) chunks, (\d+) took two walks")


@pytest.fixture(scope="module")
def ctxs():
    """{1: the one-walk context (the default, set explicitly), 0: the two-walk context}."""
    return {k: knobs.context(NDFL_STATS=1, NDFL_DEFLATE_ONEWALK=k) for k in (1, 0)}


def emit_stats(capfd):
    """(chunks, two-walk chunks) of the calls since the last read, one pair per call."""
    return [(int(a), int(b)) for a, b in STATS_LINE.findall(capfd.readouterr().err)]


def both_equal_oracle(ctxs, capfd, data, strategy, chunk_len=65536):
    """deflate() of both contexts against the oracle; returns the one-walk run's (chunks, two walks)."""
    exp = O.deflate(data, strategy, chunk_len)
    nch = max(1, -(-len(data) // chunk_len))
    capfd.readouterr()
    got = ctxs[1].deflate(data, strategy, chunk_len=chunk_len)
    one = emit_stats(capfd)
    two_run = ctxs[0].deflate(data, strategy, chunk_len=chunk_len)
    two = emit_stats(capfd)
    assert got == exp, (strategy, len(data), "one walk")
    assert two_run == exp, (strategy, len(data), "two walks")
    assert len(one) == 1 and one[0][0] == nch, one
    assert two == [(nch, nch)], two                     # NDFL_DEFLATE_ONEWALK=0: every chunk
    return one[0]


# ---- 1. lane overflow under dynamic codes -----------------------------------------------------------
def ruler_with_rare_bytes():
    """131072 bytes, two chunks: byte i is the number of k in 1..9 with 2^k | (i + 1) (no two equal
    neighbours, geometric frequencies), then 64 different rare bytes on chunk 0's lane 500 and on chunk
    1's lane 7, whose last byte starts a piece of three equal bytes."""
    i1 = np.arange(1, 131073, dtype=np.int64)
    data = np.zeros(131072, dtype=np.uint8)
    for k in range(1, 10):
        data += (i1 % (1 << k) == 0).astype(np.uint8)
    data[32000:32064] = np.arange(100, 164, dtype=np.uint8)
    data[65536 + 448:65536 + 512] = np.arange(100, 164, dtype=np.uint8)
    data[65536 + 511:65536 + 514] = 200
    return data.tobytes()


@pytest.mark.parametrize("strategy", ["RLE_DYNAMIC", "LITERAL_DYNAMIC"])
def test_lane_overflow_under_dynamic_codes(ctxs, capfd, strategy):
    data = ruler_with_rare_bytes()
    assert len(data) == 131072 and data[:8] == bytes([0, 1, 0, 2, 0, 1, 0, 3])
    assert both_equal_oracle(ctxs, capfd, data, strategy) == (2, 2)


# ---- 2. the 576-bit edge under fixed codes ----------------------------------------------------------
def fixed_edge(extra):
    """One chunk of 8-bit literals (0..143) with lane 9's 64 bytes 9-bit literals (144..207); `extra`
    bytes from the lane's last one on are 250: a piece of 1 + ... equal bytes that starts on the lane."""
    data = bytearray((7 * i) % 144 for i in range(65536))
    data[576:640] = bytes(144 + j for j in range(64))
    if extra:
        data[639:639 + extra] = bytes([250]) * extra
    return bytes(data)


@pytest.mark.parametrize("extra,two_walks", [(0, 0), (2, 1), (3, 1)])
def test_slot_edge_under_fixed_codes(ctxs, capfd, extra, two_walks):
    """64 x 9 = 576 bits fill the slot exactly; 65 and 66 literals (585, 594 bits) pass it."""
    assert both_equal_oracle(ctxs, capfd, fixed_edge(extra), "RLE_STATIC") == (1, two_walks)


# ---- 3. lanes without a bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,two_walks", [("RLE_DYNAMIC", 0), ("RLE_STATIC", 1)])
def test_zero_bit_lanes(ctxs, capfd, strategy, two_walks):
    """65536 equal bytes: lane 0 carries every token (254 runs of 258: 13 bits each under the fixed
    codes, 2 under the dynamic ones), the 1023 other lanes none."""
    assert both_equal_oracle(ctxs, capfd, b"\x05" * 65536, strategy) == (1, two_walks)


# ---- 4. shapes ----------------------------------------------------------------------------------------
def shape_inputs():
    rng = random.Random(0x0E1)
    out = [b""]
    for n in [1, 63, 64, 65, 1000, 65535, 65537, 200003]:
        out.append(rng.randbytes(n))
        for lengths in ([1, 2, 3, 4], [100, 257, 258, 259, 600, 5000]):
            buf = bytearray()
            while len(buf) < n:
                buf += bytes([rng.randrange(3)]) * rng.choice(lengths)
            out.append(bytes(buf[:n]))
    return out


INPUTS = shape_inputs()


def shifted(comp, bits, start):
    """The oracle's stream (from bit 0) as bytes of a stream that starts at bit `start`."""
    return (int.from_bytes(comp, "little") << start).to_bytes((bits + start + 7) // 8, "little")


def raw_call(ctx, hist, data, strategy, chunk_len, hist_limit, start):
    """ndfl_deflate_chunks on host buffers, final; (the stream's bytes with the bits before `start`
    cleared, end bits)."""
    import ndfl
    cap = ndfl._lib.load().ndfl_deflate_bound(len(data), chunk_len) + 16
    out = ctypes.create_string_buffer(cap)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    hb = ctypes.create_string_buffer(hist, max(1, len(hist)))
    end, _ = ctx.deflate_chunks_raw(ctypes.addressof(hb) if hist else None, len(hist), hist_limit, ctypes.addressof(src),
                                    len(data), chunk_len, strategy, True, start, ctypes.addressof(out), cap, 0)
    got = bytearray(out.raw[:(end + 7) // 8])
    got[0] &= 0xFF & ~((1 << start) - 1)
    return bytes(got), end


@pytest.mark.parametrize("chunk_len", [64, 777, 4096, 65536])
@pytest.mark.parametrize("strategy", PRESETS)
def test_shapes(ctxs, strategy, chunk_len):
    for hist_limit in (0, 32768):
        for data in INPUTS:
            comp, bits = O.deflate_chunks(b"", data, True, strategy, chunk_len, hist_limit)
            for start in (0, 5):
                exp = (shifted(comp, bits, start), bits + start)
                for k in (1, 0):
                    got = raw_call(ctxs[k], b"", data, strategy, chunk_len, hist_limit, start)
                    assert got == exp, (strategy, chunk_len, hist_limit, start, len(data), "one walk" if k else "two walks")


@pytest.mark.parametrize("strategy", PRESETS)
def test_history_ends_with_the_first_byte(ctxs, strategy):
    """The first piece continues the history (lead 0): it is a run from its first byte on."""
    rng = random.Random(0x1EAD)
    for head in (1, 2, 3, 4, 70, 300):
        data = b"\x09" * head + rng.randbytes(500) + b"\x09" * 700
        hist = rng.randbytes(100) + b"\x09"
        for chunk_len in (64, 65536):
            comp, bits = O.deflate_chunks(hist, data, True, strategy, chunk_len, 32768)
            for start in (0, 5):
                exp = (shifted(comp, bits, start), bits + start)
                for k in (1, 0):
                    assert raw_call(ctxs[k], hist, data, strategy, chunk_len, 32768, start) == exp, (strategy, head, chunk_len, start, k)


# ---- 5. the segmented kernel --------------------------------------------------------------------------
def test_segmented_emit(ctxs):
    """One ndfl_deflate_batch_chunked call over five buffers, the lane-overflow input among ordinary
    ones: each stream is its own deflate() and the oracle's."""
    rle_dynamic = (True, 3, 258, 1, 1)
    cfg = (rle_dynamic, 65536, 32768)
    rng = random.Random(0x5E6)
    bufs = [H.mixed(rng, 70000), H.salad(rng, 1000), ruler_with_rare_bytes(), b"\x05" * 65536, H.mixed(rng, 65536 + 5)]
    items = H.raws(bufs)

    def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
        params, chunk_len, hist_limit = cfg
        return ctx.deflate_batch_chunked_raw(in_addr, in_size, out_addr, out_size, recs, *params, chunk_len, hist_limit, flags)

    for k in (1, 0):
        res = H.run_check(raw, H.lz_oracle, ctxs[k], items, cfg, "one walk" if k else "two walks")
        assert all(r[0] == 0 for r in res)
        for buf in bufs:
            assert ctxs[k].deflate(buf, "RLE_DYNAMIC") == H.lz_oracle(buf, *cfg)[0] == O.deflate(buf, "RLE_DYNAMIC")
