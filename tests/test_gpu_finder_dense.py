"""The header finder's dense scan (ndfl_inflate_find_compact_kernel), position for position.

Stage 1 of the finder tests every bit position of the stream with cheap masks and, for dynamic
headers, the Kraft sum of the code-length code; what it leaves (the survivors) goes to the strict
stage.  `ctx.inflate_headers(data, survivors=True)` returns both sets.  Here the survivor set is
compared with a numpy model of stage 1 written below, and the accepted set with the oracle's scan of
every bit position (or_scan_headers), on streams built to sit on the scan's edges:

    dense mask pattern  `24 49 92` repeated: the bits 001 at every third position, so 10-11 positions
                        of every word of every lane pass the cheap masks (more than any per-pass
                        take of the wave list up to 10), and none passes the Kraft test
    straddles           a real encoder header with HCLEN = 15 (74 bits) starting at bit 23..31 of the
                        last word of a wave, of a workgroup's span (16 and 64 words per thread), and
                        with its last words the input's last; ending exactly at the input's last bit,
                        and one bit past it
    stored offsets      LEN/NLEN = 0000/ffff in a zero stream at each byte offset of a word (every one
                        gives a stored header at each of the 8 bit phases before it), also crossing
                        into the next word, the next wave and the next workgroup
    config-4 mix        1 MiB compressed with RLE_DYNAMIC
    range               a range decode whose first and last bit fall inside a word takes exactly the
                        oracle's headers of that range as chain starts
"""
import ctypes

import numpy as np
import pytest

import corpus
import oracle_lib as O

pytestmark = pytest.mark.gpu

DYN = 1 << 63
SEG_BITS = 65536 * 8
SEG_CAP = 256


@pytest.fixture(scope="module")
def ctx():
    import ndfl
    return ndfl.Context(0)


def stage1_model(data):
    """The finder's stage 1 at every bit position of `data`: the set of survivors, as the library lists
    them (bit position, bit 63 set for a dynamic header)."""
    nbits = len(data) * 8
    b = np.concatenate([np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little"),
                        np.zeros(256, np.uint8)])         # (the finder reads zeros past the input)

    def field(pos, off, n):
        v = np.zeros(len(pos), np.int64)
        for i in range(n):
            v |= b[pos + off + i].astype(np.int64) << i
        return v

    P = np.arange(max(0, nbits - 2), dtype=np.int64)      # BFINAL and BTYPE inside the input
    P = P[b[P] == 0]                                       # BFINAL = 0
    # dynamic: BTYPE = 2, HLIT and HDIST < 30, the HCLEN + 4 lengths complete (Kraft sum 128/128) and
    # inside the input
    D = P[(b[P + 1] == 0) & (b[P + 2] == 1)]
    D = D[(field(D, 3, 5) < 30) & (field(D, 8, 5) < 30)]
    ncl = field(D, 13, 4) + 4
    kraft = np.zeros(len(D), np.int64)
    for i in range(19):
        l = field(D, 17 + 3 * i, 3)
        kraft += np.where((i < ncl) & (l > 0), 128 >> l, 0)
    D = D[(kraft == 128) & (D + 17 + 3 * ncl <= nbits)]
    # stored: BTYPE = 0, zero padding to the byte boundary, LEN = ~NLEN, the block inside the input
    S = P[(b[P + 1] == 0) & (b[P + 2] == 0)]
    al = (S + 3 + 7) & ~7
    pad = np.zeros(len(S), np.int64)
    for k in range(7):
        pad |= np.where(S + 3 + k < al, b[S + 3 + k], 0)
    ln, nl = field(al, 0, 16), field(al, 16, 16)
    S = S[(pad == 0) & ((ln ^ nl) == 0xFFFF) & (al + 32 + 8 * ln <= nbits)]
    return {int(p) | DYN for p in D} | {int(p) for p in S}


def check(ctx, data, model=None):
    """Survivors against the model, accepted headers against the oracle; returns (survivors, headers)."""
    got, stats, sv = ctx.inflate_headers(data, survivors=True)
    want = stage1_model(data) if model is None else model
    assert stats[3] == 0 and stats[0] == len(sv)
    assert len(set(sv)) == len(sv), "a survivor listed twice"
    lost, extra = sorted(want - set(sv)), sorted(set(sv) - want)
    assert not lost and not extra, (f"{len(lost)} survivors lost (first {[hex(x) for x in lost[:6]]}), "
                                    f"{len(extra)} extra (first {[hex(x) for x in extra[:6]]})")
    exp = O.scan_headers(data)
    assert max(np.bincount(np.array(exp, np.int64) // SEG_BITS), default=0) <= SEG_CAP
    assert got == exp
    assert set(got) <= {p & ~DYN for p in sv}
    return set(sv), got


# -- dense mask pattern ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [4 << 10, 1 << 20])
def test_dense_mask_pattern(ctx, size):
    data = (bytes.fromhex("244992") * (size // 3 + 1))[:size]
    w = np.frombuffer(data[:size & ~3], "<u4").astype(np.uint64)
    w = w[:-1] | (w[1:] << np.uint64(32))
    pm = ~w & ~(w >> np.uint64(1)) & (w >> np.uint64(2)) & np.uint64(0xFFFFFFFF)
    per_word = np.array([bin(int(x)).count("1") for x in pm[:4096]])
    assert per_word.min() == 10 and per_word.max() == 11   # every lane past a take of up to 10
    sv, got = check(ctx, data)
    assert not sv and not got


# -- one header with HCLEN = 15 across word, wave and workgroup edges ----------------------------------
@pytest.fixture(scope="module")
def hclen15_block():
    """The first bytes of an encoder block whose header has HCLEN = 15: byte frequencies along the
    Fibonacci numbers give literal code lengths up to 15, so the code-length code uses symbol 15, the
    last of the 19 in the header's order."""
    f = [1, 1]
    while len(f) < 23:
        f.append(f[-1] + f[-2])
    a = np.concatenate([np.full(c, 33 + i, np.uint8) for i, c in enumerate(f)])
    np.random.default_rng(1).shuffle(a)
    comp = O.deflate(a.tobytes(), "RLE_DYNAMIC")
    v = int.from_bytes(comp[:4], "little")
    assert v & 7 == 4 and (v >> 13) & 15 == 15            # BFINAL 0, BTYPE 2, HCLEN 15
    assert 0 in O.scan_headers(comp[:2048])               # the oracle accepts it with its lengths in reach
    return comp[:2048]


def shifted(block, pos, nbytes):
    """`nbytes` of zeros with the bits of `block` from bit `pos` on (cut at the end)."""
    return ((int.from_bytes(block, "little") << pos) & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")


@pytest.mark.parametrize("word", [5, 63, 700])
def test_header_behind_a_dense_word(ctx, hclen15_block, word):
    # The dense stream has no survivor, so it cannot show a list loop that drops the positions past a
    # pass's take.  Here the header stands at bit 29..31 of a word whose lower bits are the dense
    # pattern: at least 8 positions of the word pass the cheap masks before it, so it is the 9th or
    # later of its lane, and the lanes around it are as dense.
    size = 64 << 10
    dense = int.from_bytes((bytes.fromhex("244992") * (size // 3 + 1))[:size], "little")
    nb = 8 * len(hclen15_block)
    for off in (29, 30, 31):
        pos = 32 * word + off
        v = (dense & ~(((1 << nb) - 1) << pos)) | (int.from_bytes(hclen15_block, "little") << pos)
        data = v.to_bytes(size + len(hclen15_block) + 8, "little")[:size]
        W = int.from_bytes(data[4 * word:4 * word + 8], "little")
        big = ((W >> 4) & (W >> 5) & (W >> 6) & (W >> 7)) | ((W >> 9) & (W >> 10) & (W >> 11) & (W >> 12))
        pm = ~W & ~(W >> 1) & (W >> 2) & ~big & 0xFFFFFFFF
        assert pm >> off & 1 and bin(pm & ((1 << off) - 1)).count("1") >= 8
        sv, got = check(ctx, data)
        assert pos | DYN in sv, (word, off)


# the last word of the first wave, of a later wave, of a workgroup's span at 16 and at 64 words per thread
@pytest.mark.parametrize("word", [63, 255, 4095, 16383])
def test_header_straddles_words(ctx, hclen15_block, word):
    for off in range(23, 32):
        pos = 32 * word + off
        data = shifted(hclen15_block, pos, 4 * (word + 1) + len(hclen15_block) + 64)
        sv, got = check(ctx, data)
        assert pos | DYN in sv and pos in got, (word, off)


@pytest.mark.parametrize("word", [127, 4095])
def test_header_at_the_input_end(ctx, hclen15_block, word):
    # the 74 header bits end exactly at the input's last bit: bit 30 of `word`, three more words of input
    pos = 32 * word + 30
    data = shifted(hclen15_block, pos, (pos + 74) // 8)
    assert len(data) * 8 == pos + 74 and (len(data) + 3) // 4 == word + 4
    sv, got = check(ctx, data)
    assert pos | DYN in sv and not got
    # one bit later, the same input length: the last length's last bit is past the end
    pos += 1
    data = shifted(hclen15_block, pos, (pos + 73) // 8)
    assert len(data) * 8 == pos + 73
    sv, got = check(ctx, data)
    assert pos | DYN not in sv and not got


# -- stored headers -----------------------------------------------------------------------------------
def test_stored_header_offsets(ctx):
    # LEN = 0000 at byte a, NLEN = ffff: stored headers at the 8 bit positions 8a - 10 .. 8a - 3.  Byte
    # offsets 0..3 of a word inside a wave, at a wave's last word (LEN/NLEN in the next wave's words), at
    # the last word of a round of the workgroup and of its span (16 and 64 words per thread).
    for r in range(4):
        data = bytearray(4 * 16384 + 4096)
        at = [4 * w + r for w in (10, 63, 66, 255, 258, 4095, 4098, 16383)]
        for a in at:
            data[a + 2:a + 4] = b"\xff\xff"
        sv, got = check(ctx, bytes(data))
        for a in at:
            for p in range(8 * a - 10, 8 * a - 2):
                assert p in sv, (a, p)


def test_stored_block_inside_the_input_or_not(ctx):
    # LEN = 0100 (1 byte), NLEN = feff at byte 61: al + 32 + 8 must be inside the input
    for n, inside in ((66, True), (65, False)):
        data = bytearray(n)
        data[61:65] = bytes.fromhex("0100feff")
        sv, got = check(ctx, bytes(data))
        assert (8 * 61 - 3 in sv) == inside


# -- the config-4 mix ---------------------------------------------------------------------------------
def test_c4_mix(ctx):
    data = corpus.c4_mixed(1 << 20).numpy().tobytes()
    comp = O.deflate(data, "RLE_DYNAMIC")
    sv, got = check(ctx, comp)
    assert len(got) >= len(data) // 65536 - 2 and len(sv) > len(got)


# -- w_lo / scan_end ----------------------------------------------------------------------------------
def test_range_inside_words(ctx):
    """The library has no call that returns a range decode's chain starts (ndfl_inflate_headers scans a
    whole stream), so a range is checked by what it does expose: the decoded bytes and the number of
    chain starts the decode took, against the oracle's headers strictly inside the range.  One long
    range, and short ones of one to three blocks: a short range holds so few headers that one lost at
    the range's first or last word cannot be made up for by another."""
    chunk = 8192
    rng = np.random.default_rng(11)
    data = (rng.integers(0, 6, 1 << 20, dtype=np.uint8) * 9).tobytes()
    comp = O.deflate(data, "RLE_DYNAMIC", chunk_len=chunk)
    seams = [int(x) for x in np.cumsum(np.array(O.block_bits(data, "RLE_DYNAMIC", chunk), dtype=np.uint64))]
    headers = O.scan_headers(comp)
    # block k + 1 starts at seams[k]: a start and an end well inside a word
    inside = [k for k in range(len(seams) - 1) if 8 <= seams[k] % 32 <= 24]
    short = [(inside[k], inside[k + 1]) for k in range(4, len(inside) - 1, max(1, len(inside) // 8)) if inside[k + 1] - inside[k] <= 3]
    assert len(short) >= 4
    for a, b in [(inside[2], inside[-2])] + short:
        s_bit, e_bit = seams[a], seams[b]
        want = [p for p in headers if s_bit < p < e_bit]
        assert len(want) >= b - a - 1
        window = data[:(a + 1) * chunk][-32768:]
        oreason, oout, obits = O.inflate_range(comp, s_bit, e_bit, window)
        assert oreason is None and obits == e_bit and oout == data[(a + 1) * chunk:(b + 1) * chunk]
        hbuf = bytearray(window + bytes(len(oout) + 64))
        cbuf = (ctypes.c_uint8 * len(hbuf)).from_buffer(hbuf)
        cin = ctypes.create_string_buffer(comp, len(comp))
        r, olen, bits = ctx.inflate_range_raw(ctypes.addressof(cin), len(comp), s_bit, e_bit, ctypes.addressof(cbuf),
                                              len(window), len(oout) + 64, 0)
        assert (r, olen, bits) == (0, len(oout), e_bit)
        assert bytes(hbuf[len(window):len(window) + olen]) == oout
        # the chain starts: the range's first bit, then the accepted headers strictly inside the range
        assert int(ctx.timings()["inflate_candidates"]) == 1 + len(want), (a, b)
