"""The token-level stream writer and its reference expander (token_stream.py), pinned on the CPU before
any kernel sees the streams: for every family stream, expand() against the CPU oracle (bytes, Reason,
consumed bits) and against zlib, the tokens adversarial_hist.walk_blocks reads back against the tokens
written, and the seams against the walked block offsets."""
import zlib

import pytest

import adversarial_hist as A
import oracle_lib as O
import token_stream as T

NAMES = [n for f in T.FAMILIES for n in T.stream_names(f)]


def check_stream(comp, seams, blocks, kinds, reason, out):
    oreason, oout, obits = O.inflate(comp)
    assert oreason == reason
    assert oout == out
    has_reserved = any(t[0] == "R" for b in blocks for t in b)
    if reason is None:
        assert zlib.decompress(comp, -15) == out
    if has_reserved:
        with pytest.raises(ValueError, match="reserved length symbol"):
            A.walk_blocks(comp)
        return
    walked = A.walk_blocks(comp)
    assert [b["bit"] for b in walked] == seams
    assert [b["btype"] for b in walked] == [{"stored": 0, "fixed": 1, "dynamic": 2}[k] for k in kinds]
    assert [b["final"] for b in walked] == [0] * (len(blocks) - 1) + [1]
    if reason is None:
        assert obits == walked[-1]["end_bit"] and (obits + 7) // 8 == len(comp)   # the stream's length in bits
    for i, (b, toks) in enumerate(zip(walked, blocks)):
        if b["btype"] == 0:
            assert b["stored"] == bytes(t[1] for t in toks), i
        else:
            assert b["tokens"] == [t[1] if t[0] == "L" else (t[1], t[2]) for t in toks], i


@pytest.mark.parametrize("name", NAMES)
def test_family_stream(name):
    s = T.by_name(name)
    assert s.reason in (None, T.COPY_BEFORE)
    assert s.cases == sorted(s.cases, key=lambda c: c[0]) and s.cases[0][0] == 0
    check_stream(s.comp, s.seams, s.blocks, s.kinds, s.reason, s.out)


def test_stream_names_match_the_builders():
    for f in T.FAMILIES:
        assert [s.name for s in T.family(f)] == T.stream_names(f)


def test_family_b_edges_fall_on_every_bit_of_a_pend_word():
    """Family B steps its leading literals R through 0..31 from case to case instead of crossing R with
    every (P, F, d, l): what matters is where the pending run's two edges fall in a 32-byte pend group,
    and in every stream both edges must take all 32 positions, for the short and the long copies."""
    for s in T.family("B"):
        first, last = set(), set()
        for at, label in s.cases[1:]:
            _, p, f, d, length, r = label
            first.add(((at + r) % 32, length > 3))
            last.add(((at + r + p) % 32, length > 3))
        want = {(b, long) for b in range(32) for long in (False, True)}
        assert first == want and last == want, s.name


def test_family_a_covers_the_sweep():
    labels = {lab[1:] for s in T.family("A") if s.name.endswith("fixed") for _, lab in s.cases}
    assert labels == {(d, l, p) for d in range(1, 41) for l in T.A_LENS for p in range(17)}
    for s in T.family("A"):
        assert (s.name.endswith("mixed")) == ("stored" in s.kinds)


@pytest.mark.parametrize("distance", [7, 1, 32768])
def test_family_d(distance):
    """The depth family's expected bytes are tiled with numpy: expand() agrees at 64 KiB, and the 1 MiB
    stream (the same literals, more copies) continues the same bytes."""
    s, want = T.family_d(distance, 65536)
    assert T.expand(s.blocks) == (None, want)
    check_stream(s.comp, s.seams, s.blocks, s.kinds, None, want)
    big, want_big = T.family_d(distance)
    assert len(want_big) >= 1 << 20 and want_big[:len(want)] == want
    assert O.inflate(big.comp)[:2] == (None, want_big)
    assert zlib.decompress(big.comp, -15) == want_big
    assert [b["bit"] for b in A.walk_blocks(big.comp)] == big.seams
    if distance == 7:
        assert len(big.comp) < 2048                     # 1 MiB from under 2 KB


def test_family_f_ranges():
    cases = T.family_f_ranges()
    assert {c.dict_len for c in cases} == set(T.F_DICT_LENS)
    assert any(c.reason for c in cases) and any(c.reason is None for c in cases)
    for c in cases:
        oreason, oout, _ = O.inflate_range(c.comp, c.seams[c.k], None, c.window)
        assert (oreason, oout) == (c.reason, c.out), c.name
        assert len(c.window) == c.dict_len
        if c.reason:
            assert c.reason == T.COPY_BEFORE and len(c.out) == c.n, c.name
        walked = A.walk_blocks(c.comp)
        assert [b["bit"] for b in walked] == c.seams, c.name


def test_writer_edges():
    """The dynamic header's corners: an empty block (the end of block alone gets a second literal), one
    distance code (it gets a neighbour), no distance code, and a stored block between Huffman blocks."""
    blocks = [[], [("L", 5)], [("M", 3, 1)], [("L", 6), ("L", 7)], [("M", 258, 4), ("M", 4, 2)], []]
    kinds = ["dynamic", "dynamic", "dynamic", "stored", "dynamic", "dynamic"]
    comp, seams = T.stream(blocks, kinds)
    reason, out = T.expand(blocks)
    assert reason is None and out[:6] == bytes([5, 5, 5, 5, 6, 7])
    check_stream(comp, seams, blocks, kinds, reason, out)
    walked = A.walk_blocks(comp)
    assert walked[0]["lit_lens"][0] == 1 and walked[0]["lit_lens"][256] == 1
    assert sum(1 for l in walked[2]["dist_lens"] if l) == 2
    assert walked[1]["dist_lens"] == [0]


def test_expand_stops_at_the_dictionary_start():
    blocks = [[("L", 1), ("L", 2)], [("M", 3, 3), ("L", 9)]]
    assert T.expand(blocks) == (T.COPY_BEFORE, bytes([1, 2]))
    assert T.expand(blocks, b"\x07") == (None, bytes([1, 2, 7, 1, 2, 9]))
