"""Pins the CPU oracle's encoder.  The reference's own tests only round-trip the encoder
(T/DeflaterOutputStreamTest.java:109-115), so encoder bytes are pinned here by:
  (1) N-version agreement with tests/pyref_deflate.py (independent restatement, different algorithms),
  (2) the hand-derived known-answer tests of SURVEY.md App. A.8,
  (3) round-trip validity through Python zlib and through the oracle's own decoder,
  (4) equivalence of the exhaustive distance loop and the exact-prefix chain walk (FULL_*),
  (5) the same on the inputs of tests/adversarial_hist.py, which make the 15-bit and 7-bit length
      limits bind and reach the header's edge cases, each with its engagement condition asserted
      on the oracle's own stream (so a generator that stops reaching its edge fails here).
"""
import random
import zlib

import pytest

import adversarial_hist as A
import oracle_lib as O
import pyref_deflate as P


def samples(seed):
    rng = random.Random(seed)
    out = [b"", b"\x00", b"ab", b"aaa", b"\x00" * 5000, bytes(range(256)) * 3]
    for n in [7, 100, 1000, 3000]:
        out.append(bytes(rng.randrange(256) for _ in range(n)))
        out.append(bytes(rng.choice(b"ab") for _ in range(n)))
        buf = bytearray()
        while len(buf) < n:
            buf += bytes([rng.randrange(4)]) * rng.randrange(1, 300)
        out.append(bytes(buf[:n]))
        words = [b"the ", b"of ", b"deflate ", b"gpu ", b"xgmi ", b"\n"]
        out.append(b"".join(rng.choice(words) for _ in range(n // 4))[:n])
    return out


@pytest.mark.parametrize("strategy", list(P.PRESETS))
def test_nversion_presets(strategy):
    for i, data in enumerate(samples(1)):
        for chunk_len, hist in [(65536, 32768), (1000, 32768), (97, 1), (500, 0), (256, 100)]:
            if strategy.startswith("FULL") and len(data) > 1200:
                continue
            a = O.deflate(data, strategy, chunk_len, hist)
            b = P.deflate(data, strategy, chunk_len, hist)
            assert a == b, (strategy, i, chunk_len, hist)


def test_nversion_custom_lz_params():
    rng = random.Random(5)
    for _ in range(20):
        data = bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 900)))
        min_run = rng.randrange(3, 10)
        max_run = rng.randrange(min_run, 259)
        min_dist = rng.randrange(1, 20)
        max_dist = rng.randrange(min_dist, 400)
        dyn = rng.random() < 0.5
        a = O.deflate_lz(data, dyn, min_run, max_run, min_dist, max_dist, 300, 32768)
        b = P.deflate(data, chunk_len=300, params=(dyn, min_run, max_run, min_dist, max_dist))
        assert a == b


@pytest.mark.parametrize("strategy", O.STRATEGIES)
def test_roundtrip_zlib_and_oracle(strategy):
    rng = random.Random(11)
    for data in samples(2) + [bytes(rng.randrange(256) for _ in range(150000)), b"\x07" * 200000]:
        if strategy.startswith("FULL") and len(data) > 20000:
            data = data[:20000]
        comp = O.deflate(data, strategy)
        assert zlib.decompress(comp, -15) == data
        reason, out, bits = O.inflate(comp)
        assert reason is None and out == data and (bits + 7) // 8 == len(comp)


def test_full_brute_equals_chain_walk():
    rng = random.Random(7)
    words = [bytes(rng.randrange(97, 101) for _ in range(rng.randrange(2, 6))) for _ in range(30)]
    for n in [0, 5, 300, 4000, 20000]:
        data = b" ".join(rng.choice(words) for _ in range(n // 3))[:n]
        for chunk_len, hist in [(65536, 32768), (3000, 32768), (1500, 700)]:
            for strat in ["FULL_DYNAMIC", "FULL_STATIC"]:
                assert O.deflate(data, strat, chunk_len, hist, brute=True) == O.deflate(data, strat, chunk_len, hist)


def test_package_merge_tie_order_kat():
    """chunk 0 of 1 MiB zeros has litHist {0:1, 256:1, 257:1, 285:254} and the
    reference's tie order gives 285->1, 257->2, 0->3, 256->3 (not 0->2)."""
    h = [0] * 286
    h[0], h[256], h[257], h[285] = 1, 1, 1, 254
    L = P.package_merge(h, 15)
    assert (L[285], L[257], L[0], L[256]) == (1, 2, 3, 3)
    h = [0] * 286
    h[256], h[258], h[285] = 1, 1, 254
    L = P.package_merge(h, 15)
    assert (L[285], L[256], L[258]) == (1, 2, 2)


def test_zeros_1mib_structure():
    data = b"\x00" * (1 << 20)
    comp = O.deflate(data)
    assert comp == P.deflate(data)
    bits = O.block_bits(data)
    assert len(bits) == 16
    assert len(set(bits[1:])) == 1          # chunks 1..15 identical blocks (different from chunk 0)
    assert bits[0] != bits[1]
    assert zlib.decompress(comp, -15) == data
    # bfinal only on the last block: first 3 bits of the stream = bfinal 0, btype 2
    assert comp[0] & 7 == 0b100


def test_empty_input():
    comp = O.deflate(b"")
    assert comp == P.deflate(b"")
    assert zlib.decompress(comp, -15) == b""
    assert comp[0] & 7 == 0b101            # bfinal=1, btype=2 (dynamic)


def test_gzip_config1_fixture():
    """Config 1: gzip of 1 MiB zeros named zeros_1MiB.bin, mtime 1700000000."""
    data = b"\x00" * (1 << 20)
    gz = O.gzip_compress(data, name=b"zeros_1MiB.bin", mtime=1700000000, os_=3, header_crc=True)
    hdr = bytes.fromhex("1f8b080a00f15365000" + "3" + "7a65726f735f314d69422e62696e00")
    assert gz[:len(hdr)] == hdr
    assert gz[len(hdr):len(hdr) + 2] == (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little")
    assert gz[-8:] == bytes.fromhex("1cea38a700001000")
    assert zlib.decompress(gz, 31) == data
    reason, out, hd, end = O.gunzip(gz + b"trailing")
    assert reason is None and out == data and end == len(gz)
    assert hd["mtime"] == 1700000000 and hd["os"] == 3 and hd["has_header_crc"]


MULTI_SETS = [
    ["UNCOMPRESSED"],
    [P.PRESETS["RLE_DYNAMIC"], "UNCOMPRESSED"],
    ["UNCOMPRESSED", P.PRESETS["LITERAL_STATIC"]],
    [P.PRESETS["LITERAL_DYNAMIC"], P.PRESETS["RLE_STATIC"], "UNCOMPRESSED", P.PRESETS["FULL_DYNAMIC"]],
    [P.PRESETS["FULL_STATIC"], P.PRESETS["FULL_DYNAMIC"]],
]


@pytest.mark.parametrize("k", range(len(MULTI_SETS)))
def test_nversion_multistrategy(k):
    """MultiStrategy / Uncompressed: the oracle (closed-form Uncompressed lengths, D/comp/
    Uncompressed.java:22-26) against pyref (lengths measured by writing) and round trips."""
    subs = MULTI_SETS[k]
    rng = random.Random(40 + k)
    for data in samples(3)[:12] + [bytes(rng.randrange(256) for _ in range(70000)), b"\x05" * 70000]:
        for chunk_len, hist in [(65536, 32768), (700, 32768), (97, 1), (65535, 0)]:
            if any(s != "UNCOMPRESSED" and s[4] > 1 for s in subs) and len(data) > 5000:
                continue
            a = O.deflate_multi(data, subs, chunk_len, hist)
            b = P.deflate_multi(data, subs, chunk_len, hist)
            assert a == b, (k, len(data), chunk_len, hist)
            assert zlib.decompress(a, -15) == data


def test_uncompressed_preset_equals_single_multistrategy():
    for data in samples(4)[:10]:
        assert O.deflate(data, "UNCOMPRESSED") == O.deflate_multi(data, ["UNCOMPRESSED"])
        assert O.deflate(data, "RLE_DYNAMIC") == O.deflate_multi(data, [P.PRESETS["RLE_DYNAMIC"]])


@pytest.mark.parametrize("sub", [P.PRESETS["RLE_DYNAMIC"], P.PRESETS["FULL_STATIC"], P.PRESETS["LITERAL_DYNAMIC"],
                                 "UNCOMPRESSED"])
def test_nversion_binarysplit(sub):
    """BinarySplit: oracle against pyref (lengths measured by writing, the reference's position-0
    accumulation kept in both) and round trips."""
    rng = random.Random(60)
    datas = samples(5)[:14] + [bytes(rng.randrange(256) for _ in range(3000)) + b"\x00" * 3000]
    for data in datas:
        for chunk_len, hist, m in [(65536, 32768, 64), (700, 32768, 50), (1024, 0, 100), (300, 10, 1)]:
            if sub != "UNCOMPRESSED" and sub[4] > 1 and len(data) > 2000:
                continue
            a = O.deflate_binsplit(data, sub, m, chunk_len, hist)
            b = P.deflate_binsplit(data, sub, m, chunk_len, hist)
            assert a == b, (sub, len(data), chunk_len, hist, m)
            assert zlib.decompress(a, -15) == data


def test_strategy_ref_pinned_by_oracle():
    """tests/strategy_ref.py (the checker of the GPU plugin tests) agrees with the oracle's own
    MultiStrategy / BinarySplit drivers wherever both apply."""
    import random
    import strategy_ref as R
    rng = random.Random(3)
    data = b"".join(bytes([rng.randrange(3)]) * rng.randrange(1, 400) + rng.randbytes(rng.randrange(0, 300))
                    for _ in range(600))[:150_000]
    assert R.stream(data, R.LzLeaf("RLE_DYNAMIC")) == O.deflate(data, "RLE_DYNAMIC")
    assert R.stream(data, R.Multi(R.LzLeaf("RLE_DYNAMIC"), R.UncLeaf())) == \
        O.deflate_multi(data, [(1, 3, 258, 1, 1), "UNCOMPRESSED"])
    assert R.stream(data, R.Split(R.UncLeaf(), 1000)) == O.deflate_binsplit(data, "UNCOMPRESSED", 1000)
    assert R.stream(data, R.Split(R.LzLeaf("RLE_DYNAMIC"), 2000)) == O.deflate_binsplit(data, (1, 3, 258, 1, 1), 2000)


# ---- code construction at the length limits and header edges (tests/adversarial_hist.py) ----

def _oracle_streams(case):
    """(label, oracle stream, pyref stream or None) per way `case` is encoded."""
    mode, arg, chunk_len, hist = case.encode_args
    if mode == "preset":
        return [(st, O.deflate(case.data, st, chunk_len, hist), P.deflate(case.data, st, chunk_len, hist)) for st in arg]
    comp = O.deflate_lz(case.data, *arg, chunk_len, hist)
    slow = arg[4] > 1 and len(case.data) > 20000       # pyref's distance loop is quadratic
    return [(arg, comp, None if slow else P.deflate(case.data, chunk_len=chunk_len, hist_limit=hist, params=arg))]


BRUTE = {"fib_to29", "lz_all_codes"}        # the exhaustive loop takes seconds at these sizes: two cases


@pytest.mark.parametrize("cls", A.CLASSES)
def test_adversarial_cases(cls):
    """Every generator case: oracle == pyref (or, for the large-distance LZ cases, the planned parse,
    the exhaustive distance loop on two of them, and package-merge of the walked histograms), zlib
    round trip, header lengths == pyref's package_merge of the walked histograms at 15 / 15 / 7, and
    the class's engagement condition on the first way the case is encoded."""
    for case in A.cases(cls):
        for k, (label, comp, ref) in enumerate(_oracle_streams(case)):
            where = (cls, case.name, label)
            assert zlib.decompress(comp, -15) == case.data, where
            if ref is not None:
                assert comp == ref, (where, A.explain(ref, comp))
            blocks = A.walk_blocks(comp)
            assert (blocks[-1]["end_bit"] + 7) // 8 == len(comp), where
            for b in blocks:
                assert (b["lit_lens"], b["dist_lens"], b["cl_lens"]) == A.expected_lengths(b), (where, b["bit"])
            if case.plan is not None:
                copies = [t for t in blocks[0]["tokens"] if not isinstance(t, int)]
                assert len(blocks) == 1 and copies == [(4, d) for _, d in case.plan], where
            if case.name in BRUTE:
                mode, arg, chunk_len, hist = case.encode_args
                assert O.deflate_lz(case.data, *arg, chunk_len, hist, brute=True) == comp, where
            if k == 0:
                assert A.engaged(case.kind, blocks), where


def test_adversarial_case_counts():
    """What the issue of these tests asks each class to hold."""
    n = {cls: len(A.cases(cls)) for cls in A.CLASSES}
    assert n["lit_limit"] >= 11 and n["cl_limit"] >= 3 and n["dist_limit"] == 3 and n["dist_fixups"] >= 5
    assert max(len(c.data) for cls in A.CLASSES for c in A.cases(cls)) <= 65536
    assert all(len(c) == 512 for c in A.cl_runs_sweep_chunks())
    assert len(A.cases("lit_limit")[6].data) == 65535
    assert [len(c.data) for c in A.cases("all_symbols")][0] == 33920


def test_adversarial_hclen_reached():
    """The HCLEN values (as counts) the cases reach; 4 cannot occur (adversarial_hist docstring)."""
    seen = set()
    for cls in A.CLASSES:
        for case in A.cases(cls):
            for _, comp, _ in _oracle_streams(case)[:1]:
                seen |= {b["hclen"] for b in A.walk_blocks(comp) if b["btype"] == 2}
    assert 4 not in seen
    assert seen >= A.HCLEN_REACHED, sorted(seen)


def test_tie_pairs_counter():
    assert A.tie_pairs([1, 1, 2, 2, 2, 2], 15) == 1          # the package 1+1 meets the leaves of 2
    assert A.tie_pairs([1, 2, 4, 8, 16], 15) == 0            # packages 3, 7, 15: no leaf has those
    assert A.tie_pairs([8] * 16, 15) == 0                    # packages are 16, 32, ...
    assert A.tie_pairs([1] * 16 + [2] * 16, 15) == 8         # eight packages of 2 meet sixteen leaves of 2


def test_walk_blocks_replays_input():
    """walk_blocks pinned: its tokens decode back to the input, on a 15-bit literal code, a 15-bit
    distance code, the 101-block sweep, and a stream of stored, static and dynamic blocks."""
    lit = A.cases("lit_limit")[6]
    dist = A.cases("dist_limit")[0]
    sweep = A.cases("cl_runs")[0]
    mixed = sweep.data[:3000] + random.Random(9).randbytes(3000)
    for data, comp in [(lit.data, O.deflate(lit.data, "LITERAL_DYNAMIC")),
                       (dist.data, O.deflate_lz(dist.data, *dist.encode_args[1])),
                       (sweep.data, O.deflate(sweep.data, "RLE_DYNAMIC", 512, 0)),
                       (mixed, O.deflate_mixed(mixed, ["RLE_DYNAMIC", "UNCOMPRESSED", "FULL_STATIC"], 1000))]:
        blocks = A.walk_blocks(comp)
        assert A.replay(blocks) == data
        assert [b["bit"] for b in blocks[1:]] == [b["end_bit"] for b in blocks[:-1]]
        assert O.inflate(comp)[2] == blocks[-1]["end_bit"]
    assert "streams equal" == A.explain(comp, comp)
    bad = bytearray(O.deflate(lit.data, "LITERAL_DYNAMIC"))
    bad[40] ^= 0x10
    assert "block 0" in A.explain(O.deflate(lit.data, "LITERAL_DYNAMIC"), bytes(bad))
