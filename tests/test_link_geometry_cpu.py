"""The constructions of tests/link_geometry.py bite: for every stream of every family the CPU oracle (and zlib, on
the valid ones) agrees with the builder's expected Reason, bytes and consumed bits, the segment-cap condition holds
(at most SEG_CAP accepted headers per 64 KiB of input everywhere but in family O), no stream holds a header candidate
it was not built with, and the host model -- the candidate list, the alias representatives, the bucket keys, the
linked chain list -- shows that each case reaches the edge it is named for.  Nothing here asks the library.  The
model's constants are read out of the kernels' sources as text.  The number of cases per family is pinned.
"""
import bisect
import os
import re
import zlib

import pytest

import link_geometry as G
import oracle_lib as O

HIP = os.path.join(O.ROOT, "deflate-library-java_amd", "csrc", "hip")


def by_name(family):
    return {c.name: c for c in G.cases(family)}


def test_constants_are_the_kernels():
    k = open(os.path.join(HIP, "inflate_kernels.hip")).read()
    common = open(os.path.join(HIP, "ndfl_common.hpp")).read()
    assert "constexpr uint32_t SCAN_T = 256, SCAN_PER = 8, SCAN_TILE = SCAN_T * SCAN_PER;" in common
    assert G.SCAN_TILE == 256 * 8
    assert re.search(r"constexpr uint32_t SEG_CAP = (\d+);", k).group(1) == str(G.SEG_CAP)
    assert re.search(r"constexpr uint32_t SEG_BYTES = (\d+);", k).group(1) == str(G.SEG_BYTES)
    assert re.search(r"constexpr uint32_t OB_NB = (\d+);", k).group(1) == str(G.OB_NB)
    assert f"cands[j - 1] + {G.ALIAS_WINDOW} >= p" in k
    assert "min<uint64_t>(OB_NB - 1, len >> 15)" in k
    assert "((e.end_bit - e.start_bit) >> 15) + (e.out_count >> 14)" in k
    assert "#define NDFL_NEED_INPUT  64" in open(os.path.join(O.ROOT, "include", "ndfl.h")).read()


def test_case_counts_are_pinned():
    assert G.COUNTS == {"L": 24, "B": 4, "A": 7, "D": 2, "E": 26, "R": 23, "O": 1}
    for f in G.FAMILIES:
        cs = G.cases(f)
        assert len(cs) == G.COUNTS[f], (f, len(cs))
        assert len({c.name for c in cs}) == len(cs)
        assert all(len(c.comp) <= 5 << 20 and len(c.out) <= 5 << 20 for c in cs)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_and_zlib_agree_with_the_builder(family):
    for c in G.cases(family):
        cap = len(c.out) + 1024
        if c.code == G.E_ARG:
            # the range end lies inside a block: no range decode ends there
            reason, out, bits = O.inflate_range(c.comp, c.start_bit, None, c.window)
            assert reason is None and bits not in (c.end_bit,) and c.end_bit not in c.seams, c.name
            continue
        if c.partial:
            # the truncated input: UNEXPECTED_END_OF_STREAM as a whole; the expected stop is the last seam whose
            # preceding block lies wholly in it, and the range decode up to it gives the expected bytes
            assert O.inflate(c.comp, out_cap=cap)[0] == G.UEOS, c.name
            assert c.bits in c.seams and c.bits <= 8 * len(c.comp), c.name
            nxt = c.seams[c.seams.index(c.bits) + 1]
            assert nxt > 8 * len(c.comp), c.name
            if c.bits:
                assert O.inflate_range(c.comp, 0, c.bits, out_cap=cap) == (None, c.out, c.bits), c.name
            else:
                assert c.out == b""
            continue
        whole = c.start_bit == 0 and c.end_bit is None
        got = O.inflate(c.comp, out_cap=cap) if whole else \
            O.inflate_range(c.comp, c.start_bit, c.end_bit, c.window, out_cap=cap)
        assert G.reason_code(got[0]) == c.code, (c.name, got[0])
        assert got[1] == c.out, c.name
        assert got[2] == c.bits, (c.name, got[2], c.bits)
        if whole and c.code == 0:
            d = zlib.decompressobj(-15)
            assert d.decompress(c.comp) == c.out and d.eof, c.name
            assert len(d.unused_data) == len(c.comp) - (c.bits + 7) // 8, c.name


def built_candidates(c):
    """The headers a stream was built with: its non-final dynamic blocks, its non-final stored blocks as the bits
    name them (link_geometry.named_stored_headers), family D's decoys (a stored one at its bits 0 .. 5)."""
    nb = 8 * len(c.comp)
    bit = lambda q: c.comp[q >> 3] >> (q & 7) & 1
    res = {s for s, k in zip(c.seams, c.kinds) if k == "dynamic" and s + 3 <= nb and not bit(s)}
    for qs in G.named_stored_headers(c).values():
        res.update(qs)
    res.update(c.info.get("planted", ()))
    for lab, p, _ in c.info.get("decoys", ()):
        res.update([p] if lab in ("b", "e_inside", "d_after") else range(p, p + 6))
    return res


@pytest.mark.parametrize("family", [f for f in G.FAMILIES if f != "O"])
def test_segment_cap_and_no_accidental_candidate(family):
    for c in G.cases(family):
        counts = G.segment_counts(c.comp)
        assert max(counts.values(), default=0) <= G.SEG_CAP, (c.name, counts.most_common(2))
        found, built = set(G.scan(c.comp)), built_candidates(c)
        if c.name == "B_count_buckets":
            # an empty stored block's LEN field (16 zero bits, then FFFF, then the next empty block's zeros) reads as
            # a stored header of LEN 65,535 wherever those bytes end on a plausible header: a decoy the stream was not
            # built with, inside a stored block, in no long chain's way (the model counts it like any candidate)
            extra = found - built
            assert len(extra) < 100 and all(c.kinds[bisect.bisect_right(c.seams, p) - 1] == "stored" for p in extra)
            found -= extra
        assert found <= built, (c.name, sorted(found - built)[:5])
        if not c.partial and c.code in (0, G.E_ARG):
            assert found == built, (c.name, sorted(built - found)[:5])
        if "stored" not in c.kinds:
            # dynamic blocks have no aliases: the candidates are the seams (a header turned into BTYPE 3 is none)
            assert found <= set(c.seams) and G.alias_groups(c) == {}, c.name


def test_family_o_is_over_the_cap():
    (c,) = G.cases("O")
    counts = G.segment_counts(c.comp)
    assert len(counts) == 4 and sum(1 for v in counts.values() if v > G.SEG_CAP) >= 3, counts
    assert all(v > 1200 for s, v in counts.items() if s < 3), counts
    assert G.timings(c)[0] == 682


def test_family_l_reaches_its_lengths():
    cs = by_name("L")
    for n in G.L_NS:
        c = cs[f"L_{n}"]
        assert G.timings(c) == (n, n), c.name                       # n candidates, n chains
        assert G.chain_list(c) == list(c.seams[:n])
        f = cs[f"L_{n}_fixedlast"]
        assert G.timings(f) == (max(1, n - 1), max(1, n - 1)), f.name
        assert f.kinds[n - 1] == "fixed" and f.out == c.out
    # the jump levels ceil(log2 n) (at least 1) take every value from 1 to 13, and n sits on both sides of every
    # power of two that the tile and the 256-thread block are
    nlev = lambda n: max(1, (n - 1).bit_length())
    assert {nlev(n) for n in G.L_NS} >= {1, 2, 8, 9, 11, 12, 13}
    assert [nlev(n) for n in (255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)] == [8, 8, 9, 11, 11, 12, 12, 12, 13]
    # consecutive blocks differ, and each copies from the one before it
    toks = [G.pool_tokens(i) for i in (1, 2, 252)]
    assert ("M", 6, 18) in toks[0] and len({tuple(t[:2]) for t in toks}) == 3


def test_family_b_fills_every_bucket_on_both_sides_of_every_edge():
    cs = by_name("B")
    c = cs["B_count_buckets"]
    cands = G.candidates(c)
    buckets = G.count_buckets(c)
    at = dict(zip(cands, buckets))
    assert {b for b in buckets if b is not None} == set(range(G.OB_NB))
    for seam, bits in c.info["want"].items():
        k = cands.index(seam)
        assert cands[k + 1] - seam == bits, (seam, bits)            # the next candidate stands right behind the block
        assert at[seam] == G.OB_NB - 1 - min(G.OB_NB - 1, bits >> 15)
    wants = sorted(c.info["want"].values())
    for k in G.B_UNITS:
        assert k * G.UNIT - 1 in wants and k * G.UNIT in wants
    below, at_edge = (G.OB_NB - 1 - min(G.OB_NB - 1, (k * G.UNIT - d) >> 15) for d in (1, 0))
    assert (below, at_edge) == (0, 0) and max(G.B_UNITS) > G.OB_NB            # beyond the clamp
    assert [G.OB_NB - 1 - ((1 * G.UNIT - d) >> 15) for d in (1, 0)] == [23, 22]
    # a tile edge of the candidate list inside the stream, with aliases (left out of the order) on both sides
    assert len(cands) > 2 * G.SCAN_TILE
    for edge in (G.SCAN_TILE, 2 * G.SCAN_TILE):
        assert None in buckets[edge - 8:edge] and None in buckets[edge:edge + 8], edge
    assert set(G.emit_buckets(c)) >= {0, 23}
    # the emit key: chains of few input bits and a large output
    seen = set()
    for i in range(len(G.B_EMIT_SPLIT)):
        e = cs[f"B_emit_buckets_{i}"]
        lst = G.chain_list(e)
        eb = dict(zip(lst, G.emit_buckets(e)))
        off = dict(zip(e.seams, e.outs))
        for seam, n in e.info["want_out"].items():
            k = lst.index(seam)
            assert lst[k + 1] - seam < G.UNIT and off[lst[k + 1]] - off[seam] == n, (e.name, seam)
            assert eb[seam] == G.OB_NB - 1 - min(G.OB_NB - 1, n >> 14)
            seen.add(n)
    for j in range(1, G.OB_NB + 1):
        assert j * G.OUT_UNIT - 1 in seen and j * G.OUT_UNIT in seen
    assert 30 * G.OUT_UNIT in seen


def test_family_a_groups_have_the_sizes_named():
    cs = by_name("A")

    def groups_by_bit(c):
        cands = G.candidates(c)
        return {cands[r]: [cands[k] for k in ks] for r, ks in G.alias_groups(c).items()}

    # after a fixed block that ends at each bit offset: the group is what the bits name, its first member lies
    # before the true header (inside the fixed block's end of block), for every offset
    c = cs["A_after_fixed_offsets"]
    named = G.named_stored_headers(c)
    g = groups_by_bit(c)
    offs, before = set(), 0
    for seam, qs in named.items():
        prev = c.kinds[c.seams.index(seam) - 1]
        if prev == "fixed":
            assert g[qs[0]] == qs and qs[0] <= seam and len(qs) >= 2, (seam, qs)
            offs.add(seam % 8)
            before += qs[0] < seam
    assert offs == set(range(8)) and before == 7     # (a header 6 bits into a byte: LEN lies 10 bits on, none earlier)
    for name in ("A_header_byte_00", "A_empty_stored_x8", "A_group_on_segment_edge"):
        c = cs[name]
        g = groups_by_bit(c)
        named = G.named_stored_headers(c)
        for seam, size in c.info["sizes"].items():
            qs = named[seam]
            assert len(qs) == size and g[qs[0]] == qs, (name, seam, qs)
    c = cs["A_header_byte_00"]
    (seam,) = c.info["sizes"]
    assert G.named_stored_headers(c)[seam] == list(range(seam, seam + 6))          # after the true header
    c = cs["A_empty_stored_x8"]
    cands = G.candidates(c)
    assert all(b - a == 40 for a, b in zip(c.seams[2:9], c.seams[3:10]))
    assert all(len(ks) == 6 for ks in list(G.alias_groups(c).values())[1:])
    c = cs["A_first_block_stored"]
    assert G.alias_groups(c)[0] == [0, 1, 2, 3, 4, 5] and G.candidates(c)[:6] == [0, 1, 2, 3, 4, 5]
    c = cs["A_group_on_segment_edge"]
    (qs,) = [qs for s, qs in G.named_stored_headers(c).items() if s in c.info["sizes"]]
    assert qs[0] < c.info["edge"] <= qs[-1] and len({q // (8 * G.SEG_BYTES) for q in qs}) == 2
    c = cs["A_group_on_index_256"]
    qs = G.named_stored_headers(c)[c.info["stored"]]
    ks = [G.candidates(c).index(q) for q in qs]
    assert ks == list(range(252, 260)) and G.alias_groups(c)[252] == ks
    # a dynamic candidate within the window before stored ones: they are no aliases of it, only of each other
    c = cs["A_dynamic_before_stored_lookalikes"]
    cands, found = G.candidates(c), G.scan(c.comp)
    p, qs = c.info["dynamic"], c.info["planted"]
    assert p in c.seams and p in found and all(q in found for q in qs) and qs[0] - p <= G.ALIAS_WINDOW
    assert G.stored_key(c.comp, p) is None and len({G.stored_key(c.comp, q) for q in qs}) == 1
    k = cands.index(p)
    reps = G.alias_reps(c.comp, cands)
    assert cands[k + 1:k + 7] == qs and reps[k:k + 7] == [k] + [k + 1] * 6
    assert all(q not in G.chain_list(c) for q in qs) and p in G.chain_list(c)
    # the window has slack: headers with one LEN position lie within [LEN - 10, LEN - 3], at most 7 bits apart, so any
    # window from 7 bits up marks the same groups (a window of 9 for 10 changes no result; 6 would)
    narrower = 0
    for c in cs.values():
        cands = G.candidates(c)
        assert G.alias_reps(c.comp, cands, 7) == G.alias_reps(c.comp, cands), c.name
        narrower += G.alias_reps(c.comp, cands, 6) != G.alias_reps(c.comp, cands)
    assert narrower >= 3                             # (the groups of 8)
    for c in cs.values():
        if "planted" in c.info:
            continue
        assert G.timings(c)[0] == 1 + sum(1 for s, k in zip(c.seams[1:], c.kinds[1:-1]) if k != "fixed"), c.name


def test_family_d_decoys_are_candidates_and_end_as_stated():
    for c in G.cases("D"):
        found = set(G.scan(c.comp))
        assert len(c.info["decoys"]) == 6
        lst = G.chain_list(c)
        for lab, p, how in c.info["decoys"]:
            assert p in found and p not in c.seams and p not in lst, (c.name, lab)
            reason = O.inflate_range(c.comp, p, None)[0]
            assert reason == (None if how == "joins" else how), (c.name, lab, reason)
        # every decoy but the ones in and after the final block has a lower candidate index than the last true chain
        cands = G.candidates(c)
        assert sum(1 for lab, p, _ in c.info["decoys"] if cands.index(p) < cands.index(lst[-1])) == 4
        assert G.timings(c)[0] == len(lst) == (6 if c.code else 5), (c.name, len(lst))


def test_family_e_indices_are_the_models():
    cs = by_name("E")
    for t in G.E_TS:
        c = cs[f"E_reserved_t{t}"]
        lst = G.chain_list(c)
        assert len(lst) == t + 1 and lst[t] == c.seams[t] and c.stop_at == c.seams[t + 1]       # chain t runs into it
        assert c.stop_at not in G.scan(c.comp) and len(c.out) == 20 * (t + 1)
        assert G.timings(c) == (t + 1, G.POOL - 1 if t < G.POOL - 1 else G.POOL)
        c = cs[f"E_partial_in_block_t{t}"]
        lst = G.chain_list(c)
        assert len(lst) == t + 1 and lst[t] == c.bits == c.seams[t] < 8 * len(c.comp) < c.seams[t + 1]
        c = cs[f"E_partial_in_second_block_t{t}"]
        lst = G.chain_list(c)
        assert len(lst) == t + 1 and lst[t] == c.info["stored"] and c.kinds[t:t + 2] == ("stored", "fixed")
        assert c.bits == c.seams[t + 1] < 8 * len(c.comp)
        c = cs[f"E_partial_on_seam_t{t}"]
        assert c.silent and c.bits == 8 * len(c.comp) == c.seams[t + 1]
    assert {t // G.SCAN_TILE for t in G.E_TS} == {0, 1, 2} and {2047, 2048} <= set(G.E_TS)
    c = cs["E_reserved_two_tiles"]
    assert len(G.chain_list(c)) == 1001 and c.info["later"] // G.SCAN_TILE != c.info["t"] // G.SCAN_TILE
    c = cs["E_copy_before_four_tiles"]
    assert len(G.chain_list(c)) == G.POOL                            # every chain is linked: the emit pass finds them
    assert len({t // G.SCAN_TILE for t in (c.info["t"],) + c.info["later"]}) == 3 and len(c.out) == 41


def test_family_r_slices_fall_where_named():
    cs = by_name("R")
    for i, j in G.R_PAIRS:
        c = cs[f"R_{i}_{'end' if j is None else j}"]
        n = (G.POOL if j is None else j) - i
        assert G.timings(c) == (n, n), c.name                       # the start header is not counted twice
        assert len(c.window) == min(32768, 20 * i) and len(c.out) == 20 * n + (8 if j is None else 0)
    assert {j - i for i, j in G.R_PAIRS if j} >= {1, 255, 256, 2047, 2048}
    whole = len(G.scan(cs["R_0_1"].comp))
    assert whole == G.POOL                                          # candidates before and behind a slice exist
    for name, n in (("R_end_on_fixed_start", 3), ("R_end_on_final_start", 3), ("R_end_on_fixed_start_long", 2048),
                    ("R_start_on_fixed_start", 1), ("R_start_on_fixed_start_mid", 295)):
        c = cs[name]
        assert G.timings(c) == (n, n), (name, G.timings(c))
        edge = c.start_bit if "start_on" in name else c.end_bit
        assert edge in c.seams and edge not in G.scan(c.comp), name
    for name in ("R_start_after_its_aliases", "R_start_after_its_aliases_short"):
        c = cs[name]
        before = [p for p in G.scan(c.comp) if c.start_bit - 10 <= p < c.start_bit]
        assert before and G.candidates(c)[0] == c.start_bit and not set(before) & set(G.candidates(c)), name
        assert G.alias_groups(c), name
    for d in (-1, 1):
        c = cs[f"R_end_seam{d:+d}"]
        assert c.code == G.E_ARG and c.end_bit - d in c.seams
