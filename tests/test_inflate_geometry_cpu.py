"""The constructions of tests/inflate_geometry.py bite: for every case the CPU oracle agrees with
token_stream.expand (bytes, Reason, consumed bits), and the host model of the count pass's round geometry shows
that the case hits the limit it is named for -- the token's start against the round or segment end, the pair split,
the round's span, the candidate's offset, the lanes that do not synchronise.  The model's constants are read out of
the kernels' headers as text, so a retune fails here and sends its author to these cases.  The number of cases per
family is pinned.  (Measured: 3.5 s, nearly all of it the builders; the spec / verify simulation of families C and
P takes 0.2 s.)
"""
import bisect
import os
import re

import pytest

import inflate_geometry as G
import oracle_lib as O
from inflate_geometry import LPW, PW_MIN, XCP1, XCP2, Sim, geo, rspan, seg

rounds_of = G.tested_rounds

HIP = os.path.join(O.ROOT, "deflate-library-java_amd", "csrc", "hip")


def by_name(family):
    return {c.name: c for c in G.cases(family)}


def test_constants_are_the_kernels():
    wave = open(os.path.join(HIP, "inflate_wave.hpp")).read()
    rec = open(os.path.join(HIP, "inflate_records.hpp")).read()

    def define(text, name):
        m = re.findall(rf"^#define {name} (\d+)\b", text, re.M)
        assert len(m) == 1, name
        return int(m[0])

    assert define(wave, "NDFL_LPW") == G.LPW and define(rec, "NDFL_PW_MIN") == G.PW_MIN
    assert define(wave, "NDFL_XCP1") == G.XCP1 and define(wave, "NDFL_XCP2") == G.XCP2
    assert define(wave, "NDFL_PH_FALLBACK") == G.PH_FALLBACK and define(wave, "NDFL_PH_FRONTIER") == G.PH_FRONTIER
    assert define(wave, "NDFL_PHASE_SWITCH") == G.PHASE_SWITCH
    assert re.search(r"constexpr uint32_t LB = (\d+);", rec).group(1) == str(G.LB)
    assert re.search(r"constexpr uint32_t DB = (\d+);", rec).group(1) == str(G.DB)
    assert "constexpr uint64_t RSPAN = 64ull * LPW * 32;" in wave
    assert "constexpr uint64_t SPAN_W = RSPAN * W;" in open(os.path.join(HIP, "inflate_wg.hpp")).read()
    assert re.search(r"const uint32_t lim = min\(stop, nb - min\(nb, (\d+)u\)\);", wave).group(1) == str(G.TAIL)
    assert re.findall(r"phased = n8 >= (\d+);", wave) == [str(G.N8_PHASED)]
    assert "g.base = rs & ~31ull;" in wave
    # seg_pw as the header has it, for every span a round can have
    assert all(G.seg_pw(span, nl) == max(PW_MIN, -(-(-(-span // nl)) // 32))
               for nl in (64, 256) for span in range(1, 64 * LPW * 32 * (nl // 64) + 1, 97))


def test_case_counts_are_pinned():
    assert G.COUNTS == {"R": 89, "S": 23, "C": 24, "T": 29, "P": 14, "K": 6}
    for f in G.FAMILIES:
        cs = G.cases(f)
        assert len(cs) == G.COUNTS[f], (f, len(cs))
        assert len({c.name for c in cs}) == len(cs)
        assert all(len(c.comp) <= G.MAX_COMP and len(c.out) <= G.MAX_OUT for c in cs)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_agrees_with_expand(family):
    for c in G.cases(family):
        reason, out, bits = O.inflate(c.comp, out_cap=len(c.out) + 1024)
        assert reason == c.reason, (c.name, reason)
        assert out == c.out, c.name
        assert (c.bits is None) == (c.reason is not None)
        if c.reason is None:
            assert bits == c.bits, (c.name, bits, c.bits)


@pytest.mark.parametrize("family", ["R", "S", "C", "T", "P"])
def test_no_candidate_but_the_real_headers(family):
    for c in G.cases(family):
        real, alias = G.real_headers(c)
        if c.name.startswith("P_short_round"):          # (their round end is a planted header: that one and its aliases)
            extra = set(G.candidates(c.comp)) - {0} - real - alias
            assert min(extra) == c.info["E"] and extra <= set(range(c.info["E"], c.info["E"] + 8)), c.name
            continue
        assert G.clean(c), c.name
        assert real <= set(G.candidates(c.comp)), c.name      # (and the finder sees every real one)


def width_at(c, at):
    st = c.blocks[c.k].starts
    i = bisect.bisect_left(st, at)
    assert st[i] == at
    return st[i + 1] - at if at != st[-1] else c.blocks[c.k].end - at


def test_r_tokens_start_k_bits_before_a_round_end():
    n = 0
    for c in G.cases("R"):
        if not c.name.startswith("R_token"):
            continue
        n += 1
        i = c.info
        rounds = rounds_of(c, c.W)
        assert len(rounds) == i["round"] + 2, c.name
        r = rounds[i["round"]]
        assert r.E - r.rs == rspan(c.W) and i["at"] == r.E - i["k"] and width_at(c, i["at"]) == i["w"], c.name
        if i["k"] < i["w"]:                             # the round is cut inside the token
            assert r.exit == i["at"] + i["w"] > r.E, c.name
        elif i["k"] == i["w"]:                          # the token ends on the round end
            assert r.exit == r.E == i["at"] + i["w"], c.name
        else:                                           # it ends one bit before: no token fills a 1-bit gap, so the
            nxt = i["at"] + i["w"]                      # next one starts there and the round is cut inside that one
            assert nxt == r.E - 1 and width_at(c, nxt) >= 2 and r.exit == nxt + width_at(c, nxt), c.name
    assert n == 57
    ws = {(c.W, c.info["w"]) for c in G.cases("R") if c.name.startswith("R_token")}
    assert ws == {(W, w) for W in (1, 4) for w in (2, 15, 16, 31, 48)} | {(1, 46)}
    assert {c.blocks[c.k].d0 % 32 for c in G.cases("R")} >= set(G.D0_MODS)


def test_r_end_of_block_alone_in_its_round():
    n = 0
    for c in G.cases("R"):
        if not c.name.startswith("R_eob_alone"):
            continue
        n += 1
        b = c.blocks[c.k]
        rounds = rounds_of(c, c.W)
        assert len(rounds) == 2, c.name
        full, last = rounds
        assert full.E - full.rs == rspan(c.W) and full.exit == full.E == last.rs == b.starts[-1], c.name
        assert b.end - b.starts[-1] == c.info["eobw"] and last.done, c.name
        if c.info["follow"] == "stored":                # its header is a candidate: the span is the code's width
            assert last.E == b.end and last.E - last.rs == c.info["eobw"], c.name
        else:
            assert last.E == 8 * len(c.comp), c.name
    assert n == 18


def test_r_short_last_rounds():
    n = 0
    for c in G.cases("R"):
        if not c.name.startswith("R_last_round"):
            continue
        n += 1
        last = rounds_of(c, c.W)[-1]
        g = geo(last.rs, last.E, c.W)
        assert last.E - last.rs == c.info["span"] and g.pw == PW_MIN, c.name
        live = [j for j in range(g.nl) if seg(g, j)[0] < seg(g, j)[1]]
        assert live == list(range(-(-c.info["span"] // (32 * PW_MIN)))), c.name
    assert n == 14


def test_s_tokens_at_the_segment_ends():
    n = last = 0
    for c in G.cases("S"):
        r = rounds_of(c, c.W)[0]
        g = geo(r.rs, r.E, c.W)
        b = c.blocks[c.k]
        if c.name.startswith("S_last"):                 # the round ends with the cut input, in the last lane
            last += 1
            (j, at), = c.info["at"]
            s, e = seg(g, j)
            assert g.pw == PW_MIN and j == g.nl - 1 and e == r.E == 8 * len(c.comp) and c.reason == G.UEOS, c.name
            assert s < at == e - c.info["off"] and width_at(c, at) == 48, c.name
            assert len(rounds_of(c, c.W)) == (2 if c.info["off"] == 48 else 1), c.name
        elif c.name.startswith("S_big"):
            n += 1
            assert g.pw == c.info["pw"] and g.pw in (PW_MIN, LPW), c.name
            assert len(rounds_of(c, c.W)) == (1 if g.pw == PW_MIN else 2), c.name
            lanes = [j for j, _ in c.info["at"]]
            assert lanes == G.s_lanes(c.W, g.pw == PW_MIN) and {0, 1, 31, 62} <= set(lanes), c.name
            for j, at in c.info["at"]:
                e = seg(g, j)[1]
                assert at == e - c.info["off"] and width_at(c, at) == 48, (c.name, j)
                assert (at + 48 == e) == (c.info["off"] == 48), (c.name, j)
        else:
            st = b.starts
            per_lane = [bisect.bisect_left(st, seg(g, j)[1]) - bisect.bisect_left(st, seg(g, j)[0]) for j in range(g.nl)]
            widths = {y - x for x, y in zip(st, st[1:]) if x < r.E}
            assert g.pw == LPW and widths == {c.info["all"]}, c.name
            if c.info["all"] == 1:
                assert per_lane == [448] * g.nl, c.name
            elif c.info["all"] == 2:                    # 57,792 bytes per lane: under the phase runs' 16-bit counts
                assert per_lane == [224] * 64 and 224 * 258 == 57792 < 65536, c.name
            else:
                assert min(per_lane) >= 9 and (r.E - b.d0) % 48 != 0, c.name
    assert n == 12 and last == 6


def lane_of(c, lane, W=1):
    r = rounds_of(c, W)[0]
    g = geo(r.rs, r.E, W)
    s, e = seg(g, lane)
    b = c.blocks[c.k]
    return b, s, e, next(t for t in b.starts if t >= s)


def test_c_boundaries_and_pairs_at_the_checkpoints():
    n = 0
    for c in G.cases("C"):
        i = c.info
        if c.name.startswith("C_boundary"):
            n += 1
            b, s, e, entry = lane_of(c, G.C_LANE)
            assert e - s == 32 * LPW and i["at"] == s + i["cp"] + i["d"] and i["at"] in b.starts, c.name
            pos, term = Sim(c.comp, b.code).run_to(entry, s + i["cp"])
            assert not term and pos == (i["at"] if i["d"] >= 0 else i["at"] + 15), c.name
        elif c.name.startswith("C_pair"):
            n += 1
            b, s, e, entry = lane_of(c, G.C_LANE)
            stop = s + i["stop"]
            assert i["at"] + 2 == stop + i["d"] and i["at"] in b.starts and i["at"] + 2 in b.starts, c.name
            sim = Sim(c.comp, b.code)
            end, kind, ntok, split = sim.step(i["at"], stop)
            assert (ntok, split, end) == ((2, False, i["at"] + 4) if i["d"] < 0 else (1, True, i["at"] + 2)), c.name
            # the decode from the lane's true entry takes this very step, and stands on the first boundary at or
            # past the stop
            pos = entry
            while pos < i["at"]:
                pos = sim.step(pos, stop)[0]
            assert pos == i["at"], c.name
            assert sim.run_to(entry, stop)[0] == (i["at"] + 4 if i["d"] < 0 else i["at"] + 2), c.name
    assert n == 15


def test_c_last_lane_segments():
    for L in (1, 64, 65, 192):
        c = by_name("C")[f"C_last_lane_{L}"]
        rounds = rounds_of(c, 1)
        assert len(rounds) == 1
        g = geo(rounds[0].rs, rounds[0].E, 1)
        s, e = seg(g, 63)
        assert e - s == L and g.pw == c.info["pw"] and e == c.blocks[c.k].end
        assert (s + min(XCP1, e - s) == e) == (L <= 64) and s + min(XCP2, e - s) == e


def test_c_lanes_that_do_not_synchronise():
    for c in G.cases("C"):
        if not c.name.startswith("C_nslow"):
            continue
        rounds = rounds_of(c, 1)
        got = G.block_nslow(c, rounds, 1)
        want = c.info["nslow"]
        if len(want) == 2 and want[0] > G.PHASE_SWITCH:
            want = [want[0], 0]                         # the next round is phase-mapped
        assert got[:len(want)] == want and sum(got[len(want):]) == 0, (c.name, got)
        sim = Sim(c.comp, c.blocks[c.k].code)
        assert sim.round_nslow(rounds[0].rs, rounds[0].E, 1)[1] == list(range(3, 3 + want[0])), c.name
        assert c.blocks[c.k].code.n8 == G.N8_PHASED - 1
    names = [c.name for c in G.cases("C") if c.name.startswith("C_nslow")]
    assert names == ["C_nslow_1", "C_nslow_8", "C_nslow_9", "C_nslow_49_then_9", "C_nslow_48_then_9"]


def test_t_tails():
    for c in G.cases("T"):
        b, nb = c.blocks[c.k], 8 * len(c.comp)
        if c.name.startswith("T_eob_gap"):
            assert nb - b.end == c.info["gap"], c.name
        elif c.name.startswith("T_tail"):
            at = nb - c.info["back"]
            # run_to: lim = nb - TAIL; a token that starts before lim is the bit buffer's, any later one the
            # checked decoder's
            assert at in b.starts and c.info["path"] == ("unchecked" if at < nb - G.TAIL else "checked"), c.name
            whole = c.name == "T_tail_match48_at48"     # a whole match as the input's last 48 bits, nothing after
            assert c.reason == (G.EMPTY_DIST if c.info["kind"] == "lenonly" else G.UEOS if whole else None), c.name
            if c.info["kind"] == "match48":
                assert width_at(c, at) == 48 and at + 48 == (nb if whole else nb - 1), c.name
        else:
            assert c.reason == G.UEOS and nb == 8 * c.info["cut"], c.name
    paths = [(c.info["kind"], c.info["back"], c.info["path"]) for c in G.cases("T") if c.name.startswith("T_tail")]
    assert sorted(paths) == sorted([
        ("lit2", 3, "checked"), ("lit2", 49, "unchecked"), ("lit15", 16, "checked"), ("pair", 5, "checked"),
        ("pair", 48, "checked"), ("pair", 49, "unchecked"), ("match31", 32, "checked"), ("match48", 49, "unchecked"),
        ("match48", 48, "checked"), ("lenonly", 20, "checked"), ("lenonly", 49, "unchecked")])
    c = by_name("T")["T_cut_in_token"]
    r = rounds_of(c._replace(comp=by_name("T")["T_cut_last1"].comp + b"\0"), 1)
    at = c.info["at"]
    g = geo(r[1].rs, r[1].E, 1)
    assert seg(g, 7)[0] <= at < seg(g, 7)[1] and at < 8 * len(c.comp) < at + 48 and width_at(c, at) == 48
    c = by_name("T")["T_cut_token_44_of_48"]
    assert c.info["at"] == at and 8 * len(c.comp) == at + 44 and G.TAIL - 8 < 44 <= G.TAIL
    assert sorted(len(by_name("T")["T_cut_last1"].comp) + 1 - c.info["cut"] for c in G.cases("T")
                  if c.name.startswith("T_cut_last")) == list(range(1, 9))


def test_p_phase_mapped_rounds():
    p = by_name("P")
    assert p["P_n8_191"].blocks[2].code.n8 == 191 and p["P_n8_192"].blocks[2].code.n8 == 192
    assert G.block_nslow(p["P_n8_192"], rounds_of(p["P_n8_192"], 1)) == [0, 0]
    ds = []
    for c in G.cases("P"):
        if c.name.startswith("P_entry"):
            d, ph = G.entry_phase(c)
            ds.append(d)
            b, s, e, entry = lane_of(c, G.P_LANE)
            assert entry == s + d == c.info["at"] + 48 and c.blocks[c.k].code.n8 >= G.N8_PHASED, c.name
            assert ph == (d if d < 8 else d - 8 if d < 16 else None), (c.name, ph)
    assert ds == [0, 1, 7, 8, 9, 15, 16, 30, 47]
    for ov in (0, 1):                                   # a short round whose last token overhangs its end
        c = p[f"P_short_round_overhang{ov}"]
        b = c.blocks[c.k]
        r = rounds_of(c, 1)[0]
        assert b.code.n8 >= G.N8_PHASED and r.rs == b.d0 and r.E == c.info["E"] and not r.done, c.name
        assert geo(r.rs, r.E, 1).pw == PW_MIN and r.exit - r.E == ov, c.name
        assert r.exit == c.info["at"] + 48 and width_at(c, c.info["at"]) == 48, c.name
    c = p["P_escape_len_at_segment_end"]
    b, s, e, entry = lane_of(c, G.P_LANE)
    code = b.code
    assert code.n8 == 254 and all(code.lc[x] == (G.rev8(x), 8) for x in range(254))
    assert all(cc & 0x7F == 0x7F for cc, l in filter(None, code.lc[254:]))    # under the escape prefix
    assert c.info["at"] < s < c.info["at"] + 15 and width_at(c, c.info["at"]) == 48


def test_k_planted_candidates_cut_rounds():
    for c in G.cases("K"):
        cands = G.candidates(c.comp)
        if "want" not in c.info:
            real_end = c.blocks[-1].end
            assert c.bits == real_end and len(c.comp) - (real_end + 7) // 8 == c.info["trailing"], c.name
            if c.name == "K_trailing_copy_before":
                first = next(x for x in cands if x >= real_end)
                assert O.inflate_range(c.comp, first)[0] == "COPY_FROM_BEFORE_DICTIONARY_START"
            else:
                assert O.inflate(c.comp[(real_end + 7) // 8:]) == (None, b"hello", 8 * 10)
            continue
        b = c.blocks[c.k]
        assert set(c.info["want"]) <= set(cands) and all(b.d0 < x < b.end for x in c.info["want"]), c.name
        rounds = rounds_of(c, 1)
        cut = [r for r in rounds if r.E == c.info["want"][0]]
        assert len(cut) == 1 and not cut[0].done, c.name
        at = max(t for t in b.starts if t <= c.info["want"][0])
        if c.name == "K_in_token":
            assert width_at(c, at) == 48 and all(at < x < at + 48 for x in c.info["want"])
            assert cut[0].exit == at + 48
        elif c.name == "K_on_boundary":
            assert at == c.info["want"][0] == cut[0].exit
        elif c.name == "K_after_round_start":
            assert cut[0].rs == b.d0 and cut[0].E == b.d0 + 1
        else:
            assert cut[0].rs == b.d0 and cut[0].E == b.d0 + rspan(1) - 1
