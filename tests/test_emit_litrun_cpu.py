"""The constructions of tests/emit_litrun.py bite: for every case the CPU oracle agrees with token_stream.expand
(bytes, Reason, consumed bits), and the host model of the fast emit pass's token loop (emit_litrun.trace: the
literal-run loop of at most K steps, its margin before the lane's end, the general step after it) shows that each
case hits the limit it is named for.  The model's constants are read out of the kernel's header as text, so a
retune of K or of the margin fails here and sends its author to these cases.
"""
import os
import re

import pytest

import emit_litrun as E
import inflate_geometry as G
import oracle_lib as O


def by_name(family):
    return {c.name: c for c in E.cases(family)}


def test_constants_are_the_kernels():
    wave = open(os.path.join(E.HIP, "inflate_wave.hpp")).read()
    assert E.litrun_k() >= 2
    # the run's exit test and its margin, the checked tail, the pair rule's table width
    assert "if (!((e >> 31) && bb.pos + 2u * LB < lim)) break;" in wave and E.MARGIN == 2 * G.LB
    assert re.search(r"const uint32_t lim = min\(end, nb - min\(nb, (\d+)u\)\);", wave).group(1) == str(E.TAIL)
    assert "for (uint32_t k = 0; k < NDFL_EMITF_LITRUN_K; k++) {" in wave
    # 2K + 1 steps of at most LB bits, the widest terminator and the margin fit one full lane segment
    assert (2 * E.litrun_k() + 1) * G.LB + 48 + E.MARGIN < E.PER


def test_case_counts_are_pinned():
    assert E.COUNTS == {"N": 12, "O": 5, "T": 2, "M": 1, "P": 2, "E": 4}
    for f in E.FAMILIES:
        cs = E.cases(f)
        assert len(cs) == E.COUNTS[f], (f, len(cs))
        assert len({c.name for c in cs}) == len(cs)
        assert all(len(c.comp) <= G.MAX_COMP and len(c.out) <= 64 << 10 for c in cs)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_oracle_agrees_with_expand(family):
    for c in E.cases(family):
        reason, out, bits = O.inflate(c.comp, out_cap=len(c.out) + 1024)
        assert reason == c.reason, (c.name, reason)
        assert out == c.out, c.name
        assert (c.bits is None) == (c.reason is not None)
        if c.reason is None:
            assert bits == c.bits, (c.name, bits, c.bits)


def test_the_code_has_the_table_forms_it_names():
    c = E.code()
    prim = [s for s in range(256) if 0 < c.lit[s] <= G.LB]
    assert sorted(c.lit[s] for s in prim) == [1, 2, 3, 5, 6, 7, 8, 9, 10] and set(E.BULK + E.RUN) <= set(prim)
    # no two run literals make a primary-table pair; (A2, B3) does
    assert all(c.lit[a] + c.lit[b] > G.LB for a in E.RUN for b in E.RUN) and c.lit[E.A2] + c.lit[E.B3] <= G.LB
    # the long literal/length codes fit the 320 extension words (second-level tables); the two 15-bit distance
    # codes do not fit the 64 (a 128-word table: the canonical slow path)
    assert len([l for l in c.lit if l > G.LB]) + 32 <= 320
    assert c.lit[E.Z15] == 15 and c.dist[29] == 15 and 1 << (15 - G.DB) > 64
    assert {E.code("A").width(E.tail_token(E.code("A"), w)) for w in range(1, 21) if w != 4} == set(range(1, 21)) - {4}
    assert E.code("B").width(E.tail_token(E.code("B"), 4)) == 4


def test_n_runs_end_where_they_are_named():
    K = E.litrun_k()
    assert E.n_steps() == [K - 1, K, K + 1, 2 * K + 1]
    seen = set()
    for c in E.cases("N"):
        r, g = E.first_round(c)
        assert g.pw == G.LPW, c.name
        b = c.blocks[c.k]
        for lane, n, at, term_at in c.info["cells"]:
            entry, end = E.lane_span(c, lane)
            assert entry == at, (c.name, lane)
            if c.info["term"] == "eob":                 # (the run's last literal is still MARGIN bits before it)
                assert end == b.end == term_at + 15 <= 8 * len(c.comp) - E.TAIL, c.name
            else:
                assert term_at + 48 + E.MARGIN < end, (c.name, lane)
            ev = E.trace(c, lane)
            # the model's outer iterations from the lane's entry: runs of K steps ended by the step limit with a
            # literal for the general step, then the rest ended by the terminator, which the general step takes
            want, left, pos = [], n, at
            while left > K:
                want += [("run", K, "K"), ("tok", "L")]
                left -= K + 1
            want += [("run", left, "K" if left == K else "token"), ("tok", "E" if c.info["term"] == "eob" else
                                                                   "L" if c.info["term"] == "lit15" else "M")]
            got = [e[:3] if e[0] == "run" else e[:2] for e in ev[:len(want)]]
            assert got == want, (c.name, lane, n, got)
            assert ev[len(want) - 1][2] == term_at, (c.name, lane)
            seen.add((c.info["term"], c.info["pair_last"], n))
            if c.info["term"] == "eob":
                assert term_at == b.starts[-1] and r.done, c.name
    assert seen == ({(t, p, n) for t in E.TERMS for p in (False, True) for n in E.n_steps()} |
                    {("dist1", False, 0)} | {("eob", False, n) for n in E.n_steps()})
    # the deferred terminator reaches before its lane's first byte; the dist-1 run after 0 steps does too
    c = by_name("N")["N_deferred_single"]
    assert all(n + 1 < 120 for _, n, _, _ in c.info["cells"])


def test_o_literals_end_every_offset_before_their_lanes_end():
    offs = {"single": set(), "pair": set()}
    in_run = {"single": set(), "pair": set()}
    for c in E.cases("O"):
        kind = c.info["kind"]
        for lane, off, at, p in c.info["cells"]:
            entry, end = E.lane_span(c, lane)
            ev = E.trace(c, lane)
            if kind == "split":
                # the table's pair (A2, B3) with the lane's end after its first literal: split, by the general step
                assert end == p == at + 2 and ("tok", "L", at, True) in ev, (c.name, lane)
                continue
            assert end - p == off and entry < at, (c.name, lane, off)
            offs[kind].add(off)
            width = p - at
            eligible = at + E.MARGIN < end              # (lim = end: the input's end is far)
            assert eligible == (off + width > E.MARGIN), (c.name, off)
            runs = [e for e in ev if e[0] == "run" and e[3] <= at < e[4]]
            toks = [e for e in ev if e[0] == "tok" and e[2] == at]
            assert len(runs) + len(toks) == 1 and (eligible or toks), (c.name, off)
            if runs:
                in_run[kind].add(off)
            # the last run of every lane ends at the margin or at a token: never past lim
            assert all(e[4] < end for e in ev if e[0] == "run"), (c.name, lane)
    assert offs == {"single": set(range(21)), "pair": set(range(21))}
    assert in_run["single"] and min(in_run["single"]) >= 11 and in_run["pair"] and min(in_run["pair"]) >= 16


def test_t_runs_reach_the_input_tail():
    t = by_name("T")
    c = t["T_run_to_end"]
    b, nb = c.blocks[c.k], 8 * len(c.comp)
    r, g = E.first_round(c)
    assert r.done and b.end > nb - 8
    # the last live lane: the run loop stops MARGIN bits before lim = nb - 48, the bit buffer goes on to lim, the
    # checked decoder takes the literals after it and the end of block
    lane = max(j for j in range(64) if E.lane_span(c, j)[0] < r.exit)
    ev = E.trace(c, lane)
    lim = nb - E.TAIL
    assert any(e[0] == "run" and e[2] == "margin" for e in ev)
    tail = [e for e in ev if e[0] == "tok" and e[2] >= lim]
    assert len(tail) >= 4 and [e[1] for e in tail[:-1]] == ["L"] * (len(tail) - 1) and tail[-1][1] == "E"
    c = t["T_cut_in_run"]
    assert c.reason == G.UEOS and t["T_run_to_end"].out.startswith(c.out) and 0 < len(c.out) < len(t["T_run_to_end"].out)
    at = 8 * len(c.comp)
    b = c.blocks[c.k]
    assert at not in b.starts and all(x[0] == "L" for x in b.tokens)


def test_m_p_e_blocks_are_what_they_are_named():
    c, = E.cases("M")
    assert all(t[0] == "M" for t in c.blocks[c.k].tokens) and len(c.blocks[c.k].tokens) == 230
    r, g = E.first_round(c)
    assert g.pw == G.PW_MIN and sum(1 for j in range(1, 64) if E.lane_span(c, j)[0] < r.exit) >= 3
    p = by_name("P")
    assert p["P_lit8_dist1"].blocks[2].code.n8 == G.N8_PHASED == 192
    kc = p["P_escape_dist1"].blocks[2].code
    assert kc.n8 == 254 and all(cc & 0x7F == 0x7F for cc, l in filter(None, kc.lc[254:]))
    for c in p.values():
        toks = c.blocks[c.k].tokens
        assert sum(1 for t in toks if t[0] == "M" and t[2] == 1) == 90
        assert all(toks[i - 1][0] == "L" for i, t in enumerate(toks) if t[0] == "M")
    for c in E.cases("E"):
        assert c.reason == c.info["reason"], c.name
        if c.blocks:
            lane = c.info["lane"]
            ev = E.trace(c, lane)
            # (the model's token step knows no output: the copy from before the start is a match to it)
            assert ev[0][:3] == ("run", 3, "token") and ev[1][:2] == ("tok", "M" if c.name == "E_copy_before" else "B"), \
                (c.name, ev[:2])
    assert sorted(c.reason for c in E.cases("E")) == sorted([G.EMPTY_DIST, E.RSV_DIST, E.RSV_LEN, "COPY_FROM_BEFORE_DICTIONARY_START"])
