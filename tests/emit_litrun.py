"""Hand-placed token streams for the fast emit pass's literal-run loop (csrc/hip/inflate_wave.hpp:
ndfl_inflate_emit_fast_kernel, token_loop).

A lane of the fast emit kernel replays its segment of a round -- from the first token boundary at or past the
segment's nominal start to the next lane's -- in outer iterations: first up to K = NDFL_EMITF_LITRUN_K steps of the
literal-run loop (a step is one primary-table entry, a literal or a literal pair, taken while the entry starts more
than MARGIN = 2 LB bits before lim = min(lane end, input end - 48)), then one general token step.  Every limit of
that loop sits at an exact bit position or step count, so the streams are written with the block writer of
tests/inflate_geometry.py (explicit code lengths, every token's start known) and the loop is restated here on the
host:

    lane_span(case, j)       lane j's [entry, end) in the tested block's first round (the count pass's W = 1 geometry)
    trace(case, j)           the lane's outer iterations: ("run", steps, why, from, to) and ("tok", kind, at, split)

Families (cases(name)):
    N  literal runs of K-1, K, K+1 and 2K+1 steps from a lane's entry, ended by a dist-1 run (also 0 steps: the run
       is the lane's first token), a match reaching into the previous lane (deferred), a 15-bit literal (second-level
       table), a match whose distance code takes the canonical slow path, the end of block; the run's last step a
       single literal or a pair
    O  a literal (10 bits) or a literal pair (2 + 3 bits) ending 0..20 bits before its lane's end, every offset, and
       the pair that the lane's end splits
    T  a literal run into the input's last 48 bits, and the same stream cut inside the run
    M  a block of matches only
    P  blocks of the four-literal (TP_LIT8) and the escape-scan steps: literal runs ended by dist-1 runs
    E  a reserved length symbol, a reserved distance symbol, a length code under an empty distance code and a copy
       from before the output's start, each after a literal run

Not built: a literal/length code on the canonical slow path, because no valid block has one.  That path is taken
when the second-level tables need more than LX = 320 extension words.  A complete code's codes are sorted by length,
so a 10-bit prefix whose longest code has l bits holds 2^(l - 10) table words and, when all its codes have l bits, as
many symbols; only the prefixes where the length steps up hold fewer symbols than words, and together they waste
fewer than 32 words.  With at most 286 symbols that is under 318 words.  The distance code's slow path (two 15-bit
codes: a 128-word table against DX = 64) stands for it in family N.
Test infrastructure only.
"""
import functools
import os
import random
import re

import inflate_geometry as G
import oracle_lib as O
import token_stream as TS

HIP = os.path.join(O.ROOT, "deflate-library-java_amd", "csrc", "hip")
LB, TAIL = G.LB, G.TAIL
MARGIN = 2 * LB


@functools.lru_cache(maxsize=None)
def litrun_k():
    """NDFL_EMITF_LITRUN_K as the kernel's header has it."""
    m = re.findall(r"^#define NDFL_EMITF_LITRUN_K (\d+)\b", open(os.path.join(HIP, "inflate_wave.hpp")).read(), re.M)
    assert len(m) == 1
    return int(m[0])


# ---- the code ---------------------------------------------------------------------------------------------------
X1, A2, B3, L5, L6, L7, F8, G9, H10, Y11, Y12, Y13, Z15 = 0x58, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x6B, 0x5A
RUN = [G9, H10, F8]                     # no two of them fit the primary table together: one step each


@functools.lru_cache(maxsize=None)
def code(variant="A", dist="slow"):
    """One literal of every length 1..13 but 4 (variant "B": but 5), (258, d) under a 4-bit (5-bit) length code, a
    literal, the length symbols 257 (3) and 281 (131..162) and the end of block in 15 bits.  Literals of up to 10
    bits are primary-table entries, the longer ones go to second-level tables.  dist: "slow" (G.D_SLOW), None (the
    empty distance code), "rsv" (32 lengths of 5 bits: the reserved symbols 30 and 31 have codes)."""
    lens = [0] * 286
    for s, l in ((X1, 1), (A2, 2), (B3, 3), (285, 4), (L5, 5), (L6, 6), (L7, 7), (F8, 8), (G9, 9), (H10, 10), (Y11, 11),
                 (Y12, 12), (Y13, 13), (Z15, 15), (257, 15), (281, 15), (256, 15)):
        lens[s] = l
    if variant == "B":
        lens[285], lens[L5] = 5, 4
    d = {"slow": G.D_SLOW, None: None, "rsv": [5] * 32}[dist]
    return G.Code(f"litrun_{variant}_{dist}", lens, d)


def tail_token(c, width):
    """A single token of `width` bits of code c."""
    lits = {c.lit[s]: s for s in (X1, A2, B3, L5, L6, L7, F8, G9, H10, Y11, Y12, Y13, Z15)}
    if width in lits:
        return ("L", lits[width])
    for t in (("M", 3, 1), ("M", 3, 4)) + tuple(("M", 258, dd) for dd in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65)):
        if c.width(t) == width:
            return t
    raise AssertionError((c.name, width))


BULK = [L5, L6, L7, F8, G9, H10]        # the filler: primary-table literals only


def run_tokens(n, pair_last):
    """n literal-run steps whose last literal differs from the one before it; pair_last: the last step is the pair
    (A2, B3)."""
    toks = [("L", RUN[i % 3]) for i in range(n)]
    if pair_last and n:
        if n > 1:
            toks[-2] = ("L", H10)       # (10 bits: never the first of a pair)
        toks[-1:] = [("L", A2), ("L", B3)]
    return toks


# ---- the model ----------------------------------------------------------------------------------------------------
def first_round(case):
    r = G.tested_rounds(case, 1)[0]
    return r, G.geo(r.rs, r.E, 1)


def lane_span(case, j):
    """Lane j's [entry, end) in the tested block's first round: from the first token boundary at or past its
    nominal start to the next lane's (the last live lane: to the round's exit)."""
    r, g = first_round(case)
    b = case.blocks[case.k]
    bounds = b.starts + [b.end]

    def entry(q):
        if q >= g.nl:
            return r.exit
        s = G.seg(g, q)[0]
        return min(next((t for t in bounds if t >= s), r.exit), r.exit) if q else r.rs
    return entry(j), entry(j + 1)


def trace(case, j, K=None):
    """Lane j's outer iterations in the plain instance of the token loop: ("run", steps, why, from, to) for the
    literal-run loop (why: "K" the step limit, "token" an entry that is no primary-table literal, "margin" an entry
    within MARGIN bits of lim) and ("tok", kind, at, split) for the general step after it."""
    K = litrun_k() if K is None else K
    b = case.blocks[case.k]
    sim = G.Sim(case.comp, b.code)
    nb = 8 * len(case.comp)
    pos, end = lane_span(case, j)
    lim = min(end, nb - min(nb, TAIL))
    ev = []
    while pos < end:
        if pos < lim:
            p0, steps, why = pos, 0, "K"
            while steps < K:
                _, kind, l1 = sim.one(pos)
                if not (kind == "L" and l1 <= LB):
                    why = "token"
                    break
                if not pos + MARGIN < lim:
                    why = "margin"
                    break
                nxt, kind, _, split = sim.step(pos, end)
                assert kind == "L" and not split and nxt < lim
                pos = nxt
                steps += 1
            ev.append(("run", steps, why, p0, pos))
        nxt, kind, _, split = sim.step(pos, end)
        ev.append(("tok", kind, pos, split))
        pos = nxt
        if kind in "EB":
            break
    return ev


# ---- the cases ----------------------------------------------------------------------------------------------------
PER = 32 * G.LPW                        # a full round's lane segment
N_LANES = [4, 8, 12, 16, 20]


def n_steps():
    K = litrun_k()
    return [K - 1, K, K + 1, 2 * K + 1]


def _stream(c, idx, seed, prelude=True):
    return G.Stream(c, G.D0_MODS[idx % 5], 0x11700 + 64 * idx + seed, prelude=prelude)


def _retry(build, ok=lambda c: True):
    for seed in range(50):
        c = build(seed)
        if G.clean(c) and ok(c):
            return c
    raise AssertionError(c.name)


# (the deferred one: 120 bytes back from at most 2K + 2 bytes into the lane; distances 129..16384 have no code)
TERMS = {"dist1": ("M", 140, 1), "deferred": ("M", 258, 120), "lit15": ("L", Z15), "slowdist": ("M", 3, 24577 + 99)}


def _family_n():
    res = []
    c = code()
    idx = 0
    for term, tok in TERMS.items():
        for pair_last in (False, True):
            steps = ([0] if term == "dist1" and not pair_last else []) + n_steps()

            def build(seed):
                st = _stream(c, idx, seed)
                b = st.builder(c, False, bulk=BULK)
                cells = []
                for lane, n in zip(N_LANES, steps):
                    at = b.d0 + lane * PER
                    b.fill_to(at)
                    for t in run_tokens(n, pair_last):
                        b.put(t)
                    cells.append((lane, n, at, b.put(tok)))
                    b.put(("L", G9))
                b.fill_to(b.d0 + G.rspan(1) + 300)
                st.add(b.close())
                G.tail_blocks(st, "fixed")
                return G.finish(f"N_{term}_{'pair' if pair_last else 'single'}", "N", st.w, st.blocks, 1,
                                {"term": term, "pair_last": pair_last, "cells": cells}, st.k)
            res.append(_retry(build))
            idx += 1
    # ended by the end of block: one round of pw = LPW that the block does not fill, the run in its last live lane
    for n in n_steps():
        def build(seed):
            st = _stream(c, idx, seed)
            b = st.builder(c, False, bulk=BULK)
            lane = 60
            at = b.d0 + lane * PER
            b.fill_to(at)
            for t in run_tokens(n, False):
                b.put(t)
            st.add(b.close())
            G.tail_blocks(st, "stored")                     # (the input's last 48 bits lie past the block's end)
            return G.finish(f"N_eob_{n}", "N", st.w, st.blocks, 1,
                            {"term": "eob", "pair_last": False, "cells": [(lane, n, at, b.starts[-1])]}, st.k)
        res.append(_retry(build, lambda c: first_round(c)[1].pw == G.LPW))
        idx += 1
    return res


def _family_o():
    res = []
    idx = 100
    for variant, offs in (("A", [o for o in range(MARGIN + 1) if o != 4]), ("B", [4])):
        c = code(variant)
        for kind in ("single", "pair"):
            def build(seed):
                st = _stream(c, idx, seed)
                b = st.builder(c, False, bulk=BULK)
                cells = []
                for i, off in enumerate(offs):
                    lane = 2 + 2 * i
                    e = b.d0 + (lane + 1) * PER             # the lane's nominal end
                    lit = [("L", H10)] if kind == "single" else [("L", A2), ("L", B3)]
                    w = sum(c.width(t) for t in lit)
                    # the literal ends on the nominal end itself (off 0), else one bit before it: the token after
                    # it, off bits wide, is then the one that crosses the nominal end
                    p = e if off == 0 else e - 1
                    b.fill_to(p - w - 10)
                    b.put(("L", H10))                       # (nothing before the literal pairs with it)
                    at = b.pos
                    for t in lit:
                        b.put(t)
                    assert b.pos == p
                    if off:
                        b.put(tail_token(c, off))
                    b.put(("L", H10))
                    cells.append((lane, off, at, p))
                b.fill_to(b.d0 + G.rspan(1) + 300)
                st.add(b.close())
                G.tail_blocks(st, "fixed")
                return G.finish(f"O_{kind}_{variant}", "O", st.w, st.blocks, 1, {"kind": kind, "cells": cells}, st.k)
            res.append(_retry(build))
            idx += 1
    # the pair (A2, B3) of the primary table with the lane's end between its two literals
    c = code()

    def build(seed):
        st = _stream(c, idx, seed)
        b = st.builder(c, False, bulk=BULK)
        cells = []
        for lane in (3, 40):
            e = b.d0 + (lane + 1) * PER
            b.fill_to(e - 12)
            b.put(("L", H10))
            at = b.put(("L", A2))
            b.put(("L", B3))
            b.put(("L", H10))
            cells.append((lane, 0, at, e))
        b.fill_to(b.d0 + G.rspan(1) + 300)
        st.add(b.close())
        G.tail_blocks(st, "fixed")
        return G.finish("O_pair_split", "O", st.w, st.blocks, 1, {"kind": "split", "cells": cells}, st.k)
    res.append(_retry(build))
    return res


def _family_t():
    c = code()

    def build(seed):
        st = _stream(c, 200, seed)
        b = st.builder(c, True, bulk=BULK)
        b.fill_to(b.d0 + 9000)
        for i in range(12):                                 # (the last 48 bits: literals, then the end of block)
            b.put(("L", RUN[i % 3]))
        st.add(b.close())
        return st
    for seed in range(50):
        st = build(seed)
        whole = G.finish("T_run_to_end", "T", st.w, st.blocks, 1, {}, st.k)
        if G.clean(whole):
            break
    else:
        raise AssertionError(whole.name)
    cut = (st.blocks[st.k].d0 + 4000) // 8
    return [whole, G.finish("T_cut_in_run", "T", st.w, st.blocks, 1, {"cut": cut}, st.k, cut=cut)]


@functools.lru_cache(maxsize=None)
def match_code():
    """(258, d) in 1 + 1 bits, (3, d) in 2 + 1, the end of block in 2; d = 1, 2."""
    lens = [0] * 286
    lens[285], lens[257], lens[256] = 1, 2, 2
    return G.Code("matches", lens, [1, 1])


def _family_m():
    c = match_code()
    st = G.Stream(c, 13, 0, prelude=False)
    b = st.builder(c, False, bulk=[])
    for i in range(230):
        b.put(("M", 258 if i % 3 else 3, 1 + i % 2))
    st.add(b.close())
    G.tail_blocks(st, "fixed")
    return [G.finish("M_matches_only", "M", st.w, st.blocks, 1, {}, st.k)]


def _family_p():
    res = []
    # TP_LIT8: 192 literals of 8 bits; four-literal steps, a 3-bit literal now and then, dist-1 runs after them
    c = G.phased_code(192)
    lits = [s for s in range(256) if c.lit[s] == 8]

    def build8(seed):
        st = _stream(c, 300, seed)
        b = st.builder(c, False, bulk=[])
        at = []
        for i in range(90):
            for _ in range(5 + (7 * i) % 23):
                b.put(("L", st.rng.choice(lits)))
            if i % 3 == 0:
                b.put(("L", G.P_LIT3))
            at.append(b.put(("M", 3, 1)))
        G._fill8(b, b.pos + 8 * 700, lits)
        st.add(b.close())
        G.tail_blocks(st, "fixed")
        return G.finish("P_lit8_dist1", "P", st.w, st.blocks, 1, {"at": at, "n8": 192}, st.k)
    res.append(_retry(build8))
    # escape prefix: 254 literals of 8 bits, the rest under 1111111; eight-literal steps to the first escape byte
    kc = G.k_code()

    def builde(seed):
        st = G.Stream(kc, 8 * (seed % 4), 0x11A00 + seed)
        b = st.builder(kc, False, bulk=[])
        at = []
        for i in range(90):
            for _ in range(3 + (5 * i) % 29):
                b.put(("L", st.rng.randrange(254)))
            if i % 4 == 0:
                b.put(("L", 255))                           # (a 9-bit literal under the escape prefix)
            at.append(b.put(("M", 131 + i % 32, 1)))
        for _ in range(900):
            b.put(("L", st.rng.randrange(254)))
        st.add(b.close())
        G.tail_blocks(st, "fixed")
        return G.finish("P_escape_dist1", "P", st.w, st.blocks, 1, {"at": at, "n8": 254}, st.k)
    res.append(_retry(builde))
    return res


RSV_LEN, RSV_DIST = "RESERVED_LENGTH_SYMBOL", "RESERVED_DISTANCE_SYMBOL"


def _family_e():
    res = []
    E_LANE = 7

    def lead(c, idx, seed, prelude=True):
        """A block of code c up to a literal run of three steps at lane E_LANE's entry."""
        st = _stream(c, idx, seed, prelude)
        b = st.builder(c, True, bulk=BULK)
        b.fill_to(b.d0 + E_LANE * PER)
        for t in run_tokens(3, False):
            b.put(t)
        return st, b

    def done(name, st, b, reason, upto):
        b.fill_to(b.pos + 2 * PER + G.rspan(1))
        st.add(b.close())
        return G.finish(name, "E", st.w, st.blocks, 1, {"lane": E_LANE, "reason": reason}, st.k, reason=reason, upto=upto)

    # a length code under the empty distance code
    def b_empty(seed):
        st, b = lead(code("A", None), 400, seed, prelude=False)
        upto = len(b.tokens)
        b.put(("X", 285, 0))
        return done("E_empty_dist", st, b, G.EMPTY_DIST, upto)
    res.append(_retry(b_empty))

    # a distance symbol of 30: (258, symbol 30) written by hand -- the length code, then the symbol's 5-bit code
    def b_rsv_dist(seed):
        c = code("A", "rsv")
        st, b = lead(c, 401, seed)
        upto = len(b.tokens)
        b.starts.append(b.pos)
        b.tokens.append(("L", 0))                           # (a placeholder: never expanded, upto stops before it)
        b.w.bits(*c.lc[285])
        b.w.bits(*c.dc[30])
        return done("E_reserved_dist", st, b, RSV_DIST, upto)
    res.append(_retry(b_rsv_dist))

    # a copy from before the output's start: no prelude, a distance far past the few hundred bytes so far
    def b_before(seed):
        st, b = lead(code(), 402, seed, prelude=False)
        upto = len(b.tokens)
        assert len(TS.expand([x.tokens for x in st.blocks] + [b.tokens])[1]) < 24577
        b.put(("M", 3, 24577))
        return done("E_copy_before", st, b, TS.COPY_BEFORE, upto)
    res.append(_retry(b_before))

    # the reserved length symbol 286: only the fixed code has it; a fixed block of three rounds' worth of literals
    w = TS.BitWriter()
    rng = random.Random(0xE286)
    toks = [("L", rng.randrange(144)) for _ in range(5000)]
    TS.write_block(w, toks + [("R", 286)] + toks[:400], "fixed", True)
    comp = w.getbytes()
    res.append(G.Case("E_reserved_len", "E", comp, [], RSV_LEN, bytes(t[1] for t in toks), None, 1,
                      {"reason": RSV_LEN}, 0))
    return res


_BUILDERS = {"N": _family_n, "O": _family_o, "T": _family_t, "M": _family_m, "P": _family_p, "E": _family_e}
FAMILIES = list(_BUILDERS)
COUNTS = {"N": 12, "O": 5, "T": 2, "M": 1, "P": 2, "E": 4}


@functools.lru_cache(maxsize=None)
def cases(name):
    return _BUILDERS[name]()
