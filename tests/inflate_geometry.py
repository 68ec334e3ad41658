"""Hand-placed token streams for the decoder's count pass at its round, segment and checkpoint limits.

The count pass (csrc/hip/inflate_wave.hpp: ndfl_inflate_count_wave_kernel, round_decode, round_decode_phased;
inflate_wg.hpp for W waves per chain) cuts a Huffman block into rounds of at most RSPAN_W = 64 W LPW 32 bits, a
round into 64 W lane segments of seg_pw() words, decodes every segment speculatively and re-decodes it from the
true entry until the decode stands on a recorded checkpoint (XCP1 / XCP2 bits into the segment, or its end).  Every
one of these has an edge at an exact bit position, and no stream written by an encoder chooses where its tokens
fall.  This module writes blocks from explicit code lengths, token by token, with every token's start bit known:

    Code(lit, dist)                    explicit code lengths; the Kraft sums are checked in integers
    Builder(w, code, final)            a dynamic block under construction: put(token), fill_to(bit), close()
    Stream(code, mod, seed)            shim (fixed block) + prelude (a window of 33,541 bytes) + blocks
    token_stream.expand                the expected bytes (shares no code with the oracle or the library)

and restates the round geometry on the host (the model):

    seg_pw / geo / seg                 inflate_records.hpp seg_pw, seg_start, seg_end; make_geo (base = rs & ~31)
    all_rounds / tested_rounds         the round loop of the count kernels for the true decode: E = min(first
                                       candidate after rs, limit, rs + RSPAN_W), the next round starts at the last
                                       lane's exit, a block ends in the round where its end of block starts
    Sim                                families C and P only: tok<true>'s pair split, spec_run / verify_run (a
                                       lane's first verify starts from its predecessor's SPECULATIVE exit) and the
                                       count of lanes that do not synchronise (nslow), phase_of's entry match

Families (cases(name)): R round ends, S segment ends, C checkpoints, T input tail, P phase-mapped rounds, K false
header candidates inside a Huffman block.  Every stream is a fixed-Huffman shim (it sets the tested block's first
data bit mod 32), where distances need one a prelude block (a 33,541-byte window), the block under test, and what
the case says follows it.  The table forms: long literal/length codes in second-level tables throughout, distance
codes on the canonical slow path ("slow": the 48-bit token needs a 15-bit distance code, which only that form
holds) and in second-level tables ("two": the widest token is then 46 bits).

Not built: a literal/length code on the canonical slow path (more than 320 extension words take nearly 286 long
codes); family P's overhang of 47 bits (a candidate one bit into a 48-bit token needs a zero as the second bit
of a 15-bit code, and a complete code's 15-bit codes are its last values: they begin with ones) and family P at
W = 4.  The last lane of a short round ends where the block ends unless the input ends there: family S's cases
for it are truncated streams.  The nslow cases of family C are built for W = 1.
Test infrastructure only.
"""
import bisect
import collections
import functools
import random

import oracle_lib as O
import pyref_deflate as P
import token_stream as TS

# ---- the decoder's constants (test_inflate_geometry_cpu reads the defaults out of the headers) ---------------
LPW, PW_MIN, XCP1, XCP2, TAIL = 14, 4, 64, 192, 48
PH_FALLBACK, PH_FRONTIER, PHASE_SWITCH, LB, DB, N8_PHASED = 8, 4, 48, 10, 8, 192
EMPTY_DIST = "LENGTH_ENCOUNTERED_WITH_EMPTY_DISTANCE_CODE"
UEOS = "UNEXPECTED_END_OF_STREAM"
MAX_COMP, MAX_OUT = 64 << 10, 4 << 20


def rspan(W):
    return 64 * W * LPW * 32


def seg_pw(span, nl=64):
    pw = ((span + nl - 1) // nl + 31) // 32
    return max(pw, PW_MIN)


Geo = collections.namedtuple("Geo", "rs E base r0 re pw per nl")


def geo(rs, E, W=1):
    base = rs & ~31
    pw = seg_pw(E - rs, 64 * W)
    return Geo(rs, E, base, rs - base, E - base, pw, 32 * pw, 64 * W)


def seg(g, j):
    """Lane j's nominal segment [s, e) in absolute bits; the last lane ends at the round end."""
    s = min(g.rs + j * g.per, g.E)
    e = g.E if j == g.nl - 1 else min(g.rs + (j + 1) * g.per, g.E)
    return s, e


# ---- codes ----------------------------------------------------------------------------------------------------
def kraft(lens):
    """The Kraft sum in units of 2^-15 (a complete code: 1 << 15)."""
    return sum(1 << (15 - l) for l in lens if l)


class Code:
    """Explicit code lengths.  lit: 286 lengths; dist: up to 30 lengths, or None for the empty distance code (one
    length of zero)."""

    def __init__(self, name, lit, dist):
        assert len(lit) in (286, 288) and lit[256] and (dist is None or 2 <= len(dist) <= 32)
        assert kraft(lit) == 1 << 15, (name, kraft(lit))
        assert dist is None or kraft(dist) == 1 << 15, (name, kraft(dist))
        self.name, self.lit, self.dist = name, list(lit), None if dist is None else list(dist)
        self.lc = P.canonical(self.lit, 15)
        self.dc = None if dist is None else P.canonical(self.dist, 15)
        self.ldec = {(l, c): s for s, (c, l) in ((s, x) for s, x in enumerate(self.lc) if x)}
        self.ddec = {} if dist is None else {(l, c): s for s, (c, l) in ((s, x) for s, x in enumerate(self.dc) if x)}
        self.lmin = min(l for l in lit if l)
        self.dmin = 0 if dist is None else min(l for l in dist if l)
        self.hdr_bits = 17 + 3 * 19 + 4 * (286 + (1 if dist is None else len(self.dist)))
        self.n8 = sum(1 for l in lit if l == 8)

    def width(self, t):
        if t[0] == "L":
            return self.lc[t[1]][1]
        if t[0] == "X":
            return self.lc[t[1]][1] + LEN_EXTRA[t[1] - 257]
        (ls, lne, _), (ds, dne, _) = P.len_sym(t[1]), P.dist_sym(t[2])
        return self.lc[ls][1] + lne + self.dc[ds][1] + dne


LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]


@functools.lru_cache(maxsize=None)
def fixed_code():
    return Code("fixed", P.STATIC_LIT_LENS, [5] * 32)


def complete(fixed, lmin, nsym=286):
    """286 literal/length lengths with fixed[sym] = length and the rest of the code space given to unused
    symbols (literals first, from 255 down, then length symbols), the largest pieces first, none shorter than
    lmin bits."""
    lens = [0] * nsym
    for s, l in fixed.items():
        lens[s] = l
    rem = (1 << 15) - kraft(lens)
    free = [s for s in list(range(255, -1, -1)) + list(range(258, nsym)) if s not in fixed]
    assert rem >= 0
    for l in range(lmin, 16):
        unit = 1 << (15 - l)
        while rem >= unit:
            lens[free.pop(0)] = l
            rem -= unit
    assert rem == 0
    return lens


def dist_lens(multiset, pinned):
    """30 distance lengths: pinned[sym] = length, the other lengths of the multiset to the lowest free symbols."""
    rest = sorted(multiset)
    for l in pinned.values():
        rest.remove(l)
    lens = [0] * 30
    for s, l in pinned.items():
        lens[s] = l
    free = [s for s in range(30) if s not in pinned]
    for l in rest:
        lens[free.pop(0)] = l
    return lens


A2, B3, Z15 = 0x61, 0x62, 0x5A           # the filler literals of 2 and 3 bits, the 15-bit literal
D_SLOW = dist_lens(list(range(1, 15)) + [15, 15], {0: 1, 10: 7, 28: 15, 29: 15})    # canonical slow path (128 > 64)
D_TWO = dist_lens(list(range(1, 13)) + [13, 13], {0: 1, 10: 7, 28: 13, 29: 13})     # second-level tables


@functools.lru_cache(maxsize=None)
def general_code(eobw, form="slow", need_one=True):
    """Filler literals of 2 and 3 bits, a 15-bit literal, (258, 1) at 4 + 1 bits, 15-bit length codes with 0 and 5
    extra bits, the end of block in eobw bits with a last bit of 1; the long literal/length codes go to
    second-level tables.  form "slow": distance codes 1..14, 15, 15 (the canonical slow path: the big token has
    48 bits); "two": 1..12, 13, 13 (second-level tables: 46 bits)."""
    base = {A2: 2, B3: 3, 285: 4, Z15: 15, 257: 15, 281: 15, 256: eobw}
    # (the end of block's last bit is 1 -- no stored header after it is found a bit early -- when an odd number
    # of literals share its length: the variants move it by one place in its class)
    for extra in ({}, {0x63: eobw}, {258: 15}, {0x63: eobw, 258: 15}, {258: 15, 259: 15}):
        fixed = {**base, **extra}
        for lmin in range(12, 3, -1):
            try:
                lens = complete(fixed, lmin)
                break
            except IndexError:
                continue
        else:
            continue
        c = Code(f"general_eob{eobw}_{form}", lens, D_SLOW if form == "slow" else D_TWO)
        cc, l = c.lc[256]
        if cc >> (l - 1) & 1 or not need_one:
            return c
    raise AssertionError(eobw)


def big_token(code, rng=None):
    """The widest match of a general code: 15-bit length code + 5 extra + the longest distance code + 13 extra."""
    x = rng.randrange(32) if rng else 0
    y = rng.randrange(8192) if rng else 0
    return ("M", 131 + x, 24577 + y)


def token_of_width(code, w, rng=None):
    big = code.width(big_token(code))
    if w == big:
        return big_token(code, rng)
    t = {2: ("L", A2), 3: ("L", B3), 15: ("L", Z15), 16: ("M", 3, 1),
         31: ("M", 131 + (rng.randrange(32) if rng else 0), 33 + (rng.randrange(16) if rng else 0))}[w]
    assert code.width(t) == w, (code.name, t, w)
    return t


# ---- the block writer -----------------------------------------------------------------------------------------
Blk = collections.namedtuple("Blk", "kind hdr d0 starts end final code tokens")
Blk.__doc__ = """One written block: hdr its BFINAL bit, d0 its first data bit, starts every token's start bit (a Huffman
block: the end of block's last), end the bit after it."""


def write_dynamic_header(w, code, final):
    """Every length sent as a plain code-length symbol under a 4-bit code-length code (symbols 0..15)."""
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    nd = 1 if code.dist is None else len(code.dist)
    w.bits(286 - 257, 5)
    w.bits(nd - 1, 5)
    w.bits(19 - 4, 4)
    for s in P.CLC_ORDER:
        w.bits(4 if s < 16 else 0, 3)
    for l in code.lit + ([0] if code.dist is None else code.dist):
        w.bits(int(format(l, "04b")[::-1], 2), 4)


class Builder:
    """A dynamic block under construction on the BitWriter w; pos is the next token's start bit."""

    def __init__(self, w, code, final, rng, bulk=None):
        self.w, self.code, self.final, self.rng = w, code, final, rng
        self.hdr = w.n
        write_dynamic_header(w, code, final)
        assert w.n - self.hdr == code.hdr_bits
        self.d0 = w.n
        self.tokens, self.starts = [], []
        # the bulk filler: literals of 9..13 bits (random: a reseed moves every bit after it)
        self.bulk = bulk if bulk is not None else [s for s in range(256) if 9 <= code.lit[s] <= 13]

    @property
    def pos(self):
        return self.w.n

    def _enc(self, t):
        """The token's bits as [(value, width)] pieces of at most 31 bits (one piece where it fits)."""
        c = self.code
        if t[0] == "L":
            return [c.lc[t[1]]]
        if t[0] == "X":
            cc, l = c.lc[t[1]]
            return [(cc | t[2] << l, l + LEN_EXTRA[t[1] - 257])]
        (ls, lne, lex), (ds, dne, dex) = P.len_sym(t[1]), P.dist_sym(t[2])
        cc, l = c.lc[ls]
        dc, dl = c.dc[ds]
        a, b = (cc | lex << l, l + lne), (dc | dex << dl, dl + dne)
        return [(a[0] | b[0] << a[1], a[1] + b[1])] if a[1] + b[1] <= 31 else [a, b]

    def put(self, t):
        self.starts.append(self.w.n)
        self.tokens.append(t)
        for v, n in self._enc(t):
            self.w.bits(v, n)
        return self.starts[-1]

    def repeat(self, t, n):
        """n copies of token t (a short one goes out several to a write)."""
        enc = self._enc(t)
        width = sum(x[1] for x in enc)
        pos = self.w.n
        self.starts.extend(range(pos, pos + n * width, width))
        self.tokens.extend([t] * n)
        if len(enc) == 1 and 2 * width <= 31:
            k = 31 // width
            v = sum(enc[0][0] << (i * width) for i in range(k))
            for _ in range(n // k):
                self.w.bits(v, k * width)
            n %= k
        for _ in range(n):
            for v, nb in enc:
                self.w.bits(v, nb)

    def fill_to(self, target):
        """Filler literals up to exactly bit `target`: codes of 2 and 3 bits reach any amount of 2 or more."""
        r = target - self.pos
        assert r == 0 or r >= 2, (target, self.pos)
        while target - self.pos > 40 and self.bulk:
            self.put(("L", self.rng.choice(self.bulk)))
        r = target - self.pos
        if r & 1:
            self.put(("L", B3))
            r -= 3
        for _ in range(r // 2):
            self.put(("L", A2))
        assert self.pos == target

    def place(self, target, t):
        """Token t with its start on bit `target`."""
        self.fill_to(target)
        return self.put(t)

    def close(self):
        self.starts.append(self.w.n)
        self.w.bits(*self.code.lc[256])
        return Blk("dynamic", self.hdr, self.d0, self.starts, self.w.n, self.final, self.code, self.tokens)


def write_fixed(w, tokens, final):
    hdr = w.n
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    d0 = w.n
    lc, _ = TS._fixed_codes()
    starts = []
    for t in tokens:
        assert t[0] == "L"
        starts.append(w.n)
        w.bits(*lc[t[1]])
    starts.append(w.n)
    w.bits(*lc[256])
    return Blk("fixed", hdr, d0, starts, w.n, final, None, list(tokens))


def write_stored(w, data, final):
    hdr = w.n
    TS.write_block(w, [("L", b) for b in data], "stored", final)
    return Blk("stored", hdr, w.n - 8 * len(data), [], w.n, final, None, [("L", b) for b in data])


D0_MODS = [0, 1, 31, 13, 22]            # the tested block's first data bit mod 32


def shim_tokens(mod, rest_bits):
    """Fixed-Huffman literals, 8- and 9-bit ones mixed, so that 3 + 8 a + 9 b + 7 + rest_bits = mod (mod 32)."""
    for n in range(2, 40):
        for b in range(1, n):
            a = n - b
            if (3 + 8 * a + 9 * b + 7 + rest_bits) % 32 == mod:
                return [("L", 65 + i) for i in range(a)] + [("L", 200 + i) for i in range(b)]
    raise AssertionError(mod)


PRELUDE_COPIES = 130                    # 1 + 130 * 258 = 33,541 bytes: every distance has a source


def write_prelude(w, code):
    """A non-final dynamic block of one literal and 130 (258, 1) copies: the window of the blocks after it."""
    b = Builder(w, code, False, None, bulk=[])
    b.put(("L", A2))
    b.repeat(("M", 258, 1), PRELUDE_COPIES)
    return b.close()


def prelude_bits(code):
    return code.hdr_bits + 2 + PRELUDE_COPIES * 5 + code.lc[256][1]


Case = collections.namedtuple("Case", "name family comp blocks reason out bits W info k")
Case.__doc__ = """One stream.  blocks: [Blk] in stream order; reason / out: token_stream.expand of the tokens (an error case:
set by its builder); bits: the consumed bits (None where the Reason is not None); W: the count width the geometry
is targeted at (None: none); info: what the case is named for (checked against the model on the CPU); k: the index
of the block under test."""


def finish(name, family, w, blocks, W, info, k, reason=None, upto=None, trailing=b"", cut=None):
    """The case of the written stream.  reason / upto: an error case ends with `reason` before token `upto` of
    block k; trailing: bytes after the final block; cut: the stream truncated to `cut` bytes (the expectation is
    UNEXPECTED_END_OF_STREAM after the tokens that lie wholly inside it)."""
    comp = w.getbytes() + trailing
    bits = blocks[-1].end
    toks = [b.tokens for b in blocks]
    if reason is not None:
        toks = toks[:k] + [toks[k][:upto]]
        bits = None
    r, out = TS.expand(toks)
    assert r is None
    if cut is not None:
        # the tokens that lie wholly inside the cut input, then UNEXPECTED_END_OF_STREAM
        comp = comp[:cut]
        b = blocks[k]
        assert b.d0 < 8 * cut < b.end
        n = sum(1 for e in b.starts[1:] if e <= 8 * cut)
        r, out = TS.expand([x.tokens for x in blocks[:k]] + [b.tokens[:n]])
        reason, bits = UEOS, None
    assert len(comp) <= MAX_COMP and len(out) <= MAX_OUT, (name, len(comp), len(out))
    return Case(name, family, comp, blocks, reason, out, bits, W, info, k)


class Stream:
    """shim + prelude + the block under test at a chosen first data bit mod 32."""

    def __init__(self, code, mod, seed, prelude=True):
        self.w = TS.BitWriter()
        self.rng = random.Random(seed)
        pre = general_code(15)
        rest = (prelude_bits(pre) if prelude else 0) + code.hdr_bits
        self.blocks = [write_fixed(self.w, shim_tokens(mod, rest), False)]
        if prelude:
            self.blocks.append(write_prelude(self.w, pre))
        self.k = len(self.blocks)

    def builder(self, code, final, bulk=None):
        return Builder(self.w, code, final, self.rng, bulk)

    def add(self, blk):
        self.blocks.append(blk)
        return blk


def tail_blocks(st, follow):
    """What follows the block under test: "nothing" (it was final), "fixed" (a final fixed block), "stored" (a
    non-final stored block -- its header is a candidate -- and a final fixed block)."""
    if follow == "stored":
        st.add(write_stored(st.w, b"\xff\xff\xff", False))
    if follow in ("fixed", "stored"):
        st.add(write_fixed(st.w, [("L", 0x21), ("L", 0xF0)], True))


# ---- the model: candidates, chains and rounds -------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def candidates(comp):
    """The count pass's chain starts: bit 0 and the header finder's candidates (oracle_lib.scan_headers)."""
    return tuple(sorted({0} | set(O.scan_headers(comp))))


def _stored_key(comp, p):
    h = (int.from_bytes(comp[p >> 3:(p >> 3) + 2], "little") >> (p & 7)) & 7
    if h >> 1 or p + 3 > 8 * len(comp):
        return None
    return ((p + 3 + 7) & ~7, h & 1)


def counted(comp, cands):
    """The candidates whose chains are counted: a stored header's aliases (the same LEN position and BFINAL bit
    read a few bits earlier or later) take the first one's result (ndfl_inflate_alias_mark_kernel)."""
    res = []
    for k, p in enumerate(cands):
        key, rep, j = _stored_key(comp, p), k, k
        if key is not None:
            while j > 0 and cands[j - 1] + 10 >= p:
                if _stored_key(comp, cands[j - 1]) == key:
                    rep = j - 1
                j -= 1
        if rep == k:
            res.append(p)
    return res


def real_headers(case):
    """The block headers a finder may report (non-final stored and dynamic ones) and the aliases of the stored."""
    real, alias = set(), set()
    nb = 8 * len(case.comp)
    bit = lambda q: case.comp[q >> 3] >> (q & 7) & 1
    for b in case.blocks:
        if b.final or b.kind == "fixed" or b.hdr + 3 > nb:
            continue
        real.add(b.hdr)
        if b.kind == "stored":
            al = (b.hdr + 3 + 7) & ~7
            for q in range(max(0, al - 10), al - 2):
                if (q + 3 + 7) & ~7 == al and all(not bit(x) for x in range(q, al)):
                    alias.add(q)
    return real, alias - real


Round = collections.namedtuple("Round", "blk rs E exit done")
Round.__doc__ = """One round of block index blk: [rs, E), exit = the last lane's exit (the next round's start; the block's end
when done)."""


def chain_rounds(case, start, cands, W):
    """The rounds of the chain that starts at the real header `start`, as the count kernels' round loop makes
    them from the true token starts.  In a truncated stream the first token that ends past the input ends the
    decode as the end of block does."""
    limit = 8 * len(case.comp)
    i = next(i for i, b in enumerate(case.blocks) if b.hdr == start)
    res = []
    for n, b in enumerate(case.blocks[i:]):
        if n and b.hdr in cands:
            break
        if b.kind != "stored":
            rs, ends = b.d0, b.starts[1:] + [b.end]
            eob = b.starts[min(bisect.bisect_right(ends, limit), len(ends) - 1)]    # (or the token cut by the end)
            while True:
                ci = bisect.bisect_right(cands, rs)
                nxt = cands[ci] if ci < len(cands) else limit
                E = max(min(nxt, limit, rs + rspan(W)), rs + 1)
                if eob < E:
                    res.append(Round(i + n, rs, E, b.end, True))
                    break
                ex = b.starts[bisect.bisect_left(b.starts, E)]
                res.append(Round(i + n, rs, E, ex, False))
                rs = ex
        if b.final or b.end > limit:
            break
    return res


def all_rounds(case, W):
    """Every counted chain's rounds (a chain that starts at a false candidate: None)."""
    cands = candidates(case.comp)
    heads = {b.hdr for b in case.blocks}
    return [chain_rounds(case, c, cands, W) if c in heads else None for c in counted(case.comp, cands)]


def tested_rounds(case, W):
    """The rounds of the block under test (its chain starts at its header, or at bit 0 when it is final)."""
    cands = candidates(case.comp)
    b = case.blocks[case.k]
    start = b.hdr if b.hdr in cands else max(c for c in cands if c <= b.hdr)
    return [r for r in chain_rounds(case, start, cands, W) if r.blk == case.k]


# ---- the model: tokens, speculation and verification (families C and P) -------------------------------------------
class Sim:
    """The token decoder of one block over the stream's bits, with tok<true>'s rules: a literal pair (two literal
    codes of at most LB bits together) is one step unless its first literal reaches `stop` or the pair the
    input's end; a token that ends past the input is the end of the decode."""

    def __init__(self, comp, code):
        self.data = bytes(comp) + bytes(32)
        self.nb = 8 * len(comp)
        self.code = code

    def peek(self, pos):
        b = pos >> 3
        return int.from_bytes(self.data[b:b + 5], "little") >> (pos & 7)

    def _sym(self, pos, dec, lmin):
        v = self.peek(pos)
        for l in range(lmin, 16):
            s = dec.get((l, v & ((1 << l) - 1)))
            if s is not None:
                return s, l
        raise AssertionError("incomplete code")

    def one(self, pos):
        """A single token at pos: (end, kind, first code length); kind "L", "M", "E" (end of block), "B" (error)."""
        c = self.code
        s, l = self._sym(pos, c.ldec, c.lmin)
        if s < 256:
            return pos + l, "L" if pos + l <= self.nb else "B", l
        if s == 256:
            return pos + l, "E" if pos + l <= self.nb else "B", l
        if s > 285:
            return pos + l, "B", l
        end = pos + l + LEN_EXTRA[s - 257]
        if end > self.nb or c.dist is None:
            return end, "B", l
        ds, dl = self._sym(end, c.ddec, c.dmin)
        if ds > 29:
            return end + dl, "B", l
        end += dl + DIST_EXTRA[ds]
        return end, "M" if end <= self.nb else "B", l

    def step(self, pos, stop):
        """One step of tok<true> / tok_bb<true>: (end, kind, tokens in the step, split): split = a pair that the
        table holds was cut because its first literal reaches stop."""
        end, kind, l1 = self.one(pos)
        if kind != "L" or l1 >= LB:
            return end, kind, 1, False
        s2, l2 = self._sym(end, self.code.ldec, self.code.lmin)
        if s2 >= 256 or l1 + l2 > LB:                  # (no pair in the primary table)
            return end, kind, 1, False
        if pos + l1 < stop and pos + l1 + l2 <= self.nb:
            return end + l2, "L", 2, False
        return end, kind, 1, not pos + l1 < stop

    def run_to(self, pos, stop):
        """run_to: (pos, terminal)."""
        while pos < stop:
            pos, kind, _, _ = self.step(pos, stop)
            if kind in "EB":
                return pos, True
        return pos, False

    def spec(self, st, C1, C2, e):
        """spec_run: (end, terminal, cp1, cp2): the first token boundary at or past each checkpoint (None: the run
        ended before it)."""
        pos, cp1, cp2 = st, None, None
        pos, term = self.run_to(pos, C1)
        if term:
            return pos, True, cp1, cp2
        cp1 = pos
        if pos < C2:
            pos, term = self.run_to(pos, C2)
            if term:
                return pos, True, cp1, cp2
        cp2 = pos
        pos, term = self.run_to(pos, e)
        return pos, term, cp1, cp2

    def verify(self, t0, C1, C2, e, p0):
        """verify_run without phase runs: (synchronised, end, terminal)."""
        pend, pterm, cp1, cp2 = p0
        pos, term = self.run_to(t0, C1)
        if term:
            return False, pos, True
        if cp1 == pos:
            return True, pend, pterm
        if pos < C2:
            pos, term = self.run_to(pos, C2)
            if term:
                return False, pos, True
        if cp2 == pos:
            return True, pend, pterm
        pos, term = self.run_to(pos, e)
        if term:
            return False, pos, True
        return pos == pend and not pterm, pos, False

    def round_nslow(self, rs, E, W=1):
        """The lanes of the round [rs, E) whose first verify does not synchronise, as round_decode (W = 1: up to
        the first lane whose speculation ended the block) and round_decode_wg (per wave) count them:
        (nslow, [lane])."""
        g = geo(rs, E, W)
        sp, fin, term = [], [], []
        for j in range(g.nl):
            s, e = seg(g, j)
            sp.append(self.spec(s, s + min(XCP1, e - s), s + min(XCP2, e - s), e))
        for j in range(g.nl):
            s, e = seg(g, j)
            if j == 0:
                fin.append(True)
                term.append(sp[0][1])
            else:
                f, _, t = self.verify(sp[j - 1][0], s + min(XCP1, e - s), s + min(XCP2, e - s), e, sp[j])
                fin.append(f)
                term.append(t)
        total, lanes = 0, []
        for wv in range(W):
            L = range(64 * wv, 64 * wv + 64)
            um = [j for j in L if not fin[j]]
            t0 = next((j for j in L if fin[j] and term[j]), 64 * wv + 64)
            if not um or um[0] >= t0:
                continue
            if W == 1:
                first_term = next((j for j in L if sp[j][1]), 63)
                um = [j for j in um if j <= first_term]
            total += len(um)
            lanes += um
        return total, lanes

    def phase_entry(self, g, j, entry):
        """phase_of for lane j entered at `entry`: (d, phase or None): d = entry - s_j; an entry with d < 8 is phase
        d, a later one the phase whose first token ends there (offsets under 255)."""
        s, e = seg(g, j)
        d = entry - s
        if d < 8:
            return d, d
        for f in range(8):
            if s + f < e:
                end, kind, _ = self.one(s + f)
                if kind in "LM" and end - s < 255 and end - s == d:
                    return d, f
        return d, None


def stat_rounds(case, W):
    """The count pass's `rounds` statistic: every counted chain's rounds (no chain may start at a false candidate)."""
    chains = all_rounds(case, W)
    assert None not in chains, case.name
    return sum(len(ch) for ch in chains)


def block_nslow(case, rounds, W=1):
    """[nslow] of one block's rounds: a block whose literal/length code has N8_PHASED lengths of 8 is phase-mapped
    from its first round, any other from the round after one with more than PHASE_SWITCH W such lanes (a
    phase-mapped round counts none)."""
    b = case.blocks[rounds[0].blk]
    code = fixed_code() if b.kind == "fixed" else b.code
    phased = sum(1 for l in code.lit if l == 8) >= N8_PHASED
    sim, res = Sim(case.comp, code), []
    for r in rounds:
        n = 0 if phased else sim.round_nslow(r.rs, r.E, W)[0]
        phased = phased or n > PHASE_SWITCH * W
        res.append(n)
    return res


def stat_nslow(case, W=1):
    """The count pass's `slow-verify lanes` statistic."""
    chains = all_rounds(case, W)
    assert None not in chains, case.name
    total = 0
    for ch in chains:
        for blk in sorted({r.blk for r in ch}):
            total += sum(block_nslow(case, [r for r in ch if r.blk == blk], W))
    return total


# ---- family R: round ends ---------------------------------------------------------------------------------------
def _full_rounds(b, W, n):
    """Fill block builder b through n - 1 full rounds (each exit two bits past its end); returns the n-th round's
    start."""
    rs = b.d0
    for _ in range(n - 1):
        b.fill_to(rs + rspan(W) - 1)
        b.put(("L", B3))
        rs = b.pos
    return rs


def _family_r():
    res = []
    idx = 0
    for W, forms in ((1, ("slow", "two")), (4, ("slow",))):
        for form in forms:
            code = general_code(15, form)
            big = code.width(big_token(code))
            for w in (2, 15, 16, 31, big):
                for k in sorted({1, w - 1, w, w + 1} - {0}):
                    n = 1 + idx % 3
                    for seed in range(50):
                        st = Stream(code, D0_MODS[idx % 5], 0x5200 + 64 * idx + seed)
                        b = st.builder(code, True)
                        rs = _full_rounds(b, W, n)
                        at = b.place(rs + rspan(W) - k, token_of_width(code, w, st.rng))
                        b.fill_to(b.pos + 2 * st.rng.randrange(40, 160))
                        st.add(b.close())
                        c = finish(f"R_token_W{W}_{form}_w{w}_k{k}_n{n}", "R", st.w, st.blocks, W,
                                   {"round": n - 1, "at": at, "w": w, "k": k}, st.k)
                        if clean(c):
                            break
                    else:
                        raise AssertionError(c.name)
                    res.append(c)
                    idx += 1
    # the last token ends exactly at a round end: the next round is the end-of-block code alone
    for W in (1, 4):
        for eobw in (1, 7, 15):
            for follow in ("nothing", "fixed", "stored"):
                code = l1_code() if eobw == 1 else general_code(eobw)
                for seed in range(50):
                    st = Stream(code, D0_MODS[idx % 5], 0x5300 + 64 * idx + seed, prelude=eobw != 1)
                    b = st.builder(code, follow == "nothing")
                    if eobw == 1:
                        b.repeat(("L", L1_LIT), rspan(W))
                    else:
                        b.fill_to(b.d0 + rspan(W) - 15)
                        b.put(("L", Z15))
                    st.add(b.close())
                    tail_blocks(st, follow)
                    c = finish(f"R_eob_alone_W{W}_eob{eobw}_{follow}", "R", st.w, st.blocks, W,
                               {"eobw": eobw, "follow": follow}, st.k)
                    if clean(c):
                        break
                else:
                    raise AssertionError(c.name)
                res.append(c)
                idx += 1
    # last rounds of a few bits: a full round of 1-bit literals, then span - 1 more and the 1-bit end of block,
    # ended by the stored header after it
    for W in (1, 4):
        for span in (1, 31, 32, 33, 127, 128, 129):
            code = l1_code()
            st = Stream(code, D0_MODS[idx % 5], 0x5400 + idx, prelude=False)
            b = st.builder(code, False)
            b.repeat(("L", L1_LIT), rspan(W) + span - 1)
            st.add(b.close())
            tail_blocks(st, "stored")
            c = finish(f"R_last_round_W{W}_span{span}", "R", st.w, st.blocks, W, {"span": span}, st.k)
            assert clean(c), c.name
            res.append(c)
            idx += 1
    return res


def clean(case):
    """No candidate other than the real interior headers (and the stored ones' aliases)."""
    real, alias = real_headers(case)
    return set(candidates(case.comp)) - {0} <= real | alias


L1_LIT = 0x55


@functools.lru_cache(maxsize=None)
def l1_code():
    """One literal and the end of block, 1 bit each ('0' and '1'); no distance code."""
    lens = [0] * 286
    lens[L1_LIT] = lens[256] = 1
    return Code("l1", lens, None)


@functools.lru_cache(maxsize=None)
def copy_code():
    """(258, 1) in 2 bits: a 1-bit length code and a 1-bit distance code."""
    lens = [0] * 286
    lens[285] = lens[256] = 1
    return Code("copy2", lens, [1, 1])


# ---- family S: segment ends -------------------------------------------------------------------------------------
def s_lanes(W, short):
    nl = 64 * W
    js = [0, 1, 31, 62] + ([63, 64, nl - 2] if W > 1 else [])
    return js if short else js + [nl - 1]


def _family_s():
    res = []
    code = general_code(15)
    big = code.width(big_token(code))
    assert big == 48
    idx = 0
    for W in (1, 4):
        nl = 64 * W
        for short in (False, True):
            per = 32 * (PW_MIN if short else LPW)
            for off in (1, 47, 48):
                for seed in range(50):
                    st = Stream(code, D0_MODS[idx % 5], 0x5500 + 64 * idx + seed)
                    b = st.builder(code, False)
                    ats = []
                    for j in s_lanes(W, short):
                        ats.append((j, b.place(b.d0 + (j + 1) * per - off, big_token(code, st.rng))))
                    if short:           # the block ends inside the last lane's segment: one round of pw = PW_MIN
                        b.fill_to(b.d0 + (nl - 1) * per + 70)
                    else:
                        b.fill_to(b.pos + 300)
                    st.add(b.close())
                    tail_blocks(st, "stored")
                    c = finish(f"S_big_W{W}_pw{per // 32}_e-{off}", "S", st.w, st.blocks, W,
                               {"pw": per // 32, "off": off, "at": ats}, st.k)
                    if clean(c):
                        break
                else:
                    raise AssertionError(c.name)
                res.append(c)
                idx += 1
        # the last lane of a short round: the round ends where the (cut) input ends, 1, 47 and 48 bits after the
        # token's start
        for off in (1, 47, 48):
            for seed in range(50):
                st = Stream(code, D0_MODS[idx % 5], 0x5580 + 64 * idx + seed)
                b = st.builder(code, True)
                end = -(-(b.d0 + (nl - 1) * 32 * PW_MIN + 60) // 8) * 8
                at = b.place(end - off, big_token(code, st.rng))
                b.fill_to(b.pos + 200)
                st.add(b.close())
                c = finish(f"S_last_W{W}_pw{PW_MIN}_e-{off}", "S", st.w, st.blocks, W,
                           {"pw": PW_MIN, "off": off, "at": [(nl - 1, at)]}, st.k, cut=end // 8)
                if clean(c):
                    break
            else:
                raise AssertionError(c.name)
            res.append(c)
            idx += 1
        # a round of nothing but 48-bit tokens
        for seed in range(50):
            st = Stream(code, D0_MODS[idx % 5], 0x5600 + 64 * idx + seed)
            b = st.builder(code, False)
            while b.pos < b.d0 + rspan(W) + 100:
                b.put(big_token(code, st.rng))
            st.add(b.close())
            tail_blocks(st, "fixed")
            c = finish(f"S_all_big_W{W}", "S", st.w, st.blocks, W, {"all": 48}, st.k)
            if clean(c):
                break
        else:
            raise AssertionError(c.name)
        res.append(c)
        idx += 1
        # a round of 1-bit literals: primary-table pairs, 448 tokens per lane
        st = Stream(l1_code(), D0_MODS[idx % 5], 0, prelude=False)
        b = st.builder(l1_code(), False)
        b.repeat(("L", L1_LIT), rspan(W) + 77)
        st.add(b.close())
        tail_blocks(st, "fixed")
        c = finish(f"S_all_1bit_W{W}", "S", st.w, st.blocks, W, {"all": 1}, st.k)
        assert clean(c)
        res.append(c)
        idx += 1
    # a round of (258, 1) copies at 2 bits each: 57,792 bytes per lane (W = 1: four waves' worth is past the
    # output limit of a case)
    st = Stream(copy_code(), D0_MODS[idx % 5], 0)
    # (the prelude's window is the copies' source)
    b = st.builder(copy_code(), False)
    b.repeat(("M", 258, 1), rspan(1) // 2 + 9)
    st.add(b.close())
    tail_blocks(st, "fixed")
    c = finish("S_all_copy258_W1", "S", st.w, st.blocks, 1, {"all": 2}, st.k)
    assert clean(c)
    res.append(c)
    return res


# ---- family C: checkpoints ----------------------------------------------------------------------------------------
C_LANE = 5                              # the lane whose checkpoints the cases aim at (a full round: pw = LPW)


@functools.lru_cache(maxsize=None)
def plock_code():
    """A code that never resynchronises on the stream of family C's nslow cases, with 191 lengths of 8 (one short
    of the phase-mapped rounds): 32 literals of 7 bits (codes 00xxxxx, never in the stream), 190 literals of 8
    bits (literal v - 32 has the code v, 64 <= v < 254), the length symbol 257 in 8 bits (code 11111110), a
    literal and the end of block in 9.  Distance codes '0', '10', '110', '111': (3, 2) has 10 bits, (3, 3) 11."""
    lens = [0] * 286
    for s in range(32):
        lens[s] = 7
    for s in range(32, 222):
        lens[s] = 8
    lens[257] = 8
    lens[222] = lens[256] = 9
    c = Code("plock", lens, [1, 2, 3, 3])
    assert c.lc[0x55 + 0x55 - 32] == (int("10101010"[::-1], 2), 8) and c.lc[257] == (int("11111110"[::-1], 2), 8)
    return c


PL_A, PL_B = ("M", 3, 2), ("M", 3, 3)   # 10 and 11 bits: a decode that reads one leaves the 8-bit grid by 2 or 3


def _plock_bits(b, bits):
    """The bit string as 8-bit literals of the plock code (every window is one: none starts with 00 or is 1111111x)."""
    assert len(bits) % 8 == 0
    for i in range(0, len(bits), 8):
        v = int(bits[i:i + 8], 2)
        assert 64 <= v < 254, bits[i:i + 8]
        b.put(("L", v - 32))


def _alt(n):
    """n alternating bits that start with 1 and end with 0 (an odd n: the first 1 doubled)."""
    return ("1" if n & 1 else "") + "10" * (n // 2)


def _plock_round(b, rs, a, n):
    """From the builder's position (on the 8-bit grid of the round that starts at rs) to the end of that round:
    lanes a .. a + n - 1 are the ones whose first verify does not synchronise.  A true (3, 2) at the end of lane
    a - 1 takes the true decode 2 bits off the grid for the rest of the round (its 8-bit literals spell every bit
    after it); lane q's speculation, on the grid, reads a planted (3, 3) or (3, 2) pattern near its end and
    leaves at phase 3 or 2, the phase lane q + 1's speculation does not leave at; the last lane of the run
    has no pattern, so the lane after it is verified from a start on the grid: its own speculation."""
    per = 32 * LPW
    s = lambda j: rs + j * per
    assert (b.pos - rs) % 8 == 0 and b.pos <= s(a) - 16 and n >= 1
    _plock_bits(b, "10101010" * ((s(a) - 16 - b.pos) // 8))
    b.put(PL_A)
    bits, pos = "", b.pos
    for i, q in enumerate(range(a, a + n - 1)):
        at = s(q) + per - 16
        bits += _alt(at - pos)
        bits += "11111110" + ("110" if i % 2 == 0 else "10")
        pos = at + (11 if i % 2 == 0 else 10)
    end = rs + rspan(1) + 2                         # a token boundary of the true decode just past the round's end
    bits += _alt(end - pos)
    _plock_bits(b, bits)
    return b.pos


def _family_c():
    res = []
    code = general_code(15)
    per = 32 * LPW
    idx = 0

    def stream(tag):
        nonlocal idx
        idx += 1
        return Stream(code, D0_MODS[idx % 5], 0xC000 + 64 * idx + tag)

    def done(st, b, name, info, follow="fixed"):
        b.fill_to(b.d0 + rspan(1) + 200)
        st.add(b.close())
        tail_blocks(st, follow)
        return finish(name, "C", st.w, st.blocks, 1, info, st.k)

    # token boundaries around the checkpoints
    for cp, off in (("C1", XCP1), ("C2", XCP2)):
        for d in (-1, 0, 1):
            for seed in range(50):
                st = stream(seed)
                b = st.builder(code, False)
                at = b.place(b.d0 + C_LANE * per + off + d, ("L", Z15))
                c = done(st, b, f"C_boundary_{cp}{d:+d}", {"cp": off, "d": d, "at": at})
                if clean(c):
                    break
            else:
                raise AssertionError(c.name)
            res.append(c)
    # literal pairs whose first literal ends before, at and past a stop
    for stop, off in (("C1", XCP1), ("C2", XCP2), ("e", per)):
        for d in (-1, 0, 1):
            for seed in range(50):
                st = stream(seed)
                b = st.builder(code, False)
                at = b.d0 + C_LANE * per + off + d - 2
                b.place(at - 15, ("L", Z15))
                b.put(("L", A2))
                b.put(("L", A2))
                b.put(("L", Z15))
                c = done(st, b, f"C_pair_{stop}{d:+d}", {"stop": off, "d": d, "at": at})
                if clean(c):
                    break
            else:
                raise AssertionError(c.name)
            res.append(c)
    # last-lane segments that end before the checkpoints: one round, ended by the stored header after it
    for L in (1, 64, 65, 192):
        pw = next(q for q in range(PW_MIN, LPW + 1) if seg_pw(63 * 32 * q + L) == q)
        for seed in range(50):
            st = stream(seed)
            b = st.builder(code, False)
            b.fill_to(b.d0 + 63 * 32 * pw + L - 15)
            st.add(b.close())
            tail_blocks(st, "stored")
            c = finish(f"C_last_lane_{L}", "C", st.w, st.blocks, 1, {"last": L, "pw": pw}, st.k)
            if clean(c):
                break
        else:
            raise AssertionError(c.name)
        res.append(c)
    # lanes that do not synchronise: 1, 8, 9 (the phase runs engage), 49 (the block's next round is phase-mapped:
    # its 9 are not counted), and 48, after which they are
    pc = plock_code()
    for n1, n2 in ((1, 0), (8, 0), (9, 0), (49, 9), (48, 9)):
        st = Stream(pc, 8 * (idx % 4), 0, prelude=False)
        idx += 1
        b = st.builder(pc, False, bulk=[])
        for _ in range(4):
            b.put(("L", 0xAA - 32))
        rs2 = _plock_round(b, b.d0, 3, n1)
        if n2:
            _plock_round(b, rs2, 3, n2)
        _plock_bits(b, "10101010" * 27)     # (the end of block past its lane's first checkpoint)
        st.add(b.close())
        tail_blocks(st, "fixed")
        c = finish(f"C_nslow_{n1}" + (f"_then_{n2}" if n2 else ""), "C", st.w, st.blocks, 1,
                   {"nslow": [n1, n2] if n2 else [n1]}, st.k)
        assert clean(c), c.name
        res.append(c)
    return res


# ---- family T: the input's tail -----------------------------------------------------------------------------------
def _family_t():
    res = []
    code = general_code(15)
    idx = 0
    # the final end of block ends 0..7 bits before the input's last bit
    for gap in range(8):
        for seed in range(50):
            st = Stream(code, D0_MODS[idx % 5], 0x7000 + 64 * idx + seed)
            b = st.builder(code, True)
            t = b.d0 + 400
            while (t + 15 + gap) % 8:
                t += 1
            b.fill_to(t)
            st.add(b.close())
            c = finish(f"T_eob_gap{gap}", "T", st.w, st.blocks, None, {"gap": gap}, st.k)
            if clean(c):
                break
        else:
            raise AssertionError(c.name)
        res.append(c)
        idx += 1
    # each token kind inside the last 48 bits (the checked decoder) and as the last token before them
    c1 = general_code(1, "slow", False)
    ced = Code("general_eob1_nodist", c1.lit, None)
    # (kind, code, tokens, start before the input's end, the decoder run_to gives it to: the register bit buffer
    # up to 49 bits before the end, the checked one from 48)
    kinds = [("lit2", c1, [("L", A2)], 3, "checked"), ("lit2", c1, [("L", A2)], 49, "unchecked"),
             ("lit15", c1, [("L", Z15)], 16, "checked"), ("pair", c1, [("L", A2), ("L", A2)], 5, "checked"),
             ("pair", c1, [("L", A2), ("L", A2)], 48, "checked"), ("pair", c1, [("L", A2), ("L", A2)], 49, "unchecked"),
             ("match31", c1, None, 32, "checked"), ("match48", c1, None, 49, "unchecked"),
             ("lenonly", ced, [("X", 281, 21)], 20, "checked"), ("lenonly", ced, [("X", 281, 21)], 49, "unchecked")]
    for kind, cd, toks, back, path in kinds:
        for seed in range(50):
            st = Stream(cd, D0_MODS[idx % 5], 0x7400 + 64 * idx + seed)
            b = st.builder(cd, True)
            nb = (b.d0 + 600) & ~7
            if toks is None:
                toks = [token_of_width(cd, 31 if kind == "match31" else 48, st.rng)]
            b.place(nb - back - 15, ("L", Z15))
            upto = len(b.tokens)
            for t in toks:
                b.put(t)
            err = kind == "lenonly"
            if not (err and back == 20):
                b.fill_to(nb - 1)
            st.add(b.close() if not (err and back == 20) else
                   Blk("dynamic", b.hdr, b.d0, b.starts + [b.pos], b.pos, True, cd, b.tokens))
            c = finish(f"T_tail_{kind}_at{back}", "T", st.w, st.blocks, None, {"kind": kind, "back": back, "path": path},
                       st.k, reason=EMPTY_DIST if err else None, upto=upto)
            if clean(c):
                break
        else:
            raise AssertionError(c.name)
        assert len(c.comp) * 8 == nb, (c.name, len(c.comp) * 8, nb)
        res.append(c)
        idx += 1
    # the stream cut at each of its last 8 bytes, and inside a 48-bit token of lane 7 of the second round ...
    st = Stream(code, 13, 0x7800)
    b = st.builder(code, True)
    rs = _full_rounds(b, 1, 2)
    at = rs + 7 * 32 * LPW + 100
    at += -(at + 44) % 8                    # (44 of its 48 bits end on a byte)
    b.place(at, big_token(code, st.rng))
    at2 = rs + 9 * 32 * LPW + 100
    at2 += -(at2 + 48) % 8                  # (a second one ends on a byte)
    b.place(at2, big_token(code, st.rng))
    b.fill_to(rs + rspan(1) + 300)
    st.add(b.close())
    n = len(st.w.getbytes())
    for i in range(1, 9):
        res.append(finish(f"T_cut_last{i}", "T", st.w, st.blocks, 1, {"cut": n - i}, st.k, cut=n - i))
    res.append(finish("T_cut_in_token", "T", st.w, st.blocks, 1, {"cut": (at + 20) // 8, "at": at}, st.k,
                      cut=(at + 20) // 8))
    # ... and 4 bits before its end: it starts 44 bits before the input's end, the first start that run_to's
    # unchecked bit buffer must leave to the checked decoder
    res.append(finish("T_cut_token_44_of_48", "T", st.w, st.blocks, 1, {"cut": (at + 44) // 8, "at": at}, st.k,
                      cut=(at + 44) // 8))
    # a whole 48-bit match in the input's last 48 bits (the checked decoder), and nothing after it
    res.append(finish("T_tail_match48_at48", "T", st.w, st.blocks, 1,
                      {"kind": "match48", "back": 48, "path": "checked", "cut": (at2 + 48) // 8}, st.k, cut=(at2 + 48) // 8))
    assert all(clean(c) for c in res[-11:])
    return res


# ---- family P: phase-mapped rounds --------------------------------------------------------------------------------
P_LIT3 = 0x20
P_LANE = 9


@functools.lru_cache(maxsize=None)
def phased_code(n8):
    """n8 literals of 8 bits (0x30 up), one of 3 bits, 15-bit length codes with 0 and 5 extra bits; D_SLOW."""
    fixed = {P_LIT3: 3, 281: 15, 257: 15, 256: 15}
    for s in range(0x30, 0x30 + n8):
        fixed[s] = 8
    if n8 < 192:
        for s in range(0x30 + n8, 0x30 + n8 + 2 * (192 - n8)):
            fixed[s] = 9
    c = Code(f"phased_{n8}", complete(fixed, 9), D_SLOW)
    assert c.n8 == n8
    return c


def _fill8(b, target, lits):
    """8-bit literals (random) and up to seven 3-bit ones, to exactly bit `target`."""
    r = target - b.pos
    n3 = 3 * r % 8
    assert r >= 3 * n3, (r, n3)
    for _ in range(n3):
        b.put(("L", P_LIT3))
    for _ in range((r - 3 * n3) // 8):
        b.put(("L", b.rng.choice(lits)))
    assert b.pos == target


def _family_p():
    res = []
    per = 32 * LPW
    idx = 0
    for n8 in (191, 192):
        code = phased_code(n8)
        lits = [s for s in range(256) if code.lit[s] == 8]
        for seed in range(50):
            st = Stream(code, D0_MODS[idx % 5], 0xF000 + 64 * idx + seed)
            b = st.builder(code, False, bulk=[])
            _fill8(b, b.d0 + rspan(1) + rspan(1) // 2, lits)
            st.add(b.close())
            tail_blocks(st, "fixed")
            c = finish(f"P_n8_{n8}", "P", st.w, st.blocks, 1, {"n8": n8}, st.k)
            if clean(c):
                break
        else:
            raise AssertionError(c.name)
        res.append(c)
        idx += 1
    code = phased_code(192)
    lits = [s for s in range(256) if code.lit[s] == 8]
    for d in (0, 1, 7, 8, 9, 15, 16, 30, 47):
        for seed in range(200):
            st = Stream(code, D0_MODS[idx % 5], 0xF400 + 256 * idx + seed)
            b = st.builder(code, False, bulk=[])
            sj = b.d0 + P_LANE * per
            _fill8(b, sj + d - 48, lits)
            # the token's last 8 bits (distance extra bits) are an 8-bit literal's code: the phase run that
            # starts on them ends its first token on the token's end
            v = code.lc[st.rng.choice(lits)][0]
            y = st.rng.randrange(32) | v << 5
            at = b.put(("M", 131 + st.rng.randrange(32), 24577 + y))
            assert b.pos == sj + d
            _fill8(b, b.d0 + rspan(1) + 900, lits)
            st.add(b.close())
            tail_blocks(st, "fixed")
            c = finish(f"P_entry_d{d}", "P", st.w, st.blocks, 1, {"d": d, "at": at, "lane": P_LANE}, st.k)
            if clean(c) and _entry_as_named(c):
                break
        else:
            raise AssertionError(c.name)
        res.append(c)
        idx += 1
    # an escape-prefix block (254 literals of 8 bits): a 48-bit token whose length code lies under the escape
    # prefix starts 7 bits before a segment end
    kc = k_code()
    for seed in range(50):
        st = Stream(kc, 8 * (seed % 4), 0xF800 + seed)
        b = st.builder(kc, False, bulk=[])
        sj = b.d0 + P_LANE * per
        pad = (sj - 7 - b.d0) % 8
        for _ in range(pad):                        # (nine-bit literals take the stream off the byte grid)
            b.put(("L", 255))
        while b.pos + 8 <= sj - 7:
            b.put(("L", st.rng.randrange(254)))
        at = b.put(big_token(kc, st.rng))
        for _ in range((rspan(1) + 500) // 8):
            b.put(("L", st.rng.randrange(254)))
        st.add(b.close())
        tail_blocks(st, "fixed")
        c = finish("P_escape_len_at_segment_end", "P", st.w, st.blocks, 1, {"at": at, "lane": P_LANE, "back": sj - at},
                   st.k)
        if clean(c) and 0 < sj - at <= 15:
            break
    else:
        raise AssertionError(c.name)
    res.append(c)
    # a short phase-mapped round ended by a planted stored header: the 48-bit token before it ends on the round
    # end (its last bit a 1, the header in the next byte) and one bit past it (its last bit a 0: the header's first)
    for ov, y in ((0, 1 << 12), (1, 1 << 11)):
        st = Stream(kc, 8 * ov, 0xF900 + ov)
        b = st.builder(kc, False, bulk=[])
        _kfill(b, 600)
        at = b.put(("M", 131, 24577 + y))
        end = b.pos
        _k_plant(b, [0x00])
        _kfill(b, 2000)
        st.add(b.close())
        tail_blocks(st, "fixed")
        res.append(finish(f"P_short_round_overhang{ov}", "P", st.w, st.blocks, 1, {"overhang": ov, "at": at, "E": end - ov},
                          st.k))
    return res


def entry_phase(c):
    """The model's phase_of for a P_entry case: (d, phase or None)."""
    b = c.blocks[c.k]
    r = tested_rounds(c, 1)[0]
    g = geo(r.rs, r.E, 1)
    s, _ = seg(g, c.info["lane"])
    entry = next(t for t in b.starts + [b.end] if t >= s)
    return Sim(c.comp, b.code).phase_entry(g, c.info["lane"], entry)


def _entry_as_named(c):
    d, ph = entry_phase(c)
    want = d if d < 8 else d - 8 if d < 16 else None
    return d == c.info["d"] and ph == want


# ---- family K: false header candidates inside a Huffman block --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k_code():
    """254 literals of 8 bits in symbol order (a byte-aligned literal writes the bit-reversed byte of the builder's
    choice), everything else under the prefix 1111111; the 48-bit token's extra bits are 18 zero bits."""
    fixed = {s: 8 for s in range(254)}
    fixed.update({281: 15, 256: 15})
    return Code("k254", complete(fixed, 9), D_SLOW)


def rev8(x):
    return int(format(x, "08b")[::-1], 2)


def _kbytes(b, data):
    for x in data:
        assert rev8(x) < 254, hex(x)
        b.put(("L", rev8(x)))


K_LEN = 257                             # LEN 01 01, NLEN FE FE: bytes the 254 literals can write
K_STORED = bytes([1, 1, 0xFE, 0xFE])


def _kfill(b, n):
    """n bytes that hold no header: bit 0 set (BFINAL) and bits 1..2 set (the reserved block type)."""
    _kbytes(b, [0x07 | b.rng.randrange(15) << 3 for _ in range(n)])


def _k_plant(b, hdr_bytes):
    """The stored header's own bytes, LEN / NLEN, LEN data bytes and a byte that reads as a fixed block's header."""
    _kbytes(b, hdr_bytes)
    _kbytes(b, K_STORED)
    _kfill(b, K_LEN)
    _kbytes(b, [0x02])


def _family_k():
    res = []
    kc = k_code()
    for name in ("in_token", "on_boundary", "after_round_start", "round_end_minus_1"):
        st = Stream(kc, 8 * (len(res) % 4), 0xE000 + len(res))
        b = st.builder(kc, False, bulk=[])
        assert b.d0 % 8 == 0
        if name == "after_round_start":
            want = [b.d0 + 1]
            _k_plant(b, [0x01])
            _kfill(b, 3000)
        elif name == "round_end_minus_1":
            _kfill(b, rspan(1) // 8 - 1)
            want = [b.pos + 7]
            _k_plant(b, [0x40, 0x00])
            _kfill(b, 1000)
        else:
            _kfill(b, 1500)
            if name == "in_token":
                at = b.put(("M", 131, 24577))
                want = list(range(b.pos - 10, b.pos - 2))
                _k_plant(b, [])
            else:
                _kbytes(b, [0xF7])                  # (a set bit before it: no alias a bit early)
                want = [b.pos]
                _k_plant(b, [0x00])
            _kfill(b, 3000)
        st.add(b.close())
        tail_blocks(st, "fixed")
        res.append(finish(f"K_{name}", "K", st.w, st.blocks, 1, {"want": want}, st.k))
    # bytes after the real final block: a header whose chain ends in COPY_FROM_BEFORE_DICTIONARY_START, and a
    # complete final stored block
    w2 = TS.BitWriter()
    TS.write_block(w2, [], "stored", False)
    TS.write_block(w2, [("L", 1), ("M", 3, 30000), ("L", 2)], "fixed", True)
    code = general_code(15)
    for name, trailing in (("copy_before", w2.getbytes()), ("stored", b"\x01\x05\x00\xfa\xffhello")):
        st = Stream(code, 13, 0xE100)
        b = st.builder(code, True)
        b.fill_to(b.d0 + 5000)
        st.add(b.close())
        res.append(finish(f"K_trailing_{name}", "K", st.w, st.blocks, None, {"trailing": len(trailing)}, st.k,
                          trailing=trailing))
    return res


_BUILDERS = {"R": _family_r, "S": _family_s, "C": _family_c, "T": _family_t, "P": _family_p, "K": _family_k}
COUNTS = {"R": 89, "S": 23, "C": 24, "T": 29, "P": 14, "K": 6}
FAMILIES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def cases(name):
    return _BUILDERS[name]()
