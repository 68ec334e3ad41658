"""Hand-built LZ77 token streams for the decoder's copy and resolve paths.

The decoder's emit pass (inflate_wave.hpp: ndfl_inflate_emit_wave_kernel, ndfl_inflate_emit_fast_kernel)
never runs an LZ77 copy the way the reference does: a lane executes a copy itself (wr_copy, five width
classes) only when every source byte is its own and final, and defers every other one (ref[] back-
references, pend bitmap bits, ndfl_inflate_resolve_kernel).  Which of the two a copy takes depends on
its distance, its length, where its source lies relative to the lane's first byte and its pending
bytes, and how deep the chain of references behind it is -- none of which a stream written by an
encoder chooses.  This module writes streams token by token instead:

    write_block(w, tokens, kind, final)   one block from ("L", byte) / ("M", length, distance) tokens
    stream(blocks, kinds)                 the blocks as one raw DEFLATE stream, with the block seams
    expand(blocks, window)                the reference: out.append(out[-d]), byte at a time

and the case families A..F (family(name)) built from them, seeded and built once per process.
A dynamic block takes its code lengths from the token histogram exactly as pyref_deflate.compress_block
does.  expand() shares no code with the CPU oracle or the library.  Test infrastructure only.
"""
import collections
import functools
import random

import numpy as np

import pyref_deflate as P

COPY_BEFORE = "COPY_FROM_BEFORE_DICTIONARY_START"
MAX_BLOCK_BITS = 8192          # lane segments are then NDFL_PW_MIN words = 128 bits (inflate_records.hpp)


class BitWriter:
    """LSB-first bit writer that moves whole bytes to a bytearray as it goes (pyref_deflate.BitWriter
    keeps one big integer: quadratic on streams of this size)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.k = 0

    @property
    def n(self):
        return 8 * len(self.buf) + self.k

    def bits(self, v, nb):
        assert 0 <= nb <= 31 and v >> nb == 0
        self.acc |= v << self.k
        self.k += nb
        if self.k >= 32:
            nbytes = self.k >> 3
            self.buf += (self.acc & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")
            self.acc >>= 8 * nbytes
            self.k -= 8 * nbytes

    def getbytes(self):
        nbytes = (self.k + 7) >> 3
        return bytes(self.buf) + self.acc.to_bytes(nbytes, "little")


@functools.lru_cache(maxsize=None)
def _fixed_codes():
    return P.canonical(P.STATIC_LIT_LENS, 9), P.canonical([5] * 32, 5)


@functools.lru_cache(maxsize=1 << 16)
def _match_syms(length, distance):
    return P.len_sym(length), P.dist_sym(distance)


def write_block(w, tokens, kind, final):
    """One block.  tokens: ("L", byte) and ("M", length, distance); a fixed block also takes
    ("R", symbol): a bare literal/length symbol (286 / 287: the reserved ones the fixed code can carry).
    kind: "fixed", "dynamic" or "stored" (literals only, at most 65,535)."""
    if kind == "stored":
        assert len(tokens) <= 65535 and all(t[0] == "L" for t in tokens)
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.bits(0, (8 - w.n % 8) % 8)
        w.bits(len(tokens), 16)
        w.bits(len(tokens) ^ 0xFFFF, 16)
        for t in tokens:
            w.bits(t[1], 8)
        return
    w.bits(1 if final else 0, 1)
    if kind == "fixed":
        w.bits(1, 2)
        lcodes, dcodes = _fixed_codes()
    else:
        assert kind == "dynamic"
        w.bits(2, 2)
        lit = [0] * 286
        dist = [0] * 30
        for t in tokens:
            if t[0] == "L":
                lit[t[1]] += 1
            else:
                (ls, _, _), (ds, _, _) = _match_syms(t[1], t[2])
                lit[ls] += 1
                dist[ds] += 1
        lit[256] += 1
        if sum(1 for c in lit if c) == 1:           # the end of block alone: a second literal, never sent
            lit[0] += 1
        ln = 286
        while ln > 257 and lit[ln - 1] == 0:
            ln -= 1
        lit = lit[:ln]
        llens = P.package_merge(lit, 15)
        used = [i for i, c in enumerate(dist) if c]
        if len(used) == 1:                           # a single distance code gets a neighbour
            u = used[0]
            dist[u + 1 if u < 29 else u - 1] = 1
        dn = 30
        while dn > 1 and dist[dn - 1] == 0:
            dn -= 1
        dist = dist[:dn]
        empty = dn == 1 and dist[0] == 0             # no distance code at all: one zero length
        dlens = [0] if empty else P.package_merge(dist, 15)
        seq = P.cl_rle(llens + dlens)
        clh = [0] * 19
        for s, _ in seq:
            clh[s] += 1
        cllens = P.package_merge(clh, 7)
        reo = [cllens[P.CLC_ORDER[i]] for i in range(19)]
        ncl = 19
        while ncl > 4 and reo[ncl - 1] == 0:
            ncl -= 1
        w.bits(ln - 257, 5)
        w.bits(dn - 1, 5)
        w.bits(ncl - 4, 4)
        for i in range(ncl):
            w.bits(reo[i], 3)
        clcodes = P.canonical(cllens, 7)
        for s, e in seq:
            c, l = clcodes[s]
            w.bits(c, l)
            if s >= 16:
                w.bits(e, {16: 2, 17: 3, 18: 7}[s])
        lcodes = P.canonical(llens, 15)
        dcodes = None if empty else P.canonical(dlens, 15)
    bits = w.bits
    for t in tokens:
        if t[0] == "L":
            c, l = lcodes[t[1]]
            bits(c, l)
        elif t[0] == "M":
            (ls, lne, lex), (ds, dne, dex) = _match_syms(t[1], t[2])
            c, l = lcodes[ls]
            bits(c | lex << l, l + lne)
            c, l = dcodes[ds]
            bits(c | dex << l, l + dne)
        else:
            assert t[0] == "R" and kind == "fixed"
            c, l = lcodes[t[1]]
            bits(c, l)
    c, l = lcodes[256]
    bits(c, l)


def stream(blocks, kinds):
    """The blocks as one raw DEFLATE stream (the last one final).  Returns (bytes, seams): seams[i] is
    the bit offset of block i's BFINAL bit."""
    assert len(blocks) == len(kinds) and blocks
    w = BitWriter()
    seams = []
    for i, (toks, kind) in enumerate(zip(blocks, kinds)):
        seams.append(w.n)
        write_block(w, toks, kind, i == len(blocks) - 1)
    return w.getbytes(), seams


def expand(blocks, window=b""):
    """The reference decode of token blocks after `window`: (None, bytes), or
    (COPY_FROM_BEFORE_DICTIONARY_START, the bytes before the offending token) when a distance exceeds
    len(window) + the bytes produced so far."""
    out = bytearray(window)
    nw = len(window)
    for toks in blocks:
        for t in toks:
            if t[0] == "L":
                out.append(t[1])
            elif t[0] == "M":
                d = t[2]
                if d > len(out):
                    return COPY_BEFORE, bytes(out[nw:])
                for _ in range(t[1]):
                    out.append(out[-d])
            else:
                raise ValueError("expand: a bare symbol is no token (it must lie behind the first error)")
    return None, bytes(out[nw:])


# ----------------------------------------------------------------------------------------------
# building blocks of the families
# ----------------------------------------------------------------------------------------------

Stream = collections.namedtuple("Stream", "name comp seams blocks kinds cases reason out")
Stream.__doc__ = """One family stream: comp / seams from stream(blocks, kinds); cases: [(output offset, label)] in
ascending order, the case boundaries; reason / out: expand(blocks)."""


class _Seq:
    """A token sequence under construction, with its output length and the case boundaries."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.toks = []
        self.cuts = {0}             # token indices where a new block must start
        self.n = 0
        self.cases = []

    def case(self, *label):
        self.cases.append((self.n, label))

    def lits(self, count):
        r = self.rng
        self.toks += [("L", r.randrange(256)) for _ in range(count)]
        self.n += count

    def copy(self, length, distance):
        assert 3 <= length <= 258 and 1 <= distance <= min(32768, self.n)
        self.toks.append(("M", length, distance))
        self.n += length

    def cut(self):
        self.cuts.add(len(self.toks))

    def blocks(self, per_block):
        """The tokens in blocks of at most per_block tokens, a new one at every cut()."""
        out, cur = [], []
        for i, t in enumerate(self.toks):
            if cur and (len(cur) >= per_block or i in self.cuts):
                out.append(cur)
                cur = []
            cur.append(t)
        out.append(cur)
        return out


def literalize(blocks, kinds):
    """blocks with the copies of every "stored" block turned into the literals they stand for (a stored
    block holds bytes only), so that a stored block is a copy source for the block after it."""
    out = bytearray()
    res = []
    for toks, kind in zip(blocks, kinds):
        at = len(out)
        for t in toks:
            if t[0] == "L":
                out.append(t[1])
            else:
                for _ in range(t[1]):
                    out.append(out[len(out) - t[2]])
        res.append([("L", b) for b in out[at:]] if kind == "stored" else toks)
    return res


def _make(name, blocks, kinds, cases, small_blocks=None):
    """small_blocks: the indices of the blocks that must stay within MAX_BLOCK_BITS (default: all)."""
    if "stored" in kinds:
        blocks = literalize(blocks, kinds)
    comp, seams = stream(blocks, kinds)
    ends = seams[1:] + [8 * len(comp)]
    for i in (range(len(blocks)) if small_blocks is None else small_blocks):
        if kinds[i] != "stored":
            assert ends[i] - seams[i] <= MAX_BLOCK_BITS, (name, i, ends[i] - seams[i])
    reason, out = expand(blocks)
    return Stream(name, comp, seams, blocks, kinds, cases, reason, out)


def _cycle(kinds, n):
    return [kinds[i % len(kinds)] for i in range(n)]


LAYOUTS = {"fixed": ["fixed"], "dynamic": ["dynamic"], "mixed": ["dynamic", "fixed", "stored"]}
PER_BLOCK = 200                 # tokens per block: under MAX_BLOCK_BITS for every family (checked in _make)


def case_at(s, offset):
    """The label of the family case that produced output byte `offset` of stream s."""
    label = None
    for at, lab in s.cases:
        if at > offset:
            break
        label = lab
    return label


# ----------------------------------------------------------------------------------------------
# Family A: wr_copy's width classes, wr_flush_word's remainder and the held literal words
# ----------------------------------------------------------------------------------------------

A_LENS = [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 257, 258]


def _family_a():
    res = []
    for half, dists in (("lo", range(1, 21)), ("hi", range(21, 41))):
        q = _Seq(0xA0 + len(half) + dists[0])
        for dist in dists:
            for length in A_LENS:
                for p in range(17):
                    q.case("A", dist, length, p)
                    q.lits(max(dist, 1) + p)
                    q.copy(length, dist)
                    q.copy(length, dist)        # its source: the first copy's bytes, final or pending
        blocks = q.blocks(PER_BLOCK)
        for lay, kinds in LAYOUTS.items():
            res.append(_make(f"A_{half}_{lay}", blocks, _cycle(kinds, len(blocks)), q.cases))
    return res


# ----------------------------------------------------------------------------------------------
# Family B: the defer decision at the lane's own pending bytes (the 32-byte pend groups)
# ----------------------------------------------------------------------------------------------

def _family_b():
    """A far copy of P bytes (another lane's: always deferred), F literals, then a copy (l, d) with d in
    {F, F+1, F+P-1, F+P, F+P+1} and l in {3, min(d, 40), d+5}: its source is wholly final, straddles the
    final / pending edge by one byte on either side, is wholly pending, or reaches before the pending
    run.  P in 3..40, F in 0..40; one stream per distance variant.  R = 0..31 literals in front, stepped
    from case to case (crossing R with every case would be 32 times the streams), so that the run's
    edges fall on every bit of a pend word -- test_token_stream_cpu checks that they do."""
    res = []
    for v in range(5):              # one stream per distance variant: F, F+1, F+P-1, F+P, F+P+1
        q = _Seq(0xB0 + v)
        q.case("B", "lead")
        q.lits(1100)
        r = 0
        for p in range(3, 41):
            for f in range(0, 41):
                d = [f, f + 1, f + p - 1, f + p, f + p + 1][v]
                if d < 1:
                    continue
                for length in sorted({3, min(d, 40), d + 5}):
                    if length < 3:
                        continue
                    q.case("B", p, f, d, length, r)
                    q.lits(r)                                   # the edges on every bit of a pend word
                    q.copy(p, q.rng.randrange(300, 1000))       # another lane's bytes: always deferred
                    q.lits(f)
                    q.copy(length, d)
                    r = (r + 1) % 32
        blocks = q.blocks(PER_BLOCK)
        res.append(_make(f"B_{v}", blocks, _cycle(["dynamic", "fixed"], len(blocks)), q.cases))
    return res


# ----------------------------------------------------------------------------------------------
# Family C: dist-1 runs and their anchors (lsp / lastsrc)
# ----------------------------------------------------------------------------------------------

def _family_c():
    q = _Seq(0xC0)
    q.case("C", "lead")
    q.lits(1100)
    rng = q.rng
    while q.n < 600_000:
        kind = rng.randrange(4)
        for _ in range(rng.randrange(1, 13)):
            if kind == 0:           # a long run: spans several lanes, so a lane starts inside it
                k = rng.randrange(1, 13)
                q.case("C", "run", k)
                q.lits(1)
                for _ in range(k):
                    q.copy(258, 1)
            elif kind == 1:         # a run directly after a deferred far copy
                p, length = rng.randrange(3, 41), rng.randrange(3, 259)
                q.case("C", "far+run", p, length)
                q.copy(p, rng.randrange(300, 1000))
                q.copy(length, 1)
            elif kind == 2:         # a far copy directly after a run
                p, length = rng.randrange(3, 41), rng.randrange(3, 259)
                q.case("C", "run+far", length, p)
                q.lits(1)
                q.copy(length, 1)
                q.copy(p, rng.randrange(300, 1000))
            else:
                nl, length = rng.randrange(4), rng.randrange(3, 21)
                q.case("C", "short", nl, length)
                q.lits(nl)
                q.copy(length, 1)
    blocks = q.blocks(PER_BLOCK)
    return [_make(f"C_{lay}", blocks, _cycle(kinds, len(blocks)), q.cases)
            for lay, kinds in (("dynamic", ["dynamic"]), ("mixed", ["dynamic", "fixed"]))]


# ----------------------------------------------------------------------------------------------
# Family D: depth -- every byte depends on the previous block
# ----------------------------------------------------------------------------------------------

D_BLOCK = 254
D_LIT_BLOCK = 4096              # the leading literals' blocks (these need not stay small)


def family_d(distance, out_len=1 << 20):
    """max(distance, 7) random literals, then (258, distance) copies only, in dynamic blocks of 254
    tokens, to at least out_len bytes.  Returns (Stream with out = None, expected bytes by tiling)."""
    return _family_d(distance, out_len)


@functools.lru_cache(maxsize=None)
def _family_d(distance, out_len):
    rng = random.Random(0xD0 + distance)
    nlit = max(distance, 7)
    lits = [("L", rng.randrange(256)) for _ in range(nlit)]
    ncopy = -(-(out_len - nlit) // 258)
    copies = [("M", 258, distance)] * ncopy
    if nlit <= 7:
        toks = lits + copies
        blocks = [toks[i:i + D_BLOCK] for i in range(0, len(toks), D_BLOCK)]
        small = range(len(blocks))
    else:
        blocks = [lits[i:i + D_LIT_BLOCK] for i in range(0, nlit, D_LIT_BLOCK)]
        nl = len(blocks)
        blocks += [copies[i:i + D_BLOCK] for i in range(0, ncopy, D_BLOCK)]
        small = range(nl, len(blocks))
    kinds = ["dynamic"] * len(blocks)
    comp, seams = stream(blocks, kinds)
    ends = seams[1:] + [8 * len(comp)]
    assert all(ends[i] - seams[i] <= MAX_BLOCK_BITS for i in small)
    head = np.array([t[1] for t in lits], dtype=np.uint8)
    total = nlit + 258 * ncopy
    want = np.concatenate([head, np.resize(head[nlit - distance:], total - nlit)]).tobytes()
    cases = [(0, ("D", distance, "literals")), (nlit, ("D", distance, "copies"))]
    return Stream(f"D_{distance}_{out_len}", comp, seams, blocks, kinds, cases, None, None), want


# ----------------------------------------------------------------------------------------------
# Family E: far and mixed distances, copies of copies
# ----------------------------------------------------------------------------------------------

E_DISTS = [32768, 32767, 32766, 24577, 16385, 16384, 259, 258, 257]


def _family_e():
    q = _Seq(0xE0)
    q.case("E", "literals")
    q.lits(40_000)
    q.cut()
    nlit_tokens = len(q.toks)
    rng = q.rng
    prev = 0
    for i in range(2000):
        length = rng.choice([3, 258, rng.randrange(3, 259)])
        if i % 4 == 3:              # the source overlaps the previous copy's destination
            dist = rng.randrange(1, prev + 2)
        else:
            dist = rng.choice(E_DISTS)
        q.case("E", i, length, dist)
        q.copy(length, dist)
        prev = length
    lit_blocks = [q.toks[i:i + D_LIT_BLOCK] for i in range(0, nlit_tokens, D_LIT_BLOCK)]
    rest = q.toks[nlit_tokens:]
    copy_blocks = [rest[i:i + PER_BLOCK] for i in range(0, len(rest), PER_BLOCK)]
    blocks = lit_blocks + copy_blocks
    small = range(len(lit_blocks), len(blocks))
    return [_make(f"E_{lay}", blocks, ["dynamic"] * len(lit_blocks) + _cycle(kinds, len(copy_blocks)), q.cases, small)
            for lay, kinds in (("dynamic", ["dynamic"]), ("mixed", ["fixed", "dynamic"]))]


# ----------------------------------------------------------------------------------------------
# Family F: the dictionary bound
# ----------------------------------------------------------------------------------------------

F_POSITIONS = [1, 2, 3, 4, 7, 8, 15, 16, 17, 258, 32768]
F_LIT_BLOCK = 800               # literals per block (under MAX_BLOCK_BITS in a dynamic block)
F_PLACEMENTS = ["first", "third", "before_reserved"]


def _family_f():
    """Whole-stream decodes: `pos` literals, then a copy whose distance is pos (valid: it reaches byte
    0) or pos + 1 (COPY_FROM_BEFORE_DICTIONARY_START with out_len == pos).  The copy sits in the first
    block, in the third or a later block after dynamic blocks, or in a block followed by a fixed block
    that holds the reserved length symbol 286 (the copy error comes first in stream order and wins;
    in the valid stream the copy's block is followed by more tokens instead)."""
    res = []
    for pos in F_POSITIONS:
        for over in (0, 1):
            if pos + over > 32768:              # (DEFLATE has no distance 32,769: position 32,768 is valid only)
                continue
            for place in F_PLACEMENTS:
                q = _Seq(0xF000 + 8 * pos + 4 * over + F_PLACEMENTS.index(place))
                q.lits(pos)
                lits = list(q.toks)
                length = q.rng.choice([3, 10, 258])
                tail = [("M", length, pos + over)] + [("L", q.rng.randrange(256)) for _ in range(5)]
                tail += [("M", 7, 3), ("L", 1)]
                small = None
                if place == "first":
                    blocks, kinds = [lits + tail], ["dynamic" if pos & 1 else "fixed"]
                    small = []
                else:
                    if pos <= 2 * F_LIT_BLOCK:
                        half = (pos + 1) // 2
                        blocks = [lits[:half], lits[half:]]       # (the second one empty for pos == 1)
                    else:
                        blocks = [lits[i:i + F_LIT_BLOCK] for i in range(0, pos, F_LIT_BLOCK)]
                    kinds = ["dynamic"] * len(blocks)
                    blocks.append(tail)
                    kinds.append("dynamic" if place == "third" else "fixed")
                    if place == "before_reserved":
                        blocks.append([("L", 65), ("R", 286), ("L", 66)] if over else [("L", 65), ("M", 4, 1), ("L", 66)])
                        kinds.append("fixed")
                name = f"F_{pos}_{'over' if over else 'exact'}_{place}"
                cases = [(0, ("F", pos, over, place, "literals")), (pos, ("F", pos, over, place, "copy"))]
                s = _make(name, blocks, kinds, cases, small)
                assert (s.reason, len(s.out)) == ((COPY_BEFORE, pos) if over else (None, pos + length + 5 + 7 + 1 + (6 if place == "before_reserved" else 0)))
                res.append(s)
    return res


F_DICT_LENS = [0, 1, 2, 7, 258, 32767, 32768]
RangeCase = collections.namedtuple("RangeCase", "name comp seams blocks k dict_len n window reason out")
RangeCase.__doc__ = """A range decode from seams[k] with the last dict_len bytes before it as the window: the range's
first block holds n literals and then a copy that reaches dict_len + n bytes back (valid) or one byte
further (reason = COPY_FROM_BEFORE_DICTIONARY_START, len(out) == n).  reason / out: expand(blocks[k:], window)."""


def _family_f_ranges():
    rng = random.Random(0xF5)
    pre = [("L", rng.randrange(256)) for _ in range(32768 + 40)]
    pre_blocks = [pre[i:i + D_LIT_BLOCK] for i in range(0, len(pre), D_LIT_BLOCK)]
    pre_bytes = bytes(t[1] for t in pre)
    k = len(pre_blocks)
    res = []
    for dict_len in F_DICT_LENS:
        for n in (0, 1, 5):
            for over in (0, 1):
                d = dict_len + n + over
                if not 1 <= d <= 32768:         # no such distance in DEFLATE
                    continue
                first = [("L", rng.randrange(256)) for _ in range(n)] + [("M", rng.choice([3, 9, 258]), d)]
                first += [("L", rng.randrange(256)) for _ in range(4)]
                second = [("L", 7), ("M", 20, 2), ("L", 9)]
                blocks = pre_blocks + [first, second]
                kinds = ["dynamic"] * k + (["fixed", "dynamic"] if n & 1 else ["dynamic", "fixed"])
                comp, seams = stream(blocks, kinds)
                window = pre_bytes[len(pre_bytes) - dict_len:]
                reason, out = expand(blocks[k:], window)
                assert (reason, len(out)) == ((COPY_BEFORE, n) if over else (None, len(out)))
                res.append(RangeCase(f"FR_{dict_len}_{n}_{'over' if over else 'exact'}", comp, seams, blocks, k,
                                     dict_len, n, window, reason, out))
    return res


_BUILDERS = {"A": _family_a, "B": _family_b, "C": _family_c, "E": _family_e, "F": _family_f}
FAMILIES = list(_BUILDERS)      # (family D: family_d(distance, out_len); the range decodes: family_f_ranges())


@functools.lru_cache(maxsize=None)
def family(name):
    """The streams of family A, B, C, E or F (a list of Stream), built once per process."""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def family_f_ranges():
    return _family_f_ranges()


def stream_names(name):
    """The names of family(name)'s streams without building them (for parametrising tests)."""
    if name == "A":
        return [f"A_{h}_{lay}" for h in ("lo", "hi") for lay in LAYOUTS]
    if name == "B":
        return [f"B_{v}" for v in range(5)]
    if name == "C":
        return ["C_dynamic", "C_mixed"]
    if name == "E":
        return ["E_dynamic", "E_mixed"]
    return [f"F_{pos}_{'over' if over else 'exact'}_{place}" for pos in F_POSITIONS for over in (0, 1)
            if pos + over <= 32768 for place in F_PLACEMENTS]


def by_name(name):
    return next(s for s in family(name[0]) if s.name == name)
