"""Inputs that drive the encoder's per-block code construction to its limits, and a header walker.

The GPU encoder builds every dynamic block's codes with one builder (pm_lengths / canon_codes /
build_block_codes of huffman_build.hpp), instantiated at 64 threads for the split pipeline's codes
kernel and at 1024 threads for the one-kernel and the LZ77 encoders.  Random bytes, short runs and Zipf text never make the
15-bit limit bind on the literal/length or distance alphabet, nor the 7-bit limit on the code-length
alphabet; the generators below do, and also reach the single-distance-code fix-ups, HLIT = 286,
HDIST = 30 and the code-length run lengths at which the run decomposition changes shape.

    cases(cls)        -> the Case(name, data, encode_args, kind, plan) of cls in CLASSES, seeded, cached
    walk_blocks(comp) -> one dict per block of a raw DEFLATE stream (header fields, the three length
                         arrays, the code-length symbol sequence, the token histograms and tokens)
    engaged(...)      -> the engagement condition of a class, evaluated on walked blocks
    explain(exp, got) -> first differing block / header field of two streams, for failure messages

encode_args is ("preset", strategy_names, chunk_len, hist_limit) for inputs the LITERAL_* / RLE_* /
FULL_* presets encode, or ("lz", (dynamic, min_run, max_run, min_dist, max_dist), chunk_len,
hist_limit) for explicit Lz77Huffman parameters.

Written from RFC 1951 and tests/pyref_deflate.py.  Test infrastructure only (a helper module like
corpus.py and knobs.py, not a conftest).

HCLEN values (as counts of code-length code lengths sent) the cases reach on the oracle's streams:
5, 6, 7, 8, 13, 14, 16, 17, 18 and 19 (HCLEN_REACHED, asserted by test_oracle_deflate.
test_adversarial_hclen_reached).  HCLEN = 4 is unreachable: any dynamic block has at least two
code-length symbols in use, package-merge gives a two-symbol alphabet two 1-bit codes, and symbol 1
sits at position 17 of the transmission order, so a block that used only the first four positions
(16, 17, 18, 0) would need a length-1 code-length symbol it cannot name.
"""
import collections
import functools
import random

import numpy as np

import pyref_deflate as P

CLASSES = ["lit_limit", "cl_limit", "dist_limit", "dist_fixups", "cl_runs", "all_symbols"]

Case = collections.namedtuple("Case", "name data encode_args kind plan", defaults=(None,))

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_EXTRA = {16: 2, 17: 3, 18: 7}

RLE = (True, 3, 258, 1, 1)


# ----------------------------------------------------------------------------------------------
# header walker
# ----------------------------------------------------------------------------------------------

class _Bits:
    def __init__(self, comp):
        self.b = bytes(comp) + b"\0" * 8
        self.n = len(comp) * 8
        self.p = 0

    def peek(self, k):
        q = self.p >> 3
        b = self.b
        return ((b[q] | b[q + 1] << 8 | b[q + 2] << 16 | b[q + 3] << 24) >> (self.p & 7)) & ((1 << k) - 1)

    def take(self, k):
        v = self.peek(k)
        self.p += k
        if self.p > self.n:
            raise ValueError("walk_blocks: stream ends inside a block")
        return v


def _table(lens):
    """Decode table of the canonical code of `lens` (RFC 1951 3.2.2): index = the next `width` stream
    bits, entry = (symbol, length) or None."""
    width = max(lens) if lens else 0
    if width == 0:
        return 0, []
    tab = [None] * (1 << width)
    code = 0
    for cl in range(1, width + 1):
        code <<= 1
        for s, l in enumerate(lens):
            if l == cl:
                if code >> cl:
                    raise ValueError("walk_blocks: over-full code")
                rev = int(format(code, f"0{cl}b")[::-1], 2)
                for i in range(rev, 1 << width, 1 << cl):
                    tab[i] = (s, cl)
                code += 1
    return width, tab


def _sym(br, width, tab):
    e = tab[br.peek(width)] if width else None
    if e is None:
        raise ValueError("walk_blocks: bits match no code")
    br.p += e[1]
    if br.p > br.n:
        raise ValueError("walk_blocks: stream ends inside a block")
    return e[0]


def walk_blocks(comp):
    """The blocks of a raw DEFLATE stream.  Per block: bit (offset of BFINAL), end_bit, final, btype;
    for a dynamic block hlit / hdist / hclen as counts (257..286, 1..30, 4..19), cl_lens (by symbol),
    cl_seq ((symbol, extra) as transmitted), cl_hist, lit_lens, dist_lens; for every Huffman block
    lit_hist (286), dist_hist (30) and tokens (a byte value, or (length, distance)); the end-of-block
    symbol is counted in lit_hist[256].  A stored block has `stored` (its bytes) instead."""
    br = _Bits(comp)
    blocks = []
    while True:
        blk = {"bit": br.p}
        blk["final"] = br.take(1)
        bt = blk["btype"] = br.take(2)
        if bt == 3:
            raise ValueError("walk_blocks: reserved block type")
        if bt == 0:
            br.p = (br.p + 7) & ~7
            n = br.take(16)
            if br.take(16) != n ^ 0xFFFF:
                raise ValueError("walk_blocks: stored length mismatch")
            q = br.p >> 3
            blk["stored"] = br.b[q:q + n]
            br.p += 8 * n
            if br.p > br.n:
                raise ValueError("walk_blocks: stream ends inside a stored block")
        else:
            if bt == 1:
                lit_lens, dist_lens = list(P.STATIC_LIT_LENS), [5] * 30
            else:
                hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[P.CLC_ORDER[i]] = br.take(3)
                cw, ct = _table(cl_lens)
                seq, lens = [], []
                while len(lens) < hlit + hdist:
                    s = _sym(br, cw, ct)
                    e = br.take(CL_EXTRA[s]) if s >= 16 else None
                    seq.append((s, e))
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ValueError("walk_blocks: repeat with no previous length")
                        lens += [lens[-1]] * (3 + e)
                    else:
                        lens += [0] * ((3 if s == 17 else 11) + e)
                if len(lens) != hlit + hdist:
                    raise ValueError("walk_blocks: code lengths overrun HLIT + HDIST")
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
                cl_hist = [0] * 19
                for s, _ in seq:
                    cl_hist[s] += 1
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, cl_seq=seq, cl_hist=cl_hist,
                           lit_lens=lit_lens, dist_lens=dist_lens)
            lw, lt = _table(lit_lens)
            dw, dt = _table(dist_lens)
            lit_hist, dist_hist, toks = [0] * 286, [0] * 30, []
            while True:
                s = _sym(br, lw, lt)
                if s >= 286:
                    raise ValueError("walk_blocks: reserved length symbol")
                lit_hist[s] += 1
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    run = LEN_BASE[s - 257] + br.take(LEN_EXTRA[s - 257])
                    d = _sym(br, dw, dt)
                    if d >= 30:
                        raise ValueError("walk_blocks: reserved distance symbol")
                    dist_hist[d] += 1
                    toks.append((run, DIST_BASE[d] + br.take(DIST_EXTRA[d])))
            blk.update(lit_hist=lit_hist, dist_hist=dist_hist, tokens=toks)
        blk["end_bit"] = br.p
        blocks.append(blk)
        if blk["final"]:
            return blocks


def replay(blocks):
    """The bytes the walked blocks decode to (pins walk_blocks: must equal the encoder's input)."""
    out = bytearray()
    for b in blocks:
        if b["btype"] == 0:
            out += b["stored"]
            continue
        for t in b["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                run, d = t
                if d > len(out):
                    raise ValueError("replay: copy from before the start")
                for _ in range(run):
                    out.append(out[-d])
    return bytes(out)


def explain(exp, got):
    """Where `got` first leaves `exp` (two DEFLATE streams): the block and the first header field,
    length array or token that differs."""
    if exp == got:
        return "streams equal"
    eb = walk_blocks(exp)
    try:
        gb = walk_blocks(got)
    except (ValueError, IndexError) as e:
        gb = None
        err = e
    byte = next((i for i, (a, b) in enumerate(zip(exp, got)) if a != b), min(len(exp), len(got)))
    head = f"{len(got)} bytes for {len(exp)}, first differing byte {byte}"
    if gb is None:
        k = max((i for i, b in enumerate(eb) if b["bit"] <= 8 * byte), default=0)
        return f"{head}, in or before block {k} of {len(eb)} (at bit {eb[k]['bit']}); got does not parse: {err}"
    for k, (a, b) in enumerate(zip(eb, gb)):
        for f in ["bit", "final", "btype", "hlit", "hdist", "hclen", "cl_lens", "cl_seq", "lit_lens", "dist_lens",
                  "lit_hist", "dist_hist", "tokens", "stored", "end_bit"]:
            if a.get(f) != b.get(f):
                x, y = a.get(f), b.get(f)
                if isinstance(x, (list, bytes)) and isinstance(y, (list, bytes)):
                    i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                    x, y = f"[{i}]: {list(x[i:i + 6])}", f"[{i}]: {list(y[i:i + 6])}"
                return f"{head}; block {k} of {len(eb)} (bit {a['bit']}): {f} differs, expected {x}, got {y}"
    return f"{head}; {len(gb)} blocks for {len(eb)}"


# ----------------------------------------------------------------------------------------------
# engagement conditions (always evaluated on the oracle's stream)
# ----------------------------------------------------------------------------------------------

def tie_pairs(freqs, max_len):
    """Largest number, over the package-merge levels, of package/leaf pairs of equal frequency in the
    merged order (each such pair is a place where 'packages first' decides the lengths).  The
    package frequencies do not depend on the tie order, so a plain sort gives them."""
    leaves = sorted(f for f in freqs if f > 0)
    pk, best = [], 0
    for _ in range(max_len):
        cl, cp = collections.Counter(leaves), collections.Counter(pk)
        best = max(best, sum(min(n, cl[f]) for f, n in cp.items()))
        merged = sorted(pk + leaves)
        pk = [merged[2 * k] + merged[2 * k + 1] for k in range(len(merged) // 2)]
    return best


def _dyn(blocks):
    return [b for b in blocks if b["btype"] == 2]


def lit_hist_of(b):
    """The literal/length histogram the encoder ran package-merge on (trimmed to HLIT)."""
    return b["lit_hist"][:b["hlit"]]


def dist_hist_of(b):
    """The distance histogram after the single-code fix-up, trimmed to HDIST."""
    h = list(b["dist_hist"])
    used = [i for i, c in enumerate(h) if c]
    if len(used) == 1:
        h[used[0] + 1 if used[0] < 29 else used[0] - 1] = 1
    return h[:b["hdist"]]


def expected_lengths(b):
    """(literal, distance, code-length) lengths that package-merge at limits 15 / 15 / 7 gives for the
    histograms walked from dynamic block `b`, as the encoder forms them: a dummy literal 0 in an
    empty block, the single-distance-code fix-up, [0] for an unused distance alphabet."""
    h = lit_hist_of(b)
    if sum(h) == 1:
        h[0] += 1
    d = dist_hist_of(b)
    return (P.package_merge(h, 15), P.package_merge(d, 15) if any(d) else [0], P.package_merge(b["cl_hist"], 7))


def engaged(kind, blocks):
    """True when some block of `blocks` (walk_blocks of the ORACLE's stream) meets the condition of
    `kind` (a Case's kind: a name, or a tuple of a name and what the generator planned)."""
    want = None
    if isinstance(kind, tuple):
        kind, want = kind[0], kind[1:] if len(kind) > 2 else kind[1]
    bl = _dyn(blocks)
    if kind == "lit15":
        return any(max(b["lit_lens"]) == 15 and max(P.package_merge(lit_hist_of(b), 32)) > 15 for b in bl)
    if kind == "lit15_exact":
        return any(max(b["lit_lens"]) == 15 == max(P.package_merge(lit_hist_of(b), 32)) for b in bl)
    if kind == "ties":
        return any(tie_pairs(lit_hist_of(b), 15) >= 8 for b in bl)
    if kind == "flat":
        return any(len(set(lit_hist_of(b)[:255])) == 1 and b["lit_hist"][0] > 1 for b in bl)
    if kind == "cl7":
        return any(P.package_merge(b["cl_hist"], 7) != P.package_merge(b["cl_hist"], 15) and 7 in b["cl_lens"]
                   for b in bl)
    if kind == "dist15":
        return any(15 in b["dist_lens"] and max(P.package_merge(dist_hist_of(b), 32)) > 15
                   and (want is None or b["dist_hist"] == want) for b in bl)
    if kind == "one_dist":
        nb = want + 1 if want < 29 else want - 1
        return any([i for i, c in enumerate(b["dist_hist"]) if c] == [want]
                   and [i for i, l in enumerate(b["dist_lens"]) if l] == sorted([want, nb]) for b in bl)
    if kind == "no_dist":
        return any(sum(b["dist_hist"]) == 0 and b["hdist"] == 1 and b["dist_lens"] == [0] for b in bl)
    if kind == "run":
        L, start = want
        return any(len(set(b["lit_lens"][start:start + L])) == 1 and b["lit_lens"][start] == L.bit_length()
                   and (start == 0 or b["lit_lens"][start - 1] == 0) and b["lit_lens"][start + L] == 0 for b in bl)
    if kind == "cl_runs":
        return cl_run_shapes(blocks) >= CL_RUN_SHAPES
    if kind == "hlit286":
        return any(b["hlit"] == 286 for b in bl)
    if kind == "hlit286_hdist30":
        return any(b["hlit"] == 286 and b["hdist"] == 30 and min(b["lit_hist"][257:]) > 0
                   and min(b["dist_hist"]) > 0 for b in bl)
    raise KeyError(kind)


def cl_run_shapes(blocks):
    """What the code-length sequences of `blocks` contain, for the cl_runs condition: the set of
    (symbol, extra) with symbol >= 16, plus ("split", k) for a zero run sent as 138 + k (k < 3
    single zeros, or symbol 17 for k = 3..10)."""
    seen = set()
    for b in _dyn(blocks):
        seq = b["cl_seq"]
        for i, (s, e) in enumerate(seq):
            if s >= 16:
                seen.add((s, e))
            if (s, e) == (18, 127) and i + 1 < len(seq):
                k = 0
                while i + 1 + k < len(seq) and seq[i + 1 + k] == (0, None):
                    k += 1
                if k:
                    seen.add(("split", k))
                elif seq[i + 1][0] == 17:
                    seen.add(("split", 3 + seq[i + 1][1]))
    return seen


HCLEN_REACHED = {5, 6, 7, 8, 13, 14, 16, 17, 18, 19}
CL_RUN_SHAPES = {(18, 127), (17, 0), (17, 7), (16, 0), (16, 3), ("split", 1), ("split", 3)}


# ----------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------

def _shuffled(freqs, seed):
    """Bytes with the given {value: count}, in a seeded random order."""
    vals = np.repeat(np.array(list(freqs.keys()), dtype=np.uint8), list(freqs.values()))
    return vals[np.random.RandomState(seed).permutation(len(vals))].tobytes()


def _lit(name, freqs, seed, kind):
    return Case(name, _shuffled(freqs, seed), ("preset", ("LITERAL_DYNAMIC", "RLE_DYNAMIC"), 65536, 32768), kind)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _lit_limit():
    """Shuffled literal chunks: Fibonacci frequencies over 16..22 byte values and 1, 1, 2, 4, ... over
    16 and 17 symbols (the end-of-block symbol is one of the 1s) for the 15-bit limit, all-equal
    frequencies over 255 and 256 values, and k symbols at each of 1, 2, 4, ... for package/leaf ties
    at every level.  The conditions hold for LITERAL_DYNAMIC (and any parse that finds no match); in
    RLE_DYNAMIC / FULL_DYNAMIC streams of the skewed chunks the repeats change the histogram."""
    out = []
    for i, k in enumerate([16, 17, 18, 20, 22]):
        vals = random.Random(100 + k).sample(range(256), k)
        out.append(_lit(f"fib{k}", dict(zip(vals, _fib(k))), 10 + i, "lit15"))
    for i, k in enumerate([16, 17]):
        # with the end-of-block symbol as the other 1: frequencies 1, 1, 2, 4, ... over k symbols
        vals = random.Random(200 + k).sample(range(256), k - 1)
        # (k = 16 reaches 15 bits exactly with the limit not binding, k = 17 needs the limit)
        out.append(_lit(f"pow2_{k}", {v: 1 << t for t, v in enumerate(vals)}, 20 + i, "lit15" if k > 16 else "lit15_exact"))
    for n in [255, 256]:
        out.append(_lit(f"flat{n}", {v: 8 for v in range(n)}, 30 + n, "flat"))
    for k, levels in [(16, 11), (24, 10)]:
        vals = random.Random(300 + k).sample(range(256), k * levels)
        out.append(_lit(f"ties{k}x{levels}", {v: 1 << (j // k) for j, v in enumerate(vals)}, 40 + k, "ties"))
    return out


def _cl_hist_of_literals(freqs):
    h = [0] * 257
    for v, c in freqs.items():
        h[v] = c
    h[256] = 1
    seq = P.cl_rle(P.package_merge(h, 15) + [0])
    clh = [0] * 19
    for s, _ in seq:
        clh[s] += 1
    return clh


def _cl_limit(seed=7, want=4, max_tries=200):
    """Seeded search: literal histograms with c_t symbols of frequency 2^t, c_t drawn from a Fibonacci
    list, 8..14 tiers; a hit is one whose code-length histogram needs the 7-bit limit."""
    rng = random.Random(seed)
    out = []
    for t in range(max_tries):
        counts = [rng.choice([1, 1, 2, 3, 5, 8, 13, 21, 34]) for _ in range(rng.randrange(8, 15))]
        if sum(counts) > 256 or sum(c << i for i, c in enumerate(counts)) > 65535:
            continue
        vals = rng.sample(range(256), sum(counts))
        freqs, j = {}, 0
        for i, c in enumerate(counts):
            for _ in range(c):
                freqs[vals[j]] = 1 << i
                j += 1
        clh = _cl_hist_of_literals(freqs)
        if P.package_merge(clh, 7) != P.package_merge(clh, 15):
            out.append(_lit(f"tiers_try{t}", freqs, 50 + t, "cl7"))
            if len(out) == want:
                break
    return out


def _unique_copies(seed, plan, prefix, run=4):
    """`prefix` random bytes, then per entry of `plan` (a distance code) 4 fresh random bytes and a
    `run`-byte copy whose source, at a distance inside that code, is a window that occurs once in
    everything before it (so the copy has exactly one candidate match and no tie-break is involved).
    The byte before the copy differs from the byte before its source, so no match starts early.
    Returns (data, [(position, distance)]) or None when the parse is not the planned one."""
    rs = np.random.RandomState(seed)
    data = bytearray(rs.bytes(prefix))
    cnt = collections.Counter(bytes(data[i:i + run]) for i in range(prefix - run + 1))
    copies = []
    for code in plan:
        p = len(data) + 4
        lo, hi = DIST_BASE[code], min(DIST_BASE[code] + (1 << DIST_EXTRA[code]) - 1, p - 1)
        for _ in range(200):
            d = int(rs.randint(max(lo, 2 * run), hi + 1))
            g = bytes(data[p - d:p - d + run])
            if cnt[g] == 1:
                break
        else:
            return None
        fresh = bytearray(rs.bytes(4))
        while fresh[3] == data[p - d - 1]:
            fresh[3] = int(rs.randint(256))
        old = len(data)
        data += fresh + g
        for i in range(old - run + 1, len(data) - run + 1):
            cnt[bytes(data[i:i + run])] += 1
        copies.append((p, d))
    # the greedy parse with min_run = max_run = run, distances 1..32768: exactly the planned copies
    data = bytes(data)
    where = collections.defaultdict(list)
    planned = dict(copies)
    i = 0
    for q in range(len(data) - run + 1):
        where[data[q:q + run]].append(q)
    while i + run <= len(data):
        c = [q for q in where[data[i:i + run]] if q < i and i - q <= 32768]
        if i in planned:
            if [i - q for q in c] != [planned[i]]:
                return None
            i += run
        else:
            if c:
                return None
            i += 1
    return data, copies


def _dist_plan(first, counts, seed):
    plan = [first + i for i, c in enumerate(counts) for _ in range(c)]
    random.Random(seed).shuffle(plan)
    hist = [0] * 30
    for c in plan:
        hist[c] += 1
    return plan, hist


def _dist_limit():
    """17 distance codes with Fibonacci counts 1, 1, 2, ..., 1597 (4 180 copies of 4 bytes, encoded
    with min_run = max_run = 4): codes 13..29 and 12..28 with the near codes rare, and codes 13..29
    with the far codes rare.  The last is possible within 65 536 bytes because a source may be any
    window that is still unique, not only a fresh 4-byte group."""
    out = []
    fib = _fib(17)
    for name, first, counts in [("fib_to29", 13, fib), ("fib_to28", 12, fib), ("fib_far_rare", 13, fib[::-1])]:
        for seed in range(1000, 1040):
            plan, hist = _dist_plan(first, counts, seed)
            r = _unique_copies(seed, plan, 28672)
            if r is not None:
                break
        else:
            raise AssertionError(f"dist_limit {name}: no seed gives the planned parse")
        out.append(Case(name, r[0], ("lz", (True, 4, 4, 1, 32768), 65536, 32768), ("dist15", hist), r[1]))
    return out


def _dist_fixups():
    rs = np.random.RandomState(77)
    far = rs.bytes(24590)
    mid = rs.bytes(150)
    runs = b"a" * 40 + b"bc" + b"d" * 300 + b"e"
    full = (True, 3, 258, 1, 32768)
    # (True, 3, 258, 1, 1) and (True, 0, 0, 0, 0) are the RLE / LITERAL presets (the split or fused
    # kernels); any other parameters take the LZ77 kernel, so each fix-up is named once per route
    return [
        Case("only_code0_rle", runs, ("lz", RLE, 65536, 32768), ("one_dist", 0)),
        Case("only_code0_lz", runs, ("lz", (True, 3, 257, 1, 1), 65536, 32768), ("one_dist", 0)),
        Case("only_code29", far + far[:9], ("lz", (True, 3, 258, 24577, 32768), 65536, 32768), ("one_dist", 29)),
        Case("only_code13", mid + mid[50:58], ("lz", (True, 3, 258, 100, 100), 65536, 32768), ("one_dist", 13)),
        Case("no_dist_literal", mid * 2, ("lz", (True, 0, 0, 0, 0), 65536, 32768), ("no_dist", None)),
        Case("no_dist_lz", mid, ("lz", (True, 258, 258, 1, 32768), 65536, 32768), ("no_dist", None)),
        Case("empty_rle", b"", ("lz", RLE, 65536, 32768), ("no_dist", None)),
        Case("empty_literal", b"", ("lz", (True, 0, 0, 0, 0), 65536, 32768), ("no_dist", None)),
        Case("empty_lz", b"", ("lz", full, 65536, 32768), ("no_dist", None)),
    ]


def cl_runs_sweep_chunks():
    """512-byte chunks whose literal code lengths are two symbols a zero run of a chosen length apart,
    or k consecutive byte values: the zero runs 0..4, 9..12, 137..141, 200, 254 and their
    remainders, and non-zero runs of many lengths."""
    chunks = []
    for gap in [0, 1, 2, 3, 4, 9, 10, 11, 12, 137, 138, 139, 140, 141, 200, 254]:
        for a in [0, 1, 7, 100]:
            b = a + gap + 1
            if b <= 255:
                chunks.append(bytes([a, b]) * 256)
    for k in [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 64, 128, 256]:
        for start in [0, 3, 238]:
            if start + k <= 256:
                chunks.append((bytes(range(start, start + k)) * (512 // k + 1))[:512])
    return chunks


def _run_chunk(L, start, seed):
    """A chunk in which exactly the byte values start .. start+L-1 get one common code length l
    (2^l > L), as a maximal run: each occurs once, and symbols from 200 upwards, with the
    end-of-block symbol, take the rest of the Kraft sum with frequencies 2^j, so the histogram is
    dyadic and every optimal code has exactly these lengths."""
    l = L.bit_length()
    freqs = {start + i: 1 for i in range(L)}
    rest = (1 << l) - L                     # in units of 2^-l; its lowest set bit ends in the EOB symbol
    nxt = 200
    low = rest & -rest
    for j in range(l - 1, -1, -1):
        if rest >> j & 1 and (1 << j) != low:
            freqs[nxt] = 1 << j
            nxt += 3
    j = low.bit_length() - 1                # 2^j = 2^(j-1) + ... + 2 + 1 + 1 (the last 1 is the EOB)
    for t in range(j - 1, -1, -1):
        freqs[nxt] = 1 << t
        nxt += 3
    assert nxt <= 256 and start + L <= 200
    return _shuffled(freqs, seed)


def _cl_runs():
    lit = ("LITERAL_DYNAMIC", "RLE_DYNAMIC")
    out = [Case("sweep512", b"".join(cl_runs_sweep_chunks()), ("preset", lit, 512, 0), "cl_runs")]
    for L in [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 66, 128]:
        for start in [0, 3, 4, 5]:
            out.append(Case(f"run{L}_at{start}", _run_chunk(L, start, 1000 * L + start),
                            ("preset", lit, 65536, 32768), ("run", L, start)))
    return out


def _all_symbols():
    hl = bytearray()
    for r in range(3, 259):
        hl += bytes([r & 255]) * (r + 1)
    hl += bytes(range(256))
    # every length symbol against every distance code: copies of one length per symbol from one
    # distance per code, two fresh bytes between copies (the parse may merge or move a few; the
    # condition on the oracle's stream says whether all 29 + 30 symbols are still there)
    rs = np.random.RandomState(5)
    lz = bytearray(rs.bytes(24700))
    for rep in range(3):
        for i in range(30):
            run = LEN_BASE[(i + 7 * rep) % 29] + (rep if LEN_EXTRA[(i + 7 * rep) % 29] else 0)
            d = min(DIST_BASE[i] + (int(rs.randint(1 << DIST_EXTRA[i])) if DIST_EXTRA[i] else 0), len(lz))
            for _ in range(run):
                lz.append(lz[-d])
            lz += rs.bytes(2)
    for i in range(29):
        d = DIST_BASE[10 + i % 20]
        for _ in range(LEN_BASE[i]):
            lz.append(lz[-d])
        lz += rs.bytes(2)
    return [Case("hlit286", bytes(hl), ("preset", ("RLE_DYNAMIC",), 65536, 32768), "hlit286"),
            Case("lz_all_codes", bytes(lz), ("lz", (True, 3, 258, 1, 32768), 65536, 32768), "hlit286_hdist30")]


_GEN = {"lit_limit": _lit_limit, "cl_limit": _cl_limit, "dist_limit": _dist_limit, "dist_fixups": _dist_fixups,
        "cl_runs": _cl_runs, "all_symbols": _all_symbols}


@functools.lru_cache(maxsize=None)
def cases(cls):
    """The cases of one class (built once per process; every generator is seeded)."""
    return tuple(_GEN[cls]())
