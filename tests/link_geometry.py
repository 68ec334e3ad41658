"""Hand-built streams for the decoder's candidate list and chain linking at their list, tile and range limits.

Between the count pass and the emit pass the decoder (csrc/capi/ndfl_inflate.cpp, Decode::devlink) turns the
header finder's per-segment lists into one sorted candidate list (ndfl_inflate_segsum / segscan / compact /
cand_slice), marks stored-header aliases (alias_mark / alias_copy), orders the chains for the count pass
(order_count / order), links them from the range start by pointer jumping (link_init / jump / path), orders the
linked chains for the emit pass (emit_order_count / emit_order) and picks the first error (first_error / summary).
The host linker, Decode::hostlink (NDFL_HOST_LINK=1), is a second implementation of the same stage.  Every one of
these has a limit at an exact count or bit position: tiles of SCAN_TILE = 2,048 items, 256-thread grid-stride
loops, ceil(log2 n) jump levels, 24 buckets of 32 Kibit, the 10-bit alias window, two binary searches on the range,
an atomicMin.  No stream written by an encoder chooses its chain structure; these do:

    Build                      a stream under construction: dyn / fixed / stored blocks, every block's seam (the bit of
                               its BFINAL bit) and the output offset at it; the expected bytes as it goes
    the code                   ONE dynamic code for every dynamic block (literals 0..224 and length 3 in 8 bits, the
                               rest in 9; distances in 4 and 5 bits), sent under a code-length code of 7-bit codes:
                               a header of 2,283 bits, so that a block of a few tokens is still 290 bytes and a 64 KiB
                               finder segment holds at most 229 of them
    model                      restated from the kernels, not imported from them: the candidate list, the alias
                               representatives, the count and emit buckets, the linked chain list, timings[5..7]

Families (cases(name)): L list length and jump levels, B bucket orders, A stored-header aliases, D decoy headers (the
links form a forest), E first error and partial input, R range slices, O over the segment cap.  A chain starts at
bit 0 (the range start) and at every accepted non-final stored or dynamic header; a final block is no chain start, so
a stream of N chains is N non-final dynamic blocks and a small final fixed block that rides in the last chain.

The segment-cap condition: the decoder keeps at most SEG_CAP = 256 accepted headers per 64 KiB of input, and which
ones it keeps is not pinned, so every stream but family O's holds at most 256 per segment (test_link_geometry_cpu).

Test infrastructure only.
"""
import collections
import functools
import random

import oracle_lib as O
import pyref_deflate as P
import token_stream as TS

# ---- the decoder's constants (restated; test_link_geometry_cpu reads them out of the sources) --------------------
SCAN_TILE, SEG_CAP, SEG_BYTES, OB_NB, ALIAS_WINDOW = 2048, 256, 65536, 24, 10
NONE = (1 << 64) - 1
NEED_INPUT, E_ARG, E_CAPACITY = 64, -1, -3
RESERVED, COPY_BEFORE, UEOS = "RESERVED_BLOCK_TYPE", TS.COPY_BEFORE, "UNEXPECTED_END_OF_STREAM"
REV8 = bytes(int(format(v, "08b")[::-1], 2) for v in range(256))


def reason_code(reason):
    return 0 if reason is None else O.REASONS.index(reason) + 1


# ---- the bit writer's bulk path ---------------------------------------------------------------------------------
def flush(w):
    """Every whole byte of the writer's accumulator into its buffer (TS.BitWriter.bits leaves up to 31 bits)."""
    nbytes = w.k >> 3
    if nbytes:
        w.buf += (w.acc & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")
        w.acc >>= 8 * nbytes
        w.k -= 8 * nbytes


def put_bits(w, v, n):
    """n bits of v (any n) at the writer's position."""
    assert v >> n == 0
    w.acc |= v << w.k
    w.k += n
    flush(w)


# ---- the one dynamic code -----------------------------------------------------------------------------------------
LIT_LENS = [8] * 225 + [9] * 31 + [9] + [8] + [9] * 28      # 226 codes of 8 bits, 60 of 9: complete
DIST_LENS = [4, 4] + [5] * 28                               # complete
CL_WIDE = {0: 1, 1: 2, 2: 3, 3: 4, 6: 5, 4: 7, 5: 7, 8: 7, 9: 7}   # the four lengths in use cost 7 bits each
LC = P.canonical(LIT_LENS, 15)
DC = P.canonical(DIST_LENS, 15)
WIDE_HDR_BITS = 17 + 3 * 18 + 7 * 316
EOB_BITS = 9
assert LC[256][0] >> 8 == 1     # the end of block's last bit is a 1: no stored header after it is found a bit early
RUN_UNIT = (LC[285][0] | DC[0][0] << 9, 13)                 # (258, 1): 9 + 4 bits


@functools.lru_cache(maxsize=None)
def _header(final):
    cl = [0] * 19
    for s, l in CL_WIDE.items():
        cl[s] = l
    w = TS.BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(286 - 257, 5)
    w.bits(30 - 1, 5)
    reo = [cl[s] for s in P.CLC_ORDER]
    ncl = 19
    while ncl > 4 and reo[ncl - 1] == 0:
        ncl -= 1
    w.bits(ncl - 4, 4)
    for i in range(ncl):
        w.bits(reo[i], 3)
    cc = P.canonical(cl, 7)
    for l in LIT_LENS + DIST_LENS:
        w.bits(*cc[l])
    assert w.n == WIDE_HDR_BITS
    return int.from_bytes(w.getbytes(), "little"), w.n


def enc_tokens(toks):
    v = n = 0
    for t in toks:
        if t[0] == "L":
            c, l = LC[t[1]]
            v |= c << n
            n += l
        else:
            (ls, lne, lex), (ds, dne, dex) = P.len_sym(t[1]), P.dist_sym(t[2])
            c, l = LC[ls]
            v |= (c | lex << l) << n
            n += l + lne
            c, l = DC[ds]
            v |= (c | dex << l) << n
            n += l + dne
    return v, n


def enc_dyn(parts, final=False):
    """One dynamic block as (value, bits).  parts: bytes (a run of 8-bit literals, values under 225), ("RUN", n)
    (n copies (258, 1)), or a list of ("L", b) / ("M", length, distance) tokens."""
    v, n = _header(final)
    for p in parts:
        if isinstance(p, (bytes, bytearray)):
            assert not p or max(p) < 225
            pv, pn = int.from_bytes(bytes(p).translate(REV8), "little"), 8 * len(p)
        elif isinstance(p, tuple):
            assert p[0] == "RUN"
            pv, pn = RUN_UNIT[0] * (((1 << (13 * p[1])) - 1) // ((1 << 13) - 1)), 13 * p[1]
        else:
            pv, pn = enc_tokens(p)
        v |= pv << n
        n += pn
    c, l = LC[256]
    return v | c << n, n + l


def produce(parts, before):
    """The bytes the parts decode to after the output `before`: (bytes, None), or (the bytes before the offending
    token, COPY_BEFORE).  Token lists go through token_stream.expand."""
    out = bytearray(before[-32768:])
    base = len(out)
    for p in parts:
        if isinstance(p, (bytes, bytearray)):
            out += p
        elif isinstance(p, tuple):
            out += out[-1:] * (258 * p[1])
        else:
            reason, got = TS.expand([p], bytes(out[-32768:]))
            out += got
            if reason is not None:
                return bytes(out[base:]), reason
    return bytes(out[base:]), None


# 8-bit literals whose codes hold no two zero bits in a row and begin and end with a one: a run of them holds no
# "00", so no header of any kind (a chain start has BFINAL = 0 and a BTYPE of 00 or 10: two zero bits in three)
SAFE = [v for v in range(225) if "00" not in format(v, "08b") and format(v, "08b")[0] == format(v, "08b")[7] == "1"]


def safe_lits(rng, n):
    return bytes(rng.choice(SAFE) for _ in range(n))


def filler(rng, n):
    """n bytes that hold no header: bit 0 (BFINAL) and bits 1..2 (the reserved block type) set in every byte, so a
    stored header read at bits 3..7 finds LEN and NLEN with equal low bits."""
    return bytes(0x07 | rng.randrange(32) << 3 for _ in range(n))


# ---- the stream builder -----------------------------------------------------------------------------------------
class Build:
    """A stream under construction.  seams[i]: the bit of block i's BFINAL bit; outs[i]: the output offset there;
    out: the expected bytes (up to the first COPY_FROM_BEFORE_DICTIONARY_START token: err = its output offset)."""

    def __init__(self):
        self.w = TS.BitWriter()
        self.seams, self.kinds, self.outs = [], [], []
        self.out = bytearray()
        self.err = None
        self.end = None

    def _add(self, kind, produced, reason=None):
        self.kinds.append(kind)
        if self.err is None:
            self.out += produced
            if reason is not None:
                self.err = len(self.out)

    def _open(self, final):
        self.seams.append(self.w.n)
        self.outs.append(len(self.out))
        if final:
            assert self.end is None
            self.end = -1

    def _close(self):
        flush(self.w)
        if self.end == -1:
            self.end = self.w.n

    def dyn(self, parts, final=False):
        self._open(final)
        put_bits(self.w, *enc_dyn(parts, final))
        self._add("dynamic", *produce(parts, self.out))
        self._close()

    def pre(self, kind, v, n, produced, final=False):
        """A block encoded before (value, bits) that decodes to `produced` wherever it stands."""
        self._open(final)
        put_bits(self.w, v, n)
        self._add(kind, produced)
        self._close()

    def fixed(self, toks, final=False):
        self._open(final)
        put_bits(self.w, *enc_fixed(tuple(toks), final))
        self._add("fixed", *produce([list(toks)], self.out))
        self._close()

    def stored(self, data, final=False):
        """The direct stored-block writer: header, padding, LEN / NLEN, then the bytes as they are."""
        assert len(data) <= 65535
        self._open(final)
        w = self.w
        put_bits(w, 1 if final else 0, 3)
        put_bits(w, 0, -w.n % 8)
        assert w.k == 0
        w.buf += len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + bytes(data)
        self._add("stored", bytes(data))
        self._close()

    def raw(self, data):
        """Bytes after the final block."""
        put_bits(self.w, 0, -self.w.n % 8)
        self.w.buf += bytes(data)


@functools.lru_cache(maxsize=None)
def enc_fixed(toks, final):
    w = TS.BitWriter()
    TS.write_block(w, list(toks), "fixed", final)
    return int.from_bytes(w.getbytes(), "little"), w.n


def flip(comp, bit):
    b = bytearray(comp)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


Case = collections.namedtuple("Case", "name family comp seams kinds outs start_bit end_bit window partial code out bits "
                                      "stop_at silent info")
Case.__doc__ = """One decode.  comp: the input; seams / kinds / outs: per block (outs: the output offset at its seam, of the
whole stream); start_bit, end_bit (None: to the final block), window: the range (a whole-stream case: 0, None, b"");
partial: NDFL_IN_PARTIAL; code, out, bits: the expected return code, bytes and consumed bits; stop_at: the bit where
the count pass's linked list ends (the model cuts the chain list after the chain that holds it); silent: include/ndfl.h
does not say what the call returns, the device path is pinned to the host-link path; info: what the case is named
for."""


def case(name, family, b, comp=None, *, start=0, end=None, window=b"", partial=False, code=0, out=None, bits=None,
         stop_at=None, silent=False, info=None):
    comp = b.w.getbytes() if comp is None else comp
    out = bytes(b.out) if out is None else out
    if bits is None:
        bits = b.end
    if stop_at is None:
        stop_at = b.seams[-1] if end is None else end - 1
    return Case(name, family, comp, tuple(b.seams), tuple(b.kinds), tuple(b.outs), start, end, window, partial, code, out,
                bits, stop_at, silent, info or {})


# ---- the model ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def scan(comp):
    """The finder's accepted headers over the whole input (oracle_lib.scan_headers)."""
    return tuple(O.scan_headers(comp))


def candidates(c):
    """The decode's candidate list: slot 0 is the range start, then the accepted headers strictly inside
    (start_bit, end_bit) (ndfl_inflate_cand_slice_kernel's two binary searches)."""
    end = NONE if c.end_bit is None else c.end_bit
    return [c.start_bit] + [p for p in scan(c.comp) if c.start_bit < p < end]


def stored_key(comp, p):
    """(LEN position, BFINAL) of a stored header read at bit p, else None (stored_key in inflate_kernels.hip)."""
    h = (int.from_bytes(comp[p >> 3:(p >> 3) + 2], "little") >> (p & 7)) & 7
    if h >> 1 or p + 3 > 8 * len(comp):
        return None
    return ((p + 3 + 7) & ~7, h & 1)


def alias_reps(comp, cands, window=ALIAS_WINDOW):
    """Per candidate index k, the index counted for it: the lowest index at most ALIAS_WINDOW bits before it (walking
    down while cands[j - 1] + 10 >= cands[k]) with the same stored key; else k."""
    reps = []
    for k, p in enumerate(cands):
        key, rep, j = stored_key(comp, p), k, k
        if key is not None:
            while j > 0 and cands[j - 1] + window >= p:
                if stored_key(comp, cands[j - 1]) == key:
                    rep = j - 1
                j -= 1
        reps.append(rep)
    return reps


def alias_groups(c):
    """{representative candidate index: [the indices that take its result]} for the groups of more than one."""
    g = collections.defaultdict(list)
    for k, r in enumerate(alias_reps(c.comp, candidates(c))):
        g[r].append(k)
    return {r: ks for r, ks in g.items() if len(ks) > 1}


def count_buckets(c):
    """Per candidate, the count pass's claim bucket (OrderBucket): 23 - min(23, bits to the next candidate >> 15), the
    last one's to end_bit; None for an alias (bucket OB_NB: left out of the order)."""
    cands = candidates(c)
    reps = alias_reps(c.comp, cands)
    end = NONE if c.end_bit is None else c.end_bit
    res = []
    for k, p in enumerate(cands):
        nx = cands[k + 1] if k + 1 < len(cands) else end
        res.append(OB_NB - 1 - min(OB_NB - 1, (nx - p) >> 15) if reps[k] == k else None)
    return res


def chain_list(c):
    """The linked chain list: the range start and every true seam inside the range that is a candidate, cut after the
    chain that holds stop_at (the first error the count pass sees, the final block, the range end)."""
    cs = set(candidates(c)[1:])
    lst = [c.start_bit] + [s for s in c.seams if s in cs]
    return [s for s in lst if s <= c.stop_at]


def emit_buckets(c):
    """Per linked chain of a valid whole-stream case, the emit pass's claim bucket (EmitBucket)."""
    assert c.code == 0 and c.end_bit is None and c.start_bit == 0
    lst = chain_list(c)
    off = dict(zip(c.seams, c.outs))
    off[0] = 0
    res = []
    for i, s in enumerate(lst):
        e, o = (lst[i + 1], off[lst[i + 1]]) if i + 1 < len(lst) else (c.bits, len(c.out))
        res.append(OB_NB - 1 - min(OB_NB - 1, ((e - s) >> 15) + ((o - off[s]) >> 14)))
    return res


def timings(c):
    """The model's ndfl_ctx_timings entries [5] linked chains and [7] header candidates ([6], repaired boundaries, is
    0: a chain stops at candidates and at the range end only, so it never stops on a boundary that needs repair)."""
    return len(chain_list(c)), len(candidates(c))


def segment_counts(comp):
    """Accepted headers per 64 KiB finder segment."""
    return collections.Counter(p // (8 * SEG_BYTES) for p in scan(comp))


def named_stored_headers(c):
    """What a stored block's header is found as, from the bits alone: per non-final stored block, the positions
    q in [LEN position - 10, LEN position - 3] whose bits up to the LEN position are all zero."""
    bit = lambda q: c.comp[q >> 3] >> (q & 7) & 1
    res = {}
    for s, kind in zip(c.seams, c.kinds):
        if kind != "stored" or bit(s):
            continue
        al = (s + 3 + 7) & ~7
        res[s] = [q for q in range(max(0, al - 10), al - 2) if all(not bit(x) for x in range(q, al))]
    return res


# ---- family L: list length and jump levels ------------------------------------------------------------------------------
L_NS = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]
POOL = 4100                                     # chain blocks of the pool (families E and R use all of them)
FINAL_TOKS = (("L", 0x45), ("M", 5, 9), ("L", 0x4E), ("L", 0x44))


def pool_tokens(i):
    """Block i's tokens: 20 bytes that name the block (i mod 251, i // 251), copies into the previous block."""
    r = random.Random(0x1000 + i)
    toks = [("L", i % 251), ("L", i // 251)] + [("L", r.randrange(256)) for _ in range(4)]
    toks.append(("M", 6, 18) if i else ("M", 6, 5))
    toks += [("L", r.randrange(256)) for _ in range(5)] + [("M", 3, 2)]
    return toks


@functools.lru_cache(maxsize=None)
def pool():
    """(tokens, dynamic (value, bits), produced bytes) per pool block; the blocks decode one after the other."""
    out = bytearray()
    res = []
    for i in range(POOL):
        toks = pool_tokens(i)
        got, reason = produce([toks], out)
        assert reason is None and len(got) == 20
        out += got
        res.append((toks, enc_dyn([toks]), got))
    return res


def pool_stream(n, fixed_at=(), replace=None):
    """Pool blocks 0..n-1 (those in fixed_at as fixed blocks; replace: {index: function(Build)} writes something else
    there) and the final fixed block."""
    b = Build()
    pl = pool()
    for i in range(n):
        toks, (v, nb), got = pl[i]
        if replace:                                 # (a block's copies reach into the block before it)
            got = produce([toks], b.out)[0]
        if replace and i in replace:
            replace[i](b)
        elif i in fixed_at:
            b.pre("fixed", *enc_fixed(tuple(toks), False), got)
        else:
            b.pre("dynamic", v, nb, got)
    b.fixed(FINAL_TOKS, final=True)
    return b


def _family_l():
    res = []
    for n in L_NS:
        res.append(case(f"L_{n}", "L", pool_stream(n), info={"N": n, "chains": n}))
        # the last chain block fixed: its chain is absent, the chain before it holds it and the final block
        res.append(case(f"L_{n}_fixedlast", "L", pool_stream(n, fixed_at={n - 1}), info={"N": n, "chains": max(1, n - 1)}))
    return res


# ---- family E: first error and partial input ---------------------------------------------------------------------------
E_TS = [0, 1, 2047, 2048, 2049, POOL - 1]


def reserved_at(b, comp, k):
    """comp with block k's header turned into BTYPE 3 (a dynamic block: bit 1; a fixed one: bit 2)."""
    return flip(comp, b.seams[k] + (1 if b.kinds[k] == "dynamic" else 2))


def _error_case(name, family, b, comp, k, info):
    reason, out, bits = O.inflate(comp, out_cap=len(b.out) + 1024)
    assert reason == RESERVED
    return case(name, family, b, comp, code=reason_code(RESERVED), out=bytes(b.out[:b.outs[k]]), bits=bits,
                stop_at=b.seams[k], info=info)


def thin_stream(errors):
    """POOL chain blocks of four literals each (16,400 bytes in all: every distance of 32,768 reaches before the
    stream), those in `errors` with a (3, 32768) copy after their first literal: the count pass links every chain, the
    emit pass reports COPY_FROM_BEFORE_DICTIONARY_START in each of them."""
    b = Build()
    for i in range(POOL):
        lits = bytes([i % 225, i // 225, (7 * i) % 225, (13 * i + 5) % 225])
        b.dyn([[("L", lits[0]), ("M", 3, 32768), ("L", lits[1])]] if i in errors else [lits])
    b.fixed(FINAL_TOKS, final=True)
    return b


def two_block_chain(b):
    r = random.Random(0xE2)
    b.stored(filler(r, 300))
    b.fixed([("L", r.randrange(256)) for _ in range(12)])


def _family_e():
    res = []
    base = pool_stream(POOL)
    comp = base.w.getbytes()
    for t in E_TS:
        res.append(_error_case(f"E_reserved_t{t}", "E", base, reserved_at(base, comp, t + 1), t + 1, {"t": t}))
    two = reserved_at(base, reserved_at(base, comp, 3501), 1001)
    res.append(_error_case("E_reserved_two_tiles", "E", base, two, 1001, {"t": 1000, "later": 3500}))
    # errors only the emit pass sees: every chain is linked, the first in stream order wins
    errs = (10, 2100, 3000, POOL - 1)
    tb = thin_stream(errs)
    tcomp = tb.w.getbytes()
    reason, out, bits = O.inflate(tcomp)
    assert reason == COPY_BEFORE and len(out) == tb.err == 4 * errs[0] + 1
    # (the count pass does not see these errors: it sizes the output by every chain's bytes, which out_cap must hold)
    total = 4 * POOL + 4 * len(errs) + 8
    res.append(case("E_copy_before_four_tiles", "E", tb, code=reason_code(COPY_BEFORE), bits=bits,
                    info={"t": errs[0], "later": errs[1:], "emit_only": True, "cap": total}))
    # partial input (ndfl_inflate_range, end_bit = UINT64_MAX, NDFL_IN_PARTIAL), truncated ...
    for t in E_TS:
        # ... inside the block of chain t
        cut = (base.seams[t] + WIDE_HDR_BITS + 60) // 8
        assert base.seams[t] + WIDE_HDR_BITS < 8 * cut < base.seams[t + 1]
        res.append(case(f"E_partial_in_block_t{t}", "E", base, comp[:cut], partial=True, code=NEED_INPUT,
                        out=bytes(base.out[:base.outs[t]]), bits=base.seams[t], stop_at=8 * cut, info={"t": t, "cut": cut}))
        # ... inside the second block of a two-block chain (a stored candidate, then a fixed block), and exactly on
        # that block's seam
        vb = pool_stream(POOL, replace={t: two_block_chain})
        vcomp = vb.w.getbytes()
        fx = t + 1                                  # (block t is the stored one, t + 1 the fixed one)
        assert vb.kinds[t:t + 2] == ["stored", "fixed"] and vb.seams[fx] % 8 == 0
        cut = (vb.seams[fx] + 40) // 8
        assert vb.seams[fx] + 3 < 8 * cut < vb.seams[fx + 1] - 7
        res.append(case(f"E_partial_in_second_block_t{t}", "E", vb, vcomp[:cut], partial=True, code=NEED_INPUT,
                        out=bytes(vb.out[:vb.outs[fx]]), bits=vb.seams[fx], stop_at=8 * cut,
                        info={"t": t, "cut": cut, "stored": vb.seams[t]}))
        # (include/ndfl.h speaks of an input that ends inside a block; it is silent on one that ends on a seam)
        cut = vb.seams[fx] // 8
        res.append(case(f"E_partial_on_seam_t{t}", "E", vb, vcomp[:cut], partial=True, code=NEED_INPUT,
                        out=bytes(vb.out[:vb.outs[fx]]), bits=vb.seams[fx], stop_at=8 * cut, silent=True,
                        info={"t": t, "cut": cut, "stored": vb.seams[t]}))
    return res


# ---- family R: range slices -------------------------------------------------------------------------------------------
R_PAIRS = [(0, 1), (0, 2), (1, 2), (0, 255), (0, 256), (1, 257), (255, 256), (0, 2047), (0, 2048), (1, 2049), (3, 2051),
           (2047, 2048), (2040, 2050), (2048, None)]


def _range_case(name, b, comp, i, j, **kw):
    """Seam i to seam j (None: to the final block) of stream b with expand's last 32 KiB before seam i as the window."""
    lo = b.outs[i]
    hi = len(b.out) if j is None else b.outs[j]
    return case(name, "R", b, comp, start=b.seams[i], end=None if j is None else b.seams[j],
                window=bytes(b.out[max(0, lo - 32768):lo]), out=bytes(b.out[lo:hi]),
                bits=b.end if j is None else b.seams[j], info=dict({"i": i, "j": j}, **kw))


def _family_r():
    res = []
    base = pool_stream(POOL)
    comp = base.w.getbytes()
    for i, j in R_PAIRS:
        res.append(_range_case(f"R_{i}_{'end' if j is None else j}", base, comp, i, j))
    # the range end one bit off a seam: a block straddles it (LF_RANGE)
    for d in (-1, 1):
        c = _range_case(f"R_end_seam{d:+d}", base, comp, 2, 7)
        res.append(c._replace(end_bit=c.end_bit + d, code=E_ARG, out=b"", bits=0))
    # boundaries that are no candidates: a fixed block's start and the final block's start as the range end, a fixed
    # block's start as the range start
    n = 2050
    fb = pool_stream(n, fixed_at={n - 1, 5})
    fcomp = fb.w.getbytes()
    res.append(_range_case("R_end_on_fixed_start", fb, fcomp, n - 4, n - 1, boundary="fixed"))
    res.append(_range_case("R_end_on_final_start", fb, fcomp, n - 4, n, boundary="final"))
    res.append(_range_case("R_end_on_fixed_start_long", fb, fcomp, 0, n - 1, boundary="fixed"))
    res.append(_range_case("R_start_on_fixed_start", fb, fcomp, n - 1, None, boundary="fixed"))
    res.append(_range_case("R_start_on_fixed_start_mid", fb, fcomp, 5, 300, boundary="fixed"))
    # aliases of the start header just before start_bit, and stored candidates inside the range
    ab = _alias_stream_offsets()
    acomp = ab.w.getbytes()
    k = ab.kinds.index("stored")
    assert len(named_stored_headers(case("x", "R", ab))[ab.seams[k]]) > 1
    res.append(_range_case("R_start_after_its_aliases", ab, acomp, k, None, boundary="stored"))
    res.append(_range_case("R_start_after_its_aliases_short", ab, acomp, k, k + 4, boundary="stored"))
    return res


# ---- family A: stored-header aliases -------------------------------------------------------------------------------------
def fixed_ending_at(off, seed):
    """Fixed-block literals whose block, started on a byte, ends `off` bits into a byte: 3 + 8 a + 9 b + 7."""
    nb = (off - 2) % 8
    r = random.Random(seed)
    return [("L", r.randrange(144)) for _ in range(2)] + [("L", 144 + r.randrange(112)) for _ in range(nb)]


def _alias_stream_offsets():
    """A stored block after a fixed block that ends at each of the 8 bit offsets (the fixed end of block is seven
    zero bits: the aliases lie before the true header, inside the previous block), each followed by a stored block
    (it puts the next fixed block on a byte)."""
    b = Build()
    r = random.Random(0xA0)
    for off in range(8):
        assert b.w.n % 8 == 0
        b.fixed(fixed_ending_at(off, 0xA00 + off))
        assert b.w.n % 8 == off
        b.stored(filler(r, 40))
    b.fixed(FINAL_TOKS, final=True)
    return b


def _family_a():
    res = []
    r = random.Random(0xA1)
    res.append(case("A_after_fixed_offsets", "A", _alias_stream_offsets(), info={"groups": 8}))
    # a header byte of 0x00: the aliases lie after the true header, at bits +1 .. +5
    b = Build()
    b.stored(filler(r, 50) + b"\xff")
    b.stored(filler(r, 50))
    b.fixed(FINAL_TOKS, final=True)
    res.append(case("A_header_byte_00", "A", b, info={"sizes": {b.seams[1]: 6}}))
    # k consecutive empty stored blocks: candidates 40 bits apart against the 10-bit window
    b = Build()
    b.dyn([bytes(range(30))])
    for _ in range(8):
        b.stored(b"")
    b.fixed(FINAL_TOKS, final=True)
    res.append(case("A_empty_stored_x8", "A", b, info={"sizes": {s: 6 for s in b.seams[2:9]}}))
    # the stream begins with a stored block: its aliases have representative slot 0
    b = Build()
    b.stored(filler(r, 60))
    b.dyn([bytes(range(40))])
    b.fixed(FINAL_TOKS, final=True)
    res.append(case("A_first_block_stored", "A", b, info={"rep0": 6}))
    # an alias group that straddles a 64 KiB finder segment edge: bits 524,286 .. 524,293
    b = Build()
    b.stored(b"\xff" * 65523)                   # 5 + 65,523 bytes, then a fixed block of 8 bytes up to byte 65,536
    b.fixed([("L", 200 + i) for i in range(6)])
    assert b.w.n == 8 * SEG_BYTES
    b.stored(filler(r, 80))
    b.fixed(FINAL_TOKS, final=True)
    res.append(case("A_group_on_segment_edge", "A", b, info={"sizes": {b.seams[2]: 8}, "edge": 8 * SEG_BYTES}))
    # an alias group that straddles candidate index 256: 42 groups of 6 before it (indices 0 .. 251), the first in
    # segment 0 and 41 empty stored blocks in segment 1 (none has 65,535 bytes behind it: its LEN field, 16 zero bits
    # and FFFF, would read as a stored header of that length)
    b = Build()
    b.stored(b"\xff" * 65535)
    for _ in range(41):
        b.stored(b"")
    b.fixed(fixed_ending_at(0, 0xA66))
    b.stored(filler(r, 80))
    b.fixed(FINAL_TOKS, final=True)
    res.append(case("A_group_on_index_256", "A", b, info={"index": 256, "stored": b.seams[-2]}))
    res.append(_lookalike_case())
    return res


# A dynamic header that reads as a stored header from its second byte on: HDIST = 0 and HCLEN = 8 make that byte
# 0x00, and these code-length code lengths (for the symbols 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4; found by search:
# a complete code with lengths for 0, 8 and 9) put LEN = 10,241 into bytes 2 .. 3 and its complement into bytes 4 .. 5.
LOOKALIKE_CL = [0, 0, 0, 2, 1, 6, 7, 7, 3, 5, 5, 5]
LOOKALIKE_LEN = 10241


def enc_lookalike(lits):
    """A non-final dynamic block of 8-bit literals under the one literal/length code and no distance code."""
    w = TS.BitWriter()
    w.bits(0, 1)
    w.bits(2, 2)
    w.bits(286 - 257, 5)
    w.bits(0, 5)
    w.bits(12 - 4, 4)
    cl = [0] * 19
    for sym, l in zip(P.CLC_ORDER, LOOKALIKE_CL):
        w.bits(l, 3)
        cl[sym] = l
    cc = P.canonical(cl, 7)
    for l in LIT_LENS + [0]:
        w.bits(*cc[l])
    v, n = int.from_bytes(w.getbytes(), "little"), w.n
    assert v >> 8 & 0xFF == 0 and v >> 16 & 0xFFFF == LOOKALIKE_LEN == (v >> 32 & 0xFFFF) ^ 0xFFFF
    v |= int.from_bytes(bytes(lits).translate(REV8), "little") << n
    n += 8 * len(lits)
    return v | LC[256][0] << n, n + EOB_BITS


def _lookalike_case():
    """A dynamic candidate at most 10 bits before stored ones that are no aliases of it: the real dynamic header at
    p and the stored headers its bytes read as at p + 8 .. p + 13 (LEN 10,241; the byte they end on, planted in
    the stored data behind the block, reads as a fixed block's header, so the finder accepts them)."""
    r = random.Random(0xA7)
    b = Build()
    b.stored(filler(r, 30))
    p = b.w.n
    assert p % 8 == 0
    lits = safe_lits(r, 40)
    b.pre("dynamic", *enc_lookalike(lits), lits)
    data_at = ((b.w.n + 3 + 7) >> 3) + 4                    # the next stored block's first data byte
    land = p // 8 + 6 + LOOKALIKE_LEN
    data = bytearray(filler(r, 10600))
    data[land - data_at] = 0xFA                             # BFINAL 0, BTYPE 01
    b.stored(data)
    b.fixed(FINAL_TOKS, final=True)
    return case("A_dynamic_before_stored_lookalikes", "A", b, info={"planted": list(range(p + 8, p + 14)), "dynamic": p})


# ---- family D: decoy headers ---------------------------------------------------------------------------------------------
def dyn_bytes(parts):
    """A non-final dynamic block from bit 0 of a byte, its last byte filled up with ones (what follows it reads as a
    final block of the reserved type)."""
    v, n = enc_dyn(parts)
    pad = -n % 8
    return (v | ((1 << pad) - 1) << n).to_bytes((n + pad) // 8, "little")


def stored_decoy(n):
    """A non-final stored header (byte 0x00: found at bits 0 .. 5) with LEN = n."""
    return b"\x00" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little")


def _decoy_stream(with_error):
    r = random.Random(0xD0)
    b = Build()
    decoys = []                                 # (label, byte offset in the block's data, how its range decode ends)
    at = lambda data: b.w.n + (-(b.w.n + 3) % 8) + 3 + 32 + 8 * len(data)       # the bit of the next data byte

    b.dyn([bytes(range(64))])
    # (a) a stored decoy whose LEN ends exactly on the block's real end: its chain joins the true path
    d = filler(r, 700) + b"\xff"
    decoys.append(("a", at(d), "joins"))
    d += stored_decoy(900) + filler(r, 900)
    b.stored(d)
    # (b) a real dynamic block's bytes: its chain decodes that block and dies on what follows
    d = filler(r, 400) + b"\xff"
    decoys.append(("b", at(d), RESERVED))
    d += dyn_bytes([bytes(r.randrange(225) for _ in range(50))]) + b"\xff" + filler(r, 2200)
    b.stored(d)
    # (c) a decoy whose LEN lands on another decoy, whose LEN ends on the block's real end
    d = filler(r, 300) + b"\xff"
    decoys.append(("c1", at(d), "joins"))
    d += stored_decoy(500) + filler(r, 499) + b"\xff"
    decoys.append(("c2", at(d), "joins"))
    d += stored_decoy(1200) + filler(r, 1200)
    b.stored(d)
    b.dyn([bytes(r.randrange(225) for _ in range(300))])
    err_block = None
    if with_error:
        # (f) the decoys above have lower candidate indices than this real error
        b.dyn([bytes(range(10))])
        err_block = len(b.seams)
        b.dyn([bytes(range(10, 20))])
        b.dyn([bytes(range(20, 30))])
    # (e) decoys inside the final block and in the bytes after it; (d) the one after it is a dynamic block whose
    # tokens run past the end of the input
    d = filler(r, 200) + b"\xff"
    decoys.append(("e_inside", at(d), RESERVED))
    d += dyn_bytes([bytes(r.randrange(225) for _ in range(40))]) + b"\xff" + filler(r, 100)
    b.stored(d, final=True)
    b.raw(filler(r, 64) + b"\xff")
    decoys.append(("d_after", b.w.n, UEOS))
    b.raw(dyn_bytes([bytes(r.randrange(225) for _ in range(400))])[:WIDE_HDR_BITS // 8 + 200])
    info = {"decoys": decoys}
    if not with_error:
        return case("D_decoys", "D", b, info=info)
    comp = reserved_at(b, b.w.getbytes(), err_block)
    info["decoys"] = [(lab, p, RESERVED if how == "joins" else how) for lab, p, how in decoys]
    return _error_case("D_decoys_before_an_error", "D", b, comp, err_block, info)


def _family_d():
    return [_decoy_stream(False), _decoy_stream(True)]


# ---- family B: bucket orders -----------------------------------------------------------------------------------------------
B_UNITS = list(range(1, OB_NB)) + [OB_NB, OB_NB + 6]          # k x 32,768 bits; the last two beyond the clamp
UNIT = 32768


def dyn_of_bits(total, r):
    """The parts of a wide dynamic block of exactly `total` bits: 8-bit literals and up to seven 9-bit ones."""
    rest = total - WIDE_HDR_BITS - EOB_BITS
    nb = rest % 8                                   # 8 a + 9 b = rest: b = rest mod 8
    a = (rest - 9 * nb) // 8
    assert a >= 0
    return [safe_lits(r, a), [("L", 225 + r.randrange(31)) for _ in range(nb)]]


def _count_bucket_stream():
    """Per edge k x 32,768 bits, a chain one bit below and a chain exactly at it (a dynamic block of that many bits,
    the next candidate right behind it), empty stored blocks between them: each is a counted chain of 40 bits and
    five aliases, as many as keep every segment within the cap."""
    r = random.Random(0xB0)
    b = Build()
    want = {}                                       # seam -> bits to the next candidate
    used = collections.Counter()                    # (an upper bound of) the candidates per segment so far
    for k in B_UNITS:
        for total in (k * UNIT - 1, k * UNIT):
            want[b.w.n] = total
            used[b.w.n // (8 * SEG_BYTES)] += 1
            b.dyn(dyn_of_bits(total, r))
            seg = b.w.n // (8 * SEG_BYTES)
            m = min(30, (240 - used[seg]) // 8, (8 * SEG_BYTES * (seg + 1) - b.w.n) // 48 - 1)
            for _ in range(max(1, m)):
                b.stored(b"")
            used[seg] += 8 * max(1, m)
    b.dyn([bytes(range(50))])
    b.fixed(FINAL_TOKS, final=True)
    return case("B_count_buckets", "B", b, info={"want": want})


B_EMIT_SPLIT = [range(1, 13), range(13, 19), range(19, OB_NB + 1)]   # out_count >> 14 edges j x 16,384 per stream
OUT_UNIT = 16384


def run_of_bytes(n, v):
    """The parts of a block that decodes to n bytes v: a literal, (258, 1) copies, literals."""
    assert n >= 1
    k = (n - 1) // 258
    return [bytes([v]), ("RUN", k), bytes([v]) * (n - 1 - 258 * k)]


def _emit_bucket_stream(i, js):
    """Per edge j x 16,384 output bytes, a chain of one byte less and a chain of exactly that many, each a dynamic
    block of under 32,768 bits (runs of (258, 1) copies)."""
    b = Build()
    want = {}                                       # seam -> output bytes of the chain
    v = 0
    for j in js:
        for n in (j * OUT_UNIT - 1, j * OUT_UNIT):
            want[b.w.n] = n
            b.dyn(run_of_bytes(n, SAFE[v % len(SAFE)]))
            v += 1
    if js[-1] == OB_NB:                             # beyond the clamp
        want[b.w.n] = 30 * OUT_UNIT
        b.dyn(run_of_bytes(30 * OUT_UNIT, SAFE[7]))
    b.dyn([bytes(range(50))])
    b.fixed(FINAL_TOKS, final=True)
    return case(f"B_emit_buckets_{i}", "B", b, info={"want_out": want})


def _family_b():
    return [_count_bucket_stream()] + [_emit_bucket_stream(i, js) for i, js in enumerate(B_EMIT_SPLIT)]


# ---- family O: over the cap ------------------------------------------------------------------------------------------------
def _family_o():
    """300-byte stored blocks over 200 KiB: well over 256 accepted headers in each of three segments.  True boundaries
    are dropped and chains run through them."""
    r = random.Random(0x0F)
    b = Build()
    b.dyn([bytes(range(100))])
    for _ in range(680):
        b.stored(filler(r, 300))
    b.dyn([bytes(range(100, 200)), [("M", 40, 350)]])
    b.fixed(FINAL_TOKS, final=True)
    return [case("O_stored_300", "O", b)]


_BUILDERS = {"L": _family_l, "B": _family_b, "A": _family_a, "D": _family_d, "E": _family_e, "R": _family_r,
             "O": _family_o}
COUNTS = {"L": 24, "B": 4, "A": 7, "D": 2, "E": 26, "R": 23, "O": 1}
FAMILIES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def cases(name):
    return _BUILDERS[name]()
