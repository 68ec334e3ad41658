"""Inputs for the LZ77 match search whose greedy parse is known from how they were built.

The parse-driven search of lz77_kernels.hip has limits that random and text inputs reach rarely or
never: the 32 KiB window and the carried history, the run cap and the chunk end, the 13-bit trigram
buckets of lzp_search (64 candidates per step, the nearest-distances shortcut of long buckets), the
8 KiB tiles with their 512-position wave segments and 256-position lead-in, the encode kernel's walk
segments and 64-step windows, and the fallback search for positions no wave reached.  The builders
below put one match at a chosen place relative to one of those limits:

    filler(n, seed, seen)          random bytes in which no 3-byte window occurs twice: nothing in
                                   filler can match, because min_run >= 3
    plant(buf, dst, dist, run)     a copy of run bytes from dst - dist to dst, fenced so that it neither
                                   starts early nor runs on, the seams' trigrams still unique
    crowd(buf, at, trigram, k, s)  k occurrences of one trigram, each followed by distinct bytes: a long
                                   hash bucket whose members have runs of 3 or 4 only
    lzp_hash(trigram)              the kernel's bucket of a trigram, restated
    match_tokens(comp, data)       [(position, run, distance)] of a stream's match tokens

    cases(family) -> the Case(name, data, params, chunk_len, hist_limit, planted, exact) of family
                     "A".."F", seeded, cached.  planted: the match tokens the design requires, sorted;
                     exact: they are all the match tokens of the stream (every case without a crowd).
                     A construction that must NOT be found is expressed by its absence under exact.

Every builder asserts its own position arithmetic while it builds; tests/test_lz_geometry_cpu.py checks
every case against the CPU oracle (planted is contained in, or equals, the oracle's match tokens) and
pins the number of cases per family.  Test infrastructure only (a helper module, not a conftest).
"""
import collections
import functools
import random

import adversarial_hist as A

# ---- the geometry of lz77_kernels.hip, each stated once ---------------------------------------------
TILE = 8192          # LZP_TILE: positions per workgroup of the parse-driven search
WSEG = 512           # LZP_SEG: positions per wave of a tile
LEAD = 256           # LZP_LEAD: the first wave's lead-in before a tile inside a chunk
WIN = 32768          # LZ_WIN: the window before a tile; the largest distance
NEAR_BUCKET = 128    # LZP_NEAR: buckets longer than this test the nearest distances first
NEAR_DIST = 64       # the distances that shortcut tests (one per lane)
LANES = 64           # steps per LDS read of the encode kernel's walk; candidates per search step

FULL = (True, 3, 258, 1, 32768)
FAMILIES = "ABCDEF"

Case = collections.namedtuple("Case", "name data params chunk_len hist_limit planted exact")


class PlantError(AssertionError):
    """A copy could not be fenced where it was put; the case builder tries its next seed."""


def lzp_hash(trigram):
    """lz77_kernels.hip's lzp_hash, restated: the 13 high bits of the 24-bit prefix (little-endian) times
    2654435761 mod 2^32.  A change of the kernel's hash only makes the bucket cases weaker ones."""
    k = trigram[0] | trigram[1] << 8 | trigram[2] << 16
    return ((k * 2654435761) & 0xFFFFFFFF) >> 19


def filler(n, seed, seen, avoid=frozenset()):
    """n greedy random bytes in which no 3-byte window occurs twice, nor one that is in `seen` (shared by
    the pieces of one buffer; updated).  avoid: buckets of lzp_hash that no window may fall into."""
    rng = random.Random(seed)
    out = bytearray()
    pool, at = b"", 0
    while len(out) < n:
        if at == len(pool):
            pool, at = rng.randbytes(2 * n + 64), 0
        c = pool[at]
        at += 1
        if len(out) >= 2:
            t = (out[-2], out[-1], c)
            if t in seen or (avoid and lzp_hash(t) in avoid):
                continue
            seen.add(t)
        out.append(c)
    return bytes(out)


def _first(buf, i):
    """The trigram at i does not occur before i."""
    return buf.find(bytes(buf[i:i + 3])) == i


def _once(buf, i):
    return _first(buf, i) and buf.find(bytes(buf[i:i + 3]), i + 1) == -1


def plant(buf, dst, dist, run, others=(), locked=()):
    """Copies run bytes from dst - dist to dst (the copy may overlap its source).  The byte before the
    copy then differs from the byte before the source, and the byte after it from the byte after the
    source (`others`: further positions that hold the same bytes and get the same fences), so the match
    neither starts early nor runs on; and the trigrams across both seams occur nowhere else, so nothing
    but the planted copy can match there.  Where that fails, the filler byte before or after the copy is
    drawn again (never one inside a `locked` (begin, end) range or inside the source) and the copy and the
    checks are repeated; PlantError if the bytes that would have to change are not free."""
    src, n = dst - dist, len(buf)
    assert 0 <= src < dst and dst + run <= n and run >= 1
    rng = random.Random(dst * 65599 + dist * 31 + run)
    srcs = (src,) + tuple(others)
    overlap = dist <= run                        # the bytes from the source on repeat with period dist

    def free(i):
        return 0 <= i < n and not (src <= i < src + run) and not any(a <= i < b for a, b in locked)

    moved_lo = moved_hi = False
    for _ in range(200):
        for k in range(run):
            buf[dst + k] = buf[src + k]
        lo_bad = dst >= 1 and any(s >= 1 and buf[s - 1] == buf[dst - 1] for s in srcs)
        hi_bad = dst + run < n and any(buf[s + run] == buf[dst + run] for s in srcs)
        for i in ([dst - 3] if moved_lo else []) + [dst - 2, dst - 1]:
            if i >= 0 and not (_first(buf, i) if overlap and i >= src else _once(buf, i)):
                lo_bad = True
        for i in [dst + run - 2, dst + run - 1] + ([dst + run] if moved_hi else []):
            if i >= dst and i + 3 <= n and not _once(buf, i):
                hi_bad = True
        if not lo_bad and not hi_bad:
            return
        if lo_bad:
            if not free(dst - 1):
                raise PlantError(("before", dst, dist, run))
            buf[dst - 1] = rng.randrange(256)
            moved_lo = True
        if hi_bad:
            if not free(dst + run):
                raise PlantError(("after", dst, dist, run))
            buf[dst + run] = rng.randrange(256)
            moved_hi = True
    raise PlantError(("tries", dst, dist, run))


def crowd(buf, at, trigram, k, stride, skip=()):
    """k occurrences of `trigram` at at, at + stride, ..., each followed by two bytes that differ from
    entry to entry (for k <= 250: both of them) and are not in `skip`, so two entries, or an entry and a
    source whose fourth byte is in skip, share a run of 3, at most 4.  Returns the range written."""
    assert stride >= 5 and at + k * stride <= len(buf)
    vals = [v for v in range(256) if v not in skip and v not in trigram]
    m = len(vals)
    for i in range(k):
        p = at + i * stride
        buf[p:p + 3] = trigram
        buf[p + 3] = vals[i % m]
        buf[p + 4] = vals[(i + 50 + i // m) % m]
    return at, at + (k - 1) * stride + 5


def match_tokens(comp, data):
    """[(position, run, distance)] of the match tokens of a raw DEFLATE stream of `data`."""
    blocks = A.walk_blocks(comp)
    assert A.replay(blocks) == data
    pos, out = 0, []
    for b in blocks:
        if b["btype"] == 0:
            pos += len(b["stored"])
            continue
        for t in b["tokens"]:
            if isinstance(t, int):
                pos += 1
            else:
                out.append((pos, t[0], t[1]))
                pos += t[0]
    assert pos == len(data)
    return out


def copy_tokens(dst, dist, run, params=FULL, chunk_len=65536, hist_limit=32768):
    """The match tokens of the greedy parse inside a fenced copy whose only source lies dist before it:
    at most max_run and up to the chunk end at a time; fewer than min_run bytes are literals; a position
    whose source lies before the chunk's history or outside min_dist..max_dist is a literal, and the copy
    goes on behind it.  (Not for an overlapping copy with dist < min_dist: its farther periods match.)"""
    _, min_run, max_run, min_dist, max_dist = params
    out, p, end = [], dst, dst + run
    while p < end:
        cs = p // chunk_len * chunk_len
        r = min(end - p, max_run, cs + chunk_len - p)
        if min_dist <= dist <= max_dist and p - dist >= cs - min(hist_limit, cs) and r >= min_run:
            out.append((p, r, dist))
            p += r
        else:
            p += 1
    return out


def bucket_size(data, q, trigram=None):
    """Entries of the bucket that lzp_search tests at position q of a single call with one 64 KiB chunk per
    tile row: the window's positions (LEAD + WIN before q's tile up to the tile's end) that hash like q's
    trigram, q itself included."""
    h = lzp_hash(trigram or data[q:q + 3])
    p0 = q // TILE * TILE
    return sum(1 for r in range(max(0, p0 - LEAD - WIN), min(p0 + TILE, len(data) - 2)) if lzp_hash(data[r:r + 3]) == h)


def call_starts(n, chunk_len, batch_bytes, piece):
    """Where DeflaterOutputStream(chunk_len, ..., batch_bytes) starts its GPU calls when n bytes are written
    `piece` at a time (streams.py: a call once more than max(batch_bytes, chunk_len + 1) bytes are pending,
    of all whole chunks but the last)."""
    batch = max(batch_bytes, chunk_len + 1)
    starts, done, pending = [0], 0, 0
    for off in range(0, n, piece):
        pending += min(piece, n - off)
        if pending > batch:
            take = (pending - 1) // chunk_len * chunk_len
            if take:
                done += take
                pending -= take
                starts.append(done)
    return starts


# ---- a buffer under construction --------------------------------------------------------------------
class _Buf:
    def __init__(self, n, seed, params=FULL, chunk_len=65536, hist_limit=32768, avoid=frozenset()):
        self.seen = set()
        self.buf = bytearray(filler(n, seed, self.seen, avoid))
        self.cfg = (params, chunk_len, hist_limit)
        self.locked = []
        self.planted = []

    def lock(self, a, b):
        self.locked.append((a - 1, b + 1))

    def copy(self, dst, dist, run, tokens=None, others=()):
        """plant + the tokens the copy gives (copy_tokens, or `tokens` stated by the caller)."""
        plant(self.buf, dst, dist, run, others, self.locked)
        self.lock(dst, dst + run)
        self.lock(dst - dist, dst - dist + run)
        for s in others:
            self.lock(s, s + run)
        self.planted += copy_tokens(dst, dist, run, *self.cfg) if tokens is None else tokens

    def case(self, name, exact=True, n=None):
        data = bytes(self.buf if n is None else self.buf[:n])
        return Case(name, data, *self.cfg, sorted(self.planted), exact)


def _seeded(fn, *args):
    """fn(seed, *args) for the first seed at which every copy could be fenced."""
    for seed in range(1, 40):
        try:
            return fn(seed * 7919, *args)
        except PlantError:
            continue
    raise AssertionError(("no seed fences every copy", fn.__name__, args))


# ---- A. window limits ---------------------------------------------------------------------------------
A_DESTS = [5 * TILE - 1, 6 * TILE, 7 * TILE + 1, 8 * TILE + 3 * WSEG, 9 * TILE + 4 * WSEG - 1]


def _a_window(seed, dist, params=FULL):
    """A 20-byte copy at distance `dist` to the last, the first and the second position of a tile and to
    the first and the last position of a wave segment inside one."""
    assert [q % TILE for q in A_DESTS[:3]] == [TILE - 1, 0, 1]
    assert [q % WSEG for q in A_DESTS[3:]] == [0, WSEG - 1] and all(q % TILE not in (0, 1, TILE - 1) for q in A_DESTS[3:])
    b = _Buf(A_DESTS[-1] + 300, seed, params)
    for q in A_DESTS:
        assert q - dist >= 0
        b.copy(q, dist, 20)
    return b


def _a_only_far(seed):
    """min_dist = max_dist = 32768: of copies at 100, 32767 and 32768 only the last is found."""
    params = (True, 3, 258, 32768, 32768)
    b = _Buf(6 * TILE + 400, seed, params)
    b.copy(5 * TILE - 1, 32767, 20)
    b.copy(5 * TILE + 3 * WSEG, 32768, 20)
    b.copy(5 * TILE + 5 * WSEG, 100, 20)
    assert b.planted == [(5 * TILE + 3 * WSEG, 20, 32768)]
    return b


def _a_max_dist(seed):
    b = _Buf(3000, seed, (True, 3, 258, 1, 300))
    b.copy(1000, 300, 30)
    b.copy(2000, 301, 30)
    assert b.planted == [(1000, 30, 300)]
    return b


def _a_min_dist(seed, min_dist):
    """A source at min_dist - 1 only: an overlapping copy, so the bytes repeat with that period and the
    nearest allowed source is two periods back, from the copy's second period on; then a copy at min_dist."""
    params = (True, 3, 258, min_dist, 32768)
    b = _Buf(2000, seed, params)
    d = min_dist - 1
    # position 500 + k has its source d * 2 back once that lies in the periodic region [500 - d, 540)
    b.copy(500, d, 40, tokens=[(500 + d, 40 - d, 2 * d)])
    b.copy(1000, min_dist, 40)
    assert b.planted[1] == (1000, 40, min_dist)
    return b


def _a_hist(seed, h):
    """chunk_len 4096, hist_limit h.  For offsets j of a later chunk: a source at chunk_start - h is found
    at distance j + h (for h = 0 and j > 0: a source at the chunk's start); one a byte earlier is found
    from the copy's second byte on; a source inside the chunk is always found."""
    c = 4096
    b = _Buf(13 * c, seed, FULL, c, h)
    k = 5                                                  # chunks 5.. have 20000 bytes before them
    assert k * c > 20000
    for j in (0, 1, 100):
        cs = k * c
        if h + j:
            b.copy(cs + j, j + h, 20)
            assert b.planted[-1] == (cs + j, 20, j + h)
        k += 1
        cs = k * c
        n0 = len(b.planted)
        b.copy(cs + j, j + h + 1, 20)
        assert b.planted[n0:] == [(cs + j + 1, 19, j + h + 1)], (h, j, b.planted[n0:])
        k += 1
    cs = k * c
    b.copy(cs + 300, 250, 20)
    assert b.planted[-1] == (cs + 300, 20, 250) and (k + 1) * c <= len(b.buf)
    return b


PIECE = 1000          # bytes per write of the across-calls streams (call_starts)


def _a_call_edge(seed, chunk_len, offset):
    """Copies at distance exactly 32768 to offset 0 or 1 of the second GPU call of a stream written PIECE
    bytes at a time with batch_bytes 40000 and 65536 (call_starts): the source is the first or second byte
    of the history carried over from the call before.  One more at 32767, and one at 32769 (not found)."""
    n = 65536 + 3000
    starts = {call_starts(n, chunk_len, batch, PIECE)[1] for batch in (40000, 65536)}
    assert starts == ({65536} if chunk_len == 65536 else {40960, 65536}), starts
    b = _Buf(n, seed, FULL, chunk_len)
    for s in sorted(starts):
        b.copy(s + offset, 32768, 20)
        assert b.planted[-1] == (s + offset, 20, 32768) and (s + offset) % chunk_len == offset
        b.copy(s + 1000, 32767, 20)
        b.copy(s + 2000, 32769, 20)
    assert len(b.planted) == 2 * len(starts)
    return b


def _family_a():
    out = [_seeded(_a_window, d).case(f"window_{d}") for d in (32767, 32768, 32769)]
    assert out[2].planted == [] and len(out[0].planted) == len(out[1].planted) == 5
    out.append(_seeded(_a_max_dist).case("max_dist_300"))
    out += [_seeded(_a_min_dist, m).case(f"min_dist_{m}") for m in (2, 3)]
    out.append(_seeded(_a_only_far).case("only_32768"))
    out += [_seeded(_a_hist, h).case(f"hist_{h}") for h in (0, 1, 300, 20000)]
    out += [_seeded(_a_call_edge, c, o).case(f"call_offset{o}_chunk{c}") for c in (65536, 4096) for o in (0, 1)]
    return out


# ---- B. run limits ------------------------------------------------------------------------------------
def _b_runs(seed):
    b = _Buf(9000, seed)
    at = 3000
    for k, run in enumerate((3, 4, 257, 258, 259, 516, 600)):
        b.copy(at, 2500 + 7 * k, run)
        at += run + 40
    assert [t[1] for t in b.planted] == [3, 4, 257, 258, 258, 258, 258, 258, 258, 84] and at < 9000
    return b


def _b_overlap(seed, d):
    """Overlapping copies at distance d: runs 258, 259 and 600 of period d."""
    b = _Buf(3000, seed)
    at = 300
    for run in (258, 259, 600):
        b.copy(at, d, run)
        at += run + 100
    assert [t[1] for t in b.planted] == [258, 258, 258, 258, 84] and {t[2] for t in b.planted} == {d}
    return b


def _b_max_run(seed):
    b = _Buf(2000, seed, (True, 3, 100, 1, 32768))
    b.copy(1000, 700, 150)
    assert b.planted == [(1000, 100, 700), (1100, 50, 700)]
    return b


def _b_min_run(seed):
    b = _Buf(2000, seed, (True, 4, 258, 1, 32768))
    b.copy(1000, 700, 3)
    b.copy(1200, 700, 4)
    assert b.planted == [(1200, 4, 700)]
    return b


def _b_chunk_cut(seed, h):
    """100-byte copies that the end of a 4096-byte chunk cuts with 1, 2, 3 and 40 bytes left: fewer than
    min_run are literals, and the copy resumes in the next chunk where the history reaches its source."""
    c = 4096
    b = _Buf(6 * c, seed, FULL, c, h)
    for k, left in enumerate((1, 2, 3, 40)):
        e = (k + 1) * c
        n0 = len(b.planted)
        b.copy(e - left, 600, 100)
        want = [(e - left, left, 600)] if left >= 3 else []
        assert b.planted[n0:] == want + ([(e, 100 - left, 600)] if h >= 600 else []), (h, left)
    return b


def _b_tile_cross(seed):
    """A 258-byte copy across position 8192 inside one chunk is not cut; neither is one whose source crosses it."""
    b = _Buf(TILE + 2000, seed)
    b.copy(TILE - 100, 5000, 258)
    b.copy(TILE + 800, 800 + 100, 258)
    assert b.planted == [(TILE - 100, 258, 5000), (TILE + 800, 258, 900)]
    return b


def _b_chunk_end(seed, tail):
    """A 258-byte copy that ends exactly at position 65536 of a 64 KiB chunk (tail: bytes after it)."""
    b = _Buf(65536 + tail, seed)
    b.copy(65536 - 258, 30000, 258)
    b.copy(65536 - 1000, 9, 300)                            # a capped overlapping one before it
    assert (65536 - 258, 258, 30000) in b.planted
    return b


B_CALLS = (40960, 65536)       # where the second call of the streams below starts with batch_bytes 40000 / 65536


def _b_calls(seed, kind):
    """The run limits against carried history: 68536 bytes in 4096-byte chunks, written PIECE bytes at a time,
    so the second GPU call starts at B_CALLS[0] or B_CALLS[1] (call_starts).  Behind each of the two starts,
    with every source before it: "runs": an overlapping copy at distance 1 (= min_dist) that straddles the start (the
    chunk end cuts it there, and it resumes at the call's first byte for the full 258), a 258-byte copy and
    a 600-byte one (258 + 258 + 84); "chunk_cut": a 100-byte copy cut with 40 bytes left that resumes at
    the call's first byte; "max_run_100": a 150-byte copy under max_run 100."""
    c, n = 4096, 65536 + 3000
    assert tuple(call_starts(n, c, batch, PIECE)[1] for batch in (40000, 65536)) == B_CALLS
    b = _Buf(n, seed, (True, 3, 100, 1, 32768) if kind == "max_run_100" else FULL, c)
    for s in B_CALLS:
        assert s % c == 0
        n0 = len(b.planted)
        if kind == "runs":
            b.copy(s - 100, 1, 400)
            assert b.planted[n0:] == [(s - 100, 100, 1), (s, 258, 1), (s + 258, 42, 1)]
            b.copy(s + 600, 2000, 258)
            b.copy(s + 1000, 3500, 600)
            assert [t[1] for t in b.planted[n0 + 3:]] == [258, 258, 258, 84]
            want = 5
        elif kind == "chunk_cut":
            b.copy(s - 40, 600, 100)
            assert b.planted[n0:] == [(s - 40, 40, 600), (s, 60, 600)]
            want = 1
        else:
            b.copy(s + 300, 2000, 150)
            assert b.planted[n0:] == [(s + 300, 100, 2000), (s + 400, 50, 2000)]
            want = 2
        # destinations in the second call, sources in the first
        assert sum(1 for q, r, d in b.planted[n0:] if q >= s > q - d) == want, (kind, s)
    return b


def carried(case, batch_bytes):
    """The planted tokens of a case whose destination lies in a later GPU call than the first byte of their
    source, when the case is streamed PIECE bytes at a time with this batch_bytes."""
    starts = call_starts(len(case.data), case.chunk_len, batch_bytes, PIECE)[1:]
    return [(q, r, d) for q, r, d in case.planted if any(q >= s > q - d for s in starts)]


# planted tokens with a carried source, summed over a family, per batch_bytes (pinned by the CPU test)
CARRIED = {"A": {40000: 19, 65536: 12}, "B": {40000: 8, 65536: 8}}


def _family_b():
    out = [_seeded(_b_runs).case("runs")]
    out += [_seeded(_b_overlap, d).case(f"overlap_{d}") for d in (1, 2, 3)]
    out += [_seeded(_b_max_run).case("max_run_100"), _seeded(_b_min_run).case("min_run_4")]
    out += [_seeded(_b_chunk_cut, h).case(f"chunk_cut_hist{h}") for h in (32768, 0)]
    out.append(_seeded(_b_tile_cross).case("tile_cross"))
    out += [_seeded(_b_chunk_end, t).case(f"ends_at_65536_tail{t}") for t in (0, 1000)]
    out += [_seeded(_b_calls, k).case(f"calls_{k}") for k in ("runs", "chunk_cut", "max_run_100")]
    return out


# ---- C. ties and crowded buckets ------------------------------------------------------------------------
def _c_tie(seed):
    """Two sources with equal runs: the nearer one wins."""
    b = _Buf(4000, seed)
    b.copy(1500, 1000, 30)                                  # the second source, itself a copy of the first
    b.copy(3000, 1500, 30, others=(500,))
    assert b.planted == [(1500, 30, 1000), (3000, 30, 1500)]
    return b


def _c_longer(seed):
    """A farther source that is longer by exactly 1: the farther one wins."""
    b = _Buf(4000, seed)
    b.copy(1500, 1000, 30)
    b.copy(3000, 2500, 31)
    assert b.buf[1530] != b.buf[530] == b.buf[3030]
    assert b.planted == [(1500, 30, 1000), (3000, 31, 2500)]
    return b


def colliding_trigrams(count=3):
    """Printable trigrams with distinct first bytes in one bucket of lzp_hash."""
    first = b"lzp"
    out = [first]
    for x in range(0x20, 0x7F):
        for y in range(0x20, 0x7F):
            for z in range(0x20, 0x7F):
                t = bytes((x, y, z))
                if all(t[0] != o[0] for o in out) and lzp_hash(t) == lzp_hash(first):
                    out.append(t)
                    if len(out) == count:
                        return out
                    break
            else:
                continue
            break
    raise AssertionError("no colliding trigrams among the printable ones")


def _c_bucket(seed, k, source_first):
    """A bucket of exactly k entries at the destination: the source, k - 2 crowd entries of the same
    trigram with runs of 3, and the destination itself.  The 40-byte source lies before the crowd (the
    farthest entry) or behind it (the nearest)."""
    t = b"lzp"
    h = lzp_hash(t)
    b = _Buf(2600, seed, avoid={h})
    s = 100 if source_first else 300 + 5 * (k - 2) + 60
    dst = 300 + 5 * (k - 2) + 200
    b.buf[s:s + 3] = t
    b.lock(*crowd(b.buf, 300, t, k - 2, 5, skip=(b.buf[s + 3],)))
    b.copy(dst, dst - s, 40)
    data = bytes(b.buf)
    if bucket_size(data, dst) != k or data[dst:dst + 3] != t:
        raise PlantError(("bucket", k, bucket_size(data, dst)))
    assert b.planted == [(dst, 40, dst - s)]
    return b


def _c_three_trigrams(seed):
    """One bucket shared by three distinct trigrams: 70 entries of each of the two others between the
    source and the destination."""
    t1, t2, t3 = colliding_trigrams()
    assert len({t1, t2, t3}) == 3 and lzp_hash(t1) == lzp_hash(t2) == lzp_hash(t3)
    b = _Buf(2600, seed, avoid={lzp_hash(t1)})
    b.buf[100:103] = t1
    b.lock(*crowd(b.buf, 300, t2, 70, 5))
    b.lock(*crowd(b.buf, 700, t3, 70, 5))
    b.copy(1500, 1400, 40)
    data = bytes(b.buf)
    if bucket_size(data, 1500) != 142:
        raise PlantError("bucket")
    return b


def _c_far_cap(seed):
    """A cap-length source only beyond 200 crowded nearer candidates with runs of 3, the nearest of them
    within the 64 distances the shortcut tests: the far one wins."""
    t = b"lzp"
    b = _Buf(3000, seed, avoid={lzp_hash(t)})
    b.buf[100:103] = t
    lo, hi = crowd(b.buf, 500, t, 200, 5, skip=(b.buf[103],))
    b.lock(lo, hi)
    dst = hi + 3
    assert dst - (hi - 5) <= NEAR_DIST and bucket_size(bytes(b.buf), 100) > NEAR_BUCKET
    b.copy(dst, dst - 100, 258)
    assert b.planted == [(dst, 258, dst - 100)]
    return b


def _c_near_and_far_cap(seed):
    """Cap-length sources within the 64 nearest distances and far: a 40-periodic stretch of 516 bytes far
    back, 200 crowd entries, then the same stretch again.  Its first 258 bytes can only come from far
    back (the nearest phase that still has 258 bytes: 240 into the far stretch); the second 258 have
    sources 40 back and far back, and the nearest wins."""
    b = _Buf(4000, seed)
    f, r, d = 100, 2200, 40
    b.copy(f + d, d, 516 - d)                               # the far stretch [f, f + 516)
    t = bytes(b.buf[f + 258 % d:f + 258 % d + 3])           # the trigram at the second token's start
    b.lock(*crowd(b.buf, 800, t, 200, 5, skip=(b.buf[f + 258 % d + 3],)))
    b.planted = copy_tokens(f + d, d, 516 - d)
    plant(b.buf, r, r - f, 516, locked=b.locked)
    b.lock(r, r + 516)
    assert bucket_size(bytes(b.buf), r + 258) > NEAR_BUCKET and d <= NEAR_DIST
    b.planted += [(r, 258, r - f - 240), (r + 258, 258, d)]
    return b


def _c_chunk_end_caps(seed, near_run):
    """The end of a 4096-byte chunk lies 20 bytes behind the destination, in a bucket long enough for the
    nearest-distances shortcut.  near_run 30: it caps a run of 30 from 50 back and a run of 258 from far
    back to the same 20, and the near one wins.  near_run 19: the near run is one short of the capped far
    one, so the shortcut must not take it, and the far one wins.  The far one goes on in the next chunk."""
    c = 4096
    t = b"lzp"
    b = _Buf(c + 1000, seed, FULL, c, 32768, avoid={lzp_hash(t)})
    f, q = 100, c - 20
    b.buf[f:f + 3] = t
    b.lock(*crowd(b.buf, 1000, t, 200, 5, skip=(b.buf[f + 3],)))
    b.copy(q - 50, q - 50 - f, near_run)
    first = (q, 20, 50) if near_run >= 20 else (q, 20, q - f)
    b.copy(q, q - f, 258, tokens=[first, (c, 238, q - f)], others=(q - 50,) if near_run >= 20 else ())
    assert 50 <= NEAR_DIST and bucket_size(bytes(b.buf), q) > NEAR_BUCKET and q + 20 == c
    return b


C_BUCKETS = (63, 64, 65, 127, 128, 129, 192, 193)


def _family_c():
    out = [_seeded(_c_tie).case("tie_nearer_wins"), _seeded(_c_longer).case("farther_longer_by_1")]
    for k in C_BUCKETS:
        for first in (True, False):
            out.append(_seeded(_c_bucket, k, first).case(f"bucket_{k}_source_{'first' if first else 'last'}", exact=False))
    out.append(_seeded(_c_three_trigrams).case("three_trigrams_one_bucket", exact=False))
    out.append(_seeded(_c_far_cap).case("cap_source_behind_200", exact=False))
    out.append(_seeded(_c_near_and_far_cap).case("cap_sources_near_and_far", exact=False))
    out.append(_seeded(_c_chunk_end_caps, 30).case("chunk_end_caps_near_and_far", exact=False))
    out.append(_seeded(_c_chunk_end_caps, 19).case("chunk_end_near_one_short_of_cap", exact=False))
    return out


# ---- D. tile and wave-segment geometry --------------------------------------------------------------------
D_BOUNDS = (WSEG, 3 * WSEG, TILE - LEAD, TILE, TILE + WSEG, 2 * TILE)
D_CHUNKS = (512, 777, 1000, 4096, 4097, 8192)


def _d_starts(seed, delta, chunk_len):
    """A 20-byte copy starting delta off each boundary."""
    b = _Buf(2 * TILE + 300, seed, FULL, chunk_len)
    for i, bd in enumerate(D_BOUNDS):
        src = 30 + 40 * i
        b.copy(bd + delta, bd + delta - src, 20)
    if chunk_len == 65536:
        assert [t[0] for t in b.planted] == [bd + delta for bd in D_BOUNDS]
    return b


def _d_span_copies(seed, chunk_len):
    """A 100-byte copy across each boundary, 50 bytes on either side."""
    b = _Buf(2 * TILE + 300, seed, FULL, chunk_len)
    for i, bd in enumerate(D_BOUNDS):
        src = 100 if i == 0 else 600 + 110 * i             # sources of their own, clear of every copy
        b.copy(bd - 50, bd - 50 - src, 100)
    return b


def _d_span_sources(seed, chunk_len):
    """A 100-byte source across each boundary, copied behind the last one."""
    b = _Buf(2 * TILE + 1600, seed, FULL, chunk_len)
    for i, bd in enumerate(D_BOUNDS):
        dst = 2 * TILE + 100 + 200 * i
        b.copy(dst, dst - (bd - 50), 100)
    return b


def _d_length(seed, n):
    """A buffer of n bytes that ends with a 30-byte copy, and a copy at its first tile's end."""
    b = _Buf(n, seed)
    b.copy(n - 30, 3000, 30)
    b.copy(TILE - 300, 2000, 30)
    assert b.planted[0] == (n - 30, 30, 3000) and len(b.buf) == n
    return b


def _d_pass_over(seed, chunk_len):
    """TILE + WSEG + 100 bytes that end with a 258-byte copy: it starts in the tile's second segment and
    covers the whole last, 100-position one, so the true path passes over a segment."""
    n = TILE + WSEG + 100
    b = _Buf(n, seed, FULL, chunk_len)
    dst = n - 258
    assert TILE < dst < TILE + WSEG and dst + 258 == n
    b.copy(dst, 4000, 258)
    return b


def _d_off_lead(seed):
    """A 1000-byte copy from 6 positions before the lead-in's start: the true path enters the tile at
    TILE - 4 and visits TILE + 254, the lead path (from TILE - 256: 258 more) TILE + 2 and TILE + 260."""
    b = _Buf(2 * TILE, seed)
    dst = TILE - LEAD - 6
    b.copy(dst, 5000, 1000)
    assert [t[0] for t in b.planted] == [dst, dst + 258, dst + 516, dst + 774] and dst + 516 == TILE + 254
    return b


def _family_d():
    out = [_seeded(_d_starts, d, 65536).case(f"starts_{d:+d}") for d in (-1, 0, 1)]
    out += [_seeded(_d_span_copies, 65536).case("span_copies"), _seeded(_d_span_sources, 65536).case("span_sources")]
    out += [_seeded(_d_length, n).case(f"length_{n}") for n in (TILE - 1, TILE, TILE + 1, TILE + WSEG - 1, TILE + WSEG + 1)]
    out += [_seeded(_d_pass_over, 65536).case("pass_over_last_segment"), _seeded(_d_off_lead).case("off_lead")]
    for c in D_CHUNKS:
        out += [_seeded(_d_starts, d, c).case(f"starts_{d:+d}_chunk{c}") for d in (-1, 0, 1)]
        out += [_seeded(_d_span_copies, c).case(f"span_copies_chunk{c}"),
                _seeded(_d_span_sources, c).case(f"span_sources_chunk{c}"), _seeded(_d_pass_over, c).case(f"pass_over_chunk{c}")]
    return out


# ---- E. parses that do not merge ----------------------------------------------------------------------------
E_PERIODS = (1, 2, 3, 7, 255, 256, 257, 258, 259, 512, 8191, 8192, 8193)
E_LEN = 3 * TILE + 100


def _e_period(p, chunk_len):
    """filler(p) repeated: every position from p on has a source p back that reaches the cap (or the chunk
    end), so parses started at different positions keep their offset for ever."""
    for seed in range(1, 40):
        seen = set()
        unit = filler(p, 1000 * p + seed, seen)
        wrap = (unit + unit)[p - 2:p + 2] if p >= 3 else b""
        if all(tuple(wrap[i:i + 3]) not in seen for i in range(len(wrap) - 2)):
            break
    else:
        raise AssertionError(("no period", p))
    data = (unit * (E_LEN // p + 1))[:E_LEN]
    planted, q = [], p
    while q < E_LEN:
        r = min(258, q // chunk_len * chunk_len + chunk_len - q, E_LEN - q)
        if r >= 3:
            planted.append((q, r, p))
            q += r
        else:
            q += 1
    return Case(f"period_{p}_chunk{chunk_len}", data, FULL, chunk_len, 32768, planted, True)


def _family_e():
    return [_e_period(p, c) for c in (65536, 4096) for p in E_PERIODS]


# ---- F. walk windows ----------------------------------------------------------------------------------------
def _f_lanes(seed, chunk_len):
    """Copies whose start within the chunk is 62, 63, 0 and 1 (mod LANES), short ones and ones longer than
    a 64-step window, none cut by a chunk end."""
    b = _Buf(9000, seed, FULL, chunk_len)
    at, got = 3500, []
    for run in (3, 10, 64, 65, 130):
        for res in (62, 63, 0, 1):
            w = next(w for w in range(at, at + 2 * chunk_len)
                     if w % chunk_len % LANES == res and w % chunk_len + run <= chunk_len)
            got.append(w % chunk_len % LANES)
            b.copy(w, w - (100 + 150 * (len(got) - 1)), run)
            at = w + run + 70
    assert got == [62, 63, 0, 1] * 5 and at < 9000 and len(b.planted) == 20
    return b


def _f_back_to_back(seed, runs, start):
    """Copies one right after the other from `start`, each from a source of its own."""
    b = _Buf(6000, seed)
    at, src = start, 100
    for run in runs:
        for _ in range(30):
            try:
                b.copy(at, at - src, run)
                break
            except PlantError:
                src += 1
        else:
            raise PlantError("back to back")
        src += run + 9
        at += run
    if any(b.buf[d + r] == b.buf[d - dist + r] for d, r, dist in b.planted):
        raise PlantError("a later copy moved a fence")
    assert src < start - 300 and [t[1] for t in b.planted] == [r for run in runs for r in [258] * (run // 258) + [run % 258] if r]
    return b


def _family_f():
    out = [_seeded(_f_lanes, c).case(f"lanes_chunk{c}") for c in (65536, 1000)]
    # 64 tokens of 3 bytes back to back: a 64-step window of the walk (64 positions from wherever the window
    # before it ended, not aligned to the chunk) then holds about 22 tokens; only literals fill one with 64.
    # Then copies of a window's size and more: windows of one token each
    out.append(_seeded(_f_back_to_back, (3,) * 64, 3008).case("back_to_back_64x3"))
    out.append(_seeded(_f_back_to_back, (64, 64, 61, 3, 65, 63, 258, 130, 4, 60), 3071).case("back_to_back_window_sized"))
    return out


_GEN = {"A": _family_a, "B": _family_b, "C": _family_c, "D": _family_d, "E": _family_e, "F": _family_f}
COUNTS = {"A": 15, "B": 14, "C": 23, "D": 48, "E": 26, "F": 4}


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family (built once per process; every builder is seeded)."""
    return tuple(_GEN[family]())


def pure_filler(n=3 * TILE, seed=5):
    """Nothing matches: every position is a literal and every parse merges at once."""
    return filler(n, seed, set())
