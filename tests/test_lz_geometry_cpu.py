"""The constructions of tests/lz_geometry.py bite: on the CPU oracle's stream of every case the planted
match tokens are there (and, for a case without a crowd, are all the match tokens there are, so what
must not be found is not), the brute-force search gives the same bytes for the cases small enough for
it, and the geometry each family is about holds for the case's data.  The number of cases per family is
pinned: a builder whose design does not come out fails here, it is not dropped.
"""
import functools

import pytest

import lz_geometry as G
import oracle_lib as O
from lz_geometry import LANES, LEAD, NEAR_BUCKET, NEAR_DIST, TILE, WIN, WSEG

BRUTE_MAX = 20000                  # the exhaustive search takes about 6 s per 100 KB
BRUTE_CASES = {"A": 3, "B": 7, "C": 23, "D": 48, "E": 0, "F": 4}
BRUTE_PERIODS = (1, 258, 8193)     # of family E (24,676 bytes each: about 1.5 s apiece)


@functools.lru_cache(maxsize=None)
def expected(family, i):
    c = G.cases(family)[i]
    return O.deflate_lz(c.data, *c.params, c.chunk_len, c.hist_limit)


def test_case_counts_are_pinned():
    assert G.COUNTS == {"A": 15, "B": 14, "C": 23, "D": 48, "E": 26, "F": 4}
    for f in G.FAMILIES:
        cs = G.cases(f)
        assert len(cs) == G.COUNTS[f], (f, len(cs))
        assert len({c.name for c in cs}) == len(cs)
        assert all(len(c.data) <= 100_000 for c in cs)
        assert all(c.planted == sorted(c.planted) for c in cs)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_planted_tokens_are_the_oracles(family):
    for i, c in enumerate(G.cases(family)):
        toks = G.match_tokens(expected(family, i), c.data)
        if c.exact:
            assert toks == c.planted, (c.name, [t for t in toks if t not in c.planted][:5],
                                       [t for t in c.planted if t not in toks][:5])
        else:
            assert set(c.planted) <= set(toks), (c.name, [t for t in c.planted if t not in toks])
        assert c.planted or c.name == "window_32769", c.name


@pytest.mark.parametrize("family", G.FAMILIES)
def test_brute_force_search_agrees(family):
    n = 0
    for i, c in enumerate(G.cases(family)):
        if len(c.data) <= BRUTE_MAX:
            n += 1
            assert O.deflate_lz(c.data, *c.params, c.chunk_len, c.hist_limit, brute=True) == expected(family, i), c.name
    assert n == BRUTE_CASES[family], (family, n)


@pytest.mark.parametrize("p", BRUTE_PERIODS)
def test_brute_force_search_agrees_on_periods(p):
    """Family E is above BRUTE_MAX; three of its periods get the exhaustive search all the same."""
    i, c = next((i, c) for i, c in enumerate(G.cases("E")) if c.name == f"period_{p}_chunk65536")
    assert O.deflate_lz(c.data, *c.params, c.chunk_len, c.hist_limit, brute=True) == expected("E", i)


def test_lzp_hash_and_filler():
    assert G.lzp_hash(b"\0\0\0") == 0 and G.lzp_hash(b"\x01\0\0") == 2654435761 >> 19
    assert 0 <= G.lzp_hash(b"\xff\xff\xff") < 8192
    t = G.colliding_trigrams()
    assert len({G.lzp_hash(x) for x in t}) == 1 and len({x[0] for x in t}) == 3
    data = G.pure_filler()
    assert len({data[i:i + 3] for i in range(len(data) - 2)}) == len(data) - 2
    assert G.match_tokens(O.deflate_lz(data, *G.FULL), data) == []


def by_name(family):
    return {c.name: c for c in G.cases(family)}


def test_geometry_of_the_window_cases():
    a = by_name("A")
    for d in (WIN - 1, WIN):
        qs = [t[0] for t in a[f"window_{d}"].planted]
        assert [t[2] for t in a[f"window_{d}"].planted] == [d] * 5
        assert [q % TILE for q in qs[:3]] == [TILE - 1, 0, 1] and [q % WSEG for q in qs[3:]] == [0, WSEG - 1]
    c = a[f"window_{WIN + 1}"]                             # the same copies, one byte too far
    for q in G.A_DESTS:
        assert c.data[q:q + 20] == c.data[q - WIN - 1:q - WIN - 1 + 20] and c.planted == []
    assert a["max_dist_300"].planted == [(1000, 30, 300)] and a["max_dist_300"].data[2000:2030] == a["max_dist_300"].data[1699:1729]
    assert [t[2] for t in a["min_dist_2"].planted] == [2, 2] and [t[2] for t in a["min_dist_3"].planted] == [4, 3]
    assert [t[2] for t in a["only_32768"].planted] == [32768]
    for h in (0, 1, 300, 20000):
        c = a[f"hist_{h}"]
        assert (c.chunk_len, c.hist_limit) == (4096, h)
        found = [(q % 4096, d) for q, r, d in c.planted if r == 20]
        assert found == [(j, j + h) for j in (0, 1, 100) if j + h] + [(300, 250)]
        cut = [(q % 4096, d) for q, r, d in c.planted if r == 19]            # one byte before the history
        assert cut == [(j + 1, j + h + 1) for j in (0, 1, 100)]
    for chunk_len, starts in ((65536, [65536]), (4096, [40960, 65536])):
        for off in (0, 1):
            c = a[f"call_offset{off}_chunk{chunk_len}"]
            assert [q for q, r, d in c.planted if d == 32768] == [s + off for s in starts]
            assert [d for q, r, d in c.planted] == [32768, 32767] * len(starts)


def test_geometry_of_the_run_and_bucket_cases():
    b, c = by_name("B"), by_name("C")
    assert [r for _, r, _ in b["runs"].planted] == [3, 4, 257, 258, 258, 258, 258, 258, 258, 84]
    for d in (1, 2, 3):
        assert all(t[2] == d for t in b[f"overlap_{d}"].planted) and max(t[1] for t in b[f"overlap_{d}"].planted) == 258
    assert [r for _, r, _ in b["max_run_100"].planted] == [100, 50] and [r for _, r, _ in b["min_run_4"].planted] == [4]
    cut = b["chunk_cut_hist32768"].planted
    assert [(q % 4096 or 4096, r) for q, r, _ in cut] == [(4096, 99), (4096, 98), (4093, 3), (4096, 97), (4056, 40), (4096, 60)]
    assert [(4096 - q % 4096, r) for q, r, _ in b["chunk_cut_hist0"].planted] == [(3, 3), (40, 40)]
    assert all(q < TILE < q + r or q - d < TILE < q - d + r for q, r, d in b["tile_cross"].planted)
    for t in (0, 1000):
        assert (65536 - 258, 258, 30000) in b[f"ends_at_65536_tail{t}"].planted and len(b[f"ends_at_65536_tail{t}"].data) == 65536 + t
    # the run limits against carried history: destinations in the second call, sources in the first
    for batch, s in zip((40000, 65536), G.B_CALLS):
        for name, want in (("runs", [(s, 258, 1), (s + 600, 258, 2000), (s + 1000, 258, 3500), (s + 1258, 258, 3500),
                                     (s + 1516, 84, 3500)]),
                           ("chunk_cut", [(s, 60, 600)]), ("max_run_100", [(s + 300, 100, 2000), (s + 400, 50, 2000)])):
            case = b[f"calls_{name}"]
            assert G.call_starts(len(case.data), case.chunk_len, batch, G.PIECE)[1] == s and case.chunk_len == 4096
            assert G.carried(case, batch) == want and all(q >= s > q - d for q, r, d in want)
        assert (s - 100, 100, 1) in b["calls_runs"].planted and (s - 40, 40, 600) in b["calls_chunk_cut"].planted
    assert {bb: sum(len(G.carried(c, bb)) for c in G.cases("B")) for bb in (40000, 65536)} == G.CARRIED["B"]
    assert {bb: sum(len(G.carried(c, bb)) for c in G.cases("A")) for bb in (40000, 65536)} == G.CARRIED["A"]
    for k in G.C_BUCKETS:
        for where in ("first", "last"):
            case = c[f"bucket_{k}_source_{where}"]
            (q, r, d), = case.planted
            assert G.bucket_size(case.data, q) == k
            others = [p for p in range(q) if case.data[p:p + 3] == case.data[q:q + 3]]
            assert len(others) == k - 1 and (others[0] if where == "first" else others[-1]) == q - d
    assert {k > NEAR_BUCKET for k in G.C_BUCKETS} == {True, False} and {k % LANES for k in G.C_BUCKETS} >= {63, 0, 1}
    (q, r, d), = c["three_trigrams_one_bucket"].planted
    data = c["three_trigrams_one_bucket"].data
    assert len({data[p:p + 3] for p in range(len(data) - 2) if G.lzp_hash(data[p:p + 3]) == G.lzp_hash(data[q:q + 3])}) == 3
    (q, r, d), = c["cap_source_behind_200"].planted
    data = c["cap_source_behind_200"].data
    nearer = [p for p in range(q - d + 1, q) if data[p:p + 3] == data[q:q + 3]]
    assert r == 258 and len(nearer) == 200 and q - nearer[-1] <= NEAR_DIST and G.bucket_size(data, q) > NEAR_BUCKET
    q, r, d = c["cap_sources_near_and_far"].planted[-1]
    data = c["cap_sources_near_and_far"].data
    far = [p for p in range(q - NEAR_DIST) if data[p:p + 258] == data[q:q + 258]]
    assert (r, d) == (258, 40) and d <= NEAR_DIST and far and G.bucket_size(data, q) > NEAR_BUCKET
    case = c["chunk_end_caps_near_and_far"]
    q, r, d = case.planted[1]
    assert q + r == case.chunk_len and d <= NEAR_DIST and case.planted[2][1:] == (238, case.planted[0][2] + 50)
    assert case.data[q:q + 258] == case.data[100:358] and case.data[q:q + 30] == case.data[q - d:q - d + 30]
    case = c["chunk_end_near_one_short_of_cap"]
    (n0, nr, nd), (q, r, d), _ = case.planted
    assert (nr, q - n0, r) == (19, 50, 20) and q + r == case.chunk_len and d > NEAR_DIST
    assert case.data[q:q + 19] == case.data[n0:n0 + 19] and case.data[q + 19] != case.data[n0 + 19]


def test_geometry_of_the_tile_and_walk_cases():
    d, e, f = by_name("D"), by_name("E"), by_name("F")
    for delta in (-1, 0, 1):
        assert [q for q, _, _ in d[f"starts_{delta:+d}"].planted] == [b + delta for b in G.D_BOUNDS]
    assert set(G.D_BOUNDS) == {TILE, 2 * TILE, WSEG, 3 * WSEG, TILE - LEAD, TILE + WSEG}
    assert [q + 50 for q, r, _ in d["span_copies"].planted] == list(G.D_BOUNDS)
    assert sorted(q - dist + 50 for q, r, dist in d["span_sources"].planted) == list(G.D_BOUNDS)
    for n in (TILE - 1, TILE, TILE + 1, TILE + WSEG - 1, TILE + WSEG + 1):
        assert len(d[f"length_{n}"].data) == n and d[f"length_{n}"].planted[-1][:2] == (n - 30, 30)
    c = d["pass_over_last_segment"]
    (q, r, _), = c.planted
    assert len(c.data) == TILE + WSEG + 100 and q < TILE + WSEG and q + r == len(c.data) and r == 258
    assert [q for q, _, _ in d["off_lead"].planted][:3] == [TILE - LEAD - 6, TILE - 4, TILE + 254]
    for chunk_len in G.D_CHUNKS:
        names = [n for n in d if n.endswith(f"_chunk{chunk_len}")]
        for delta in (-1, 0, 1):                           # the starts are where they were; the chunk ends move
            data = d[f"starts_{delta:+d}_chunk{chunk_len}"].data
            assert all(data[bd + delta:bd + delta + 20] == data[30 + 40 * i:50 + 40 * i] for i, bd in enumerate(G.D_BOUNDS))
        assert len(names) == 6 and all(d[n].chunk_len == chunk_len for n in names)
    for name, c in e.items():
        assert len(c.data) == 3 * TILE + 100
    # period 258: the true path visits the multiples of 258, the lead path of the second tile TILE - LEAD + 258 k
    on_path = {q for q, _, _ in e["period_258_chunk65536"].planted}
    assert TILE - LEAD + 258 not in on_path and 8256 in on_path and 8256 % 258 == 0
    # at 4096 the encode walk's segments are 256 positions: every 258-run passes over one
    assert all(r in (258, 4096 - q % 4096, 3 * TILE + 100 - q) for q, r, _ in e["period_258_chunk4096"].planted)
    for chunk_len in (65536, 1000):
        starts = [q % chunk_len % LANES for q, _, _ in f[f"lanes_chunk{chunk_len}"].planted]
        assert starts == [62, 63, 0, 1] * 5
    toks = f["back_to_back_64x3"].planted
    assert len(toks) == 64 and all(b[0] == a[0] + 3 for a, b in zip(toks, toks[1:])) and toks[0][0] % LANES == 0
    toks = f["back_to_back_window_sized"].planted
    assert all(b[0] == a[0] + a[1] for a, b in zip(toks, toks[1:])) and toks[0][0] % LANES == LANES - 1
