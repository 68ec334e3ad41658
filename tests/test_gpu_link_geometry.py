"""GPU decode of the candidate-list and chain-linking limit cases of tests/link_geometry.py (what each case reaches is
pinned on the CPU by tests/test_link_geometry_cpu.py), through four contexts:

    default      the device-side list and linking (Decode::devlink)
    host_link    NDFL_HOST_LINK=1: the host linker (Decode::hostlink), the second implementation of the stage
    no_alias     NDFL_NO_ALIAS=1: every stored-header alias counted as a chain of its own
    w4           NDFL_COUNT_W=4: the workgroup count kernel, its own chain loop

Device input, device output pre-filled with 0xEE, guard bytes after out_cap.  Every case and context: the return
code, out_len, consumed bits, the bytes and the guard; ndfl_ctx_timings [5] linked chains and [7] header candidates
against the host model (everywhere but in family O, whose kept headers are not pinned), [6] repaired boundaries == 0
on the three device-link contexts; and the four contexts agree.  A case on which include/ndfl.h is silent (a partial
input that ends exactly on a seam) is pinned to the host-link path.  Family R runs plain and with
NDFL_DICT_DEFERRED + ndfl_inflate_resolve.  One capacity pair per family at out_cap = n - 1.  A fifth context,
NDFL_STATS=1, shows that no case's default decode is handed over to the host linker (LINK_FALLBACK).

Measured on an MI355X: 1.6 s for family L on the four contexts, 1.3 s for E, 0.7 s for B, under 0.3 s for every other
test.  Each of these changes to a scratch copy of the library fails a case here: the emit order's placing a tile's
last item on its first (L_2048: a chain's bytes stay 0xEE), one jump level too few (the no-fallback test: the decode
is right, through the host linker), S[0] - S[node] from the other sum buffer (L_2), `<` for `<=` in cand_slice's
first search (L_1: the start header counted twice), a plain store for atomicMin (E_copy_before_four_tiles).  Two
do not and cannot: `<=` for `<` in cand_slice's second search (the finder scans [start_bit, end_bit) only, so the
list holds nothing at or past end_bit) and an alias window of 9 for 10 (headers with one LEN position lie at most 7
bits apart; test_link_geometry_cpu pins that slack).
"""
import collections

import pytest

import knobs
import link_geometry as G

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, 64
WAYS = collections.OrderedDict([("default", {}), ("host_link", {"NDFL_HOST_LINK": 1}), ("no_alias", {"NDFL_NO_ALIAS": 1}),
                                ("w4", {"NDFL_COUNT_W": 4})])
DEVICE_LINK = [w for w in WAYS if w != "host_link"]


@pytest.fixture(scope="module")
def ndfl():
    import torch  # noqa: F401 (before libndfl.so: the device tests share torch's stream)
    import ndfl as N
    return N


@pytest.fixture(scope="module")
def contexts(ndfl):
    return {w: knobs.context(**env) for w, env in WAYS.items()}


Got = collections.namedtuple("Got", "code out_len bits data rest guard chains repairs cands")


def to_dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def decode(ndfl, ctx, c, src, cap, deferred=False):
    """One decode of case c into a fresh buffer [window | cap bytes | guard]: Got.data = out[0, out_len), rest = what
    lies between out_len and out_cap, guard = the bytes after out_cap."""
    import torch
    dl = len(c.window)
    out = torch.full((dl + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    if dl and not deferred:
        out[:dl] = to_dev(c.window)
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
    if c.start_bit == 0 and c.end_bit is None and not c.partial and not dl:
        r, olen, bits = ctx.inflate_raw(src.data_ptr(), len(c.comp), out.data_ptr(), cap, flags)
    else:
        flags |= (ndfl.IN_PARTIAL if c.partial else 0) | (ndfl.DICT_DEFERRED if deferred else 0)
        r, olen, bits = ctx.inflate_range_raw(src.data_ptr(), len(c.comp), c.start_bit, c.end_bit, out.data_ptr(), dl, cap,
                                              flags)
    if deferred and r == 0:
        if dl:
            out[:dl] = to_dev(c.window)         # (the window arrives after the decode)
        ctx.inflate_resolve()
    t = ctx.timings()
    got = out.cpu().numpy().tobytes()
    assert got[:dl] == (c.window if not deferred or r == 0 else bytes([FILL]) * dl), (c.name, "window changed")
    n = min(olen, cap) if r >= 0 else 0
    return Got(r, olen, bits, got[dl:dl + n], got[dl + n:dl + cap], got[dl + cap:], int(t["inflate_chains"]),
               int(t["inflate_repairs"]), int(t["inflate_candidates"]))


def clean(b):
    return b == bytes([FILL]) * len(b)


def check(c, way, g):
    where = (c.name, way)
    assert clean(g.guard), (where, "guard bytes written")
    if c.code == G.E_ARG:
        assert g.code == G.E_ARG, (where, g.code)
        return
    assert (g.code, g.out_len, g.bits) == (c.code, len(c.out), c.bits), (where, g.code, g.out_len, g.bits)
    assert g.data == c.out, (where, next((i for i, (x, y) in enumerate(zip(g.data, c.out)) if x != y), None))
    if c.code == 0:
        assert clean(g.rest), (where, "bytes written past out_len")
    if c.family != "O":
        assert (g.chains, g.cands) == G.timings(c), (where, g.chains, g.cands, G.timings(c))
    else:
        assert 1 <= g.chains <= G.timings(c)[0], (where, g.chains)
    if way in DEVICE_LINK:
        assert g.repairs == 0, (where, g.repairs)


def run_family(ndfl, contexts, family, deferred=False):
    for c in G.cases(family):
        if deferred and c.code != 0:
            continue
        src = to_dev(c.comp)
        cap = c.info.get("cap", len(c.out)) + (GUARD if c.code == 0 else 1024)
        got = {w: decode(ndfl, contexts[w], c, src, cap, deferred) for w in WAYS}
        ref = got["host_link"]
        for w, g in got.items():
            if not c.silent:
                check(c, w, g)
            print(c.name, w, g.code, g.out_len, g.bits, g.chains, g.repairs, g.cands)
            # the four contexts agree (the bytes between an error's out_len and out_cap are not promised)
            assert (g.code, g.out_len, g.bits, g.data) == (ref.code, ref.out_len, ref.bits, ref.data), (c.name, w)
            assert clean(g.guard) and (g.code != 0 or clean(g.rest)), (c.name, w)
            if family != "O" and g.code >= 0:
                assert (g.chains, g.cands) == (ref.chains, ref.cands), (c.name, w, g.chains, ref.chains)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_family_on_four_contexts(ndfl, contexts, family):
    run_family(ndfl, contexts, family)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_device_link_takes_no_fallback(ndfl, capfd, family):
    """The device-side path hands a decode over to the host linker when a linked chain stops on a boundary that is
    no candidate (LINK_FALLBACK): the result is right, so nothing else shows it.  Under NDFL_STATS=1 each path names
    itself once per decode: no case here may take the host's."""
    ctx = knobs.context(NDFL_STATS=1)
    for c in G.cases(family):
        src = to_dev(c.comp)
        capfd.readouterr()
        g = decode(ndfl, ctx, c, src, c.info.get("cap", len(c.out)) + 1024)
        err = capfd.readouterr().err
        assert err.count("[ndfl] device link: chains") == 1 and "[ndfl] finder quick survivors" not in err, (c.name, err[-400:])
        if not c.silent and c.code != G.E_ARG:
            assert (g.code, g.out_len, g.bits, g.data) == (c.code, len(c.out), c.bits, c.out), c.name


def test_range_slices_with_a_deferred_window(ndfl, contexts):
    run_family(ndfl, contexts, "R", deferred=True)


CAPACITY = {"L": "L_257", "B": "B_emit_buckets_0", "A": "A_after_fixed_offsets", "D": "D_decoys", "R": "R_1_257",
            "O": "O_stored_300", "E": "E_reserved_t2049"}


@pytest.mark.parametrize("family", G.FAMILIES)
def test_capacity_one_byte_short(ndfl, contexts, family):
    """out_cap = n - 1: NDFL_E_CAPACITY, out_len = n, nothing written; out_cap = n: the decode.  Family E's stream also
    holds a real error behind the n bytes (include/ndfl.h does not say which of the two a short buffer reports): the
    device-link contexts are pinned to the host-link path's answer."""
    c = next(c for c in G.cases(family) if c.name == CAPACITY[family])
    n = len(c.out)
    src = to_dev(c.comp)
    got = {w: decode(ndfl, contexts[w], c, src, n - 1) for w in WAYS}
    for w, g in got.items():
        print(c.name, w, g.code, g.out_len, g.bits)
        assert clean(g.data) and clean(g.rest) and clean(g.guard), (c.name, w, "written")
        assert (g.code, g.out_len) == (got["host_link"].code, got["host_link"].out_len), (c.name, w, g.code, g.out_len)
        if c.code == 0:
            assert (g.code, g.out_len) == (G.E_CAPACITY, n), (c.name, w, g.code, g.out_len)
    if c.code == 0:
        for w in WAYS:
            g = decode(ndfl, contexts[w], c, src, n)
            assert (g.code, g.out_len, g.bits, g.data) == (0, n, c.bits, c.out) and clean(g.guard), (c.name, w, "exact capacity")
