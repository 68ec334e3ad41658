"""GPU parity of the LZ77 match search at its window, run, tile and bucket limits: the constructed inputs
of tests/lz_geometry.py (every match at a chosen place relative to a limit of lz77_kernels.hip; their
parses are pinned on the CPU by tests/test_lz_geometry_cpu.py) through every search path, byte for byte
against O.deflate_lz(data, *params, chunk_len, hist_limit):

    default     lzp_search per tile + the encode kernel's walk and fallback (ctx.deflate)
    no lead     NDFL_LZ_LEAD=0: tiles are entered at positions no wave searched, the fallback supplies them
    chain       NDFL_LZ_SEARCH=chain: the hash-chain search at every position
    segmented   the SEG = true instantiations: every case of one (params, chunk_len, hist_limit) as one batch
                of RAW streams through ndfl_deflate_batch_chunked, in builder order, reversed (the tiles then
                fall at other places in each stream) and with slabs of 8192 staged bytes
    across      families A and B through DeflaterOutputStream, written 1000 bytes at a time with batch_bytes
                40000 and 65536: the window, history and run-limit cases built for it (call_offset*, calls_*)
                have their destinations in the second call and their sources in the history carried over
                from the first; the cases shorter than a batch go out in one call

On a mismatch the message names the case and the first differing block and token.  The engagement test
reads the fallback count that a context created with NDFL_LZ_STATS=1 prints.
"""
import collections
import functools
import io
import re

import pytest

import adversarial_hist as A
import deflate_batch_harness as H
import knobs
import lz_geometry as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

WAYS = {"default": {}, "no_lead": {"NDFL_LZ_LEAD": "0"}, "chain": {"NDFL_LZ_SEARCH": "chain"}}


@pytest.fixture(scope="module")
def ndfl():
    import torch  # noqa: F401 (before libndfl.so, as in deflate_batch_harness.ctx: the segmented tests share torch's stream)
    import ndfl as N
    return N


@pytest.fixture(scope="module")
def contexts(ndfl):
    return {way: knobs.context(**env) if env else ndfl.Context(0) for way, env in WAYS.items()}


@functools.lru_cache(maxsize=None)
def expected(family, i):
    """The oracle's stream of case i of a family (computed once, shared by the tests)."""
    c = G.cases(family)[i]
    return O.deflate_lz(c.data, *c.params, c.chunk_len, c.hist_limit)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("family", G.FAMILIES)
def test_search_matches_oracle(ndfl, contexts, family, way):
    wrong = []                                             # every failing case is named, not only the first
    for i, c in enumerate(G.cases(family)):
        got = contexts[way].deflate(c.data, ndfl.Lz77Huffman(*c.params), chunk_len=c.chunk_len, hist_limit=c.hist_limit)
        exp = expected(family, i)
        if got != exp:
            wrong.append((c.name, A.explain(exp, got)))
    assert not wrong, (way, family, wrong)


# ---- segmented: ndfl_deflate_batch_chunked ----------------------------------------------------------------
def raw(ctx, in_addr, in_size, out_addr, out_size, recs, cfg, flags):
    """ndfl_deflate_batch_chunked; cfg: (params, chunk_len, hist_limit)."""
    params, chunk_len, hist_limit = cfg
    return ctx.deflate_batch_chunked_raw(in_addr, in_size, out_addr, out_size, recs, *params, chunk_len, hist_limit, flags)


def batches(family):
    """{(params, chunk_len, hist_limit): [case]} of a family, in builder order."""
    out = collections.OrderedDict()
    for c in G.cases(family):
        out.setdefault((c.params, c.chunk_len, c.hist_limit), []).append(c)
    return out


def run_batches(ctx, family, what, reverse=False):
    for cfg, cs in batches(family).items():
        cs = cs[::-1] if reverse else cs
        try:
            H.run_check(raw, H.lz_oracle, ctx, H.raws([c.data for c in cs]), cfg, what)
        except AssertionError as e:
            raise AssertionError((what, family, [c.name for c in cs], cfg, e.args)) from None


@pytest.fixture(scope="module")
def seg_ctx(ndfl):
    import torch
    c = ndfl.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@pytest.fixture(scope="module")
def small_slab(ndfl):
    import torch
    c = knobs.context(NDFL_SEG_SLAB=8192)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@pytest.mark.parametrize("family", G.FAMILIES)
def test_segmented_matches_oracle(seg_ctx, family):
    run_batches(seg_ctx, family, "segmented")
    run_batches(seg_ctx, family, "segmented, reversed", reverse=True)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_segmented_in_small_slabs(small_slab, family):
    run_batches(small_slab, family, "segmented, 8192-byte slabs")


# ---- across calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_bytes", [40000, 65536])
@pytest.mark.parametrize("family", ["A", "B"])
def test_history_carried_across_calls(ndfl, contexts, family, batch_bytes):
    carried, wrong = 0, []
    for i, c in enumerate(G.cases(family)):
        bout = io.BytesIO()
        d = ndfl.DeflaterOutputStream(bout, c.chunk_len, c.hist_limit, ndfl.Lz77Huffman(*c.params),
                                      context=contexts["default"], batch_bytes=batch_bytes)
        for off in range(0, len(c.data), G.PIECE):
            d.write(c.data, off, min(G.PIECE, len(c.data) - off))
        d.finish()
        exp = expected(family, i)
        if bout.getvalue() != exp:
            wrong.append((c.name, A.explain(exp, bout.getvalue())))
        carried += len(G.carried(c, batch_bytes))
    assert not wrong, (family, batch_bytes, wrong)
    # planted tokens whose destination lay in a later call than their source
    assert carried == G.CARRIED[family][batch_bytes], carried


# ---- engagement: the fallback search runs where the design says, and only there ----------------------------
def fallbacks(ctx, ndfl, capfd, data):
    capfd.readouterr()
    ctx.deflate(data, ndfl.Lz77Huffman(*G.FULL))
    err = capfd.readouterr().err
    m = re.search(r"\[ndfl\] lz parse-driven match:.* (\d+) fallback searches in the encode kernel", err)
    assert m, err
    return int(m.group(1))


def test_fallback_search_engages(ndfl, capfd):
    """Period 258: the true path visits the multiples of 258 and the second tile's lead path 7936 + 258 k, so
    they never merge and every token of the later tiles comes from lz_match_global.  off_lead: the true
    path enters the second tile on a 1000-byte copy that began 6 positions before the lead-in's start.
    Pure filler: every position is a literal, every parse merges at once, no fallback."""
    ctx = knobs.context(NDFL_LZ_STATS=1)
    e = {c.name: c for c in G.cases("E")}["period_258_chunk65536"]
    d = {c.name: c for c in G.cases("D")}["off_lead"]
    counts = {"period_258": fallbacks(ctx, ndfl, capfd, e.data), "off_lead": fallbacks(ctx, ndfl, capfd, d.data),
              "pure_filler": fallbacks(ctx, ndfl, capfd, G.pure_filler())}
    print("fallback searches:", counts)
    assert counts["period_258"] > 0 and counts["off_lead"] > 0 and counts["pure_filler"] == 0, counts
