"""ndfl_inflate_bgzf on the GPU: a blocked gzip (BGZF) file's members found and laid out on the device and
decoded in one call.  Every case is compared field by field with the host model of tests/bgzf_files.py
(whose per-member outcomes are the CPU oracle's), on the default context, on one wave
(NDFL_BATCH_WAVES=1) and with the discovery and layout grids held to three workgroups (NDFL_BGZF_GRID=3:
every workgroup strides over tiles, as it does by itself only from 32 MiB of input or a million candidates
on); `out` is pre-filled with a canary and checked outside the stored bytes; the
well-formed files are also compared with Context.inflate_members on host-built items.

The cases are the places where the new kernels (csrc/hip/inflate_bgzf.hip) can go wrong: member counts
around every tile and block constant and past the candidate list's first capacity, headers of every
shape, member starts straddling a scan tile's edge, look-alike headers off the chain, every way a chain
can end, the first error in file order, and the capacity rules.
"""
import ctypes
import gzip
import random
import struct

import pytest

import bgzf_files as B
import knobs
import oracle_lib as O
from test_oracle_inflate import reserved_symbol_streams

pytestmark = pytest.mark.gpu

FILL = 0xA5
GZIP = 2
UEOS = "UNEXPECTED_END_OF_STREAM"
CONTEXTS = {}


@pytest.fixture(scope="module", params=["default", "one wave", "strided"])
def ctx(request):
    import torch
    import ndfl
    if request.param not in CONTEXTS:
        c = (ndfl.Context(0) if request.param == "default" else knobs.context(NDFL_BATCH_WAVES=1)
             if request.param == "one wave" else knobs.context(NDFL_BGZF_GRID=3))
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        CONTEXTS[request.param] = c
    return CONTEXTS[request.param]


def code_of(status):
    return 0 if status is None else status if isinstance(status, int) else O.REASONS.index(status) + 1


def exact_cap(f):
    """The output capacity of a call that names none: exactly the total of the ISIZE fields -- but no more
    than 1 MiB (the last four bytes of a member cut short are anything): such a file is a capacity case."""
    members, _ = B.chain(bytes(f))
    return min(sum(m[2] for m in members), 1 << 20)


def run(ctx, f, out_cap=None, table_cap=None, null_out=False):
    """One call on host buffers.  out_cap None: exact_cap.  Returns (result, table, the whole out buffer:
    out_cap bytes and 64 more, all pre-filled with FILL)."""
    members, _ = B.chain(bytes(f))
    cap = exact_cap(f) if out_cap is None else out_cap
    src = ctypes.create_string_buffer(bytes(f), max(1, len(f)))
    out = ctypes.create_string_buffer(bytes([FILL]) * (cap + 64), cap + 64)
    tcap = len(members) + 1 if table_cap is None else table_cap
    res, table = ctx.inflate_bgzf_raw(ctypes.addressof(src), len(f), None if null_out else ctypes.addressof(out),
                                      0 if null_out else cap, 0, table_cap=tcap)
    return res, table, out.raw


def check(f, got, out_cap=None, table_cap=None, what=""):
    """`got` = run()'s return against the model, field by field, and the canary."""
    res, table, out = got
    cap = exact_cap(f) if out_cap is None else out_cap
    m = B.model(f, cap)
    code, sym, n, bad, olen, consumed = res
    assert code == code_of(m["status"]), (what, res, m["status"])
    assert sym == (m["symbol"] if code > 0 else -1), (what, res)
    assert (n, bad, olen, consumed) == (m["n_members"], m["bad_member"], m["out_len"], m["consumed_bytes"]), \
        (what, res, {k: v for k, v in m.items() if k not in ("out", "table")})
    tcap = n + 1 if table_cap is None else table_cap
    assert table == m["table"][:min(tcap, n + 1)], what
    fill = bytes([FILL])
    if code == B.E_CAPACITY:
        assert out == fill * len(out), (what, "written under E_CAPACITY")
        return m
    stored = len(m["out"])
    assert out[:stored] == m["out"], (what, "output differs")
    clean_from = stored if code == 0 else m["total"]           # (on a Reason [out_len, total) is unspecified)
    assert out[clean_from:] == fill * (len(out) - clean_from), (what, "canary")
    assert clean_from <= cap
    return m


def run_check(ctx, f, what="", **kw):
    return check(f, run(ctx, f, **kw), kw.get("out_cap"), kw.get("table_cap"), what)


def sub(a, b, v):
    return bytes([a, b]) + struct.pack("<H", len(v)) + v


# ---- member counts, header shapes --------------------------------------------------------------------------

@pytest.mark.parametrize("name,members", B.well_formed_files(), ids=[f[0] for f in B.well_formed_files()])
def test_well_formed(ctx, name, members):
    f = b"".join(members)
    m = run_check(ctx, f, name, out_cap=B.offsets(members)[-1][1])       # (exactly enough, also above exact_cap's 1 MiB)
    assert m["status"] is None and m["n_members"] == len(members) and m["consumed_bytes"] == len(f)
    assert m["out"] == gzip.decompress(f)
    if not members or len(members) > 20000:                # (marshalling a quarter of a million items takes seconds)
        return
    # the same members as host-built items of ndfl_inflate_members
    items = [(p, q - p, o, o2 - o, GZIP, 0) for (p, o), (q, o2) in zip(m["table"], m["table"][1:])]
    src = ctypes.create_string_buffer(f, len(f))
    out = ctypes.create_string_buffer(bytes([FILL]) * (m["total"] + 1), m["total"] + 1)
    res = ctx.inflate_members_raw(ctypes.addressof(src), len(f), ctypes.addressof(out), m["total"], items, 0)
    assert all(r[0] == 0 for r in res) and out.raw == m["out"] + bytes([FILL])


def test_python_index_and_decode(ctx):
    for name, members in B.well_formed_files()[:8]:
        f = b"".join(members)
        m = B.model(f)
        assert ctx.bgzf_index(f) == m["table"], name
        assert ctx.inflate_bgzf(f) == (None, m["out"], len(f), len(members)), name


def test_not_a_member_start(ctx):
    """A header that fails the member-start rule ends the chain in front of it -- at byte 0: no member."""
    rng = random.Random(7)
    d = B.text(rng, 300)
    good = B.member(d)
    n0 = len(B.member(d)) - 1
    for what, m in (("FLG without bit 2", B.member(d, flg=0)), ("wrong SLEN", B.member(d, slen=3)),
                    ("SLEN 0", B.member(d, slen=0)), ("BX", B.member(d, ids=b"BX")),
                    ("BSIZE + 1 one below the minimum", B.member(d, bsize=12 + 6 + 8 - 2)),
                    ("BC cut by XLEN", B.member(d, before=sub(1, 1, b"q"))[:10] + b"\x09\x00" +
                     B.member(d, before=sub(1, 1, b"q"))[12:]),
                    ("method 9", good[:2] + b"\x09" + good[3:]), ("magic", b"\x1f\x8c" + good[2:])):
        r = run_check(ctx, good + m + good, what)
        assert r["n_members"] == 1 and r["consumed_bytes"] == len(good) and r["status"] is None, what
        r = run_check(ctx, m + good, what + " at byte 0")
        assert r["n_members"] == 0 and r["out_len"] == 0 and r["consumed_bytes"] == 0 and r["status"] is None, what
    # the minimum itself is a member start (its 26 bytes hold no DEFLATE data, and the chain goes on into its body:
    # a Reason, or a capacity case by the ISIZE read there)
    r = run_check(ctx, good + B.member(d, bsize=12 + 6 + 8 - 1) + good, "BSIZE + 1 at the minimum")
    assert r["n_members"] >= 2 and r["status"] is not None and n0 > 26


# ---- tile edges ----------------------------------------------------------------------------------------------

def filler(rng, length):
    """One member of exactly `length` bytes (a padding subfield before BC makes up the difference)."""
    d = B.text(rng, 900)
    base = len(B.member(d, before=sub(1, 1, b"")))
    assert length >= base
    m = B.member(d, before=sub(1, 1, bytes(length - base)))
    assert len(m) == length
    return m


def test_member_starts_across_a_scan_tile_edge(ctx):
    """A member start at every offset from T - 20 to T + 1 of the scan's tile, and of its second tile: the
    12 fixed bytes, the extra field and the BC subfield straddle the edge in every way."""
    T = B.constants()["FIND_TILE"]
    rng = random.Random(11)
    d = B.text(rng, 200)
    for edge in (T, 2 * T):
        for at in range(edge - 20, edge + 2):
            for second in (B.member(d), B.member(d, before=sub(5, 5, b"0123456789"))):
                first = filler(rng, at) if edge == T else filler(rng, 3000) + filler(rng, at - 3000)
                f = first + second + B.EOF
                m = run_check(ctx, f, f"start at {at}")
                assert m["status"] is None and m["consumed_bytes"] == len(f) and at in [t[0] for t in m["table"]]


def test_thread_edges_inside_a_tile(ctx):
    """Member starts at 16 consecutive offsets: every position of a scan thread's own bytes."""
    rng = random.Random(13)
    d = B.text(rng, 50)
    for at in range(1000, 1017):
        f = filler(rng, at) + B.member(d) + B.EOF
        assert run_check(ctx, f, f"start at {at}")["n_members"] == 3


def test_device_input_at_every_alignment(ctx):
    import torch
    import ndfl
    name, members = [x for x in B.well_formed_files() if x[0] == "65 members"][0]
    f = b"".join(members)
    m = B.model(f)
    n = len(f)
    for align in range(4):
        for padded in (False, True):
            d_in = torch.zeros((n + ndfl.IN_PAD_BYTES + 32,), dtype=torch.uint8, device="cuda")
            assert d_in.data_ptr() % 16 == 0
            d_in[align:align + n].copy_(torch.frombuffer(bytearray(f), dtype=torch.uint8))
            d_out = torch.full((m["total"] + 64,), FILL, dtype=torch.uint8, device="cuda")
            flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | (ndfl.IN_PADDED if padded else 0)
            res, table = ctx.inflate_bgzf_raw(d_in.data_ptr() + align, n, d_out.data_ptr(), m["total"], flags,
                                              table_cap=len(members) + 1)
            check(f, (res, table, bytes(d_out.cpu().numpy())), what=f"align {align} padded {padded}")
    assert ctx.last_kernel_ms() > 0


# ---- false candidates ------------------------------------------------------------------------------------

def test_look_alike_headers_off_the_chain(ctx):
    rng = random.Random(17)
    d = B.text(rng, 400)
    fakes = b"".join(B.member(B.text(rng, 60 + k)) for k in range(6))          # complete members chaining to each other
    carrier = B.member(b"head" + fakes + b"tail", level=0)
    assert fakes in carrier
    after = B.member(d)
    # a complete fake header in a stored payload's last bytes, its BSIZE leading to the real start behind it
    hdr = bytearray(B.member(b"")[:18])
    hdr[16:18] = struct.pack("<H", 18 + 8 - 1)
    lure = B.member(d + bytes(hdr), level=0)
    assert lure[-26:-8] == bytes(hdr)
    f = B.member(d) + carrier + lure + after + B.EOF
    starts = [p for p in range(len(f)) if B.member_start(f, p)]
    m = run_check(ctx, f, "look-alikes")
    assert m["status"] is None and m["n_members"] == 5 and len(starts) == 5 + 6 + 1 and m["consumed_bytes"] == len(f)
    assert B.member_start(f, len(f) - 28 - len(after) - 26) == 26               # the lure points at `after`
    # the same bytes without the first member: byte 0 still decides
    g = b"x" + f
    assert run_check(ctx, g, "shifted")["n_members"] == 0
    # look-alikes denser than the candidate list's first capacity: the file is scanned again
    many = B.member(bytes(hdr) * 3000, level=0) + B.member(bytes(hdr) * 3000, level=0) + B.EOF
    assert len([p for p in range(0, len(many)) if many[p:p + 3] == b"\x1f\x8b\x08"]) > B.list_capacity(len(many))
    m = run_check(ctx, many, "dense look-alikes")
    assert m["status"] is None and m["n_members"] == 3


# ---- chain ends ------------------------------------------------------------------------------------------

def test_cut_at_every_byte_of_the_last_member(ctx):
    rng = random.Random(19)
    a, b = B.member(B.text(rng, 500)), B.member(B.text(rng, 100))
    # (a stored block of zeros: the layout reads a cut member's last four bytes as its ISIZE, and where they
    # are not small -- the stored block's NLEN, the trailer's CRC -- the cut file is a capacity case)
    last = B.member(bytes(40), level=0, before=sub(2, 2, b"ab"), name=b"nm", hcrc=True)
    assert len(last) < 120
    f = a + b + last
    seen = set()
    for cut in range(len(a) + len(b), len(f) + 1):
        m = run_check(ctx, f[:cut], f"cut at {cut - len(a) - len(b)}")
        seen.add((m["n_members"], m["status"]))
        assert m["consumed_bytes"] == (cut if m["n_members"] == 3 else len(a) + len(b))
    assert seen == {(2, None), (3, UEOS), (3, B.E_CAPACITY), (3, None)}


def test_chain_ends(ctx):
    rng = random.Random(23)
    d = B.text(rng, 600)
    a, b = B.member(d), B.member(d[:77])
    m = run_check(ctx, a + b + rng.randbytes(40) + a, "garbage where the next header should be")
    assert m["n_members"] == 2 and m["status"] is None and m["consumed_bytes"] == len(a) + len(b)
    m = run_check(ctx, a + b + B.EOF + b"junk", "trailing junk")
    assert m["n_members"] == 3 and m["consumed_bytes"] == len(a) + len(b) + 28
    m = run_check(ctx, a + b, "no EOF marker")
    assert m["n_members"] == 2 and m["status"] is None
    # BSIZE overstates the member: the bytes behind the trailer are skipped (they end with the ISIZE again)
    padded = B.member(d, pad=b"padding!" + struct.pack("<I", len(d)))
    m = run_check(ctx, a + padded + b + B.EOF, "padding")
    assert m["n_members"] == 4 and m["status"] is None and m["out"] == d + d + d[:77]
    # ... and where they do not, the layout's ISIZE is wrong: that member's size mismatch
    for pad in (bytes(5), struct.pack("<I", len(d) + 9)):
        m = run_check(ctx, a + B.member(d, pad=pad) + b + B.EOF, "padding, other ISIZE")
        assert (m["status"], m["bad_member"]) == (B.SIZE_MISMATCH, 1)
    # BSIZE understates the member: it loses its last four bytes, and what follows is no member start (the
    # four before them, read as its ISIZE, are written to say its length: the case is the decode's, not capacity's)
    m = run_check(ctx, a + B.member(d, bsize_add=-4, crc=len(d)) + b + B.EOF, "BSIZE understates")
    assert (m["status"], m["bad_member"], m["n_members"]) == (UEOS, 1, 2)


# ---- errors ------------------------------------------------------------------------------------------------

def error_members(rng):
    d = B.text(rng, 800)
    name, body, _, reason, symbol = reserved_symbol_streams()[0]
    return d, {
        "crc": (B.member(d, crc=0x12345678), "DECOMPRESSED_CHECKSUM_MISMATCH"),
        "isize small": (B.member(d, isize=len(d) - 5), B.SIZE_MISMATCH),
        "isize large": (B.member(d, isize=len(d) + 5), B.SIZE_MISMATCH),
        "reserved flags": (B.member(d, flg=4 | 0x40), "GZIP_RESERVED_FLAGS_SET"),
        "os byte": (B.member(d, os_=14), "GZIP_UNSUPPORTED_OPERATING_SYSTEM"),
        "header crc": (B.member(d, hcrc=True)[:18] + b"\0\0" + B.member(d, hcrc=True)[20:], "HEADER_CHECKSUM_MISMATCH"),
        "deflate": (B.member(b"", body=body), reason),
    }


def test_first_error_in_file_order(ctx):
    rng = random.Random(29)
    d, bad = error_members(rng)
    good = [B.member(B.text(rng, 100 + 37 * k)) for k in range(9)]
    for what, (m, reason) in bad.items():
        for at in (0, 4, 9):
            ms = good[:at] + [m] + good[at:]
            r = run_check(ctx, b"".join(ms), f"{what} at {at}")
            assert (r["status"], r["bad_member"], r["n_members"]) == (reason, at, 10), (what, at, r["status"])
            if what.startswith("isize"):
                assert r["out_len"] == r["table"][at][1] + len(d)
                assert r["table"][at + 1][1] - r["table"][at][1] == len(d) + (5 if "large" in what else -5)
            if what == "deflate":
                assert r["symbol"] == reserved_symbol_streams()[0][4] and r["symbol"] >= 0
    # two bad members, both orders: the lower index wins
    for x, y in (("crc", "isize small"), ("isize small", "crc"), ("deflate", "os byte"), ("os byte", "deflate")):
        ms = good[:2] + [bad[x][0]] + good[2:7] + [bad[y][0]] + good[7:]
        r = run_check(ctx, b"".join(ms), f"{x} before {y}")
        assert (r["status"], r["bad_member"]) == (bad[x][1], 2)
    # ... also with hundreds of members between and behind them
    ms = [B.EMPTY] * 300 + [bad["isize large"][0]] + [B.EMPTY] * 300 + [bad["crc"][0]] + good + [B.EMPTY] * 300
    r = run_check(ctx, b"".join(ms), "far apart")
    assert (r["status"], r["bad_member"]) == (B.SIZE_MISMATCH, 300)


# ---- capacity ----------------------------------------------------------------------------------------------

def test_capacity_and_tables(ctx):
    rng = random.Random(31)
    ms = [B.member(B.text(rng, 300 + k)) for k in range(5)] + [B.EMPTY]
    f = b"".join(ms)
    total = B.model(f)["total"]
    n = len(ms)
    for cap in (total - 1, 0, 1):
        m = run_check(ctx, f, f"out_cap {cap}", out_cap=cap)
        assert m["status"] == B.E_CAPACITY and m["out_len"] == total and len(m["table"]) == n + 1
    res, table, _ = run(ctx, f, null_out=True)
    assert res == (B.E_CAPACITY, -1, n, n, total, len(f)) and table == B.offsets(ms)
    for tcap in (0, 1, n, n + 1, n + 5):
        run_check(ctx, f, f"table_cap {tcap}", table_cap=tcap)
        run_check(ctx, f, f"table_cap {tcap}, no room", table_cap=tcap, out_cap=total - 1)
    run_check(ctx, f, "more room than needed", out_cap=total + 40)
    # a bad member AND too little room: nothing is decoded
    g = b"".join(ms[:2] + [B.member(b"abc", crc=5)] + ms[2:])
    assert run_check(ctx, g, "bad member, no room", out_cap=total)["status"] == B.E_CAPACITY
    assert run_check(ctx, g, "bad member, room", out_cap=total + 3)["status"] == "DECOMPRESSED_CHECKSUM_MISMATCH"


def test_isize_sum_past_32_bits(ctx):
    """Lying ISIZEs that sum past 2^32: the required size is exact in 64 bits, and nothing is decoded."""
    ms = [B.member(b"tiny", isize=0xFFFFFFF0), B.member(b"small", isize=0xFFFFFF00), B.member(b"x", isize=0x80000000),
          B.EMPTY]
    f = b"".join(ms)
    total = 0xFFFFFFF0 + 0xFFFFFF00 + 0x80000000
    for null_out, cap in ((True, 0), (False, 4096)):
        got = run(ctx, f, out_cap=cap, null_out=null_out)
        assert got[0] == (B.E_CAPACITY, -1, 4, 4, total, len(f))
        assert got[1] == [(0, 0), (len(ms[0]), 0xFFFFFFF0), (len(ms[0]) + len(ms[1]), 0xFFFFFFF0 + 0xFFFFFF00),
                          (len(f) - 28, total), (len(f), total)]
        assert got[2] == bytes([FILL]) * len(got[2])


def test_arguments(ctx):
    import ndfl
    L = ndfl._lib.load()
    f = B.member(b"args") + B.EOF
    src = ctypes.create_string_buffer(f, len(f))
    out = ctypes.create_string_buffer(64)
    res = ndfl._lib.BgzfResult()
    tab = (ndfl._lib.BgzfMember * 4)()
    a_in, a_out = ctypes.addressof(src), ctypes.addressof(out)
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, len(f), a_out, 64, None, tab, 4, 0) == ndfl._lib.E_ARG
    assert L.ndfl_inflate_bgzf(ctx._h, None, len(f), a_out, 64, ctypes.byref(res), tab, 4, 0) == ndfl._lib.E_ARG
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, len(f), None, 64, ctypes.byref(res), tab, 4, 0) == ndfl._lib.E_ARG
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, len(f), a_out, 64, ctypes.byref(res), None, 4, 0) == ndfl._lib.E_ARG
    assert L.ndfl_inflate_bgzf(None, a_in, len(f), a_out, 64, ctypes.byref(res), tab, 4, 0) == ndfl._lib.E_ARG
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, len(f), a_out, 64, ctypes.byref(res), tab, 4, 0) == 0
    assert (res.n_members, res.out_len, out.raw[:4]) == (2, 4, b"args")
    with pytest.raises(ndfl.NdflError) as e:
        ctx.inflate_bgzf(f, out_cap=3)
    assert e.value.code == ndfl._lib.E_CAPACITY
    # more than 8 GiB of input is refused before anything is read (candidate indices are 32-bit)
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, (8 << 30) + 1, a_out, 64, ctypes.byref(res), tab, 4,
                               ndfl.IN_DEVICE) == ndfl._lib.E_UNSUPPORTED
    # no input: no member, and no kernel time left over from the call before
    assert L.ndfl_inflate_bgzf(ctx._h, a_in, 0, a_out, 64, ctypes.byref(res), tab, 4, 0) == 0
    assert (res.n_members, res.out_len, res.consumed_bytes, tab[0].in_off, tab[0].out_off) == (0, 0, 0, 0, 0)
    assert ctx.last_kernel_ms() == 0


def test_python_returns_the_stored_bytes(ctx):
    """Context.inflate_bgzf on a Reason: the bytes stored, which end with the failing member's region."""
    import ndfl
    a, b = b"first member " * 5, b"second member " * 5
    for isize, kept in ((len(b) - 9, len(b) - 9), (len(b) + 9, len(b))):
        f = B.member(a) + B.member(b, isize=isize) + B.member(a) + B.EOF
        for cap in (None, len(a) + isize + len(a)):
            reason, out, consumed, n = ctx.inflate_bgzf(f, out_cap=cap)
            assert (reason, consumed, n) == (ndfl.Reason.DECOMPRESSED_SIZE_MISMATCH, len(f), 4)
            assert out == a + b[:kept]


# ---- the Python module ---------------------------------------------------------------------------------------

def test_python_round_trip(ctx):
    import ndfl
    rng = random.Random(37)
    for n in (0, 1, 65280, 65281, 200000):
        d = rng.randbytes(n)
        f = ndfl.bgzf.compress(d, context=ctx)
        assert gzip.decompress(f) == d and ndfl.bgzf.decompress(f, context=ctx) == d
        members, consumed = B.chain(f)
        assert consumed == len(f) and len(members) == -(-n // 65280) + 1 and f.endswith(B.EOF)
        for p, mlen, isize in members:
            assert mlen <= 65536 and (f[p + 16] | f[p + 17] << 8) == mlen - 1 and f[p + 9] == 255
        assert sum(m[2] for m in members) == n
    text = B.text(rng, 150000)
    f = ndfl.bgzf.compress(text, block_len=40000, strategy=ndfl.Strategy.RLE_DYNAMIC, context=ctx)
    assert len(B.chain(f)[0]) == 5 and gzip.decompress(f) == text and ndfl.bgzf.decompress(f, context=ctx) == text
    with pytest.raises(ValueError):
        ndfl.bgzf.decompress(f + b"junk", context=ctx)
    with pytest.raises(ValueError):
        ndfl.bgzf.decompress(gzip.compress(text), context=ctx)
    with pytest.raises(ValueError):
        ndfl.bgzf.decompress(b"", context=ctx)
    bad = bytearray(f)
    bad[len(f) - 28 - 6] ^= 1                                  # the last data member's CRC
    with pytest.raises(ndfl.DataFormatException) as e:
        ndfl.bgzf.decompress(bytes(bad), context=ctx)
    assert e.value.getReason() == ndfl.Reason.DECOMPRESSED_CHECKSUM_MISMATCH
