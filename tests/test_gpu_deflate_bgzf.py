"""ndfl_deflate_bgzf (include/ndfl.h) on the GPU: a buffer to a blocked gzip (BGZF) file in one call.

The expected file is put together here from pieces that are older than the call: every block through
Context.deflate_members on the wave path with MultiStrategy(X, Uncompressed.SINGLETON) -- the reference's
choice per member -- BSIZE patched in on the host, the members joined, the closing member appended.  The call
must give the same bytes; the files are also read by Python's gzip, walked by BSIZE in plain Python and decoded
by ndfl_inflate_bgzf, whose member table the call's own table must equal.
"""
import ctypes
import functools
import gzip
import os
import random
import re
import struct

import pytest

import bgzf_files as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "deflate-library-java_amd", "csrc", "hip", "deflate_bgzf.hip")
FILL = 0xA5
E_ARG, E_UNSUPPORTED, E_CAPACITY = -1, -2, -3
PRESETS = ["FULL_DYNAMIC", "FULL_STATIC", "RLE_DYNAMIC", "LITERAL_STATIC"]
BLOCK_LENS = [1, 7, 255, 4096, 65280, 65505]
# bytes of a file per block_len: a few blocks and an odd tail (for the 64 KiB sizes: three blocks and a tail)
TOTAL = {1: 150, 7: 1000, 255: 5003, 4096: 45001, 65280: 3 * 65280 + 1234, 65505: 3 * 65505 + 777}
KINDS = ["text", "zeros", "random", "alternating"]


@functools.lru_cache(maxsize=None)
def constants():
    """The tile and block constants of csrc/hip/deflate_bgzf.hip, read out of the source."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (\w+) = (\d+);", open(KERNELS).read())}


@pytest.fixture(scope="module")
def ctx():
    import torch                                           # (before libndfl.so: one HIP runtime for both)
    import ndfl
    c = ndfl.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def preset(name):
    import ndfl
    return getattr(ndfl.Lz77Huffman, name)


def tuple_of(x):
    return (int(x.useDynamicHuffmanCodes),) + tuple(x.params)


@functools.lru_cache(maxsize=None)
def data_of(kind, block_len, total):
    rng = random.Random(f"{kind} {block_len} {total}")
    if kind == "text":
        return B.text(rng, total)
    if kind == "zeros":
        return bytes(total)
    if kind == "random":
        return rng.randbytes(total)
    makers = [lambda n: B.text(rng, n), lambda n: bytes(n), lambda n: rng.randbytes(n)]
    return b"".join(makers[k % 3](min(block_len, total - at)) for k, at in enumerate(range(0, total, block_len)))


def expected_file(ctx, data, block_len, x):
    """The parent's composition, not through bgzf.compress."""
    import ndfl
    from ndfl import bgzf
    blocks = [data[i:i + block_len] for i in range(0, len(data), block_len)]
    members = []
    if blocks:
        members = ctx.deflate_members(blocks, ndfl.FMT_GZIP,
                                      meta=ndfl.GzipMetadata(operatingSystem="UNKNOWN", extraField=bgzf.EXTRA),
                                      strategy=ndfl.MultiStrategy(x, ndfl.Uncompressed.SINGLETON))
    return b"".join(bgzf.member_with_bsize(m) for m in members) + bgzf.EOF


def call(ctx, data, block_len, x, out_cap=None, align=0, null_out=False, table_cap=None, tup=None):
    """One call on host buffers, `out` at byte `align` of a buffer filled with FILL (out_cap None: the bound).
    Returns (result, table, the whole buffer, out_cap)."""
    import ndfl
    L = ndfl._lib.load()
    cap = L.ndfl_bgzf_bound(len(data), block_len) if out_cap is None else out_cap
    src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
    buf = ctypes.create_string_buffer(bytes([FILL]) * (align + cap + 64), align + cap + 64)
    nm = -(-len(data) // max(1, block_len)) + 1
    res, table = ctx.deflate_bgzf_raw(ctypes.addressof(src), len(data), None if null_out else ctypes.addressof(buf) + align,
                                      0 if null_out else cap, tuple_of(x) if tup is None else tup, block_len, 0,
                                      table_cap=nm + 1 if table_cap is None else table_cap)
    return res, table, buf.raw, cap


PRODUCED = {}


def produced(ctx, xname, block_len, kind):
    """(data, result, table, file) of the call for one of the shared files, made once."""
    key = (xname, block_len, kind)
    if key not in PRODUCED:
        data = data_of(kind, block_len, TOTAL[block_len])
        res, table, raw, cap = call(ctx, data, block_len, preset(xname))
        assert res[0] == 0 and res[4] <= cap, res
        assert raw[res[4]:] == bytes([FILL]) * (len(raw) - res[4])
        PRODUCED[key] = (data, res, table, raw[:res[4]])
    return PRODUCED[key]


def walk(f):
    """[(offset, length)] of the members of file f by BSIZE alone, in plain Python; the walk must end at len(f)."""
    out, p = [], 0
    while p < len(f):
        assert f[p:p + 4] == b"\x1f\x8b\x08\x04", p
        assert f[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        n = struct.unpack("<H", f[p + 16:p + 18])[0] + 1
        out.append((p, n))
        p += n
    assert p == len(f)
    return out


# ---- 3. the bytes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_len", BLOCK_LENS)
@pytest.mark.parametrize("xname", PRESETS)
def test_bytes_equal_the_members_path(ctx, xname, block_len):
    for kind in KINDS:
        data, res, table, f = produced(ctx, xname, block_len, kind)
        want = expected_file(ctx, data, block_len, preset(xname))
        assert f == want, (kind, len(f), len(want))
        got, table2 = ctx.deflate_bgzf(data, block_len, preset(xname))
        assert got == want and table2 == table, kind
        assert res[1] == -(-len(data) // block_len) + 1 and res[2] == res[1]


def test_stored_and_fixed_forms_cross(ctx):
    """Random bytes under FULL_STATIC: near 68 bytes a block the stored form (8 n + 40 bits) and the fixed
    one (8 to 9 bits a byte, and 10 more) cross, so both forms occur -- and ties, where chance gives them."""
    stored = fixed = 0
    rng = random.Random(68)
    x = preset("FULL_STATIC")
    for block_len in range(40, 101):
        data = rng.randbytes(24 * block_len + block_len // 2)
        res, table, raw, cap = call(ctx, data, block_len, x)
        assert res[0] == 0
        assert raw[:res[4]] == expected_file(ctx, data, block_len, x), block_len
        stored += res[3]
        fixed += res[1] - 1 - res[3]
    print("stored", stored, "fixed", fixed)
    assert stored > 0 and fixed > 0


# ---- 4. independent of the project -----------------------------------------------------------------------

@pytest.mark.parametrize("block_len", BLOCK_LENS)
@pytest.mark.parametrize("xname", PRESETS)
def test_files_read_elsewhere(ctx, xname, block_len):
    from ndfl import bgzf
    for kind in KINDS:
        data, res, table, f = produced(ctx, xname, block_len, kind)
        assert gzip.decompress(f) == data, kind
        members = walk(f)
        assert len(members) == res[1] and all(n <= 65536 for _, n in members)
        assert f.endswith(B.EOF) and members[-1] == (len(f) - 28, 28)
        assert bgzf.decompress(f, context=ctx) == data, kind


# ---- 5. the table ----------------------------------------------------------------------------------------

def member_counts():
    """1 (empty input), 2, and T - 1, T, T + 1, 2 T + 1 members for the size and offsets passes' tile; the
    same in TILES for the step of the scan kernel they share with the decoder (ndfl_bgzf_sum_kernel, SUM_BLOCK
    tile sums a step)."""
    T, S = constants()["SIZE_TILE"], B.constants()["SUM_BLOCK"]
    return [1, 2, T - 1, T, T + 1, 2 * T + 1] + [T * tiles for tiles in (S - 1, S)] + [T * S + 1, T * 2 * S + 1]


@pytest.mark.parametrize("n_members", member_counts())
def test_table_is_the_decoders(ctx, n_members):
    block_len = 16
    unit = B.text(random.Random(n_members), 4099)          # (4099: the blocks of a period differ)
    n = (n_members - 1) * block_len - (5 if n_members > 1 else 0)
    data = (unit * (n // len(unit) + 1))[:n]
    x = preset("LITERAL_STATIC" if n_members > 4096 else "FULL_DYNAMIC")
    res, table, raw, cap = call(ctx, data, block_len, x)
    assert res[0] == 0 and res[1] == n_members and res[2] == n_members
    f = raw[:res[4]]
    assert len(table) == n_members + 1 and table[-1] == (len(f), len(data)) and table[0] == (0, 0)
    assert table == ctx.bgzf_index(f)
    if n_members <= 4096:
        assert gzip.decompress(f) == data
    else:
        from ndfl import bgzf
        assert bgzf.decompress(f, context=ctx) == data
    # a table_cap below n_members + 1: the first entries, nothing else
    short = call(ctx, data, block_len, x, table_cap=min(3, n_members))[1]
    assert short == table[:min(3, n_members)]


# ---- 6. alignment ----------------------------------------------------------------------------------------

def alignment_files():
    """Alternating text, zero and random blocks of 29..32 bytes under FULL_DYNAMIC: the random ones are stored
    (a dynamic header alone outweighs them: members of 60..63 bytes), the zero ones are not, so offsets and
    lengths run through every residue."""
    return [(bl, data_of("alternating", bl, 40 * bl + 3)) for bl in (29, 30, 31, 32)]


def residues(table):
    offs = [t[0] for t in table]
    return {o % 4 for o in offs[:-1]}, {(b - a) % 4 for a, b in zip(offs, offs[1:])}


@pytest.mark.parametrize("align", range(4))
def test_host_output_at_every_alignment(ctx, align):
    x = preset("FULL_DYNAMIC")
    offs, lens = set(), set()
    for block_len, data in alignment_files():
        res, table, raw, cap = call(ctx, data, block_len, x, align=align)
        assert res[0] == 0 and res[3] > 0
        assert raw[:align] == bytes([FILL]) * align
        assert raw[align:align + res[4]] == expected_file(ctx, data, block_len, x)
        assert raw[align + res[4]:] == bytes([FILL]) * (len(raw) - align - res[4])
        o, n = residues(table)
        offs |= o
        lens |= n
        # every third block is random: stored, a member of block_len + 31 bytes
        assert all(table[k + 1][0] - table[k][0] == block_len + 31 for k in range(2, 40, 3))
    assert offs == {0, 1, 2, 3} and lens == {0, 1, 2, 3}


@pytest.mark.parametrize("align", range(4))
def test_device_buffers_at_every_alignment(ctx, align):
    import torch
    import ndfl
    x = preset("FULL_DYNAMIC")
    offs, lens = set(), set()
    for block_len, data in alignment_files():
        want = expected_file(ctx, data, block_len, x)
        in_at = (align + 1) % 4
        d_in = torch.zeros((len(data) + 32,), dtype=torch.uint8, device="cuda")
        d_in[in_at:in_at + len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        d_out = torch.full((len(want) + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        nm = -(-len(data) // block_len) + 1
        res, table = ctx.deflate_bgzf_raw(d_in.data_ptr() + in_at, len(data), d_out.data_ptr() + align, len(want), tuple_of(x),
                                          block_len, ndfl.IN_DEVICE | ndfl.OUT_DEVICE, table_cap=nm + 1)
        got = bytes(d_out.cpu().numpy())
        assert res[0] == 0 and res[4] == len(want)
        assert got[:align] == bytes([FILL]) * align
        assert got[align:align + len(want)] == want
        assert got[align + len(want):] == bytes([FILL]) * (len(got) - align - len(want))
        assert table == ctx.bgzf_index(want)
        o, n = residues(table)
        offs |= o
        lens |= n
    assert offs == {0, 1, 2, 3} and lens == {0, 1, 2, 3}
    assert ctx.last_kernel_ms() > 0


# ---- 7. capacity -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_capacity(ctx, kind):
    import ndfl
    L = ndfl._lib.load()
    block_len = 255
    data, res, table, f = produced(ctx, "FULL_DYNAMIC", block_len, kind)
    n = len(f)
    short, _, raw, _ = call(ctx, data, block_len, preset("FULL_DYNAMIC"), out_cap=n - 1)
    assert short[0] == E_CAPACITY and short[4] == n and short[1] == res[1]
    assert raw == bytes([FILL]) * len(raw)
    exact, table2, raw, _ = call(ctx, data, block_len, preset("FULL_DYNAMIC"), out_cap=n)
    assert exact[0] == 0 and exact[4] == n and raw[:n] == f and raw[n:] == bytes([FILL]) * 64 and table2 == table
    sizing, table3, _, _ = call(ctx, data, block_len, preset("FULL_DYNAMIC"), null_out=True)
    assert sizing[0] == E_CAPACITY and sizing[4] == n and table3 == table
    bound = L.ndfl_bgzf_bound(len(data), block_len)
    assert n <= bound
    if kind == "random":
        assert n == bound and res[3] == res[1] - 1


# ---- 8. limits -------------------------------------------------------------------------------------------

def test_random_blocks_fill_a_member_exactly(ctx):
    data, res, table, f = produced(ctx, "FULL_DYNAMIC", 65505, "random")
    assert res[3] == res[1] - 1 == 4
    members = walk(f)
    for p, n in members[:3]:
        assert n == 65536 and f[p + 16:p + 18] == b"\xff\xff"
    assert members[3][1] == 777 + 31


def test_a_member_too_long(ctx):
    from ndfl import bgzf
    rng = random.Random(65536)
    data = B.text(rng, 65536) + rng.randbytes(65536) + B.text(rng, 100)
    res, table, raw, cap = call(ctx, data, 65536, preset("FULL_DYNAMIC"))
    assert res[0] == E_UNSUPPORTED and res[1] == 4 and res[2] == 1, res
    with pytest.raises(ValueError):
        bgzf.compress(data, block_len=65536, context=ctx)
    with pytest.raises(ValueError):
        ctx.deflate_bgzf(data, 65536)
    ok = bgzf.compress(data[:65536] + data[-100:], block_len=65536, context=ctx)
    assert gzip.decompress(ok) == data[:65536] + data[-100:]


def test_empty_input(ctx):
    res, table, raw, cap = call(ctx, b"", 65280, preset("FULL_DYNAMIC"))
    assert cap == 28 and res == (0, 1, 1, 0, 28)
    assert raw[:28] == B.EOF and raw[28:] == bytes([FILL]) * 64
    assert table == [(0, 0), (28, 0)]
    assert ctx.deflate_bgzf(b"") == (B.EOF, [(0, 0), (28, 0)])


def test_arguments(ctx):
    import ndfl
    x = preset("FULL_DYNAMIC")
    with pytest.raises(ndfl.NdflError) as e:
        call(ctx, b"abc", 0, x, out_cap=100)
    assert e.value.code == E_ARG
    res, table, raw, _ = call(ctx, b"abc", 65537, x, out_cap=100)
    assert res == (E_UNSUPPORTED, 0, 0, 0, 0) and table == [] and raw == bytes([FILL]) * len(raw)
    for tup in [(1, 2, 258, 1, 32768), (1, 3, 259, 1, 32768), (1, 5, 4, 1, 10), (1, 3, 258, 0, 10), (1, 3, 258, 1, 32769),
                (1, 3, 258, 10, 9)]:
        for block_len in (65280, 65537):                  # (the tuple is checked first)
            with pytest.raises(ndfl.NdflError) as e:
                call(ctx, b"abc", block_len, x, out_cap=100, tup=tup)
            assert e.value.code == E_ARG, tup
    L = ndfl._lib.load()
    one = ndfl._lib.BgzfWriteResult()
    args = (ctypes.byref(one), None, 0, 1, 3, 258, 1, 32768, 65280, 0)
    buf = ctypes.create_string_buffer(64)
    assert L.ndfl_deflate_bgzf(None, ctypes.addressof(buf), 3, ctypes.addressof(buf), 64, *args) == E_ARG
    assert L.ndfl_deflate_bgzf(ctx._h, None, 3, ctypes.addressof(buf), 64, *args) == E_ARG
    assert L.ndfl_deflate_bgzf(ctx._h, ctypes.addressof(buf), 3, None, 64, *args) == E_ARG
    assert L.ndfl_deflate_bgzf(ctx._h, ctypes.addressof(buf), 3, ctypes.addressof(buf), 64, None, *args[1:]) == E_ARG
    assert L.ndfl_deflate_bgzf(ctx._h, ctypes.addressof(buf), 3, ctypes.addressof(buf), 64, args[0], None, 5, *args[3:]) == E_ARG
    # past 8 GiB: refused before the input is read
    assert L.ndfl_deflate_bgzf(ctx._h, ctypes.addressof(buf), (8 << 30) + 1, None, 0, *args) == E_UNSUPPORTED
    assert L.ndfl_deflate_bgzf(ctx._h, ctypes.addressof(buf), 1 << 31, None, 0, *args[:8], 1, 0) == E_UNSUPPORTED


# ---- 9. bgzf.compress ------------------------------------------------------------------------------------

def test_compress_goes_through_the_call(ctx):
    import ndfl
    from ndfl import bgzf
    data = data_of("alternating", 4096, TOTAL[4096])
    assert bgzf.compress(data, block_len=4096, context=ctx) == expected_file(ctx, data, 4096, preset("FULL_DYNAMIC"))
    static = ndfl.MultiStrategy(ndfl.Lz77Huffman.FULL_STATIC, ndfl.Uncompressed.SINGLETON)
    assert bgzf.compress(data, block_len=4096, strategy=static, context=ctx) == expected_file(ctx, data, 4096, preset("FULL_STATIC"))
    data = data_of("alternating", 65280, TOTAL[65280])
    assert bgzf.compress(data, context=ctx) == expected_file(ctx, data, 65280, preset("FULL_DYNAMIC"))
    three = ndfl.MultiStrategy(ndfl.Lz77Huffman.FULL_DYNAMIC, ndfl.Lz77Huffman.RLE_DYNAMIC, ndfl.Uncompressed.SINGLETON)
    f = bgzf.compress(data, strategy=three, context=ctx)
    assert gzip.decompress(f) == data and bgzf.decompress(f, context=ctx) == data and walk(f)[-1][1] == 28
