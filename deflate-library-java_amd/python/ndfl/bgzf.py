"""Blocked gzip (BGZF) files -- bgzip, BAM, tabix-indexed VCF / BED: a concatenation of gzip members of
at most 64 KiB, each with its own length (BSIZE) in a `BC` extra subfield, closed by an empty member.

decompress() is one ndfl_inflate_bgzf call (after its sizing call): the members are found and laid
out on the GPU and decoded in one launch.  compress() is one ndfl_deflate_bgzf call for the strategies
that call takes -- a MultiStrategy of one Lz77Huffman and Uncompressed, the default among them: the blocks
are compressed, sized and packed back to back on the GPU.  Any other strategy cuts the data into blocks
on the host and compresses them in one deflate_members call; only BSIZE, which depends on the compressed
length, is then patched in on the host.
"""
import ctypes

from . import _lib
from . import DataFormatException, Lz77Huffman, MultiStrategy, Reason, Uncompressed, _ctx_default, check

BLOCK_LEN = 65280                    # bgzip's: an incompressible block stays under 65,536 bytes
MAX_MEMBER = 65536                   # BSIZE is 16 bits and holds the member's length - 1
EXTRA = b"BC\x02\x00\x00\x00"        # the subfield, BSIZE still 0
BSIZE_AT = 16                        # 10 fixed bytes, XLEN, SI1, SI2, SLEN
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member_with_bsize(member):
    """`member` (written with EXTRA as its whole extra field) with BSIZE = its length - 1."""
    n = len(member)
    if n > MAX_MEMBER:
        raise ValueError(f"BGZF member of {n} bytes: more than {MAX_MEMBER}; use a smaller block_len")
    if member[10:BSIZE_AT] != b"\x06\x00" + EXTRA[:4]:
        raise ValueError("not a member written with the BC subfield first")
    return member[:BSIZE_AT] + (n - 1).to_bytes(2, "little") + member[BSIZE_AT + 2:]


def _device_tuple(strategy):
    """The Lz77Huffman X when `strategy` is exactly MultiStrategy(X, Uncompressed.SINGLETON), what
    ndfl_deflate_bgzf writes; else None."""
    if isinstance(strategy, MultiStrategy) and len(strategy.substrategies) == 2:
        x, u = strategy.substrategies
        if isinstance(x, Lz77Huffman) and u is Uncompressed.SINGLETON:
            return x
    return None


def compress(data, block_len=BLOCK_LEN, strategy=None, context=None):
    """`data` as a BGZF file: one member per block_len bytes, then the 28-byte EOF member (empty input:
    the EOF member alone).  The default strategy takes the smaller of a FULL_DYNAMIC block and a stored one.
    ValueError when a member would be longer than 65,536 bytes."""
    from .streams import GzipMetadata
    data = bytes(data)
    if not 1 <= block_len <= 65536:
        raise ValueError("block_len: 1..65536")
    if strategy is None:
        strategy = MultiStrategy(Lz77Huffman.FULL_DYNAMIC, Uncompressed.SINGLETON)
    x = _device_tuple(strategy)
    if x is not None:
        return _ctx_default(context).deflate_bgzf(data, block_len, x)[0]
    blocks = [data[i:i + block_len] for i in range(0, len(data), block_len)]
    members = []
    if blocks:
        meta = GzipMetadata(operatingSystem="UNKNOWN", extraField=EXTRA)
        members = _ctx_default(context).deflate_members(blocks, _lib.FMT_GZIP, meta=meta, strategy=strategy)
    return b"".join(member_with_bsize(m) for m in members) + EOF


def decompress(data, context=None):
    """The bytes of a BGZF file.  DataFormatException on the first failing member's Reason; ValueError
    when the members do not cover all of `data` (trailing bytes, or a plain gzip file) or there is none."""
    ctx = _ctx_default(context)
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    need = ctx.inflate_bgzf_raw(ctypes.addressof(src), len(data), None, 0, 0)[0][4]
    out = ctypes.create_string_buffer(max(1, need))
    (code, sym, n, _, olen, consumed), _ = ctx.inflate_bgzf_raw(ctypes.addressof(src), len(data),
                                                               ctypes.addressof(out), need, 0)
    check(code, "ndfl_inflate_bgzf")
    if code:
        raise DataFormatException(Reason(code - 1), symbol=sym)
    if n == 0:
        raise ValueError("not a BGZF file: no member with a BC subfield at byte 0")
    if consumed != len(data):
        raise ValueError(f"BGZF members end at byte {consumed} of {len(data)}")
    return out.raw[:olen]
