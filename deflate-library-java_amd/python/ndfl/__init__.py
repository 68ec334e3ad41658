"""ndfl -- MI355X-native DEFLATE codec, host-side mirror of io.nayuki.deflate.

The classes here mirror the reference's public API (same names, argument meaning and error
behaviour) on top of the C ABI in include/ndfl.h.  All codec work happens in libndfl.so's HIP
kernels; this module only buffers bytes, writes container headers and raises exceptions.

    DeflaterOutputStream   D/DeflaterOutputStream.java
    InflaterInputStream    D/InflaterInputStream.java
    DataFormatException    D/DataFormatException.java (with Reason)
    GzipMetadata           D/GzipMetadata.java
    GzipOutputStream       D/GzipOutputStream.java
    GzipInputStream        D/GzipInputStream.java
    ZlibOutputStream/ZlibInputStream/ZlibMetadata   D/Zlib*.java
"""
import ctypes
import enum
import io
import sys

from . import _lib
from ._lib import IN_DEVICE, OUT_DEVICE, DICT_DEFERRED, IN_PADDED, IN_PAD_BYTES, IN_PARTIAL, NEED_INPUT, NO_END, STRATEGIES, NdflError, check, load, reason_name
from ._lib import FMT_RAW, FMT_ZLIB, FMT_GZIP, SUM_NONE, SUM_CRC32, SUM_ADLER32

__all__ = ["Context", "Reason", "DataFormatException", "Lz77Huffman", "Uncompressed", "MultiStrategy", "BinarySplit", "DeflaterOutputStream", "InflaterInputStream", "BitOutputStream",
           "GzipMetadata", "GzipOutputStream", "GzipInputStream", "ZlibMetadata", "ZlibOutputStream",
           "ZlibInputStream", "Strategy", "default_context", "compress", "decompress", "crc32_combine"]


class Reason(enum.Enum):
    """DataFormatException.Reason (D/DataFormatException.java:61-83), same ordinal order."""
    UNEXPECTED_END_OF_STREAM = 0
    RESERVED_BLOCK_TYPE = 1
    UNCOMPRESSED_BLOCK_LENGTH_MISMATCH = 2
    HUFFMAN_CODE_UNDER_FULL = 3
    HUFFMAN_CODE_OVER_FULL = 4
    NO_PREVIOUS_CODE_LENGTH_TO_COPY = 5
    CODE_LENGTH_CODE_OVER_FULL = 6
    END_OF_BLOCK_CODE_ZERO_LENGTH = 7
    RESERVED_LENGTH_SYMBOL = 8
    RESERVED_DISTANCE_SYMBOL = 9
    LENGTH_ENCOUNTERED_WITH_EMPTY_DISTANCE_CODE = 10
    COPY_FROM_BEFORE_DICTIONARY_START = 11
    HEADER_CHECKSUM_MISMATCH = 12
    UNSUPPORTED_COMPRESSION_METHOD = 13
    DECOMPRESSED_CHECKSUM_MISMATCH = 14
    DECOMPRESSED_SIZE_MISMATCH = 15
    GZIP_INVALID_MAGIC_NUMBER = 16
    GZIP_RESERVED_FLAGS_SET = 17
    GZIP_UNSUPPORTED_OPERATING_SYSTEM = 18


class DataFormatException(Exception):
    """Unchecked in the reference (extends RuntimeException, D/DataFormatException.java:15): it is
    not made sticky by InflaterInputStream and not caught by the CLIs."""

    def __init__(self, reason, msg=None, symbol=-1):
        self.reason = reason
        if msg is None:
            msg = load().ndfl_error_string(reason.value + 1).decode()
            # the reference names the reserved symbol: "Reserved run length symbol: " + sym,
            # "Reserved distance symbol: " + sym (D/decomp/Open.java:516, 550, 659, 674)
            if symbol >= 0 and reason in (Reason.RESERVED_LENGTH_SYMBOL, Reason.RESERVED_DISTANCE_SYMBOL):
                msg += f": {symbol}"
        super().__init__(msg)

    def getReason(self):
        return self.reason


class Strategy(enum.Enum):
    """Lz77Huffman presets (D/comp/Lz77Huffman.java:298-305) and Uncompressed."""
    LITERAL_STATIC = 0
    LITERAL_DYNAMIC = 1
    RLE_STATIC = 2
    RLE_DYNAMIC = 3
    FULL_STATIC = 4
    FULL_DYNAMIC = 5
    UNCOMPRESSED = 6


class Lz77Huffman:
    """The Lz77Huffman record (D/comp/Lz77Huffman.java:20-39): greedy longest-match LZ77 over
    distances [searchMinimumDistance, searchMaximumDistance] with runs in [searchMinimumRunLength,
    searchMaximumRunLength], then static or dynamic Huffman codes.  Validation as :28-38
    (ValueError = IllegalArgumentException).  Presets as class attributes (:298-305)."""

    def __init__(self, useDynamicHuffmanCodes, searchMinimumRunLength, searchMaximumRunLength,
                 searchMinimumDistance, searchMaximumDistance):
        p = (searchMinimumRunLength, searchMaximumRunLength, searchMinimumDistance, searchMaximumDistance)
        mnr, mxr, mnd, mxd = p
        if not (p == (0, 0, 0, 0) or (3 <= mnr <= mxr <= 258 and 1 <= mnd <= mxd <= 32768)):
            raise ValueError("Invalid minimum/maximum run-length/distance")
        self.useDynamicHuffmanCodes = bool(useDynamicHuffmanCodes)
        self.params = p

    def __eq__(self, other):
        return isinstance(other, Lz77Huffman) and (self.useDynamicHuffmanCodes, self.params) == \
            (other.useDynamicHuffmanCodes, other.params)

    def __hash__(self):
        return hash((self.useDynamicHuffmanCodes, self.params))

    def __repr__(self):
        return f"Lz77Huffman({self.useDynamicHuffmanCodes}, {', '.join(map(str, self.params))})"

    def decide(self, b, off, historyLen, dataLen):
        """Strategy.decide (D/comp/Lz77Huffman.java:42-59), encoded on the GPU (ndfl_decide)."""
        return self._decide(b, off, historyLen, dataLen)

    def _decide(self, b, off, historyLen, dataLen, context=None):
        from .plugin import library_decide
        return library_decide(self, b, off, historyLen, dataLen, context)


Lz77Huffman.LITERAL_STATIC = Lz77Huffman(False, 0, 0, 0, 0)
Lz77Huffman.LITERAL_DYNAMIC = Lz77Huffman(True, 0, 0, 0, 0)
Lz77Huffman.RLE_STATIC = Lz77Huffman(False, 3, 258, 1, 1)
Lz77Huffman.RLE_DYNAMIC = Lz77Huffman(True, 3, 258, 1, 1)
Lz77Huffman.FULL_STATIC = Lz77Huffman(False, 3, 258, 1, 32768)
Lz77Huffman.FULL_DYNAMIC = Lz77Huffman(True, 3, 258, 1, 32768)


class _UncompressedType:
    """Uncompressed.SINGLETON (D/comp/Uncompressed.java:14-54): stored blocks of <= 65535 bytes."""

    def __repr__(self):
        return "Uncompressed.SINGLETON"

    def decide(self, b, off, historyLen, dataLen):
        """Strategy.decide (D/comp/Uncompressed.java:22-51)."""
        return self._decide(b, off, historyLen, dataLen)

    def _decide(self, b, off, historyLen, dataLen, context=None):
        from .plugin import library_decide
        return library_decide(self, b, off, historyLen, dataLen, context)


class Uncompressed:
    SINGLETON = _UncompressedType()


class MultiStrategy:
    """MultiStrategy(strats...) (D/comp/MultiStrategy.java:19-57): per chunk and output bit position,
    the first substrategy giving the fewest bits.  Substrategies: any Strategy (the library's
    classes, or a user object with decide()); a flat list of at most 8 Lz77Huffman / Uncompressed
    runs batched on the GPU (ndfl_deflate_chunks_multi), anything else per chunk (ndfl.plugin)."""

    def __init__(self, *strats):
        if strats is None or any(s is None for s in strats):
            raise TypeError("strategy")
        if len(strats) == 0:
            raise ValueError("Empty list of strategies")
        for st in strats:
            if not (isinstance(st, Strategy) or hasattr(st, "decide")):
                raise TypeError(f"not a strategy: {st!r}")
        self.substrategies = tuple(strats)

    def decide(self, b, off, historyLen, dataLen):
        return self._decide(b, off, historyLen, dataLen)

    def _decide(self, b, off, historyLen, dataLen, context=None):
        from .plugin import library_decide
        return library_decide(self, b, off, historyLen, dataLen, context)


class BinarySplit:
    """BinarySplit(strat, minBlockLen) (D/comp/BinarySplit.java:15-82): halve each chunk recursively
    while both halves exceed minBlockLen, keeping a split when it takes fewer bits.  Over an
    Lz77Huffman the whole stream is batched on the GPU (ndfl_deflate_chunks_binsplit; many buffers in
    one launch: Context.deflate_batch, ndfl_deflate_batch_binsplit); over any other Strategy it runs per
    chunk (ndfl.plugin: ndfl_decide for the library's classes)."""

    def __init__(self, strat, minBlockLen):
        if strat is None:
            raise TypeError("strat")
        if minBlockLen < 1:
            raise ValueError("Non-positive minimum block length")
        self.substrategy = strat
        self.minimumBlockLength = int(minBlockLen)

    def decide(self, b, off, historyLen, dataLen):
        return self._decide(b, off, historyLen, dataLen)

    def _decide(self, b, off, historyLen, dataLen, context=None):
        from .plugin import library_decide
        return library_decide(self, b, off, historyLen, dataLen, context)


def _desc(st):
    d = _lib.StrategyDesc()
    if isinstance(st, _UncompressedType):
        d.kind = _lib.KIND_UNCOMPRESSED
    else:
        d.kind = _lib.KIND_LZ77
        d.dynamic = int(st.useDynamicHuffmanCodes)
        d.min_run, d.max_run, d.min_dist, d.max_dist = st.params
    return d


def _ptr(obj):
    """(address, keepalive) of bytes-like / torch tensor."""
    if hasattr(obj, "data_ptr"):
        return obj.data_ptr(), obj
    if isinstance(obj, (bytes, bytearray, memoryview)):
        b = bytes(obj)
        buf = ctypes.create_string_buffer(b, max(1, len(b)))
        return ctypes.addressof(buf), buf
    raise TypeError(type(obj))


class Context:
    """One device context (HIP stream + device scratch).  Not reentrant.

    Stream ordering: unless set_stream() named a stream, every call that touches device memory
    runs on torch's current stream of this device when torch has initialised the GPU (so a
    tensor a torch kernel is still producing, or a block the caching allocator reuses, is ordered
    like any torch op), else after the device's default stream (the C ABI's own rule,
    include/ndfl.h)."""

    def __init__(self, device=0):
        L = load()
        h = ctypes.c_void_p()
        check(L.ndfl_ctx_create(ctypes.byref(h), device, 0), "ndfl_ctx_create")
        self._h = h
        self.device = device
        self._explicit_stream = False
        self._bound = None

    def _order(self):
        """Bind torch's current stream (see the class docstring) before a device call."""
        if self._explicit_stream:
            return
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_initialized():
            return
        h = torch.cuda.current_stream(self.device).cuda_stream
        if h != self._bound:
            check(load().ndfl_ctx_set_stream(self._h, ctypes.c_void_p(h)))
            self._bound = h

    def close(self):
        if getattr(self, "_h", None):
            load().ndfl_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        """Run this context's calls on the caller's HIP stream (None / 0: the default rule)."""
        check(load().ndfl_ctx_set_stream(self._h, ctypes.c_void_p(stream_handle)))
        self._explicit_stream = bool(stream_handle)
        self._bound = stream_handle

    def last_kernel_ms(self):
        return load().ndfl_ctx_last_kernel_ms(self._h)

    def timings(self):
        """{'deflate', 'inflate_find', 'inflate_count', 'inflate_emit', 'inflate_span'} in ms, then the
        last decode's counts (include/ndfl.h, ndfl_ctx_timings)."""
        arr = (ctypes.c_double * 10)()
        load().ndfl_ctx_timings(self._h, arr, 10)
        keys = ["deflate", "inflate_find", "inflate_count", "inflate_emit", "inflate_span", "inflate_chains",
                "inflate_repairs", "inflate_candidates", "inflate_flat_chains", "inflate_pending_after_dev_rounds"]
        return dict(zip(keys, list(arr)))

    # -- raw C-ABI wrappers ------------------------------------------------------------------
    def deflate_chunks_raw(self, hist_addr, hist_len, hist_limit, data_addr, n, chunk_len, strategy, final,
                           start_bitpos, out_addr, out_cap, flags, crc=None):
        L = load()
        self._order()
        endbits = ctypes.c_uint64(0)
        crcv = ctypes.c_uint32(crc if crc is not None else 0)
        crcp = ctypes.byref(crcv) if crc is not None else None
        if isinstance(strategy, BinarySplit):
            d = _desc(strategy.substrategy)
            r = L.ndfl_deflate_chunks_binsplit(self._h, hist_addr, hist_len, hist_limit, data_addr, n, chunk_len,
                                               ctypes.byref(d), strategy.minimumBlockLength, int(final), start_bitpos,
                                               out_addr, out_cap, ctypes.byref(endbits), crcp, flags)
            check(r, "ndfl_deflate_chunks_binsplit")
        elif isinstance(strategy, (MultiStrategy, _UncompressedType)):
            subs = strategy.substrategies if isinstance(strategy, MultiStrategy) else (strategy,)
            arr = (_lib.StrategyDesc * len(subs))(*[_desc(x) for x in subs])
            r = L.ndfl_deflate_chunks_multi(self._h, hist_addr, hist_len, hist_limit, data_addr, n, chunk_len, arr,
                                            len(subs), int(final), start_bitpos, out_addr, out_cap,
                                            ctypes.byref(endbits), crcp, flags)
            check(r, "ndfl_deflate_chunks_multi")
        elif isinstance(strategy, Lz77Huffman):
            r = L.ndfl_deflate_chunks_lz77(self._h, hist_addr, hist_len, hist_limit, data_addr, n, chunk_len,
                                           int(strategy.useDynamicHuffmanCodes), *strategy.params, int(final),
                                           start_bitpos, out_addr, out_cap, ctypes.byref(endbits), crcp, flags)
            check(r, "ndfl_deflate_chunks_lz77")
        else:
            r = L.ndfl_deflate_chunks(self._h, hist_addr, hist_len, hist_limit, data_addr, n, chunk_len,
                                      _strategy_id(strategy), int(final), start_bitpos, out_addr, out_cap,
                                      ctypes.byref(endbits), crcp, flags)
            check(r, "ndfl_deflate_chunks")
        return endbits.value, (crcv.value if crc is not None else None)

    def deflate(self, data, strategy=Strategy.RLE_DYNAMIC, chunk_len=65536, hist_limit=32768, with_crc=False):
        """Whole-stream compress of host bytes (DeflaterOutputStream write-all + finish)."""
        data = bytes(data)
        L = load()
        cap = L.ndfl_deflate_bound(len(data), chunk_len) + 16
        out = ctypes.create_string_buffer(cap)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        endbits, crc = self.deflate_chunks_raw(None, 0, hist_limit, ctypes.addressof(src), len(data), chunk_len,
                                               strategy, True, 0, ctypes.addressof(out), cap, 0,
                                               crc=0 if with_crc else None)
        comp = out.raw[:(endbits + 7) // 8]
        return (comp, crc) if with_crc else comp

    def inflate_raw(self, in_addr, in_len, out_addr, out_cap, flags):
        """Returns (code, out_len, consumed_bits); code = 0 / reason+1 / <0 error."""
        L = load()
        self._order()
        olen = ctypes.c_uint64(0)
        bits = ctypes.c_uint64(0)
        r = L.ndfl_inflate(self._h, in_addr, in_len, out_addr, out_cap, ctypes.byref(olen), ctypes.byref(bits),
                           flags)
        return r, olen.value, bits.value

    def inflate(self, data, out_cap=None):
        """Decode a whole raw DEFLATE stream held in host memory.  Returns (reason|None, bytes, bits)."""
        data = bytes(data)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        cap = out_cap if out_cap is not None else 4 * len(data) + 65536
        while True:
            out = ctypes.create_string_buffer(max(1, cap))
            r, olen, bits = self.inflate_raw(ctypes.addressof(src), len(data), ctypes.addressof(out), cap, 0)
            if r == _lib.E_CAPACITY and out_cap is None:
                cap = olen + 16
                continue
            check(r, "ndfl_inflate")
            reason = None if r == 0 else Reason(r - 1)
            return reason, out.raw[:olen], bits

    def error_symbol(self):
        """ndfl_ctx_error_symbol: the reserved symbol behind the last decode's RESERVED_LENGTH_SYMBOL /
        RESERVED_DISTANCE_SYMBOL (286/287, 30/31), or -1."""
        return load().ndfl_ctx_error_symbol(self._h)

    def data_format_error(self, code):
        """The DataFormatException of a decode that returned Reason+1 `code`, with the reference's
        message (the symbol appended where D/decomp/Open.java appends it)."""
        return DataFormatException(Reason(code - 1), symbol=self.error_symbol())

    def data_format_error_for(self, result):
        """The DataFormatException of one stream of a batch: `result` is its (code, error_symbol, out_len,
        consumed_bits) from inflate_batch_raw, code a Reason+1; the message names the stream's own
        reserved symbol."""
        return DataFormatException(Reason(result[0] - 1), symbol=result[1])

    def _batch_raw(self, name, item_type, result_type, fields, in_addr, in_size, out_addr, out_size, items, *rest):
        """One batch entry point `name`: `items` marshalled as item_type, `rest` = its arguments after n
        (one given as a function is evaluated once the items are marshalled).  Returns the `fields` of
        every stream's result_type as a tuple."""
        self._order()
        n = len(items)
        arr = (item_type * max(1, n))(*[item_type(*map(int, it)) for it in items])
        res = (result_type * max(1, n))()
        rest = [a() if callable(a) else a for a in rest]
        check(getattr(load(), name)(self._h, in_addr, in_size, out_addr, out_size, arr, res, n, *rest), name)
        return [tuple(getattr(r, f) for f in fields) for r in res[:n]]

    def _inflate_packed(self, raw, name, streams, more, out_caps):
        """inflate_batch / inflate_members: the streams packed back to back and run through `raw` (entry
        point `name`); without out_caps the streams that overflowed are run again with the size they
        reported.  more[i]: stream i's item fields after out_cap.  Returns (reason|None, bytes) followed
        by the result's fields after out_len, per stream."""
        n = len(streams)
        done = [None] * n
        todo = list(range(n))
        caps = [4 * len(s) + 65536 for s in streams] if out_caps is None else [int(c) for c in out_caps]
        while todo:
            packed = b"".join(streams[i] for i in todo)
            src = ctypes.create_string_buffer(packed, max(1, len(packed)))
            items, in_off, out_off = [], 0, 0
            for i in todo:
                items.append((in_off, len(streams[i]), out_off, caps[i]) + tuple(more[i]))
                in_off += len(streams[i])
                out_off += caps[i]
            out = ctypes.create_string_buffer(max(1, out_off))
            res = raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items, 0)
            again = []
            for i, it, r in zip(todo, items, res):
                code, olen = r[0], r[2]
                if code == _lib.E_CAPACITY and out_caps is None:
                    caps[i] = olen
                    again.append(i)
                    continue
                check(code, name)
                done[i] = (None if code == 0 else Reason(code - 1),
                           ctypes.string_at(ctypes.addressof(out) + it[2], min(olen, it[3]))) + tuple(r[3:])
            todo = again
        return done

    def inflate_batch_raw(self, in_addr, in_size, out_addr, out_size, items, flags):
        """ndfl_inflate_batch: `items` is a sequence of (in_off, in_len, out_off, out_cap).  Returns one
        (code, error_symbol, out_len, consumed_bits) per stream; code = 0 / Reason+1 / E_CAPACITY."""
        return self._batch_raw("ndfl_inflate_batch", _lib.BatchItem, _lib.BatchResult,
                               ("status", "error_symbol", "out_len", "consumed_bits"),
                               in_addr, in_size, out_addr, out_size, items, flags)

    def inflate_batch(self, streams, out_caps=None):
        """Decode many independent raw DEFLATE streams (host bytes) in one call.  Returns one
        (reason|None, bytes, consumed_bits) per stream.  With out_caps (one capacity per stream) a stream
        that needs more raises NdflError(E_CAPACITY); without, every region is 4 * len + 65536 bytes and
        only the streams that overflowed are run again, with the size they reported."""
        streams = [bytes(s) for s in streams]
        return self._inflate_packed(self.inflate_batch_raw, "ndfl_inflate_batch", streams, [()] * len(streams), out_caps)

    def inflate_members_raw(self, in_addr, in_size, out_addr, out_size, items, flags):
        """ndfl_inflate_members: `items` is a sequence of (in_off, in_len, out_off, out_cap, format, sum)
        with format a FMT_* and sum a SUM_* (read for FMT_RAW only).  Returns one (code, error_symbol,
        out_len, consumed_bits, checksum, header_len) per stream; code = 0 / Reason+1 / E_CAPACITY /
        E_ARG (a zlib header whose CINFO the reference's ZlibMetadata refuses)."""
        return self._batch_raw("ndfl_inflate_members", _lib.MemberItem, _lib.MemberResult,
                               ("status", "error_symbol", "out_len", "consumed_bits", "checksum", "header_len"),
                               in_addr, in_size, out_addr, out_size, items, flags)

    def inflate_members(self, streams, format, sum=None, out_caps=None):
        """Decode many zlib members (FMT_ZLIB), gzip members (FMT_GZIP: one member per stream) or raw
        DEFLATE streams (FMT_RAW, with `sum` = SUM_CRC32 / SUM_ADLER32 / None) held in host bytes, in one
        call, checksums verified on the GPU.  `format` is one FMT_* for all streams or one per stream.
        Returns one (reason|None, bytes, consumed_bits, checksum, header_len) per stream; consumed_bits / 8
        is a container member's whole length.  Capacities as in inflate_batch: with out_caps a stream that
        needs more raises NdflError(E_CAPACITY); without, every region is 4 * len + 65536 bytes and only
        the streams that overflowed are run again, with the size they reported."""
        streams = [bytes(s) for s in streams]
        fmts = [int(format)] * len(streams) if isinstance(format, int) else [int(f) for f in format]
        kind = _lib.SUM_NONE if sum is None else int(sum)
        return self._inflate_packed(self.inflate_members_raw, "ndfl_inflate_members", streams,
                                    [(f, kind) for f in fmts], out_caps)

    def inflate_bgzf_raw(self, in_addr, in_len, out_addr, out_cap, flags, table_cap=0):
        """ndfl_inflate_bgzf: a whole blocked gzip (BGZF) file, its members found on the device.  Returns
        ((code, error_symbol, n_members, bad_member, out_len, consumed_bytes), table) with code = 0 /
        Reason+1 of the first failing member / E_CAPACITY (out_len: the bytes required) and table the first
        min(table_cap, n_members + 1) (in_off, out_off) entries; other negative codes raise."""
        self._order()
        res = _lib.BgzfResult()
        tab = (_lib.BgzfMember * max(1, table_cap))()
        r = load().ndfl_inflate_bgzf(self._h, in_addr, in_len, out_addr, out_cap, ctypes.byref(res),
                                     tab if table_cap else None, table_cap, flags)
        if r != _lib.E_CAPACITY:
            check(r, "ndfl_inflate_bgzf")
        n = min(table_cap, res.n_members + 1)
        return ((res.status, res.error_symbol, res.n_members, res.bad_member, res.out_len, res.consumed_bytes),
                [(t.in_off, t.out_off) for t in tab[:n]])

    def inflate_bgzf(self, data, out_cap=None):
        """Decode a blocked gzip (BGZF) file held in host bytes in one call.  Returns (reason|None, bytes,
        consumed_bytes, n_members): on a Reason the bytes decoded AND stored before the first failing member's
        error (a member stores no more than its ISIZE: its region ends where the next one's begins),
        consumed_bytes = the offset just past the last member found (bytes after it are ignored).  Without
        out_cap a sizing call (which trusts the members' ISIZE fields) comes first and the decode runs at
        the exact size; with it a file that needs more raises NdflError(E_CAPACITY)."""
        data = bytes(data)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        if out_cap is None:
            out_cap = self.inflate_bgzf_raw(ctypes.addressof(src), len(data), None, 0, 0)[0][4]
        out = ctypes.create_string_buffer(max(1, out_cap))
        (code, sym, n, bad, olen, consumed), _ = self.inflate_bgzf_raw(ctypes.addressof(src), len(data),
                                                                      ctypes.addressof(out), out_cap, 0)
        check(code, "ndfl_inflate_bgzf")
        if code:
            # the failing member's region ends at the next table entry
            table = self.inflate_bgzf_raw(ctypes.addressof(src), len(data), None, 0, 0, table_cap=bad + 2)[1]
            olen = min(olen, table[bad + 1][1])
        return (None if code == 0 else Reason(code - 1)), out.raw[:olen], consumed, n

    def bgzf_index(self, data):
        """The member table of a blocked gzip (BGZF) file in host bytes, without decoding it: one (in_off,
        out_off) per member and a last entry (consumed_bytes, total output) -- from the members' BSIZE and
        ISIZE fields, which it trusts."""
        data = bytes(data)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        n = self.inflate_bgzf_raw(ctypes.addressof(src), len(data), None, 0, 0)[0][2]
        return self.inflate_bgzf_raw(ctypes.addressof(src), len(data), None, 0, 0, table_cap=n + 1)[1]

    def deflate_bgzf_raw(self, in_addr, in_len, out_addr, out_cap, strategy_tuple, block_len, flags, table_cap=0):
        """ndfl_deflate_bgzf: `in_len` bytes as a blocked gzip (BGZF) file of one member per block_len bytes
        and the closing empty member, each member MultiStrategy(Lz77Huffman(*strategy_tuple),
        Uncompressed.SINGLETON) of its block; strategy_tuple = (dynamic, min_run, max_run, min_dist, max_dist).
        Returns ((code, n_members, bad_member, n_stored, out_len), table) with code = 0 / E_CAPACITY (out_len:
        the bytes required; out_addr = None, out_cap = 0 sizes the file) / E_UNSUPPORTED (a member above 65,536
        bytes: bad_member; or block_len above 65536: all else 0) and table the first min(table_cap, n_members
        + 1) (file offset, data offset) entries; other negative codes raise."""
        self._order()
        res = _lib.BgzfWriteResult()
        tab = (_lib.BgzfMember * max(1, table_cap))()
        dynamic, min_run, max_run, min_dist, max_dist = strategy_tuple
        r = load().ndfl_deflate_bgzf(self._h, in_addr, in_len, out_addr, out_cap, ctypes.byref(res),
                                     tab if table_cap else None, table_cap, int(dynamic), min_run, max_run, min_dist,
                                     max_dist, block_len, flags)
        if r not in (_lib.E_CAPACITY, _lib.E_UNSUPPORTED):
            check(r, "ndfl_deflate_bgzf")
        n = min(table_cap, res.n_members + 1) if res.n_members else 0
        return (r, res.n_members, res.bad_member, res.n_stored, res.out_len), [(t.in_off, t.out_off) for t in tab[:n]]

    def deflate_bgzf(self, data, block_len=65280, strategy=Lz77Huffman.FULL_DYNAMIC):
        """`data` (host bytes) as a blocked gzip (BGZF) file in one call: (bytes, table), table = one (file
        offset, data offset) per member, the closing empty one included, and a last entry (file length,
        len(data)) -- what bgzf_index gives for the file.  `strategy` is the Lz77Huffman of
        MultiStrategy(strategy, Uncompressed.SINGLETON).  ValueError when
        a member would exceed 65,536 bytes (an incompressible block with block_len above 65505)."""
        if not isinstance(strategy, Lz77Huffman):
            raise TypeError("strategy: an Lz77Huffman")
        tup = (strategy.useDynamicHuffmanCodes,) + tuple(strategy.params)
        data = bytes(data)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        cap = load().ndfl_bgzf_bound(len(data), block_len) if 1 <= block_len <= 65536 else 0
        out = ctypes.create_string_buffer(max(1, cap))
        (code, n, bad, _, olen), table = self.deflate_bgzf_raw(ctypes.addressof(src), len(data), ctypes.addressof(out), cap,
                                                               tup, block_len, 0, table_cap=len(data) // max(1, block_len) + 3)
        if code == _lib.E_UNSUPPORTED and n:
            raise ValueError(f"BGZF member {bad} of more than 65536 bytes; use a smaller block_len")
        check(code, "ndfl_deflate_bgzf")
        return out.raw[:olen], table

    _DEFLATE_RESULT = ("status", "checksum", "out_len", "end_bits")

    def deflate_batch_raw(self, in_addr, in_size, out_addr, out_size, items, strategy, chunk_len, hist_limit, flags):
        """ndfl_deflate_batch: `items` is a sequence of (in_off, in_len, out_off, out_cap, format, sum):
        item i's raw bytes, the region of its compressed member, its container (FMT_*) and, for FMT_RAW,
        the checksum wanted (SUM_*).  Returns one (status, checksum, out_len, end_bits) per stream; status
        = 0 / E_CAPACITY."""
        def sid():
            v = _strategy_id(strategy)
            if not isinstance(v, int):               # (strategy objects: only the presets are batched)
                raise NdflError(_lib.E_UNSUPPORTED, "ndfl_deflate_batch")
            return v
        return self._batch_raw("ndfl_deflate_batch", _lib.MemberItem, _lib.DeflateResult, self._DEFLATE_RESULT,
                               in_addr, in_size, out_addr, out_size, items, sid, chunk_len, hist_limit, flags)

    def deflate_batch_lz77_raw(self, in_addr, in_size, out_addr, out_size, items, dynamic, min_run, max_run, min_dist,
                               max_dist, chunk_len, hist_limit, flags):
        """ndfl_deflate_batch_lz77: deflate_batch_raw with Lz77Huffman(dynamic, min_run, max_run, min_dist,
        max_dist) as the strategy; the same items and the same (status, checksum, out_len, end_bits) per
        stream."""
        return self._batch_raw("ndfl_deflate_batch_lz77", _lib.MemberItem, _lib.DeflateResult, self._DEFLATE_RESULT,
                               in_addr, in_size, out_addr, out_size, items, int(dynamic), min_run, max_run, min_dist,
                               max_dist, chunk_len, hist_limit, flags)

    def deflate_batch_chunked_raw(self, in_addr, in_size, out_addr, out_size, items, dynamic, min_run, max_run, min_dist,
                                  max_dist, chunk_len, hist_limit, flags):
        """ndfl_deflate_batch_chunked: deflate_batch_lz77_raw with one workgroup per chunk instead of one wave
        per stream (medium buffers); every valid tuple, the literal-only and the RLE form included; the
        same items and the same (status, checksum, out_len, end_bits) per stream."""
        return self._batch_raw("ndfl_deflate_batch_chunked", _lib.MemberItem, _lib.DeflateResult, self._DEFLATE_RESULT,
                               in_addr, in_size, out_addr, out_size, items, int(dynamic), min_run, max_run, min_dist,
                               max_dist, chunk_len, hist_limit, flags)

    def deflate_batch_multi_raw(self, in_addr, in_size, out_addr, out_size, items, subs, chunk_len, hist_limit, flags):
        """ndfl_deflate_batch_multi: deflate_batch_raw with MultiStrategy(subs...) as the strategy, `subs` a
        sequence of Lz77Huffman / Uncompressed.SINGLETON (or ready-made _lib.StrategyDesc records); the
        same items and the same (status, checksum, out_len, end_bits) per stream."""
        descs = [x if isinstance(x, _lib.StrategyDesc) else _desc(x) for x in subs]
        arr = (_lib.StrategyDesc * max(1, len(descs)))(*descs)
        return self._batch_raw("ndfl_deflate_batch_multi", _lib.MemberItem, _lib.DeflateResult, self._DEFLATE_RESULT,
                               in_addr, in_size, out_addr, out_size, items, arr, len(descs), chunk_len, hist_limit,
                               flags)

    def deflate_batch_binsplit_raw(self, in_addr, in_size, out_addr, out_size, items, sub, min_block_len, chunk_len,
                                   hist_limit, flags):
        """ndfl_deflate_batch_binsplit: deflate_batch_raw with BinarySplit(sub, min_block_len) as the strategy,
        `sub` an Lz77Huffman (or a ready-made _lib.StrategyDesc record, or None for a null pointer); the
        same items and the same (status, checksum, out_len, end_bits) per stream."""
        d = sub if sub is None or isinstance(sub, _lib.StrategyDesc) else _desc(sub)
        return self._batch_raw("ndfl_deflate_batch_binsplit", _lib.MemberItem, _lib.DeflateResult, self._DEFLATE_RESULT,
                               in_addr, in_size, out_addr, out_size, items, None if d is None else ctypes.byref(d),
                               min_block_len, chunk_len, hist_limit, flags)

    @staticmethod
    def _batch_subs(strategy):
        """The substrategies ndfl_deflate_batch_multi takes for `strategy` (Uncompressed.SINGLETON, or a
        MultiStrategy over a flat list of at most 8 Lz77Huffman / Uncompressed), None for the strategies
        of the other two batch calls; any other MultiStrategy is not batched."""
        if isinstance(strategy, _UncompressedType):
            return (strategy,)
        if not isinstance(strategy, MultiStrategy):
            return None
        subs = strategy.substrategies
        if len(subs) > 8 or not all(isinstance(x, (Lz77Huffman, _UncompressedType)) for x in subs):
            raise NdflError(_lib.E_UNSUPPORTED, "ndfl_deflate_batch_multi")
        return subs

    @staticmethod
    def _chunks_tuple(strategy):
        """The Lz77Huffman that path="chunks" runs for `strategy` (an Lz77Huffman, or a preset's name or
        id); Uncompressed, MultiStrategy and BinarySplit are not encoded by chunk workgroups."""
        s = _strategy_id(strategy)
        if isinstance(s, Lz77Huffman):
            return s
        if isinstance(s, int) and Strategy.LITERAL_STATIC.value <= s <= Strategy.FULL_DYNAMIC.value:
            return getattr(Lz77Huffman, Strategy(s).name)
        raise NdflError(_lib.E_UNSUPPORTED, "ndfl_deflate_batch_chunked")

    def _deflate_packed(self, buffers, fmt, kind, headers, strategy, chunk_len, hist_limit, path="wave"):
        """One batch over host buffers: each region is its header's bytes (the caller's part of a
        container) followed by room for ndfl_deflate_bound(len) bytes and the trailer.  Returns one
        (bytes from the header on, end_bits, checksum) per buffer."""
        L = load()
        if path not in ("wave", "chunks"):
            raise ValueError('path: "wave" or "chunks"')
        buffers = [bytes(b) for b in buffers]
        if path == "chunks":
            strategy = self._chunks_tuple(strategy)
        subs = self._batch_subs(strategy)
        split = isinstance(strategy, BinarySplit)
        if split and not isinstance(strategy.substrategy, Lz77Huffman):
            raise NdflError(_lib.E_UNSUPPORTED, "ndfl_deflate_batch_binsplit")
        packed = b"".join(buffers)
        src = ctypes.create_string_buffer(packed, max(1, len(packed)))
        items, regions, in_off, out_off = [], [], 0, 0
        for b, h in zip(buffers, headers):
            # (BinarySplit: its Lz77Huffman's size, a split is taken only when it is shorter)
            cap = L.ndfl_deflate_bound(len(b), chunk_len) * (2 if isinstance(strategy, Lz77Huffman) or subs or split
                                                             else 1) + 8
            if subs:
                # the larger of that and the stored size (5 bytes a block, two blocks for a 65,536-byte
                # chunk), and a byte per chunk for the bits the choice depends on the bit position by
                chunks = max(1, -(-len(b) // max(1, chunk_len)))
                cap = max(cap, len(b) + 5 * chunks * (2 if chunk_len > 65535 else 1) + 8) + chunks
            items.append((in_off, len(b), out_off + len(h), cap, fmt, kind))
            regions.append(out_off)
            in_off += len(b)
            out_off += len(h) + cap
        out = ctypes.create_string_buffer(max(1, out_off))
        for at, h in zip(regions, headers):
            ctypes.memmove(ctypes.addressof(out) + at, bytes(h), len(h))
        if path == "chunks":
            res = self.deflate_batch_chunked_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items,
                                                 strategy.useDynamicHuffmanCodes, *strategy.params, chunk_len, hist_limit,
                                                 0)
        elif subs:
            res = self.deflate_batch_multi_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items,
                                               subs, chunk_len, hist_limit, 0)
        elif split:
            res = self.deflate_batch_binsplit_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items,
                                                  strategy.substrategy, strategy.minimumBlockLength, chunk_len, hist_limit,
                                                  0)
        elif isinstance(strategy, Lz77Huffman):      # (a preset's name or id keeps ndfl_deflate_batch)
            res = self.deflate_batch_lz77_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items,
                                              strategy.useDynamicHuffmanCodes, *strategy.params, chunk_len, hist_limit, 0)
        else:
            res = self.deflate_batch_raw(ctypes.addressof(src), len(packed), ctypes.addressof(out), out_off, items,
                                         strategy, chunk_len, hist_limit, 0)
        done = []
        for at, h, r in zip(regions, headers, res):
            status, checksum, olen, end_bits = r
            check(status, "ndfl_deflate_batch")
            done.append((ctypes.string_at(ctypes.addressof(out) + at, len(h) + olen), end_bits, checksum))
        return done

    def deflate_batch(self, buffers, strategy=Strategy.RLE_DYNAMIC, chunk_len=65536, hist_limit=32768, sum=None,
                      path="wave"):
        """Compress many independent host buffers in one call, each as deflate() compresses it alone
        (RLE_* / LITERAL_* presets by name or id through ndfl_deflate_batch; an Lz77Huffman instance, FULL_*
        among them, through ndfl_deflate_batch_lz77; Uncompressed.SINGLETON, or a MultiStrategy over a flat
        list of at most 8 Lz77Huffman / Uncompressed, through ndfl_deflate_batch_multi; a BinarySplit over an
        Lz77Huffman through ndfl_deflate_batch_binsplit; any other MultiStrategy or BinarySplit raises
        NdflError(E_UNSUPPORTED)).  Returns one (bytes, end_bits, checksum) per buffer; checksum is
        the buffer's CRC-32 / Adler-32 with sum = SUM_CRC32 / SUM_ADLER32, else 0.
        path="wave" (the default) is one wave per buffer, for many small buffers; path="chunks" sends a
        preset's name or id or an Lz77Huffman through ndfl_deflate_batch_chunked, one workgroup per chunk,
        for buffers of one to a few dozen chunks -- the same bytes -- and raises NdflError(E_UNSUPPORTED)
        for Uncompressed, MultiStrategy and BinarySplit."""
        buffers = list(buffers)
        kind = _lib.SUM_NONE if sum is None else int(sum)
        return self._deflate_packed(buffers, _lib.FMT_RAW, kind, [b""] * len(buffers), strategy, chunk_len, hist_limit,
                                    path)

    def deflate_members(self, buffers, format, meta=None, strategy=Strategy.RLE_DYNAMIC, chunk_len=65536,
                        hist_limit=32768, path="wave"):
        """Compress many independent host buffers into complete zlib (FMT_ZLIB) or gzip (FMT_GZIP)
        members in one call: what ZlibOutputStream / GzipOutputStream write for each buffer alone.  The
        header is `meta`'s (a ZlibMetadata / GzipMetadata; default ZlibMetadata.DEFAULT / GzipMetadata()),
        the trailer the kernel's; `strategy` as for deflate_batch (BinarySplit(Lz77Huffman, minBlockLen) through
        ndfl_deflate_batch_binsplit among them) and `path` as for deflate_batch.  Returns one bytes object per
        buffer."""
        from .streams import GzipMetadata, ZlibMetadata
        buffers = list(buffers)
        fmt = int(format)
        if fmt == _lib.FMT_ZLIB:
            header = bytes((meta if meta is not None else ZlibMetadata.DEFAULT).header_bytes())
        elif fmt == _lib.FMT_GZIP:
            meta = meta if meta is not None else GzipMetadata()
            header = bytes(meta.header_bytes())
            if meta.hasHeaderCrc:
                header += (self.crc32(header) & 0xFFFF).to_bytes(2, "little")
        else:
            raise ValueError("format: FMT_ZLIB or FMT_GZIP")
        done = self._deflate_packed(buffers, fmt, _lib.SUM_NONE, [header] * len(buffers), strategy, chunk_len,
                                    hist_limit, path)
        return [d[0] for d in done]

    def inflate_range_raw(self, in_addr, in_len, start_bit, end_bit, out_addr, dict_len, out_cap, flags):
        """ndfl_inflate_range: decode bits [start_bit, end_bit) into out_addr + dict_len, with the
        dict_len bytes at out_addr as the window.  Returns (code, out_len, consumed_bits)."""
        L = load()
        self._order()
        olen = ctypes.c_uint64(0)
        bits = ctypes.c_uint64(0)
        r = L.ndfl_inflate_range(self._h, in_addr, in_len, start_bit, NO_END if end_bit is None else end_bit,
                                 out_addr, dict_len, out_cap, ctypes.byref(olen), ctypes.byref(bits), flags)
        return r, olen.value, bits.value

    def inflate_sync_raw(self, in_addr, in_len, from_bit, window_bits, flags):
        """ndfl_inflate_sync: first confirmed block boundary at or past from_bit (None: none)."""
        self._order()
        v = ctypes.c_uint64(0)
        check(load().ndfl_inflate_sync(self._h, in_addr, in_len, from_bit, window_bits, ctypes.byref(v), flags),
              "ndfl_inflate_sync")
        return None if v.value == NO_END else v.value

    def inflate_headers_raw(self, in_addr, in_len, flags, survivors=False):
        """ndfl_inflate_headers (diagnostics): the decoder's chain starts, sorted; with survivors=True
        also the finder's survivors.  Returns (headers, stats[, survivors])."""
        L = load()
        self._order()
        n = ctypes.c_uint64(0)
        st = (ctypes.c_uint64 * 4)()
        check(L.ndfl_inflate_headers(self._h, in_addr, in_len, flags, None, 0, ctypes.byref(n), None, 0, st),
              "ndfl_inflate_headers")
        hs = (ctypes.c_uint64 * max(1, n.value))()
        ns = min(st[0], 2 * in_len + 65536) if survivors else 0
        sv = (ctypes.c_uint64 * max(1, ns))()
        check(L.ndfl_inflate_headers(self._h, in_addr, in_len, flags, hs, n.value, ctypes.byref(n),
                                     sv if ns else None, ns, st), "ndfl_inflate_headers")
        res = (list(hs[:n.value]), list(st))
        return res + (list(sv[:min(ns, st[0])]),) if survivors else res

    def inflate_headers(self, data, survivors=False):
        """inflate_headers_raw over a stream in host memory."""
        data = bytes(data)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        return self.inflate_headers_raw(ctypes.addressof(src), len(data), 0, survivors)

    def inflate_resolve(self):
        """Finish a DICT_DEFERRED range decode once the window is written; returns re-emitted chains."""
        self._order()
        n = ctypes.c_uint64(0)
        check(load().ndfl_inflate_resolve(self._h, ctypes.byref(n)), "ndfl_inflate_resolve")
        return n.value

    def inflate_tail_raw(self, tail_len, dst_addr):
        """ndfl_inflate_tail: the last tail_len output bytes of the pending DICT_DEFERRED decode (its
        window written) into device memory at dst_addr; False if a reference chain is too long
        (NDFL_E_UNSUPPORTED: resolve first)."""
        self._order()
        r = load().ndfl_inflate_tail(self._h, tail_len, ctypes.c_void_p(dst_addr))
        if r == _lib.E_UNSUPPORTED:
            return False
        check(r, "ndfl_inflate_tail")
        return True

    def inflate_tail_map_raw(self, tail_len, dst_addr):
        """ndfl_inflate_tail_map: the last tail_len output bytes of the pending DICT_DEFERRED decode
        as a map of its window (u32 per byte at dst_addr, device memory: window index, or
        TAIL_LITERAL | value); False if a reference chain is too long (NDFL_E_UNSUPPORTED)."""
        self._order()
        r = load().ndfl_inflate_tail_map(self._h, tail_len, ctypes.c_void_p(dst_addr))
        if r == _lib.E_UNSUPPORTED:
            return False
        check(r, "ndfl_inflate_tail_map")
        return True

    def bits_shift_raw(self, in_addr, nbits, shift, out_addr, out_cap):
        """ndfl_bits_shift on device buffers: in's first nbits bits placed at bit `shift` of out."""
        self._order()
        check(load().ndfl_bits_shift(self._h, in_addr, nbits, shift, out_addr, out_cap, IN_DEVICE | OUT_DEVICE),
              "ndfl_bits_shift")

    def crc32(self, data, crc=0, flags=0):
        self._order()
        addr, keep = _ptr(data)
        n = data.numel() * data.element_size() if hasattr(data, "numel") else len(data)
        v = ctypes.c_uint32(crc)
        check(load().ndfl_crc32(self._h, ctypes.byref(v), addr, n, flags), "ndfl_crc32")
        return v.value


    def adler32(self, data, adler=1, flags=0):
        self._order()
        addr, keep = _ptr(data)
        n = data.numel() * data.element_size() if hasattr(data, "numel") else len(data)
        v = ctypes.c_uint32(adler)
        check(load().ndfl_adler32(self._h, ctypes.byref(v), addr, n, flags), "ndfl_adler32")
        return v.value


def _ctx_default(context):
    return context if context is not None else default_context()


def _batchable(s):
    """Strategies the batched GPU calls take whole (ndfl_deflate_chunks / _lz77 / _multi /
    _binsplit); others go chunk by chunk through the plugin API."""
    if isinstance(s, (Strategy, str, int, Lz77Huffman, _UncompressedType)):
        return True
    if isinstance(s, MultiStrategy):
        return len(s.substrategies) <= 8 and all(isinstance(x, (Lz77Huffman, _UncompressedType))
                                                 for x in s.substrategies)
    if isinstance(s, BinarySplit):
        return isinstance(s.substrategy, Lz77Huffman)
    return False


def _strategy_id(s):
    if isinstance(s, (Lz77Huffman, MultiStrategy, _UncompressedType, BinarySplit)):
        return s
    if isinstance(s, Strategy):
        return s.value
    if isinstance(s, str):
        return STRATEGIES[s]
    return int(s)


def crc32_combine(a, b, len_b):
    return load().ndfl_crc32_combine(a, b, len_b)


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def compress(data, strategy=Strategy.RLE_DYNAMIC):
    return default_context().deflate(data, strategy)


def decompress(data):
    ctx = default_context()
    reason, out, _ = ctx.inflate(data)
    if reason is not None:
        raise ctx.data_format_error(reason.value + 1)
    return out


from .streams import (DeflaterOutputStream, InflaterInputStream, GzipMetadata, GzipOutputStream,  # noqa: E402
                      GzipInputStream, ZlibMetadata, ZlibOutputStream, ZlibInputStream)
from .plugin import BitOutputStream  # noqa: E402
from . import bgzf  # noqa: E402
