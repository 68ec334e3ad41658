#!/usr/bin/env python3
"""Many independent raw DEFLATE streams: one ndfl_inflate call per stream (--mode loop) against one
ndfl_inflate_batch call (--mode batch).  Not bench.py: this measures the batch entry points only.

Container members and checksums (--format zlib | gzip | raw-crc): one ndfl_inflate_members call
(--mode members: header, decode, checksum and trailer check in one launch) against what a caller had
to do before it (--mode batch+sum): one ndfl_inflate_batch call on the DEFLATE data -- the header
lengths handed to it for nothing -- and then one ndfl_adler32 (zlib) or ndfl_crc32 (gzip, raw-crc)
call per stream on the device-resident output.  The members are the same streams in a 2-byte zlib
or 10-byte gzip header and their trailer.  --mode takes a comma-separated list (the streams of a
shape are made once).

Inputs are seeded word-salad text (as tests/test_gpu_inflate.py::test_zlib_streams), compressed with
Python's zlib, raw (wbits=-15), in three shapes: 65,536 x 512 B, 4,096 x 4 KiB, 256 x 1 MiB.  Inputs
and outputs are device-resident; every stream starts 16-byte aligned and is followed by
NDFL_IN_PAD_BYTES zero bytes, so the loop decodes in place (NDFL_IN_PADDED) -- its best case -- and
the batch reads the same buffer.  Timing: wall clock around the calls (both are complete when they
return), median of --reps after --warmup, one JSON line per shape.  The first pass checks every
output byte against the original data.

--mode loop needs only ndfl_inflate, so it also runs on a build without the batch entry point
(NDFL_LIB_PATH selects the library): that is the baseline.  Likewise --mode batch+sum runs on a build
without ndfl_inflate_members.

The encoder's side (--mode deflate | deflate-loop, --data text | runs; see deflate_modes): one
ndfl_deflate_batch call against one ndfl_deflate_chunks call per buffer, RLE_DYNAMIC with the CRC-32
of each buffer, on the same three shapes; the lines are "bench": "batch_deflate".  With the LZ77 search
(--mode deflate-lz | deflate-lz-loop): one ndfl_deflate_batch_lz77 call against one
ndfl_deflate_chunks_lz77 call per buffer, FULL_DYNAMIC, everything else the same; the lines are "bench":
"batch_deflate_lz".  The four modes may share one run (--mode deflate,deflate-lz: both batch kernels on
the same buffers, their kernel times and compressed sizes side by side).  With the per-chunk choice of
block (--mode deflate-multi | deflate-multi-loop): one ndfl_deflate_batch_multi call against one
ndfl_deflate_chunks_multi call per buffer, MultiStrategy(Uncompressed, FULL_STATIC, FULL_DYNAMIC); the
lines are "bench": "batch_deflate_multi" (--mode deflate-lz,deflate-multi: what sizing two more
candidates costs, and what it saves, on the same buffers).  With split blocks (--mode deflate-binsplit |
deflate-binsplit-loop): one ndfl_deflate_batch_binsplit call against one ndfl_deflate_chunks_binsplit call
per buffer, BinarySplit(FULL_DYNAMIC, 256); the lines are "bench": "batch_deflate_binsplit".  The loop's
call refuses halvings of an odd length, so the comparison needs buffer sizes that are powers of two with
chunk_len equal to the buffer size (65,536 for the 1 MiB shape: 16 full chunks); these two modes, and
deflate-lz next to them in one run, use that chunk_len.  512-byte buffers are too short to split at 256
(one search per stream); --data mixed (a quarter each of digits, the text, random bytes and 16-valued
bytes) gives the larger ones something to split.  Through the chunk encoders (--mode deflate-chunked:
RLE_DYNAMIC, beside deflate and deflate-loop; --mode deflate-chunked-lz: FULL_DYNAMIC, beside deflate-lz and
deflate-lz-loop): one ndfl_deflate_batch_chunked call, a workgroup per chunk, everything else the same;
the lines carry the sibling modes' "bench".  The deflate modes have a fourth shape, 4,096 x 64 KiB.

Blocked gzip files (--mode bgzf | bgzf-hostwalk | bgzf-loop; see bgzf_modes): one ndfl_inflate_bgzf call
against one ndfl_inflate_members call on items a host walk built, and against one call per member.
Writing them (--mode bgzf-deflate | bgzf-deflate-host; see bgzf_deflate_modes): one ndfl_deflate_bgzf call
against the blocks through Context.deflate_members with the headers patched and the members joined on the host.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import struct
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "deflate-library-java_amd", "python"))

SHAPES = {"64Kx512B": (65536, 512), "4Kx4KiB": (4096, 4096), "256x1MiB": (256, 1 << 20), "4Kx64KiB": (4096, 65536)}
INFLATE_SHAPES = ("64Kx512B", "4Kx4KiB", "256x1MiB")
DEFLATE_MODES = ("deflate", "deflate-loop", "deflate-lz", "deflate-lz-loop", "deflate-multi", "deflate-multi-loop",
                 "deflate-binsplit", "deflate-binsplit-loop", "deflate-chunked", "deflate-chunked-lz")


def make_streams(name, seed):
    import numpy as np
    n, size = SHAPES[name]
    rng = random.Random(seed)
    words = [rng.randbytes(rng.randrange(2, 9)) for _ in range(200)]
    rs = np.random.RandomState(seed)
    datas, comps = [], []
    for _ in range(n):
        idx = rs.randint(0, 200, size // 4 + 1)
        data = b"".join(map(words.__getitem__, idx))[:size]
        assert len(data) == size
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
        datas.append(data)
        comps.append(co.compress(data) + co.flush())
    return datas, comps


def wrap(fmt, raw, data):
    """(member bytes, header length, the checksum its trailer holds) of one stream in --format fmt."""
    if fmt == "zlib":
        a = zlib.adler32(data)
        return b"\x78\x9c" + raw + a.to_bytes(4, "big"), 2, a
    c = zlib.crc32(data)
    if fmt == "gzip":
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", c, len(data) & 0xFFFFFFFF), 10, c
    return raw, 0, c


def make_buffers(name, seed, kind):
    """The raw buffers of the deflate modes: make_streams' word-salad text ("text"), or that text with
    runs of 4..47 equal bytes spliced in between pieces of 8..63 bytes ("runs": RLE has something to do)."""
    import numpy as np
    n, size = SHAPES[name]
    rng = random.Random(seed)
    words = [rng.randbytes(rng.randrange(2, 9)) for _ in range(200)]
    rs = np.random.RandomState(seed)
    datas = []
    for _ in range(n):
        idx = rs.randint(0, 200, size // 4 + 1)
        data = b"".join(map(words.__getitem__, idx))[:size]
        if kind == "runs":
            # segments alternate: 8..63 bytes of the text as it is, then 4..47 bytes overwritten with one value
            m = size // 12 + 2
            seg = np.empty(2 * m, dtype=np.int64)
            seg[0::2] = rs.randint(8, 64, m)
            seg[1::2] = rs.randint(4, 48, m)
            vals = rs.randint(0, 256, m).astype(np.uint8)
            which = np.repeat(np.arange(2 * m), seg)[:size]
            text = np.frombuffer(data, dtype=np.uint8)
            data = np.where(which & 1, vals[which >> 1], text).astype(np.uint8).tobytes()
        if kind == "mixed":
            q = size // 4
            text = np.frombuffer(data, dtype=np.uint8)
            data = np.concatenate([text[:q] % 10 + 48, text[q:2 * q], rs.randint(0, 256, q).astype(np.uint8),
                                   text[3 * q:] % 16 + 192]).astype(np.uint8).tobytes()
        assert len(data) == size
        datas.append(data)
    return datas


def deflate_modes(a, modes):
    """--mode deflate: one ndfl_deflate_batch call (raw DEFLATE with the CRC-32 of each buffer);
    --mode deflate-loop: one ndfl_deflate_chunks call per buffer with crc_inout, which also runs on a
    build without the batch entry point (NDFL_LIB_PATH): the baseline.  --mode deflate-lz and
    deflate-lz-loop: the same with ndfl_deflate_batch_lz77 and ndfl_deflate_chunks_lz77, FULL_DYNAMIC
    (the loop again runs on a build without the batch entry point).  --mode deflate-multi and
    deflate-multi-loop: ndfl_deflate_batch_multi and ndfl_deflate_chunks_multi with
    MultiStrategy(Uncompressed, FULL_STATIC, FULL_DYNAMIC), likewise.  --mode deflate-binsplit and
    deflate-binsplit-loop: ndfl_deflate_batch_binsplit and ndfl_deflate_chunks_binsplit with
    BinarySplit(FULL_DYNAMIC, 256), likewise; --mode deflate-chunked and deflate-chunked-lz:
    ndfl_deflate_batch_chunked with the RLE_DYNAMIC tuple and with FULL_DYNAMIC; with chunk_len = min(the buffer size, 65536) for every mode of
    the run (the loop refuses halvings of an odd length).  Input and output are
    device-resident; every buffer and every output region starts 16-byte aligned, and a region holds
    ndfl_deflate_bound bytes, so the loop's encoder writes it in place.  The first pass decodes every
    region with ndfl_inflate_members (raw + CRC-32) and compares the bytes and the checksums."""
    import torch
    import ndfl
    ctx = ndfl.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    L = ndfl._lib.load()
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE
    strategy = ndfl._lib.STRATEGIES["RLE_DYNAMIC"]
    full_dynamic = (1, 3, 258, 1, 32768)             # Lz77Huffman.FULL_DYNAMIC
    rle_dynamic = (1, 3, 258, 1, 1)                  # Lz77Huffman.RLE_DYNAMIC
    D = ndfl._lib.StrategyDesc                       # MultiStrategy(Uncompressed, FULL_STATIC, FULL_DYNAMIC)
    t3 = (D * 3)(D(ndfl._lib.KIND_UNCOMPRESSED, 0, 0, 0, 0, 0), D(ndfl._lib.KIND_LZ77, 0, 3, 258, 1, 32768),
                 D(ndfl._lib.KIND_LZ77, 1, 3, 258, 1, 32768))
    fd = D(ndfl._lib.KIND_LZ77, 1, 3, 258, 1, 32768)  # BinarySplit(FULL_DYNAMIC, 256)
    min_block_len = 256
    hist_limit = 32768
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        chunk_len = min(size, 65536) if any("binsplit" in m for m in modes) else 65536
        datas = make_buffers(name, a.seed, a.data)
        if a.buffers:
            n = min(n, a.buffers)
            datas = datas[:n]
        want = b"".join(datas)
        crcs = [zlib.crc32(d) for d in datas]
        in_stride = (size + 15) // 16 * 16
        cap = (L.ndfl_deflate_bound(size, chunk_len) + 16 + 15) // 16 * 16
        host = bytearray(n * in_stride)
        for i, d in enumerate(datas):
            host[i * in_stride:i * in_stride + size] = d
        d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
        d_out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        d_back = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        for mode in modes:
            out_lens, sums = [0] * n, [0] * n
            chunked = mode in ("deflate-chunked", "deflate-chunked-lz")
            batch = chunked or mode in ("deflate", "deflate-lz", "deflate-multi", "deflate-binsplit")
            lz = mode in ("deflate-lz", "deflate-lz-loop", "deflate-chunked-lz")
            multi = mode in ("deflate-multi", "deflate-multi-loop")
            split = mode in ("deflate-binsplit", "deflate-binsplit-loop")
            if batch:
                arr = (ndfl._lib.MemberItem * n)(*[ndfl._lib.MemberItem(i * in_stride, size, i * cap, cap, ndfl._lib.FMT_RAW,
                                                                        ndfl._lib.SUM_CRC32) for i in range(n)])
                res = (ndfl._lib.DeflateResult * n)()

            def once():
                if batch:
                    if chunked:
                        rc = L.ndfl_deflate_batch_chunked(ctx._h, pi, n * in_stride, po, n * cap, arr, res, n,
                                                          *(full_dynamic if lz else rle_dynamic), chunk_len, hist_limit, flags)
                    elif split:
                        rc = L.ndfl_deflate_batch_binsplit(ctx._h, pi, n * in_stride, po, n * cap, arr, res, n, ctypes.byref(fd),
                                                           min_block_len, chunk_len, hist_limit, flags)
                    elif multi:
                        rc = L.ndfl_deflate_batch_multi(ctx._h, pi, n * in_stride, po, n * cap, arr, res, n, t3, 3, chunk_len,
                                                        hist_limit, flags)
                    elif lz:
                        rc = L.ndfl_deflate_batch_lz77(ctx._h, pi, n * in_stride, po, n * cap, arr, res, n, *full_dynamic,
                                                       chunk_len, hist_limit, flags)
                    else:
                        rc = L.ndfl_deflate_batch(ctx._h, pi, n * in_stride, po, n * cap, arr, res, n, strategy, chunk_len,
                                                  hist_limit, flags)
                    assert rc == 0, rc
                    return ctx.last_kernel_ms()
                bits, crc = u64(0), u32(0)
                for i in range(n):
                    crc.value = 0
                    if split:
                        rc = L.ndfl_deflate_chunks_binsplit(ctx._h, None, 0, hist_limit, pi + i * in_stride, size, chunk_len,
                                                            ctypes.byref(fd), min_block_len, 1, 0, po + i * cap, cap,
                                                            ctypes.byref(bits), ctypes.byref(crc), flags)
                    elif multi:
                        rc = L.ndfl_deflate_chunks_multi(ctx._h, None, 0, hist_limit, pi + i * in_stride, size, chunk_len, t3,
                                                         3, 1, 0, po + i * cap, cap, ctypes.byref(bits), ctypes.byref(crc),
                                                         flags)
                    elif lz:
                        rc = L.ndfl_deflate_chunks_lz77(ctx._h, None, 0, hist_limit, pi + i * in_stride, size, chunk_len,
                                                        *full_dynamic, 1, 0, po + i * cap, cap, ctypes.byref(bits),
                                                        ctypes.byref(crc), flags)
                    else:
                        rc = L.ndfl_deflate_chunks(ctx._h, None, 0, hist_limit, pi + i * in_stride, size, chunk_len, strategy,
                                                   1, 0, po + i * cap, cap, ctypes.byref(bits), ctypes.byref(crc), flags)
                    assert rc == 0, rc
                    out_lens[i] = (bits.value + 7) // 8
                    sums[i] = crc.value
                return None

            times, kms = [], None
            for it in range(a.warmup + a.reps):
                d_out.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kms = once()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if it == 0:
                    if batch:
                        assert all(r.status == 0 for r in res)
                        out_lens, sums = [r.out_len for r in res], [r.checksum for r in res]
                    assert sums == crcs, "checksums differ"
                    back = ctx.inflate_members_raw(po, n * cap, d_back.data_ptr(), n * size,
                                                   [(i * cap, out_lens[i], i * size, size, ndfl._lib.FMT_RAW,
                                                     ndfl._lib.SUM_CRC32) for i in range(n)], flags)
                    assert all(r[0] == 0 and r[2] == size and r[4] == c for r, c in zip(back, crcs)), "round trip"
                    assert bytes(d_back.cpu().numpy()) == want, "round trip: bytes differ"
                if it >= a.warmup:
                    times.append(dt)
            med = statistics.median(times)
            line = {"bench": "batch_deflate_binsplit" if split else "batch_deflate_multi" if multi else "batch_deflate_lz" if lz
                    else "batch_deflate", "label": a.label, "mode": mode, "data": a.data,
                    "shape": name, "buffers": n, "buffer_bytes": size, "in_bytes": n * size, "out_bytes": sum(out_lens),
                    "strategy": "BINSPLIT(FULL_DYNAMIC,256)" if split else "MULTI(UNCOMPRESSED,FULL_STATIC,FULL_DYNAMIC)" if multi
                    else "FULL_DYNAMIC" if lz else "RLE_DYNAMIC", "chunk_len": chunk_len,
                    "ms_median": round(med, 3), "ms_all": [round(t, 3) for t in times],
                    "in_MBps": round(n * size / med / 1e3, 1)}
            if kms is not None:
                line["kernel_ms_last"] = round(kms, 3)
            print(json.dumps(line), flush=True)
        del d_in, d_out, d_back


BGZF_MODES = ("bgzf", "bgzf-hostwalk", "bgzf-loop")
BGZF_SIZES = {"16MiB": 256, "256MiB": 4096, "1GiB": 16384}          # blocks of 65,280 bytes
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_modes(a, modes):
    """A blocked gzip (BGZF) file of 65,280-byte blocks of the --data corpus (text | mixed), zlib level 6,
    device-resident and padded, decoded into device memory three ways:
      bgzf           one ndfl_inflate_bgzf call: the members found and laid out on the device.
      bgzf-hostwalk  the members found by a walk over a HOST copy of the file (BSIZE, ISIZE), then one
                     ndfl_inflate_members call on those items: the best a build without ndfl_inflate_bgzf
                     can do.  The walk is timed with the call ("walk_ms" is its share); bringing a
                     device-resident file to the host for it is not ("d2h_ms", measured once).
      bgzf-loop      one ndfl_inflate_members call per member, each told only where it starts: the next
                     start is consumed_bits / 8 of the one before.
    The distinct blocks are the 4,096 buffers of shape 4Kx64KiB; larger files repeat them (members are
    independent).  Lines are "bench": "bgzf"; bgzf's carry the event times of discovery with layout
    ("layout_ms") and of the members kernel with the reduction ("decode_ms")."""
    import numpy as np
    import torch
    import ndfl
    ctx = ndfl.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | ndfl.IN_PADDED
    L = ndfl._lib.load()
    block = 65280
    sizes = a.shapes.split(",") if a.shapes else list(BGZF_SIZES)
    distinct = min(4096, max(BGZF_SIZES[s] for s in sizes))
    datas = [d[:block] for d in make_buffers("4Kx64KiB", a.seed, a.data)[:distinct]]
    members = []
    for d in datas:
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
        body = co.compress(d) + co.flush()
        n = 18 + len(body) + 8
        members.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", n - 1) + body +
                       struct.pack("<II", zlib.crc32(d), len(d)))
    d_want = torch.frombuffer(bytearray(b"".join(datas)), dtype=torch.uint8).cuda()
    for name in sizes:
        nblocks = BGZF_SIZES[name]
        file = b"".join(members[i % distinct] for i in range(nblocks)) + BGZF_EOF
        total = nblocks * block
        host = bytearray((len(file) + ndfl.IN_PAD_BYTES + 15) // 16 * 16)
        host[:len(file)] = file
        d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
        d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_copy = bytes(d_in[:len(file)].cpu().numpy())
        d2h_ms = (time.perf_counter() - t0) * 1e3
        assert host_copy == file
        for mode in modes:
            extra = {}

            def once():
                if mode == "bgzf":
                    res = ndfl._lib.BgzfResult()
                    rc = L.ndfl_inflate_bgzf(ctx._h, pi, len(file), po, total, ctypes.byref(res), None, 0, flags)
                    assert rc == 0 and res.n_members == nblocks + 1 and res.out_len == total, (rc, res.n_members)
                    assert res.consumed_bytes == len(file)
                    t = ctx.timings()
                    extra.update(layout_ms=round(t["inflate_find"], 3), decode_ms=round(t["inflate_emit"], 3))
                    return ctx.last_kernel_ms()
                if mode == "bgzf-hostwalk":
                    t0 = time.perf_counter()
                    items, p, o = [], 0, 0
                    while p < len(host_copy):
                        mlen = (host_copy[p + 16] | host_copy[p + 17] << 8) + 1     # (BC is these files' first subfield)
                        isize = int.from_bytes(host_copy[p + mlen - 4:p + mlen], "little")
                        items.append((p, mlen, o, isize))
                        p += mlen
                        o += isize
                    arr = np.zeros((len(items), 5), dtype=np.uint64)
                    arr[:, :4] = items
                    arr[:, 4] = ndfl._lib.FMT_GZIP                                  # format (low word), sum = 0
                    res = (ndfl._lib.MemberResult * len(items))()
                    extra["walk_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                    rc = L.ndfl_inflate_members(ctx._h, pi, len(file), po, total,
                                                arr.ctypes.data_as(ctypes.POINTER(ndfl._lib.MemberItem)), res, len(items), flags)
                    assert rc == 0 and all(r.status == 0 for r in res), rc
                    return ctx.last_kernel_ms()
                p, o = 0, 0
                item = (ndfl._lib.MemberItem * 1)()
                res = (ndfl._lib.MemberResult * 1)()
                while p < len(file):
                    item[0] = ndfl._lib.MemberItem(p, min(65536, len(file) - p), o, min(65536, total - o), ndfl._lib.FMT_GZIP, 0)
                    rc = L.ndfl_inflate_members(ctx._h, pi, len(file), po, total, item, res, 1, flags)
                    assert rc == 0 and res[0].status == 0, (rc, res[0].status, p)
                    p += res[0].consumed_bits // 8
                    o += res[0].out_len
                assert o == total
                return None

            times, kms = [], None
            for it in range(a.warmup + a.reps):
                d_out.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kms = once()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if it == 0:
                    for k in range(0, nblocks, distinct):
                        m = min(distinct, nblocks - k) * block
                        assert torch.equal(d_out[k * block:k * block + m], d_want[:m]), "decoded bytes differ"
                if it >= a.warmup:
                    times.append(dt)
            med = statistics.median(times)
            line = {"bench": "bgzf", "label": a.label, "mode": mode, "data": a.data, "file": name, "members": nblocks + 1,
                    "in_bytes": len(file), "out_bytes": total, "ms_median": round(med, 3),
                    "ms_all": [round(t, 3) for t in times], "out_MBps": round(total / med / 1e3, 1), **extra}
            if mode == "bgzf-hostwalk":
                line["d2h_ms"] = round(d2h_ms, 3)
            if kms is not None:
                line["kernel_ms_last"] = round(kms, 3)
            print(json.dumps(line), flush=True)
        del d_in, d_out


BGZF_DEFLATE_MODES = ("bgzf-deflate", "bgzf-deflate-host")


def bgzf_deflate_modes(a, modes):
    """The write side: the --data corpus (text | runs | mixed) in blocks of 65,280 bytes, the shapes of the
    bgzf modes, as a blocked gzip (BGZF) file with MultiStrategy(FULL_DYNAMIC, Uncompressed) per member:
      bgzf-deflate       one ndfl_deflate_bgzf call, device to device ("io": "device", into a buffer of
                         ndfl_bgzf_bound bytes) and host to host ("io": "host", bytes in, bytes out:
                         Context.deflate_bgzf).
      bgzf-deflate-host  what a build without the call does, host to host: the data sliced into blocks,
                         Context.deflate_members on the wave path, BSIZE patched into every member and the
                         members joined on the host ("io": "host").
    Lines are "bench": "bgzf-deflate".  The first file of every mode is read back with Python's gzip."""
    import gzip
    import torch
    import ndfl
    from ndfl import bgzf
    ctx = ndfl.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    L = ndfl._lib.load()
    block = 65280
    x = ndfl.Lz77Huffman.FULL_DYNAMIC
    tup = (1,) + tuple(x.params)
    sizes = a.shapes.split(",") if a.shapes else list(BGZF_SIZES)
    distinct = min(4096, max(BGZF_SIZES[s] for s in sizes))
    datas = [d[:block] for d in make_buffers("4Kx64KiB", a.seed, a.data)[:distinct]]
    for name in sizes:
        nblocks = BGZF_SIZES[name]
        data = b"".join(datas[i % distinct] for i in range(nblocks))
        total = len(data)
        for mode in modes:
            for io in (("device", "host") if mode == "bgzf-deflate" else ("host",)):
                state = {}
                if io == "device":
                    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
                    cap = L.ndfl_bgzf_bound(total, block)
                    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")

                def once():
                    if io == "device":
                        res = ndfl._lib.BgzfWriteResult()
                        rc = L.ndfl_deflate_bgzf(ctx._h, d_in.data_ptr(), total, d_out.data_ptr(), cap, ctypes.byref(res), None, 0,
                                                 *tup, block, ndfl.IN_DEVICE | ndfl.OUT_DEVICE)
                        assert rc == 0 and res.n_members == nblocks + 1, (rc, res.n_members)
                        state.update(out_len=res.out_len, n_stored=res.n_stored)
                        return ctx.last_kernel_ms()
                    if mode == "bgzf-deflate":
                        state["file"] = ctx.deflate_bgzf(data, block, x)[0]
                        return ctx.last_kernel_ms()
                    blocks = [data[i:i + block] for i in range(0, total, block)]
                    members = ctx.deflate_members(blocks, ndfl.FMT_GZIP,
                                                  meta=ndfl.GzipMetadata(operatingSystem="UNKNOWN", extraField=bgzf.EXTRA),
                                                  strategy=ndfl.MultiStrategy(x, ndfl.Uncompressed.SINGLETON))
                    state["file"] = b"".join(bgzf.member_with_bsize(m) for m in members) + bgzf.EOF
                    return ctx.last_kernel_ms()

                times, kms = [], None
                for it in range(a.warmup + a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    kms = once()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if it == 0:
                        f = bytes(d_out[:state["out_len"]].cpu().numpy()) if io == "device" else state["file"]
                        assert gzip.decompress(f) == data, "the file does not hold the data"
                        state["out_len"] = len(f)
                    if it >= a.warmup:
                        times.append(dt)
                med = statistics.median(times)
                line = {"bench": "bgzf-deflate", "label": a.label, "mode": mode, "io": io, "data": a.data, "file": name,
                        "members": nblocks + 1, "in_bytes": total, "out_bytes": state["out_len"], "ms_median": round(med, 3),
                        "ms_all": [round(t, 3) for t in times], "in_MBps": round(total / med / 1e3, 1),
                        "kernel_ms_last": round(kms, 3)}
                if "n_stored" in state:
                    line["n_stored"] = state["n_stored"]
                print(json.dumps(line), flush=True)
                if io == "device":
                    del d_in, d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True,
                    help="comma-separated: loop, batch, members, batch+sum; or deflate, deflate-loop, deflate-lz, "
                         "deflate-lz-loop, deflate-multi, deflate-multi-loop, deflate-binsplit, deflate-binsplit-loop, "
                         "deflate-chunked, deflate-chunked-lz; or bgzf, bgzf-hostwalk, bgzf-loop (--shapes: 16MiB, "
                         "256MiB, 1GiB; --data text | mixed); or bgzf-deflate, bgzf-deflate-host (the same shapes; "
                         "--data text | runs | mixed)")
    ap.add_argument("--data", choices=["text", "runs", "mixed"], default="text", help="deflate modes: the buffers' content")
    ap.add_argument("--buffers", type=int, default=0, help="deflate modes: only the first N buffers of each shape")
    ap.add_argument("--format", choices=["zlib", "gzip", "raw-crc"], default="zlib",
                    help="members / batch+sum: the container of each stream")
    ap.add_argument("--shapes", default="", help="default: every shape of the modes (the deflate modes have 4Kx64KiB too)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if all(m in BGZF_MODES for m in a.mode.split(",")):
        return bgzf_modes(a, a.mode.split(","))
    if all(m in BGZF_DEFLATE_MODES for m in a.mode.split(",")):
        return bgzf_deflate_modes(a, a.mode.split(","))
    if all(m in DEFLATE_MODES for m in a.mode.split(",")):
        a.shapes = a.shapes or ",".join(SHAPES)
        return deflate_modes(a, a.mode.split(","))
    a.shapes = a.shapes or ",".join(INFLATE_SHAPES)
    import torch
    import ndfl
    ctx = ndfl.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | ndfl.IN_PADDED
    modes = a.mode.split(",")
    assert all(m in ("loop", "batch", "members", "batch+sum") for m in modes), modes
    L = ndfl._lib.load()
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        datas, comps = make_streams(name, a.seed)
        want = b"".join(datas)
        for mode in modes:
            contained = mode in ("members", "batch+sum")
            fmt = a.format if contained else "raw"
            packed = [wrap(fmt, c, d) for c, d in zip(comps, datas)] if contained else [(c, 0, 0) for c in comps]
            in_offs, off = [], 0
            for m, _, _ in packed:
                in_offs.append(off)
                off += (len(m) + ndfl.IN_PAD_BYTES + 15) // 16 * 16
            host = bytearray(off + 16)
            for o, (m, _, _) in zip(in_offs, packed):
                host[o:o + len(m)] = m
            d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
            d_out = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
            pi, po = d_in.data_ptr(), d_out.data_ptr()
            # the batch's view: the DEFLATE data alone (behind the header, which batch+sum is told for nothing)
            items = [(in_offs[i] + packed[i][1], len(comps[i]), i * size, size) for i in range(n)]
            sums = [0] * n

            # the batches go straight to the C ABI with their item and result arrays built once (the
            # Python wrapper's per-item conversions would be most of the small shapes' time)
            if mode in ("batch", "batch+sum"):
                arr = (ndfl._lib.BatchItem * n)(*[ndfl._lib.BatchItem(*it) for it in items])
                res = (ndfl._lib.BatchResult * n)()
            if mode == "members":
                f, k = {"zlib": (ndfl._lib.FMT_ZLIB, 0), "gzip": (ndfl._lib.FMT_GZIP, 0),
                        "raw-crc": (ndfl._lib.FMT_RAW, ndfl._lib.SUM_CRC32)}[fmt]
                arr = (ndfl._lib.MemberItem * n)(*[ndfl._lib.MemberItem(in_offs[i], len(packed[i][0]), i * size, size, f, k)
                                                   for i in range(n)])
                res = (ndfl._lib.MemberResult * n)()
            sum_call = L.ndfl_adler32 if fmt == "zlib" else L.ndfl_crc32
            sum_init = 1 if fmt == "zlib" else 0

            def once():
                if mode == "members":
                    rc = L.ndfl_inflate_members(ctx._h, pi, len(host), po, n * size, arr, res, n, flags)
                    assert rc == 0, rc
                    return ctx.last_kernel_ms()
                if mode in ("batch", "batch+sum"):
                    rc = L.ndfl_inflate_batch(ctx._h, pi, len(host), po, n * size, arr, res, n, flags)
                    assert rc == 0, rc
                    kms = ctx.last_kernel_ms()
                    if mode == "batch+sum":
                        v = ctypes.c_uint32()
                        for i in range(n):
                            v.value = sum_init
                            rc = sum_call(ctx._h, ctypes.byref(v), po + i * size, res[i].out_len, ndfl.IN_DEVICE)
                            assert rc == 0, rc
                            sums[i] = v.value
                    return kms
                for io, il, oo, oc in items:
                    r, olen, _ = ctx.inflate_raw(pi + io, il, po + oo, oc, flags)
                    assert r == 0 and olen == size
                return None

            times, kms = [], None
            for it in range(a.warmup + a.reps):
                d_out.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kms = once()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if it == 0:
                    assert bytes(d_out.cpu().numpy()) == want, "decoded bytes differ"
                    if mode != "loop":
                        assert all(r.status == 0 and r.out_len == size for r in res)
                    if mode == "members":
                        # (a raw stream's consumed_bits end inside its last byte, a member's are its length)
                        assert all(r.checksum == m[2] and (r.consumed_bits + 7) // 8 == len(m[0]) for r, m in zip(res, packed))
                    if mode == "batch+sum":
                        assert sums == [m[2] for m in packed], "checksums differ"
                if it >= a.warmup:
                    times.append(dt)
            med = statistics.median(times)
            line = {"bench": "batch_inflate", "label": a.label, "mode": mode, "shape": name, "streams": n,
                    "stream_bytes": size, "in_bytes": sum(len(m[0]) for m in packed), "out_bytes": n * size,
                    "ms_median": round(med, 3), "ms_all": [round(t, 3) for t in times],
                    "out_MBps": round(n * size / med / 1e3, 1)}
            if contained:
                line["format"] = fmt
            if kms is not None:
                line["kernel_ms_last"] = round(kms, 3)
            print(json.dumps(line), flush=True)
            del d_in, d_out


if __name__ == "__main__":
    main()
