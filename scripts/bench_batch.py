#!/usr/bin/env python3
"""Many independent raw DEFLATE streams: one ndfl_inflate call per stream (--mode loop) against one
ndfl_inflate_batch call (--mode batch).  Not bench.py: this measures the batch entry point only.

Inputs are seeded word-salad text (as tests/test_gpu_inflate.py::test_zlib_streams), compressed with
Python's zlib, raw (wbits=-15), in three shapes: 65,536 x 512 B, 4,096 x 4 KiB, 256 x 1 MiB.  Inputs
and outputs are device-resident; every stream starts 16-byte aligned and is followed by
NDFL_IN_PAD_BYTES zero bytes, so the loop decodes in place (NDFL_IN_PADDED) -- its best case -- and
the batch reads the same buffer.  Timing: wall clock around the calls (both are complete when they
return), median of --reps after --warmup, one JSON line per shape.  The first pass checks every
output byte against the original data.

--mode loop needs only ndfl_inflate, so it also runs on a build without the batch entry point
(NDFL_LIB_PATH selects the library): that is the baseline.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "deflate-library-java_amd", "python"))

SHAPES = {"64Kx512B": (65536, 512), "4Kx4KiB": (4096, 4096), "256x1MiB": (256, 1 << 20)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["loop", "batch"], required=True)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import ndfl
    ctx = ndfl.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    flags = ndfl.IN_DEVICE | ndfl.OUT_DEVICE | ndfl.IN_PADDED
    for name in a.shapes.split(","):
        n, size = SHAPES[name]
        datas, comps = make_streams(name, a.seed)
        in_offs, off = [], 0
        for c in comps:
            in_offs.append(off)
            off += (len(c) + ndfl.IN_PAD_BYTES + 15) // 16 * 16
        host = bytearray(off + 16)
        for o, c in zip(in_offs, comps):
            host[o:o + len(c)] = c
        d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
        d_out = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        items = [(in_offs[i], len(comps[i]), i * size, size) for i in range(n)]
        want = b"".join(datas)

        # the batch goes straight to the C ABI with its item and result arrays built once (the
        # Python wrapper's per-item conversions would be most of the small shapes' time)
        L = ndfl._lib.load()
        if a.mode == "batch":
            arr = (ndfl._lib.BatchItem * n)(*[ndfl._lib.BatchItem(*it) for it in items])
            res = (ndfl._lib.BatchResult * n)()

        def once():
            if a.mode == "batch":
                rc = L.ndfl_inflate_batch(ctx._h, pi, len(host), po, n * size, arr, res, n, flags)
                assert rc == 0, rc
                return ctx.last_kernel_ms()
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
                if a.mode == "batch":
                    assert all(r.status == 0 and r.out_len == size for r in res)
            if it >= a.warmup:
                times.append(dt)
        med = statistics.median(times)
        line = {"bench": "batch_inflate", "label": a.label, "mode": a.mode, "shape": name, "streams": n,
                "stream_bytes": size, "in_bytes": sum(map(len, comps)), "out_bytes": n * size,
                "ms_median": round(med, 3), "ms_all": [round(t, 3) for t in times],
                "out_MBps": round(n * size / med / 1e3, 1)}
        if kms is not None:
            line["kernel_ms_last"] = round(kms, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
