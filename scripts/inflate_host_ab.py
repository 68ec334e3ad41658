#!/usr/bin/env python3
"""A/B driver for the inflate host code (csrc/capi/ndfl_inflate.cpp): the same calls on whichever library
NDFL_LIB_PATH names, so that two builds can be compared launch by launch and call by call.

  inflate_host_ab.py drive           every kind of inflate call once (below); one result line per call.  Run it under
                                     `rocprofv3 --kernel-trace -- python scripts/inflate_host_ab.py drive` for the ordered
                                     launch list, and with NDFL_STATS=1 for the statistics lines (stderr).
  inflate_host_ab.py time LABEL ROUND FILE
                                     30 warm-up and 300 timed calls per case, wall time around the raw call; appends one
                                     JSON line per case to FILE and prints its median.
  inflate_host_ab.py verdict FILE    per case: round medians per label, pooled medians, and whether `new`'s pooled median
                                     is not above the largest round median of `parent` or `ctrl`.

Streams: link_geometry.pool_stream(12) (3.6 KB, the stream of tests/test_gpu_inflate_abi.py) and the family-L stream of
4,097 chains.  drive: a whole decode of both on default, NDFL_HOST_LINK=1, NDFL_NO_ALIAS=1 and NDFL_COUNT_W=4 contexts;
then, default context, small stream: a deferred range decode from block 5 with tail, tail map and resolve, a sync
probe, a headers call."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "deflate-library-java_amd", "python"), os.path.join(ROOT, "tests")]
WAYS = [("default", {}), ("host_link", {"NDFL_HOST_LINK": "1"}), ("no_alias", {"NDFL_NO_ALIAS": "1"}),
        ("count_w4", {"NDFL_COUNT_W": "4"})]
K = 5                                           # the range decodes start at block 5's seam
u64 = ctypes.c_uint64


def context(ndfl, env):
    """A context whose switches come from `env` (they are read when the context is created)."""
    os.environ.update(env)
    try:
        ctx = ndfl.Context(0)
        ctx._order()                            # (the raw calls below run on torch's current stream, as its own ops)
        return ctx
    finally:
        for k in env:
            del os.environ[k]


class Calls:
    """The raw calls on one stream: host input; host output, or a device buffer for the deferred range decode."""

    def __init__(self, ndfl, torch, b):
        self.L, self.lib, self.b = ndfl._lib.load(), ndfl._lib, b
        comp = b.w.getbytes()
        self.expect, self.n = bytes(b.out), len(comp)
        self.src = ctypes.create_string_buffer(comp, len(comp))
        self.out = ctypes.create_string_buffer(len(self.expect) + 64)
        self.olen, self.bits = u64(0), u64(0)
        self.start, self.dl = b.seams[K], b.outs[K]
        self.dev = torch.zeros(len(self.expect) + 64, dtype=torch.uint8, device="cuda")
        self.tail = torch.zeros(4096, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def inflate(self, ctx):
        return self.L.ndfl_inflate(ctx._h, ctypes.addressof(self.src), self.n, ctypes.addressof(self.out), len(self.out),
                                   ctypes.byref(self.olen), ctypes.byref(self.bits), 0)

    def range_deferred(self, ctx):
        return self.L.ndfl_inflate_range(ctx._h, ctypes.addressof(self.src), self.n, self.start, 2 ** 64 - 1,
                                         self.dev.data_ptr(), self.dl, len(self.expect) - self.dl, ctypes.byref(self.olen),
                                         ctypes.byref(self.bits), self.lib.OUT_DEVICE | self.lib.DICT_DEFERRED)

    def resolve(self, ctx):
        return self.L.ndfl_inflate_resolve(ctx._h, ctypes.byref(self.olen))

    def sync(self, ctx):
        return self.L.ndfl_inflate_sync(ctx._h, ctypes.addressof(self.src), self.n, 1, self.n * 8, ctypes.byref(self.bits), 0)


def drive(ndfl, torch, G):
    small, chains = G.pool_stream(12), G.pool_stream(4097)
    for way, env in WAYS:
        ctx = context(ndfl, env)
        for name, b in (("pool12", small), ("L_4097", chains)):
            c = Calls(ndfl, torch, b)
            r = c.inflate(ctx)
            ok = r == 0 and c.out.raw[:c.olen.value] == c.expect and c.bits.value == b.end
            print(f"{way} {name} inflate: code {r} out_len {c.olen.value} bits {c.bits.value} {'ok' if ok else 'WRONG'}")
    ctx = context(ndfl, {})
    c = Calls(ndfl, torch, small)
    window = torch.frombuffer(bytearray(c.expect[:c.dl]), dtype=torch.uint8).cuda()
    r = c.range_deferred(ctx)
    print(f"range deferred from block {K}: code {r} out_len {c.olen.value} bits {c.bits.value}")
    n_tail = min(64, c.olen.value)
    r = c.L.ndfl_inflate_tail_map(ctx._h, n_tail, c.tail.data_ptr())
    print(f"tail map: code {r} {c.tail[:n_tail].cpu().tolist()}")
    c.dev[:c.dl] = window
    torch.cuda.synchronize()
    tail = torch.zeros(n_tail, dtype=torch.uint8, device="cuda")
    r = c.L.ndfl_inflate_tail(ctx._h, n_tail, tail.data_ptr())
    print(f"tail: code {r} {'ok' if bytes(tail.cpu().tolist()) == c.expect[-n_tail:] else 'WRONG'}")
    r = c.resolve(ctx)
    got = bytes(c.dev[:len(c.expect)].cpu().tolist())
    print(f"resolve: code {r} groups {c.olen.value} {'ok' if got == c.expect else 'WRONG'}")
    r = c.sync(ctx)
    print(f"sync probe from bit 1: code {r} sync_bit {c.bits.value} {'ok' if c.bits.value in small.seams else 'WRONG'}")
    res = ctx.inflate_headers(small.w.getbytes())
    print(f"headers: {list(res[0])} stats {list(res[1])}")


def timed(ndfl, torch, G, label, rnd, path):
    c = Calls(ndfl, torch, G.pool_stream(12))
    dflt, host = context(ndfl, {}), context(ndfl, {"NDFL_HOST_LINK": "1"})

    def range_resolve(ctx):
        return c.range_deferred(ctx) or c.resolve(ctx)
    cases = [("inflate default", dflt, c.inflate), ("inflate host_link", host, c.inflate),
             ("range deferred + resolve", dflt, range_resolve), ("sync", dflt, c.sync)]
    with open(path, "a") as f:
        for name, ctx, call in cases:
            us = []
            for k in range(330):
                t0 = time.perf_counter()
                r = call(ctx)
                t1 = time.perf_counter()
                assert r == 0, (name, r)
                if k >= 30:
                    us.append((t1 - t0) * 1e6)
            q = statistics.quantiles(us, n=10)
            print(f"round {rnd} {label:6s} {name:26s} median {statistics.median(us):9.2f} us  p10 {q[0]:9.2f}  p90 {q[-1]:9.2f}")
            f.write(json.dumps({"label": label, "round": rnd, "case": name, "us": us}) + "\n")


def verdict(path):
    rows = [json.loads(line) for line in open(path)]
    for name in dict.fromkeys(r["case"] for r in rows):
        med, pooled = {}, {}
        for r in rows:
            if r["case"] == name:
                med.setdefault(r["label"], []).append(statistics.median(r["us"]))
                pooled.setdefault(r["label"], []).extend(r["us"])
        bound = max(med["parent"] + med["ctrl"])
        new = statistics.median(pooled["new"])
        print(f"{name:26s} pooled median us: " + "  ".join(f"{k} {statistics.median(v):.2f}" for k, v in pooled.items()) +
              f"; largest parent/ctrl round median {bound:.2f}: new {'passes' if new <= bound else 'IS ABOVE IT'}")


if __name__ == "__main__":
    if sys.argv[1] == "verdict":
        verdict(sys.argv[2])
    else:
        import torch
        torch.cuda.init()                       # (torch's runtime first, as the ABI tests do)
        import ndfl
        import link_geometry
        if sys.argv[1] == "drive":
            drive(ndfl, torch, link_geometry)
        else:
            timed(ndfl, torch, link_geometry, sys.argv[2], int(sys.argv[3]), sys.argv[4])
