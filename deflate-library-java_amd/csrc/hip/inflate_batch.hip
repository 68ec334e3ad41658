// inflate_batch.hip -- batched inflate: many independent raw DEFLATE streams in one launch
// (ndfl_inflate_batch, include/ndfl.h).
//
// The one-stream decoder (inflate_kernels.hip) parallelises INSIDE a stream: header finder, strict
// stage, count, link, emit, resolve -- several launches and two host syncs, which is the whole cost
// of a 2 KiB stream.  This kernel parallelises ACROSS streams instead: a persistent grid of one-wave
// workgroups, each wave claiming stream indices from an atomic ticket and decoding its stream
// serially from the first bit, so the launch count does not depend on the number of streams and the
// host syncs once.  Per block, lane 0 parses the header (wv::parse_hdr_core: the reference's check
// order) and the wave builds the tables (wv::build_code_l, the Tabs entry format of the one-stream
// passes); the token loop is wave-uniform: every lane holds the same bit position and the same
// token (made scalar with readfirstlane), and the 64 lanes share the byte work -- literals are
// gathered one per lane and stored together, copies and stored blocks are done 64 bytes a step.
//
// Window: the stream's last 32 KiB of output live in an LDS ring per wave, indexed by the output
// ADDRESS modulo 32 KiB (so a 16-byte aligned global store reads a 16-byte aligned ring slot that
// never wraps).  Every copy source comes from the ring; completed spans are flushed to global
// memory -- 16-byte stores between exact-width byte stores at a span's two ends, clamped to the
// stream's region, so no store overhangs it.  No lane ever reads back global memory another lane has
// written, so no fence between stores and loads is needed; the ring costs occupancy instead (LDS per
// wave and waves per CU: DESIGN.md §4, "Batched inflate").  Past out_cap the decode goes on in the
// ring alone (all checks need positions only), which gives NDFL_E_CAPACITY its required size and
// keeps a later Reason exact.
//
// A wave decodes several streams one after another: the code lengths are zeroed per block, the
// tables rebuilt per block, the pending literals, the staged input and the ring positions reset per
// stream (the ring's old bytes are unreachable: a distance past the stream's own start is
// COPY_FROM_BEFORE_DICTIONARY_START).
//
// The header parse and the table build are the forceinline cores (parse_hdr_core, build_code_l), not
// the parse_hdr / build_tables wrappers: build_tables_l is __noinline__ and parse_hdr is not forced
// inline, and a real call's stack lives in scratch memory, which this kernel must not have (DESIGN.md
// §7 item 9: wrong values when two scratch-using waves of one kernel share a SIMD).
#pragma once

namespace bat {
using namespace inf;
using namespace wv;

constexpr uint32_t RING = 32768, RMASK = RING - 1;
constexpr uint32_t IW = 128;                  // staged input words per wave (512 bytes)
constexpr uint32_t STORED_STEP = 8192;        // bytes of a stored block copied between flush checks
constexpr uint64_t NO_STAGE = ~0ull >> 1;

// The reader the issue of a per-stream bit base asks for is inf::In itself, re-based: stream i's `w`
// is the word holding its first byte, its first bit is 8 * (in_off & 3), and nbits / nwords end at its
// last byte, so In::ld never returns a word past the stream's last one and every position check
// (pos > nbits) is the stream's own.  Bits of the neighbour in the stream's last word are never
// acted on: each read is followed by its position check before any value-dependent check.
__device__ __forceinline__ In stream_in(const uint32_t* w, uint64_t in_off, uint64_t in_len) {
    const uint64_t mis = in_off & 3;
    return In{w + (in_off >> 2), (mis + in_len + 3) >> 2, (mis + in_len) * 8};
}

// The whole table build of a Huffman block (the body of wv::build_tables_l, inlined): error or 0 in
// bits 0..7, empty distance code in bit 8.
__device__ __forceinline__ int build_block_tables(LShared* S, int lane, lu32* scr) {
    if (S->h_btype == 1) {
        for (uint32_t s = (uint32_t)lane; s < 320; s += 64) {
            uint32_t l;
            if (s < 288) l = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            else l = 5;
            S->lens[s] = (uint8_t)l;
        }
        __syncthreads();
    }
    const int e = build_code_l<false, LB, true>(S, 0, 288, S->t.lit, S->t.lx, LX, true, lane, scr);
    if (e) return e;
    const uint32_t numDist = S->h_numdist;
    const uint32_t dl = (lane < 32) ? S->lens[288 + lane] : 0u;
    if (S->h_btype != 1 && numDist == 1 && S->lens[288] == 0) return 0x100;
    const uint32_t ones = (uint32_t)__popcll(__ballot(dl == 1)), other = (uint32_t)__popcll(__ballot(dl > 1));
    __syncthreads();
    if (ones == 1 && other == 0 && lane == 0) S->lens[288 + 31] = 1;
    __syncthreads();
    return build_code_l<false, DB>(S, 288, 32, S->t.dst, S->t.dx, DX, false, lane, scr);
}

// One stream's output state (wave-uniform).  Positions are output ADDRESSES: o = the next byte's,
// fl = the first byte not yet flushed, [obeg, oend) = the stream's region.
struct Out {
    uint8_t* ring;         // LDS, RING bytes, 16-byte aligned
    uint64_t obeg, oend, o, fl;
    uint32_t npend;        // literals held in registers (lane k holds the k-th), not yet in the ring
};

// Store ring bytes [fl, fend) that lie inside the region; the ring keeps them.
__device__ __forceinline__ void flush_to(Out& q, uint64_t fend, int lane) {
    if (fend <= q.fl) return;
    wsync();                                   // the ring writes of other lanes
    uint64_t a = q.fl;
    const uint64_t b = min(fend, q.oend);
    q.fl = fend;
    if (a >= b) return;
    const uint32_t head = (uint32_t)min((uint64_t)((16u - (uint32_t)(a & 15)) & 15u), b - a);
    if ((uint32_t)lane < head) *(uint8_t*)(a + lane) = q.ring[(a + lane) & RMASK];
    a += head;
    const uint64_t nv = (b - a) >> 4;
    for (uint64_t i = (uint64_t)lane; i < nv; i += 64)
        *(uint4*)(a + 16 * i) = *(const uint4*)&q.ring[(a + 16 * i) & RMASK];
    a += nv * 16;
    const uint32_t tail = (uint32_t)(b - a);
    if ((uint32_t)lane < tail) *(uint8_t*)(a + lane) = q.ring[(a + lane) & RMASK];
}
// Room for n more bytes (n <= RING - 16): ring slots are reused only once flushed.  A flush between
// blocks ends on a 16-byte boundary, so only a region's two ends see byte stores.
__device__ __forceinline__ void make_room(Out& q, uint32_t n, int lane) {
    if (q.o + n - q.fl > RING) flush_to(q, q.o & ~15ull, lane);
}
__device__ __forceinline__ void flush_pending(Out& q, uint32_t pend, int lane) {
    if (!q.npend) return;
    make_room(q, q.npend, lane);
    if ((uint32_t)lane < q.npend) q.ring[(q.o + lane) & RMASK] = (uint8_t)pend;
    q.o += q.npend;
    q.npend = 0;
    wsync();
}
__device__ __forceinline__ void add_literal(Out& q, uint32_t& pend, uint32_t b, int lane) {
    pend = (uint32_t)lane == q.npend ? b : pend;
    if (++q.npend == 64) flush_pending(q, pend, lane);
}
// A copy of n (3..258) bytes from dist (1..32768) back, the pending literals already in the ring.
// dist >= 64 or dist >= n: 64 bytes a step straight from the ring (a step's sources were written by
// earlier steps; with dist near 32768 a step's sources share slots only with its own or later
// destinations, and each step reads before it writes).  Otherwise the source is a period of dist
// bytes: byte k comes from byte k mod dist of the last dist bytes, which no step overwrites.
__device__ __forceinline__ void copy_run(Out& q, uint32_t n, uint32_t dist, int lane) {
    make_room(q, n, lane);
    const uint64_t src = q.o - dist;
    if (dist >= 64 || dist >= n) {
        for (uint32_t k0 = 0; k0 < n; k0 += 64) {
            const uint32_t k = k0 + (uint32_t)lane;
            const uint8_t v = q.ring[(src + k) & RMASK];        // (k >= n: read, not written)
            wsync();
            if (k < n) q.ring[(q.o + k) & RMASK] = v;
            wsync();
        }
    } else {
        uint32_t m = (uint32_t)lane % dist;
        const uint32_t step = 64u % dist;
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) {
            q.ring[(q.o + k) & RMASK] = q.ring[(src + m) & RMASK];
            m += step;
            m -= m >= dist ? dist : 0u;
        }
    }
    q.o += n;
    wsync();
}


// The wave-uniform stream state is scalar in the token loop.  Across a block's header parse and
// table build it is parked in vector registers: the build keeps its per-length values scalar, and
// with this state scalar too the kernel spilled SGPRs.
__device__ __forceinline__ uint64_t to_v(uint64_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint32_t to_v(uint32_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint32_t to_s(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t to_s(uint64_t x) {       // (the builtin returns int: no sign extension)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ void park(Out& q, uint64_t& cur, uint64_t& iw0) {
    q.o = to_v(q.o); q.fl = to_v(q.fl); q.npend = to_v(q.npend); cur = to_v(cur); iw0 = to_v(iw0);
}
__device__ __forceinline__ void unpark(Out& q, uint64_t& cur, uint64_t& iw0) {
    q.o = to_s(q.o); q.fl = to_s(q.fl); q.npend = to_s(q.npend); cur = to_s(cur); iw0 = to_s(iw0);
}

}  // namespace bat

// results[i].status: the decoder's internal Reason (R_*, the host maps it and derives the symbol),
// NDFL_E_CAPACITY, or 0; out_len and consumed_bits as the C ABI documents them.
extern "C" __global__ void __launch_bounds__(64)
ndfl_inflate_batch_kernel(const uint32_t* w, uint8_t* out, const ndfl_batch_item* items, ndfl_batch_result* results,
                          uint32_t n, uint32_t* ticket) {
    using namespace bat;
    __shared__ __attribute__((aligned(16))) Shared S;
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ uint32_t inw[IW];
    __shared__ uint32_t s_ticket;
    const int lane = threadIdx.x;
    // The table build gets the lane index read back from LDS (S.kind_, which this kernel does not use
    // otherwise): computed from threadIdx, the build's many lane masks and lane-derived constants are
    // hoisted out of the stream loop and held -- spilled, 88 SGPRs -- across the token loop.
    S.kind_[lane] = (uint8_t)lane;
    uint32_t* scr = S.exit_;                    // the build's 64 words (this kernel has no rounds)
    w = (const uint32_t*)to_v((uint64_t)(uintptr_t)w);
    out = (uint8_t*)to_v((uint64_t)(uintptr_t)out);
    items = (const ndfl_batch_item*)to_v((uint64_t)(uintptr_t)items);
    results = (ndfl_batch_result*)to_v((uint64_t)(uintptr_t)results);
    ticket = (uint32_t*)to_v((uint64_t)(uintptr_t)ticket);
    n = to_v(n);
    for (;;) {
        __syncthreads();
        if (lane == 0) s_ticket = atomicAdd(ticket, 1u);
        __syncthreads();
        // (the stream's constants -- its index, item, input view and region -- are parked in vector
        // registers too, like the kernel's arguments: none of them is needed in the token loop's scalars)
        const uint32_t si = to_v((uint32_t)s_ticket);
        if (to_s(si) >= to_s(n)) break;
        ndfl_batch_item it = items[si];
        it.in_off = to_v(it.in_off); it.in_len = to_v(it.in_len);
        it.out_off = to_v(it.out_off); it.out_cap = to_v(it.out_cap);
        const In in = stream_in(w, it.in_off, it.in_len);
        const uint64_t p0 = (it.in_off & 3) * 8;
        Out q;
        q.ring = ring;
        q.obeg = (uint64_t)(uintptr_t)out + it.out_off;
        q.oend = q.obeg + it.out_cap;
        q.o = q.obeg; q.fl = q.obeg; q.npend = 0;
        uint32_t pend = 0;                      // this lane's pending literal
        uint64_t iw0 = NO_STAGE;                // first input word staged in inw
        uint64_t cur = p0;
        uint32_t reason = 0;
        for (;;) {
            park(q, cur, iw0);
            for (uint32_t s = (uint32_t)lane; s < 320; s += 64) S.lens[s] = 0;
            __syncthreads();
            if (lane == 0) {
                Hdr h;
                parse_hdr_core(in, cur, S.lens, S.cl_tab, h);
                hdr_to_shared(h, S);
            }
            __syncthreads();
            reason = __builtin_amdgcn_readfirstlane(S.h_err);
            if (reason) break;
            const uint32_t btype = __builtin_amdgcn_readfirstlane(S.h_btype);
            if (btype == 0) {
                unpark(q, cur, iw0);
                const uint64_t d0 = to_s(S.h_d0);
                const bool bfinal = __builtin_amdgcn_readfirstlane(S.h_bfinal) != 0;
                // stored: a wave-wide copy of the bytes the input still has, then the length check
                flush_pending(q, pend, lane);
                const uint64_t avail = (in.nbits - d0) / 8, ln = to_s(S.h_len);
                const uint64_t take = min(avail, ln), ib = d0 >> 3;
                for (uint64_t done = 0; done < take;) {
                    const uint32_t chunk = (uint32_t)min(take - done, (uint64_t)STORED_STEP);
                    make_room(q, chunk, lane);
                    for (uint32_t i = (uint32_t)lane * 4; i < chunk; i += 256) {
                        const uint64_t b = ib + done + i;
                        const uint64_t two = ((uint64_t)in.ld((b >> 2) + 1) << 32) | in.ld(b >> 2);
                        const uint32_t v = (uint32_t)(two >> (8 * (uint32_t)(b & 3)));
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++)
                            if (i + k < chunk) q.ring[(q.o + i + k) & RMASK] = (uint8_t)(v >> (8 * k));
                    }
                    q.o += chunk;
                    done += chunk;
                    wsync();
                }
                if (take < ln) { reason = R_UEOS; break; }
                cur = d0 + 8 * ln;
                if (bfinal) break;
                continue;
            }
            const int bt = build_block_tables((LShared*)&S, (int)S.kind_[lane], (lu32*)scr);
            reason = __builtin_amdgcn_readfirstlane((uint32_t)bt & 0xFFu);
            if (reason) break;
            const bool ed = __builtin_amdgcn_readfirstlane((uint32_t)bt & 0x100u) != 0;
            unpark(q, cur, iw0);
            const uint64_t d0 = to_s(S.h_d0);
            const bool bfinal = __builtin_amdgcn_readfirstlane(S.h_bfinal) != 0;
            // the wave-uniform token loop
            uint64_t pos = d0;
            bool eob = false;
            while (!eob && !reason) {
                const uint64_t wi = pos >> 5;
                if (wi < iw0 || wi + 3 > iw0 + IW) {
                    wsync();                    // the reads of the words staged before
                    iw0 = wi;
#pragma unroll
                    for (uint32_t k = 0; k < IW / 64; k++) inw[k * 64 + lane] = in.ld(iw0 + k * 64 + lane);
                    wsync();
                }
                const uint32_t r = (uint32_t)(wi - iw0), sh = (uint32_t)pos & 31;
                const uint32_t wa = inw[r], wb = inw[r + 1], wc = inw[r + 2];
                const uint32_t lo = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(wb, wa, sh));
                const uint32_t hi = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(wc, wb, sh));
                const uint32_t e = __builtin_amdgcn_readfirstlane(S.t.lit[lo & ((1u << LB) - 1u)]);
                const uint32_t nb = (uint32_t)min(in.nbits - pos, (uint64_t)0xFFFFFFFFu);
                uint32_t adv = 0;
                Tok tk;
                tok_e<true>(lo, hi, e, adv, S.t, ed, 0xFFFFFFFFu, nb, tk);
                const uint32_t kind = __builtin_amdgcn_readfirstlane(tk.kind);
                const uint32_t val = __builtin_amdgcn_readfirstlane(tk.val);
                const uint32_t tn = __builtin_amdgcn_readfirstlane(tk.n);
                const uint32_t dist = __builtin_amdgcn_readfirstlane(tk.dist);
                pos += to_s(adv);
                if (kind == K_LIT) {
                    add_literal(q, pend, val & 0xFFu, lane);
                    if (tn == 2) add_literal(q, pend, (val >> 8) & 0xFFu, lane);
                } else if (kind == K_LEN) {
                    flush_pending(q, pend, lane);
                    if (dist > q.o - q.obeg) reason = R_COPY_BEFORE;
                    else copy_run(q, tn, dist, lane);
                } else if (kind == K_EOB) {
                    eob = true;
                } else {
                    reason = val;
                }
            }
            if (reason) break;
            cur = pos;
            if (bfinal) break;
        }
        unpark(q, cur, iw0);
        flush_pending(q, pend, lane);
        flush_to(q, q.o, lane);
        if (lane == 0) {
            const uint64_t total = q.o - q.obeg;
            ndfl_batch_result rr;
            rr.status = reason ? (int32_t)reason : total > it.out_cap ? NDFL_E_CAPACITY : 0;
            rr.error_symbol = -1;
            rr.out_len = total;
            rr.consumed_bits = reason ? 0 : cur - p0;
            results[si] = rr;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------
struct BatchScratch {
    void* d_items = nullptr; size_t d_items_cap = 0;   // the items, then the results, then the ticket
    void* d_out = nullptr; size_t d_out_cap = 0;       // host-output staging
    void release() {
        if (d_items) hipFree(d_items);
        if (d_out) hipFree(d_out);
        d_items = d_out = nullptr;
        d_items_cap = d_out_cap = 0;
    }
};

// The batch on stream s (arguments already validated): one launch, one host sync.  results[i].status
// comes back as the kernel wrote it (internal Reason codes; the C ABI maps them).  Host output goes
// through a device staging buffer and only each stream's stored bytes are copied into `out`.
static int inflate_batch_run(InflateScratch& S, BatchScratch& B, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                             const uint8_t* in, uint64_t in_size, uint8_t* out, const ndfl_batch_item* items,
                             ndfl_batch_result* results, uint32_t n, uint32_t flags, double* last_ms) {
    const uint32_t* d_w = nullptr;
    INF_RC(stage_input(S, s, in, in_size, flags, &d_w));
    const size_t items_b = (size_t)n * sizeof(ndfl_batch_item), res_b = (size_t)n * sizeof(ndfl_batch_result);
    INF_CHK(inf_ensure(&B.d_items, &B.d_items_cap, items_b + res_b + 16));
    ndfl_batch_result* d_res = (ndfl_batch_result*)((char*)B.d_items + items_b);
    uint32_t* d_ticket = (uint32_t*)((char*)d_res + res_b);
    INF_CHK(hipMemcpyAsync(B.d_items, items, items_b, hipMemcpyHostToDevice, s));
    INF_CHK(hipMemsetAsync(d_ticket, 0, 16, s));
    // the span of `out` the regions cover (host output: staged on the device)
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!items[i].out_cap) continue;
        lo = std::min(lo, items[i].out_off);
        hi = std::max(hi, items[i].out_off + items[i].out_cap);
    }
    const bool out_dev = (flags & 2u) != 0;
    uint8_t* d_out = out;                        // the kernel's `out` (item offsets are relative to it)
    std::vector<uint8_t> h_span;
    if (!out_dev) {
        if (hi > lo) INF_CHK(inf_ensure(&B.d_out, &B.d_out_cap, hi - lo));
        d_out = (uint8_t*)B.d_out - (hi > lo ? lo : 0);
    }
    static const uint32_t auto_grid = wave_grid(ndfl_inflate_batch_kernel, 256 * 16);
    uint32_t grid = std::min(n, auto_grid);
    if (S.knobs.batch_waves) grid = std::min(grid, S.knobs.batch_waves);
    if (S.knobs.stats) fprintf(stderr, "[ndfl] inflate batch: %u streams, %u waves (of %u)\n", n, grid, auto_grid);
    INF_CHK(hipEventRecord(e0, s));
    hipLaunchKernelGGL(ndfl_inflate_batch_kernel, dim3(grid), dim3(64), 0, s, d_w, d_out, (const ndfl_batch_item*)B.d_items,
                       d_res, n, d_ticket);
    INF_CHK(hipGetLastError());
    INF_CHK(hipEventRecord(e1, s));
    INF_CHK(hipMemcpyAsync(results, d_res, res_b, hipMemcpyDeviceToHost, s));
    if (!out_dev && hi > lo) {
        h_span.resize(hi - lo);
        INF_CHK(hipMemcpyAsync(h_span.data(), B.d_out, hi - lo, hipMemcpyDeviceToHost, s));
    }
    INF_CHK(hipStreamSynchronize(s));
    float ms = 0;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *last_ms = ms;
    if (!out_dev)
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t nb = std::min(results[i].out_len, items[i].out_cap);
            if (nb) memcpy(out + items[i].out_off, h_span.data() + (items[i].out_off - lo), nb);
        }
    return 0;
}
