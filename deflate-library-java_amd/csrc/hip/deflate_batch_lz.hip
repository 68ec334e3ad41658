// deflate_batch_lz.hip -- batched LZ77 deflate: many independent buffers compressed in one launch with
// any Lz77Huffman(dynamic, minRun, maxRun, minDist, maxDist), FULL_* among them
// (ndfl_deflate_batch_lz77, include/ndfl.h).  The LZ77 counterpart of deflate_batch.hip, whose launch
// shape, bit buffer, region stores, checksum folding and stream frame (the ticket claim, the stream's
// start, the header, the end-of-block code, the trailer and the result) it shares (dbat::): a persistent
// grid of one-wave workgroups, an atomic ticket over the stream indices, each stream encoded chunk by
// chunk, serially, by one wave that waits on no other.
//
// ndfl_deflate_chunks_lz77 searches with three kernels over one staging buffer with one history start
// (LzArgs.vstart).  Here a wave carries its stream's history itself: the hash chains of the stream run
// on across its chunk ends, and a chunk's window starts at its own stream offset
// cs - min(hist_limit, cs), never at a neighbour's bytes.  Per chunk (= block), in steps of 64
// consecutive positions, one lane per position:
//   link    the position's 3-byte prefix is hashed (HBITS bits) and linked to the previous position of
//           the stream in the same bucket through a head table in LDS; positions of one step that share
//           a bucket are resolved in position order by readlane, as ndfl_lz_links_kernel does.  link[q]
//           is a u16 distance (0: none within 32 KiB) in the wave's ring in device memory.
//   search  each lane walks its position's chain nearest-first and keeps strictly longer runs: the loop
//           of ndfl_lz_match_kernel, i.e. the longest run in the window, the smallest distance among
//           equal runs (D/comp/Lz77Huffman.java:68-90).  Bytes are read from `in`.
//   parse   the greedy parse chases through the 64 results with readlane; a run that ends past the step
//           carries the next parse position into the next step (a run is capped at the chunk's end).
//           Each token (run << 16 | dist - 1, or the literal) goes to the wave's token list in device
//           memory and, for dynamic codes, into the LDS histograms.
// then build_block_codes<64, true>, the header, and the tokens again, 64 a step: each lane's bits
// counted, wave-scanned and put into the LDS bit buffer (a token is <= 48 bits).
// The input's checksum is folded in a walk of its own over the chunk (16 bytes per lane, as
// dbat::walk_chunk folds it).
//
// Device memory of a wave (owned by the context, BatchLzScratch): the link ring and the token list.
// The same wave writes and reads them, other lanes' values after a __syncthreads() (a workgroup-scope
// fence: one CU, one vector L1).
//
// No scratch memory: everything is forced inline, no per-lane array is indexed by a variable, and the
// lane index is an opaque_lane() (see deflate_batch.hip).
// D/ = src/io/nayuki/deflate/ in the reference
#pragma once
#include "deflate_batch.hip"

namespace dblz {

using dbat::BitOut;
using dbat::make_room;
using dbat::OBW;
using dbat::rfl;
using dbat::to_s;
using dbat::to_v;

constexpr uint32_t HBITS = 12;                // head table: 4,096 x u16
constexpr uint32_t NHEAD = 1u << HBITS;
constexpr uint32_t HNONE = 0xFFFFu;           // empty head entry
// A head entry is a position's offset from a base that follows the stream: when a step starts REBASE_AT
// or more past the base, the base moves up by REBASE and the entries below it are emptied.  Offsets stay
// below REBASE_AT + 2 * 64 < HNONE, and an emptied entry was more than 32,768 before the step.
constexpr uint32_t REBASE_AT = 49152, REBASE = 16384;
constexpr uint32_t MAXD = 32768;              // the largest distance
constexpr uint32_t RING_MAX = 65536;          // link ring entries (a power of two >= MAXD + 64)
static_assert(REBASE_AT + 128 < HNONE && REBASE_AT - REBASE >= MAXD && RING_MAX >= MAXD + 64, "head offsets and ring");
static_assert(31 + 64 * 48 <= 32 * OBW, "a step of 64 tokens fits the flushed bit buffer");

__device__ __forceinline__ uint32_t hash3(uint32_t k) { return (k * 2654435761u) >> (32 - HBITS); }

struct Args : dbat::FrameArgs {
    uint32_t hist_limit;
    int32_t dynamic;
    uint32_t min_run, max_run, min_dist, max_dist;    // 3 <= min_run <= max_run <= 258, 1 <= min_dist <= max_dist <= 32768
    const uint32_t* crc_tab;  // slicing-by-4 tables (1024 u32), then x^(8k) k<64, then x^(8*64k) k<1024
    uint16_t* ring;           // ring_mask + 1 links per wave
    uint32_t ring_mask;       // entries - 1: RING_MAX - 1, or a power of two >= the longest in_len, - 1
    uint32_t* toks;           // tok_cap tokens per wave
    uint32_t tok_cap;         // >= min(chunk_len, longest in_len)
};

// LDS of one wave: 20,824 bytes, 7 waves per CU (160 KiB / 20,824 = 7.87).
struct Lds : dbat::Lds {      // (HuffScr first, the codes, the bit buffer, the ticket)
    uint16_t head[NHEAD];     // bucket -> offset of its last position from the base, or HNONE
};

struct Search {
    uint32_t min_run, max_run, min_dist, max_dist;
};

// Bytes [r, r + 4) of P, zero from P + rend on (nothing at or past P + rend is read).
__device__ __forceinline__ uint32_t ld4(const uint8_t* P, uint32_t r, uint32_t rend) {
    uint32_t w = 0;
    if (r + 4 <= rend) {
        __builtin_memcpy(&w, P + r, 4);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (r + k < rend) w |= (uint32_t)P[r + k] << (8 * k);
    }
    return w;
}

// The chunk's bytes into the checksum ck (kind: NDFL_SUM_*): the steps and the folding of
// dbat::walk_chunk<true>.
__device__ __forceinline__ void fold_chunk(uint64_t v_tab, const uint8_t* cp, uint32_t len_c, uint32_t kind, uint32_t& ck) {
    if (kind == NDFL_SUM_NONE) return;
    for (uint32_t sb = 0; sb < len_c; sb += dbat::STEP) dbat::fold_step(v_tab, kind, dbat::load_step(cp, len_c, sb), ck);
}

// Link, search and parse of one chunk.  Positions are window-relative: P = the stream's byte at offset
// hs = cs - min(hist_limit, cs), the chunk starts at rc0 = cs - hs, P + rend ends what may be read (the
// stream's end, or a few bytes past the chunk's).  hsm = (uint32_t)hs: the ring slot of position r is
// (hsm + r) & mask.  cb = cs - the head table's base, carried from chunk to chunk.  Returns the number
// of tokens stored in toks[].
// PART: the whole of it (LZ_ALL), or one of its two halves for a caller that searches a chunk more than
// once (deflate_batch_multi.hip): LZ_LINK links the chunk's positions (head table, ring, rebase; cb is
// used and nothing else, returns 0), LZ_SEARCH searches and parses a chunk whose positions are all linked
// already (cb is not used).  Linking a chunk twice would link its positions to their own later entries
// in the head table.  With the whole chunk linked before its first position is searched, the ring must
// hold the chunk and its window at once: mask + 1 >= min(the stream, hist_limit + the chunk's length).
constexpr int LZ_ALL = 0, LZ_LINK = 1, LZ_SEARCH = 2;
template <int PART = LZ_ALL>
__device__ __forceinline__ uint32_t lz_chunk(Lds& S, const Search& sp, const uint8_t* P, uint32_t rc0, uint32_t len_c,
                                             uint32_t rend, uint32_t hsm, uint16_t* ring, uint32_t mask, uint32_t* toks,
                                             bool dyn, uint32_t& cb) {
    uint32_t pos = 0;                         // the next parse position (chunk-relative, <= len_c)
    uint32_t ntok = 0;
    for (uint32_t sb = 0; sb < len_c; sb += 64) {
        const int lane = opaque_lane();
        const uint32_t t = sb + (uint32_t)lane;
        const bool inb = t < len_c;
        const uint32_t ri = rc0 + t;
        if constexpr (PART != LZ_SEARCH) {
            if (cb + sb >= REBASE_AT) {       // (a step adds 64: one move keeps cb + sb below REBASE_AT)
                for (uint32_t k = (uint32_t)lane; k < NHEAD; k += 64) {
                    const uint32_t v = S.head[k];
                    S.head[k] = (uint16_t)((v != HNONE && v >= REBASE) ? v - REBASE : HNONE);
                }
                cb -= REBASE;
                __syncthreads();
            }
        }
        // ---- link: the stream's last two positions have no 3-byte prefix and are not linked -------
        const uint32_t wi0 = inb ? ld4(P, ri, rend) : 0u;
        uint32_t d = 0;
        if constexpr (PART != LZ_SEARCH) {
            const bool hasp = inb && ri + 2 < rend;
            uint32_t h = 0x10000u + (uint32_t)lane;               // a bucket of its own
            if (hasp) h = hash3(wi0 & 0xFFFFFFu);
            int prevLane = -1;
            bool last = true;
            // (every compare below is a lane mask in a scalar pair.  LZ_LINK is inlined into a kernel with
            // more live scalar state than this file's: keep its scan at 4, or that kernel spills SGPRs)
            constexpr int UNROLL = PART == LZ_LINK ? 4 : 8;
#pragma unroll UNROLL
            for (int k = 0; k < 64; k++) {
                const uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)h, k);
                const bool eq = hk == h;
                if (eq && k < lane) prevLane = k;
                if (eq && k > lane) last = false;
            }
            const uint32_t off = cb + t;
            if (hasp) {
                if (prevLane >= 0) {
                    d = (uint32_t)(lane - prevLane);
                } else {
                    const uint32_t hv = S.head[h];
                    if (hv != HNONE) { d = off - hv; if (d > MAXD) d = 0; }
                }
            }
            if (hasp && last) S.head[h] = (uint16_t)off;          // (one wave: after every lane's read above)
            if (inb) ring[(hsm + ri) & mask] = (uint16_t)d;
            __syncthreads();                                      // the step's links, for every lane
            if constexpr (PART == LZ_LINK) continue;
        } else {
            if (inb) d = ring[(hsm + ri) & mask];                 // (linked before: the caller's LZ_LINK pass)
        }
        // ---- search (ndfl_lz_match_kernel's walk) --------------------------------------------------
        // The walk reads link[rj] for rlo <= rj <= ri only.  Those positions are this stream's, all of
        // them linked by now (the stream is linked in order, this step included), and none of their
        // slots has been written again: the newest link is at most 32,768 + 63 past rlo, less than the
        // ring (or the ring holds the whole stream).  So no link of an earlier stream or an earlier lap
        // is read; and whatever a link held, a hop is followed only while it stays at or above rlo.
        const uint32_t maxlen = inb ? min(sp.max_run, len_c - t) : 0u;
        const int32_t lo_s = max((int32_t)ri - (int32_t)sp.max_dist, 0);
        const int32_t hi_s = (int32_t)ri - (int32_t)sp.min_dist;
        const uint32_t rlo = (uint32_t)lo_s, rhi = (uint32_t)hi_s;    // (rhi is used only when hi_s >= lo_s)
        bool act = inb && t >= pos && maxlen >= sp.min_run && hi_s >= lo_s;   // (positions before pos are inside a run)
        uint32_t best = 0, bestd = 0, want = 0, rj = ri;
        // Bound: a pass ends the lane's walk or lowers rj by d >= 1, and rj stays >= rlo >= ri - 32,768:
        // at most 32,768 passes.  The compare loop adds 4 to k up to maxlen <= 258.
        while (act) {
            if (d == 0 || d > rj - rlo) break;
            rj -= d;
            d = ring[(hsm + rj) & mask];
            if (rj > rhi) continue;                               // nearer than min_dist: only the hop
            const uint32_t x0 = ld4(P, rj, rend) ^ wi0;
            const uint32_t sbyte = P[rj + best];                  // (rj + best < ri + maxlen <= the chunk's end)
            if ((x0 & 0xFFFFFFu) == 0 && (best < 3 || sbyte == want)) {   // can be longer
                uint32_t run;
                if (x0) run = 3;
                else {
                    uint32_t k = 4;
                    for (;;) {
                        if (k >= maxlen) { run = maxlen; break; }
                        const uint32_t y = ld4(P, rj + k, rend) ^ ld4(P, ri + k, rend);
                        if (y) { run = k + ((uint32_t)__builtin_ctz(y) >> 3); break; }
                        k += 4;
                    }
                }
                run = min(run, maxlen);
                if (run > best) {
                    best = run;
                    bestd = ri - rj;
                    if (best >= maxlen) break;
                    want = P[ri + best];
                }
            }
        }
        const bool isrun = best >= sp.min_run;
        const uint32_t m = isrun ? (best << 16 | (bestd - 1)) : (wi0 & 0xFFu);
        const uint32_t stp = isrun ? best : 1u;
        // ---- parse: from pos through the step's results (at most 64 hops: each adds >= 1) -----------
        const uint32_t lim = min(64u, len_c - sb);
        uint32_t pp = rfl(pos - sb);                              // (pos >= sb: the step before ended at or past it)
        uint64_t tm = 0;                                          // bit i: a token starts at lane i
        while (pp < lim) {
            tm |= 1ull << pp;
            pp += (uint32_t)__builtin_amdgcn_readlane((int)stp, (int)pp);
            pp = rfl(pp);
        }
        pos = sb + pp;
        if ((tm >> lane) & 1ull) {
            toks[ntok + (uint32_t)__builtin_popcountll(tm & ((1ull << lane) - 1ull))] = m;
            if (dyn) {
                if (!isrun) atomicAdd(&S.scr.hlit[m], 1u);
                else {
                    uint32_t sym, ne, ex;
                    run_sym(best, sym, ne, ex);
                    atomicAdd(&S.scr.hlit[sym], 1u);
                    dist_sym(bestd - 1, sym, ne, ex);
                    atomicAdd(&S.scr.hdist[sym], 1u);
                }
            }
        }
        ntok += (uint32_t)__builtin_popcountll(tm);
    }
    return ntok;
}

// The chunk's tokens into the bit buffer, 64 a step.
__device__ __forceinline__ void emit_tokens(Lds& S, BitOut& bo, const uint32_t* toks, uint32_t ntok) {
    for (uint32_t i0 = 0; i0 < ntok; i0 += 64) {
        const int lane = opaque_lane();
        uint32_t c0 = 0, l0 = 0, ex1 = 0, ne1 = 0, c2 = 0, l2 = 0, ex3 = 0, ne3 = 0;
        if (i0 + (uint32_t)lane < ntok) {
            const uint32_t m = toks[i0 + (uint32_t)lane];
            const uint32_t run = m >> 16;
            if (!run) {
                const uint32_t e = S.litCode[m & 0xFFu];
                c0 = e & 0xFFFFu; l0 = e >> 16;
            } else {
                uint32_t sym;
                run_sym(run, sym, ne1, ex1);
                const uint32_t e = S.litCode[sym];
                c0 = e & 0xFFFFu; l0 = e >> 16;
                dist_sym(m & 0xFFFFu, sym, ne3, ex3);
                const uint32_t f = S.distCode[sym];
                c2 = f & 0xFFFFu; l2 = f >> 16;
            }
        }
        const uint32_t mybits = l0 + ne1 + l2 + ne3;              // <= 15 + 5 + 15 + 13
        const uint32_t incl = wave_incl_scan_l(mybits, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        make_room(bo, total);
        BitPut bp; bp.init(bo.obuf, bo.fill + incl - mybits);
        bp.put(c0, l0);
        bp.put(ex1, ne1);
        bp.put(c2, l2);
        bp.put(ex3, ne3);
        bp.flush();
        bo.fill += total;
    }
}

// For the callers that size a block before they emit it (deflate_batch_multi.hip, deflate_batch_binsplit.hip).
// The bits of the block's tokens and its end-of-block code under the codes in S.litCode / S.distCode,
// from the histograms (hdist0: the distances before the builder's dummy neighbour).
__device__ __forceinline__ uint32_t token_bits(Lds& S) {
    const int lane = opaque_lane();
    uint32_t b = 0;
    for (uint32_t t = (uint32_t)lane; t < 288; t += 64) {
        const uint32_t ex = (t < 265 || t >= 285) ? 0u : (t - 261) >> 2;      // extra bits of a length symbol
        b += S.scr.hlit[t] * ((S.litCode[t] >> 16) + ex);
    }
    if (lane < 30) {
        const uint32_t ex = lane < 4 ? 0u : ((uint32_t)lane - 2) >> 1;        // of a distance symbol
        b += S.scr.hdist0[lane] * ((S.distCode[lane] >> 16) + ex);
    }
    return rfl(dbat::wave_sum_l(b, lane));
}

}  // namespace dblz

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_batch_lz_kernel(dblz::Args a) {
    using namespace dblz;
    __shared__ __attribute__((aligned(16))) Lds S;
    // the arguments are needed once per stream or per chunk: parked (dbat::to_v)
    const dbat::Frame f = dbat::park_frame(a);
    const uint64_t v_tab = to_v((uint64_t)(uintptr_t)a.crc_tab);
    const uint64_t v_ring = to_v((uint64_t)(uintptr_t)(a.ring + (size_t)blockIdx.x * ((size_t)a.ring_mask + 1)));
    const uint64_t v_toks = to_v((uint64_t)(uintptr_t)(a.toks + (size_t)blockIdx.x * a.tok_cap));
    const uint32_t v_mask = to_v(a.ring_mask);
    const uint32_t v_hist = to_v(a.hist_limit);
    const uint32_t v_dyn = to_v((uint32_t)(a.dynamic != 0));
    const uint32_t v_minr = to_v(a.min_run), v_maxr = to_v(a.max_run), v_mind = to_v(a.min_dist), v_maxd = to_v(a.max_dist);
    for (;;) {
        dbat::Stream st;
        if (!dbat::claim_stream(S, f, st)) break;
        // the running state, all of it started afresh for the stream: checksum and bit buffer (begin_stream),
        // head table and its base (the ring needs no clearing: lz_chunk reads only links this stream has written)
        BitOut bo = dbat::begin_stream(S, f, st);
        uint32_t v_fill = to_v(0u), v_cb = to_v(0u);
        uint64_t v_cs = to_v((uint64_t)0);
        for (uint32_t j = (uint32_t)opaque_lane(); j < NHEAD / 2; j += 64) ((uint32_t*)S.head)[j] = HNONE << 16 | HNONE;
        for (;;) {
            if (to_s(v_dyn)) dbat::begin_block_hist(S);
            __syncthreads();
            uint32_t v_ntok;
            {
                const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), len - cs);
                const uint64_t hs = cs - min((uint64_t)to_s(v_hist), cs);      // chunk 0 has no history
                const uint8_t* P = (const uint8_t*)(uintptr_t)(to_s(st.v_src) + hs);
                const uint32_t rc0 = (uint32_t)(cs - hs);
                const uint32_t rend = (uint32_t)min(len - hs, (uint64_t)rc0 + len_c + 8);
                uint32_t ck = to_s(st.v_ck);
                fold_chunk(v_tab, P + rc0, len_c, to_s(st.v_kind), ck);
                st.v_ck = to_v(ck);
                const Search sp{to_s(v_minr), to_s(v_maxr), to_s(v_mind), to_s(v_maxd)};
                uint32_t cb = to_s(v_cb);
                v_ntok = to_v(lz_chunk(S, sp, P, rc0, len_c, rend, (uint32_t)hs, (uint16_t*)(uintptr_t)to_s(v_ring),
                                       to_s(v_mask), (uint32_t*)(uintptr_t)to_s(v_toks), to_s(v_dyn) != 0, cb));
                v_cb = to_v(cb + len_c);
                if (to_s(v_dyn)) dbat::end_block_hist(S, len_c);
            }
            __syncthreads();                                          // the histograms and the token list
            uint32_t hb;
            {
                const uint64_t len = to_s(st.v_len), cs = to_s(v_cs);
                const bool is_final = len - cs <= (uint64_t)to_s(f.v_chunk_len);
                hb = build_block_codes<64, true>(S.scr, to_s(v_dyn) != 0, is_final, S.litCode, S.distCode);
            }
            bo.fill = to_s(v_fill);
            dbat::put_header(S, bo, hb);
            emit_tokens(S, bo, (const uint32_t*)(uintptr_t)to_s(v_toks), to_s(v_ntok));
            {
                const uint64_t cs = to_s(v_cs);
                v_cs = to_v(cs + min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs));
            }
            dbat::put_eob(S, bo);
            v_fill = to_v(bo.fill);
            if (to_s(v_cs) >= to_s(st.v_len)) break;
        }
        dbat::finish_stream(f, st, bo, v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// The link rings and token lists of the grid's waves: grown on demand, kept by the context.
struct BatchLzScratch {
    void* d_mem = nullptr; size_t d_mem_cap = 0;
    void release() {
        if (d_mem) hipFree(d_mem);
        d_mem = nullptr;
        d_mem_cap = 0;
    }
};

// The most device memory the rings and token lists may take; the grid is lowered to fit.  A wave needs
// at most 128 KiB of links and 256 KiB of tokens, so the budget never leaves fewer than 682 waves.
// deflate_batch_multi.hip's BatchMultiLaunch shares the scratch and the budget: a wave of its kernel
// needs at most 256 KiB of links and two token lists of 256 KiB, so never fewer than 341 waves.
constexpr size_t BATCH_LZ_BUDGET = (size_t)256 << 20;

// batch_run's launcher for ndfl_deflate_batch_lz_kernel.
struct BatchLzLaunch {
    BatchLzScratch& Z;
    const Knobs& knobs;
    const ndfl_member_item* items;       // host
    dblz::Args a;                         // n, chunk_len, hist_limit, dynamic, the search parameters, crc_tab;
                                          //   deflate_batch_run sets `in`
    uint32_t grid = 0;
    // Before the launch is timed: sizes the wave's ring and token list from the batch, lowers the grid to
    // the budget and grows the scratch (first use only).
    int prepare() {
        uint64_t longest = 0;
        for (uint32_t i = 0; i < a.n; i++) longest = std::max(longest, items[i].in_len);
        uint32_t ring = 64;
        while (ring < dblz::RING_MAX && ring < longest) ring <<= 1;
        a.tok_cap = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(a.chunk_len, longest));
        const size_t per_wave = (size_t)ring * 2 + (size_t)a.tok_cap * 4;
        grid = batch_grid<ndfl_deflate_batch_lz_kernel>(a.n, knobs, "deflate batch lz77", per_wave, BATCH_LZ_BUDGET);
        INF_CHK(inf_ensure(&Z.d_mem, &Z.d_mem_cap, (size_t)grid * per_wave));
        a.toks = (uint32_t*)Z.d_mem;
        a.ring = (uint16_t*)((char*)Z.d_mem + (size_t)grid * a.tok_cap * 4); a.ring_mask = ring - 1;
        return 0;
    }
    int operator()(hipStream_t s, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                   uint32_t* d_ticket) {
        a.out = d_out; a.items = d_items; a.results = d_res; a.ticket = d_ticket;
        hipLaunchKernelGGL(ndfl_deflate_batch_lz_kernel, dim3(grid), dim3(64), 0, s, a);
        return 0;
    }
};
