// deflate_batch_lz.hip -- batched LZ77 deflate: many independent buffers compressed in one launch with
// any Lz77Huffman(dynamic, minRun, maxRun, minDist, maxDist), FULL_* among them
// (ndfl_deflate_batch_lz77, include/ndfl.h), and dblz::, the chunk layer that the three LZ batch kernels
// share (this one, deflate_batch_multi.hip, deflate_batch_binsplit.hip).  Launch shape, bit buffer, region
// stores, checksum folding and stream frame are deflate_batch.hip's (dbat::).
//
// ndfl_deflate_chunks_lz77 searches with three kernels over one staging buffer with one history start
// (LzArgs.vstart).  Here a wave carries its stream's history itself: the hash chains of the stream run
// on across its chunk ends, and a chunk's window starts at its own stream offset
// cs - min(hist_limit, cs), never at a neighbour's bytes.  Per chunk, in steps of 64 consecutive
// positions, one lane per position (lz_chunk):
//   link    the position's 3-byte prefix is hashed (HBITS bits) and linked to the previous position of
//           the stream in the same bucket through a head table in LDS; positions of one step that share
//           a bucket are resolved in position order by readlane, as ndfl_lz_links_kernel does.  link[q]
//           is a u16 distance (0: none within 32 KiB) in the wave's ring in device memory.
//   search  each lane walks its position's chain nearest-first and keeps strictly longer runs: the loop
//           of ndfl_lz_match_kernel, i.e. the longest run in the window, the smallest distance among
//           equal runs (D/comp/Lz77Huffman.java:68-90).  Bytes are read from `in`.
//   parse   the greedy parse chases through the 64 results with readlane; a run that ends past the step
//           carries the next parse position into the next step (a run is capped at the range's end).
//           Each token (run << 16 | dist - 1, or the literal) goes to a token list in device memory
//           and, for dynamic codes, into the LDS histograms.
// A block is then build_block_codes<64, true>, the header, and the tokens again, 64 a step: each lane's
// bits counted, wave-scanned and put into the LDS bit buffer (a token is <= 48 bits).
//
// The chunk layer, all of it forced inline, in the order a kernel uses it:
//   LzArgs, Wave, park_wave     the arguments the three kernels share, parked per wave (as dbat::park_frame);
//   LzState, begin_lz           the stream's running state (bit fill, head table base, chunk start), afresh;
//   chunk_view                  the chunk's geometry from the parked values: the ONE place that knows where
//                               a chunk's window starts and what may be read.  Recomputed at every use;
//   fold_chunk, fold_and_link   the chunk's bytes into the checksum; its positions linked whole;
//   search_block, size_block    a range of a linked chunk as one block: tokens and histograms, then its
//                               codes, header and exact size in bits;
//   emit_block                  header, tokens, end of block;
//   advance_chunk               the next chunk, if the stream has one.
// This kernel links as it searches (lz_chunk<LZ_ALL>); the other two link a chunk whole (fold_and_link)
// and then search it, or ranges of it, as often as they need (search_block).
//
// Device memory of a wave (BatchLzScratch; batch_lz_sizes below has the sizes and the minimum grid): the
// link ring and the token lists.  The same wave writes and reads them, other lanes' values after a
// __syncthreads() (a workgroup-scope fence: one CU, one vector L1).
//
// No scratch memory: everything is forced inline, no per-lane array is indexed by a variable, the lane
// index is an opaque_lane() in every step, wave-uniform state is parked (dbat::to_v).
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
// The most link ring entries (powers of two) under the two ways a chunk is linked.  As it is searched,
// step by step: a walk reaches MAXD back from a step of 64.  Whole, before its first position is searched:
// the ring holds the chunk and its window at once, 65,536 + MAXD.
constexpr uint32_t RING_STREAMED_MAX = 65536, RING_WHOLE_MAX = 131072;
static_assert(REBASE_AT + 128 < HNONE && REBASE_AT - REBASE >= MAXD, "head offsets");
static_assert(RING_STREAMED_MAX >= MAXD + 64 && RING_WHOLE_MAX >= MAXD + 65536, "ring");
static_assert(31 + 64 * 48 <= 32 * OBW, "a step of 64 tokens fits the flushed bit buffer");

__device__ __forceinline__ uint32_t hash3(uint32_t k) { return (k * 2654435761u) >> (32 - HBITS); }

// What every LZ batch kernel is given after the frame's arguments (sized by batch_lz_sizes, below).
struct LzArgs : dbat::FrameArgs {
    uint32_t hist_limit;
    const uint32_t* crc_tab;  // slicing-by-4 tables (1024 u32), then x^(8k) k<64, then x^(8*64k) k<1024
    uint16_t* ring;           // ring_mask + 1 links per wave
    uint32_t ring_mask;       // entries - 1
    uint32_t* toks;           // the wave's token lists, tok_cap tokens each
    uint32_t tok_cap;         // >= min(chunk_len, longest in_len)
};

struct Args : LzArgs {
    int32_t dynamic;
    uint32_t min_run, max_run, min_dist, max_dist;    // 3 <= min_run <= max_run <= 258, 1 <= min_dist <= max_dist <= 32768
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

// Link, search and parse of one chunk, or of a range of it.  Positions are window-relative (chunk_view,
// below): P = the stream's byte at the window's start hs, the range starts at rc0, P + rend ends what may
// be read.  hsm = (uint32_t)hs: the ring slot of position r is (hsm + r) & mask.  cb = the chunk's start -
// the head table's base, carried from chunk to chunk.  Returns the number of tokens stored in toks[].
// PART: the whole of it (LZ_ALL), or one of its two halves for a caller that searches a chunk more than
// once: LZ_LINK links the chunk's positions (head table, ring, rebase; cb is used and nothing else,
// returns 0), LZ_SEARCH searches and parses a range whose chunk is linked already (cb is not used).
// Linking a chunk twice would link its positions to their own later entries in the head table.  With the
// whole chunk linked before its first position is searched, the ring must hold the chunk and its window
// at once: mask + 1 >= min(the stream, hist_limit + the chunk's length).
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

// ---- the chunk layer --------------------------------------------------------------------------------
// The wave's part of LzArgs.  Needed once per chunk or per block: parked (dbat::to_v).  n_lists: the token
// lists a wave of the kernel has.
struct Wave {
    uint64_t v_tab, v_ring, v_toks;
    uint32_t v_mask, v_hist;
};
__device__ __forceinline__ Wave park_wave(const LzArgs& a, uint32_t n_lists) {
    Wave w;
    w.v_tab = to_v((uint64_t)(uintptr_t)a.crc_tab);
    w.v_ring = to_v((uint64_t)(uintptr_t)(a.ring + (size_t)blockIdx.x * ((size_t)a.ring_mask + 1)));
    w.v_toks = to_v((uint64_t)(uintptr_t)(a.toks + (size_t)blockIdx.x * n_lists * a.tok_cap));
    w.v_mask = to_v(a.ring_mask);
    w.v_hist = to_v(a.hist_limit);
    return w;
}
__device__ __forceinline__ uint16_t* ring_of(const Wave& w) { return (uint16_t*)(uintptr_t)to_s(w.v_ring); }
__device__ __forceinline__ uint32_t* toks_of(const Wave& w) { return (uint32_t*)(uintptr_t)to_s(w.v_toks); }

// The stream's running state, parked across the code construction: the bit buffer's fill after the last
// block, the chunk's start cs and cb = cs - the head table's base.
struct LzState {
    uint32_t v_fill, v_cb;
    uint64_t v_cs;
};
// All of it started afresh for a stream, the head table emptied (the ring needs no clearing: lz_chunk
// reads only links this stream has written).
__device__ __forceinline__ LzState begin_lz(Lds& S) {
    LzState z;
    z.v_fill = to_v(0u); z.v_cb = to_v(0u);
    z.v_cs = to_v((uint64_t)0);
    for (uint32_t j = (uint32_t)opaque_lane(); j < NHEAD / 2; j += 64) ((uint32_t*)S.head)[j] = HNONE << 16 | HNONE;
    return z;
}

// The current chunk: its len_c bytes start at stream offset cs = v_cs, its window at hs = cs - min(hist_limit, cs)
// (chunk 0 has no history, and no chunk sees a neighbour's bytes).  P = the stream's byte at hs; the chunk is
// P[rc0, rc0 + len_c), and P + rend ends what may be read: the stream's end, or a few bytes past the chunk's.
// is_final: the stream's last chunk.
// Scalars, derived from parked values: call it again wherever the view is needed, and carry it across no
// code construction and no search, so that nothing wave-uniform stays live in SGPRs there (dbat::to_v).
struct ChunkView {
    uint32_t len_c;
    uint64_t hs;
    const uint8_t* P;
    uint32_t rc0, rend;
    bool is_final;
};
__device__ __forceinline__ ChunkView chunk_view(const dbat::Frame& f, const dbat::Stream& st, const Wave& w, uint64_t v_cs) {
    const uint64_t cs = to_s(v_cs), len = to_s(st.v_len), chunk_len = (uint64_t)to_s(f.v_chunk_len);
    const uint32_t v_hist = w.v_hist;
    ChunkView c;
    c.len_c = (uint32_t)min(chunk_len, len - cs);
    c.hs = cs - min((uint64_t)to_s(v_hist), cs);
    c.P = (const uint8_t*)(uintptr_t)(to_s(st.v_src) + c.hs);
    c.rc0 = (uint32_t)(cs - c.hs);
    c.rend = (uint32_t)min(len - c.hs, (uint64_t)c.rc0 + c.len_c + 8);
    c.is_final = len - cs <= chunk_len;
    return c;
}

// The chunk's bytes into the stream's checksum: the steps and the folding of dbat::walk_chunk<true>.
__device__ __forceinline__ void fold_chunk(const Wave& w, dbat::Stream& st, const ChunkView& c) {
    const uint32_t kind = to_s(st.v_kind);
    if (kind == NDFL_SUM_NONE) return;
    uint32_t ck = to_s(st.v_ck);
    for (uint32_t sb = 0; sb < c.len_c; sb += dbat::STEP)
        dbat::fold_step(w.v_tab, kind, dbat::load_step(c.P + c.rc0, c.len_c, sb), ck);
    st.v_ck = to_v(ck);
}

// A chunk that is searched more than once: folded, and (link: some search has a distance in its window,
// a literal-only one follows no link) its positions linked, whole, before any of them is searched.
__device__ __forceinline__ void fold_and_link(Lds& S, const dbat::Frame& f, dbat::Stream& st, const Wave& w, LzState& z,
                                              bool link) {
    const ChunkView c = chunk_view(f, st, w, z.v_cs);
    fold_chunk(w, st, c);
    if (link) {
        const Search none{0u, 0u, 0u, 0u};
        uint32_t cb = to_s(z.v_cb);
        lz_chunk<LZ_LINK>(S, none, c.P, c.rc0, c.len_c, c.rend, (uint32_t)c.hs, ring_of(w), to_s(w.v_mask), nullptr, true, cb);
        z.v_cb = to_v(cb + c.len_c);
    }
}

// Bytes [a, a + n) of the chunk (a + n <= len_c).
struct Range {
    uint32_t a, n;
};

// A range of the chunk (linked whole: fold_and_link) as one block, first half: its tokens under sp into
// toks[] and the histograms, hdist copied to hdist0, because the code builder gives a single used distance
// code a dummy neighbour.  Returns the number of tokens.  Any number of size_block()s may follow.
__device__ __forceinline__ uint32_t search_block(Lds& S, const dbat::Frame& f, const dbat::Stream& st, const Wave& w,
                                                 uint64_t v_cs, const Search& sp, const Range& r, uint32_t* toks) {
    dbat::begin_block_hist(S);
    __syncthreads();
    const ChunkView c = chunk_view(f, st, w, v_cs);
    uint32_t nocb = 0;
    const uint32_t ntok = lz_chunk<LZ_SEARCH>(S, sp, c.P, c.rc0 + r.a, r.n, c.rend, (uint32_t)c.hs, ring_of(w), to_s(w.v_mask),
                                              toks, true, nocb);
    dbat::end_block_hist(S, r.n);
    __syncthreads();                                              // the histograms and the token list
    {
        const int lane = opaque_lane();
        if (lane < 32) S.scr.hdist0[lane] = S.scr.hdist[lane];
    }
    __syncthreads();
    return ntok;
}

// Second half: the codes of the block whose histograms are in place (static: the fixed codes) into
// S.litCode / S.distCode, its header into S.scr.hdr(), and (parked) the header's bits and the block's exact
// size: the header plus, from the histograms, count x (code length + extra bits), end of block included.
// An empty block's dummy literal is counted and not emitted: taken off again.
struct BlockSize {
    uint32_t v_hb, v_bits;
};
__device__ __forceinline__ BlockSize size_block(Lds& S, bool dynamic, bool is_final, bool empty) {
    BlockSize b;
    b.v_hb = to_v(build_block_codes<64, true>(S.scr, dynamic, is_final, S.litCode, S.distCode));
    b.v_bits = to_v(to_s(b.v_hb) + token_bits(S) - (empty ? rfl(S.litCode[0]) >> 16 : 0u));
    return b;
}

// The block in place (header words, codes) with its tokens into the bit buffer.
__device__ __forceinline__ void emit_block(Lds& S, BitOut& bo, uint32_t hb, const uint32_t* toks, uint32_t ntok) {
    dbat::put_header(S, bo, hb);
    emit_tokens(S, bo, toks, ntok);
    dbat::put_eob(S, bo);
}

// On to the next chunk; false when the stream has none.
__device__ __forceinline__ bool advance_chunk(const dbat::Frame& f, const dbat::Stream& st, const Wave& w, LzState& z) {
    z.v_cs = to_v(to_s(z.v_cs) + chunk_view(f, st, w, z.v_cs).len_c);
    return to_s(z.v_cs) < to_s(st.v_len);
}

}  // namespace dblz

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_batch_lz_kernel(dblz::Args a) {
    using namespace dblz;
    __shared__ __attribute__((aligned(16))) Lds S;
    const dbat::Frame f = dbat::park_frame(a);
    const Wave w = park_wave(a, 1);
    const uint32_t v_dyn = to_v((uint32_t)(a.dynamic != 0));
    const uint32_t v_minr = to_v(a.min_run), v_maxr = to_v(a.max_run), v_mind = to_v(a.min_dist), v_maxd = to_v(a.max_dist);
    for (;;) {
        dbat::Stream st;
        if (!dbat::claim_stream(S, f, st)) break;
        BitOut bo = dbat::begin_stream(S, f, st);
        LzState z = begin_lz(S);
        do {
            // ---- the chunk: folded, then linked, searched and parsed in one pass -------------------------
            if (to_s(v_dyn)) dbat::begin_block_hist(S);
            __syncthreads();
            uint32_t v_ntok;
            {
                const ChunkView c = chunk_view(f, st, w, z.v_cs);
                fold_chunk(w, st, c);
                const Search sp{to_s(v_minr), to_s(v_maxr), to_s(v_mind), to_s(v_maxd)};
                uint32_t cb = to_s(z.v_cb);
                v_ntok = to_v(lz_chunk(S, sp, c.P, c.rc0, c.len_c, c.rend, (uint32_t)c.hs, ring_of(w), to_s(w.v_mask),
                                       toks_of(w), to_s(v_dyn) != 0, cb));
                z.v_cb = to_v(cb + c.len_c);
                if (to_s(v_dyn)) dbat::end_block_hist(S, c.len_c);
            }
            __syncthreads();                                          // the histograms and the token list
            // ---- its block ------------------------------------------------------------------------------
            const uint32_t hb = build_block_codes<64, true>(S.scr, to_s(v_dyn) != 0, chunk_view(f, st, w, z.v_cs).is_final,
                                                            S.litCode, S.distCode);
            bo.fill = to_s(z.v_fill);
            emit_block(S, bo, hb, toks_of(w), to_s(v_ntok));
            z.v_fill = to_v(bo.fill);
        } while (advance_chunk(f, st, w, z));
        dbat::finish_stream(f, st, bo, z.v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// The link rings and token lists of the grid's waves: grown on demand, kept by the context.
struct BatchLzScratch {
    DevBuf d_mem;
    void release() { d_mem.release(); }
};

// The most device memory the rings and token lists may take; the grid is lowered to fit.
constexpr size_t BATCH_LZ_BUDGET = (size_t)256 << 20;

// A wave's memory for a batch whose longest stream has `longest` bytes: n_lists token lists of tok_cap
// tokens (a chunk's tokens: one per byte at most, 64 at least) and a ring of `ring` links, a power of two
// from 64 on.  A kernel that links a chunk as it searches it needs the stream, or RING_STREAMED_MAX links;
// one that links it whole first (linked_whole) the chunk and its window at once,
// min(longest, hist_limit + chunk_len), or RING_WHOLE_MAX.  No list (n_lists 0: nothing is searched): no
// memory.
//   per wave, at most    streamed, 1 list   whole, 1 list   whole, 2 lists
//   links                128 KiB            256 KiB         256 KiB
//   tokens               256 KiB            256 KiB         512 KiB
//   waves the budget never goes below:  682  512             341
struct BatchLzSizes {
    uint32_t ring, tok_cap;
    size_t per_wave;          // bytes
};
static inline BatchLzSizes batch_lz_sizes(uint64_t longest, uint32_t chunk_len, uint32_t hist_limit, bool linked_whole,
                                          uint32_t n_lists) {
    BatchLzSizes z{64, 0, 0};
    if (!n_lists) return z;
    const uint64_t span = linked_whole ? std::min<uint64_t>(longest, (uint64_t)hist_limit + chunk_len) : longest;
    const uint32_t ring_max = linked_whole ? dblz::RING_WHOLE_MAX : dblz::RING_STREAMED_MAX;
    while (z.ring < ring_max && z.ring < span) z.ring <<= 1;
    z.tok_cap = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(chunk_len, longest));
    z.per_wave = (size_t)z.ring * 2 + (size_t)z.tok_cap * 4 * n_lists;
    return z;
}

// An Lz77Huffman descriptor (validated) as the kernels' search.  The literal-only form searches a window
// with no distance in it: nothing is ever a run.
static inline dblz::Search search_of(const ndfl_strategy_desc& d) {
    if (d.min_run == 0) return dblz::Search{3u, 258u, 1u, 0u};
    return dblz::Search{(uint32_t)d.min_run, (uint32_t)d.max_run, (uint32_t)d.min_dist, (uint32_t)d.max_dist};
}

// batch_run's launcher for an LZ batch kernel: KERNEL(A), A a dblz::LzArgs.  The caller fills a's n,
// chunk_len, hist_limit, crc_tab and what is the kernel's own; deflate_batch_run sets `in`.
template <class A, void (*KERNEL)(A), bool LINKED_WHOLE, uint32_t N_LISTS, const char* LABEL>
struct BatchLzLaunchT {
    BatchLzScratch& Z;
    const Knobs& knobs;
    const ndfl_member_item* items;       // host
    A a;
    uint32_t n_lists = N_LISTS;           // (0: this call searches nothing)
    uint32_t grid = 0;
    // Before the launch is timed: sizes the wave's ring and token lists from the batch, lowers the grid to
    // the budget, grows the scratch (first use only) and carves it: every wave's lists, then every wave's ring.
    int prepare() {
        uint64_t longest = 0;
        for (uint32_t i = 0; i < a.n; i++) longest = std::max(longest, items[i].in_len);
        const BatchLzSizes z = batch_lz_sizes(longest, a.chunk_len, a.hist_limit, LINKED_WHOLE, n_lists);
        grid = batch_grid<KERNEL>(a.n, knobs, LABEL, z.per_wave, BATCH_LZ_BUDGET);
        if (z.per_wave) INF_CHK(Z.d_mem.ensure((size_t)grid * z.per_wave));
        a.tok_cap = z.tok_cap;
        a.toks = Z.d_mem.as<uint32_t>();
        a.ring = (uint16_t*)(Z.d_mem.as<char>() + (size_t)grid * z.tok_cap * 4 * n_lists); a.ring_mask = z.ring - 1;
        return 0;
    }
    int operator()(hipStream_t s, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                   uint32_t* d_ticket) {
        a.out = d_out; a.items = d_items; a.results = d_res; a.ticket = d_ticket;
        hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(64), 0, s, a);
        return 0;
    }
};

static constexpr char BATCH_LZ_LABEL[] = "deflate batch lz77";
using BatchLzLaunch = BatchLzLaunchT<dblz::Args, ndfl_deflate_batch_lz_kernel, false, 1, BATCH_LZ_LABEL>;
