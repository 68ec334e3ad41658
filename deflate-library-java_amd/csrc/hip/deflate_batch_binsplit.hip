// deflate_batch_binsplit.hip -- batched BinarySplit deflate: many independent buffers compressed in one
// launch, every chunk split into the blocks that BinarySplit(Lz77Huffman(...), minBlockLen) of
// D/comp/BinarySplit.java:21-82 chooses (ndfl_deflate_batch_binsplit, include/ndfl.h).  The fourth of the
// batch kernels, with the launch shape of its siblings: a persistent grid of one-wave workgroups, an
// atomic ticket over the stream indices, each stream encoded chunk by chunk, serially, by one wave that
// waits on no other.  The stream frame, the bit buffer, the region stores and the checksum folding are
// deflate_batch.hip's (dbat::), the link, the search and parse, the token emitter and the block's size
// from its histograms deflate_batch_lz.hip's (dblz::).
//
// Lz77Huffman's bit lengths are the same at every bit position, so the reference's recursion (:36-69)
// is this rule: a block [a, a + n) has the halves f = (n + 1) / 2 and s = n - f; it is split iff
// min(f, s) > minBlockLen and bits(a, f) + bits(a + f, s) < bits(a, n), bits() being the size of the
// range as ONE Lz77Huffman block whose window starts at the chunk's history (the sub-decide keeps `off`
// and passes historyLen + firstHalfLen, :44-46); each half is then treated the same way.  Per chunk:
//   fold    the chunk's bytes into the stream's checksum;
//   link    the chunk's positions, once (dblz::lz_chunk<LZ_LINK>), unless the search is literal-only;
//   walk    the split tree depth-first, the left half first, so that leaves are met in stream order and
//       each is emitted at once into the stream's bit buffer.  A node is SIZED by the multi kernel's
//       candidate step on (rc0 + a, n): begin_block_hist, dblz::lz_chunk<LZ_SEARCH>, end_block_hist, the
//       hdist0 copy, build_block_codes<64, true>, header bits + dblz::token_bits (an empty block's dummy
//       literal taken off).  Of a node that may be split the right half is sized first and the left
//       half last.  When the halves win, the right half, (start, length, bits), waits on the stack in
//       LDS and the walk goes on with the left half, whose tokens and codes are the ones in place: if
//       its own halves are too short to try, it is emitted without another search.  So is a chunk too
//       short to split: one search, as in ndfl_deflate_batch_lz_kernel.  Any other leaf is searched and
//       built once more.  Every node is sized exactly once; BFINAL is known when a node is sized (the
//       chunk is the stream's last and the node ends it), so a block is never built twice for its flag.
// The stack holds the right halves of the nodes on the way down: a split node has n / 2 > minBlockLen
// >= 1, so n >= 4, and the k-th node on the way has n <= 65,536 >> k: at most 15 of them.
//
// Device memory of a wave (BatchLzScratch): one token list and the link ring.  The chunk is linked
// whole before its first position is searched, so the ring holds the chunk and its window at once, as
// the multi kernel's: the power of two >= min(the longest stream, hist_limit + chunk_len), at most
// 131,072 links.  At most 256 KiB of links and 256 KiB of tokens per wave; with BATCH_LZ_BUDGET the
// grid never falls below 512 waves.
//
// No scratch memory: everything is forced inline, no per-lane array is indexed by a variable, the lane
// index is an opaque_lane() in every step, wave-uniform state is parked (dbat::to_v).
// D/ = src/io/nayuki/deflate/ in the reference
#pragma once
#include "deflate_batch_multi.hip"

namespace dbsp {

using dbat::BitOut;
using dbat::rfl;
using dbat::to_s;
using dbat::to_v;

constexpr uint32_t NSTK = 16;                 // stack entries: > the 15 right halves that can wait at once
// what the next search and build is for
constexpr uint32_t OP_NODE = 0;               // a node of its own: the chunk
constexpr uint32_t OP_RIGHT = 1;              // the current node's right half, to size it
constexpr uint32_t OP_LEFT = 2;               // its left half, to size it
constexpr uint32_t OP_EMIT = 3;               // a leaf sized before, to emit it

struct Args : dbat::FrameArgs {
    uint32_t hist_limit;
    int32_t dynamic;
    uint32_t min_run, max_run, min_dist, max_dist;    // the search's (literal only: 3, 258, 1, 0: no distance at all)
    uint32_t min_block;       // minBlockLen >= 1
    int32_t link;             // the window holds a distance: the chunks are linked
    const uint32_t* crc_tab;  // as dblz::Args
    uint16_t* ring;           // ring_mask + 1 links per wave
    uint32_t ring_mask;
    uint32_t* toks;           // tok_cap tokens per wave
    uint32_t tok_cap;         // >= min(chunk_len, longest in_len)
};

// LDS of one wave: 21,016 bytes, 7 waves per CU (160 KiB / 21,016 = 7.8).
struct Lds : dblz::Lds {
    uint32_t stk[3 * NSTK];   // the waiting right halves: start, length, bits
};

}  // namespace dbsp

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_batch_binsplit_kernel(dbsp::Args a) {
    using namespace dbsp;
    __shared__ __attribute__((aligned(16))) Lds S;
    const dbat::Frame f = dbat::park_frame(a);
    const uint64_t v_tab = to_v((uint64_t)(uintptr_t)a.crc_tab);
    const uint64_t v_ring = to_v((uint64_t)(uintptr_t)(a.ring + (size_t)blockIdx.x * ((size_t)a.ring_mask + 1)));
    const uint64_t v_toks = to_v((uint64_t)(uintptr_t)(a.toks + (size_t)blockIdx.x * a.tok_cap));
    const uint32_t v_mask = to_v(a.ring_mask);
    const uint32_t v_hist = to_v(a.hist_limit), v_link = to_v((uint32_t)(a.link != 0));
    const uint32_t v_dyn = to_v((uint32_t)(a.dynamic != 0)), v_minb = to_v(a.min_block);
    const uint32_t v_run = to_v(a.min_run | a.max_run << 16);
    const uint32_t v_mind = to_v(a.min_dist), v_maxd = to_v(a.max_dist);
    for (;;) {
        dbat::Stream st;
        if (!dbat::claim_stream(S, f, st)) break;
        // the running state, all of it started afresh for the stream (as ndfl_deflate_batch_lz_kernel)
        BitOut bo = dbat::begin_stream(S, f, st);
        uint32_t v_fill = to_v(0u), v_cb = to_v(0u);
        uint64_t v_cs = to_v((uint64_t)0);
        for (uint32_t j = (uint32_t)opaque_lane(); j < dblz::NHEAD / 2; j += 64)
            ((uint32_t*)S.head)[j] = dblz::HNONE << 16 | dblz::HNONE;
        for (;;) {
            __syncthreads();
            {
                const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), len - cs);
                const uint64_t hs = cs - min((uint64_t)to_s(v_hist), cs);      // chunk 0 has no history
                const uint8_t* P = (const uint8_t*)(uintptr_t)(to_s(st.v_src) + hs);
                const uint32_t rc0 = (uint32_t)(cs - hs);
                const uint32_t rend = (uint32_t)min(len - hs, (uint64_t)rc0 + len_c + 8);
                uint32_t ck = to_s(st.v_ck);
                dblz::fold_chunk(v_tab, P + rc0, len_c, to_s(st.v_kind), ck);
                st.v_ck = to_v(ck);
                if (to_s(v_link)) {                               // (a literal-only search follows no link)
                    const dblz::Search none{0u, 0u, 0u, 0u};
                    uint32_t cb = to_s(v_cb);
                    dblz::lz_chunk<dblz::LZ_LINK>(S, none, P, rc0, len_c, rend, (uint32_t)hs,
                                                  (uint16_t*)(uintptr_t)to_s(v_ring), to_s(v_mask), nullptr, true, cb);
                    v_cb = to_v(cb + len_c);
                }
            }
            __syncthreads();                                          // the chunk's links
            // ---- the split tree (offsets are the chunk's) ---------------------------------------------
            // the range searched and built next, and what for; the current node and its bits; its right
            // half's bits between OP_RIGHT and OP_LEFT; the stack's height
            uint32_t v_ta = to_v(0u), v_tn, v_op = to_v(OP_NODE);
            uint32_t v_ca = to_v(0u), v_cn, v_cbits = to_v(0u), v_rbits = to_v(0u), v_sp = to_v(0u);
            {
                const uint64_t cs = to_s(v_cs);
                v_tn = to_v((uint32_t)min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs));
                v_cn = v_tn;
            }
            for (;;) {
                // ---- the range's block: tokens, histograms, codes, header, and its exact size ---------
                uint32_t v_ntok, v_hb, v_bits;
                dbat::begin_block_hist(S);
                __syncthreads();
                {
                    const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                    const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), len - cs);
                    const uint64_t hs = cs - min((uint64_t)to_s(v_hist), cs);
                    const uint8_t* P = (const uint8_t*)(uintptr_t)(to_s(st.v_src) + hs);
                    const uint32_t rc0 = (uint32_t)(cs - hs);
                    const uint32_t rend = (uint32_t)min(len - hs, (uint64_t)rc0 + len_c + 8);
                    const uint32_t run = to_s(v_run);
                    const dblz::Search sp{run & 0xFFFFu, run >> 16, to_s(v_mind), to_s(v_maxd)};
                    uint32_t nocb = 0;
                    v_ntok = to_v(dblz::lz_chunk<dblz::LZ_SEARCH>(S, sp, P, rc0 + to_s(v_ta), to_s(v_tn), rend, (uint32_t)hs,
                                                                  (uint16_t*)(uintptr_t)to_s(v_ring), to_s(v_mask),
                                                                  (uint32_t*)(uintptr_t)to_s(v_toks), true, nocb));
                    dbat::end_block_hist(S, to_s(v_tn));
                }
                __syncthreads();                                      // the histograms and the token list
                {
                    const int lane = opaque_lane();
                    if (lane < 32) S.scr.hdist0[lane] = S.scr.hdist[lane];
                }
                __syncthreads();
                {
                    // the stream's last block, if the range is a leaf: it ends the stream's last chunk
                    const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                    const bool is_final = cs + to_s(v_ta) + to_s(v_tn) >= len;
                    v_hb = to_v(build_block_codes<64, true>(S.scr, to_s(v_dyn) != 0, is_final, S.litCode, S.distCode));
                }
                {
                    // (an empty block's dummy literal is counted and not emitted)
                    const bool empty = to_s(v_tn) == 0;
                    v_bits = to_v(to_s(v_hb) + dblz::token_bits(S) - (empty ? rfl(S.litCode[0]) >> 16 : 0u));
                }
                // ---- what the size decides --------------------------------------------------------------
                const uint32_t op = to_s(v_op);
                bool emit = op == OP_EMIT;
                if (op == OP_RIGHT) {
                    v_rbits = v_bits;
                    v_ta = v_ca; v_tn = to_v((to_s(v_cn) + 1u) >> 1);
                    v_op = to_v(OP_LEFT);
                } else if (op == OP_LEFT && to_s(v_bits) + to_s(v_rbits) >= to_s(v_cbits)) {
                    v_ta = v_ca; v_tn = v_cn;                          // the halves do not win: a leaf, built again
                    v_op = to_v(OP_EMIT);
                } else if (op != OP_EMIT) {
                    // the chunk, or a left half whose split won: the block in place is the current node's
                    if (op == OP_LEFT) {
                        const uint32_t sp = to_s(v_sp), fh = (to_s(v_cn) + 1u) >> 1;
                        if (opaque_lane() == 0) {
                            S.stk[3 * sp] = to_s(v_ca) + fh; S.stk[3 * sp + 1] = to_s(v_cn) - fh; S.stk[3 * sp + 2] = to_s(v_rbits);
                        }
                        v_sp = to_v(sp + 1u);
                        v_cn = to_v(fh);
                    }
                    v_cbits = v_bits;
                    const uint32_t cn = to_s(v_cn);
                    if ((cn >> 1) > to_s(v_minb)) {                    // min(f, s) = n / 2
                        v_ta = to_v(to_s(v_ca) + ((cn + 1u) >> 1)); v_tn = to_v(cn >> 1);
                        v_op = to_v(OP_RIGHT);
                    } else {
                        emit = true;
                    }
                }
                if (!emit) continue;
                // ---- a leaf: the block in place ---------------------------------------------------------
                bo.fill = to_s(v_fill);
                dbat::put_header(S, bo, to_s(v_hb));
                dblz::emit_tokens(S, bo, (const uint32_t*)(uintptr_t)to_s(v_toks), to_s(v_ntok));
                dbat::put_eob(S, bo);
                v_fill = to_v(bo.fill);
                if (to_s(v_sp) == 0) break;
                __syncthreads();                                      // (the stack's stores)
                {
                    const uint32_t sp = to_s(v_sp) - 1u;
                    v_sp = to_v(sp);
                    v_ca = to_v(rfl(S.stk[3 * sp])); v_cn = to_v(rfl(S.stk[3 * sp + 1])); v_cbits = to_v(rfl(S.stk[3 * sp + 2]));
                    const uint32_t ca = to_s(v_ca), cn = to_s(v_cn);
                    if ((cn >> 1) > to_s(v_minb)) {
                        v_ta = to_v(ca + ((cn + 1u) >> 1)); v_tn = to_v(cn >> 1);
                        v_op = to_v(OP_RIGHT);
                    } else {
                        v_ta = v_ca; v_tn = v_cn;
                        v_op = to_v(OP_EMIT);
                    }
                }
                __syncthreads();                                      // (read before the next store)
            }
            {
                const uint64_t cs = to_s(v_cs);
                v_cs = to_v(cs + min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs));
            }
            if (to_s(v_cs) >= to_s(st.v_len)) break;
        }
        dbat::finish_stream(f, st, bo, v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// The wave's ring entries and token list entries for a batch whose longest stream is `longest` bytes: the
// ring holds a chunk and its window at once (a power of two, 64..dbm::RING_MAX), the list a chunk's tokens.
static inline void batch_binsplit_sizes(uint64_t longest, uint32_t chunk_len, uint32_t hist_limit, uint32_t* ring,
                                        uint32_t* tok_cap) {
    const uint64_t span = std::min<uint64_t>(longest, (uint64_t)hist_limit + chunk_len);
    uint32_t r = 64;
    while (r < dbm::RING_MAX && r < span) r <<= 1;
    *ring = r;
    *tok_cap = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(chunk_len, longest));
}

// batch_run's launcher for ndfl_deflate_batch_binsplit_kernel.
struct BatchBinsplitLaunch {
    BatchLzScratch& Z;
    const Knobs& knobs;
    const ndfl_member_item* items;       // host
    dbsp::Args a;                         // n, chunk_len, hist_limit, min_block, crc_tab, set_search(); deflate_batch_run sets `in`
    uint32_t grid = 0;
    // The substrategy (validated) as the kernel's search.
    void set_search(const ndfl_strategy_desc& d) {
        a.dynamic = d.dynamic != 0;
        // the literal-only form searches a window with no distance in it: nothing is ever a run
        const bool lit = d.min_run == 0;
        a.min_run = lit ? 3u : (uint32_t)d.min_run; a.max_run = lit ? 258u : (uint32_t)d.max_run;
        a.min_dist = lit ? 1u : (uint32_t)d.min_dist; a.max_dist = lit ? 0u : (uint32_t)d.max_dist;
        a.link = a.max_dist >= a.min_dist;
    }
    // Before the launch is timed: sizes the wave's ring and token list from the batch, lowers the grid to
    // the budget and grows the scratch (first use only).
    int prepare() {
        uint64_t longest = 0;
        for (uint32_t i = 0; i < a.n; i++) longest = std::max(longest, items[i].in_len);
        uint32_t ring;
        batch_binsplit_sizes(longest, a.chunk_len, a.hist_limit, &ring, &a.tok_cap);
        const size_t per_wave = (size_t)ring * 2 + (size_t)a.tok_cap * 4;
        grid = batch_grid<ndfl_deflate_batch_binsplit_kernel>(a.n, knobs, "deflate batch binsplit", per_wave, BATCH_LZ_BUDGET);
        INF_CHK(inf_ensure(&Z.d_mem, &Z.d_mem_cap, (size_t)grid * per_wave));
        a.toks = (uint32_t*)Z.d_mem;
        a.ring = (uint16_t*)((char*)Z.d_mem + (size_t)grid * a.tok_cap * 4); a.ring_mask = ring - 1;
        return 0;
    }
    int operator()(hipStream_t s, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                   uint32_t* d_ticket) {
        a.out = d_out; a.items = d_items; a.results = d_res; a.ticket = d_ticket;
        hipLaunchKernelGGL(ndfl_deflate_batch_binsplit_kernel, dim3(grid), dim3(64), 0, s, a);
        return 0;
    }
};
