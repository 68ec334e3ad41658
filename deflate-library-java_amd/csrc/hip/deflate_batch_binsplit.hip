// deflate_batch_binsplit.hip -- batched BinarySplit deflate: many independent buffers compressed in one
// launch, every chunk split into the blocks that BinarySplit(Lz77Huffman(...), minBlockLen) of
// D/comp/BinarySplit.java:21-82 chooses (ndfl_deflate_batch_binsplit, include/ndfl.h).  The fourth of the
// batch kernels: the stream frame is deflate_batch.hip's (dbat::), the chunk, its links, its searches and
// its blocks' sizing and emit deflate_batch_lz.hip's (dblz::).  What is this file's: the split tree.
//
// Lz77Huffman's bit lengths are the same at every bit position, so the reference's recursion (:36-69)
// is this rule: a block [a, a + n) has the halves f = (n + 1) / 2 and s = n - f; it is split iff
// min(f, s) > minBlockLen and bits(a, f) + bits(a + f, s) < bits(a, n), bits() being the size of the
// range as ONE Lz77Huffman block whose window starts at the chunk's history (the sub-decide keeps `off`
// and passes historyLen + firstHalfLen, :44-46); each half is then treated the same way.  Per chunk:
//   dblz::fold_and_link, once (no link pass when the search is literal-only);
//   walk    the split tree depth-first, the left half first, so that leaves are met in stream order and
//       each is emitted at once into the stream's bit buffer.  A node is SIZED as the multi kernel sizes
//       a candidate, on its range of the chunk: dblz::search_block, then dblz::size_block.  Of a node
//       that may be split the right half is sized first and the left half last.  When the halves win, the right half, (start, length, bits), waits on the stack in
//       LDS and the walk goes on with the left half, whose tokens and codes are the ones in place: if
//       its own halves are too short to try, it is emitted without another search.  So is a chunk too
//       short to split: one search, as in ndfl_deflate_batch_lz_kernel.  Any other leaf is searched and
//       built once more.  Every node is sized exactly once; BFINAL is known when a node is sized (the
//       chunk is the stream's last and the node ends it), so a block is never built twice for its flag.
// The stack holds the right halves of the nodes on the way down: a split node has n / 2 > minBlockLen
// >= 1, so n >= 4, and the k-th node on the way has n <= 65,536 >> k: at most 15 of them.
//
// D/ = src/io/nayuki/deflate/ in the reference
#pragma once
#include "deflate_batch_lz.hip"

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

struct Args : dblz::LzArgs {  // (one token list per wave)
    int32_t dynamic;
    uint32_t min_run, max_run, min_dist, max_dist;    // the search's (search_of)
    uint32_t min_block;       // minBlockLen >= 1
    int32_t link;             // the window holds a distance: the chunks are linked
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
    const dblz::Wave w = dblz::park_wave(a, 1);
    const uint32_t v_link = to_v((uint32_t)(a.link != 0));
    const uint32_t v_dyn = to_v((uint32_t)(a.dynamic != 0)), v_minb = to_v(a.min_block);
    const uint32_t v_run = to_v(a.min_run | a.max_run << 16);
    const uint32_t v_mind = to_v(a.min_dist), v_maxd = to_v(a.max_dist);
    for (;;) {
        dbat::Stream st;
        if (!dbat::claim_stream(S, f, st)) break;
        BitOut bo = dbat::begin_stream(S, f, st);
        dblz::LzState z = dblz::begin_lz(S);
        do {
            __syncthreads();
            dblz::fold_and_link(S, f, st, w, z, to_s(v_link) != 0);
            __syncthreads();                                          // the chunk's links
            // ---- the split tree (offsets are the chunk's) ---------------------------------------------
            // the range searched and built next, and what for; the current node and its bits; its right
            // half's bits between OP_RIGHT and OP_LEFT; the stack's height
            uint32_t v_ta = to_v(0u), v_tn = to_v(dblz::chunk_view(f, st, w, z.v_cs).len_c), v_op = to_v(OP_NODE);
            uint32_t v_ca = to_v(0u), v_cn = v_tn, v_cbits = to_v(0u), v_rbits = to_v(0u), v_sp = to_v(0u);
            for (;;) {
                // ---- the range's block: tokens, histograms, codes, header, and its exact size ---------
                uint32_t v_ntok;
                {
                    const uint32_t run = to_s(v_run);
                    const dblz::Search sp{run & 0xFFFFu, run >> 16, to_s(v_mind), to_s(v_maxd)};
                    v_ntok = to_v(dblz::search_block(S, f, st, w, z.v_cs, sp, dblz::Range{to_s(v_ta), to_s(v_tn)},
                                                     dblz::toks_of(w)));
                }
                uint32_t v_hb, v_bits;
                {
                    // the stream's last block, if the range is a leaf: it ends the stream's last chunk
                    const dblz::ChunkView c = dblz::chunk_view(f, st, w, z.v_cs);
                    const dblz::BlockSize b = dblz::size_block(S, to_s(v_dyn) != 0,
                                                               c.is_final && to_s(v_ta) + to_s(v_tn) == c.len_c,
                                                               to_s(v_tn) == 0);
                    v_hb = b.v_hb; v_bits = b.v_bits;
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
                bo.fill = to_s(z.v_fill);
                dblz::emit_block(S, bo, to_s(v_hb), dblz::toks_of(w), to_s(v_ntok));
                z.v_fill = to_v(bo.fill);
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
        } while (dblz::advance_chunk(f, st, w, z));
        dbat::finish_stream(f, st, bo, z.v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
static constexpr char BATCH_BINSPLIT_LABEL[] = "deflate batch binsplit";

// batch_run's launcher for ndfl_deflate_batch_binsplit_kernel: chunks linked whole, one token list.
struct BatchBinsplitLaunch
    : BatchLzLaunchT<dbsp::Args, ndfl_deflate_batch_binsplit_kernel, true, 1, BATCH_BINSPLIT_LABEL> {
    // The substrategy (validated) as the kernel's search.
    void set_search(const ndfl_strategy_desc& d) {
        const dblz::Search sp = search_of(d);
        a.dynamic = d.dynamic != 0;
        a.min_run = sp.min_run; a.max_run = sp.max_run; a.min_dist = sp.min_dist; a.max_dist = sp.max_dist;
        a.link = a.max_dist >= a.min_dist;
    }
};
