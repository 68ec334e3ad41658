// deflate_batch_multi.hip -- batched MultiStrategy deflate: many independent buffers compressed in one
// launch, every chunk as the block of whichever substrategy takes the fewest bits
// (ndfl_deflate_batch_multi, include/ndfl.h): MultiStrategy(strats...) of D/comp/MultiStrategy.java:31-57
// over Lz77Huffman records and Uncompressed.SINGLETON (D/comp/Uncompressed.java:19-51).  The third of the
// batch kernels: the stream frame is deflate_batch.hip's (dbat::), the chunk, its links, its searches and
// its blocks' sizing and emit deflate_batch_lz.hip's (dblz::).  What is this file's: the candidates, the
// best so far, and the stored block.
//
// The host hands the kernel CANDIDATES, not substrategies: exact duplicates are dropped (a later equal
// one can never win), the Lz77Huffman ones are grouped by their (min_run, max_run, min_dist, max_dist),
// a group's static one before its dynamic one, and each carries its index in the caller's list.  Per
// chunk (= block), after dblz::fold_and_link (one walk and one link pass, whichever block type wins),
// per candidate, in the host's order:
//   the first of a group searches (dblz::search_block) into the wave's CURRENT token list and the LDS
//       histograms, which the rest of the group shares;
//   dblz::size_block gives its codes, header and exact size;
//       Uncompressed: 8 len + 40 max(ceil(len / 65535), 1) + ((13 - p) % 8 - 5) bits at bit position p;
//   fewer bits than the best so far, or as many from an earlier index in the caller's list, makes
//       it the best: its two code tables, its header words and their bit count, and its token count are
//       copied to the LDS's second set, and its token list becomes the one the next group's search does
//       NOT write (the wave has two lists) -- so the best so far is never searched or built again.
// Then the best is emitted: dblz::emit_block from the second set, or the stored blocks: 3 header bits,
// zero bits to the byte, LEN, NLEN, the bytes, at most 65,535 a block, BFINAL on the stream's last block
// only.  The bytes go through the same bit buffer, 64 lanes x 4 bytes a step (they are byte aligned, a
// BitPut takes them as two 16-bit puts), so the flush, the out_cap clamp and the "no byte outside the
// region" rule stay one implementation.
//
// The candidates are parked as the rest of the wave-uniform state is: lane k holds candidate k's three
// words, read with readlane.
// D/ = src/io/nayuki/deflate/ in the reference
#pragma once
#include "deflate_batch_lz.hip"
#include <algorithm>
#include <utility>
#include <vector>

namespace dbm {

using dbat::BitOut;
using dbat::make_room;
using dbat::rfl;
using dbat::to_s;
using dbat::to_v;

constexpr uint32_t MAXC = 8;                  // candidates (= substrategies) at most
// a candidate's flags; its index in the caller's list is flags >> 8
constexpr uint32_t C_STORED = 1, C_DYNAMIC = 2, C_SEARCH = 4;   // C_SEARCH: the first of its group

struct Args : dblz::LzArgs {  // (two token lists per wave)
    uint32_t n_cand;          // 1..MAXC
    uint32_t c_flags[MAXC];
    uint32_t c_run[MAXC];     // min_run | max_run << 16
    uint32_t c_dist[MAXC];    // min_dist | max_dist << 16 (literal only: 1 | 0 << 16, no distance at all)
    int32_t link;             // some candidate has a distance in its window: the chunks are linked
};

// LDS of one wave: 22,424 bytes, 7 waves per CU (160 KiB / 22,424 = 7.3).
struct Lds : dblz::Lds {
    uint32_t b_lit[288];      // the best candidate so far: its codes,
    uint32_t b_dist[32];
    uint32_t b_hdr[HDRW];     // and its header words
};

// The chunk's len_c bytes at cp as stored blocks (D/comp/Uncompressed.java:32-46).  The walk's own
// values are parked across make_room (v_cp, v_len_c, v_final: parked by the caller).
__device__ __forceinline__ void put_stored(BitOut& bo, uint64_t v_cp, uint32_t v_len_c, uint32_t v_final) {
    uint32_t v_at = to_v(0u);
    do {
        make_room(bo, 3 + 7 + 32);
        {
            const uint32_t left = to_s(v_len_c) - to_s(v_at);
            const uint32_t n = min(left, 65535u);
            const uint32_t lenpos = (bo.fill + 3 + 7) & ~7u;
            if (opaque_lane() == 0) {
                BitPut bp; bp.init(bo.obuf, bo.fill);
                bp.put((to_s(v_final) && n == left) ? 1u : 0u, 3);          // BFINAL, BTYPE 00; the padding is zero already
                bp.flush();
                bp.init(bo.obuf, lenpos);
                bp.put(n, 16);
                bp.put(n ^ 0xFFFFu, 16);
                bp.flush();
            }
            bo.fill = lenpos + 32;
        }
        for (uint32_t v_sb = to_v(0u);; v_sb = to_v(to_s(v_sb) + 256u)) {
            if (to_s(v_sb) >= min(to_s(v_len_c) - to_s(v_at), 65535u)) break;
            make_room(bo, 8 * 256);
            const int lane = opaque_lane();
            const uint32_t at = to_s(v_at), n = min(to_s(v_len_c) - at, 65535u), sb = to_s(v_sb);
            const uint32_t L = min(256u, n - sb), o = 4 * (uint32_t)lane;
            if (o < L) {
                const uint32_t k = min(4u, L - o);
                const uint32_t w = dblz::ld4((const uint8_t*)(uintptr_t)to_s(v_cp), at + sb + o, at + n);   // (zero past the block's end)
                BitPut bp; bp.init(bo.obuf, bo.fill + 8 * o);
                bp.put(w & 0xFFFFu, 8 * min(k, 2u));
                if (k > 2) bp.put(w >> 16, 8 * (k - 2));
                bp.flush();
            }
            bo.fill += 8 * L;
        }
        v_at = to_v(to_s(v_at) + min(to_s(v_len_c) - to_s(v_at), 65535u));
    } while (to_s(v_at) < to_s(v_len_c));
}

}  // namespace dbm

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_batch_multi_kernel(dbm::Args a) {
    using namespace dbm;
    __shared__ __attribute__((aligned(16))) Lds S;
    const dbat::Frame f = dbat::park_frame(a);
    const dblz::Wave w = dblz::park_wave(a, 2);
    const uint32_t v_tcap = to_v(a.tok_cap), v_ncand = to_v(a.n_cand), v_link = to_v((uint32_t)(a.link != 0));
    // candidate k in lane k
    uint32_t v_cf = 0, v_cr = 0, v_cd = 0;
    {
        const int lane = opaque_lane();
#pragma unroll
        for (int k = 0; k < (int)MAXC; k++)
            if (lane == k) { v_cf = a.c_flags[k]; v_cr = a.c_run[k]; v_cd = a.c_dist[k]; }
    }
    for (;;) {
        dbat::Stream st;
        if (!dbat::claim_stream(S, f, st)) break;
        BitOut bo = dbat::begin_stream(S, f, st);
        dblz::LzState z = dblz::begin_lz(S);
        do {
            __syncthreads();
            dblz::fold_and_link(S, f, st, w, z, to_s(v_link) != 0);
            __syncthreads();                                          // the chunk's links
            // the best candidate so far: its bits and index, its header's bits, its token count and list
            uint32_t v_bbits = to_v(0xFFFFFFFFu), v_bidx = to_v(0xFFFFFFFFu), v_bhb = to_v(0u), v_bntok = to_v(0u);
            uint32_t v_bsel = to_v(1u), v_bstored = to_v(0u);
            uint32_t v_ntok = to_v(0u), v_csel = to_v(0u);            // the current group's token count and list
            // (the loop's own values are parked across the code construction too)
            for (uint32_t v_k = to_v(0u); to_s(v_k) < to_s(v_ncand); v_k = to_v(to_s(v_k) + 1u)) {
                const uint32_t v_cfk = to_v((uint32_t)__builtin_amdgcn_readlane((int)v_cf, (int)to_s(v_k)));
                uint32_t v_bits, v_hb = to_v(0u);
                if (to_s(v_cfk) & C_STORED) {
                    const uint32_t len_c = dblz::chunk_view(f, st, w, z.v_cs).len_c;
                    const uint32_t nblk = max((len_c + 65534u) / 65535u, 1u);
                    v_bits = to_v(8 * len_c + 40 * nblk + ((13u - (to_s(z.v_fill) & 7u)) & 7u) - 5u);
                } else {
                    if (to_s(v_cfk) & C_SEARCH) {
                        v_csel = to_v(to_s(v_bsel) ^ 1u);             // not the best's list
                        const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)v_cr, (int)to_s(v_k));
                        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)v_cd, (int)to_s(v_k));
                        const dblz::Search sp{cr & 0xFFFFu, cr >> 16, cd & 0xFFFFu, cd >> 16};
                        const dblz::Range whole{0u, dblz::chunk_view(f, st, w, z.v_cs).len_c};
                        v_ntok = to_v(dblz::search_block(S, f, st, w, z.v_cs, sp, whole,
                                                         dblz::toks_of(w) + (size_t)to_s(v_csel) * to_s(v_tcap)));
                    }
                    const dblz::ChunkView c = dblz::chunk_view(f, st, w, z.v_cs);
                    const dblz::BlockSize b = dblz::size_block(S, (to_s(v_cfk) & C_DYNAMIC) != 0, c.is_final, c.len_c == 0);
                    v_hb = b.v_hb; v_bits = b.v_bits;
                }
                {
                    const uint32_t bits = to_s(v_bits), idx = to_s(v_cfk) >> 8;
                    if (bits < to_s(v_bbits) || (bits == to_s(v_bbits) && idx < to_s(v_bidx))) {
                        v_bbits = to_v(bits); v_bidx = to_v(idx);
                        v_bstored = to_v(to_s(v_cfk) & C_STORED);
                        if (!(to_s(v_cfk) & C_STORED)) {
                            v_bhb = v_hb; v_bntok = v_ntok; v_bsel = v_csel;
                            const int lane = opaque_lane();
                            for (int t = lane; t < 288; t += 64) S.b_lit[t] = S.litCode[t];
                            if (lane < 32) S.b_dist[lane] = S.distCode[lane];
                            for (int t = lane; t < HDRW; t += 64) S.b_hdr[t] = S.scr.hdr()[t];
                        }
                    }
                }
                __syncthreads();
            }
            // ---- the best one's block ---------------------------------------------------------------
            bo.fill = to_s(z.v_fill);
            if (to_s(v_bstored)) {
                const dblz::ChunkView c = dblz::chunk_view(f, st, w, z.v_cs);
                put_stored(bo, to_v((uint64_t)(uintptr_t)(c.P + c.rc0)), to_v(c.len_c), to_v((uint32_t)c.is_final));
            } else {
                {
                    const int lane = opaque_lane();
                    for (int t = lane; t < 288; t += 64) S.litCode[t] = S.b_lit[t];
                    if (lane < 32) S.distCode[lane] = S.b_dist[lane];
                    for (int t = lane; t < HDRW; t += 64) S.scr.hdr()[t] = S.b_hdr[t];
                }
                __syncthreads();
                dblz::emit_block(S, bo, to_s(v_bhb), dblz::toks_of(w) + (size_t)to_s(v_bsel) * to_s(v_tcap), to_s(v_bntok));
            }
            z.v_fill = to_v(bo.fill);
        } while (dblz::advance_chunk(f, st, w, z));
        dbat::finish_stream(f, st, bo, z.v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
static constexpr char BATCH_MULTI_LABEL[] = "deflate batch multi";

// batch_run's launcher for ndfl_deflate_batch_multi_kernel: chunks linked whole, two token lists.
struct BatchMultiLaunch : BatchLzLaunchT<dbm::Args, ndfl_deflate_batch_multi_kernel, true, 2, BATCH_MULTI_LABEL> {
    // The caller's substrategies (validated) as the kernel's candidates.  Returns their number; c_flags[0] >> 8
    // is the index of the first one's substrategy.  With no Lz77Huffman among them the wave needs no memory.
    uint32_t set_candidates(const ndfl_strategy_desc* strats, uint32_t n_strats) {
        struct C { uint32_t flags, run, dist; };
        std::vector<C> cs;
        std::vector<std::pair<uint32_t, uint32_t>> groups;            // (run, dist) in order of first appearance
        for (uint32_t k = 0; k < n_strats; k++) {
            const ndfl_strategy_desc& d = strats[k];
            C c{k << 8, 0u, 0u};
            if (d.kind == NDFL_KIND_UNCOMPRESSED) {
                c.flags |= dbm::C_STORED;
            } else {
                if (d.dynamic) c.flags |= dbm::C_DYNAMIC;
                const dblz::Search sp = search_of(d);
                c.run = sp.min_run | sp.max_run << 16;
                c.dist = sp.min_dist | sp.max_dist << 16;
            }
            bool dup = false;
            for (const C& e : cs) dup = dup || ((e.flags & 0xFFu) == (c.flags & 0xFFu) && e.run == c.run && e.dist == c.dist);
            if (dup) continue;                                        // (an equal earlier one wins every tie)
            cs.push_back(c);
            if (!(c.flags & dbm::C_STORED) &&
                std::find(groups.begin(), groups.end(), std::make_pair(c.run, c.dist)) == groups.end())
                groups.push_back({c.run, c.dist});
        }
        uint32_t m = 0;
        n_lists = groups.empty() ? 0u : 2u;
        a.link = 0;
        for (const auto& g : groups) a.link |= (g.second >> 16) >= (g.second & 0xFFFFu);
        for (const C& c : cs)
            if (c.flags & dbm::C_STORED) { a.c_flags[m] = c.flags; a.c_run[m] = a.c_dist[m] = 0; m++; }
        for (const auto& g : groups) {
            bool first = true;
            for (uint32_t dyn = 0; dyn < 2; dyn++)                    // the static one before the dynamic one
                for (const C& c : cs) {
                    if ((c.flags & dbm::C_STORED) || c.run != g.first || c.dist != g.second) continue;
                    if (((c.flags & dbm::C_DYNAMIC) != 0) != (dyn != 0)) continue;
                    a.c_flags[m] = c.flags | (first ? dbm::C_SEARCH : 0u); a.c_run[m] = c.run; a.c_dist[m] = c.dist;
                    first = false;
                    m++;
                }
        }
        a.n_cand = m;
        return m;
    }
};
