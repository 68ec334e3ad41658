// deflate_batch_multi.hip -- batched MultiStrategy deflate: many independent buffers compressed in one
// launch, every chunk as the block of whichever substrategy takes the fewest bits
// (ndfl_deflate_batch_multi, include/ndfl.h): MultiStrategy(strats...) of D/comp/MultiStrategy.java:31-57
// over Lz77Huffman records and Uncompressed.SINGLETON (D/comp/Uncompressed.java:19-51).  The third of the
// batch kernels, with the launch shape of its two siblings: a persistent grid of one-wave workgroups, an
// atomic ticket over the stream indices, each stream encoded chunk by chunk, serially, by one wave that
// waits on no other.  The stream frame, the bit buffer, the region stores and the checksum folding are
// deflate_batch.hip's (dbat::), the link, search and parse and the token emitter deflate_batch_lz.hip's
// (dblz::).
//
// The host hands the kernel CANDIDATES, not substrategies: exact duplicates are dropped (a later equal
// one can never win), the Lz77Huffman ones are grouped by their (min_run, max_run, min_dist, max_dist),
// a group's static one before its dynamic one, and each carries its index in the caller's list.  Per
// chunk (= block):
//   fold    the chunk's bytes into the stream's checksum: one walk, whichever block type wins;
//   link    the chunk's positions, once (dblz::lz_chunk<LZ_LINK>), unless every search is literal-only;
//   per candidate, in the host's order:
//       the first of a group searches and parses (dblz::lz_chunk<LZ_SEARCH>) into the wave's CURRENT
//       token list and the LDS histograms, which the rest of the group shares; hdist is copied to
//       hdist0, because the code builder gives a single used distance code a dummy neighbour;
//       build_block_codes<64, true> (static: the fixed codes), and the block's exact size: the header's
//       bits plus, from the histograms, count x (code length + extra bits), end of block included (the
//       dummy literal an empty block counts is taken off again: it is not emitted);
//       Uncompressed: 8 len + 40 max(ceil(len / 65535), 1) + ((13 - p) % 8 - 5) bits at bit position p;
//       fewer bits than the best so far, or as many from an earlier index in the caller's list, makes
//       it the best: its two code tables, its header words and their bit count, and its token count are
//       copied to the LDS's second set, and its token list becomes the one the next group's search does
//       NOT write (the wave has two lists) -- so the best so far is never searched or built again;
//   emit    the best: header, tokens and end of block from the second set (dblz::emit_tokens), or the
//       stored blocks: 3 header bits, zero bits to the byte, LEN, NLEN, the bytes, at most 65,535 a
//       block, BFINAL on the stream's last block only.  The bytes go through the same bit buffer, 64
//       lanes x 4 bytes a step (they are byte aligned, a BitPut takes them as two 16-bit puts), so the
//       flush, the out_cap clamp and the "no byte outside the region" rule stay one implementation.
//
// Device memory of a wave (BatchLzScratch): two token lists and the link ring.  The chunk is linked
// whole before its first position is searched, so the ring holds the chunk and its window at once:
// the power of two >= min(the longest stream, hist_limit + chunk_len), at most 131,072 links.  At most
// 256 KiB of links and 2 x 256 KiB of tokens per wave; with BATCH_LZ_BUDGET the grid never falls below
// 341 waves.
//
// No scratch memory: everything is forced inline, no per-lane array is indexed by a variable, the lane
// index is an opaque_lane() in every step, wave-uniform state is parked (dbat::to_v).  The candidates
// are parked too: lane k holds candidate k's three words, read with readlane.
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
constexpr uint32_t RING_MAX = 131072;         // link ring entries: >= 32,768 + 65,536

struct Args : dbat::FrameArgs {
    uint32_t hist_limit;
    uint32_t n_cand;          // 1..MAXC
    uint32_t c_flags[MAXC];
    uint32_t c_run[MAXC];     // min_run | max_run << 16
    uint32_t c_dist[MAXC];    // min_dist | max_dist << 16 (literal only: 1 | 0 << 16, no distance at all)
    int32_t has_lz;           // some candidate is not C_STORED
    int32_t link;             // some candidate has a distance in its window: the chunks are linked
    const uint32_t* crc_tab;  // as dblz::Args
    uint16_t* ring;           // ring_mask + 1 links per wave
    uint32_t ring_mask;
    uint32_t* toks;           // 2 x tok_cap tokens per wave
    uint32_t tok_cap;         // >= min(chunk_len, longest in_len)
};

// LDS of one wave: 22,424 bytes, 7 waves per CU (160 KiB / 22,424 = 7.3).
struct Lds : dblz::Lds {
    uint32_t b_lit[288];      // the best candidate so far: its codes,
    uint32_t b_dist[32];
    uint32_t b_hdr[HDRW];     // and its header words
};

using dblz::token_bits;       // a block's exact size from its histograms (shared with deflate_batch_binsplit.hip)

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
    const uint64_t v_tab = to_v((uint64_t)(uintptr_t)a.crc_tab);
    const uint64_t v_ring = to_v((uint64_t)(uintptr_t)(a.ring + (size_t)blockIdx.x * ((size_t)a.ring_mask + 1)));
    const uint64_t v_toks = to_v((uint64_t)(uintptr_t)(a.toks + (size_t)blockIdx.x * 2 * a.tok_cap));
    const uint32_t v_mask = to_v(a.ring_mask), v_tcap = to_v(a.tok_cap);
    const uint32_t v_hist = to_v(a.hist_limit), v_ncand = to_v(a.n_cand), v_link = to_v((uint32_t)(a.link != 0));
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
                if (to_s(v_link)) {                               // (literal-only searches follow no link)
                    const dblz::Search none{0u, 0u, 0u, 0u};
                    uint32_t cb = to_s(v_cb);
                    dblz::lz_chunk<dblz::LZ_LINK>(S, none, P, rc0, len_c, rend, (uint32_t)hs,
                                                  (uint16_t*)(uintptr_t)to_s(v_ring), to_s(v_mask), nullptr, true, cb);
                    v_cb = to_v(cb + len_c);
                }
            }
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
                    const uint64_t cs = to_s(v_cs);
                    const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs);
                    const uint32_t nblk = max((len_c + 65534u) / 65535u, 1u);
                    v_bits = to_v(8 * len_c + 40 * nblk + ((13u - (to_s(v_fill) & 7u)) & 7u) - 5u);
                } else {
                    if (to_s(v_cfk) & C_SEARCH) {
                        v_csel = to_v(to_s(v_bsel) ^ 1u);             // not the best's list
                        dbat::begin_block_hist(S);
                        __syncthreads();
                        const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                        const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), len - cs);
                        const uint64_t hs = cs - min((uint64_t)to_s(v_hist), cs);
                        const uint8_t* P = (const uint8_t*)(uintptr_t)(to_s(st.v_src) + hs);
                        const uint32_t rc0 = (uint32_t)(cs - hs);
                        const uint32_t rend = (uint32_t)min(len - hs, (uint64_t)rc0 + len_c + 8);
                        const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)v_cr, (int)to_s(v_k));
                        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)v_cd, (int)to_s(v_k));
                        const dblz::Search sp{cr & 0xFFFFu, cr >> 16, cd & 0xFFFFu, cd >> 16};
                        uint32_t* toks = (uint32_t*)(uintptr_t)to_s(v_toks) + (size_t)to_s(v_csel) * to_s(v_tcap);
                        uint32_t nocb = 0;
                        v_ntok = to_v(dblz::lz_chunk<dblz::LZ_SEARCH>(S, sp, P, rc0, len_c, rend, (uint32_t)hs,
                                                                      (uint16_t*)(uintptr_t)to_s(v_ring), to_s(v_mask),
                                                                      toks, true, nocb));
                        dbat::end_block_hist(S, len_c);
                        __syncthreads();                              // the histograms and the token list
                        {
                            const int lane = opaque_lane();
                            if (lane < 32) S.scr.hdist0[lane] = S.scr.hdist[lane];
                        }
                        __syncthreads();
                    }
                    {
                        const bool is_final = to_s(st.v_len) - to_s(v_cs) <= (uint64_t)to_s(f.v_chunk_len);
                        v_hb = to_v(build_block_codes<64, true>(S.scr, (to_s(v_cfk) & C_DYNAMIC) != 0, is_final, S.litCode,
                                                                S.distCode));
                    }
                    // (an empty block's dummy literal is counted and not emitted)
                    const bool empty = to_s(v_cs) >= to_s(st.v_len);
                    v_bits = to_v(to_s(v_hb) + token_bits(S) - (empty ? rfl(S.litCode[0]) >> 16 : 0u));
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
            bo.fill = to_s(v_fill);
            if (to_s(v_bstored)) {
                const uint64_t cs = to_s(v_cs), len = to_s(st.v_len);
                const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), len - cs);
                put_stored(bo, to_v(to_s(st.v_src) + cs), to_v(len_c),
                           to_v((uint32_t)(len - cs <= (uint64_t)to_s(f.v_chunk_len))));
            } else {
                {
                    const int lane = opaque_lane();
                    for (int t = lane; t < 288; t += 64) S.litCode[t] = S.b_lit[t];
                    if (lane < 32) S.distCode[lane] = S.b_dist[lane];
                    for (int t = lane; t < HDRW; t += 64) S.scr.hdr()[t] = S.b_hdr[t];
                }
                __syncthreads();
                dbat::put_header(S, bo, to_s(v_bhb));
                dblz::emit_tokens(S, bo, (const uint32_t*)(uintptr_t)to_s(v_toks) + (size_t)to_s(v_bsel) * to_s(v_tcap),
                                  to_s(v_bntok));
                dbat::put_eob(S, bo);
            }
            {
                const uint64_t cs = to_s(v_cs);
                v_cs = to_v(cs + min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs));
            }
            v_fill = to_v(bo.fill);
            if (to_s(v_cs) >= to_s(st.v_len)) break;
        }
        dbat::finish_stream(f, st, bo, v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// batch_run's launcher for ndfl_deflate_batch_multi_kernel.
struct BatchMultiLaunch {
    BatchLzScratch& Z;
    const Knobs& knobs;
    const ndfl_member_item* items;       // host
    dbm::Args a;                          // n, chunk_len, hist_limit, the candidates, crc_tab; deflate_batch_run sets `in`
    uint32_t grid = 0;
    // The caller's substrategies (validated) as the kernel's candidates.  Returns their number; c_flags[0] >> 8
    // is the index of the first one's substrategy.
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
                // the literal-only form searches a window with no distance in it: nothing is ever a run
                const bool lit = d.min_run == 0;
                c.run = lit ? 3u | 258u << 16 : (uint32_t)d.min_run | (uint32_t)d.max_run << 16;
                c.dist = lit ? 1u : (uint32_t)d.min_dist | (uint32_t)d.max_dist << 16;
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
        a.has_lz = !groups.empty();
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
    // Before the launch is timed: sizes the wave's ring and two token lists from the batch, lowers the
    // grid to the budget and grows the scratch (first use only).
    int prepare() {
        size_t per_wave = 0;
        uint32_t ring = 64;
        if (a.has_lz) {
            uint64_t longest = 0;
            for (uint32_t i = 0; i < a.n; i++) longest = std::max(longest, items[i].in_len);
            const uint64_t span = std::min<uint64_t>(longest, (uint64_t)a.hist_limit + a.chunk_len);
            while (ring < dbm::RING_MAX && ring < span) ring <<= 1;
            a.tok_cap = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(a.chunk_len, longest));
            per_wave = (size_t)ring * 2 + (size_t)a.tok_cap * 8;
        }
        grid = batch_grid<ndfl_deflate_batch_multi_kernel>(a.n, knobs, "deflate batch multi", per_wave, BATCH_LZ_BUDGET);
        if (per_wave) INF_CHK(inf_ensure(&Z.d_mem, &Z.d_mem_cap, (size_t)grid * per_wave));
        a.toks = (uint32_t*)Z.d_mem;
        a.ring = (uint16_t*)((char*)Z.d_mem + (size_t)grid * a.tok_cap * 8); a.ring_mask = ring - 1;
        return 0;
    }
    int operator()(hipStream_t s, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                   uint32_t* d_ticket) {
        a.out = d_out; a.items = d_items; a.results = d_res; a.ticket = d_ticket;
        hipLaunchKernelGGL(ndfl_deflate_batch_multi_kernel, dim3(grid), dim3(64), 0, s, a);
        return 0;
    }
};
