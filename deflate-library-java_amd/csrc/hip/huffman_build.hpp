// huffman_build.hpp -- the Huffman codes and header of one DEFLATE block (gfx950), built once for
// every encoder: the split pipeline's codes kernel and the batched encoder (deflate_batch.hip, with an
// opaque lane index: OPQ below) run it on one wave (NT = 64), the one-kernel RLE/LITERAL encoder and
// the LZ77 encoder on their whole workgroup (NT = 1024).
//
// Restates D/comp/Lz77Huffman.java:134-265 (trims, single-distance fix-up, package-merge lengths,
// canonical codes, code-length RLE, code-length code, header) and :309-410 (package-merge, canonical
// and fixed codes).  Every thread of the workgroup calls each function; __syncthreads() is the only
// barrier.  D/ = /root/reference/src/io/nayuki/deflate/
#pragma once
#include "ndfl_common.hpp"

namespace {

constexpr int HDRW = 80;                  // header words: >= 3 + 14 + 57 + 316 * 7 = 2286 bits: <= 7 bits per code length (a
                                          // plain entry is one <= 7-bit code; symbols 16/17/18 cost up to 9/10/14 bits but
                                          // stand for >= 3/3/11 lengths)

// One lane's bits into an LDS bit buffer: a 32-bit accumulator (one shift-or per code); a code that
// crosses the word boundary leaves its top bits as the next word's start (v >> (32 - nb_before),
// 1..30 bits since n <= 30), and the word goes out with one LDS atomicOr.
struct BitPut {
    uint32_t lo;
    uint32_t nb;
    uint32_t wb;         // byte offset of the word being filled
    char* buf;
    __device__ __forceinline__ void init(uint32_t* b, uint32_t bitpos) {
        buf = (char*)b; wb = (bitpos >> 5) * 4; nb = bitpos & 31; lo = 0;
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {     // v < 2^n, n <= 30
        const uint32_t nb0 = nb;
        lo |= v << nb0;
        nb = nb0 + n;
        if (nb >= 32) {
            atomicOr((uint32_t*)(buf + wb), lo);
            wb += 4;
            nb -= 32;
            lo = v >> (32 - nb0);
        }
    }
    __device__ __forceinline__ void flush() {
        if (nb) atomicOr((uint32_t*)(buf + wb), lo);
    }
};

// BitPut into a slot of SLOTW words that only this thread writes, from the slot's bit 0: full words go
// out with plain stores (the slot needs no zeroing, its last word's bits past the count are zero).  A
// thread that passes the slot's end stops storing and keeps counting, so bits() is its bit count
// whether or not its codes fit.  The NT threads' slots are interleaved: word k of thread t is word
// k * NT + t of `buf`, which a wave reaches without a bank conflict whatever k its lanes are at, and
// whose end is the same byte offset for every thread (no register for a slot's bounds).
template <uint32_t SLOTW, uint32_t NT>
struct BitPutSlot {
    static_assert((NT & (NT - 1)) == 0, "a power of two");
    uint32_t lo;
    uint32_t nb;
    uint32_t wb;         // byte offset in buf of the word being filled
    char* buf;
    static __device__ __forceinline__ uint32_t word(uint32_t k) { return k * NT + threadIdx.x; }
    __device__ __forceinline__ void init(uint32_t* b) { buf = (char*)b; wb = threadIdx.x * 4; nb = 0; lo = 0; }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {     // v < 2^n, n <= 30
        const uint32_t nb0 = nb;
        lo |= v << nb0;
        nb = nb0 + n;
        if (nb >= 32) {
            if (wb < SLOTW * NT * 4) *(uint32_t*)(buf + wb) = lo;
            wb += NT * 4;
            nb -= 32;
            lo = v >> (32 - nb0);
        }
    }
    __device__ __forceinline__ void flush() {
        if (nb && wb < SLOTW * NT * 4) *(uint32_t*)(buf + wb) = lo;
    }
    __device__ __forceinline__ uint32_t bits() const { return wb / (NT * 4) * 32 + nb; }
};

constexpr uint32_t CL_EXTRA_BITS[3] = {2, 3, 7};
constexpr uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// LDS of one code construction (8.8 KB: 18 one-wave workgroups per CU; the 1024-thread encoders lay
// it over their bit buffer).  The caller fills hlit/hdist.  Lifetimes share storage: the
// package-merge input keys live in pf[1] until the leaves are ranked (level 0 writes pf[1] only
// after that), the header bits in pf[0] after the last package-merge, the code-length symbols'
// header offsets in lf after the last package-merge, the per-wave partials of a workgroup scan in
// lvl outside the package-merge backtrack; the merged level is never stored (packages are summed as
// the merge produces them).  lastb is the 1024-thread RLE encoder's, dead before the first histogram
// count.
struct HuffScr {
    uint32_t hlit[288];
    uint32_t hdist[32];
    uint32_t hdist0[32];      // codes kernel: distance histogram before the single-code fix-up (token bits)
    union {
        uint32_t lf[288];         // ranked leaf frequencies (package-merge)
        uint16_t clOff[320];      // header bit offset of each code-length symbol (after the last one)
    };
    uint16_t ls[288];
    union {
        uint32_t pf[2][304];      // package frequencies of the current / next level
        uint8_t lastb[1024];      // last byte of each lane's 64
    };
    __device__ __forceinline__ uint32_t* key() { return pf[1]; }     // (292 used: n padded to 4)
    __device__ __forceinline__ uint32_t* hdr() { return pf[0]; }     // (HDRW used)
    uint32_t mpk[15 * 20];
    uint32_t lvl[16];
    __device__ __forceinline__ uint32_t* scan() { return lvl; }      // (one word per wave)
    uint32_t blc[16], nxc[16], mask[16 * 10];
    uint32_t clh[20];
    uint32_t clCode[20];
    uint32_t misc[8];         // [0] HLIT + 257, [1] HDIST + 1 (288, 32 for the fixed codes), [2] no distance code
    uint8_t clSym[320], clExtra[320];
    uint8_t lens[320];        // code lengths, literal/length then distance from lens[misc[0]]
    uint8_t clLen[32];
};

// The thread index of a builder function.  OPQ (one wave only): taken afresh as a value the compiler
// knows nothing about (opaque_lane, ndfl_common.hpp), for a kernel that builds inside a loop over
// streams (deflate_batch.hip): the builder's lane masks are then not hoisted out of that loop.
template <bool OPQ>
__device__ __forceinline__ int builder_tid() {
    if constexpr (OPQ) return opaque_lane();
    else return threadIdx.x;
}

// Exclusive sum / exclusive suffix minimum over the NT threads: in the wave, or through S.scan().
template <int NT, bool OPQ = false>
__device__ __forceinline__ uint32_t excl_scan(uint32_t v, HuffScr& S, uint32_t& total) {
    if constexpr (NT == 64 && OPQ) {
        const uint32_t incl = wave_incl_scan_l(v, opaque_lane());
        total = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
        return incl - v;
    } else if constexpr (NT == 64) {
        const uint32_t incl = wave_incl_scan(v);
        total = __shfl(incl, 63, 64);
        return incl - v;
    } else {
        return block_excl_scan<uint32_t, NT / 64>(v, S.scan(), total);
    }
}
template <int NT, bool OPQ = false>
__device__ __forceinline__ uint32_t excl_suffix_min(uint32_t v, HuffScr& S) {
    if constexpr (NT == 64 && OPQ) return wave_excl_suffix_min_l(v, 0xFFFFFFFFu, opaque_lane());
    else if constexpr (NT == 64) return wave_excl_suffix_min(v, 0xFFFFFFFFu);
    else return block_excl_suffix_min<NT / 64>(v, 0xFFFFFFFFu, S.scan());
}

// Length-limited code lengths by package-merge (D/comp/Lz77Huffman.java:309-335): merge-path
// levels, tie order packages before leaves on equal frequency, prefix backtrack.  Thread t takes
// every NT-th item.  hist: n entries; lens[0..n) receives the lengths.
template <int NT, bool OPQ = false>
__device__ void pm_lengths(const uint32_t* hist, int n, int L, uint8_t* lens, HuffScr& S) {
    const int tid = builder_tid<OPQ>(), lane = tid & 63;
    // the used symbols' keys (freq << 9 | symbol) compacted in symbol order, padded to 4 with ~0
    uint32_t nl = 0;
    for (int base = 0; base < n; base += NT) {                // uniform trip count
        const int i = base + tid;
        uint32_t k = 0xFFFFFFFFu;
        if (i < n) { const uint32_t f = hist[i]; if (f) k = f << 9 | (uint32_t)i; lens[i] = 0; }
        const uint64_t m = __ballot(k != 0xFFFFFFFFu);
        uint32_t at = nl + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), cnt = (uint32_t)__popcll(m);
        if constexpr (NT > 64) {                              // the waves before this one, and all of them
            if (lane == 0) S.scan()[tid >> 6] = cnt;
            __syncthreads();
            cnt = 0;
            for (int w = 0; w < NT / 64; w++) {
                const uint32_t cw = S.scan()[w];
                if (w < (tid >> 6)) at += cw;
                cnt += cw;
            }
            __syncthreads();
        }
        if (k != 0xFFFFFFFFu) S.key()[at] = k;
        nl += cnt;
    }
    const uint32_t nlp = (nl + 3) & ~3u;
    if ((uint32_t)tid < nlp - nl) S.key()[nl + tid] = 0xFFFFFFFFu;
    for (int t = tid; t < L * 20; t += NT) S.mpk[t] = 0;
    __syncthreads();
    // leaves sorted by (freq, symbol): rank by counting among the used keys only (a text chunk uses
    // ~100 of the 286 literal/length symbols), up to KQ keys per thread in registers
    {
        constexpr int KQ = (288 + NT - 1) / NT;
        const uint32_t nq = (nl + NT - 1) / NT;               // uniform: key slots per thread in use
        uint32_t kk[KQ], r[KQ];
#pragma unroll
        for (int q = 0; q < KQ; q++) {
            const uint32_t i = (uint32_t)tid + (uint32_t)NT * q;
            kk[q] = i < nl ? S.key()[i] : 0xFFFFFFFFu;
            r[q] = 0;
        }
        for (uint32_t j = 0; j < nlp; j += 4) {
            const uint4 v = *(const uint4*)&S.key()[j];
#pragma unroll
            for (int q = 0; q < KQ; q++)
                if ((uint32_t)q < nq)
                    r[q] += (uint32_t)(v.x < kk[q]) + (uint32_t)(v.y < kk[q]) + (uint32_t)(v.z < kk[q]) + (uint32_t)(v.w < kk[q]);
        }
#pragma unroll
        for (int q = 0; q < KQ; q++) {
            const uint32_t i = (uint32_t)tid + (uint32_t)NT * q;
            if (i < nl) { S.lf[r[q]] = kk[q] >> 9; S.ls[r[q]] = (uint16_t)(kk[q] & 511u); }
        }
    }
    __syncthreads();
    // fewer than two used symbols: all lengths zero.  No caller gets here for litlen/dist: an empty
    // block counts a dummy literal next to the end-of-block symbol, a single distance code gets its
    // dummy neighbour, and an unused distance alphabet is not built (tests/test_gpu_code_edges.py,
    // class dist_fixups)
    if (nl < 2) return;                                       // uniform
    uint32_t np = 0;
    int cur = 0;
    for (int it = 0; it < L; it++) {
        const uint32_t m = np + nl;
        const uint32_t* pf = S.pf[cur];
        // merged order: package i before leaf j iff pf[i] <= lf[j] (packages first on equal freq).
        // Thread t merges positions [k0, k1): one merge-path search for how many packages precede k0,
        // then a sequential merge (one dependent LDS read per output instead of one binary search
        // per item).  k0 is even, so the thread sums its own pairs into the next level's packages.
        uint32_t* pfn = S.pf[cur ^ 1];
        {
            const uint32_t per = (((m + NT - 1) / NT) + 1) & ~1u;
            const uint32_t k0 = min(m, (uint32_t)tid * per), k1 = min(m, k0 + per);
            uint32_t lo = k0 > nl ? k0 - nl : 0u, hi = min(k0, np);
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (pf[mid] <= S.lf[k0 - mid - 1]) lo = mid + 1; else hi = mid;
            }
            uint32_t i = lo, j = k0 - lo;
            uint32_t pv = i < np ? pf[i] : 0u, lv = j < nl ? S.lf[j] : 0u;
            const uint32_t wb = k0 & ~31u;
            uint64_t bits = 0;
            uint32_t held = 0;
            for (uint32_t pos = k0; pos < k1; pos++) {
                const bool takeP = i < np && (j >= nl || pv <= lv);
                const uint32_t item = takeP ? pv : lv;
                if (pos & 1) pfn[pos >> 1] = held + item;
                held = item;
                if (takeP) {
                    bits |= 1ull << (pos - wb);
                    i++;
                    pv = i < np ? pf[i] : 0u;
                } else {
                    j++;
                    lv = j < nl ? S.lf[j] : 0u;
                }
            }
            if ((uint32_t)bits) atomicOr(&S.mpk[it * 20 + (wb >> 5)], (uint32_t)bits);
            if ((uint32_t)(bits >> 32)) atomicOr(&S.mpk[it * 20 + (wb >> 5) + 1], (uint32_t)(bits >> 32));
        }
        __syncthreads();
        np = m >> 1;
        cur ^= 1;
    }
    // backtrack (first wave): prefix of 2(nl-1) items at the last level; leaves in the prefix of each level
    if (NT == 64 || tid < 64) {
        uint32_t m = 2 * (nl - 1);
        for (int it = L - 1; it >= 0; it--) {
            uint32_t cnt = 0;
            if (lane < 20) {
                const uint32_t w = S.mpk[it * 20 + lane];
                const uint32_t lo = (uint32_t)lane * 32;
                if (lo + 32 <= m) cnt = __popc(w);
                else if (lo < m) cnt = __popc(w & ((1u << (m - lo)) - 1));
            }
            cnt = wave_sum(cnt);
            if (lane == 0) S.lvl[it] = m - cnt;
            m = 2 * cnt;
        }
    }
    __syncthreads();
    for (uint32_t t = (uint32_t)tid; t < nl; t += NT) {
        uint32_t cl = 0;
        for (int it = 0; it < L; it++) cl += t < S.lvl[it];
        lens[S.ls[t]] = (uint8_t)cl;
    }
    __syncthreads();
}

// Canonical codes (D/comp/Lz77Huffman.java:368-391): rev(code) | len << 16 into codes[0..n).
template <int NT, bool OPQ = false>
__device__ void canon_codes(const uint8_t* lens, int n, uint32_t* codes, HuffScr& S) {
    const int tid = builder_tid<OPQ>();
    if (tid < 16) S.blc[tid] = 0;
    for (int t = tid; t < 160; t += NT) S.mask[t] = 0;
    __syncthreads();
    for (int t = tid; t < n; t += NT) {
        const uint32_t l = lens[t];
        if (l) { atomicAdd(&S.blc[l], 1u); atomicOr(&S.mask[l * 10 + (t >> 5)], 1u << (t & 31)); }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t code = 0;
        S.blc[0] = 0;
        for (int b = 1; b < 16; b++) { code = (code + S.blc[b - 1]) << 1; S.nxc[b] = code; }
    }
    __syncthreads();
    for (int t = tid; t < n; t += NT) {
        const uint32_t l = lens[t];
        uint32_t cv = 0;
        if (l) {
            uint32_t rank = 0;
            const int wi = t >> 5;
            for (int w = 0; w < wi; w++) rank += __popc(S.mask[l * 10 + w]);
            rank += __popc(S.mask[l * 10 + wi] & ((1u << (t & 31)) - 1));
            cv = (__brev(S.nxc[l] + rank) >> (32 - l)) | (l << 16);
        }
        codes[t] = cv;
    }
    __syncthreads();
}

// Code construction for one block from the final histograms in S.hlit / S.hdist (end of block
// counted).  Dynamic: D/comp/Lz77Huffman.java:143-265; static: the fixed codes of :394-410.  Leaves
// the codes (rev(code) | len << 16, zero for unused symbols) in lit_out[0..288) / dist_out[0..32),
// the code lengths in S.lens with the alphabet sizes in S.misc[0..1], and the complete header
// (bfinal through the code-length symbols, zero past it) as words in S.hdr().  Returns the header's
// bits.
template <int NT, bool OPQ = false>
__device__ __forceinline__ uint32_t build_block_codes(HuffScr& S, bool dynamic, bool is_final, uint32_t* lit_out,
                                                      uint32_t* dist_out) {
    static_assert(NT % 64 == 0 && NT <= 1024, "whole waves, at most the 16 of S.scan()");
    static_assert(!OPQ || NT == 64, "the opaque lane index is one wave's");
    const int tid = builder_tid<OPQ>(), lane = tid & 63;
    if (!dynamic) {
        // fixed codes (:394-410)
        for (int t = tid; t < 288; t += NT) {
            const uint32_t l = t < 144 ? 8 : t < 256 ? 9 : t < 280 ? 7 : 8;
            const uint32_t code = t < 144 ? 0x30 + t : t < 256 ? 0x190 + (t - 144) : t < 280 ? (t - 256) : 0xC0 + (t - 280);
            lit_out[t] = (__brev(code) >> (32 - l)) | (l << 16);
            S.lens[t] = (uint8_t)l;
        }
        if (tid < 32) {
            dist_out[tid] = (__brev((uint32_t)tid) >> 27) | (5u << 16);
            S.lens[288 + tid] = 5;
        }
        for (int i = tid; i < HDRW; i += NT) S.hdr()[i] = i ? 0u : (is_final ? 1u : 0u) | (1u << 1);
        if (tid == 0) { S.misc[0] = 288; S.misc[1] = 32; }
        __syncthreads();
        return 3;
    }
    // trim litlen histogram, keep >= 257 (:148-151); single used distance code gets a dummy
    // neighbour (:155-171); empty distance code (:172-177)
    if (NT == 64 || tid < 64) {
        const uint64_t lb = __ballot(lane < 29 && S.hlit[257 + lane] != 0);
        uint64_t db = __ballot(lane < 30 && S.hdist[lane] != 0);
        if (__popcll(db) == 1) {
            const int first = (int)__builtin_ctzll(db);
            const int nb = first < 29 ? first + 1 : first - 1;
            if (lane == 0) S.hdist[nb] = 1;
            db |= 1ull << nb;
        }
        if (lane == 0) {
            S.misc[0] = lb ? 258u + (uint32_t)(63 - __builtin_clzll(lb)) : 257u;
            S.misc[1] = db ? 1u + (uint32_t)(63 - __builtin_clzll(db)) : 1u;
            S.misc[2] = db ? 0u : 1u;
        }
    }
    __syncthreads();
    const int ln = (int)S.misc[0], dn = (int)S.misc[1];
    const bool emptyDist = S.misc[2] != 0;
    pm_lengths<NT, OPQ>(S.hlit, ln, 15, S.lens, S);
    if (emptyDist) { if (tid == 0) S.lens[ln] = 0; __syncthreads(); }
    else pm_lengths<NT, OPQ>(S.hdist, dn, 15, S.lens + ln, S);
    canon_codes<NT, OPQ>(S.lens, ln, lit_out, S);
    canon_codes<NT, OPQ>(S.lens + ln, dn, dist_out, S);
    for (int t = ln + tid; t < 288; t += NT) lit_out[t] = 0;
    if (tid >= dn && tid < 32) dist_out[tid] = 0;
    // code-length sequence RLE (:187-223) as maximal-run decomposition; thread t owns [Q t, Q t + Q)
    constexpr int Q = (320 + NT - 1) / NT;
    const int nc = ln + dn;
    uint32_t v[Q], rnext[Q];
    bool st[Q];
    uint32_t firstStart = 0xFFFFFFFFu;
#pragma unroll
    for (int q = Q - 1; q >= 0; q--) {
        const int i = Q * tid + q;
        v[q] = i < nc ? S.lens[i] : 0u;
        st[q] = i < nc && (i == 0 || S.lens[i - 1] != v[q]);
        if (st[q]) firstStart = (uint32_t)i;
    }
    uint32_t nxt = min(excl_suffix_min<NT, OPQ>(firstStart, S), (uint32_t)nc);
    uint32_t cnt[Q], mycnt = 0;
#pragma unroll
    for (int q = Q - 1; q >= 0; q--) {
        cnt[q] = 0;
        if (st[q]) {
            const uint32_t Z = nxt - (uint32_t)(Q * tid + q);
            if (v[q] == 0) { const uint32_t qq = Z / 138, r = Z % 138; cnt[q] = qq + (r >= 3 ? 1 : r); }
            else { const uint32_t rest = Z - 1, qq = rest / 6, r = rest % 6; cnt[q] = 1 + qq + (r >= 3 ? 1 : r); }
            rnext[q] = nxt;
            nxt = (uint32_t)(Q * tid + q);
        }
        mycnt += cnt[q];
    }
    uint32_t tot;
    uint32_t k = excl_scan<NT, OPQ>(mycnt, S, tot);
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if (!st[q]) continue;
        const uint32_t Z = rnext[q] - (uint32_t)(Q * tid + q);
        if (v[q] == 0) {
            uint32_t Lr = Z;
            while (Lr > 0) {
                const uint32_t r = min(Lr, 138u);
                if (r < 3) { S.clSym[k] = 0; S.clExtra[k++] = 0; Lr -= 1; }
                else if (r < 11) { S.clSym[k] = 17; S.clExtra[k++] = (uint8_t)(r - 3); Lr -= r; }
                else { S.clSym[k] = 18; S.clExtra[k++] = (uint8_t)(r - 11); Lr -= r; }
            }
        } else {
            S.clSym[k] = (uint8_t)v[q]; S.clExtra[k++] = 0;
            uint32_t Lr = Z - 1;
            while (Lr >= 3) { const uint32_t r = min(Lr, 6u); S.clSym[k] = 16; S.clExtra[k++] = (uint8_t)(r - 3); Lr -= r; }
            while (Lr > 0) { S.clSym[k] = (uint8_t)v[q]; S.clExtra[k++] = 0; Lr--; }
        }
    }
    if (tid < 20) S.clh[tid] = 0;
    __syncthreads();
    for (uint32_t t = (uint32_t)tid; t < tot; t += NT) atomicAdd(&S.clh[S.clSym[t]], 1u);
    __syncthreads();
    pm_lengths<NT, OPQ>(S.clh, 19, 7, S.clLen, S);
    canon_codes<NT, OPQ>(S.clLen, 19, S.clCode, S);
    for (int i = tid; i < HDRW; i += NT) S.hdr()[i] = 0;             // (hdr shares pf[0])
    // per-symbol header bit offsets (exclusive scan, thread t owns [Q t, Q t + Q))
    uint32_t sb[Q], lsum = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const uint32_t i = (uint32_t)(Q * tid + q);
        sb[q] = 0;
        if (i < tot) {
            const uint32_t sy = S.clSym[i];
            sb[q] = (S.clCode[sy] >> 16) + (sy >= 16 ? CL_EXTRA_BITS[sy - 16] : 0);
        }
        lsum += sb[q];
    }
    uint32_t body;
    uint32_t so = excl_scan<NT, OPQ>(lsum, S, body);
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const uint32_t i = (uint32_t)(Q * tid + q);
        if (i < tot) S.clOff[i] = (uint16_t)so;
        so += sb[q];
    }
    int ncl = 19;
    while (ncl > 4 && S.clLen[CL_ORDER[ncl - 1]] == 0) ncl--;    // (:230-234)
    __syncthreads();
    // header (:134-135,236-258) into the LDS word buffer
    if (tid == 0) {
        BitPut bp; bp.init(S.hdr(), 0);
        bp.put(is_final ? 1u : 0u, 1);
        bp.put(2u, 2);
        bp.put((uint32_t)(ln - 257), 5);
        bp.put((uint32_t)(dn - 1), 5);
        bp.put((uint32_t)ncl - 4, 4);
        for (int i = 0; i < ncl; i++) bp.put(S.clLen[CL_ORDER[i]], 3);
        bp.flush();
    }
    for (uint32_t t = (uint32_t)tid; t < tot; t += NT) {
        const uint32_t sy = S.clSym[t];
        BitPut bp; bp.init(S.hdr(), 17 + 3 * (uint32_t)ncl + S.clOff[t]);
        bp.put(S.clCode[sy] & 0xFFFF, S.clCode[sy] >> 16);
        if (sy >= 16) bp.put(S.clExtra[t], CL_EXTRA_BITS[sy - 16]);
        bp.flush();
    }
    __syncthreads();
    return 3 + 14 + 3 * (uint32_t)ncl + body;
}

}  // namespace
