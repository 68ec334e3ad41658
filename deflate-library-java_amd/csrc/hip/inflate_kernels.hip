// inflate_kernels.hip -- MI355X (gfx950) parallel DEFLATE decoder.
//
// Replaces InflaterInputStream.read -> Open.read -> {UncompressedBlock,HuffmanBlock}.read run to
// the end of one raw DEFLATE stream (D/InflaterInputStream.java:147-164, D/decomp/Open.java:83-620).
//
// A single DEFLATE stream has no block index, so the decoder speculates:
//   1. finder   every bit position is tested (32 per lane, bit-parallel btype masks); positions
//               that start a header passing the reference's own validity checks (dynamic: complete
//               code-length code, decodable code lengths, EOB present, complete litlen/distance
//               codes; stored: LEN == ~NLEN, zero padding, plausible successor) are candidates;
//   2. count    (one lane per candidate): decode blocks from the candidate until the first block
//               boundary at or past the next candidate, recording end bit, output size, status;
//   3. link     (host): follow end bit == candidate start from bit 0; boundaries that are not
//               candidates (fixed-Huffman blocks) are decoded on in parallel repair rounds;
//   4. emit     (one lane per linked chain): decode again into the final output at the chain's
//               offset.  A copy whose source precedes the chain waits (agent-scope acquire) on the
//               owning chains' completion flags; chains are claimed in order through a ticket, so a
//               lane only ever waits on chains whose lanes already run.  The loop is a per-token
//               step machine (bounded work per step) so a waiting lane never blocks its wave.
// Per-lane decoding is latency-bound, so: the bitstream is read through a double-buffered 16-byte
// prefetch, every Huffman table lives in LDS (lane-interleaved: entry e of lane l at e*64+l, bank
// conflict-free for any per-lane index), and the dynamic header is parsed in two passes over the
// stream bits so that no per-lane array (private scratch memory) is ever needed.
// Errors are the reference's DataFormatException Reasons, checked in the reference's order; the
// first error in stream order wins.  The host side of a decode: csrc/capi/ndfl_inflate.cpp.
// D/ = /root/reference/src/io/nayuki/deflate/
#pragma once
#include "ndfl_common.hpp"
#include "../../../include/ndfl.h"
#include <vector>
#include <algorithm>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

namespace inf {

constexpr uint32_t SEG_BYTES = 65536;      // finder segment (compressed bytes)
constexpr uint32_t SEG_CAP = 256;          // candidates kept per finder segment
constexpr uint64_t NONE = ~0ull;

enum : uint32_t { ST_BOUNDARY = 0, ST_FINAL = 1, ST_ERROR = 2 };
constexpr int NEED_INPUT = 64;             // NDFL_NEED_INPUT (include/ndfl.h): partial-input decode stopped
enum : int { R_UEOS = 1, R_RESERVED_BLOCK_TYPE, R_LEN_MISMATCH, R_UNDER_FULL, R_OVER_FULL, R_NO_PREV,
             R_CL_OVER_FULL, R_EOB_ZERO, R_RESERVED_LEN, R_RESERVED_DIST, R_EMPTY_DIST, R_COPY_BEFORE,
             // internal: the second reserved symbol of each alphabet (287, distance 31); the C ABI
             // returns R_RESERVED_LEN / R_RESERVED_DIST and keeps the symbol (ndfl_ctx_error_symbol),
             // which the reference puts in its message (D/decomp/Open.java:516, 550)
             R_RESERVED_LEN_HI = 20, R_RESERVED_DIST_HI = 21,
             R_INTERNAL = 100 };

constexpr int CLO[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// position of code-length symbol sy in CLO (its 3-bit length's index in the header)
constexpr int CLO_INV[19] = {3, 17, 15, 13, 11, 9, 7, 5, 4, 6, 8, 10, 12, 14, 16, 18, 0, 1, 2};

// RUN_LENGTH_TABLE / DISTANCE_TABLE of D/decomp/Open.java:841-886 in closed form.
__device__ __forceinline__ void run_base(uint32_t i, uint32_t& base, uint32_t& ne) {
    if (i < 8) { base = i + 3; ne = 0; }
    else if (i == 28) { base = 258; ne = 0; }
    else { ne = (i >> 2) - 1; base = ((4u + (i & 3)) << ne) + 3; }
}
__device__ __forceinline__ void dist_base(uint32_t d, uint32_t& base, uint32_t& ne) {
    if (d < 4) { base = d + 1; ne = 0; }
    else { ne = (d >> 1) - 1; base = ((2u + (d & 1)) << ne) + 1; }
}

constexpr uint64_t IN_PAD = 256;           // zero bytes after the staged input
static_assert(IN_PAD == NDFL_IN_PAD_BYTES, "kernel pad and the NDFL_IN_PADDED contract must agree");
// the furthest unchecked reads: In::ld4 clamps 16-byte group indices at (nwords + 3) / 4 + 1, so a
// lane reads at most ((nwords + 3) / 4 + 2) * 16 <= nwords * 4 + 44 bytes; the decode passes' round
// staging (wv::stage_round) clamps word indices at nwords + 60, i.e. nwords * 4 + 244 bytes
static_assert(3 * 4 + 2 * 16 + 16 <= IN_PAD, "16-byte prefetch clamp must stay inside the zero padding");
static_assert((60 + 1) * 4 <= IN_PAD, "round staging clamp must stay inside the zero padding");
#ifndef NDFL_FIND_WPT
#define NDFL_FIND_WPT 16
#endif
constexpr uint32_t FIND_WPT = NDFL_FIND_WPT;     // finder: input words per thread
#ifndef NDFL_STRICT_SLICE
#define NDFL_STRICT_SLICE 128
#endif
#ifndef NDFL_STRICT_REFILL
#define NDFL_STRICT_REFILL 32     // strict stage: refill a wave once this many lanes are idle
#endif
constexpr uint32_t STRICT_SLICE = NDFL_STRICT_SLICE;  // strict stage: survivors per ticket
#ifndef NDFL_COUNT_W_DEFAULT
#define NDFL_COUNT_W_DEFAULT 1
#endif
constexpr uint32_t COUNT_WAVES = 256 * 16;       // count / emit passes: persistent waves at most (the
constexpr uint32_t EMIT_WAVES = 256 * 16;        // grids are sized by occupancy, ndfl_inflate.cpp)

struct In {
    const uint32_t* w;
    uint64_t nwords;
    uint64_t nbits;
    __device__ __forceinline__ uint32_t ld(uint64_t i) const { return i < nwords ? w[i] : 0u; }
    // the input from bit p on (at least 32 bits; zeros past the end)
    __device__ __forceinline__ uint64_t win64(uint64_t p) const {
        const uint64_t i = p >> 5;
        return (((uint64_t)ld(i + 1) << 32) | ld(i)) >> (p & 31);
    }
    // unchecked 16-byte group load; positions past the end are clamped into the zero padding
    __device__ __forceinline__ u32x4 ld4(uint64_t g) const {
        const uint64_t gmax = (nwords + 3) / 4 + 1;
        return *(const u32x4*)(w + min(g, gmax) * 4);
    }
};

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, uint32_t n) { return __brev(v) >> (32 - n); }

// Simple bit reader (finder / validation paths).
struct Rd {
    uint64_t pos, bb;
    uint32_t bn;
    uint64_t nextw;
    __device__ __forceinline__ void init(const In& in, uint64_t p) {
        pos = p; nextw = p >> 5;
        bb = (uint64_t)(in.ld(nextw) >> (p & 31));
        bn = 32 - (uint32_t)(p & 31);
        nextw++;
        fill(in);
    }
    __device__ __forceinline__ void fill(const In& in) {
        if (bn <= 32) { bb |= (uint64_t)in.ld(nextw) << bn; bn += 32; nextw++; }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ __forceinline__ void skip(uint32_t n) { bb >>= n; bn -= n; pos += n; }
    __device__ __forceinline__ uint32_t get(const In& in, uint32_t n) {
        fill(in);
        uint32_t v = n ? peek(n) : 0u;
        skip(n);
        return v;
    }
};

// Decode-lane bit reader: 64-bit active buffer refilled 32 bits at a time from a 4-word group,
// with the next two 4-word groups already in flight (one 16-byte load per 128 bits consumed,
// issued 256 bits ahead of use).  The loads are unconditional (zero-padded input), so nothing
// forces an early wait on them.
struct Rp {
    uint64_t bb;
    uint32_t bn;
    uint32_t ci;          // next word of `cur` (0..3)
    uint64_t qw;          // group index of `cur`
    uint64_t pos;
    u32x4 cur, nxt, nx2;
    __device__ __forceinline__ static uint32_t pick(const u32x4& v, uint32_t i) {
        uint32_t a = (i & 1) ? v.y : v.x, b = (i & 1) ? v.w : v.z;
        return (i & 2) ? b : a;
    }
    __device__ __forceinline__ void adv(const In& in) {
        if (++ci == 4) { cur = nxt; nxt = nx2; qw++; nx2 = in.ld4(qw + 2); ci = 0; }
    }
    __device__ __forceinline__ void init(const In& in, uint64_t p) {
        pos = p;
        qw = p >> 7;
        cur = in.ld4(qw);
        nxt = in.ld4(qw + 1);
        nx2 = in.ld4(qw + 2);
        ci = (uint32_t)(p >> 5) & 3;
        bb = (uint64_t)(pick(cur, ci) >> (p & 31));
        bn = 32 - (uint32_t)(p & 31);
        adv(in);
        fill(in);
    }
    __device__ __forceinline__ void fill(const In& in) {
        if (bn <= 32) { bb |= (uint64_t)pick(cur, ci) << bn; bn += 32; adv(in); }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ __forceinline__ void skip(uint32_t n) { bb >>= n; bn -= n; pos += n; }
    __device__ __forceinline__ uint32_t get(const In& in, uint32_t n) {
        fill(in);
        uint32_t v = n ? peek(n) : 0u;
        skip(n);
        return v;
    }
};

// codeLengthsToCodeTree's error detection (D/decomp/Open.java:705-756) from per-length counts.
// Straight-line (no early exit inside the loop): fully unrolled with constant indices, so the
// counts stay in registers -- a loop with a break left them in scratch memory (round 6).
__device__ __forceinline__ int tree_check(const uint32_t (&cnt)[16]) {
    uint32_t num = 0, maxL = 0;
#pragma unroll
    for (int l = 1; l < 16; l++) { num += cnt[l]; maxL = cnt[l] ? (uint32_t)l : maxL; }
    if (num < 2) return R_UNDER_FULL;
    // (32-bit: end stays below R + 2 <= 2 * 320, or the under-full test has fired -- 64-bit
    // compares of wave-uniform values went through the vector unit)
    const uint32_t R = 2u * (num - 1);
    uint32_t next = 0, end = 2;
    int res = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16; l++) {
        const bool on = l <= maxL && res == 0;
        if (l > 1) {
            const uint32_t open = end - next;
            const bool op = on && open > 0;
            const bool uf = op && end + 2 * (open - 1) >= R;
            res = uf ? (int)R_UNDER_FULL : res;
            const bool adv = op && !uf;
            next = adv ? end : next;
            end = adv ? end + 2 * open : end;
        }
        const bool on2 = on && res == 0;
        const uint32_t c = cnt[l];
        const bool of = on2 && c > end - next;
        res = of ? (int)R_OVER_FULL : res;
        next = (on2 && !of) ? next + c : next;
    }
    if (res) return res;
    if (end != R) return R_INTERNAL;
    if (next < end) return R_UNDER_FULL;
    return 0;
}

// ---- finder ---------------------------------------------------------------------------------
// Strict check of a dynamic block header at bit p with running Kraft sums (no arrays): accepts
// exactly the headers the reference accepts.
__device__ bool strict_dynamic(const In& in, uint64_t p) {
    Rd rd; rd.init(in, p + 3);
    const uint32_t hlit = rd.get(in, 5), hdist = rd.get(in, 5), hclen = rd.get(in, 4);
    const uint32_t numLit = hlit + 257, numDist = hdist + 1, numCl = hclen + 4;
    uint32_t cl[19];
#pragma unroll
    for (int i = 0; i < 19; i++) cl[i] = 0;
#pragma unroll
    for (int i = 0; i < 19; i++)
        if ((uint32_t)i < numCl) cl[CLO[i]] = rd.get(in, 3);
    uint32_t cc[8];
#pragma unroll
    for (int l = 0; l < 8; l++) cc[l] = 0;
#pragma unroll
    for (int l = 1; l < 8; l++) {
        uint32_t c = 0;
#pragma unroll
        for (int s = 0; s < 19; s++) c += cl[s] == (uint32_t)l;
        cc[l] = c;
    }
    uint32_t kr = 0;
#pragma unroll
    for (int l = 1; l < 8; l++) kr += cc[l] << (7 - l);
    if (kr != 128) return false;
    uint32_t first[8], offs[8];
    {
        uint32_t code = 0, off = 0;
        first[0] = 0; offs[0] = 0;
#pragma unroll
        for (int l = 1; l < 8; l++) { code = (code + (l > 1 ? cc[l - 1] : 0)) << 1; first[l] = code; offs[l] = off; off += cc[l]; }
    }
    // canonical symbol list packed 6 x 5 bits per register
    uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 19; s++) {
        const uint32_t l = cl[s];
        if (l) {
            uint32_t rank = 0, o = 0;
#pragma unroll
            for (int s2 = 0; s2 < s; s2++) rank += cl[s2] == l;
#pragma unroll
            for (int l2 = 1; l2 < 8; l2++) o = (l == (uint32_t)l2) ? offs[l2] : o;
            const uint32_t pos = o + rank, wd = pos / 6, sh = (pos % 6) * 5;
#pragma unroll
            for (int q = 0; q < 4; q++) pk[q] |= (wd == (uint32_t)q) ? ((uint32_t)s << sh) : 0u;
        }
    }
    const uint32_t total = numLit + numDist;
    uint32_t i = 0;
    int runVal = -1;
    uint32_t litK = 0, distK = 0, ones = 0, other = 0, eob = 0, d0 = 0, d31 = 0;
    while (i < total) {
        rd.fill(in);
        const uint32_t r7 = rev_bits(rd.peek(7), 7);
        uint32_t sym = 0, len = 0, gi = 0;
#pragma unroll
        for (int l = 1; l < 8; l++) {
            const uint32_t idx = (r7 >> (7 - l)) - first[l];
            if (len == 0 && idx < cc[l]) { len = (uint32_t)l; gi = offs[l] + idx; }
        }
        {
            const uint32_t wd = gi / 6, sh = (gi % 6) * 5;
            uint32_t x = pk[0];
            x = wd == 1 ? pk[1] : x; x = wd == 2 ? pk[2] : x; x = wd == 3 ? pk[3] : x;
            sym = (x >> sh) & 31u;
        }
        rd.skip(len);
        uint32_t run = 1;
        if (sym < 16) runVal = (int)sym;
        else if (sym == 16) { if (runVal < 0) return false; run = rd.get(in, 2) + 3; }
        else if (sym == 17) { runVal = 0; run = rd.get(in, 3) + 3; }
        else { runVal = 0; run = rd.get(in, 7) + 11; }
        if (i + run > total || rd.pos > in.nbits) return false;
        const uint32_t v = (uint32_t)runVal;
        const uint32_t en = i + run;
        if (i < numLit) {
            const uint32_t c = min(en, numLit) - i;
            if (v) { litK += c * (32768u >> v); if (litK > 32768u) return false; }
            if (i <= 256 && 256 < en) eob = v;
        }
        if (en > numLit) {
            const uint32_t a = max(i, numLit) - numLit, b2 = en - numLit, c = b2 - a;
            if (v) { distK += c * (32768u >> v); if (distK > 32768u) return false; if (v == 1) ones += c; else other += c; }
            if (a == 0) d0 = v;
            if (a <= 31 && 31 < b2) d31 = v;
        }
        i = en;
    }
    if (eob == 0 || litK != 32768u) return false;
    if (numDist == 1 && d0 == 0) return true;
    if (ones == 1 && other == 0) return !(numDist == 32 && d31 == 1);
    return distK == 32768u;
}

// A stored block at p (LEN == ~NLEN already checked) must be final or be followed by a plausible
// header: not btype 3; stored -> LEN == ~NLEN; dynamic -> complete code-length code.  (Inlined: the
// strict stage must not use scratch memory, see there.)
__device__ __forceinline__ bool strict_stored(const In& in, uint64_t p) {
    Rd rd; rd.init(in, p);
    const uint32_t bf = rd.get(in, 1);
    const uint64_t al = (p + 3 + 7) & ~7ull;
    rd.init(in, al);
    const uint32_t ln = rd.get(in, 16);
    const uint64_t q = al + 32 + 8ull * ln;
    if (bf) return true;
    if (q + 3 > in.nbits) return false;
    rd.init(in, q);
    rd.get(in, 1);
    const uint32_t bt2 = rd.get(in, 2);
    if (bt2 == 3) return false;
    if (bt2 == 0) {
        const uint64_t al2 = (q + 3 + 7) & ~7ull;
        rd.init(in, al2);
        const uint32_t l2 = rd.get(in, 16), n2 = rd.get(in, 16);
        return l2 == (n2 ^ 0xFFFFu);
    }
    if (bt2 == 2) {
        rd.get(in, 10);
        const uint32_t ncl = rd.get(in, 4) + 4;
        uint32_t kr = 0, nz = 0;
        for (uint32_t i = 0; i < ncl; i++) { uint32_t l = rd.get(in, 3); if (l) { kr += 128u >> l; nz++; } }
        return kr == 128 && nz >= 2;
    }
    return true;   // fixed block: no cheap check
}

}  // namespace inf

// Header finder over every bit position, stage 1 (quick filter): BTYPE from two shifts of the
// input; dynamic headers need a complete code-length code (Kraft sum exactly 1 over the HCLEN+4
// 3-bit lengths); stored headers need LEN == ~NLEN at the next byte boundary and zero padding.
// Survivors (about 1 in 1000 positions) go to a global list for the strict stage.
// (amdgpu_waves_per_eu(N) is the least occupancy the register allocator must leave room for, not the
// occupancy: the finder's 40 VGPRs and 17.5 KB of LDS give 8 waves per SIMD, which
// tests/test_finder_resources.py pins)
#ifndef NDFL_FIND_WPE
#define NDFL_FIND_WPE 3
#endif
#ifndef NDFL_STRICT_WPE
#define NDFL_STRICT_WPE 5
#endif
namespace inf {
// The 32 positions of each input word, for the 64 words of a wave at once.  The cheap masks
// (BTYPE, BFINAL, HLIT/HDIST, stored LEN/NLEN) are bit-sliced per lane (bit i = position p0 + i);
// the positions they leave for the code-length code's Kraft test -- about 1 in 9 -- are compacted
// into a wave list and tested one per lane: the HCLEN + 4 three-bit lengths as one 57-bit field,
// summed by five lookups of a 4,096-entry table of the Kraft sums of four lengths (kr4).  About 30
// operations per such position (round 4; a bit-sliced Kraft test at every position took 451 per
// 32 positions).  A pass takes at most FIND_TAKE positions per lane (a dense pattern takes more
// passes; on the config-4 mix some lane of a wave has more than 8 in 1.5 % of the words).
// A wave whose 64 words and the three after them lie inside the input and the scan range (all but
// the input's last waves) loads them unchecked and needs no `valid` mask; the bounds tests of a
// tested position are done in the other waves only.
constexpr uint32_t FIND_TAKE = 8;
constexpr uint32_t FIND_CLIST = 64 * FIND_TAKE;
constexpr uint32_t FIND_CCAP = 1024;               // survivors listed in LDS per workgroup (131,072 positions; ~65 on average)
struct FindWaveScratch {
    uint32_t w[64 + 4];                            // the wave's words and the three after them
    uint16_t list[FIND_CLIST];                     // lane << 5 | bit of each position to test
};
// (survivors go to the workgroup's LDS list as 32-bit offsets from bit `pb`, bit 31 set: dynamic)
// (a workgroup's survivors past the LDS list's FIND_CCAP go straight to the global list, one global
// atomic each -- periodic bit patterns can pass the filters every few bits, and a dropped survivor
// would be a real header lost at random)
__device__ __forceinline__ void find_spill(uint64_t v, uint64_t* qlist, uint32_t* qcount, uint32_t qcap) {
    const uint32_t g = atomicAdd(qcount, 1u);
    if (g < qcap) qlist[g] = v;
}
// tw0: the wave's first word (wave-uniform); rel0: its first bit as an offset from `pb`.
__device__ __forceinline__ void find_word_wave(const In& in, uint64_t tw0, uint32_t rel0, uint64_t scan_end,
                                               uint32_t* cand, uint32_t* ncand, FindWaveScratch& fw, const uint16_t* kr4,
                                               uint64_t pb, uint64_t* qlist, uint32_t* qcount, uint32_t qcap) {
    const uint64_t nbits = in.nbits;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t t = tw0 + lane;
    const uint64_t p0 = t * 32;
    // an inner wave: every position of its 64 words is valid and in range, and every word that a lane
    // reads exists (nbits <= 32 nwords, scan_end <= nbits)
    const bool inner = (tw0 + 67) * 32 <= nbits && (tw0 + 64) * 32 <= scan_end;
    uint32_t w0, w1, w2, w3, valid = 0xFFFFFFFFu;
    if (inner) {
        const uint32_t* q = in.w + tw0 + lane;
        w0 = q[0]; w1 = q[1]; w2 = q[2]; w3 = q[3];
    } else {
        w0 = in.ld(t); w1 = in.ld(t + 1); w2 = in.ld(t + 2); w3 = in.ld(t + 3);
        if (p0 + 35 > nbits) valid = (nbits >= p0 + 3) ? (uint32_t)((1ull << (nbits - p0 - 2)) - 1) : 0u;
        if (p0 + 32 > scan_end) valid &= p0 < scan_end ? (uint32_t)((1ull << (scan_end - p0)) - 1) : 0u;
    }
    const uint64_t W = (uint64_t)w0 | ((uint64_t)w1 << 32);
    const uint32_t b1 = (uint32_t)(W >> 1), b2 = (uint32_t)(W >> 2);
    const uint32_t notfinal = ~w0;
    const uint32_t h4 = (uint32_t)(W >> 4), h5 = (uint32_t)(W >> 5), h6 = (uint32_t)(W >> 6),
                   h7 = (uint32_t)(W >> 7), d9 = (uint32_t)(W >> 9), d10 = (uint32_t)(W >> 10),
                   d11 = (uint32_t)(W >> 11), d12 = (uint32_t)(W >> 12);
    const uint32_t big = (h4 & h5 & h6 & h7) | (d9 & d10 & d11 & d12);     // HLIT or HDIST >= 30
    const uint32_t pm = ~b1 & b2 & valid & notfinal & ~big;         // before the Kraft test
    // stored headers: LEN == ~NLEN at one of the five byte offsets 1..5 that the word's positions
    // align to.  With V the window w0..w2 and n = ~(V ^ (V >> 16)), LEN == ~NLEN at byte k is "bytes k
    // and k + 1 of n are zero", i.e. byte k of m = n | (n >> 8) is zero: one xor per word and a
    // zero-byte test say whether any offset matches.  Hardly a word has one, so the per-offset masks
    // and the position loop are built only in a wave in which some lane has.
    const uint32_t nlo = ~(w0 ^ (uint32_t)(W >> 16));
    const uint32_t nhi = ~(w1 ^ ((w1 >> 16) | (w2 << 16)));
    const uint32_t mlo = nlo | ((nlo >> 8) | (nhi << 24)), mhi = nhi | (nhi >> 8);
    const uint32_t m14 = (mlo >> 8) | (mhi << 24);                  // bytes 1..4 of m
    const bool lenok = (((m14 - 0x01010101u) & ~m14 & 0x80808080u) | (uint32_t)((mhi & 0xFF00u) == 0)) != 0;
    if (__any(lenok)) {
        const uint64_t W12 = (uint64_t)w1 | ((uint64_t)w2 << 32);
        const uint32_t okm = ((m14 & 0x000000FFu) ? 0u : 0x0000003Fu) | ((m14 & 0x0000FF00u) ? 0u : 0x00003FC0u) |
                             ((m14 & 0x00FF0000u) ? 0u : 0x003FC000u) | ((m14 & 0xFF000000u) ? 0u : 0x3FC00000u) |
                             ((mhi & 0x0000FF00u) ? 0u : 0xC0000000u);
        uint32_t m0 = ~b1 & ~b2 & valid & notfinal & okm;
        while (m0) {
            const uint32_t o = __builtin_ctz(m0);
            m0 &= m0 - 1;
            const uint32_t q = o + 3, al = (q + 7) & ~7u;
            const uint32_t pad = al > q ? (uint32_t)(W >> q) & ((1u << (al - q)) - 1u) : 0u;
            if (pad) continue;
            const uint32_t ln = (al < 32 ? (uint32_t)(W >> al) : (uint32_t)(W12 >> (al - 32))) & 0xFFFFu;
            if (p0 + al + 32 + 8ull * ln <= nbits) {
                uint32_t k = atomicAdd(ncand, 1u);
                if (k < FIND_CCAP) cand[k] = rel0 + (lane << 5) + o;
                else find_spill(p0 + o, qlist, qcount, qcap);
            }
        }
    }
    // dynamic headers
    fw.w[lane] = w0;
    {
        const uint32_t e1 = __shfl(w1, 63, 64), e2 = __shfl(w2, 63, 64), e3 = __shfl(w3, 63, 64);
        if (lane < 3) fw.w[64 + lane] = lane == 0 ? e1 : lane == 1 ? e2 : e3;
    }
    uint32_t rem = pm;
    while (__any(rem != 0)) {                                        // (uniform; no empty scan pass)
        const uint32_t cnt = min((uint32_t)__popc(rem), FIND_TAKE);
        // inclusive wave scan by DPP (row shifts, then the row totals broadcast across rows)
        uint32_t incl = cnt;
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);   // row_shr:1
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);   // row_shr:2
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);   // row_shr:4
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);   // row_shr:8
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false);   // row_bcast:15
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xC, 0xF, false);   // row_bcast:31
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        {
            uint32_t k = incl - cnt;
            for (uint32_t i = 0; i < cnt; i++) {
                fw.list[k++] = (uint16_t)((lane << 5) | __builtin_ctz(rem));
                rem &= rem - 1;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t j = (uint32_t)lane; j < total; j += 64) {
            const uint32_t c = fw.list[j];
            const uint32_t lw = c >> 5, o = c & 31;
            const uint64_t A = (uint64_t)fw.w[lw] | ((uint64_t)fw.w[lw + 1] << 32);
            const uint64_t B = (uint64_t)fw.w[lw + 2] | ((uint64_t)fw.w[lw + 3] << 32);
            const uint32_t ncl = (uint32_t)((A >> (o + 13)) & 15u) + 4;
            const uint32_t sh = o + 17;                              // 17..48
            uint64_t F = (A >> sh) | (B << (64 - sh));
            F &= (1ull << (3 * ncl)) - 1;                            // the HCLEN + 4 lengths (<= 57 bits)
            const uint32_t ks = (uint32_t)kr4[F & 4095] + kr4[(F >> 12) & 4095] + kr4[(F >> 24) & 4095] +
                                kr4[(F >> 36) & 4095] + kr4[(F >> 48) & 4095];
            bool ok = ks == 128;
            if (!inner) ok = ok && tw0 * 32 + c + 17 + 3 * ncl <= nbits;   // (c = 32 lw + o; an inner wave's fields end inside the input)
            if (ok) {
                uint32_t k = atomicAdd(ncand, 1u);
                if (k < FIND_CCAP) cand[k] = (rel0 + c) | (1u << 31);
                else find_spill((pb + rel0 + c) | (1ull << 63), qlist, qcount, qcap);
            }
        }
        __builtin_amdgcn_wave_barrier();                             // (the list is rewritten next)
    }
}
// Kraft sums of four 3-bit lengths (index: four fields, the first in the low bits), x 1/128.  (Ten
// lookups of a 64-entry two-length table -- one entry per LDS bank, no bank conflicts -- measured
// slower: finder phase 6.12 -> 6.50 ms, round 5.)  The table is a constant of the code object; a
// workgroup copies it to LDS with 16-byte loads (computing it per workgroup took ~320 vector
// instructions per thread, for 16 words per thread).
struct Kr4Table { uint16_t v[4096]; };
constexpr Kr4Table kr4_make() {
    Kr4Table t{};
    for (uint32_t i = 0; i < 4096; i++) {
        uint32_t s = 0;
        for (int f = 0; f < 4; f++) { const uint32_t l = (i >> (3 * f)) & 7u; s += l ? 128u >> l : 0u; }
        t.v[i] = (uint16_t)s;
    }
    return t;
}
__device__ const Kr4Table KR4_TABLE __attribute__((aligned(16))) = kr4_make();
__device__ __forceinline__ void kr4_copy(uint16_t* kr4) {
    const u32x4* src = (const u32x4*)KR4_TABLE.v;
    u32x4* dst = (u32x4*)kr4;
    for (uint32_t i = threadIdx.x; i < sizeof(Kr4Table) / 16; i += blockDim.x) dst[i] = src[i];
}

}  // namespace inf

// The dense scan with the compacted Kraft test (find_word_wave): every position of [w_lo * 32, scan_end).
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NDFL_FIND_WPE)))
ndfl_inflate_find_compact_kernel(const uint32_t* w, uint64_t nwords, uint64_t nbits, uint64_t* qlist, uint32_t* qcount,
                                 uint32_t qcap, uint64_t w_lo, uint64_t scan_end) {
    using namespace inf;
    __shared__ uint32_t cand[FIND_CCAP];
    __shared__ uint32_t ncand, gbase;
    __shared__ __attribute__((aligned(16))) uint16_t kr4[4096];
    __shared__ FindWaveScratch fws[4];
    kr4_copy(kr4);
    if (threadIdx.x == 0) ncand = 0;
    __syncthreads();
    In in{w, nwords, nbits};
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t wg0 = w_lo + (uint64_t)blockIdx.x * FIND_WPT * 256;          // the workgroup's first word
    const uint64_t pb = wg0 * 32;                                               // and its first bit
    for (uint32_t kk = 0; kk < FIND_WPT; kk++) {
        const uint32_t wo = kk * 256 + wave * 64;                               // the wave's first word of this round
        find_word_wave(in, wg0 + wo, wo * 32, scan_end, cand, &ncand, fws[wave], kr4, pb, qlist, qcount, qcap);
    }
    // the workgroup's LDS survivors -> the global survivor list (one global atomic)
    __syncthreads();
    const uint32_t nc = min(ncand, FIND_CCAP);
    if (threadIdx.x == 0) gbase = nc ? atomicAdd(qcount, nc) : 0u;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) {
        const uint32_t c = cand[k];
        if (gbase + k < qcap) qlist[gbase + k] = (pb + (c & 0x7FFFFFFFu)) | ((uint64_t)(c >> 31) << 63);
    }
}

namespace inf {
// strict-stage reader: a 256-bit window of the input (two 16-byte groups) in registers and a 64-bit
// bit buffer filled from it.  The window moves wave-wide: when an active lane has used its window
// up, every lane past its first group loads the next two groups, so one memory wait serves the
// wave.  (A per-lane rolling prefetch -- load the next group whenever a lane crosses one -- put a
// load wait into almost every step: with ~40 lanes active some lane crosses a group nearly every
// step, and the compiler waits for the new group where it copies it into the loop's registers.)
struct SRd {
    uint64_t bb, pos, qw;    // bit buffer; the stream position of its bit 0; the window's first group
    uint32_t bn, fi;         // valid bits in bb; the next window word to add to it (8: used up)
    u32x4 cur, nxt;
    __device__ __forceinline__ static uint32_t pick(const u32x4& v, uint32_t i) {
        uint32_t a = (i & 1) ? v.y : v.x, b = (i & 1) ? v.w : v.z;
        return (i & 2) ? b : a;
    }
    __device__ __forceinline__ uint32_t pick8(uint32_t i) const {
        const uint32_t a = pick(cur, i), b = pick(nxt, i);
        return (i & 4) ? b : a;
    }
    __device__ __forceinline__ void load(const In& in, uint64_t g) {
        qw = g;
        cur = in.ld4(g);
        nxt = in.ld4(g + 1);
    }
    // 64 bits from window bit o (o < 160)
    __device__ __forceinline__ uint64_t bits64(uint32_t o) const {
        const uint32_t i = o >> 5, sh = o & 31;
        const uint64_t x = (uint64_t)pick8(i) | ((uint64_t)pick8(i + 1) << 32);
        return sh ? (x >> sh) | ((uint64_t)pick8(i + 2) << (64 - sh)) : x;
    }
    __device__ __forceinline__ void fill() {
        if (bn <= 32 && fi < 8) { bb |= (uint64_t)pick8(fi) << bn; bn += 32; fi++; }
    }
    // the buffer from stream bit p on (p - 128 qw < 224)
    __device__ __forceinline__ void seek(uint64_t p) {
        pos = p;
        const uint32_t o = (uint32_t)(p - qw * 128);
        fi = o >> 5;
        bb = (uint64_t)(pick8(fi) >> (o & 31));
        bn = 32 - (o & 31);
        fi++;
        fill();
    }
    __device__ __forceinline__ bool starved() const { return bn <= 32 && fi >= 8; }
    // move the window to the group holding the next word to add (bb and bn stay)
    __device__ __forceinline__ void reload(const In& in) {
        const uint64_t wn = qw * 4 + fi;
        load(in, wn >> 2);
        fi = (uint32_t)wn & 3u;
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ __forceinline__ void skip(uint32_t n) { bb >>= n; bn -= n; pos += n; }
};
}  // namespace inf

// Stage 2: the reference's own header checks (as strict_dynamic / strict_stored) on every
// survivor.  Each wave takes a contiguous slice of the survivor list; a lane that finishes its
// header takes the next one (refills are batched: at least 16 idle lanes), so short and long
// headers do not hold each other.  Dynamic headers decode the code lengths one symbol per step
// through a per-lane 128-entry table of the code-length code (LDS, indexed by the next 7 bits
// MSB first: canonical codes fill it in (length, symbol) order).  Accepted headers go to their
// 64 KiB segment's list.
// No scratch memory (tests/test_kernel_resources.py checks it): builds that used scratch here -- a
// call to a non-inlined strict_stored (its stack), or register spills at 5 waves/SIMD -- rejected
// 2-4 % of the real headers at full load, a different set on every run, while the same builds
// without scratch accepted exactly the oracle's set in every run.  Hence
// strict_stored is inlined, the code-length code's lengths travel as one 57-bit field, and the
// table build is a rolled loop: 94 VGPRs, no spills, 5 waves/SIMD.
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NDFL_STRICT_WPE)))
ndfl_inflate_strict_kernel(const uint32_t* w, uint64_t nwords, uint64_t nbits, const uint64_t* qlist,
                           const uint32_t* qcount, uint32_t qcap, uint32_t* seg_cnt, uint64_t* seg_list,
                           uint32_t* ticket, unsigned long long* sst) {
    using namespace inf;
    __shared__ uint4 tabs[256 * 8];                          // 128 bytes per lane
    uint8_t* tab = (uint8_t*)&tabs[threadIdx.x * 8];
    const uint32_t n = min(*qcount, qcap);
    In in{w, nwords, nbits};
    const uint32_t lane = threadIdx.x & 63u;
    // survivors are claimed STRICT_SLICE at a time from a global ticket, so the grid is sized to
    // what fits on the chip and waves that draw short headers take more slices
    uint32_t next = 0, end = 0;
    bool drained = false;
    const uint64_t below = (1ull << lane) - 1ull;
    auto record = [&](uint64_t p) {
        const uint32_t seg = (uint32_t)(p / ((uint64_t)SEG_BYTES * 8));
        const uint32_t idx = atomicAdd(&seg_cnt[seg], 1u);
        if (idx < SEG_CAP) seg_list[(uint64_t)seg * SEG_CAP + idx] = p;
    };
    bool active = false;
    uint64_t p = 0;
    SRd rd;
    rd.bb = 0; rd.pos = 0; rd.qw = 0; rd.bn = 0; rd.fi = 8;
    uint32_t i = 0, total = 0, numLit = 0, numDist = 0, litK = 0, distK = 0, nz = 0, eob = 0;
    int runVal = -1;
    uint64_t n_iter = 0, n_refill = 0, n_steps = 0;      // NDFL_STATS (sst != nullptr)
    for (;;) {
        const uint64_t idle = __ballot(!active);
        const uint32_t nidle = (uint32_t)__popcll(idle);
        n_iter++;
        if (next >= end && !drained && nidle >= NDFL_STRICT_REFILL) {
            uint32_t t = 0;
            if (lane == 0) t = atomicAdd(ticket, STRICT_SLICE);
            t = __shfl(t, 0);
            if (t >= n) drained = true;
            else { next = t; end = min(n, t + STRICT_SLICE); }
        }
        if (next < end && nidle >= NDFL_STRICT_REFILL) {
            n_refill++;
            if (!active) {
                const uint32_t k = next + (uint32_t)__popcll(idle & below);
                if (k < end) {
                    const uint64_t e = qlist[k];
                    p = e & ~(1ull << 63);
                    if (!(e >> 63)) {
                        if (strict_stored(in, p)) record(p);
                    } else {
                        // the header's fields straight from the window (p + 74 < 128 qw + 256)
                        rd.load(in, p >> 7);
                        const uint32_t o = (uint32_t)p & 127u;
                        const uint32_t h = (uint32_t)rd.bits64(o + 3);
                        const uint32_t hlit = h & 31u, hdist = (h >> 5) & 31u, hclen = (h >> 10) & 15u;
                        numLit = hlit + 257; numDist = hdist + 1; total = numLit + numDist;
                        const uint32_t numCl = hclen + 4;
                        // the numCl 3-bit code-length code lengths in stream (CLO) order as one field
                        // (two registers where a per-symbol array held 19 at the refill's peak)
                        const uint64_t F = rd.bits64(o + 17) & ((1ull << (3 * numCl)) - 1ull);
                        rd.seek(p + 17 + 3 * numCl);
                        // the stage-1 test guarantees a complete code: the runs fill all 128 entries
                        // canonical (length, symbol) order without a pass per length: each length's
                        // first entry is the byte-wise exclusive prefix sum of count x run, all seven
                        // held in one u64 (byte l = entries taken by lengths < l, at most 128)
                        uint64_t wp = 0;
                        uint32_t kraft = 0;
#pragma unroll
                        for (int sy = 0; sy < 19; sy++) {
                            const uint32_t l = (uint32_t)(F >> (3 * CLO_INV[sy])) & 7u;
                            wp += l ? ((uint64_t)(128u >> l) << (8 * l)) : 0ull;
                            kraft += l ? (128u >> l) : 0u;
                        }
                        // the byte-wise sums only hold for a complete code (every prefix <= 128): a
                        // stage-1 regression must not let an incomplete code scribble over the
                        // neighbouring lanes' tables, so such a survivor is dropped here
                        const bool complete = kraft == 128u;
                        uint64_t off = (wp * 0x0101010101010101ull) << 8;
#pragma unroll 1
                        for (int sy = 0; sy < 19; sy++) {
                            const uint32_t l = (uint32_t)(F >> (3 * CLO_INV[sy])) & 7u;
                            if (l && complete) {
                                const uint32_t sh = 8 * l, run = 128u >> l;
                                const uint32_t pos = (uint32_t)(off >> sh) & 255u;
                                off += (uint64_t)run << sh;
                                const uint32_t v = ((uint32_t)sy | (l << 5)) * 0x01010101u;
                                if (run >= 16) {
                                    for (uint32_t r = 0; r < run; r += 16) *(uint4*)(tab + pos + r) = make_uint4(v, v, v, v);
                                } else if (run == 8) {
                                    *(uint2*)(tab + pos) = make_uint2(v, v);
                                } else if (run == 4) {
                                    *(uint32_t*)(tab + pos) = v;
                                } else if (run == 2) {
                                    *(uint16_t*)(tab + pos) = (uint16_t)v;
                                } else {
                                    tab[pos] = (uint8_t)v;
                                }
                            }
                        }
                        i = 0; runVal = -1; litK = 0; distK = 0; nz = 0; eob = 0;
                        active = complete;
                    }
                }
            }
            next = min(end, next + nidle);
            continue;
        }
        if (!__any(active)) {
            if (next >= end && drained) break;
            continue;
        }
        // steps until enough lanes are idle for a refill (or none is active): a loop of its own, so
        // the step's state stays in place across iterations (the refill above is cold code)
        const bool more = next < end || !drained;
        for (uint32_t ni = nidle;;) {
        n_steps += 64 - ni;
        if (__any(active && rd.starved())) {            // (rare: once per ~20 steps, not per step)
            if (active && rd.fi >= 4) rd.reload(in);
        }
        if (active) {
            // one code-length symbol (D/decomp/Open.java's dynamic header loop, same checks)
            // one refill covers the code (<= 7 bits) and its extra bits (<= 7): no branch per symbol kind
            rd.fill();
            const uint32_t b = (uint32_t)rd.bb;
            const uint32_t te = tab[__builtin_bitreverse32(b) >> 25];
            const uint32_t sym = te & 31u, cl = te >> 5;
            const bool s16 = sym == 16, s17 = sym == 17, s18 = sym == 18;
            const uint32_t nx = s16 ? 2u : s17 ? 3u : s18 ? 7u : 0u;
            const uint32_t ex = (b >> cl) & ((1u << nx) - 1u);
            const uint32_t run = sym < 16 ? 1u : ex + (s18 ? 11u : 3u);
            const bool bad = s16 && runVal < 0;
            runVal = sym < 16 ? (int)sym : s16 ? runVal : 0;
            rd.skip(cl + nx);
            // running Kraft sums of the literal/length part [i, min(en, numLit)) and the distance part
            // (branch-free: the lane's state is only read again if it stays active)
            const uint32_t en = i + run;
            const uint32_t v = (uint32_t)runVal;
            const uint32_t wt = v ? (32768u >> v) : 0u;
            litK += (min(en, numLit) - min(i, numLit)) * wt;
            const uint32_t da = max(i, numLit) - numLit, db = max(en, numLit) - numLit, cd = db - da;
            distK += cd * wt;
            nz += v ? cd : 0u;                  // distance codes of nonzero length
            eob = (i <= 256 && 256 < en) ? v : eob;
            i = en;
            // (past the input end the window reads zeros, which only end the loop: the end test
            // below rejects such a header, as the reference's first read past the end would)
            const bool go = !(bad || en > total) && litK <= 32768u && distK <= 32768u;
            active = go && i < total;
            if (go && i >= total) {
                // the reference's end checks (as strict_dynamic): numDist <= 30 here (stage 1 drops
                // HDIST >= 30), so the single distance code's dummy-31 case cannot arise; one
                // distance code of length 1 is distK == 1/2 with one nonzero length; numDist == 1
                // with a zero length is distK == 0
                bool ok;
                if (eob == 0 || litK != 32768u || rd.pos > in.nbits) ok = false;
                else if (numDist == 1 && distK == 0) ok = true;
                else if (nz == 1 && distK == 16384u) ok = true;
                else ok = distK == 32768u;
                if (ok) record(p);
            }
        }
        const uint64_t am = __ballot(active);
        ni = 64u - (uint32_t)__popcll(am);
        if (!am || (more && ni >= NDFL_STRICT_REFILL)) break;
        n_iter++;
        }
    }
    if (sst && lane == 0) {
        atomicAdd(&sst[0], (unsigned long long)n_iter);
        atomicAdd(&sst[1], (unsigned long long)n_refill);
        atomicAdd(&sst[2], (unsigned long long)n_steps);
        atomicAdd(&sst[3], 1ull);
    }
}
// Sort each segment's candidates (arrival order is arbitrary) and compact them into one sorted
// list at the offsets of an exclusive scan of the segment counts: one wave per segment, each
// candidate placed at its rank among the segment's (positions are distinct), counted against the
// segment's list in LDS.  (One thread per segment with an insertion sort through global memory took
// 0.17 ms, its dense segments' quadratic chains of dependent reads.)
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_compact_kernel(const uint32_t* seg_cnt, const uint64_t* seg_list, const uint64_t* seg_off,
                            uint32_t nseg, uint64_t* out) {
    using namespace inf;
    __shared__ uint64_t sv[4][SEG_CAP];
    const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x * 4 + wid;
    if (seg >= nseg) return;                    // (no workgroup barrier below)
    const uint32_t c = min(seg_cnt[seg], SEG_CAP);
    const uint64_t* src = seg_list + (uint64_t)seg * SEG_CAP;
    uint64_t* o = out + seg_off[seg];
    static_assert(SEG_CAP == 256, "four candidates per lane");
    uint64_t v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t i = lane + 64u * q;
        v[q] = i < c ? src[i] : ~0ull;
        if (i < c) sv[wid][i] = v[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t r[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < c; j++) {
        const uint64_t u = sv[wid][j];
#pragma unroll
        for (int q = 0; q < 4; q++) r[q] += u < v[q] ? 1u : 0u;
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (lane + 64u * q < c) o[r[q]] = v[q];
}

struct ChainRes {
    uint64_t end_bit;     // boundary reached / final block end / error position
    uint64_t out_count;   // output bytes (before the error, if any)
    uint32_t status;      // ST_*
    uint32_t reason;      // for ST_ERROR
    uint32_t next;        // count pass, ST_BOUNDARY at a candidate: its index in the candidate list
    uint32_t pad;
    uint64_t bnd_bit;     // emit pass, ST_ERROR: start bit of the block the error is in
    uint64_t bnd_cnt;     //   and the chain's output bytes before that block (partial-input decodes)
};

struct EmitChain {
    uint64_t start_bit;
    uint64_t end_bit;     // stop at this boundary (or final / error)
    uint64_t out_off;
    uint64_t out_count;
    uint64_t slot;        // count-pass segment record of this chain (>= slot capacity: none)
};

// ---- device-side candidate list and chain linking (one host synchronization per decode) ----------
// Link summary (DevLink::info, u64): the decode's results the host reads once at the end.
enum : uint32_t { LI_NCAND = 0, LI_NCH, LI_TOTAL, LI_FLAGS, LI_STOP, LI_CODE, LI_OUTLEN, LI_CONSUMED, LI_NCAND_ALL,
                  LI_LO, LI_NREP, LI_NFLAT, LI_WORDS = 16 };
enum : uint64_t { LF_REPAIR = 1, LF_RANGE = 2, LF_CAPACITY = 4 };
constexpr uint32_t NOLINK = 0xFFFFFFFFu;

// Exclusive scan of the finder segments' candidate counts (capped at SEG_CAP) from 1 (slot 0 is
// the range start): the compact kernel's offsets; info[LI_NCAND_ALL] = the list length.  Two
// launches (ndfl_common.hpp scan_tile_*); grid = tiles.
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_segsum_kernel(const uint32_t* cnt, uint32_t nseg, uint64_t* part) {
    using namespace inf;
    scan_tile_sum([&](uint32_t i) { return (uint64_t)min(cnt[i], SEG_CAP); }, nseg, part);
}
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_segscan_kernel(const uint32_t* cnt, uint32_t nseg, uint64_t* segoff, uint64_t* info, const uint64_t* part) {
    using namespace inf;
    scan_tile_apply([&](uint32_t i) { return (uint64_t)min(cnt[i], SEG_CAP); },
                    [&](uint32_t i, uint64_t v) { segoff[i] = v; }, nseg, part, 1, info + LI_NCAND_ALL);
}

extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_cand_slice_kernel(const uint64_t* sorted, uint64_t* info, uint64_t start_bit, uint64_t end_bit,
                               uint64_t* cands) {
    __shared__ uint64_t s_lo, s_hi;
    const uint64_t na = info[LI_NCAND_ALL];
    if (threadIdx.x == 0) {
        uint64_t lo = 1, hi = na;                           // first index with value > start_bit
        while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (sorted[m] <= start_bit) lo = m + 1; else hi = m; }
        uint64_t lo2 = lo, hi2 = na;                        // first index with value >= end_bit
        while (lo2 < hi2) { const uint64_t m = (lo2 + hi2) >> 1; if (sorted[m] < end_bit) lo2 = m + 1; else hi2 = m; }
        s_lo = lo; s_hi = lo2;
        if (blockIdx.x == 0) { info[LI_NCAND] = 1 + (lo2 - lo); info[LI_LO] = lo; cands[0] = start_bit; }
    }
    __syncthreads();
    const uint64_t lo = s_lo, n = s_hi - s_lo;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256)
        cands[1 + k] = sorted[lo + k];
}

// Stored-header aliases: a stored block's header can be read at up to 8 bit positions before its
// byte-aligned LEN (the padding between the 3 header bits and the byte boundary is not checked, so
// a header with zero bits before it is also found one, two, ... bits earlier).  Candidates with the
// same BFINAL bit and the same LEN position decode identically from there on, so the count pass
// counts one of them (the first) and the others take its result (ndfl_inflate_alias_copy_kernel).
// Config 2's sync-flush empty stored blocks have ~6 aliases each, each of which otherwise counts
// the whole next piece again.
__device__ __forceinline__ uint64_t stored_key(const inf::In& in, uint64_t p) {
    const uint32_t h = (uint32_t)in.win64(p) & 7u;
    if ((h >> 1) != 0 || p + 3 > in.nbits) return ~0ull;                 // (not a stored header)
    return (((p + 3 + 7) & ~7ull) << 1) | (h & 1u);
}

// rep[k] = the candidate counted for candidate k (the first of its aliases, else k) over the
// info[LI_NCAND] candidates; info[LI_NREP] += the candidates counted (the host reads it with the
// candidate count and picks the count pass's width from it).
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_alias_mark_kernel(const uint64_t* cands, uint64_t* info, const uint32_t* w, uint64_t nwords, uint64_t nbits,
                               uint32_t* rep) {
    const inf::In in{w, nwords, nbits};
    const uint32_t n = (uint32_t)min<uint64_t>(info[LI_NCAND], 0xFFFFFFFFull);
    for (uint32_t k0 = blockIdx.x * 256; k0 < n; k0 += gridDim.x * 256) {
        const uint32_t k = k0 + threadIdx.x;
        bool own = false;
        if (k < n) {
            const uint64_t p = cands[k], key = stored_key(in, p);
            uint32_t r = k;
            if (key != ~0ull)
                for (uint32_t j = k; j > 0 && cands[j - 1] + 10 >= p; j--)
                    if (stored_key(in, cands[j - 1]) == key) r = j - 1;
            rep[k] = r;
            own = r == k;
        }
        const uint32_t c = (uint32_t)__popcll(__ballot(own));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)&info[LI_NREP], (unsigned long long)c);
    }
}

// Bucket orders (the count and emit passes' claim orders) in two launches over tiles of SCAN_TILE
// items, like the scans: the first adds each block's bucket counts into tot[OB_NB]; the second
// places the block's items -- bucket b's slots start at the sum of tot[0..b) plus what the blocks
// before it in arrival order took of bucket b (cursor[b]).  tot and cursor start at zero.  (One
// workgroup over the whole list ran at one CU's bandwidth from other XCDs' data: ~80 us each.)
constexpr uint32_t OB_NB = 24;
constexpr uint32_t OB_WORDS = 2 * OB_NB;      // tot, cursor
constexpr size_t CTK_BYTES = 512;             // chain ticket, nord, two bucket orders, first error

template <class Bk>
__device__ __forceinline__ void border_count(Bk bk, uint32_t n, uint32_t* ob) {
    __shared__ uint32_t h[OB_NB];
    const uint32_t t = threadIdx.x;
    if (t < OB_NB) h[t] = 0;
    __syncthreads();
    const uint32_t i0 = blockIdx.x * SCAN_TILE + t * SCAN_PER;
    if (i0 < n) {
        uint32_t b[SCAN_PER];
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; k++) b[k] = bk(min(i0 + k, n - 1));
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; k++) if (i0 + k < n && b[k] < OB_NB) atomicAdd(&h[b[k]], 1u);
    }
    __syncthreads();
    if (t < OB_NB && h[t]) atomicAdd(&ob[t], h[t]);
}
template <class Bk>
__device__ __forceinline__ void border_place(Bk bk, uint32_t n, uint32_t* ob, uint32_t* order, uint32_t* ntot) {
    __shared__ uint32_t h[OB_NB], base[OB_NB];
    const uint32_t t = threadIdx.x;
    if (t < OB_NB) h[t] = 0;
    __syncthreads();
    const uint32_t i0 = blockIdx.x * SCAN_TILE + t * SCAN_PER;
    uint32_t b[SCAN_PER];
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; k++) b[k] = OB_NB;
    if (i0 < n) {
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; k++) b[k] = bk(min(i0 + k, n - 1));
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; k++) {
            if (i0 + k >= n) b[k] = OB_NB;
            if (b[k] < OB_NB) atomicAdd(&h[b[k]], 1u);
        }
    }
    __syncthreads();
    if (t < OB_NB) {
        uint32_t p = 0;
        for (uint32_t q = 0; q < t; q++) p += ob[q];
        base[t] = p + (h[t] ? atomicAdd(&ob[OB_NB + t], h[t]) : 0u);
        h[t] = 0;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; k++)
        if (b[k] < OB_NB) order[base[b[k]] + atomicAdd(&h[b[k]], 1u)] = i0 + k;
    if (ntot && blockIdx.x == 0 && t == 0) {
        uint32_t p = 0;
        for (uint32_t q = 0; q < OB_NB; q++) p += ob[q];
        *ntot = p;
    }
}

// Claim order of the count pass: longest first by the bits to the next start (24 buckets of 32
// Kibit), so that no long chain is left for the end of the launch.  With `rep`
// (ndfl_inflate_alias_mark_kernel), stored-header aliases are left out of the order (*nord = the
// chains to count).  grid = tiles of n.
struct OrderBucket {
    const uint64_t* cands; uint32_t n; uint64_t end_bit; const uint32_t* rep; const uint32_t* flat;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
        const uint64_t c0 = cands[k], c1 = cands[min(k + 1, n - 1)];
        const uint32_t r = rep ? rep[k] : k;
        const uint64_t nx = k + 1 < n ? c1 : end_bit;
        const uint64_t len = nx > c0 ? nx - c0 : 0;
        if (flat && flat[k]) return OB_NB;      // (counted in flat groups)
        return r == k ? OB_NB - 1 - (uint32_t)min<uint64_t>(OB_NB - 1, len >> 15) : OB_NB;
    }
};
// flat: per candidate, nonzero for a chain counted in a flat group (ndfl_inflate_hdr_kernel), or null
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_order_count_kernel(const uint64_t* cands, uint32_t n, uint64_t end_bit, const uint32_t* rep, uint32_t* ob,
                                const uint32_t* flat) {
    border_count(OrderBucket{cands, n, end_bit, rep, flat}, n, ob);
}
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_order_kernel(const uint64_t* cands, uint32_t n, uint64_t end_bit, uint32_t* order, const uint32_t* rep,
                          uint32_t* nord, uint32_t* ob, const uint32_t* flat) {
    border_place(OrderBucket{cands, n, end_bit, rep, flat}, n, ob, order, nord);
}

// The emit pass's claim order over the linked chain list (info[LI_NCH] chains): costliest first, by
// a cost key of input bits and output bytes (32 Kbit or 16 KiB per unit), so that no long chain --
// a stream's last blocks, which share one chain -- starts at the end of the pass.  grid = tiles of
// an upper bound of the chains (the candidates).
struct EmitBucket {
    const EmitChain* chains;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
        const EmitChain& e = chains[k];
        const uint64_t key = ((e.end_bit - e.start_bit) >> 15) + (e.out_count >> 14);
        return OB_NB - 1 - (uint32_t)min<uint64_t>(OB_NB - 1, key);
    }
};
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_emit_order_count_kernel(const EmitChain* chains, const uint64_t* info, uint32_t* ob) {
    if (info[LI_FLAGS]) return;                 // (the emit pass does not run)
    border_count(EmitBucket{chains}, (uint32_t)info[LI_NCH], ob);
}
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_emit_order_kernel(const EmitChain* chains, const uint64_t* info, uint32_t* order, uint32_t* ob) {
    if (info[LI_FLAGS]) return;
    border_place(EmitBucket{chains}, (uint32_t)info[LI_NCH], ob, order, (uint32_t*)nullptr);
}

// Linking by pointer jumping.  Chain k links to the chain starting where it stopped when it stopped
// at a block boundary that is the next candidate (res[k].next), before the range end; the links form
// a forest (a false candidate's chain may end on a real boundary too).  Init: J0 = the link, S = the
// chain's output bytes, D = 1 if linked.
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_link_init_kernel(const ChainRes* res, uint32_t n, const uint64_t* cands, uint64_t end_bit, uint32_t* J0,
                              uint64_t* S, uint32_t* D) {
    using namespace inf;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const ChainRes r = res[k];
        const bool lk = r.status == ST_BOUNDARY && r.end_bit < end_bit && r.next < n && cands[r.next] == r.end_bit;
        J0[k] = lk ? r.next : NOLINK;
        S[k] = r.out_count;
        D[k] = lk ? 1u : 0u;
    }
}
// One doubling round: J_{r+1} = J_r o J_r, S and D summed along (double-buffered).
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_link_jump_kernel(const uint32_t* J, uint32_t* J2, const uint64_t* S, uint64_t* S2, const uint32_t* D,
                              uint32_t* D2, uint32_t n) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const uint32_t j = J[k];
        if (j != NOLINK) { J2[k] = J[j]; S2[k] = S[k] + S[j]; D2[k] = D[k] + D[j]; }
        else { J2[k] = NOLINK; S2[k] = S[k]; D2[k] = D[k]; }
    }
}
// The chain list from the range start: position t is the chain t links away from chain 0
// (binary lifting over the J levels), its output offset dict_len + S[0] - S[node].  The terminal
// chain sets the summary: chains, total bytes, the stop bit, flags (a boundary that is no
// candidate: repair on the host; the range end inside a block; output beyond out_cap).
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_link_path_kernel(const uint32_t* Jall, uint32_t nlev, const uint64_t* S, const uint32_t* D,
                              const ChainRes* res, const uint64_t* cands, uint32_t n, uint64_t dict_len, uint64_t end_bit,
                              uint64_t out_cap, EmitChain* chains, uint64_t* info) {
    using namespace inf;
    const uint32_t len = D[0] + 1;
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < len; t += gridDim.x * 256) {
        uint32_t node = 0;
        for (uint32_t r = 0; r < nlev; r++)
            if ((t >> r) & 1u) node = Jall[(uint64_t)r * n + node];
        const ChainRes c = res[node];
        EmitChain e;
        e.start_bit = cands[node];
        e.end_bit = c.end_bit;
        e.out_off = dict_len + S[0] - S[node];
        e.out_count = c.out_count;
        e.slot = node;
        chains[t] = e;
        if (t + 1 == len) {
            uint64_t flags = 0, stop = 0;
            if (c.status == ST_FINAL) stop = c.end_bit;
            else if (c.status == ST_BOUNDARY) {
                if (c.end_bit == end_bit) stop = end_bit;
                else if (c.end_bit > end_bit) flags |= LF_RANGE;
                else flags |= LF_REPAIR;
            }
            if (S[0] > out_cap) flags |= LF_CAPACITY;
            info[LI_NCH] = len; info[LI_TOTAL] = S[0]; info[LI_FLAGS] = flags; info[LI_STOP] = stop;
        }
    }
}
// The decode's result from the emit pass's chain results: the first error in stream order (a
// partial-input decode that ran out of input inside a block stops at that block's start instead).
// ndfl_inflate_first_error_kernel (grid = tiles of an upper bound of the chains) leaves the first
// erring chain in *first (set to ~0 before); the summary kernel (one thread) writes the result.
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_inflate_first_error_kernel(const ChainRes* er, const uint64_t* info, uint32_t* first) {
    using namespace inf;
    const uint32_t nch = (uint32_t)info[LI_NCH];
    const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER;
    if (i0 >= nch) return;
    uint32_t st[SCAN_PER];
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; k++) st[k] = er[min(i0 + k, nch - 1)].status;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; k++)
        if (i0 + k < nch && st[k] == ST_ERROR) { atomicMin(first, i0 + k); break; }
}
extern "C" __global__ void __launch_bounds__(64)
ndfl_inflate_summary_kernel(const ChainRes* er, const EmitChain* chains, uint64_t* info, uint64_t dict_len,
                            uint32_t partial, const uint32_t* firstp) {
    using namespace inf;
    if (threadIdx.x != 0) return;
    const uint32_t first = *firstp;
    if (first == NOLINK) {
        info[LI_CODE] = 0; info[LI_OUTLEN] = info[LI_TOTAL]; info[LI_CONSUMED] = info[LI_STOP];
        return;
    }
    const ChainRes r = er[first];
    if (partial && r.reason == R_UEOS) {
        info[LI_CODE] = NEED_INPUT;
        info[LI_OUTLEN] = chains[first].out_off - dict_len + r.bnd_cnt;
        info[LI_CONSUMED] = r.bnd_bit;
    } else {
        info[LI_CODE] = r.reason;
        info[LI_OUTLEN] = chains[first].out_off - dict_len + r.out_count;
        info[LI_CONSUMED] = r.end_bit;
    }
}

// Count-pass records (round records, table records) and the words the host shares with the kernels
#include "inflate_records.hpp"
static_assert((CT_ORDER + 2 * OB_WORDS + 1) * 4 <= CTK_BYTES, "ticket buffer layout");
#include "inflate_wave.hpp"
#include "inflate_wg.hpp"

// Aliases take the result (and the segment records) of the candidate counted for them.
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_alias_copy_kernel(const uint32_t* rep, uint32_t n, ChainRes* res, SegPool pool) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const uint32_t r = rep[k];
        if (r == k) continue;
        res[k] = res[r];
        if (k < pool.nslot) pool.head[k] = r < pool.nslot ? pool.head[r] : NOREC;
    }
}

// The last n bytes of a deferred-window range decode's output once the caller has written the
// window, without resolving the rest: each byte follows its back-references (pending bytes only;
// window bytes are never pending) to a final byte.  A chain longer than TAIL_STEPS sets *fail.
constexpr uint32_t TAIL_STEPS = 4096;
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_tail_kernel(const uint32_t* pend, const uint32_t* ref, const uint8_t* out, uint64_t t0, uint64_t n,
                         uint8_t* dst, uint32_t* fail) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    uint64_t p = t0 + k;
    uint32_t steps = 0;
    while ((pend[p >> 5] >> (p & 31)) & 1) {
        p -= ref[p];
        if (++steps > TAIL_STEPS) { atomicOr(fail, 1u); return; }
    }
    dst[k] = out[p];
}

// The same bytes as a map of the window: entry k = the window byte index its value comes from
// (< dict_len), or TAIL_LITERAL | value for a byte that does not depend on the window.  Needs no
// window content: GPU r's map composed with the maps of GPUs 0..r-1 gives its window directly.
constexpr uint32_t TAIL_LITERAL = 0x80000000u;
extern "C" __global__ void __launch_bounds__(256)
ndfl_inflate_tail_map_kernel(const uint32_t* pend, const uint32_t* ref, const uint8_t* out, uint64_t t0, uint64_t n,
                             uint64_t dict_len, uint32_t* dst, uint32_t* fail) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    uint64_t p = t0 + k;
    uint32_t steps = 0;
    while ((pend[p >> 5] >> (p & 31)) & 1) {
        p -= ref[p];
        if (++steps > TAIL_STEPS) { atomicOr(fail, 1u); return; }
    }
    dst[k] = p < dict_len ? (uint32_t)p : TAIL_LITERAL | out[p];
}
