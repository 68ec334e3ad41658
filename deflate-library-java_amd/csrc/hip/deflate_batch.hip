// deflate_batch.hip -- batched deflate: many independent buffers compressed in one launch
// (ndfl_deflate_batch, include/ndfl.h), the encoder's counterpart of inflate_batch.hip.
//
// ndfl_deflate_chunks parallelises INSIDE a stream: a 1024-thread workgroup per chunk, about eight
// launches and a host wait per call -- the whole cost of a 300-byte record.  This kernel parallelises
// ACROSS streams: a persistent grid of one-wave workgroups, each wave claiming stream indices from an
// atomic ticket and encoding its stream chunk by chunk, serially, carrying the bit position from
// block to block.  No workgroup waits on another: there is no look-back and no status word.
//
// Stream i is DeflaterOutputStream(out, chunk_len, hist_limit, strategy): write all bytes, finish()
// (D/DeflaterOutputStream.java:119-171) for the RLE_* and LITERAL_* presets of
// D/comp/Lz77Huffman.java:298-305, and optionally the trailer of D/ZlibOutputStream.java /
// D/GzipOutputStream.java.  Per chunk (= block) the wave walks the bytes in steps of 64 lanes x BPL
// contiguous bytes, twice:
//   count walk (dynamic codes only): the closed-form greedy RLE parse (D/comp/Lz77Huffman.java:62-130
//       with distance 1, runs 3..258) into the LDS histograms;
//   build_block_codes<64> (huffman_build.hpp, the one code builder): codes and header;
//   emit walk: the bytes again, folded into the stream's CRC-32 / Adler-32 on the way, each lane's
//       token bits counted, wave-scanned and put into the LDS bit buffer (BitPut), which is flushed
//       to the stream's region whenever the next step might not fit.
// Run pieces (maximal runs of one byte value inside a chunk) are cut at no lane or step boundary: a
// lane owns the pieces that START in its bytes, a piece's end is the next start (the lane's own next
// one, else the later lanes' first: a wave suffix-minimum), and the LAST piece started in a step is
// not tokenised there but carried (value, length so far, lead) into the next step, where it grows by
// the bytes before that step's first start and is closed by lane 0; the chunk's end closes it too.
// A chunk's first piece has no lead literal when the stream's previous byte equals it and
// hist_limit > 0 (the has_prev0 rule of deflate_kernels.hip).
//
// Region ends: the bit buffer is stored as the bytes [wbase, ...) of the stream's region, 32-bit
// stores for the words of `out` that lie wholly inside [out_off, out_off + min(out_len, out_cap)),
// byte stores for the partial words at its two ends -- nothing outside is written, at any alignment.
// Past out_cap the encoder goes on without storing, which gives NDFL_E_CAPACITY its required size.
//
// The kernel has no scratch memory: everything is forced inline (a real call's stack lives in
// scratch), and the 16 bytes a lane holds are four named words, never an array
// indexed by a variable.
// The builder runs with an opaque lane index (build_block_codes<64, true>), and so does every step
// here (opaque_lane, ndfl_common.hpp): lane masks taken from threadIdx are invariant in the loop over
// streams, get hoisted to the kernel's entry and are held in scalar pairs across everything (62 spilled
// SGPRs with the plain lane index, none with the opaque one).
// D/ = src/io/nayuki/deflate/ in the reference
#pragma once
#include "huffman_build.hpp"

namespace dbat {

constexpr uint32_t BPL = 16;                  // bytes per lane and step
constexpr uint32_t STEP = 64 * BPL;           // bytes per step
// Bit buffer words.  The most one make_room() is asked for: a step's tokens (<= 15 bits per byte:
// 15,360), a carried piece (lead + 254 x 30 + 35 bits), a header (<= 32 * HDRW bits) -- on top of
// the < 32 bits a flush leaves.
constexpr uint32_t OBW = 640;
static_assert(31 + 15 * STEP <= 32 * OBW && 31 + 32 * HDRW <= 32 * OBW && 31 + 15 + 254 * 30 + 35 <= 32 * OBW,
              "a step, a header and a carried piece each fit the flushed bit buffer");
constexpr uint32_t NONE = 0xFFFFFFFFu;

// What every kernel of the stream frame (below) is given; deflate_batch_lz.hip's Args start with it too.
struct FrameArgs {
    const uint8_t* in;
    uint8_t* out;
    const ndfl_member_item* items;
    ndfl_deflate_result* results;
    uint32_t n;
    uint32_t chunk_len;
    uint32_t* ticket;         // zeroed
};

struct Args : FrameArgs {
    int32_t hist_enabled;     // historyLookbehindLimit > 0
    int32_t rle;              // 1: RLE preset (dist 1, runs 3..258); 0: LITERAL preset
    int32_t dynamic;
    const uint32_t* crc_tab;  // slicing-by-4 tables (1024 u32)
    const uint32_t* crc_x;    // x^(8k) k<64 then x^(8*64k) k<1024
};

// LDS of one wave: 12,632 bytes, 12 waves per CU (3 per SIMD; 160 KiB / 12,632 = 12.97).  The stream
// frame's part of it: deflate_batch_lz.hip's Lds adds its head table behind.
struct Lds {
    HuffScr scr;              // (first: pm_lengths reads its keys 16 bytes at a time)
    uint32_t litCode[288];    // rev(code) | len << 16
    uint32_t distCode[32];
    uint32_t obuf[OBW + 1];   // bit buffer; the spare word is the one a full buffer's BitPut points at
    uint32_t ticket;
};

__device__ __forceinline__ uint32_t rfl(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane(x); }

// Wave-uniform values that are needed rarely are parked in vector registers (every lane holds the
// same value) and made scalar again where they are used: the code builder keeps its per-length
// values scalar, and with the stream's state scalar too the kernel spilled SGPRs (as inflate_batch.hip).
// to_s goes through to_v again, so the read-back stays where it is written and is not hoisted.
__device__ __forceinline__ uint32_t to_v(uint32_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint64_t to_v(uint64_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint32_t to_s(uint32_t x) { return rfl(to_v(x)); }
__device__ __forceinline__ uint64_t to_s(uint64_t x) {
    x = to_v(x);
    return ((uint64_t)rfl((uint32_t)(x >> 32)) << 32) | rfl((uint32_t)x);
}

// One stream's output (wave-uniform): the bit buffer holds the stream's bits from byte wbase on.  Only
// the fill is scalar; the region and wbase are needed at a flush alone and stay parked (to_v).
struct BitOut {
    uint32_t* obuf;
    uint64_t v_optr;          // out + out_off
    uint64_t v_cap;           // out_cap
    uint64_t v_wbase;         // the stream byte obuf[0] starts at (a multiple of 4)
    uint32_t fill;            // bits in obuf
};

// Bytes [0, nb) of the bit buffer to bytes [wbase, wbase + nb) of the region, clamped to out_cap.
// Lane j takes the aligned word j of `out` from the first one the span touches: stored whole when
// all four of its bytes are the span's, bytewise otherwise.
__device__ __forceinline__ void store_bytes(const BitOut& bo, uint32_t nb) {
    const int lane = opaque_lane();
    const uint64_t wbase = to_s(bo.v_wbase);
    const uint64_t e = min(wbase + nb, to_s(bo.v_cap));
    if (wbase >= e) return;
    const uint32_t n = (uint32_t)(e - wbase);
    uint8_t* A = (uint8_t*)(uintptr_t)(to_s(bo.v_optr) + wbase);
    const uint32_t mis = (uint32_t)((uintptr_t)A & 3);
    uint8_t* Ab = A - mis;                    // (only bytes at or past A are stored)
    const uint32_t ng = (mis + n + 3) >> 2;
    for (uint32_t j = (uint32_t)lane; j < ng; j += 64) {
        const uint32_t lo = j ? bo.obuf[j - 1] : 0u;
        const uint32_t hi = j <= OBW ? bo.obuf[j] : 0u;
        const uint32_t val = (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - 8 * mis));
        const int32_t b0 = (int32_t)(4 * j) - (int32_t)mis;      // the buffer byte of this word's byte 0
        if (b0 >= 0 && (uint32_t)b0 + 4 <= n) {
            *(uint32_t*)(Ab + 4 * (size_t)j) = val;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int32_t b = b0 + k;
                if (b >= 0 && (uint32_t)b < n) Ab[4 * (size_t)j + k] = (uint8_t)(val >> (8 * k));
            }
        }
    }
}

// Room for `bits` more bits: the buffer's whole words go out, its partial word moves to the front.
__device__ __forceinline__ void make_room(BitOut& bo, uint32_t bits) {
    if (bo.fill + bits <= 32 * OBW) return;
    const int lane = opaque_lane();
    const uint32_t nw = bo.fill >> 5;
    __syncthreads();
    store_bytes(bo, 4 * nw);
    const uint32_t part = (bo.fill & 31) ? bo.obuf[nw] : 0u;
    __syncthreads();
    for (uint32_t j = (uint32_t)lane; j <= nw; j += 64) bo.obuf[j] = 0;
    __syncthreads();
    if (lane == 0) bo.obuf[0] = part;
    __syncthreads();
    bo.v_wbase = to_v(to_s(bo.v_wbase) + 4 * (uint64_t)nw);
    bo.fill &= 31;
}

// ---- the tokens of one run piece (D/comp/Lz77Huffman.java:62-130, closed form) ---------------------
// A piece of plen bytes of value v whose first `lead` (0 or 1) bytes are a literal: R = plen - lead
// bytes can be matches at distance 1 -- R / 258 runs of 258, then the rest m as one run (m >= 3) or m
// literals.
template <class Sink>
__device__ __forceinline__ void piece_tokens(uint32_t v, uint32_t plen, uint32_t lead, Sink& s) {
    const uint32_t R = plen - lead;
    const uint32_t n258 = R / 258, m = R - n258 * 258;
    if (lead) s.lit(v, 1);
    if (n258) s.run258(n258);
    if (m >= 3) s.run(m);
    else if (m) s.lit(v, m);
}

struct HistSink {
    uint32_t* hl;
    uint32_t* hd;
    __device__ __forceinline__ void lit(uint32_t v, uint32_t n) { atomicAdd(&hl[v], n); }
    __device__ __forceinline__ void run258(uint32_t n) { atomicAdd(&hl[285], n); atomicAdd(&hd[0], n); }
    __device__ __forceinline__ void run(uint32_t m) {
        uint32_t sym, ne, ex; run_sym(m, sym, ne, ex);
        atomicAdd(&hl[sym], 1u); atomicAdd(&hd[0], 1u);
    }
};
// the block's wave-uniform codes: run of 258 with its distance joined (<= 30 bits), the distance code
struct Codes {
    const uint32_t* lc;
    uint32_t m258, m258l, d0c, d0l;
};
struct CountSink {
    Codes c;
    uint32_t bits;
    __device__ __forceinline__ void lit(uint32_t v, uint32_t n) { bits += n * (c.lc[v] >> 16); }
    __device__ __forceinline__ void run258(uint32_t n) { bits += n * c.m258l; }
    __device__ __forceinline__ void run(uint32_t m) {
        uint32_t sym, ne, ex; run_sym(m, sym, ne, ex);
        bits += (c.lc[sym] >> 16) + ne + c.d0l;
    }
};
struct PutSink {
    Codes c;
    BitPut bp;
    __device__ __forceinline__ void lit(uint32_t v, uint32_t n) {
        const uint32_t e = c.lc[v];
        for (uint32_t k = 0; k < n; k++) bp.put(e & 0xFFFF, e >> 16);
    }
    __device__ __forceinline__ void run258(uint32_t n) {
        for (uint32_t k = 0; k < n; k++) bp.put(c.m258, c.m258l);
    }
    __device__ __forceinline__ void run(uint32_t m) {
        uint32_t sym, ne, ex; run_sym(m, sym, ne, ex);
        const uint32_t sc = c.lc[sym];
        bp.put(sc & 0xFFFF, sc >> 16);
        bp.put(ex, ne);
        bp.put(c.d0c, c.d0l);
    }
};

// byte i (0..15) of a lane's four words: selects, no variable register index
__device__ __forceinline__ uint32_t byte_at(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) {
    const uint32_t w = i < 8 ? (i < 4 ? w0 : w1) : (i < 12 ? w2 : w3);
    return (w >> (8 * (i & 3))) & 0xFFu;
}

// The tokens of the pieces that start in this lane's bytes (F: bit i = a piece starts at byte i, at
// step position t0 + i) and end in the step: a piece ends at the lane's next start, else at the later
// lanes' first one (nxt); the step's last piece (no start after it: NONE) is the carried one, not
// taken here.  zl0: the step is a chunk's first and a first piece of value prev0 has no lead literal.
template <class Sink>
__device__ __forceinline__ void lane_pieces(uint32_t F, uint32_t t0, uint32_t nxt, uint32_t w0, uint32_t w1, uint32_t w2,
                                            uint32_t w3, bool zl0, uint32_t prev0, Sink& s) {
    for (uint32_t f = F; f;) {
        const uint32_t i = (uint32_t)__builtin_ctz(f);
        f &= f - 1;
        const uint32_t q = f ? t0 + (uint32_t)__builtin_ctz(f) : nxt;
        if (q == NONE) break;
        const uint32_t v = byte_at(w0, w1, w2, w3, i);
        piece_tokens(v, q - (t0 + i), (zl0 && t0 + i == 0 && v == prev0) ? 0u : 1u, s);
    }
}

// wave_sum / wave_xor with the lane index given (an opaque_lane(), see there)
__device__ __forceinline__ uint32_t wave_sum_l(uint32_t x, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += lane_value(x, lane ^ o);
    return x;
}
__device__ __forceinline__ uint32_t wave_xor_l(uint32_t x, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x ^= lane_value(x, lane ^ o);
    return x;
}

// A lane's vcnt (<= BPL) bytes from p as four words (zero past them), from the aligned words that hold them.
__device__ __forceinline__ void load_lane(const uint8_t* p, uint32_t vcnt, uint32_t& w0, uint32_t& w1, uint32_t& w2,
                                          uint32_t& w3) {
    w0 = 0; w1 = 0; w2 = 0; w3 = 0;
    if (vcnt == BPL) {
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
        const uint32_t* q = (const uint32_t*)(p - mis);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
        const uint32_t a4 = mis ? q[4] : 0u;                 // (holds the lane's last byte: readable)
        const uint32_t sh = 8 * mis;
        w0 = __builtin_amdgcn_alignbit(a1, a0, sh);
        w1 = __builtin_amdgcn_alignbit(a2, a1, sh);
        w2 = __builtin_amdgcn_alignbit(a3, a2, sh);
        w3 = __builtin_amdgcn_alignbit(a4, a3, sh);
    } else if (vcnt) {
#pragma unroll
        for (uint32_t i = 0; i < BPL; i++) {
            if (i < vcnt) {
                const uint32_t b = (uint32_t)p[i] << (8 * (i & 3));
                if (i < 4) w0 |= b; else if (i < 8) w1 |= b; else if (i < 12) w2 |= b; else w3 |= b;
            }
        }
    }
}

// One step of a walk over a chunk's bytes, 64 lanes x BPL contiguous bytes: the step has L bytes, of
// which lane `lane` holds the vcnt from step position t0 on (w0..w3, load_lane).
struct Step {
    int lane;
    uint32_t t0, L, vcnt, w0, w1, w2, w3;
};
// The step at byte sb of the len_c bytes at cp.
__device__ __forceinline__ Step load_step(const uint8_t* cp, uint32_t len_c, uint32_t sb) {
    Step q;
    q.lane = opaque_lane();
    q.t0 = (uint32_t)q.lane * BPL;
    q.L = min(STEP, len_c - sb);
    q.vcnt = q.L > q.t0 ? min(BPL, q.L - q.t0) : 0u;
    load_lane(cp + sb + q.t0, q.vcnt, q.w0, q.w1, q.w2, q.w3);
    return q;
}

// A step's bytes into the checksum ck (kind: NDFL_SUM_*).
__device__ __forceinline__ void fold_step(uint64_t v_tab, uint32_t kind, const Step& q, uint32_t& ck) {
    const int lane = q.lane;
    const uint32_t L = q.L, t0 = q.t0, vcnt = q.vcnt, w0 = q.w0, w1 = q.w1, w2 = q.w2, w3 = q.w3;
    const uint32_t after = vcnt ? L - (t0 + vcnt) : 0u;      // the step's bytes behind this lane's
    if (kind == NDFL_SUM_CRC32) {
        const uint32_t* T0 = (const uint32_t*)(uintptr_t)to_s(v_tab);     // slicing-by-4 tables, then x^(8k)
        const uint32_t* T1 = T0 + 256;
        const uint32_t* T2 = T0 + 512;
        const uint32_t* T3 = T0 + 768;
        const uint32_t* crc_x = T0 + 1024;
        uint32_t cr = 0;
        const uint32_t nfull = vcnt >> 2;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (k < nfull) {
                const uint32_t x = cr ^ (k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3);
                cr = T3[x & 0xFF] ^ T2[(x >> 8) & 0xFF] ^ T1[(x >> 16) & 0xFF] ^ T0[x >> 24];
            }
        }
        for (uint32_t i = nfull * 4; i < vcnt; i++) cr = T0[(cr ^ byte_at(w0, w1, w2, w3, i)) & 0xFF] ^ (cr >> 8);
        uint32_t contrib = 0;
        if (vcnt) {
            uint32_t sh = crc_x[64 + (after >> 6)];
            if (after & 63) sh = crc_multmodp(crc_x[after & 63], sh);
            contrib = crc_multmodp(sh, cr);
        }
        const uint32_t span = wave_xor_l(contrib, lane);
        uint32_t xl = crc_x[64 + (L >> 6)];
        if (L & 63) xl = crc_multmodp(crc_x[L & 63], xl);
        ck = crc_multmodp(xl, ck) ^ span;
    } else if (kind == NDFL_SUM_ADLER32) {
        // per lane s1 = sum of its bytes, s2 = sum of its running s1; the bytes behind the lane
        // count its s1 once each.  s1 <= 4,080, s2 <= 34,680, s1 * after < 2^22: 64 of them < 2^32
        uint32_t s1 = 0, s2 = 0;
#pragma unroll
        for (uint32_t i = 0; i < BPL; i++) {
            if (i < vcnt) {
                s1 += ((i < 4 ? w0 : i < 8 ? w1 : i < 12 ? w2 : w3) >> (8 * (i & 3))) & 0xFFu;
                s2 += s1;
            }
        }
        const uint32_t S1 = wave_sum_l(s1, lane), T = wave_sum_l(s2 + s1 * after, lane);
        const uint32_t A = ck & 0xFFFFu, B = ck >> 16;
        const uint32_t nb = (B + (L * A) % 65521u + T % 65521u) % 65521u, na = (A + S1) % 65521u;
        ck = nb << 16 | na;
    }
}

// The carried piece's tokens, by lane 0 (hist) or counted by all and put by lane 0 (emit).
template <bool EMIT>
__device__ __forceinline__ void close_carry(Lds& S, BitOut& bo, const Codes& cd, uint32_t cval, uint32_t clen,
                                            uint32_t clead) {
    const int lane = opaque_lane();
    if constexpr (!EMIT) {
        if (lane == 0) {
            HistSink hs{S.scr.hlit, S.scr.hdist};
            piece_tokens(cval, clen, clead, hs);
        }
    } else {
        CountSink cs{cd, 0u};
        piece_tokens(cval, clen, clead, cs);
        const uint32_t bits = rfl(cs.bits);
        make_room(bo, bits);
        if (lane == 0) {
            PutSink ps; ps.c = cd; ps.bp.init(bo.obuf, bo.fill);
            piece_tokens(cval, clen, clead, ps);
            ps.bp.flush();
        }
        bo.fill += bits;
    }
}

// One walk over a chunk's bytes: EMIT = false counts the tokens into S.scr.hlit / hdist, EMIT = true
// folds the bytes into the checksum ck (kind: NDFL_SUM_*) and puts the token bits.  prev0 = the
// stream's byte before the chunk, zl = a first piece of that value has no lead literal.  Returns the
// chunk's last byte (prev0 for an empty chunk).
template <bool EMIT>
__device__ __forceinline__ uint32_t walk_chunk(bool rle, uint64_t v_tab, Lds& S, BitOut& bo, const Codes& cd,
                                               const uint8_t* cp, uint32_t len_c, uint32_t prev0, bool zl, uint32_t kind,
                                               uint32_t& ck) {
    uint32_t prevb = prev0;
    bool open = false;
    uint32_t cval = 0, clen = 0, clead = 1;
    for (uint32_t sb = 0; sb < len_c; sb += STEP) {
        // load_step's text, kept here: with the step taken from load_step the compiler orders the start
        // mask below differently, and the kernel was 1.5 % slower on 512-byte streams (and 3.4 % faster on
        // 1 MiB ones): profiles/batch_frame_ab.txt
        const int lane = opaque_lane();
        const uint32_t t0 = (uint32_t)lane * BPL;
        const uint32_t L = min(STEP, len_c - sb);
        const uint32_t vcnt = L > t0 ? min(BPL, L - t0) : 0u;
        uint32_t w0, w1, w2, w3;
        load_lane(cp + sb + t0, vcnt, w0, w1, w2, w3);
        // ---- checksum of the bytes on their way through -------------------------------------------
        if (EMIT) { Step q{lane, t0, L, vcnt, w0, w1, w2, w3}; fold_step(v_tab, kind, q, ck); }
        // ---- piece starts: bit i = byte i differs from the byte before it ---------------------------
        uint32_t F;
        {
            const uint32_t up = lane_value(w3 >> 24, lane - 1);
            const uint32_t pb = lane ? up : prevb;
            if (rle) {
                F = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t wk = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
                    const uint32_t bk = k == 0 ? pb : (k == 1 ? w0 : k == 2 ? w1 : w2) >> 24;
                    const uint32_t x = wk ^ ((wk << 8) | bk);
                    const uint32_t hb = ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u) >> 7;
                    F |= (((hb * 0x00204081u) >> 21) & 0xFu) << (4 * k);
                }
                if (sb == 0 && lane == 0) F |= 1u;
            } else {
                F = 0xFFFFu;
            }
            F &= (1u << vcnt) - 1u;
        }
        const uint32_t fsl = F ? t0 + (uint32_t)__builtin_ctz(F) : NONE;
        const uint32_t nxt = wave_excl_suffix_min_l(fsl, NONE, lane);   // the later lanes' first start
        const uint32_t fs = rfl(min(fsl, nxt));                          // the step's first start (lane 0's)
        if (open) {
            if (fs == NONE) clen += L;
            else { clen += fs; close_carry<EMIT>(S, bo, cd, cval, clen, clead); open = false; }
        }
        const bool zl0 = zl && sb == 0;
        // ---- the pieces that start AND end in this step (all but the last one started) --------------
        if constexpr (EMIT) {
            CountSink cs{cd, 0u};
            lane_pieces(F, t0, nxt, w0, w1, w2, w3, zl0, prev0, cs);
            const uint32_t mybits = cs.bits;
            const uint32_t incl = wave_incl_scan_l(mybits, lane);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
            make_room(bo, total);
            PutSink ps; ps.c = cd; ps.bp.init(bo.obuf, bo.fill + incl - mybits);
            lane_pieces(F, t0, nxt, w0, w1, w2, w3, zl0, prev0, ps);
            ps.bp.flush();
            bo.fill += total;
        } else {
            HistSink hs{S.scr.hlit, S.scr.hdist};
            lane_pieces(F, t0, nxt, w0, w1, w2, w3, zl0, prev0, hs);
        }
        // ---- the step's last start opens the carried piece ------------------------------------------
        if (fs != NONE) {
            const uint64_t bal = __ballot(F != 0);
            const int hl = 63 - (int)__builtin_clzll(bal);
            const uint32_t li = F ? 31u - (uint32_t)__builtin_clz(F) : 0u;
            const uint32_t lv = byte_at(w0, w1, w2, w3, li);
            cval = (uint32_t)__builtin_amdgcn_readlane(lv, hl);
            const uint32_t lp = (uint32_t)__builtin_amdgcn_readlane(t0 + li, hl);
            clen = L - lp;
            clead = (zl0 && lp == 0 && cval == prev0) ? 0u : 1u;
            open = true;
        }
        // the step's last byte: before the next step's first
        {
            const uint32_t lb = vcnt ? byte_at(w0, w1, w2, w3, vcnt - 1) : 0u;
            prevb = (uint32_t)__builtin_amdgcn_readlane(lb, (int)((L - 1) / BPL));
        }
    }
    if (open) close_carry<EMIT>(S, bo, cd, cval, clen, clead);
    return prevb;
}

// ---- the stream frame ------------------------------------------------------------------------------
// What ndfl_deflate_batch_kernel and ndfl_deflate_batch_lz_kernel (deflate_batch_lz.hip) do around a
// block's tokens: claim a stream, start it, start and end a dynamic block's histograms, put the header
// and the end-of-block code, finish the stream.  One text for both, forced inline.
//
// The frame's arguments are needed once per stream or per chunk: parked (see to_v).
struct Frame {
    uint64_t v_in, v_out, v_items, v_results, v_ticket;
    uint32_t v_n, v_chunk_len;
};
__device__ __forceinline__ Frame park_frame(const FrameArgs& a) {
    Frame f;
    f.v_in = to_v((uint64_t)(uintptr_t)a.in); f.v_out = to_v((uint64_t)(uintptr_t)a.out);
    f.v_items = to_v((uint64_t)(uintptr_t)a.items); f.v_results = to_v((uint64_t)(uintptr_t)a.results);
    f.v_ticket = to_v((uint64_t)(uintptr_t)a.ticket);
    f.v_n = to_v(a.n); f.v_chunk_len = to_v(a.chunk_len);
    return f;
}

// The stream's constants, parked too, and its running checksum, parked across the code construction.
struct Stream {
    uint32_t v_si;            // its index
    uint64_t v_src, v_len;    // in + in_off, in_len
    uint32_t v_fmt, v_kind;   // NDFL_FMT_*; NDFL_SUM_*: the container's, else the item's
    uint32_t v_ck;
};

// The next stream index from the ticket; false when none is left.
__device__ __forceinline__ bool claim_stream(Lds& S, const Frame& f, Stream& st) {
    __syncthreads();
    if (opaque_lane() == 0) S.ticket = atomicAdd((uint32_t*)(uintptr_t)to_s(f.v_ticket), 1u);
    __syncthreads();
    st.v_si = to_v(S.ticket);
    return to_s(st.v_si) < to_s(f.v_n);
}

// The claimed stream's item into st, its checksum's initial value, and its output: an empty, zeroed
// bit buffer at the region's first byte.
__device__ __forceinline__ BitOut begin_stream(Lds& S, const Frame& f, Stream& st) {
    BitOut bo{S.obuf, 0ull, 0ull, to_v((uint64_t)0), 0u};
    {
        const ndfl_member_item it = ((const ndfl_member_item*)(uintptr_t)to_s(f.v_items))[to_s(st.v_si)];
        st.v_src = to_v(to_s(f.v_in) + it.in_off); st.v_len = to_v(it.in_len);
        bo.v_optr = to_v(to_s(f.v_out) + it.out_off); bo.v_cap = to_v(it.out_cap);
        st.v_fmt = to_v(it.format);
        st.v_kind = to_v(it.format == NDFL_FMT_ZLIB ? NDFL_SUM_ADLER32 : it.format == NDFL_FMT_GZIP ? NDFL_SUM_CRC32 : it.sum);
    }
    {
        const uint32_t kind = to_s(st.v_kind);
        st.v_ck = to_v(kind == NDFL_SUM_CRC32 ? 0xFFFFFFFFu : kind == NDFL_SUM_ADLER32 ? 1u : 0u);
    }
    for (uint32_t j = (uint32_t)opaque_lane(); j <= OBW; j += 64) S.obuf[j] = 0;
    return bo;
}

// A dynamic block's histograms: zeroed before its tokens are counted (the caller syncs) ...
__device__ __forceinline__ void begin_block_hist(Lds& S) {
    const int lane = opaque_lane();
    for (int t = lane; t < 288; t += 64) S.scr.hlit[t] = 0;
    if (lane < 32) S.scr.hdist[lane] = 0;
}
// ... and, after them, the counts that no byte of the chunk gives.
__device__ __forceinline__ void end_block_hist(Lds& S, uint32_t len_c) {
    if (opaque_lane() == 0) {
        atomicAdd(&S.scr.hlit[256], 1u);                  // end of block (D/comp/Lz77Huffman.java:131-132)
        if (len_c == 0) atomicAdd(&S.scr.hlit[0], 1u);    // (:146-147)
    }
}

// The block's header (S.scr.hdr(), hb bits, zero past them) into the bit buffer.
__device__ __forceinline__ void put_header(Lds& S, BitOut& bo, uint32_t hb) {
    make_room(bo, hb);
    for (uint32_t k = (uint32_t)opaque_lane(); 32 * k < hb; k += 64) {
        const uint32_t nbk = min(32u, hb - 32 * k), word = S.scr.hdr()[k];
        BitPut bp; bp.init(bo.obuf, bo.fill + 32 * k);
        bp.put(word & 0xFFFF, min(nbk, 16u));
        if (nbk > 16) bp.put(word >> 16, nbk - 16);
        bp.flush();
    }
    bo.fill += hb;
}

// The end-of-block code (D/comp/Lz77Huffman.java:285).
__device__ __forceinline__ void put_eob(Lds& S, BitOut& bo) {
    const uint32_t eob = rfl(S.litCode[256]);
    make_room(bo, eob >> 16);
    if (opaque_lane() == 0) put_end_of_block(bo.obuf, bo.fill, eob);
    bo.fill += eob >> 16;
}

// finish(): pad to a byte (zero bits), then the container's trailer, the bit buffer's last bytes and
// the stream's result.  v_fill: the bit buffer's fill after the last block.
__device__ __forceinline__ void finish_stream(const Frame& f, const Stream& st, BitOut& bo, uint32_t v_fill) {
    bo.fill = to_s(v_fill);
    const uint64_t v_end_bits = to_v(to_s(bo.v_wbase) * 8 + bo.fill);
    const uint32_t fmt = to_s(st.v_fmt);
    const uint32_t sum = to_s(st.v_kind) == NDFL_SUM_CRC32 ? ~to_s(st.v_ck) : to_s(st.v_ck);
    const uint32_t tl = fmt == NDFL_FMT_ZLIB ? 4u : fmt == NDFL_FMT_GZIP ? 8u : 0u;
    make_room(bo, 7 + 64);
    bo.fill = (bo.fill + 7) & ~7u;
    const int lane = opaque_lane();
    if (lane == 0 && tl) {
        BitPut bp; bp.init(bo.obuf, bo.fill);
        if (fmt == NDFL_FMT_ZLIB) {                               // big-endian Adler-32
            for (int k = 3; k >= 0; k--) bp.put((sum >> (8 * k)) & 0xFFu, 8);
        } else {                                                  // CRC-32, ISIZE: little-endian
            const uint32_t isz = (uint32_t)st.v_len;
            for (int k = 0; k < 4; k++) bp.put((sum >> (8 * k)) & 0xFFu, 8);
            for (int k = 0; k < 4; k++) bp.put((isz >> (8 * k)) & 0xFFu, 8);
        }
        bp.flush();
    }
    bo.fill += 8 * tl;
    __syncthreads();
    store_bytes(bo, bo.fill >> 3);
    if (lane == 0) {
        ndfl_deflate_result rr;
        rr.out_len = bo.v_wbase + (bo.fill >> 3);
        rr.status = rr.out_len > bo.v_cap ? NDFL_E_CAPACITY : 0;
        rr.checksum = sum;
        rr.end_bits = v_end_bits;
        ((ndfl_deflate_result*)(uintptr_t)f.v_results)[st.v_si] = rr;
    }
}

}  // namespace dbat

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_batch_kernel(dbat::Args a) {
    using namespace dbat;
    __shared__ __attribute__((aligned(16))) Lds S;
    const Frame f = park_frame(a);
    const uint64_t v_tab = to_v((uint64_t)(uintptr_t)a.crc_tab);
    const uint32_t v_rle = to_v((uint32_t)(a.rle != 0)), v_dyn = to_v((uint32_t)(a.dynamic != 0));
    const uint32_t v_hist = to_v((uint32_t)(a.hist_enabled != 0));
    for (;;) {
        Stream st;
        if (!claim_stream(S, f, st)) break;
        BitOut bo = begin_stream(S, f, st);
        // the running state: parked across the code construction
        uint32_t v_prevb = to_v(0u), v_fill = to_v(0u);
        uint64_t v_cs = to_v((uint64_t)0);
        for (;;) {
            Codes cd{S.litCode, 0u, 0u, 0u, 0u};
            if (to_s(v_dyn)) {
                begin_block_hist(S);
                __syncthreads();
                const uint64_t cs = to_s(v_cs);
                const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs);
                {
                    // chunk 0 has no history; a later chunk has the stream's previous byte when hist_limit > 0
                    const bool zl = to_s(v_rle) && cs > 0 && to_s(v_hist);
                    uint32_t nock = 0;
                    walk_chunk<false>(to_s(v_rle) != 0, v_tab, S, bo, cd, (const uint8_t*)(uintptr_t)(to_s(st.v_src) + cs),
                                      len_c, to_s(v_prevb), zl, NDFL_SUM_NONE, nock);
                }
                end_block_hist(S, len_c);
            }
            __syncthreads();
            uint32_t hb;
            {
                const uint64_t len = to_s(st.v_len), cs = to_s(v_cs);
                const bool is_final = len - cs <= (uint64_t)to_s(f.v_chunk_len);
                hb = build_block_codes<64, true>(S.scr, to_s(v_dyn) != 0, is_final, S.litCode, S.distCode);
            }
            {
                const uint32_t c285 = rfl(S.litCode[285]), d0 = rfl(S.distCode[0]);
                cd.d0c = d0 & 0xFFFF; cd.d0l = d0 >> 16;
                cd.m258 = (c285 & 0xFFFF) | (cd.d0c << (c285 >> 16));
                cd.m258l = (c285 >> 16) + cd.d0l;
            }
            bo.fill = to_s(v_fill);
            put_header(S, bo, hb);
            {
                const uint64_t cs = to_s(v_cs);
                const uint32_t len_c = (uint32_t)min((uint64_t)to_s(f.v_chunk_len), to_s(st.v_len) - cs);
                const bool zl = to_s(v_rle) && cs > 0 && to_s(v_hist);
                uint32_t ck = to_s(st.v_ck);
                v_prevb = to_v(walk_chunk<true>(to_s(v_rle) != 0, v_tab, S, bo, cd,
                                                (const uint8_t*)(uintptr_t)(to_s(st.v_src) + cs), len_c, to_s(v_prevb), zl,
                                                to_s(st.v_kind), ck));
                st.v_ck = to_v(ck);
                v_cs = to_v(cs + len_c);
            }
            put_eob(S, bo);
            v_fill = to_v(bo.fill);
            if (to_s(v_cs) >= to_s(st.v_len)) break;
        }
        finish_stream(f, st, bo, v_fill);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// batch_run's launcher for ndfl_deflate_batch_kernel.
struct BatchRleLaunch {
    const Knobs& knobs;
    dbat::Args a;                         // n, chunk_len, the preset and the tables; deflate_batch_run sets `in`
    uint32_t grid = 0;
    int prepare() {                       // (before the launch is timed)
        grid = batch_grid<ndfl_deflate_batch_kernel>(a.n, knobs, "deflate batch");
        return 0;
    }
    int operator()(hipStream_t s, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                   uint32_t* d_ticket) {
        a.out = d_out; a.items = d_items; a.results = d_res; a.ticket = d_ticket;
        hipLaunchKernelGGL(ndfl_deflate_batch_kernel, dim3(grid), dim3(64), 0, s, a);
        return 0;
    }
};

// Host input of a deflate batch: the span of `in` the items cover, staged in d_in.  *d_src = the
// kernel's `in` (item offsets are relative to it).
static int stage_span(DevBuf& d_in, hipStream_t s, const uint8_t* in, const ndfl_member_item* items,
                      uint32_t n, uint32_t flags, const uint8_t** d_src) {
    *d_src = in;
    if (flags & NDFL_IN_DEVICE) return 0;
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!items[i].in_len) continue;
        lo = std::min(lo, items[i].in_off);
        hi = std::max(hi, items[i].in_off + items[i].in_len);
    }
    if (hi > lo) {
        INF_CHK(d_in.ensure(hi - lo));
        INF_CHK(hipMemcpyAsync(d_in.p, in + lo, hi - lo, hipMemcpyHostToDevice, s));
    }
    *d_src = d_in.as<const uint8_t>() - (hi > lo ? lo : 0);
    return 0;
}

// ndfl_deflate_batch and ndfl_deflate_batch_lz77 on stream s (arguments already validated).  `launch`: a
// BatchRleLaunch, or deflate_batch_lz.hip's BatchLzLaunch.
template <class Launch>
static int deflate_batch_run(BatchScratch& B, DevBuf& d_in, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                             const uint8_t* in, uint8_t* out, const ndfl_member_item* items,
                             ndfl_deflate_result* results, uint32_t n, uint32_t flags, Launch launch, double* last_ms) {
    INF_RC(stage_span(d_in, s, in, items, n, flags, &launch.a.in));
    INF_RC(launch.prepare());
    return batch_run(B, s, e0, e1, out, items, results, n, flags, last_ms, launch);
}

