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
//
// ndfl_inflate_members_kernel (ndfl_inflate_members) is the same stream loop -- one text,
// inflate_batch_loop.inc, included in both kernels -- for zlib members, gzip members and raw streams
// with a checksum: lane 0 parses the container header before the DEFLATE data and the trailer after
// it, and flush_to, where every output byte passes once and in order, folds what it flushes into the
// stream's CRC-32 or Adler-32 (fold_span).  The same constraints hold for it.
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
    static constexpr bool members = false;
};
// The same with the checksum state of ndfl_inflate_members_kernel: the ring helpers below are
// templates over the two, and flush_to folds what it flushes into an OutM's checksum.
struct OutM : Out {
    uint32_t sum;          // NDFL_SUM_* of the stream's checksum
    uint32_t ck;           // its running value: the raw CRC register, or Adler's (b << 16) | a; wave-uniform,
                           //   but kept in a vector register throughout
    const uint32_t* crc_x; // the context's x^(8k) table (crc_x[k], k < 64) and x^(8 * 64k) (crc_x[64 + k])
    static constexpr bool members = true;
};

__device__ __forceinline__ uint32_t to_v(uint32_t x);

// The checksum code keeps its wave-uniform values in VECTOR registers (every lane computes the same
// value): it runs inside the token loop, whose scalar registers are all taken.
//
// a*b mod P as crc_multmodp, without its data-dependent exit: 32 steps on vector registers.
__device__ __forceinline__ uint32_t crc_mul_v(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma nounroll
    for (int k = 0; k < 32; k++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (NDFL_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8n) mod P for n < 65536 from the context's table: one product instead of crc_x8n's ~30.
__device__ __forceinline__ uint32_t x8n_tab(const uint32_t* crc_x, uint32_t n) {
    return crc_mul_v(crc_x[n & 63], crc_x[64 + (n >> 6)]);
}

// One byte into a raw CRC register (no table: the tables stay out of LDS, and a lookup in global
// memory would put a load's latency on every byte).
__device__ __forceinline__ uint32_t crc_byte(uint32_t c, uint32_t b) {
    c ^= b;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (NDFL_CRC_POLY & (0u - (c & 1u)));
    return c;
}

// Fold the L (<= RING) ring bytes from output address a on into the stream's checksum.  The span is
// cut into 64 pieces of p bytes that END at the span's end, lane k taking the k-th: the first lanes'
// pieces begin before the span, where they read zeros -- which change neither a raw CRC that starts
// at 0 nor a sum -- so every piece has the same length and lane k is followed by (63 - k) * p bytes.
// p is odd, so the lanes' byte reads spread over the LDS banks.
//   Adler-32: each lane's (s1, s2) of its piece, s2 relative to the piece's own start; the wave adds
//   s1 * (bytes after the piece) to s2 and sums.  p <= 513, so s1 <= 130,815 and s2 <= 255 * 513 *
//   514 / 2 < 2^26 (a 32 KiB span of 0xFF); both are reduced mod 65521 before the products, which
//   then stay below 65,520 * 32,768 < 2^31, and the sums of 64 of them below 2^32.
//   CRC-32: each lane's raw CRC of its piece; six rounds of c = c * x^(8 * p * 2^j) ^ (the lane 2^j
//   further on) leave the span's raw CRC in lane 0; then run = run * x^(8L) ^ span.
__device__ __forceinline__ void fold_span(OutM& q, uint64_t a, uint32_t L, int lane) {
    const uint32_t sum = (uint32_t)__builtin_amdgcn_readfirstlane(q.sum);    // (parked in a vector register)
    if (sum == NDFL_SUM_NONE) return;
    const uint32_t p = ((L + 63) >> 6) | 1u;                                 // (scalar: the loop bound)
    const uint32_t Lv = to_v(L), pv = to_v(p);
    uint32_t at = to_v((uint32_t)a) + Lv - (64u - (uint32_t)lane) * pv;      // this lane's next byte ...
    int32_t idx = (int32_t)(Lv - (64u - (uint32_t)lane) * pv);               // ... and its index in the span
    if (sum == NDFL_SUM_ADLER32) {
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t j = 0; j < p; j++, idx++, at++) {
            s1 += idx >= 0 ? (uint32_t)q.ring[at & RMASK] : 0u;
            s2 += s1;
        }
        s1 %= 65521u;
        const uint32_t t = s2 % 65521u + (s1 * ((63u - (uint32_t)lane) * pv)) % 65521u;
        const uint32_t S1 = wave_sum(s1), T = wave_sum(t);
        const uint32_t A = q.ck & 0xFFFFu, B = q.ck >> 16;
        const uint32_t nb = (B + (Lv * A) % 65521u + T) % 65521u, na = (A + S1) % 65521u;
        q.ck = nb << 16 | na;
    } else {
        uint32_t c = 0;
        for (uint32_t j = 0; j < p; j++, idx++, at++) c = crc_byte(c, idx >= 0 ? (uint32_t)q.ring[at & RMASK] : 0u);
        uint32_t X = x8n_tab(q.crc_x, pv);
#pragma nounroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t next = __shfl_down(c, o, 64);
            c = crc_mul_v(X, c) ^ next;
            X = crc_mul_v(X, X);
        }
        const uint32_t span = (uint32_t)__builtin_amdgcn_readfirstlane(c);
        q.ck = crc_mul_v(x8n_tab(q.crc_x, Lv), q.ck) ^ span;
    }
}

// Store ring bytes [fl, fend) that lie inside the region; the ring keeps them.  Every output byte
// of a stream passes here exactly once and in order, so the members kernel (an OutM) folds the span
// into the stream's checksum here -- before the clamp to the region: bytes past out_cap count.
template <class O>
__device__ __forceinline__ void flush_to(O& q, uint64_t fend, int lane) {
    if (fend <= q.fl) return;
    wsync();                                   // the ring writes of other lanes
    uint64_t a = q.fl;
    if constexpr (O::members) fold_span(q, a, (uint32_t)(fend - a), lane);
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
template <class O>
__device__ __forceinline__ void make_room(O& q, uint32_t n, int lane) {
    if (q.o + n - q.fl > RING) flush_to(q, q.o & ~15ull, lane);
}
template <class O>
__device__ __forceinline__ void flush_pending(O& q, uint32_t pend, int lane) {
    if (!q.npend) return;
    make_room(q, q.npend, lane);
    if ((uint32_t)lane < q.npend) q.ring[(q.o + lane) & RMASK] = (uint8_t)pend;
    q.o += q.npend;
    q.npend = 0;
    wsync();
}
template <class O>
__device__ __forceinline__ void add_literal(O& q, uint32_t& pend, uint32_t b, int lane) {
    pend = (uint32_t)lane == q.npend ? b : pend;
    if (++q.npend == 64) flush_pending(q, pend, lane);
}
// A copy of n (3..258) bytes from dist (1..32768) back, the pending literals already in the ring.
// dist >= 64 or dist >= n: 64 bytes a step straight from the ring (a step's sources were written by
// earlier steps; with dist near 32768 a step's sources share slots only with its own or later
// destinations, and each step reads before it writes).  Otherwise the source is a period of dist
// bytes: byte k comes from byte k mod dist of the last dist bytes, which no step overwrites.
template <class O>
__device__ __forceinline__ void copy_run(O& q, uint32_t n, uint32_t dist, int lane) {
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

// ---- container members (ndfl_inflate_members_kernel) ------------------------------------------------
// Lane 0 parses a member's header and trailer through the bounds-checked In view of the WHOLE item
// (stream_in of in_off, in_len): byte i of the item, to be read only after i < in_len has been
// checked, so no byte of the neighbour is acted on and In::ld never returns a word past the item's
// last one.  Statuses are the public codes (the containers' Reasons, 13..19, lie outside the
// decoder's internal ones), NDFL_E_ARG, or 0.
__device__ __forceinline__ uint32_t item_byte(const In& all, uint64_t mis, uint64_t i) {
    const uint64_t b = mis + i;
    return (all.ld(b >> 2) >> (8 * (uint32_t)(b & 3))) & 0xFFu;
}

// ZlibMetadata.read (D/ZlibMetadata.java:47-80), its checks in its order; hl = the header's length.
__device__ __forceinline__ int32_t parse_zlib_header(const In& all, uint64_t mis, uint64_t len, uint64_t& hl) {
    if (len < 2) return NDFL_UNEXPECTED_END_OF_STREAM;
    const uint32_t cmf = item_byte(all, mis, 0), flg = item_byte(all, mis, 1);
    if (((cmf << 8) | flg) % 31u != 0) return NDFL_HEADER_CHECKSUM_MISMATCH;
    const uint32_t cm = cmf & 15u;
    if (cm != 8 && cm != 15) return NDFL_UNSUPPORTED_COMPRESSION_METHOD;
    uint64_t i = 2;
    if (flg & 0x20u) {                          // FDICT: the 4-byte dictionary id is skipped
        if (len < 6) return NDFL_UNEXPECTED_END_OF_STREAM;
        i = 6;
    }
    if (cm == 8 && (cmf >> 4) > 7) return NDFL_E_ARG;     // the record constructor's IllegalArgumentException
    hl = i;
    return 0;
}

// GzipMetadata.read (D/GzipMetadata.java:73-146), its checks in its order.  The header CRC (FHCRC:
// the low 16 bits of the CRC-32 of every header byte before it) is taken bytewise as the bytes pass.
__device__ __forceinline__ int32_t parse_gzip_header(const In& all, uint64_t mis, uint64_t len, uint64_t& hl) {
    if (len < 2) return NDFL_UNEXPECTED_END_OF_STREAM;
    if (item_byte(all, mis, 0) != 0x1Fu || item_byte(all, mis, 1) != 0x8Bu) return NDFL_GZIP_INVALID_MAGIC_NUMBER;
    if (len < 3) return NDFL_UNEXPECTED_END_OF_STREAM;
    if (item_byte(all, mis, 2) != 8u) return NDFL_UNSUPPORTED_COMPRESSION_METHOD;
    if (len < 4) return NDFL_UNEXPECTED_END_OF_STREAM;
    const uint32_t flg = item_byte(all, mis, 3);
    if (flg & 0xE0u) return NDFL_GZIP_RESERVED_FLAGS_SET;
    if (len < 10) return NDFL_UNEXPECTED_END_OF_STREAM;          // MTIME (4), XFL, OS
    const uint32_t os = item_byte(all, mis, 9);
    if (!(os < 14 || os == 255)) return NDFL_GZIP_UNSUPPORTED_OPERATING_SYSTEM;
    const bool hcrc = (flg & 2u) != 0;
    uint32_t hc = 0xFFFFFFFFu;
    uint64_t i = 0;
    // the next byte, i < len checked by the caller
    auto take = [&]() { const uint32_t b = item_byte(all, mis, i++); if (hcrc) hc = crc_byte(hc, b); return b; };
    if (hcrc) while (i < 10) take();
    i = 10;
    if (flg & 4u) {                             // FEXTRA
        if (len - i < 2) return NDFL_UNEXPECTED_END_OF_STREAM;
        uint64_t xl = take();
        xl |= (uint64_t)take() << 8;
        if (len - i < xl) return NDFL_UNEXPECTED_END_OF_STREAM;
        if (hcrc) for (uint64_t k = 0; k < xl; k++) take();
        else i += xl;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1)    // FNAME, FCOMMENT: each to its 0 byte
        if (flg & f)
            for (;;) {
                if (i >= len) return NDFL_UNEXPECTED_END_OF_STREAM;
                if (take() == 0) break;
            }
    if (hcrc) {
        if (len - i < 2) return NDFL_UNEXPECTED_END_OF_STREAM;
        const uint32_t expect = ~hc & 0xFFFFu;
        uint32_t actual = item_byte(all, mis, i);
        actual |= item_byte(all, mis, i + 1) << 8;
        i += 2;
        if (actual != expect) return NDFL_HEADER_CHECKSUM_MISMATCH;
    }
    hl = i;
    return 0;
}

// The trailer at byte t of the item, after a decode without a Reason: zlib's big-endian Adler-32
// (D/ZlibInputStream.java:57-79), gzip's CRC-32 then ISIZE, the checksum tested first
// (D/GzipInputStream.java:76-87).  `sum` is the finished checksum of all `total` output bytes.
// Returns the Reason or 0; tl = the trailer's length.
__device__ __forceinline__ int32_t check_trailer(const In& all, uint64_t mis, uint64_t len, uint32_t fmt, uint64_t t,
                                                 uint32_t sum, uint64_t total, uint32_t& tl) {
    tl = fmt == NDFL_FMT_GZIP ? 8u : 4u;
    if (len - t < tl) return NDFL_UNEXPECTED_END_OF_STREAM;
    uint32_t v[2] = {0, 0};
    for (uint32_t k = 0; k < tl; k++) {
        const uint32_t b = item_byte(all, mis, t + k);
        if (fmt == NDFL_FMT_GZIP) v[k >> 2] |= b << (8 * (k & 3));
        else v[0] = v[0] << 8 | b;
    }
    if (v[0] != sum) return NDFL_DECOMPRESSED_CHECKSUM_MISMATCH;
    if (fmt == NDFL_FMT_GZIP && v[1] != (uint32_t)total) return NDFL_DECOMPRESSED_SIZE_MISMATCH;
    return 0;
}

template <bool M> struct Io { typedef ndfl_batch_item Item; typedef ndfl_batch_result Result; };
template <> struct Io<true> { typedef ndfl_member_item Item; typedef ndfl_member_result Result; };

}  // namespace bat

// The two kernels share one stream loop, inflate_batch_loop.inc (see there why it is included text).
extern "C" __global__ void __launch_bounds__(64)
ndfl_inflate_batch_kernel(const uint32_t* w, uint8_t* out, const ndfl_batch_item* items, ndfl_batch_result* results,
                          uint32_t n, uint32_t* ticket) {
#define NDFL_BATCH_MEMBERS 0
#include "inflate_batch_loop.inc"
#undef NDFL_BATCH_MEMBERS
}

// crc_x: the context's x^(8k) tables (d_tabs + 1024 words), read-only.
extern "C" __global__ void __launch_bounds__(64)
ndfl_inflate_members_kernel(const uint32_t* w, uint8_t* out, const ndfl_member_item* items, ndfl_member_result* results,
                            uint32_t n, uint32_t* ticket, const uint32_t* crc_x) {
#define NDFL_BATCH_MEMBERS 1
#include "inflate_batch_loop.inc"
#undef NDFL_BATCH_MEMBERS
}

// ---- host side ------------------------------------------------------------------------------------
struct BatchScratch {
    DevBuf d_items;                                    // the items, then the results, then the ticket
    DevBuf d_out;                                      // host-output staging
    void release() { d_items.release(); d_out.release(); }
};

// The grid of a batch kernel (one-wave workgroups that claim streams from a ticket): what fits on the
// chip at once, no more waves than streams, at most NDFL_BATCH_WAVES and, where every wave needs
// per_wave bytes of device memory of its own, no more than `budget` bytes of it in all.  `label` names
// the call in the NDFL_STATS line.
template <auto Kernel>
static uint32_t batch_grid(uint32_t n, const Knobs& knobs, const char* label, size_t per_wave = 0, size_t budget = 0) {
    static const uint32_t auto_grid = occupancy_grid(Kernel, 64, 256 * 16);
    uint32_t grid = std::min(n, auto_grid);
    if (knobs.batch_waves) grid = std::min(grid, knobs.batch_waves);
    if (per_wave) grid = (uint32_t)std::max<size_t>(1, std::min<size_t>(grid, budget / per_wave));
    if (knobs.stats) {
        fprintf(stderr, "[ndfl] %s: %u streams, %u waves (of %u)", label, n, grid, auto_grid);
        if (per_wave) fprintf(stderr, ", %zu scratch bytes per wave", per_wave);
        fputc('\n', stderr);
    }
    return grid;
}

// One batch call on stream s (arguments already validated, input already staged): one launch, one host
// sync.  The items, the results and the zeroed ticket share B.d_items.  Host output goes through the
// device staging buffer B.d_out, which spans the items' regions, and only each stream's stored bytes
// are copied into `out`.  launch(s, d_out, d_items, d_results, d_ticket) starts the kernel (d_out: the
// kernel's `out`, item offsets are relative to it) and returns 0 or an error code; the time between the
// two events around it becomes *last_ms, so the caller sizes the grid and whatever the kernel needs
// allocated before it comes here.  results[i] comes back as the kernel wrote it.
template <class Item, class Result, class Launch>
static int batch_run(BatchScratch& B, hipStream_t s, hipEvent_t e0, hipEvent_t e1, uint8_t* out, const Item* items,
                     Result* results, uint32_t n, uint32_t flags, double* last_ms, Launch&& launch) {
    const size_t items_b = (size_t)n * sizeof(Item), res_b = (size_t)n * sizeof(Result);
    INF_CHK(B.d_items.ensure(items_b + res_b + 16));
    Result* d_res = (Result*)(B.d_items.as<char>() + items_b);
    uint32_t* d_ticket = (uint32_t*)((char*)d_res + res_b);
    INF_CHK(hipMemcpyAsync(B.d_items.p, items, items_b, hipMemcpyHostToDevice, s));
    INF_CHK(hipMemsetAsync(d_ticket, 0, 16, s));
    uint64_t lo = ~0ull, hi = 0;                 // the span of `out` the regions cover
    for (uint32_t i = 0; i < n; i++) {
        if (!items[i].out_cap) continue;
        lo = std::min(lo, items[i].out_off);
        hi = std::max(hi, items[i].out_off + items[i].out_cap);
    }
    const bool out_dev = (flags & NDFL_OUT_DEVICE) != 0;
    uint8_t* d_out = out;
    std::vector<uint8_t> h_span;
    if (!out_dev) {
        if (hi > lo) INF_CHK(B.d_out.ensure(hi - lo));
        d_out = B.d_out.as<uint8_t>() - (hi > lo ? lo : 0);
    }
    INF_CHK(hipEventRecord(e0, s));
    INF_RC(launch(s, d_out, B.d_items.as<const Item>(), d_res, d_ticket));
    INF_CHK(hipGetLastError());
    INF_CHK(hipEventRecord(e1, s));
    INF_CHK(hipMemcpyAsync(results, d_res, res_b, hipMemcpyDeviceToHost, s));
    if (!out_dev && hi > lo) {
        h_span.resize(hi - lo);
        INF_CHK(hipMemcpyAsync(h_span.data(), B.d_out.p, hi - lo, hipMemcpyDeviceToHost, s));
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

// ndfl_inflate_batch (M = false) and ndfl_inflate_members (M = true: its items, results and kernel; crc_x =
// the context's x^(8k) tables).  results[i].status holds the internal Reason codes; the C ABI maps them.
template <bool M>
static int inflate_batch_run(InflateScratch& S, BatchScratch& B, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                             const uint8_t* in, uint64_t in_size, uint8_t* out, const typename bat::Io<M>::Item* items,
                             typename bat::Io<M>::Result* results, uint32_t n, uint32_t flags, double* last_ms,
                             const uint32_t* crc_x = nullptr) {
    typedef typename bat::Io<M>::Item Item;
    typedef typename bat::Io<M>::Result Result;
    const uint32_t* d_w = nullptr;
    INF_RC(stage_input(S, s, in, in_size, flags, &d_w));
    const uint32_t grid = M ? batch_grid<ndfl_inflate_members_kernel>(n, S.knobs, "inflate members")
                            : batch_grid<ndfl_inflate_batch_kernel>(n, S.knobs, "inflate batch");
    return batch_run(B, s, e0, e1, out, items, results, n, flags, last_ms,
                     [&](hipStream_t q, uint8_t* d_out, const Item* d_items, Result* d_res, uint32_t* d_ticket) {
        if constexpr (M)
            hipLaunchKernelGGL(ndfl_inflate_members_kernel, dim3(grid), dim3(64), 0, q, d_w, d_out, d_items, d_res, n,
                               d_ticket, crc_x);
        else
            hipLaunchKernelGGL(ndfl_inflate_batch_kernel, dim3(grid), dim3(64), 0, q, d_w, d_out, d_items, d_res, n,
                               d_ticket);
        return 0;
    });
}

