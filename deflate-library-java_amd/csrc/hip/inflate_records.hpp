// inflate_records.hpp -- what the count pass hands to the emit passes, defined once.
//
// Two kinds of record live in the SegPool:
//   * round records (start / cnt per lane, one SegMeta): each lane's exact segment of a round, so
//     the emit passes decode each segment once instead of re-running the speculation.  They are
//     linked per chain in decode order (chain slot -> head record -> next ...);
//   * table records (TabRec), one per Huffman block: the block's decode tables and header fields,
//     so the emit passes load them instead of parsing the header and building the tables again.
// The producers (the wave and workgroup count kernels, the flat groups) and the consumers (the two
// emit kernels, the flat groups' full-table tokens) go through the structs and helpers below.  The
// emit passes check each replayed segment (NDFL_E_INTERNAL on a mismatch), so a producer and a
// consumer that disagree about a layout or about the round geometry break decoding of valid
// streams: the layouts are asserted here, and the geometry has one definition (seg_pw, seg_start,
// seg_end).  The count kernels sit at the edge of their register budget (they spill, and
// tests/test_kernel_resources.py pins how much): a few of their sites fill the structs by hand, by
// field name, where the helper's form cost a spilled register more; they say so.  For the same
// reason the readers' helpers take the held record as values, not as a cursor struct.
// Also here: the word indices of the two small device buffers the host shares with the kernels.
#pragma once

// ---- shared device words ------------------------------------------------------------------------
// InflateScratch::d_stats, as u32 words (512 bytes, zeroed per decode)
enum : uint32_t {
    SW_NSLOW = 0, SW_NFIX = 1, SW_NROUND = 2,   // count pass: slow-verify lanes, fix-up sweeps, rounds (NDFL_STATS)
    SW_QCOUNT = 8,                              // the finder's quick-stage survivors
    SW_STRICT_TICKET = 10,                      // the strict stage's slice ticket
    SW_REC_CTR = 12, SW_TREC_CTR = 13,          // round / table records handed out (SegPool::ctr, bctr)
    SW_TAIL_FAIL = 14,                          // ndfl_inflate_tail: a reference chain too long
    SW_STRICT64 = 16,                           // u64[4]: the strict stage's counters (NDFL_STATS)
    SW_CLOCK64 = 32,                            // u64[]: the count and emit passes' wave clocks (NDFL_STATS)
};
// InflateScratch::d_cticket, as u32 words (CTK_BYTES)
enum : uint32_t {
    CT_TICKET = 0,                              // the count pass's chain ticket
    CT_NFLAT = 4,                               // chains listed for the flat groups
    CT_FLAT_REDO = 5,                           // flat chains sent back to the wave decode (NDFL_STATS)
    CT_FLAT_TIME64 = 6,                         // u64: the flat groups' wave time (NDFL_STATS)
    CT_NORD = 8,                                // chains in the count order
    CT_FLAT_WHY = 10,                           // [6]: flat chains sent back, by cause (NDFL_STATS)
    CT_ORDER = 16,                              // the count order's buckets, then the emit order's, then
};                                              // the first erring chain (OB_WORDS each; see CTK_BYTES)

namespace wv {

// ---- decode tables --------------------------------------------------------------------------------
constexpr uint32_t LB = 10;                 // literal/length primary bits
constexpr uint32_t DB = 8;                  // distance primary bits
// Codes longer than the primary: a second-level table per primary prefix when they fit in the
// extension area (the primary entry then points at it: length 0, [8:5] index bits, [31:16] offset),
// otherwise the canonical slow path, whose arrays take the extension area instead (primary entry 0).
constexpr uint32_t LX = 320;                // literal/length extension words
constexpr uint32_t DX = 64;                 // distance extension words
struct Tabs {
    uint32_t lit[1u << LB];
    uint32_t dst[1u << DB];
    // sub-tables, or (fallback) the entry of every symbol in canonical order [0, n), the
    // left-justified 15-bit upper limit of each length [n, n + 16), first code and rank offset per
    // length (u16) [n + 16, n + 32)
    uint32_t lx[LX];
    uint32_t dx[DX];
};
// The same tables by pointer (the fast emit pass keeps the primary tables in LDS and reads the
// extension areas -- needed only for codes longer than the primary -- from the table record).
struct TabsG {
    const uint32_t* lit;
    const uint32_t* dst;
    const uint32_t* lx;
    const uint32_t* dx;
};

// how a lane's segment ended (SegMeta::kind_ft)
enum : uint32_t { T_EXIT = 0, T_EOB = 1, T_ERR = 2 };

// ---- round geometry -------------------------------------------------------------------------------
// A round of `span` bits is decoded by nl lanes over consecutive segments of pw words each.  Words
// per lane segment at least: a short round (a small block, a block's last round) is split over
// fewer lanes rather than into segments too short for a speculative decode to meet its true token
// boundaries before the segment ends (every such lane otherwise costs a fix-up decode).
#ifndef NDFL_PW_MIN
#define NDFL_PW_MIN 4
#endif
__host__ __device__ constexpr uint32_t seg_pw(uint32_t span, uint32_t nl = 64) {
    const uint32_t pw = ((span + nl - 1) / nl + 31) / 32;
    return pw < (uint32_t)NDFL_PW_MIN ? (uint32_t)NDFL_PW_MIN : pw;
}
// lane j's nominal segment [seg_start, seg_end) of the round [r0, re) (bits relative to the round's
// word-aligned base; per = 32 pw); the last lane ends at the round end
__host__ __device__ constexpr uint32_t seg_start(uint32_t r0, uint32_t per, uint32_t re, uint32_t j) {
    return r0 + j * per < re ? r0 + j * per : re;
}
__host__ __device__ constexpr uint32_t seg_end(uint32_t r0, uint32_t per, uint32_t re, uint32_t j, uint32_t last = 63) {
    return j == last ? re : seg_start(r0, per, re, j + 1);
}

}  // namespace wv

// ---- the pool -------------------------------------------------------------------------------------
constexpr uint32_t NOREC = 0xFFFFFFFFu;
struct SegMeta {
    uint32_t ft, kind_ft, reason_ft, next;   // first lane that ended the block (64: none), how; next record
    uint64_t end_ft, exit63;                 // that lane's end bit; lane 63's exit (the next round's start)
    uint32_t pw, brec;    // the round's words per lane segment; a block's first round: its table record
    uint64_t rs;          // staging origin: the record's lane 0 segment start (absolute bit)
};
static_assert(sizeof(SegMeta) == 48 && offsetof(SegMeta, next) == 12 && offsetof(SegMeta, end_ft) == 16 &&
              offsetof(SegMeta, exit63) == 24 && offsetof(SegMeta, pw) == 32 && offsetof(SegMeta, brec) == 36 &&
              offsetof(SegMeta, rs) == 40, "SegMeta layout (write_round_meta stores it by offset)");
// A round record's meta, stored by one lane from the values at hand as 16 + 16 + 8 + 8 bytes (in the
// flat group a SegMeta built in registers was partly spilled, and its reload waited for the input
// rings' loads in flight).
__device__ __forceinline__ void write_round_meta(SegMeta* m, uint32_t ft, uint32_t kind_ft, uint32_t reason_ft, uint32_t next,
                                                 uint64_t end_ft, uint64_t exit63, uint32_t pw, uint32_t brec, uint64_t rs) {
    uint4* mq = (uint4*)m;
    mq[0] = make_uint4(ft, kind_ft, reason_ft, next);
    mq[1] = make_uint4((uint32_t)end_ft, (uint32_t)(end_ft >> 32), (uint32_t)exit63, (uint32_t)(exit63 >> 32));
    *(uint2*)(mq + 2) = make_uint2(pw, brec);
    *(uint64_t*)((uint2*)(mq + 2) + 1) = rs;
}

struct TabRec {
    wv::Tabs t;
    uint64_t hdr_bit, data_bit;              // the block's header and first data bit
    uint32_t bfinal, btype, ed;              // ed: the distance code is empty
    uint32_t phase;                          // TP_NONE, TP_LIT8, or a block's escape prefix mask (> 1)
    uint32_t pad[8];                         // (a record is a whole number of 64-byte lines)
};
static_assert(sizeof(TabRec) == 6720 && offsetof(TabRec, hdr_bit) == sizeof(wv::Tabs) && sizeof(wv::Tabs) % 16 == 0,
              "TabRec layout");
constexpr uint32_t BT_BYTES = sizeof(TabRec);
// TabRec::phase: 0 nothing special; 1 literal codes mostly of 8 bits (the decoders try four literals a
// step); above 1 an escape-prefix literal block, the value being its prefix mask repeated in the 4
// bytes (flat8_mask; the decoders scan to the next escape byte)
constexpr uint32_t TP_NONE = 0, TP_LIT8 = 1;
__device__ __forceinline__ uint32_t tab_phase(bool phased, uint32_t esc4) { return phased ? (esc4 ? esc4 : TP_LIT8) : TP_NONE; }

struct SegPool {
    uint64_t* start;      // [nrec][64]
    uint32_t* cnt;        // [nrec][64]
    SegMeta* meta;        // [nrec]
    uint32_t* head;       // [nslot] first record of the chain counted at that slot (NOREC: none)
    uint32_t* ctr;        // records handed out
    uint32_t nrec;
    uint64_t nslot;
    TabRec* bt;           // [nbt]; a block's first round record names its table record (SegMeta::brec)
    uint32_t* bctr;       // table records handed out
    uint32_t nbt;
};

// ---- claiming records -----------------------------------------------------------------------------
// Records are claimed in batches (one contended atomic per batch instead of one per record; unused
// slots of a batch stay unused).  An index at or past the pool's size means the pool is used up.
#ifndef NDFL_REC_BATCH
#define NDFL_REC_BATCH 16       // round records claimed per atomic (the pool keeps 65,536 spare)
#endif
#ifndef NDFL_TREC_BATCH
#define NDFL_TREC_BATCH 4       // table records claimed per atomic
#endif
// a wave's batch [next, end) (wave-uniform): lane 0 claims, every lane gets the index
__device__ __forceinline__ uint32_t claim_wave(uint32_t* ctr, uint32_t& next, uint32_t& end, uint32_t batch, int lane) {
    if (next >= end) {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(ctr, batch);
        b = __builtin_amdgcn_readfirstlane(b);
        next = b; end = b + batch;
    }
    return next++;
}
// a table record for a wave (NOREC: the pool is used up)
__device__ __forceinline__ uint32_t claim_table_record(const SegPool& pool, uint32_t& tb_next, uint32_t& tb_end, int lane) {
    const uint32_t b = claim_wave(pool.bctr, tb_next, tb_end, NDFL_TREC_BATCH, lane);
    return b < pool.nbt ? b : NOREC;
}

// ---- table records --------------------------------------------------------------------------------
// The block's tables `t` (LDS) and header fields into record brec, by nthreads threads (tid 0 writes
// the fields).
__device__ __forceinline__ void write_table_record(const SegPool& pool, uint32_t brec, const wv::Tabs& t, uint64_t hdr_bit,
                                                   uint64_t data_bit, uint32_t bfinal, uint32_t btype, bool ed,
                                                   uint32_t phase, uint32_t tid, uint32_t nthreads) {
    TabRec* r = pool.bt + brec;
    uint4* dst = (uint4*)&r->t;
    const uint4* src = (const uint4*)&t;
    for (uint32_t q = tid; q < sizeof(wv::Tabs) / 16; q += nthreads) dst[q] = src[q];
    if (tid == 0) {
        r->hdr_bit = hdr_bit; r->data_bit = data_bit;
        r->bfinal = bfinal; r->btype = btype; r->ed = ed ? 1u : 0u; r->phase = phase;
    }
}
__device__ __forceinline__ const TabRec* tabrec(const SegPool& pool, uint32_t idx) { return pool.bt + idx; }
__device__ __forceinline__ wv::TabsG tabs_view(const TabRec* r) { return wv::TabsG{r->t.lit, r->t.dst, r->t.lx, r->t.dx}; }

// ---- round records --------------------------------------------------------------------------------
// record idx into its chain's list: after record prev, or as the head of chain slot `slot`
__device__ __forceinline__ void link_round(const SegPool& pool, uint64_t slot, uint32_t prev, uint32_t idx) {
    if (prev == NOREC) pool.head[slot] = idx;
    else pool.meta[prev].next = idx;
}

// A chain's round records are read in order, each loaded one round ahead (its loads overlap the
// decode of the round before): rec is the record held in pm / pst / pcn (NOREC: none left).
__device__ __forceinline__ void rec_fetch(const SegPool& pool, uint32_t rec, int lane, SegMeta& pm, uint64_t& pst, uint32_t& pcn) {
    if (rec != NOREC) { pm = pool.meta[rec]; pst = pool.start[(uint64_t)rec * 64 + lane]; pcn = pool.cnt[(uint64_t)rec * 64 + lane]; }
}
// the table record of the block at bit `cur`, when the held record names it (else nullptr)
__device__ __forceinline__ const TabRec* block_tables(const SegPool& pool, uint32_t rec, const SegMeta& pm, uint64_t cur) {
    const TabRec* r = (rec != NOREC && pm.brec < pool.nbt) ? tabrec(pool, pm.brec) : nullptr;
    return (r && r->hdr_bit == cur) ? r : nullptr;
}
// This lane's segment of the round recorded in m (its start given): it ends where the next lane's
// starts, lane 63's at the recorded exit, lane ft's at the block's end, with that lane's kind and Reason.
__device__ __forceinline__ void round_lane_end(const SegMeta& m, uint64_t start, int lane, uint64_t& end, uint32_t& kind,
                                               uint32_t& reason) {
    const uint64_t nx = __shfl_down((unsigned long long)start, 1, 64);
    end = lane < 63 ? nx : m.exit63;
    kind = wv::T_EXIT; reason = 0;
    if ((uint32_t)lane == m.ft) { end = m.end_ft; kind = m.kind_ft; reason = m.reason_ft; }
}
