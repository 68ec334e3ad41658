// deflate_bgzf.hip -- the blocked gzip (BGZF) writer's own passes (ndfl_deflate_bgzf, include/ndfl.h;
// host side: csrc/capi/ndfl_deflate_bgzf.cpp).
//
// Every block of block_len input bytes is one stream of one chunk of the segmented chunk encoders
// (seg_tables.hpp), so block k's slot is staged byte k * block_len -- the input as it lies -- and its
// DEFLATE data lies at k * slot of the staged output.  The passes around the encoders, each reading what an
// earlier LAUNCH wrote:
//   tables  the chunk and stream records and the items of all blocks, by arithmetic (a thread per block)
//   (the encoders, the edge fix-up, the CRC-32 partials and their combination: ndfl_deflate_batch_chunked's)
//   size    a thread per member: the tuple's bit count from the chunk's status word, the stored block's by
//           rule -- at bit 0 MultiStrategy(X, Uncompressed) takes the stored form iff 8 * len + 40 * nblk is
//           LESS than X's bits, nblk = max(1, ceil(len / 65535)) -- the member's length, the lowest index of
//           a member above 65,536 bytes; lengths and stored members summed per tile of SIZE_TILE
//   scan    ndfl_bgzf_sum_kernel (inflate_bgzf.hip): the tile sums into tile offsets, the file's length and
//           the number of stored members
//   offsets the tile's lengths scanned again, now from the tile's offset: the member table
//   pack    a workgroup per member: header with BSIZE, body, trailer to out + off[k] -- nothing when the
//           file does not fit out_cap or a member is too long, which it reads in the head block.  The last
//           workgroup writes the closing empty member.
// The launches do not depend on the number of members.
//
// All kernels: no calls, no arrays indexed at run time outside LDS, so no scratch memory (DESIGN.md §7
// item 9; tests/test_bgzf_write_kernel_resources.py).  Their names say bgzw, not bgzf: the decoder's
// resource test counts the kernels of its own file by that substring.
#pragma once

namespace bgzw {

constexpr uint32_t SIZE_TILE = 256;           // members per workgroup of the size and offsets passes
constexpr uint32_t PACK_THREADS = 1024;       // threads of a pack workgroup, a dword each per step
constexpr uint32_t MAX_MEMBER = 65536;        // BSIZE holds a member's length - 1 in 16 bits
constexpr uint32_t HEADER_LEN = 18;           // 10 fixed bytes, XLEN, the BC subfield
constexpr uint32_t EOF_LEN = 28;              // the closing empty member
constexpr uint32_t STORED_BLOCK = 65535;      // Uncompressed's MAX_BLOCK_LEN
constexpr uint32_t STORED = 0x80000000u;      // in mlen[k]: member k is written as a stored block
constexpr uint32_t NO_BAD = 0xFFFFFFFFu;      // Head::bad while no member is too long

// What the passes leave for the host (every byte 0xFF before the first launch).
struct Head {
    uint64_t total;           // the file's length
    uint32_t n_stored;
    uint32_t bad;             // the lowest index of a member longer than MAX_MEMBER, or NO_BAD
};

// Bytes of data block k (of nblk): block_len, or the input's tail.
__device__ __forceinline__ uint32_t block_bytes(uint32_t k, uint64_t in_len, uint32_t block_len) {
    return (uint32_t)min((uint64_t)block_len, in_len - (uint64_t)k * block_len);
}

}  // namespace bgzw

// The closing member; bytes 0..15 are every member's header up to BSIZE.
__device__ __constant__ uint8_t ndfl_bgzw_eof[bgzw::EOF_LEN] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                                                0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// Block k's chunk record, stream record and item (the CRC-32 combination reads the item's in_len).
extern "C" __global__ void __launch_bounds__(bgzw::SIZE_TILE)
ndfl_bgzw_tables_kernel(uint64_t in_len, uint32_t block_len, uint32_t nblk, uint64_t slot, SegChunk* chunks,
                        SegStream* streams, ndfl_member_item* items) {
    using namespace bgzw;
    const uint32_t k = blockIdx.x * SIZE_TILE + threadIdx.x;
    if (k >= nblk) return;
    const uint64_t at = (uint64_t)k * block_len;
    const uint32_t len = block_bytes(k, in_len, block_len);
    SegChunk c;
    c.start = at; c.src = at; c.stream = k; c.len = len;
    c.flags = SEG_FIRST | SEG_LAST | (uint32_t)NDFL_SUM_CRC32 << SEG_SUM_SHIFT;
    c.pad = 0;
    chunks[k] = c;
    streams[k] = SegStream{(uint64_t)k * slot, k, 1u};
    ndfl_member_item it;
    it.in_off = at; it.in_len = len; it.out_off = 0; it.out_cap = 0;
    it.format = NDFL_FMT_GZIP; it.sum = NDFL_SUM_NONE;
    items[k] = it;
}

// Member k's length and form into mlen[k] (k = nblk: the closing member), tile t's lengths and stored
// members into tile_sum[t] and tile_cnt[t], the lowest index of a member that is too long into head->bad.
extern "C" __global__ void __launch_bounds__(bgzw::SIZE_TILE)
ndfl_bgzw_size_kernel(const uint64_t* status, uint64_t in_len, uint32_t block_len, uint32_t nblk, uint64_t slot,
                      uint32_t* mlen, uint32_t* tile_cnt, uint64_t* tile_sum, bgzw::Head* head) {
    using namespace bgzw;
    __shared__ uint32_t s_c[SIZE_TILE / 64];
    __shared__ uint64_t s_s[SIZE_TILE / 64];
    const uint32_t k = blockIdx.x * SIZE_TILE + threadIdx.x;
    uint32_t m = 0, stored = 0;
    if (k < nblk) {
        const uint32_t len = block_bytes(k, in_len, block_len);
        const uint64_t xbits = (status[k] & ST_VAL) - 8 * ((uint64_t)k * slot);
        const uint32_t nb = max(1u, (len + STORED_BLOCK - 1) / STORED_BLOCK);
        const uint64_t sbits = 8ull * len + 40ull * nb;
        stored = sbits < xbits ? 1u : 0u;                    // (a tie goes to the tuple, which is listed first)
        m = HEADER_LEN + (uint32_t)(stored ? sbits / 8 : (xbits + 7) / 8) + 8u;
        if (m > MAX_MEMBER) atomicMin(&head->bad, k);
        mlen[k] = m | (stored ? STORED : 0u);
    } else if (k == nblk) {
        m = EOF_LEN;
        mlen[k] = m;
    }
    uint32_t tc;
    uint64_t ts;
    bgzf::block_scan<SIZE_TILE>(stored, s_c, tc);
    bgzf::block_scan<SIZE_TILE>((uint64_t)m, s_s, ts);
    if (threadIdx.x == 0) { tile_cnt[blockIdx.x] = tc; tile_sum[blockIdx.x] = ts; }
}

// The member table from the lengths and the tiles' offsets (tile_sum, scanned): entry k = (member k's file
// offset, its first data byte), entry nblk + 1 = (the file's length, in_len).
extern "C" __global__ void __launch_bounds__(bgzw::SIZE_TILE)
ndfl_bgzw_offsets_kernel(const uint32_t* mlen, const uint64_t* tile_sum, const bgzw::Head* head, uint64_t in_len,
                         uint32_t block_len, uint32_t nblk, ndfl_bgzf_member* table) {
    using namespace bgzw;
    __shared__ uint64_t s_s[SIZE_TILE / 64];
    const uint32_t k = blockIdx.x * SIZE_TILE + threadIdx.x;
    const uint64_t m = k <= nblk ? (uint64_t)(mlen[k] & ~STORED) : 0ull;
    uint64_t ts;
    const uint64_t off = tile_sum[blockIdx.x] + bgzf::block_scan<SIZE_TILE>(m, s_s, ts);
    if (k < nblk) {
        table[k] = ndfl_bgzf_member{off, (uint64_t)k * block_len};
    } else if (k == nblk) {
        table[k] = ndfl_bgzf_member{off, in_len};
        table[k + 1] = ndfl_bgzf_member{head->total, in_len};
    }
}

// One workgroup per member, the closing one included: its bytes to out + table[k].in_off.  A member is
// [prefix | body | trailer]: the prefix is the header with BSIZE (and a stored block's five bytes, or all
// of the closing member), the body the staged DEFLATE bytes (at k * slot of `staged`, word-aligned) or the
// block's raw bytes (at k * block_len of `slots`, any alignment), the trailer CRC-32 and ISIZE.  Whole
// aligned words of `out` are stored as words, those inside the body from two source words
// (__builtin_amdgcn_alignbyte), the few across a seam byte by byte from LDS and the body; the bytes before
// the member's first aligned word and after its last whole one are byte stores, since the neighbours own
// the rest of those words.  Nothing is written when the file does not fit or some member is too long.
extern "C" __global__ void __launch_bounds__(bgzw::PACK_THREADS)
ndfl_bgzw_pack_kernel(const uint8_t* staged, const uint8_t* slots, const uint32_t* mlen, const ndfl_bgzf_member* table,
                      const uint32_t* sums, const bgzw::Head* head, uint64_t in_len, uint32_t block_len, uint32_t nblk,
                      uint64_t slot, uint8_t* out, uint64_t out_cap) {
    using namespace bgzw;
    __shared__ uint8_t s_pre[32], s_suf[8];
    if (head->total > out_cap || head->bad != NO_BAD) return;
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const uint32_t mw = mlen[k];
    const uint32_t m = mw & ~STORED;
    const bool stored = (mw & STORED) != 0;
    const bool last = k == nblk;
    const uint32_t len = last ? 0u : block_bytes(k, in_len, block_len);
    const uint32_t pl = last ? EOF_LEN : stored ? HEADER_LEN + 5u : HEADER_LEN;    // prefix, body, trailer
    const uint32_t sl = last ? 0u : 8u;
    const uint32_t bl = m - pl - sl;
    const uint8_t* src = stored ? slots + (uint64_t)k * block_len : staged + (uint64_t)k * slot;
    if (tid < 32) {
        uint32_t v = 0;
        if (tid < (last ? EOF_LEN : 16u)) v = ndfl_bgzw_eof[tid];
        else if (tid < HEADER_LEN) v = (m - 1) >> (8 * (tid - 16));
        else if (tid == HEADER_LEN) v = 1;                                           // BFINAL, BTYPE 00, padding
        else if (tid < HEADER_LEN + 3) v = len >> (8 * (tid - HEADER_LEN - 1));
        else if (tid < HEADER_LEN + 5) v = ~len >> (8 * (tid - HEADER_LEN - 3));
        s_pre[tid] = (uint8_t)v;
    } else if (tid < 40) {
        const uint32_t j = tid - 32;
        s_suf[j] = (uint8_t)(last ? 0u : j < 4 ? sums[k] >> (8 * j) : len >> (8 * (j - 4)));
    }
    __syncthreads();
    auto byte_at = [&](uint32_t p) -> uint32_t {
        return p < pl ? s_pre[p] : p < pl + bl ? src[p - pl] : s_suf[p - pl - bl];
    };
    uint8_t* dst = out + table[k].in_off;
    const uint32_t lead = min(m, (uint32_t)((0 - (uintptr_t)dst) & 3));
    const uint32_t nw = (m - lead) / 4;
    if (tid < lead) dst[tid] = (uint8_t)byte_at(tid);
    uint32_t* dw = (uint32_t*)(dst + lead);
    for (uint32_t w = tid; w < nw; w += PACK_THREADS) {
        const uint32_t p = lead + 4 * w;
        uint32_t v;
        if (p >= pl && p + 4 <= pl + bl) {
            const uint8_t* a = src + (p - pl);
            const uint32_t r = (uint32_t)((uintptr_t)a & 3);
            const uint32_t* sw = (const uint32_t*)(a - r);
            v = r ? __builtin_amdgcn_alignbyte(sw[1], sw[0], r) : sw[0];             // (r != 0: byte a + 3 is in sw[1])
        } else {
            v = byte_at(p) | byte_at(p + 1) << 8 | byte_at(p + 2) << 16 | byte_at(p + 3) << 24;
        }
        dw[w] = v;
    }
    const uint32_t done = lead + 4 * nw;
    if (tid < m - done) dst[done + tid] = (uint8_t)byte_at(done + tid);
}
