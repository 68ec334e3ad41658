// inflate_bgzf.hip -- blocked gzip (BGZF) files: the members found and laid out on the device, then
// decoded by ndfl_inflate_members_kernel in one launch (ndfl_inflate_bgzf, include/ndfl.h).
//
// A BGZF member carries its own length (BSIZE, in the `BC` subfield of its extra field) and its
// output length (ISIZE, its last four bytes), so the file splits without decoding a bit.  The only
// serial thing about it is the chain: member k + 1 starts where member k says it ends, and a byte
// pattern that looks like a member start elsewhere -- inside a stored block, say -- is not one.  The
// passes, none of which hands data to another workgroup inside a launch (each reads what an earlier
// LAUNCH wrote):
//   scan    every byte position is tested for a member start (member_start below: the issue's rule, and
//           nothing else of the header); FIND_TILE positions per workgroup.  Pass one counts per tile,
//           one workgroup turns the counts into offsets (ndfl_bgzf_sum_kernel), pass two tests again and writes
//           the candidates IN FILE ORDER: position and length (BSIZE + 1).
//   link    candidate i's successor is the candidate AT position pos + length (mostly i + 1, else a
//           binary search in the ordered list), or none.
//   mark    the chain from candidate 0 (if it is at byte 0) by pointer doubling: in round k every marked
//           candidate marks the one 2^k links on, and every jump doubles.  bit_length(bound on the
//           chain's length) launches, each over the candidates only; a mark read in the round that
//           writes it is that of a true chain member, so the rounds need no ordering inside a launch.
//   layout  over the candidates: (marked, ISIZE if marked) summed per tile of LIST_TILE, scanned by the
//           same one-workgroup kernel, then written: member k's ndfl_member_item (NDFL_FMT_GZIP, out_cap =
//           ISIZE) and table entry, the totals into the header block.
//   (host sync: the candidate count against the list's capacity, n_members, the total against out_cap)
//   decode  ndfl_inflate_members_kernel on the device-built items.
//   reduce  one workgroup: the failing member with the lowest index, its result and its out_off.
// 9 launches and the mark rounds: the count grows with the logarithm of the file's size (of the candidate
// count after a second scan), not with the number of members.
//
// The candidate list holds in_len / 2048 + 4096 entries at first (a BGZF block of real data is 10 to
// 25 KiB); a file with more candidates -- mostly tiny members, or payloads full of look-alikes -- is
// scanned again with room for the number the first scan counted, as the header finder does
// (FIND_OVERFLOW).
//
// All kernels: no calls, no arrays indexed at run time, so no scratch memory (DESIGN.md §7 item 9;
// tests/test_bgzf_kernel_resources.py).
#pragma once

namespace bgzf {

constexpr uint32_t FIND_THREADS = 256;        // threads of a scan workgroup
constexpr uint32_t FIND_BYTES = 16;           // consecutive positions per thread
constexpr uint32_t FIND_TILE = 4096;          // positions per workgroup step
constexpr uint32_t LIST_TILE = 256;           // candidates per workgroup step (link, mark, layout)
constexpr uint32_t SUM_BLOCK = 1024;          // threads, and entries per step, of ndfl_bgzf_sum_kernel
constexpr uint32_t LIST_MIN = 4096;           // the candidate list's first capacity: in_len / LIST_DIV + LIST_MIN
constexpr uint32_t LIST_DIV = 2048;
constexpr uint32_t FIND_GRID = 8192;          // most workgroups of a scan launch (each strides over the tiles) ...
constexpr uint32_t LIST_GRID = 1024;          // ... and of a link, mark or layout launch (NDFL_BGZF_GRID caps both)
constexpr uint32_t NO_NEXT = 0xFFFFFFFFu;
static_assert(FIND_TILE == FIND_THREADS * FIND_BYTES, "a scan step is one tile");

// What the passes leave for the host (zeroed before the first launch).
struct Head {
    uint32_t n_cand;          // candidates in the file (may exceed the list's capacity: scan again)
    uint32_t n_members;
    uint64_t total;           // the sum of the members' ISIZE
    uint64_t consumed;        // the offset just past the chain's last member
    uint32_t bad;             // reduce: the first failing member, or n_members
    int32_t bad_status;       //   its status (the kernel's internal codes)
    uint64_t bad_out_len;     //   out_off[bad] + its out_len
};

// The input: byte i, for i < len only (w has (len + 3) / 4 words).
struct View {
    const uint32_t* w;
    uint64_t len;
    __device__ __forceinline__ uint32_t byte(uint64_t i) const { return (w[i >> 2] >> (8 * (uint32_t)(i & 3))) & 0xFFu; }
    __device__ __forceinline__ uint32_t le16(uint64_t i) const { return byte(i) | byte(i + 1) << 8; }
    __device__ __forceinline__ uint32_t word(uint64_t k) const { return k < (len + 3) / 4 ? w[k] : 0u; }
};

// Is p a member start?  1f 8b 08 at p, FLG bit 2, the 12 fixed bytes and all XLEN extra bytes inside
// the input, a subfield 'B' 'C' of length 2 on the walk of the extra field (wholly inside it), and
// BSIZE + 1 >= 12 + XLEN + 8.  mlen = BSIZE + 1.
__device__ __forceinline__ bool member_start(const View& v, uint64_t p, uint32_t& mlen) {
    if (p > v.len || v.len - p < 12) return false;
    if (v.byte(p) != 0x1Fu || v.byte(p + 1) != 0x8Bu || v.byte(p + 2) != 8u || !(v.byte(p + 3) & 4u)) return false;
    const uint32_t xlen = v.le16(p + 10);
    if (v.len - p - 12 < xlen) return false;
    const uint64_t x = p + 12;
    for (uint32_t q = 0; q + 4 <= xlen;) {
        const uint32_t sl = v.le16(x + q + 2);
        if (v.byte(x + q) == 66u && v.byte(x + q + 1) == 67u && sl == 2u && q + 6 <= xlen) {
            mlen = v.le16(x + q + 4) + 1u;
            return mlen >= 12u + xlen + 8u;
        }
        q += 4 + sl;
    }
    return false;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, uint32_t o) {
    const uint32_t lo = __shfl_up((uint32_t)x, o, 64), hi = __shfl_up((uint32_t)(x >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t shfl_up_t(uint32_t x, uint32_t o) { return __shfl_up(x, o, 64); }
__device__ __forceinline__ uint64_t shfl_up_t(uint64_t x, uint32_t o) { return shfl_up64(x, o); }

// The exclusive prefix of v over the workgroup's NT threads and the workgroup's total; s_w: NT / 64
// values of LDS, free again on return.
template <uint32_t NT, class T>
__device__ __forceinline__ T block_scan(T v, T* s_w, T& total) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T y = shfl_up_t(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wid] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < NT / 64; k++) {
        const T s = s_w[k];
        base += k < wid ? s : (T)0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// The member starts among this thread's FIND_BYTES positions from at0 (a multiple of 16) on, as a bit
// mask; their lengths are computed again by whoever needs them.  The cheap test first: the four bytes
// at a position, taken from five words.
__device__ __forceinline__ uint32_t scan_positions(const View& v, uint64_t at0) {
    const uint64_t k = at0 >> 2;
    const uint32_t w0 = v.word(k), w1 = v.word(k + 1), w2 = v.word(k + 2), w3 = v.word(k + 3), w4 = v.word(k + 4);
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t j = 0; j < FIND_BYTES; j++) {
        const uint32_t a = j >> 2, sh = 8 * (j & 3);
        const uint32_t lo = a == 0 ? w0 : a == 1 ? w1 : a == 2 ? w2 : w3;
        const uint32_t hi = a == 0 ? w1 : a == 1 ? w2 : a == 2 ? w3 : w4;
        const uint32_t four = __builtin_amdgcn_alignbit(hi, lo, sh);
        if ((four & 0x04FFFFFFu) == 0x04088B1Fu) {
            uint32_t mlen;
            if (member_start(v, at0 + j, mlen)) mask |= 1u << j;
        }
    }
    return mask;
}

}  // namespace bgzf

// Scan pass one (WRITE = false): tile_cnt[t] = the member starts in tile t.  Pass two (WRITE = true):
// tile_cnt holds the tiles' offsets; candidate number i < cap goes to cpos[i], clen[i].
template <bool WRITE>
__global__ void __launch_bounds__(bgzf::FIND_THREADS)
ndfl_bgzf_scan_kernel(const uint32_t* w, uint64_t in_len, uint32_t ntiles, uint32_t* tile_cnt, uint32_t cap,
                      uint64_t* cpos, uint32_t* clen) {
    using namespace bgzf;
    __shared__ uint32_t s_w[FIND_THREADS / 64];
    const View v{w, in_len};
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t at0 = (uint64_t)t * FIND_TILE + (uint64_t)threadIdx.x * FIND_BYTES;
        const uint32_t mask = at0 < in_len ? scan_positions(v, at0) : 0u;
        uint32_t total;
        uint32_t at = block_scan<FIND_THREADS>((uint32_t)__popc(mask), s_w, total);
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) tile_cnt[t] = total;
        } else {
            at += tile_cnt[t];
            for (uint32_t m = mask; m; m &= m - 1, at++) {
                const uint64_t p = at0 + (uint32_t)(__ffs(m) - 1);
                uint32_t mlen = 0;
                member_start(v, p, mlen);
                if (at < cap) { cpos[at] = p; clen[at] = mlen; }
            }
        }
    }
}

// One workgroup: cnt[0, n) and, if given, sum[0, n) become their exclusive prefixes; the totals go to
// *tot_cnt and *tot_sum.
extern "C" __global__ void __launch_bounds__(bgzf::SUM_BLOCK)
ndfl_bgzf_sum_kernel(uint32_t* cnt, uint64_t* sum, uint32_t n, uint32_t* tot_cnt, uint64_t* tot_sum) {
    using namespace bgzf;
    __shared__ uint32_t s_c[SUM_BLOCK / 64];
    __shared__ uint64_t s_s[SUM_BLOCK / 64];
    uint32_t carry_c = 0;
    uint64_t carry_s = 0;
    for (uint32_t base = 0; base < n; base += SUM_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        uint32_t tc;
        const uint32_t c = i < n ? cnt[i] : 0u;
        const uint32_t pc = block_scan<SUM_BLOCK>(c, s_c, tc);
        if (i < n) cnt[i] = carry_c + pc;
        carry_c += tc;
        if (sum) {
            uint64_t ts;
            const uint64_t s = i < n ? sum[i] : 0ull;
            const uint64_t ps = block_scan<SUM_BLOCK>(s, s_s, ts);
            if (i < n) sum[i] = carry_s + ps;
            carry_s += ts;
        }
    }
    if (threadIdx.x == 0) {
        *tot_cnt = carry_c;
        if (sum) *tot_sum = carry_s;
    }
}

// jump[i] = the candidate at cpos[i] + clen[i], or NO_NEXT; mark[i] = 1 for candidate 0 at byte 0, else 0.
extern "C" __global__ void __launch_bounds__(bgzf::LIST_TILE)
ndfl_bgzf_link_kernel(const uint64_t* cpos, const uint32_t* clen, const uint32_t* n_cand, uint32_t cap,
                      uint32_t* jump, uint32_t* mark) {
    using namespace bgzf;
    const uint32_t n = min(*n_cand, cap);
    for (uint32_t i = blockIdx.x * LIST_TILE + threadIdx.x; i < n; i += gridDim.x * LIST_TILE) {
        const uint64_t to = cpos[i] + clen[i];
        uint32_t lo = i + 1, hi = n;                      // the first candidate at or past `to` is in [lo, hi]
        if (lo < n && cpos[lo] >= to) hi = lo;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cpos[mid] < to) lo = mid + 1;
            else hi = mid;
        }
        jump[i] = lo < n && cpos[lo] == to ? lo : NO_NEXT;
        mark[i] = i == 0 && cpos[0] == 0 ? 1u : 0u;
    }
}

// One round of pointer doubling: every marked candidate marks the one its jump names, and jump_out =
// the jump of the jump.
extern "C" __global__ void __launch_bounds__(bgzf::LIST_TILE)
ndfl_bgzf_mark_kernel(const uint32_t* n_cand, uint32_t cap, const uint32_t* jump_in, uint32_t* jump_out,
                      uint32_t* mark) {
    using namespace bgzf;
    const uint32_t n = min(*n_cand, cap);
    for (uint32_t i = blockIdx.x * LIST_TILE + threadIdx.x; i < n; i += gridDim.x * LIST_TILE) {
        const uint32_t j = jump_in[i];
        if (j == NO_NEXT) { jump_out[i] = NO_NEXT; continue; }
        if (mark[i]) mark[j] = 1u;
        jump_out[i] = jump_in[j];
    }
}

// Layout pass one (WRITE = false): tile_cnt[t] / tile_sum[t] = the members among tile t's candidates
// and the sum of their ISIZE, for every tile of the list's capacity (ntiles).  Pass two (WRITE = true): the two hold the tiles' offsets, head the
// totals; member k's item and table entry are written, and the entry after the last.
template <bool WRITE>
__global__ void __launch_bounds__(bgzf::LIST_TILE)
ndfl_bgzf_layout_kernel(const uint32_t* w, uint64_t in_len, const uint64_t* cpos, const uint32_t* clen,
                        const uint32_t* mark, uint32_t cap, uint32_t ntiles, uint32_t* tile_cnt, uint64_t* tile_sum,
                        bgzf::Head* head, ndfl_member_item* items, ndfl_bgzf_member* table) {
    using namespace bgzf;
    __shared__ uint32_t s_c[LIST_TILE / 64];
    __shared__ uint64_t s_s[LIST_TILE / 64];
    const View v{w, in_len};
    const uint32_t n = min(head->n_cand, cap);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {       // (all the list's tiles: the sum kernel reads them all)
        const uint32_t i = t * LIST_TILE + threadIdx.x;
        const bool member = i < n && mark[i] != 0;
        uint64_t pos = 0, mlen = 0, isize = 0;
        if (member) {
            pos = cpos[i];
            mlen = min((uint64_t)clen[i], in_len - pos);  // (a member start has its 12 bytes: mlen >= 12)
            const uint64_t a = pos + mlen - 4;
            isize = v.byte(a) | v.byte(a + 1) << 8 | v.byte(a + 2) << 16 | v.byte(a + 3) << 24;
        }
        uint32_t tc;
        uint64_t ts;
        uint32_t k = block_scan<LIST_TILE>(member ? 1u : 0u, s_c, tc);
        uint64_t off = block_scan<LIST_TILE>(isize, s_s, ts);
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) { tile_cnt[t] = tc; tile_sum[t] = ts; }
        } else if (member) {
            k += tile_cnt[t];
            off += tile_sum[t];
            ndfl_member_item it;
            it.in_off = pos; it.in_len = mlen; it.out_off = off; it.out_cap = isize;
            it.format = NDFL_FMT_GZIP; it.sum = NDFL_SUM_NONE;
            items[k] = it;
            table[k] = ndfl_bgzf_member{pos, off};
            if (k + 1 == head->n_members) {
                table[k + 1] = ndfl_bgzf_member{pos + mlen, head->total};
                head->consumed = pos + mlen;
            }
        }
    }
}

// One workgroup: the failing member with the lowest index.  A member fails with a status other than 0,
// or with a decoded length other than the ISIZE the layout gave it as its capacity -- possible without a
// Reason only where bytes follow its trailer inside BSIZE, and reported as the size mismatch it is.
extern "C" __global__ void __launch_bounds__(bgzf::SUM_BLOCK)
ndfl_bgzf_reduce_kernel(const ndfl_member_item* items, const ndfl_member_result* results, uint32_t n,
                        bgzf::Head* head) {
    using namespace bgzf;
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = n;
    __syncthreads();
    uint32_t bad = n;
    for (uint32_t i = threadIdx.x; i < n && bad == n; i += SUM_BLOCK)
        if (results[i].status != 0 || results[i].out_len != items[i].out_cap) bad = i;
    if (bad < n) atomicMin(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        bad = s_bad;
        head->bad = bad;
        if (bad < n) {
            const int32_t st = results[bad].status;
            head->bad_status = st == 0 || st == NDFL_E_CAPACITY ? NDFL_DECOMPRESSED_SIZE_MISMATCH : st;
            head->bad_out_len = items[bad].out_off + results[bad].out_len;
        } else {
            head->bad_status = 0;
            head->bad_out_len = head->total;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------
struct BgzfScratch {
    DevBuf d;                                 // the head, the tile counts, the candidate list, the table
    hipEvent_t ev_mid = nullptr;              // between the layout and the decode
    void release() {
        d.release();
        if (ev_mid) hipEventDestroy(ev_mid);
        ev_mid = nullptr;
    }
};

// What inflate_bgzf_run reports: ndfl_bgzf_result with the kernel's internal status.
struct BgzfOutcome {
    int32_t status = 0;
    uint32_t n_members = 0, bad_member = 0;
    uint64_t out_len = 0, consumed = 0;
};

// ndfl_inflate_bgzf on stream s (arguments validated): discovery and layout, a host sync for the sizes,
// the members kernel and the reduction, a second sync.  `table` receives min(table_cap, n_members + 1)
// entries in every case.  S.last_ms_find / S.last_ms_emit: the time up to the layout's end and from
// there on; *last_ms their sum.
static int inflate_bgzf_run(InflateScratch& S, BatchScratch& B, BgzfScratch& Z, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                            BgzfOutcome* res, ndfl_bgzf_member* table, uint32_t table_cap, uint32_t flags,
                            double* last_ms, const uint32_t* crc_x) {
    using namespace bgzf;
    *res = BgzfOutcome{};
    if (in_len == 0) {
        if (table_cap) table[0] = ndfl_bgzf_member{0, 0};
        *last_ms = 0; S.last_ms_find = 0; S.last_ms_emit = 0;   // (no kernel ran)
        return 0;
    }
    const uint32_t* d_w = nullptr;
    INF_RC(stage_input(S, s, in, in_len, flags, &d_w));
    if (!Z.ev_mid) INF_CHK(hipEventCreate(&Z.ev_mid));
    const uint32_t ntiles = (uint32_t)((in_len + FIND_TILE - 1) / FIND_TILE);
    const uint32_t grid_cap = S.knobs.bgzf_grid ? S.knobs.bgzf_grid : ~0u;
    const uint32_t scan_grid = std::min(ntiles, std::min(FIND_GRID, grid_cap));
    std::vector<ndfl_bgzf_member> h_table;               // the table's first entries, brought back with the head
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    uint64_t cap = in_len / LIST_DIV + LIST_MIN;
    Head h;
    ndfl_member_item* d_items = nullptr;
    ndfl_member_result* d_res = nullptr;
    uint32_t* d_ticket = nullptr;
    Head* d_head = nullptr;
    ndfl_bgzf_member* d_table = nullptr;
    INF_CHK(hipEventRecord(e0, s));
    for (int pass = 0;; pass++) {
        const uint32_t ltiles = (uint32_t)((cap + LIST_TILE - 1) / LIST_TILE);
        const uint32_t list_grid = std::min(ltiles, std::min(LIST_GRID, grid_cap));
        const size_t o_head = 0, o_tcnt = up(sizeof(Head)), o_cpos = o_tcnt + up((size_t)ntiles * 4),
                     o_clen = o_cpos + up(cap * 8), o_ja = o_clen + up(cap * 4), o_jb = o_ja + up(cap * 4),
                     o_mark = o_jb + up(cap * 4), o_lcnt = o_mark + up(cap * 4), o_lsum = o_lcnt + up((size_t)ltiles * 4),
                     o_table = o_lsum + up((size_t)ltiles * 8), o_end = o_table + up((cap + 1) * sizeof(ndfl_bgzf_member));
        INF_CHK(Z.d.ensure(o_end));
        const size_t items_b = cap * sizeof(ndfl_member_item), res_b = cap * sizeof(ndfl_member_result);
        INF_CHK(B.d_items.ensure(items_b + res_b + 16));
        char* z = Z.d.as<char>();
        d_head = (Head*)(z + o_head);
        uint32_t* d_tcnt = (uint32_t*)(z + o_tcnt);
        uint64_t* d_cpos = (uint64_t*)(z + o_cpos);
        uint32_t* d_clen = (uint32_t*)(z + o_clen);
        uint32_t* d_ja = (uint32_t*)(z + o_ja);
        uint32_t* d_jb = (uint32_t*)(z + o_jb);
        uint32_t* d_mark = (uint32_t*)(z + o_mark);
        uint32_t* d_lcnt = (uint32_t*)(z + o_lcnt);
        uint64_t* d_lsum = (uint64_t*)(z + o_lsum);
        d_table = (ndfl_bgzf_member*)(z + o_table);
        d_items = B.d_items.as<ndfl_member_item>();
        d_res = (ndfl_member_result*)(B.d_items.as<char>() + items_b);
        d_ticket = (uint32_t*)((char*)d_res + res_b);
        INF_CHK(hipMemsetAsync(d_head, 0, up(sizeof(Head)), s));
        INF_CHK(hipMemsetAsync(d_ticket, 0, 16, s));
        const uint32_t cap32 = (uint32_t)cap;
        hipLaunchKernelGGL(ndfl_bgzf_scan_kernel<false>, dim3(scan_grid), dim3(FIND_THREADS), 0, s, d_w, in_len, ntiles,
                           d_tcnt, cap32, d_cpos, d_clen);
        hipLaunchKernelGGL(ndfl_bgzf_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, s, d_tcnt, (uint64_t*)nullptr, ntiles,
                           &d_head->n_cand, (uint64_t*)nullptr);
        hipLaunchKernelGGL(ndfl_bgzf_scan_kernel<true>, dim3(scan_grid), dim3(FIND_THREADS), 0, s, d_w, in_len, ntiles,
                           d_tcnt, cap32, d_cpos, d_clen);
        hipLaunchKernelGGL(ndfl_bgzf_link_kernel, dim3(list_grid), dim3(LIST_TILE), 0, s, d_cpos, d_clen, &d_head->n_cand,
                           cap32, d_ja, d_mark);
        // a chain of m members needs bit_length(m - 1) rounds; m <= the candidates, and a member has >= 26 bytes
        const uint64_t longest = std::min<uint64_t>(cap, in_len / 26 + 1);
        uint32_t rounds = 0;
        while ((longest - 1) >> rounds) rounds++;
        for (uint32_t r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(ndfl_bgzf_mark_kernel, dim3(list_grid), dim3(LIST_TILE), 0, s, &d_head->n_cand, cap32, d_ja,
                               d_jb, d_mark);
            std::swap(d_ja, d_jb);
        }
        hipLaunchKernelGGL(ndfl_bgzf_layout_kernel<false>, dim3(list_grid), dim3(LIST_TILE), 0, s, d_w, in_len, d_cpos,
                           d_clen, d_mark, cap32, ltiles, d_lcnt, d_lsum, d_head, d_items, d_table);
        hipLaunchKernelGGL(ndfl_bgzf_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, s, d_lcnt, d_lsum, ltiles, &d_head->n_members,
                           &d_head->total);
        hipLaunchKernelGGL(ndfl_bgzf_layout_kernel<true>, dim3(list_grid), dim3(LIST_TILE), 0, s, d_w, in_len, d_cpos,
                           d_clen, d_mark, cap32, ltiles, d_lcnt, d_lsum, d_head, d_items, d_table);
        INF_CHK(hipGetLastError());
        INF_CHK(hipEventRecord(Z.ev_mid, s));
        INF_CHK(hipMemcpyAsync(&h, d_head, sizeof(Head), hipMemcpyDeviceToHost, s));
        // (n_members is not known yet: as many entries as the caller and the list have room for, of which the
        // first n_members + 1 are the table's and go on to the caller)
        h_table.resize((size_t)std::min<uint64_t>(table_cap, cap + 1));
        if (!h_table.empty())
            INF_CHK(hipMemcpyAsync(h_table.data(), d_table, h_table.size() * sizeof(ndfl_bgzf_member), hipMemcpyDeviceToHost, s));
        INF_CHK(hipStreamSynchronize(s));
        if (h.n_cand <= cap) break;
        if (pass) return NDFL_E_INTERNAL;                             // (the second list has room for every candidate)
        cap = h.n_cand;
        if (S.knobs.stats) fprintf(stderr, "[ndfl] inflate bgzf: %u candidates, scanning again\n", h.n_cand);
    }
    const uint32_t n = h.n_members;
    res->n_members = n;
    res->bad_member = n;
    res->consumed = h.consumed;
    res->out_len = h.total;
    const uint32_t nt = (uint32_t)std::min<uint64_t>(table_cap, (uint64_t)n + 1);
    if (nt) {
        if (n) memcpy(table, h_table.data(), (size_t)nt * sizeof(ndfl_bgzf_member));
        else table[0] = ndfl_bgzf_member{0, 0};
    }
    float ms = 0;
    if (h.total > out_cap || n == 0) {
        if (h.total > out_cap) res->status = NDFL_E_CAPACITY;
        if (hipEventElapsedTime(&ms, e0, Z.ev_mid) == hipSuccess) { *last_ms = ms; S.last_ms_find = ms; S.last_ms_emit = 0; }
        return 0;
    }
    const bool out_dev = (flags & NDFL_OUT_DEVICE) != 0;
    const uint64_t total = h.total;
    uint8_t* d_out = out;
    if (!out_dev && total) {
        INF_CHK(B.d_out.ensure(total));
        d_out = B.d_out.as<uint8_t>();
    }
    const uint32_t grid = batch_grid<ndfl_inflate_members_kernel>(n, S.knobs, "inflate bgzf");
    hipLaunchKernelGGL(ndfl_inflate_members_kernel, dim3(grid), dim3(64), 0, s, d_w, d_out, d_items, d_res, n, d_ticket,
                       crc_x);
    hipLaunchKernelGGL(ndfl_bgzf_reduce_kernel, dim3(1), dim3(SUM_BLOCK), 0, s, d_items, d_res, n, d_head);
    INF_CHK(hipGetLastError());
    INF_CHK(hipEventRecord(e1, s));
    INF_CHK(hipMemcpyAsync(&h, d_head, sizeof(Head), hipMemcpyDeviceToHost, s));
    // (on a Reason the bytes of [out_len, total) are unspecified: the whole span comes back in one copy)
    if (!out_dev && total) INF_CHK(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    float ms2 = 0;
    if (hipEventElapsedTime(&ms, e0, Z.ev_mid) == hipSuccess && hipEventElapsedTime(&ms2, Z.ev_mid, e1) == hipSuccess) {
        *last_ms = (double)ms + ms2; S.last_ms_find = ms; S.last_ms_emit = ms2;
    }
    res->status = h.bad_status;
    res->bad_member = h.bad;
    res->out_len = h.bad_out_len;
    return 0;
}
