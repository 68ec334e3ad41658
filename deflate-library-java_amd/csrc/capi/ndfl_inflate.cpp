// ndfl_inflate.cpp -- host side of one raw-DEFLATE decode (the kernels: csrc/hip/inflate_kernels.hip).
// Included by ndfl_capi.cpp directly after the kernels; the batch and BGZF runners use stage_input,
// INF_CHK and occupancy_grid.  One call is one Decode frame; DESIGN.md §4 lists its stages in launch order.
#include <chrono>
#include <unordered_map>

struct InflateScratch {
    DevBuf d_in, d_cand, d_starts, d_stops, d_res, d_cands, d_stats, d_chains, d_out;
    DevBuf d_q, d_seg;                                 // finder survivors (stage 1 -> stage 2); segment record pool
    SegPool pool{};
    DevBuf d_ref, d_pend;                              // emit: back-reference / pending bit per output byte (deferred copies)
    DevBuf d_rl;                                       // resolve: two group lists + round bits
    DevBuf d_ticket;
    DevBuf d_slow;                                     // emit: chains the fast emit pass leaves to the full one
    DevBuf d_rep;                                      // count: the candidate counted for each (stored-header aliases)
    DevBuf d_ph, d_hrec, d_cticket;                    // count pass: phase-fallback slot per wave, header record per
                                                       //   candidate, chain tickets (one per launch)
    DevBuf d_info, d_link;                             // device-side linking: summary (LI_*), pointer-jumping levels and sums
    void* h_info = nullptr;                            //   the summary's pinned host copy
    void* h_cnt = nullptr;                             // pinned: resolve list size
    Knobs knobs;                                       // the context's switches (ndfl_common.hpp)
    uint32_t q_cap = 0, q_min = 0;                     // finder survivor list: capacity of the last scan / asked minimum
    bool q_full = false;                               //   the last scan's list could not grow (budget, allocation)
    double last_ms_find = 0, last_ms_count = 0, last_ms_emit = 0, last_ms_wall = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t repairs = 0, chains = 0, candidates = 0, resolved_groups = 0, flat_chains = 0;
    uint64_t pending_after_dev = 0;                    // 32-byte groups still pending after the device-queued resolve rounds
    bool count_first = false;
    // state kept for ndfl_inflate_resolve after a deferred-window range decode
    bool pending = false;
    uint8_t* p_out = nullptr;
    uint64_t p_nbytes = 0, p_dict_len = 0;
    void release() {
        for (DevBuf* b : {&d_in, &d_cand, &d_starts, &d_stops, &d_res, &d_cands, &d_stats, &d_chains, &d_out, &d_q, &d_seg,
                          &d_ref, &d_pend, &d_rl, &d_ticket, &d_slow, &d_rep, &d_ph, &d_hrec, &d_cticket, &d_info, &d_link})
            b->release();
        for (auto& e : ev) { if (e) hipEventDestroy(e); e = nullptr; }
        for (void** h : {&h_cnt, &h_info}) { if (*h) hipHostFree(*h); *h = nullptr; }
        pending = false;
    }
};

// Persistent grid of a kernel with `threads` threads per workgroup: what fits on the chip at once
// (occupancy), at most `cap` workgroups -- `cap` itself when the runtime cannot say.  `env` names a
// workgroups-per-CU override (tuning).
template <typename K>
static uint32_t occupancy_grid(K kernel, uint32_t threads, uint32_t cap, const char* env = nullptr) {
    int dev = 0, ncu = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, (int)threads, 0) != hipSuccess || ncu <= 0 || per <= 0)
        return cap;
    if (env && getenv(env)) per = std::max(1, atoi(getenv(env)));
    return std::min<uint32_t>(cap, (uint32_t)(ncu * per));
}

// The count pass: one wave per chain (W = 1) or W waves per chain (workgroup rounds,
// inflate_wg.hpp); NDFL_COUNT_W selects W (1, 2, 4, 8).  Persistent grid sized by occupancy; the
// phase-fallback slots (d_ph) cover COUNT_WAVES waves.
static uint32_t count_w(const Knobs& k) {
    const uint32_t v = k.count_w ? k.count_w : (uint32_t)NDFL_COUNT_W_DEFAULT;
    return (v == 2 || v == 4 || v == 8) ? v : 1u;
}
static uint32_t count_wave_grid() {
    static const uint32_t g = occupancy_grid(ndfl_inflate_count_wave_kernel, 64, inf::COUNT_WAVES, "NDFL_COUNT_WPC"); return g;
}
template <uint32_t W, typename... A>
static void launch_count_wg(hipStream_t s, uint32_t nchains, A... args) {
    static const uint32_t g = occupancy_grid(ndfl_inflate_count_wg_kernel<W>, 64 * W, inf::COUNT_WAVES / W);
    hipLaunchKernelGGL(ndfl_inflate_count_wg_kernel<W>, dim3(std::min(nchains, g)), dim3(64 * W), 0, s, args...);
}
template <typename... A>
static void launch_count(hipStream_t s, uint32_t W, uint32_t nchains, A... args) {
    if (W == 1)
        hipLaunchKernelGGL(ndfl_inflate_count_wave_kernel, dim3(std::min(nchains, count_wave_grid())), dim3(64), 0, s, args...);
    else if (W == 2) launch_count_wg<2>(s, nchains, args...);
    else if (W == 4) launch_count_wg<4>(s, nchains, args...);
    else launch_count_wg<8>(s, nchains, args...);
}

static bool inf_debug() { static const bool d = getenv("NDFL_DEBUG") != nullptr; return d; }
#define INF_CHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) {                                             \
        if (inf_debug()) fprintf(stderr, "[ndfl] HIP error %d (%s) at ndfl_inflate.cpp:%d\n", (int)_e,         \
                                 hipGetErrorString(_e), __LINE__);                                              \
        return NDFL_E_DEVICE; } } while (0)
#define INF_RC(x) do { const int _r = (x); if (_r) return _r; } while (0)

constexpr int LINK_FALLBACK = 1000;      // the device linker hands over to the host linker
constexpr int FIND_OVERFLOW = 1001;      // more finder survivors than the list held: scan again
constexpr int WALK_COUNT = 1002;         // the host linker's walk needs one more boundary counted
constexpr uint32_t LI_QCOUNT = 14;       // (host copy only: the finder's survivor count)

// ---- the host linker's pure parts (no HIP call; scripts/sanitize_inflate_host.cpp drives them) ----------
// The candidate list of [start_bit, end_bit): slot 0 is the range start, then the sorted candidates
// strictly inside the range (a header found at the start itself is a duplicate of slot 0).
static void filter_range(std::vector<uint64_t>& starts, uint64_t start_bit, uint64_t end_bit) {
    if (starts.empty()) starts.resize(1);
    starts[0] = start_bit;
    size_t m = 1;
    for (size_t k = 1; k < starts.size(); k++)
        if (starts[k] > start_bit && starts[k] < end_bit) starts[m++] = starts[k];
    starts.resize(m);
}

// The count pass's claim order: longest first (by the bits to the next start), so that no long chain
// is left for the end of the launch; bucketed by 32 Kibit.  An unsorted list (repairs) keeps its order.
static std::vector<uint32_t> count_order(const std::vector<uint64_t>& st, uint64_t end_bit) {
    constexpr int NB = 24;
    const size_t n = st.size();
    std::vector<uint32_t> order(n);
    uint32_t bc[NB + 1] = {0};
    auto bucket = [&](size_t k) {
        const uint64_t nx = k + 1 < n ? st[k + 1] : end_bit;
        const uint64_t len = nx > st[k] ? nx - st[k] : 0;
        return NB - 1 - (int)std::min<uint64_t>(NB - 1, len >> 15);
    };
    if (std::is_sorted(st.begin(), st.end())) {
        for (size_t k = 0; k < n; k++) bc[bucket(k) + 1]++;
        for (int b = 0; b < NB; b++) bc[b + 1] += bc[b];
        for (size_t k = 0; k < n; k++) order[bc[bucket(k)]++] = (uint32_t)k;
    } else {
        for (size_t k = 0; k < n; k++) order[k] = (uint32_t)k;
    }
    return order;
}

// The counted chains of a range and how they link: starts[0, n0) is the sorted candidate list, the
// rest are repaired boundaries (found through `extra`); res[k] is the count pass's result of starts[k].
struct ChainLinks {
    std::vector<uint64_t> starts;
    std::vector<ChainRes> res;
    std::unordered_map<uint64_t, size_t> extra;
    uint64_t end_bit = inf::NONE, dict_len = 0;
    std::vector<EmitChain> chains;                    // the walk from the range start
    size_t n0 = 0, cur = 0;
    uint64_t produced = 0, stop_bit = 0;

    bool find_at(uint64_t b, size_t& idx) const {
        auto it = std::lower_bound(starts.begin(), starts.begin() + n0, b);
        if (it != starts.begin() + n0 && *it == b) { idx = (size_t)(it - starts.begin()); return true; }
        auto e = extra.find(b);
        if (e != extra.end()) { idx = e->second; return true; }
        return false;
    }
    bool links_on(size_t k) const { return res[k].next < n0 && starts[res[k].next] == res[k].end_bit; }
    // A boundary that is no candidate (fixed-Huffman block, header rejected by the finder) needs a
    // repair chain: every such boundary of every chain, each once (a placeholder until add() fills it).
    std::vector<uint64_t> repair_todo() {
        std::vector<uint64_t> todo;
        size_t dummy;
        for (size_t k = 0; k < res.size(); k++)
            if (res[k].status == inf::ST_BOUNDARY && res[k].end_bit < end_bit && !links_on(k) && !find_at(res[k].end_bit, dummy)) {
                extra[res[k].end_bit] = inf::NONE;
                todo.push_back(res[k].end_bit);
            }
        return todo;
    }
    void add(const std::vector<uint64_t>& todo, const std::vector<ChainRes>& r) {
        for (size_t k = 0; k < todo.size(); k++) {
            starts.push_back(todo[k]);
            res.push_back(r[k]);
            extra[todo[k]] = starts.size() - 1;
        }
    }
    // The EmitChain list from chain `cur` on.  0: the walk ended (stop_bit, produced); WALK_COUNT: the
    // chain at *need is not counted yet (past the parallel repair rounds) -- add() it, set cur to it
    // and walk on; NDFL_E_ARG: the range end is no block boundary.
    int walk(uint64_t* need) {
        using namespace inf;
        for (;;) {
            const ChainRes& r = res[cur];
            chains.push_back(EmitChain{starts[cur], r.end_bit, dict_len + produced, r.out_count, cur});
            produced += r.out_count;
            if (r.status == ST_FINAL) { stop_bit = r.end_bit; return 0; }
            if (r.status == ST_ERROR) return 0;
            if (r.end_bit == end_bit) { stop_bit = end_bit; return 0; }
            if (r.end_bit > end_bit) return NDFL_E_ARG;
            size_t nxt;
            if (links_on(cur)) { cur = r.next; continue; }
            if (find_at(r.end_bit, nxt) && nxt != (size_t)NONE) { cur = nxt; continue; }
            *need = r.end_bit;
            return WALK_COUNT;
        }
    }
};

// A decode's result from the emit pass's chain results: the first error in stream order (the emit pass
// also checks the dictionary bound exactly).  A partial-input decode that ran out of input inside a
// block stops at the last block boundary reached.
struct Outcome { int code; uint64_t produced, consumed_bits; };
static Outcome first_error(const std::vector<ChainRes>& er, const std::vector<EmitChain>& chains, uint64_t dict_len,
                           bool partial, uint64_t total, uint64_t stop_bit) {
    using namespace inf;
    for (size_t k = 0; k < er.size(); k++) {
        if (er[k].status != ST_ERROR) continue;
        if (partial && er[k].reason == R_UEOS) return {NEED_INPUT, chains[k].out_off - dict_len + er[k].bnd_cnt, er[k].bnd_bit};
        return {(int)er[k].reason, chains[k].out_off - dict_len + er[k].out_count, er[k].end_bit};
    }
    return {0, total, stop_bit};
}

// Sync probe: a chain of blocks from a header candidate that ends exactly at another candidate y has
// decoded up to y in step with the stream (a decode that starts off a block boundary re-synchronises
// inside the block and then ends at its real end-of-block), so y is a block boundary; y is taken when
// its own chain links on in turn (or is final).  NONE if there is none.
static uint64_t first_sync(const std::vector<uint64_t>& starts, const std::vector<ChainRes>& res) {
    using namespace inf;
    auto linked = [&](size_t k) {
        return res[k].status == ST_BOUNDARY && res[k].next < starts.size() && starts[res[k].next] == res[k].end_bit;
    };
    for (size_t k = 1; k < res.size(); k++) {
        if (!linked(k)) continue;
        const size_t j = res[k].next;
        if (j >= 1 && (linked(j) || res[j].status == ST_FINAL)) return starts[j];
    }
    return NONE;
}

// ---- stages shared with the batch and BGZF runners ---------------------------------------------------
// The decoder's input words: staged into a zero-padded scratch copy, so the decode lanes' 16-byte
// prefetches (up to IN_PAD bytes past the end) need no bounds checks -- unless the caller says its
// device buffer already is one (NDFL_IN_PADDED: 16-byte aligned, IN_PAD zero bytes after the data),
// in which case it is read in place.
static int stage_input(InflateScratch& S, hipStream_t s, const uint8_t* in, uint64_t in_len, uint32_t flags,
                       const uint32_t** d_w) {
    using namespace inf;
    const uint64_t nwords = (in_len + 3) / 4;
    const bool in_dev = (flags & NDFL_IN_DEVICE) != 0;
    const bool in_place = in_len && in_dev && (flags & NDFL_IN_PADDED) && ((uintptr_t)in & 15u) == 0;
    *d_w = (const uint32_t*)in;
    if (!in_place) {
        INF_CHK(S.d_in.ensure(nwords * 4 + IN_PAD));
        if (in_len) INF_CHK(hipMemcpyAsync(S.d_in.p, in, in_len, in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        INF_CHK(hipMemsetAsync(S.d_in.as<char>() + in_len, 0, nwords * 4 + IN_PAD - in_len, s));
        *d_w = S.d_in.as<const uint32_t>();
    }
    return 0;
}

// ---- resolve rounds --------------------------------------------------------------------------------------
// The resolve lists of out[0, nbytes) (32-byte groups): list sizes, two group lists, round bits --
// the carve of S.d_rl -- and the first list filled from the pending bits.
struct ResolveLists {
    uint64_t npw = 0;
    uint32_t *cnt = nullptr, *lst[2] = {nullptr, nullptr}, *nb = nullptr;   // cnt[0], [1]: list sizes; [2], [3]: bytes (statistics)
};
static int resolve_lists(InflateScratch& S, hipStream_t s, uint64_t nbytes, ResolveLists& R) {
    R.npw = (nbytes + 31) / 32;
    if (R.npw == 0) return 0;
    if (R.npw > 0xFFFFFFFFull) return NDFL_E_UNSUPPORTED;          // u32 group indices
    INF_CHK(S.d_rl.ensure(R.npw * 12 + 64));
    R.cnt = S.d_rl.as<uint32_t>();
    R.lst[0] = (uint32_t*)(S.d_rl.as<char>() + 64);
    R.lst[1] = R.lst[0] + R.npw;
    R.nb = R.lst[1] + R.npw;
    INF_CHK(hipMemsetAsync(R.cnt, 0, 8, s));
    hipLaunchKernelGGL(ndfl_inflate_pending_list_kernel, dim3((uint32_t)((R.npw + 4095) / 4096)), dim3(256), 0, s,
                       S.d_pend.as<const uint32_t>(), (uint64_t)0, R.npw, R.lst[0], R.cnt);
    INF_CHK(hipGetLastError());
    return 0;
}
// One round from list `cur` into the other: follow the references, then apply and build the next list.
static int resolve_round(InflateScratch& S, hipStream_t s, const ResolveLists& R, int cur, uint8_t* d_out, uint32_t grid,
                         uint32_t apply_grid, bool rstats) {
    uint32_t* pend = S.d_pend.as<uint32_t>();
    INF_CHK(hipMemsetAsync(R.cnt + (cur ^ 1), 0, 4, s));
    if (rstats) INF_CHK(hipMemsetAsync(R.cnt + 2 + (cur ^ 1), 0, 4, s));
    hipLaunchKernelGGL(ndfl_inflate_resolve_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t*)R.lst[cur],
                       (const uint32_t*)(R.cnt + cur), (const uint32_t*)pend, S.d_ref.as<uint32_t>(), d_out, R.nb);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_resolve_apply_kernel, dim3(apply_grid), dim3(256), 0, s, (const uint32_t*)R.lst[cur],
                       (const uint32_t*)(R.cnt + cur), pend, (const uint32_t*)R.nb, R.lst[cur ^ 1], R.cnt + (cur ^ 1),
                       rstats ? R.cnt + 2 + (cur ^ 1) : (uint32_t*)nullptr);
    INF_CHK(hipGetLastError());
    return 0;
}

// Resolve the deferred copies of an emit pass: pointer-jumping rounds over the pending 32-byte
// groups of out[0, nbytes) until none is left.  *groups = pending groups at the start.
static int resolve_rounds(InflateScratch& S, hipStream_t s, uint8_t* d_out, uint64_t nbytes, uint64_t* groups) {
    *groups = 0;
    ResolveLists R;
    INF_RC(resolve_lists(S, s, nbytes, R));
    if (R.npw == 0) return 0;
    if (!S.h_cnt) INF_CHK(hipHostMalloc(&S.h_cnt, 64, 0));
    uint32_t* h = (uint32_t*)S.h_cnt;
    // rounds are queued four at a time on grid-stride kernels; the host reads the list size between
    // batches only (pointer jumping needs ~log2(reference depth) rounds)
    const bool rstats = S.knobs.stats;
    uint32_t n = 0;
    for (int round = 0, cur = 0;; round++, cur ^= 1) {
        if ((round & 3) == 0 || rstats) {
            INF_CHK(hipMemcpyAsync(h, R.cnt + cur, 4, hipMemcpyDeviceToHost, s));
            if (rstats) INF_CHK(hipMemcpyAsync(h + 1, R.cnt + 2 + cur, 4, hipMemcpyDeviceToHost, s));
            INF_CHK(hipStreamSynchronize(s));
            n = *h;
            if (rstats) fprintf(stderr, "[ndfl] resolve round %d: %u pending groups, %u bytes\n", round, n, h[1]);
            if (round == 0) *groups = n;
            if (n == 0) return 0;
            if (round >= 96) return inf::R_INTERNAL;         // distances double each round: unreachable
        }
        INF_RC(resolve_round(S, s, R, cur, d_out, (uint32_t)std::min<uint64_t>(4096, ((uint64_t)n * 32 + 255) / 256),
                             (uint32_t)std::min<uint64_t>(1024, (n + 255) / 256), rstats));
    }
}

// Queue `rounds` resolve rounds without reading anything back (the kernels read the list sizes on
// the device; a round with nothing pending costs two empty launches).  *left = where the size of the
// list left after them is (null: nothing to resolve); the first list's size also goes to *first_count_dst.
static int resolve_rounds_dev(InflateScratch& S, hipStream_t s, uint8_t* d_out, uint64_t nbytes, int rounds,
                              uint32_t** left, uint64_t* first_count_dst) {
    *left = nullptr;
    ResolveLists R;
    INF_RC(resolve_lists(S, s, nbytes, R));
    if (R.npw == 0) return 0;
    if (first_count_dst) INF_CHK(hipMemcpyAsync(first_count_dst, R.cnt, 4, hipMemcpyDeviceToDevice, s));
    for (int round = 0; round < rounds; round++) INF_RC(resolve_round(S, s, R, round & 1, d_out, 4096, 1024, false));
    *left = R.cnt + (rounds & 1);
    return 0;
}

// ---- one decode ------------------------------------------------------------------------------------------
static float event_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; hipEventElapsedTime(&ms, a, b); return ms; }
static double host_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// The survivor list held fewer than the scan found and can still grow: the next scan has room for all.
static bool survivors_overflowed(InflateScratch& S, uint32_t found) {
    if (found <= S.q_cap || S.q_full) return false;
    S.q_min = found + 65536;
    return true;
}

// One decode of a raw DEFLATE stream, or of the block-aligned range [start_bit, end_bit) of one.
//   out       the window start: out[0, dict_len) holds the dict_len bytes of output preceding the
//             range (0 for a whole stream); decoded bytes go to out[dict_len, dict_len + n)
//   deferred  the window content is not valid yet: chains that read it (directly or through other
//             chains) are recorded and re-emitted by inflate_resolve once it is written
struct Decode {
    InflateScratch& S;
    hipStream_t s;
    // the range, the output and the flags: set by the caller
    uint64_t start_bit = 0, end_bit = inf::NONE;
    uint8_t* out = nullptr;
    uint64_t dict_len = 0, out_cap = 0;
    uint32_t flags = 0;
    bool deferred = false, partial = false;
    // the results (*last_ms: the device linker's whole wall span, the host linker's emit + resolve)
    uint64_t out_len = 0, consumed_bits = 0;
    double* last_ms = nullptr;
    // the staged input
    const uint32_t* d_w = nullptr;
    uint64_t nwords = 0, nbits = 0;
    // the finder's per-segment lists (S.d_cand), the sorted candidate list's length (S.d_cands)
    uint32_t nseg = 0, ncand = 0;
    uint64_t* d_list = nullptr;
    uint32_t* d_cnt = nullptr;
    ChainLinks L;                                           // the host linker's chains
    // where the emit pass writes: the caller's buffer or S.d_out, nbytes with the window
    uint8_t* d_out = nullptr;
    uint64_t nbytes = 0;
    double ht[6] = {0, 0, 0, 0, 0, 0};                      // NDFL_HOST_TIMES

    bool direct() const { return (flags & NDFL_OUT_DEVICE) != 0; }
    uint32_t* stats_words() const { return S.knobs.stats ? S.d_stats.as<uint32_t>() : nullptr; }
    // the calls, and the stages they share
    int run(const uint8_t* in, uint64_t in_len);
    int sync_probe(const uint8_t* in, uint64_t in_len, uint64_t* sync_bit);
    int begin(const uint8_t* in, uint64_t in_len);
    int scan(bool timed), scanned(int (Decode::*stage)(bool may_rescan));
    int link(bool may_rescan), devlink(), hostlink(bool may_rescan), host_candidates(bool may_rescan);
    int setup_pool(uint64_t nstarts), count_scratch(uint64_t n, uint32_t** d_order);
    int count_chains(const std::vector<uint64_t>& st, uint64_t slot_base, std::vector<ChainRes>& r);
    int emit_scratch(uint64_t obytes), zero_tickets(), deliver(uint64_t produced);
    int launch_emit(uint32_t nch, uint32_t* tickets, const uint64_t* info, const uint32_t* order, const uint32_t* nslow);
    int print_count_stats(bool phase_clock_note), print_devlink_count(uint32_t n, bool flat_on);
};

// What every decode starts with: the pending state cleared, the input staged, the counters and events there.
int Decode::begin(const uint8_t* in, uint64_t in_len) {
    S.pending = false;
    ht[0] = host_ms();
    nbits = in_len * 8;
    nwords = (in_len + 3) / 4;
    if (start_bit > nbits) return NDFL_E_ARG;
    INF_RC(stage_input(S, s, in, in_len, flags, &d_w));
    INF_CHK(S.d_stats.ensure(512));
    if (!S.ev[0]) for (auto& e : S.ev) INF_CHK(hipEventCreate(&e));
    return 0;
}

// The header finder phase: every bit position of [start_bit, min(end_bit, nbits)) tested for a
// block header (finder: cheap masks + the code-length code's Kraft test), the survivors checked by
// the reference's own header rules (strict stage), the accepted ones into the per-segment lists
// d_list / d_cnt (SEG_BYTES of input each; the carve of S.d_cand).  Zeroes S.d_stats and d_cnt;
// S.ev[0] / S.ev[1] bracket a timed scan.
int Decode::scan(bool timed) {
    using namespace inf;
    INF_CHK(hipMemsetAsync(S.d_stats.p, 0, 512, s));
    nseg = (uint32_t)std::max<uint64_t>(1, (nbits / 8 + SEG_BYTES - 1) / SEG_BYTES);
    INF_CHK(S.d_cand.ensure((uint64_t)nseg * SEG_CAP * 8ull + (uint64_t)nseg * 4 + 64));
    d_list = S.d_cand.as<uint64_t>();
    d_cnt = (uint32_t*)(S.d_cand.as<char>() + (uint64_t)nseg * SEG_CAP * 8ull);
    INF_CHK(hipMemsetAsync(d_cnt, 0, (uint64_t)nseg * 4, s));
    if (timed) INF_CHK(hipEventRecord(S.ev[0], s));
    // only the range's own bits are scanned: candidates outside [start_bit, end_bit) are dropped
    // later anyway (a range decode of one stream shard, or a sync probe)
    const uint64_t scan_end = std::min(end_bit, nbits);
    const uint64_t w_lo = start_bit >> 5;
    const uint64_t nw32 = scan_end > w_lo * 32 ? (scan_end + 31) / 32 - w_lo : 0;
    // The survivor list: nbits / 256 + 64 K entries (about one survivor per 1,000 positions on real
    // streams).  A scan whose survivors overflowed it is run again with room for all of them
    // (survivors_overflowed, q_min), up to Q_BUDGET entries (1 GiB of list): periodic stored data can
    // pass the filters every ~32 bits, and a 4 GiB stream of it would ask for 8 GiB.  Past the budget, or
    // when the allocation fails, the decode goes on with the list it has (q_full): a survivor past
    // the list is a chain start not taken -- the chain before it decodes through that block -- so it
    // costs parallelism, never a result.
    constexpr uint64_t Q_BUDGET = (1ull << 30) / 8;
    const uint64_t qbase = std::min<uint64_t>(0x7FFFFFFFull, nbits / 256 + 65536);
    const uint64_t qtop = std::min<uint64_t>(0x7FFFFFFFull, std::max(qbase, Q_BUDGET));
    uint32_t qcap = (uint32_t)std::max(qbase, std::min<uint64_t>(S.q_min, qtop));
    S.q_full = qcap >= qtop;
    if (S.d_q.ensure((uint64_t)qcap * 8 + 64) != hipSuccess) {
        (void)hipGetLastError();                     // (an out-of-memory result is not a sticky error)
        qcap = (uint32_t)qbase;
        S.q_full = true;
        S.q_min = 0;
        INF_CHK(S.d_q.ensure((uint64_t)qcap * 8 + 64));
    }
    S.q_cap = qcap;
    uint32_t* d_qcount = S.d_stats.as<uint32_t>() + SW_QCOUNT;
    uint64_t* d_qlist = (uint64_t*)(S.d_q.as<char>() + 64);
    static const uint32_t strict_grid = [] {          // (no cap; 1280 when the runtime cannot say)
        const uint32_t g = occupancy_grid(ndfl_inflate_strict_kernel, 256, ~0u);
        return g == ~0u ? 1280u : g;
    }();
    unsigned long long* sst = S.knobs.stats ? (unsigned long long*)(S.d_stats.as<uint32_t>() + SW_STRICT64) : nullptr;
    if (nw32) {
        const uint32_t fgrid = (uint32_t)((nw32 + 256 * FIND_WPT - 1) / (256 * FIND_WPT));
        hipLaunchKernelGGL(ndfl_inflate_find_compact_kernel, dim3(fgrid), dim3(256), 0, s, d_w, nwords, nbits, d_qlist,
                           d_qcount, qcap, w_lo, scan_end);
        INF_CHK(hipGetLastError());
        hipLaunchKernelGGL(ndfl_inflate_strict_kernel, dim3(strict_grid), dim3(256), 0, s, d_w, nwords, nbits,
                           (const uint64_t*)d_qlist, (const uint32_t*)d_qcount, qcap, d_cnt, d_list,
                           S.d_stats.as<uint32_t>() + SW_STRICT_TICKET, sst);
        INF_CHK(hipGetLastError());
    }
    if (timed) INF_CHK(hipEventRecord(S.ev[1], s));
    return 0;
}

// Segment-record pool for `nstarts` chain starts (SegPool): the rounds of all chains, one head per
// counted chain start, with room for repairs, and the per-block table records.  The record counters
// live in S.d_stats, which a scan zeroes.
int Decode::setup_pool(uint64_t nstarts) {
    using namespace inf;
    const uint64_t nslot = nstarts + std::max<uint64_t>(4096, nstarts / 2);
    const uint64_t nrec = std::min<uint64_t>(0xFFFFFFF0ull, 2 * nstarts + nbits / (wv::MAX_SPAN / 2) + 65536);
    // table records: at most one per block; bounded (a stream of tiny blocks parses the rest again)
    const uint64_t nbt = std::min<uint64_t>(nrec, S.knobs.no_bt ? 0 : (1u << 18));
    INF_CHK(S.d_seg.ensure(nrec * (64 * 8 + 64 * 4 + sizeof(SegMeta)) + nslot * 4 + 64 + nbt * BT_BYTES));
    SegPool pool;
    pool.start = S.d_seg.as<uint64_t>();
    pool.cnt = (uint32_t*)(pool.start + nrec * 64);
    pool.meta = (SegMeta*)(pool.cnt + nrec * 64);
    pool.head = (uint32_t*)(pool.meta + nrec);
    pool.ctr = S.d_stats.as<uint32_t>() + SW_REC_CTR;
    pool.bctr = S.d_stats.as<uint32_t>() + SW_TREC_CTR;
    pool.nbt = (uint32_t)nbt;
    pool.bt = (TabRec*)(((uintptr_t)(pool.head + nslot) + 63) & ~(uintptr_t)63);
    pool.nrec = (uint32_t)nrec;
    pool.nslot = nslot;
    S.pool = pool;
    INF_CHK(hipMemsetAsync(pool.head, 0xFF, nslot * 4, s));
    return 0;
}

// The count pass's scratch for n chains: stops and, behind them, the claim order (S.d_stops), the
// results, the phase-fallback slots and the tickets (the caller zeroes what its launch uses of them).
int Decode::count_scratch(uint64_t n, uint32_t** d_order) {
    using namespace inf;
    INF_CHK(S.d_stops.ensure(n * 12));
    INF_CHK(S.d_res.ensure(n * sizeof(ChainRes)));
    INF_CHK(S.d_cticket.ensure(CTK_BYTES));
    INF_CHK(S.d_ph.ensure((size_t)std::max(COUNT_WAVES, EMIT_WAVES) * sizeof(wv::PhArr)));
    *d_order = (uint32_t*)(S.d_stops.as<char>() + n * 8);
    return 0;
}

// The emit pass's scratch for obytes of output, the window included: the output placed (the caller's
// device buffer, or S.d_out with the window copied in), a back-reference per byte, the pending bits
// zeroed.  NDFL_E_UNSUPPORTED past 32-bit group indices.  (The tickets: zero_tickets, which the host
// linker queues before it and the device linker after it.)
int Decode::emit_scratch(uint64_t obytes) {
    d_out = out;
    if (!direct()) {
        INF_CHK(S.d_out.ensure(obytes + 64));
        d_out = S.d_out.as<uint8_t>();
        if (dict_len) INF_CHK(hipMemcpyAsync(d_out, out, dict_len, hipMemcpyHostToDevice, s));
    }
    nbytes = obytes;
    const uint64_t npw = (nbytes + 31) / 32;
    if (npw > 0xFFFFFFFFull) return NDFL_E_UNSUPPORTED;      // u32 group indices in the resolve lists
    INF_CHK(S.d_ref.ensure(nbytes * 4 + 64));
    INF_CHK(S.d_pend.ensure(npw * 4 + 64));
    INF_CHK(hipMemsetAsync(S.d_pend.p, 0, npw * 4 + 64, s));
    return 0;
}
int Decode::zero_tickets() {
    INF_CHK(S.d_ticket.ensure(64));
    INF_CHK(hipMemsetAsync(S.d_ticket.p, 0, 64, s));
    return 0;
}

// The full emit pass over the nch chains of S.d_chains (`info`, `order` / `nslow`: the device
// linker's summary, claim order and the fast pass's left-over list; null on the host linker).
int Decode::launch_emit(uint32_t nch, uint32_t* tickets, const uint64_t* info, const uint32_t* order, const uint32_t* nslow) {
    static const uint32_t emit_grid = occupancy_grid(ndfl_inflate_emit_wave_kernel, 64, inf::EMIT_WAVES, "NDFL_EMIT_WPC");
    hipLaunchKernelGGL(ndfl_inflate_emit_wave_kernel, dim3(std::min<uint32_t>(nch, emit_grid)), dim3(64), 0, s, d_w,
                       nwords, nbits, S.d_chains.as<const EmitChain>(), nch, tickets, d_out, S.d_res.as<ChainRes>(),
                       S.d_cands.as<const uint64_t>(), ncand, S.d_ref.as<uint32_t>(), S.d_pend.as<uint32_t>(), S.pool,
                       S.d_ph.as<wv::PhArr>(), stats_words(), info, order, nslow);
    INF_CHK(hipGetLastError());
    return 0;
}

// The produced bytes back to a host caller.
int Decode::deliver(uint64_t produced) {
    if (!direct() && produced) INF_CHK(hipMemcpy(out + dict_len, d_out + dict_len, produced, hipMemcpyDeviceToHost));
    out_len = produced;
    return 0;
}

// ---- NDFL_STATS ----------------------------------------------------------------------------------------------
// The strict stage's counters and the count pass's wave clocks, from d_stats (both linkers print them)
int Decode::print_count_stats(bool phase_clock_note) {
    uint32_t st[64] = {0};
    INF_CHK(hipMemcpy(st, S.d_stats.p, 256, hipMemcpyDeviceToHost));
    const unsigned long long* ss = (const unsigned long long*)(st + SW_STRICT64);
    fprintf(stderr, "[ndfl] strict stage: %llu waves, %llu loop trips (%llu refills), %llu lane-symbol steps\n",
            ss[3], ss[0], ss[1], ss[2]);
    const uint64_t* t64 = (const uint64_t*)(st + SW_CLOCK64);
    fprintf(stderr, "[ndfl] count wave-time (ms x waves, 100 MHz clock%s): header %.1f spec %.1f "
            "verify %.1f phases %.1f serial %.1f record %.1f build %.1f phase-mapped %.1f\n",
            phase_clock_note ? "; -DNDFL_PHASE_CLOCK builds" : "", t64[0] * 1e-5,
            t64[1] * 1e-5, t64[2] * 1e-5, t64[3] * 1e-5, t64[4] * 1e-5, t64[5] * 1e-5, t64[6] * 1e-5, t64[7] * 1e-5);
    const double span = (double)(t64[9] - ~t64[10]);
    fprintf(stderr, "[ndfl] count waves %llu: busy %.1f ms x waves, span %.3f ms, occupancy %.3f, longest chain %.3f ms\n",
            (unsigned long long)t64[11], t64[8] * 1e-5, span * 1e-5, t64[11] ? t64[8] / (span * t64[11]) : 0.0,
            t64[12] * 1e-5);
    return 0;
}

// The device linker's count pass: its n chains by outcome (wave time in 10 us units), the flat groups,
// wave time against the chain's bits (the count order's key) per 32-Kibit bucket, and the longest chains
int Decode::print_devlink_count(uint32_t n, bool flat_on) {
    using namespace inf;
    std::vector<ChainRes> cr(n);
    INF_CHK(hipMemcpyAsync(cr.data(), S.d_res.p, n * sizeof(ChainRes), hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    uint64_t cnt[3] = {0, 0, 0}, tsum[3] = {0, 0, 0}, tmax[3] = {0, 0, 0}, blk[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t st = std::min<uint32_t>(cr[k].status, 2u), t = cr[k].pad >> 16;
        cnt[st]++; tsum[st] += t; tmax[st] = std::max<uint64_t>(tmax[st], t); blk[st] += cr[k].pad & 0xFFFFu;
    }
    if (flat_on) {
        uint32_t fw[CT_ORDER] = {0};
        INF_CHK(hipMemcpy(fw, S.d_cticket.p, sizeof(fw), hipMemcpyDeviceToHost));
        const uint32_t* why = fw + CT_FLAT_WHY;
        fprintf(stderr, "[ndfl] count flat groups sent back: (unused) %u, full-table tokens %u, "
                "error %u, chain goes on %u, table %u\n", why[1], why[2], why[3], why[4], why[5]);
        const uint32_t nfl = fw[CT_NFLAT];
        const unsigned long long gt = (unsigned long long)fw[CT_FLAT_TIME64] | ((unsigned long long)fw[CT_FLAT_TIME64 + 1] << 32);
        fprintf(stderr, "[ndfl] count flat groups: %u chains in %u groups, %u sent back to the wave decode, "
                "group wave time %.3f ms mean\n", nfl, (nfl + 63) / 64, fw[CT_FLAT_REDO], nfl ? gt * 1e-5 / ((nfl + 63) / 64) : 0.0);
#ifdef NDFL_FLAT_PROF
        unsigned long long fpv[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0};
        INF_CHK(hipMemcpyFromSymbol(fpv, HIP_SYMBOL(wv::g_flat_prof), 32));
        INF_CHK(hipMemcpyToSymbol(HIP_SYMBOL(wv::g_flat_prof), z, 32));
        fprintf(stderr, "[ndfl] flat decode loops (lane 0, clock64): %llu cycles, %llu at %llu phase points\n", fpv[0], fpv[1], fpv[2]);
#endif
    }
    const char* nm[3] = {"boundary", "final", "error"};
    for (int k = 0; k < 3; k++)
        fprintf(stderr, "[ndfl] count chains %s: %llu, wave time %.2f ms (max %.3f ms), blocks %llu\n", nm[k],
                (unsigned long long)cnt[k], tsum[k] * 1e-2, tmax[k] * 1e-2, (unsigned long long)blk[k]);
    std::vector<uint64_t> cb(n);
    INF_CHK(hipMemcpy(cb.data(), S.d_cands.p, n * 8, hipMemcpyDeviceToHost));
    uint64_t bn[OB_NB] = {}, bt[OB_NB] = {}, bm[OB_NB] = {};
    uint32_t bk[OB_NB] = {};
    std::vector<uint32_t> top;
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t nx = k + 1 < n ? cb[k + 1] : end_bit, len = nx > cb[k] ? nx - cb[k] : 0;
        const uint32_t b = (uint32_t)std::min<uint64_t>(OB_NB - 1, len >> 15), t = cr[k].pad >> 16;
        bn[b]++; bt[b] += t;
        if (t >= bm[b]) { bm[b] = t; bk[b] = k; }
        top.push_back(k);
    }
    for (uint32_t b = 0; b < OB_NB; b++)
        if (bn[b]) fprintf(stderr, "[ndfl] count bits %2u x 32Ki: %6llu chains, mean %.3f ms, max %.3f ms "
                           "(chain %u at bit %llu: blocks %u, status %u, out %llu)\n", b,
                           (unsigned long long)bn[b], bt[b] * 1e-2 / bn[b], bm[b] * 1e-2, bk[b],
                           (unsigned long long)cb[bk[b]], cr[bk[b]].pad & 0xFFFFu, cr[bk[b]].status,
                           (unsigned long long)cr[bk[b]].out_count);
    const size_t nt = std::min<size_t>(8, top.size());
    std::partial_sort(top.begin(), top.begin() + nt, top.end(),
                      [&](uint32_t a, uint32_t b) { return (cr[a].pad >> 16) > (cr[b].pad >> 16); });
    for (size_t i = 0; i < nt; i++) {
        const uint32_t k = top[i];
        const uint64_t nx = k + 1 < n ? cb[k + 1] : end_bit;
        fprintf(stderr, "[ndfl] count longest: chain %u at bit %llu, %llu bits, %.3f ms, blocks %u, status %u, out %llu\n",
                k, (unsigned long long)cb[k], (unsigned long long)(nx - cb[k]), (cr[k].pad >> 16) * 1e-2,
                cr[k].pad & 0xFFFFu, cr[k].status, (unsigned long long)cr[k].out_count);
    }
    return 0;
}

// The host linker's most expensive chains (wave time, blocks, bits, output bytes)
static void print_top_chains(const ChainLinks& L) {
    std::vector<size_t> idx(L.res.size());
    for (size_t k = 0; k < idx.size(); k++) idx[k] = k;
    const size_t top = std::min<size_t>(8, idx.size());
    std::partial_sort(idx.begin(), idx.begin() + top, idx.end(),
                      [&](size_t a, size_t b) { return (L.res[a].pad >> 16) > (L.res[b].pad >> 16); });
    for (size_t t = 0; t < top; t++) {
        const ChainRes& r = L.res[idx[t]];
        fprintf(stderr, "[ndfl] count chain %zu: %.2f ms, %u blocks, start %llu, %llu bits, %llu bytes, status %u\n",
                idx[t], (r.pad >> 16) * 0.01, r.pad & 0xFFFFu, (unsigned long long)L.starts[idx[t]],
                (unsigned long long)(r.end_bit - L.starts[idx[t]]), (unsigned long long)r.out_count, r.status);
    }
}

// ---- the device linker ----------------------------------------------------------------------------------
// The decode after the header finder with everything on the device and ONE host synchronization
// in the middle (the number of chain starts, which sizes the record pool and the grids) and one at
// the end (the summary): candidate list (segment scan, compaction, the range's slice), the count
// pass in longest-first order, chain linking by pointer jumping, the emit pass, the first error,
// the resolve rounds.  Returns LINK_FALLBACK when the host's linking has to step in (a chain that
// stopped at a boundary that is no candidate; a list of chain starts too long for the jump tables, or
// none; an output bound past the scratch limits) -- the host linker then starts over from the
// finder's lists -- and FIND_OVERFLOW when the finder's survivor list was too short.
int Decode::devlink() {
    using namespace inf;
    INF_CHK(S.d_info.ensure(LI_WORDS * 8));
    if (!S.h_info) INF_CHK(hipHostMalloc(&S.h_info, LI_WORDS * 8, 0));
    uint64_t* info = S.d_info.as<uint64_t>();
    volatile uint64_t* hinfo = (volatile uint64_t*)S.h_info;
    INF_CHK(hipMemsetAsync(info, 0, LI_WORDS * 8, s));
    const uint64_t cap_all = (uint64_t)nseg * SEG_CAP + 1;      // the sorted list's length at most
    const uint32_t ntile = (nseg + SCAN_TILE - 1) / SCAN_TILE;
    INF_CHK(S.d_starts.ensure((cap_all + nseg + 2 + ntile) * 8));
    uint64_t* d_sorted = S.d_starts.as<uint64_t>();
    uint64_t* d_segoff = d_sorted + cap_all;
    uint64_t* d_part = d_segoff + nseg + 2;
    hipLaunchKernelGGL(ndfl_inflate_segsum_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint32_t*)d_cnt, nseg, d_part);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_segscan_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint32_t*)d_cnt, nseg, d_segoff,
                       info, (const uint64_t*)d_part);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_compact_kernel, dim3((nseg + 3) / 4), dim3(256), 0, s, (const uint32_t*)d_cnt,
                       (const uint64_t*)d_list, (const uint64_t*)d_segoff, nseg, d_sorted);
    INF_CHK(hipGetLastError());
    INF_CHK(S.d_cands.ensure((cap_all + 1) * 8ull));
    const uint64_t* d_cands = S.d_cands.as<const uint64_t>();
    hipLaunchKernelGGL(ndfl_inflate_cand_slice_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (cap_all + 255) / 256)),
                       dim3(256), 0, s, (const uint64_t*)d_sorted, info, start_bit, end_bit, S.d_cands.as<uint64_t>());
    INF_CHK(hipGetLastError());
    // stored-header aliases counted once (NDFL_NO_ALIAS: every candidate counted)
    const bool alias_on = !S.knobs.no_alias;
    uint32_t* d_rep = nullptr;
    if (alias_on) {
        INF_CHK(S.d_rep.ensure((size_t)cap_all * 4 + 64));
        d_rep = S.d_rep.as<uint32_t>();
        hipLaunchKernelGGL(ndfl_inflate_alias_mark_kernel, dim3((uint32_t)std::min<uint64_t>(1024, (cap_all + 255) / 256)),
                           dim3(256), 0, s, d_cands, info, d_w, nwords, nbits, d_rep);
        INF_CHK(hipGetLastError());
    }
    INF_CHK(hipMemcpyAsync((void*)hinfo, info, (LI_NREP + 1) * 8, hipMemcpyDeviceToHost, s));
    hinfo[LI_QCOUNT] = 0;
    INF_CHK(hipMemcpyAsync((void*)(hinfo + LI_QCOUNT), S.d_stats.as<const uint32_t>() + SW_QCOUNT, 4, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));                          // (1) the number of chain starts
    if (survivors_overflowed(S, (uint32_t)hinfo[LI_QCOUNT])) return FIND_OVERFLOW;
    const uint64_t n = hinfo[LI_NCAND];
    // the count pass's width: one wave per chain, unless the chains to count are few against the
    // count waves (fewer than 2 per wave), where a chain's rounds in sequence bound the pass (config
    // 2: 3,286 chains, ~1.1 per wave: 4 waves per chain count it in 2.0 ms instead of 4.0; one rank's
    // 512 MiB share of the bench at 8 GPUs: 8,191 chains, ~2.7 per wave: one wave each, 2.1 ms
    // instead of 3.1 -- profiles/r05_shard_count_width.txt; the bench's 66,770 chains: one wave
    // each) -- NDFL_COUNT_W overrides
    const uint64_t nrep = alias_on ? hinfo[LI_NREP] : n;
    const uint32_t W = S.knobs.count_w ? count_w(S.knobs) : (nrep < 2ull * count_wave_grid() && nbits >= (1ull << 24)) ? 4u : 1u;
    if (S.knobs.stats) fprintf(stderr, "[ndfl] count pass: %llu candidates, %llu counted, width %u\n",
                                      (unsigned long long)n, (unsigned long long)nrep, W);
    if (n == 0 || n > (1ull << 24)) return LINK_FALLBACK;
    ncand = (uint32_t)n;
    INF_RC(setup_pool(n));
    // count pass, longest chains first
    uint32_t* d_order = nullptr;
    INF_RC(count_scratch(n, &d_order));
    uint32_t* ctk = S.d_cticket.as<uint32_t>();
    INF_CHK(hipMemsetAsync(ctk, 0, CTK_BYTES, s));
    uint32_t *d_nord = ctk + CT_NORD, *d_nflat = ctk + CT_NFLAT;
    uint32_t* d_ob = ctk + CT_ORDER;                            // count order: tot, cursor
    const uint32_t otiles = (ncand + SCAN_TILE - 1) / SCAN_TILE;
    const bool stats_on = S.knobs.stats;
    const uint64_t limit = std::min(end_bit, nbits);
    INF_CHK(hipEventRecord(S.ev[2], s));
    // header records, and the chains whose first block is counted by one lane (flat groups: the
    // one-wave count kernel only); those leave the count order
    const bool hrec_on = !S.knobs.no_hdrrec;
    // (a flat group decodes its 64 blocks one lane each: ~7 ms of latency however few the chains, so
    // only a pass long enough to hide it takes them -- the bench's 66,770 chains; one rank's 8,191 at
    // 8 GPUs counts its incompressible blocks in wave form, by escape scans)
    const bool flat_on = hrec_on && W == 1 && S.knobs.flat && nrep >= S.knobs.flat_min;
    uint32_t *d_flist = nullptr, *d_fflag = nullptr;
    if (hrec_on) {
        INF_CHK(S.d_hrec.ensure((size_t)ncand * (sizeof(wv::HdrRec) + 8) + 64));
        d_flist = (uint32_t*)(S.d_hrec.as<char>() + (size_t)ncand * sizeof(wv::HdrRec));
        d_fflag = d_flist + ncand;
        hipLaunchKernelGGL(ndfl_inflate_hdr_kernel, dim3((ncand + 63) / 64), dim3(64), 0, s, d_w, nwords, nbits, d_cands,
                           ncand, S.d_hrec.as<wv::HdrRec>(), flat_on ? d_flist : nullptr, d_nflat, flat_on ? d_fflag : nullptr);
        INF_CHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ndfl_inflate_order_count_kernel, dim3(otiles), dim3(SCAN_T), 0, s, d_cands, ncand, end_bit,
                       (const uint32_t*)d_rep, d_ob, flat_on ? (const uint32_t*)d_fflag : nullptr);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_order_kernel, dim3(otiles), dim3(SCAN_T), 0, s, d_cands, ncand, end_bit, d_order,
                       (const uint32_t*)d_rep, (alias_on || flat_on) ? d_nord : (uint32_t*)nullptr, d_ob,
                       flat_on ? (const uint32_t*)d_fflag : nullptr);
    INF_CHK(hipGetLastError());
    if (flat_on) INF_CHK(hipMemcpyAsync(info + LI_NFLAT, d_nflat, 4, hipMemcpyDeviceToDevice, s));
    launch_count(s, W, ncand, d_w, nwords, nbits, d_cands, (const uint64_t*)nullptr, ncand, d_cands, ncand, limit,
                 S.d_res.as<ChainRes>(), stats_words(), (uint64_t)0, S.pool, ctk, S.d_ph.as<wv::PhArr>(),
                 (const uint32_t*)d_order, end_bit, hrec_on ? S.d_hrec.as<const wv::HdrRec>() : nullptr,
                 (alias_on || flat_on) ? (const uint32_t*)d_nord : nullptr, flat_on ? (const uint32_t*)d_flist : nullptr,
                 flat_on ? (const uint32_t*)d_nflat : nullptr);
    INF_CHK(hipGetLastError());
    if (alias_on) {
        hipLaunchKernelGGL(ndfl_inflate_alias_copy_kernel, dim3(std::min<uint32_t>(1024, (ncand + 255) / 256)), dim3(256), 0, s,
                           (const uint32_t*)d_rep, ncand, S.d_res.as<ChainRes>(), S.pool);
        INF_CHK(hipGetLastError());
    }
    INF_CHK(hipEventRecord(S.ev[3], s));
    if (stats_on) INF_RC(print_devlink_count(ncand, flat_on));
    // linking: J levels (u32), S and D double-buffered
    uint32_t nlev = 1;
    while ((1ull << nlev) < n) nlev++;
    INF_CHK(S.d_link.ensure((size_t)(nlev + 1) * n * 4 + 2 * n * 8 + 2 * n * 4 + 64));
    uint32_t* J = S.d_link.as<uint32_t>();
    uint64_t* Ssum[2] = {(uint64_t*)(((uintptr_t)(J + (size_t)(nlev + 1) * n) + 7) & ~(uintptr_t)7), nullptr};
    Ssum[1] = Ssum[0] + n;
    uint32_t* Dd[2] = {(uint32_t*)(Ssum[1] + n), nullptr};
    Dd[1] = Dd[0] + n;
    const uint32_t lg = (uint32_t)std::min<uint64_t>(4096, (n + 255) / 256);
    hipLaunchKernelGGL(ndfl_inflate_link_init_kernel, dim3(lg), dim3(256), 0, s, S.d_res.as<const ChainRes>(), ncand, d_cands,
                       end_bit, J, Ssum[0], Dd[0]);
    INF_CHK(hipGetLastError());
    int cur = 0;
    for (uint32_t r = 0; r < nlev; r++) {
        hipLaunchKernelGGL(ndfl_inflate_link_jump_kernel, dim3(lg), dim3(256), 0, s, (const uint32_t*)(J + (size_t)r * n),
                           J + (size_t)(r + 1) * n, (const uint64_t*)Ssum[cur], Ssum[cur ^ 1], (const uint32_t*)Dd[cur],
                           Dd[cur ^ 1], ncand);
        INF_CHK(hipGetLastError());
        cur ^= 1;
    }
    INF_CHK(S.d_chains.ensure(n * sizeof(EmitChain)));
    const EmitChain* d_chains = S.d_chains.as<const EmitChain>();
    hipLaunchKernelGGL(ndfl_inflate_link_path_kernel, dim3(lg), dim3(256), 0, s, (const uint32_t*)J, nlev,
                       (const uint64_t*)Ssum[cur], (const uint32_t*)Dd[cur], S.d_res.as<const ChainRes>(), d_cands, ncand,
                       dict_len, end_bit, out_cap, S.d_chains.as<EmitChain>(), info);
    INF_CHK(hipGetLastError());
    // the emit pass claims the linked chains costliest first (the count pass's order buffer is free)
    uint32_t* d_eob = ctk + CT_ORDER + OB_WORDS;                // emit order: tot, cursor (zeroed above)
    hipLaunchKernelGGL(ndfl_inflate_emit_order_count_kernel, dim3(otiles), dim3(SCAN_T), 0, s, d_chains,    // (chains <= candidates)
                       (const uint64_t*)info, d_eob);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_emit_order_kernel, dim3(otiles), dim3(SCAN_T), 0, s, d_chains, (const uint64_t*)info,
                       d_order, d_eob);
    INF_CHK(hipGetLastError());
    // the output's size is known on the device only: the scratch (back-references, pending bits,
    // a staging copy) is sized by out_cap, capped at DEFLATE's largest expansion (258 bytes per 2 bits)
    const uint64_t obytes = dict_len + std::min<uint64_t>(out_cap, 129 * nbits + 65536);
    if (obytes > (40ull << 30)) return LINK_FALLBACK;          // (the host linker sizes it exactly)
    if (const int rc = emit_scratch(obytes)) return rc == NDFL_E_UNSUPPORTED ? LINK_FALLBACK : rc;
    INF_RC(zero_tickets());
    if (S.knobs.test_segflip && S.pool.cnt) {         // (test: record 0, lane 0 counts one byte more)
        uint32_t c0 = 0;
        INF_CHK(hipMemcpyAsync(&c0, S.pool.cnt, 4, hipMemcpyDeviceToHost, s));
        INF_CHK(hipStreamSynchronize(s));
        c0++;
        INF_CHK(hipMemcpyAsync(S.pool.cnt, &c0, 4, hipMemcpyHostToDevice, s));
        INF_CHK(hipStreamSynchronize(s));
    }
    INF_CHK(hipEventRecord(S.ev[4], s));
    // the record-replay emit kernel first, the full one over what it leaves (NDFL_EMIT_FAST=0: the
    // full one alone)
    uint32_t* tk = S.d_ticket.as<uint32_t>();                   // [0] fast tickets, [4] full tickets, [8] slow count
    if (S.knobs.emit_fast) {
        INF_CHK(S.d_slow.ensure((size_t)ncand * 4 + 64));
        static const uint32_t fast_grid = occupancy_grid(ndfl_inflate_emit_fast_kernel, 64, EMIT_WAVES, "NDFL_EMITF_WPC");
        hipLaunchKernelGGL(ndfl_inflate_emit_fast_kernel, dim3(std::min<uint32_t>(ncand, fast_grid)), dim3(64), 0, s, d_w,
                           nwords, nbits, d_chains, tk, d_out, S.d_res.as<ChainRes>(), S.d_ref.as<uint32_t>(),
                           S.d_pend.as<uint32_t>(), S.pool, (const uint64_t*)info, (const uint32_t*)d_order,
                           S.d_slow.as<uint32_t>(), tk + 8);
        INF_CHK(hipGetLastError());
        INF_RC(launch_emit(ncand, tk + 4, info, S.d_slow.as<const uint32_t>(), tk + 8));
        if (stats_on) {
            uint32_t nsl = 0;
            INF_CHK(hipMemcpyAsync(&nsl, tk + 8, 4, hipMemcpyDeviceToHost, s));
            INF_CHK(hipStreamSynchronize(s));
            fprintf(stderr, "[ndfl] fast emit pass left %u chains to the full emit pass\n", nsl);
        }
    } else {
        INF_RC(launch_emit(ncand, tk, info, d_order, nullptr));
    }
    INF_CHK(hipEventRecord(S.ev[5], s));
    uint32_t* d_first = ctk + CT_ORDER + 2 * OB_WORDS;
    INF_CHK(hipMemsetAsync(d_first, 0xFF, 4, s));
    hipLaunchKernelGGL(ndfl_inflate_first_error_kernel, dim3(otiles), dim3(SCAN_T), 0, s, S.d_res.as<const ChainRes>(),
                       (const uint64_t*)info, d_first);
    INF_CHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_inflate_summary_kernel, dim3(1), dim3(64), 0, s, S.d_res.as<const ChainRes>(), d_chains, info,
                       dict_len, partial ? 1u : 0u, (const uint32_t*)d_first);
    INF_CHK(hipGetLastError());
    // the resolve rounds, as far as they usually go, without a host read in between
    if (!deferred) {
        uint32_t* left = nullptr;
        INF_RC(resolve_rounds_dev(S, s, d_out, nbytes, 6, &left, stats_on ? info + LI_WORDS - 3 : (uint64_t*)nullptr));
        if (left) INF_CHK(hipMemcpyAsync(info + LI_WORDS - 1, left, 4, hipMemcpyDeviceToDevice, s));
    }
    INF_CHK(hipMemcpyAsync((void*)hinfo, info, LI_WORDS * 8, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));                          // (2) the summary
    if (stats_on) {
        uint32_t st[3] = {0, 0, 0};
        INF_CHK(hipMemcpy(st, S.d_stats.p, sizeof(st), hipMemcpyDeviceToHost));
        fprintf(stderr, "[ndfl] device link: chains %llu of %u candidates; count pass: slow-verify lanes %u fixups %u "
                "rounds %u\n", (unsigned long long)hinfo[LI_NCH], ncand, st[SW_NSLOW], st[SW_NFIX], st[SW_NROUND]);
        fprintf(stderr, "[ndfl] emit: %u pending 32-byte groups before the resolve rounds, %u after six\n",
                (uint32_t)(hinfo[LI_WORDS - 3] & 0xFFFFFFFFu), (uint32_t)(hinfo[LI_WORDS - 1] & 0xFFFFFFFFu));
        INF_RC(print_count_stats(true));
    }
    const uint64_t lflags = hinfo[LI_FLAGS];
    if (lflags & LF_REPAIR) return LINK_FALLBACK;
    if (lflags & LF_RANGE) return NDFL_E_ARG;                  // the range end is no block boundary
    S.chains = hinfo[LI_NCH];
    S.candidates = ncand;
    S.flat_chains = hinfo[LI_NFLAT];
    S.repairs = 0;
    if (lflags & LF_CAPACITY) { out_len = hinfo[LI_TOTAL]; return NDFL_E_CAPACITY; }
    const uint32_t pending_left = (uint32_t)(hinfo[LI_WORDS - 1] & 0xFFFFFFFFu);
    S.pending_after_dev = deferred ? 0 : pending_left;
    if (!deferred && pending_left) {
        uint64_t groups = 0;
        INF_RC(resolve_rounds(S, s, d_out, nbytes, &groups));  // (the rest, with the host's checks)
    }
    S.last_ms_find = event_ms(S.ev[0], S.ev[1]);
    S.last_ms_count = event_ms(S.ev[2], S.ev[3]);
    S.last_ms_emit = event_ms(S.ev[4], S.ev[5]);
    if (deferred) { S.pending = true; S.p_out = d_out; S.p_nbytes = dict_len + hinfo[LI_TOTAL]; S.p_dict_len = dict_len; }
    INF_CHK(hipEventRecord(S.ev[5], s));
    INF_CHK(hipStreamSynchronize(s));
    *last_ms = S.last_ms_wall = event_ms(S.ev[0], S.ev[5]);
    INF_RC(deliver(hinfo[LI_OUTLEN]));
    consumed_bits = hinfo[LI_CONSUMED];
    return (int)hinfo[LI_CODE];
}

// ---- the host linker ----------------------------------------------------------------------------------------
// The finder's lists (already on the device) as the range's sorted candidate list, on the host
// (L.starts) and on the device (S.d_cands, ncand), and the record pool for it.  FIND_OVERFLOW (only
// when may_rescan): the survivor list was too short.
int Decode::host_candidates(bool may_rescan) {
    using namespace inf;
    std::vector<uint64_t>& starts = L.starts;
    std::vector<uint32_t> hcnt(nseg);
    uint32_t hqc = 0;
    INF_CHK(hipMemcpyAsync(hcnt.data(), d_cnt, nseg * 4ull, hipMemcpyDeviceToHost, s));
    INF_CHK(hipMemcpyAsync(&hqc, S.d_stats.as<const uint32_t>() + SW_QCOUNT, 4, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    if (may_rescan && survivors_overflowed(S, hqc)) return FIND_OVERFLOW;
    std::vector<uint64_t> hoff(nseg + 1);
    hoff[0] = 1;                                   // slot 0 is the range start
    for (uint32_t k = 0; k < nseg; k++) hoff[k + 1] = hoff[k] + std::min(hcnt[k], SEG_CAP);
    const uint64_t ncand_all = hoff[nseg];
    INF_CHK(S.d_starts.ensure((ncand_all + nseg + 2) * 8));
    uint64_t* d_sorted = S.d_starts.as<uint64_t>();
    uint64_t* d_segoff = d_sorted + ncand_all;
    INF_CHK(hipMemcpyAsync(d_segoff, hoff.data(), nseg * 8ull, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ndfl_inflate_compact_kernel, dim3((nseg + 3) / 4), dim3(256), 0, s, (const uint32_t*)d_cnt,
                       (const uint64_t*)d_list, (const uint64_t*)d_segoff, nseg, d_sorted);
    INF_CHK(hipGetLastError());
    starts.resize(ncand_all);
    INF_CHK(hipMemcpyAsync(starts.data() + 1, d_sorted + 1, (ncand_all - 1) * 8, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    filter_range(starts, start_bit, end_bit);
    // the sorted candidate list on the device: the wave passes split block data at the next one
    ncand = (uint32_t)starts.size();
    INF_CHK(S.d_cands.ensure((ncand + 1) * 8ull));
    INF_CHK(hipMemcpyAsync(S.d_cands.p, starts.data(), ncand * 8ull, hipMemcpyHostToDevice, s));
    // segment records: one head per counted chain start (index in `starts`)
    INF_RC(setup_pool(starts.size()));
    ht[1] = host_ms();
    S.repairs = 0;
    S.count_first = true;
    return 0;
}

// One count launch over the chain starts `st` (record slots from slot_base on), results into r.
// S.ev[2] / S.ev[3] bracket a decode's first one (count_first).
int Decode::count_chains(const std::vector<uint64_t>& st, uint64_t slot_base, std::vector<ChainRes>& r) {
    const size_t n = st.size();
    const std::vector<uint64_t> sp(n, end_bit);             // chains stop at exact candidates (kernel)
    const std::vector<uint32_t> order = count_order(st, end_bit);
    uint32_t* d_order = nullptr;
    INF_CHK(S.d_starts.ensure(n * 8));
    INF_RC(count_scratch(n, &d_order));
    INF_CHK(hipMemcpyAsync(S.d_starts.p, st.data(), n * 8, hipMemcpyHostToDevice, s));
    INF_CHK(hipMemcpyAsync(S.d_stops.p, sp.data(), n * 8, hipMemcpyHostToDevice, s));
    INF_CHK(hipMemcpyAsync(d_order, order.data(), n * 4, hipMemcpyHostToDevice, s));
    INF_CHK(hipMemsetAsync(S.d_cticket.p, 0, 4, s));
    if (S.count_first) INF_CHK(hipEventRecord(S.ev[2], s));
    launch_count(s, count_w(S.knobs), (uint32_t)n, d_w, nwords, nbits, S.d_starts.as<const uint64_t>(),
                 S.d_stops.as<const uint64_t>(), (uint32_t)n, S.d_cands.as<const uint64_t>(), ncand, std::min(end_bit, nbits),
                 S.d_res.as<ChainRes>(), stats_words(), slot_base, S.pool, S.d_cticket.as<uint32_t>(), S.d_ph.as<wv::PhArr>(),
                 (const uint32_t*)d_order, end_bit, (const wv::HdrRec*)nullptr, (const uint32_t*)nullptr,
                 (const uint32_t*)nullptr, (const uint32_t*)nullptr);
    INF_CHK(hipGetLastError());
    if (S.count_first) { INF_CHK(hipEventRecord(S.ev[3], s)); S.count_first = false; }
    r.resize(n);
    INF_CHK(hipMemcpyAsync(r.data(), S.d_res.p, n * sizeof(ChainRes), hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    return 0;
}

// The decode after the header finder with the host's linking (NDFL_HOST_LINK, or a hand-over of the
// device linker): the candidate list, one count launch over it, up to eight parallel rounds that
// count the boundaries that are no candidates (a final serial fallback guarantees progress), the
// walk from the range start, the emit pass, the resolve rounds paced by the host.
int Decode::hostlink(bool may_rescan) {
    using namespace inf;
    L = ChainLinks{};
    L.end_bit = end_bit; L.dict_len = dict_len;
    INF_RC(host_candidates(may_rescan));
    L.n0 = L.starts.size();
    INF_RC(count_chains(L.starts, 0, L.res));
    const bool stats_on = S.knobs.stats;
    if (stats_on) print_top_chains(L);
    S.last_ms_find = event_ms(S.ev[0], S.ev[1]);
    S.last_ms_count = event_ms(S.ev[2], S.ev[3]);
    for (int round = 0; round < 8; round++) {
        const std::vector<uint64_t> todo = L.repair_todo();
        if (todo.empty()) break;
        std::vector<ChainRes> r2;
        INF_RC(count_chains(todo, L.starts.size(), r2));
        L.add(todo, r2);
        S.repairs += todo.size();
    }
    ht[2] = host_ms();
    for (uint64_t need = 0;;) {
        const int rc = L.walk(&need);
        if (rc != WALK_COUNT) { INF_RC(rc); break; }
        std::vector<ChainRes> r1;                    // serial fallback (beyond the parallel rounds)
        INF_RC(count_chains({need}, L.starts.size(), r1));
        L.add({need}, r1);
        L.cur = L.starts.size() - 1;
        S.repairs++;
    }
    S.chains = L.chains.size();
    S.flat_chains = 0;
    S.candidates = L.n0;
    if (stats_on) {
        uint32_t st[SW_QCOUNT + 1] = {0};
        INF_CHK(hipMemcpy(st, S.d_stats.p, sizeof(st), hipMemcpyDeviceToHost));
        fprintf(stderr, "[ndfl] finder quick survivors %u; count pass: chains %zu candidates %zu repairs %llu "
                "slow-verify lanes %u fixups %u rounds %u\n", st[SW_QCOUNT], L.chains.size(), L.n0,
                (unsigned long long)S.repairs, st[SW_NSLOW], st[SW_NFIX], st[SW_NROUND]);
        INF_RC(print_count_stats(false));
    }
    const uint64_t total = L.produced;
    ht[3] = host_ms();
    if (total > out_cap) { out_len = total; return NDFL_E_CAPACITY; }

    // emit pass
    const uint32_t nch = (uint32_t)L.chains.size();
    INF_CHK(S.d_chains.ensure(nch * sizeof(EmitChain)));
    INF_CHK(S.d_res.ensure(nch * sizeof(ChainRes)));
    INF_CHK(hipMemcpyAsync(S.d_chains.p, L.chains.data(), nch * sizeof(EmitChain), hipMemcpyHostToDevice, s));
    INF_RC(zero_tickets());
    INF_RC(emit_scratch(dict_len + total));
    INF_CHK(hipEventRecord(S.ev[4], s));
    INF_RC(launch_emit(nch, S.d_ticket.as<uint32_t>(), nullptr, nullptr, nullptr));
    INF_CHK(hipEventRecord(S.ev[5], s));
    std::vector<ChainRes> er(nch);
    INF_CHK(hipMemcpyAsync(er.data(), S.d_res.p, nch * sizeof(ChainRes), hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    ht[4] = host_ms();
    S.last_ms_emit = event_ms(S.ev[4], S.ev[5]);
    if (stats_on) {
        uint64_t t64[48];
        INF_CHK(hipMemcpy(t64, S.d_stats.as<const uint32_t>() + SW_CLOCK64, sizeof(t64), hipMemcpyDeviceToHost));
        const double span = (double)(t64[17] - ~t64[18]);
        fprintf(stderr, "[ndfl] emit waves %llu: busy %.1f ms x waves, span %.3f ms, occupancy %.3f, longest chain %.3f ms\n",
                (unsigned long long)t64[19], t64[16] * 1e-5, span * 1e-5, t64[19] ? t64[16] / (span * t64[19]) : 0.0,
                t64[20] * 1e-5);
    }
    if (deferred) {
        S.pending = true;
        S.p_out = d_out; S.p_nbytes = nbytes; S.p_dict_len = dict_len;
    } else {
        uint64_t groups = 0;
        INF_RC(resolve_rounds(S, s, d_out, nbytes, &groups));
        S.resolved_groups = groups;
    }
    INF_CHK(hipEventRecord(S.ev[5], s));
    INF_CHK(hipStreamSynchronize(s));
    S.last_ms_wall = event_ms(S.ev[0], S.ev[5]);
    *last_ms = event_ms(S.ev[4], S.ev[5]);
    ht[5] = host_ms();
    if (S.knobs.host_times)
        fprintf(stderr, "[ndfl] inflate host ms: finder+starts %.2f count+repairs %.2f link %.2f emit %.2f resolve %.2f\n",
                ht[1] - ht[0], ht[2] - ht[1], ht[3] - ht[2], ht[4] - ht[3], ht[5] - ht[4]);
    const Outcome o = first_error(er, L.chains, dict_len, partial, total, L.stop_bit);
    INF_RC(deliver(o.produced));
    consumed_bits = o.consumed_bits;
    return o.code;
}

// ---- the calls ---------------------------------------------------------------------------------------------
// The linkers after a scan: the device linker unless NDFL_HOST_LINK selects the host's, which also
// takes over on LINK_FALLBACK -- from the finder's lists already on the device.  FIND_OVERFLOW asks
// for the call's one rescan; without one left, the host linker goes on with the list as it is.
int Decode::link(bool may_rescan) {
    if (!S.knobs.host_link) {
        const int rc = devlink();
        if (rc == FIND_OVERFLOW ? may_rescan : rc != LINK_FALLBACK) return rc;
    }
    return hostlink(may_rescan);
}

// The scan and the stage that follows it, and both once more if that stage found the survivor list
// too short (FIND_OVERFLOW): one rescan per call at most.
int Decode::scanned(int (Decode::*stage)(bool may_rescan)) {
    INF_RC(scan(true));
    const int rc = (this->*stage)(true);
    if (rc != FIND_OVERFLOW) return rc;
    INF_RC(scan(true));
    return (this->*stage)(false);
}

int Decode::run(const uint8_t* in, uint64_t in_len) {
    S.pending_after_dev = 0;
    INF_RC(begin(in, in_len));
    return scanned(&Decode::link);
}

// ndfl_inflate_sync: the first confirmed block boundary in [start_bit, end_bit) (NONE if none) -- the
// scan, the host's candidate list and one count launch over it, without linking or emit.
int Decode::sync_probe(const uint8_t* in, uint64_t in_len, uint64_t* sync_bit) {
    *sync_bit = inf::NONE;
    if (start_bit >= end_bit) return 0;
    INF_RC(begin(in, in_len));
    INF_RC(scanned(&Decode::host_candidates));
    INF_RC(count_chains(L.starts, 0, L.res));
    *sync_bit = first_sync(L.starts, L.res);
    return 0;
}

// Diagnostics (ndfl_inflate_headers): the finder phase alone over a whole stream.  out = the accepted
// headers in ascending order (the per-segment lists, each capped at SEG_CAP, as the decode sees
// them); surv = the finder's survivors (unsorted, bit 63 = dynamic); stats[0] survivors found,
// [1] headers accepted before the cap, [2] segments over SEG_CAP, [3] survivors past the list's
// capacity (dropped).
static int inflate_headers(InflateScratch& S, hipStream_t s, const uint8_t* in, uint64_t in_len, uint32_t flags,
                           uint64_t* out, uint64_t cap, uint64_t* n_out, uint64_t* surv, uint64_t surv_cap,
                           uint64_t* stats) {
    using namespace inf;
    Decode d{S, s};
    d.flags = flags; d.nbits = in_len * 8; d.nwords = (in_len + 3) / 4;
    INF_RC(stage_input(S, s, in, in_len, flags, &d.d_w));
    INF_CHK(S.d_stats.ensure(512));
    uint32_t qc = 0;
    for (int scans = 0; scans < 2; scans++) {                   // (as a decode: one rescan at most)
        INF_RC(d.scan(false));
        INF_CHK(hipMemcpyAsync(&qc, S.d_stats.as<const uint32_t>() + SW_QCOUNT, 4, hipMemcpyDeviceToHost, s));
        INF_CHK(hipStreamSynchronize(s));
        if (!survivors_overflowed(S, qc)) break;
    }
    const uint32_t nseg = d.nseg;
    std::vector<uint32_t> cnt(nseg);
    std::vector<uint64_t> lists((uint64_t)nseg * SEG_CAP);
    INF_CHK(hipMemcpyAsync(cnt.data(), d.d_cnt, nseg * 4ull, hipMemcpyDeviceToHost, s));
    INF_CHK(hipMemcpyAsync(lists.data(), d.d_list, lists.size() * 8, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    const uint32_t qcap = S.q_cap;
    std::vector<uint64_t> acc;
    uint64_t total = 0, over = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        total += cnt[k];
        over += cnt[k] > SEG_CAP;
        for (uint32_t i = 0; i < std::min(cnt[k], SEG_CAP); i++) acc.push_back(lists[(uint64_t)k * SEG_CAP + i]);
    }
    std::sort(acc.begin(), acc.end());
    *n_out = acc.size();
    if (out) memcpy(out, acc.data(), std::min<uint64_t>(cap, acc.size()) * 8);
    if (surv && surv_cap) {
        const uint64_t ns = std::min<uint64_t>(std::min<uint64_t>(qc, qcap), surv_cap);
        if (ns) INF_CHK(hipMemcpy(surv, S.d_q.as<const char>() + 64, ns * 8, hipMemcpyDeviceToHost));
    }
    if (stats) { stats[0] = qc; stats[1] = total; stats[2] = over; stats[3] = qc > qcap ? qc - qcap : 0; }
    return 0;
}

// ndfl_inflate_tail / ndfl_inflate_tail_map after a deferred-window range decode: `kernel` over the
// last n bytes (dst...: its arguments between n and the fail flag).  NDFL_E_UNSUPPORTED: a reference
// chain longer than TAIL_STEPS.
template <class K, class... A>
static int inflate_tail_run(InflateScratch& S, hipStream_t s, uint64_t n, K kernel, A... dst) {
    if (!S.pending) return NDFL_E_STATE;
    if (n > S.p_nbytes) return NDFL_E_ARG;
    if (n == 0) return 0;
    if (!S.h_cnt) INF_CHK(hipHostMalloc(&S.h_cnt, 64, 0));
    uint32_t* h = (uint32_t*)S.h_cnt;
    uint32_t* d_fail = S.d_stats.as<uint32_t>() + SW_TAIL_FAIL;
    INF_CHK(hipMemsetAsync(d_fail, 0, 4, s));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, S.d_pend.as<const uint32_t>(),
                       S.d_ref.as<const uint32_t>(), (const uint8_t*)S.p_out, S.p_nbytes - n, n, dst..., d_fail);
    INF_CHK(hipGetLastError());
    INF_CHK(hipMemcpyAsync(h + 8, d_fail, 4, hipMemcpyDeviceToHost, s));
    INF_CHK(hipStreamSynchronize(s));
    return h[8] ? NDFL_E_UNSUPPORTED : 0;
}
static int inflate_tail(InflateScratch& S, hipStream_t s, uint64_t n, uint8_t* dst) {
    return inflate_tail_run(S, s, n, ndfl_inflate_tail_kernel, dst);
}
static int inflate_tail_map(InflateScratch& S, hipStream_t s, uint64_t n, uint32_t* dst) {
    return inflate_tail_run(S, s, n, ndfl_inflate_tail_map_kernel, S.p_dict_len, dst);
}

// Second half of a deferred-window range decode: the caller has written the window
// (out[0, dict_len)); resolve every deferred copy (those that read the window directly or through
// other copies included).  *n_resolved = pending 32-byte groups at the start.
static int inflate_resolve(InflateScratch& S, hipStream_t s, uint64_t* n_resolved) {
    *n_resolved = 0;
    if (!S.pending) return NDFL_E_STATE;
    S.pending = false;
    INF_RC(resolve_rounds(S, s, S.p_out, S.p_nbytes, n_resolved));
    S.resolved_groups = *n_resolved;
    return 0;
}
