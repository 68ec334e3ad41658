// Host code of the raw-DEFLATE decode (csrc/capi/ndfl_inflate.cpp) under AddressSanitizer and UBSan, on the CPU, no
// GPU needed: the host linker's parts that make no HIP call -- the range filter of the candidate list (filter_range),
// the longest-first bucket order (count_order), the repair scan, the walk and the serial-fallback request (ChainLinks),
// the first-error scan (first_error), the sync probe's choice (first_sync) -- driven with hand-made ChainRes vectors,
// and the argument paths of the inflate entry points that return before the first HIP call.
// A stand-alone program:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Wno-unused-function -Wno-unused-result -Wno-unused-value -Wno-pass-failed \
//         -o sanitize_inflate_host scripts/sanitize_inflate_host.cpp && ./sanitize_inflate_host
//
// It prints "ok" and returns 0; a sanitizer report or a failed check ends it with another status.
#include "../deflate-library-java_amd/csrc/capi/ndfl_capi.cpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// A model stream: block k spans bits [bnd[k], bnd[k + 1]) and produces 10 + k % 7 bytes; the last block is final.
// A counted chain decodes one block (so every boundary that is no candidate needs a repair chain).
struct Model {
    std::vector<uint64_t> bnd;
    std::set<uint64_t> cand;                    // the finder's candidates (any subset of the boundaries)
    uint64_t end_bit = inf::NONE;
    uint32_t counted = 0;
    explicit Model(size_t nblocks) {
        for (size_t k = 0; k <= nblocks; k++) bnd.push_back(17 + 1000 * k + k % 5);
        for (size_t k = 1; k < nblocks; k++) cand.insert(bnd[k]);
    }
    uint64_t bytes(size_t k) const { return 10 + k % 7; }
    ChainRes count(uint64_t start, const std::vector<uint64_t>& sorted) {
        counted++;
        const size_t k = (size_t)(std::lower_bound(bnd.begin(), bnd.end(), start) - bnd.begin());
        CHECK(k + 1 < bnd.size() && bnd[k] == start);
        ChainRes r{};
        r.end_bit = bnd[k + 1];
        r.out_count = bytes(k);
        r.status = k + 2 == bnd.size() ? inf::ST_FINAL : inf::ST_BOUNDARY;
        const auto it = std::lower_bound(sorted.begin(), sorted.end(), r.end_bit);
        r.next = it != sorted.end() && *it == r.end_bit ? (uint32_t)(it - sorted.begin()) : 0xFFFFFFFFu;
        return r;
    }
};

// The host linker's loop (Decode::hostlink) over the model; returns the walk's code.
struct Linked { int code; ChainLinks L; uint64_t rounds = 0, serial = 0; };
static Linked link_model(Model& m, uint64_t start_bit, uint64_t dict_len) {
    Linked o{};
    ChainLinks& L = o.L;
    L.end_bit = m.end_bit; L.dict_len = dict_len;
    L.starts.assign(1, 0);
    for (uint64_t c : m.cand) L.starts.push_back(c);
    filter_range(L.starts, start_bit, m.end_bit);
    L.n0 = L.starts.size();
    const std::vector<uint64_t> sorted(L.starts);
    CHECK(count_order(L.starts, m.end_bit).size() == L.n0);
    for (uint64_t s : L.starts) L.res.push_back(m.count(s, sorted));
    for (int round = 0; round < 8; round++) {
        const std::vector<uint64_t> todo = L.repair_todo();
        if (todo.empty()) break;
        CHECK(std::set<uint64_t>(todo.begin(), todo.end()).size() == todo.size());    // each boundary once
        for (uint64_t b : todo) { size_t at = 0; CHECK(L.find_at(b, at) && at == (size_t)inf::NONE); }   // placeholders
        CHECK(L.repair_todo().empty());                                                // ... which are not asked for again
        std::vector<ChainRes> r;
        for (uint64_t b : todo) r.push_back(m.count(b, sorted));
        L.add(todo, r);
        o.rounds++;
    }
    for (uint64_t need = 0;;) {
        o.code = L.walk(&need);
        if (o.code != WALK_COUNT) break;
        L.add({need}, {m.count(need, sorted)});
        L.cur = L.starts.size() - 1;
        o.serial++;
    }
    return o;
}

// The walk's chains are the blocks from `first` on, in order, with running output offsets.
static void check_chains(const Model& m, const Linked& o, size_t first, size_t nblocks, uint64_t dict_len, uint64_t stop) {
    CHECK(o.code == 0 && o.L.chains.size() == nblocks && o.L.stop_bit == stop);
    uint64_t off = dict_len;
    for (size_t k = 0; k < nblocks; k++) {
        const EmitChain& e = o.L.chains[k];
        CHECK(e.start_bit == m.bnd[first + k] && e.end_bit == m.bnd[first + k + 1] && e.out_off == off);
        CHECK(e.out_count == m.bytes(first + k) && e.slot < o.L.starts.size() && o.L.starts[e.slot] == e.start_bit);
        off += e.out_count;
    }
    CHECK(o.L.produced == off - dict_len);
}

int main() {
    using namespace inf;
    // ---- plain chains of 1, 2 and 4,097 links: every boundary a candidate, nothing repaired ------------------------
    for (size_t n : {(size_t)1, (size_t)2, (size_t)4097}) {
        Model m(n);
        const Linked o = link_model(m, m.bnd[0], 0);
        check_chains(m, o, 0, n, 0, m.bnd[n]);
        CHECK(o.rounds == 0 && o.serial == 0 && m.counted == n);
    }
    // ---- a boundary that is no candidate: a placeholder, filled by one repair round -------------------------------
    {
        Model m(9);
        m.cand.erase(m.bnd[4]);
        const Linked o = link_model(m, m.bnd[0], 100);
        check_chains(m, o, 0, 9, 100, m.bnd[9]);
        CHECK(o.rounds == 1 && o.serial == 0 && o.L.starts.size() == o.L.n0 + 1 && o.L.starts.back() == m.bnd[4]);
    }
    // ---- twelve such boundaries in a row: eight parallel rounds, then four serial requests ------------------------
    {
        Model m(20);
        for (size_t k = 3; k < 15; k++) m.cand.erase(m.bnd[k]);
        const Linked o = link_model(m, m.bnd[0], 0);
        check_chains(m, o, 0, 20, 0, m.bnd[20]);
        CHECK(o.rounds == 8 && o.serial == 4);
    }
    // ---- ranges: from a seam to a seam, end_bit inside a block (NDFL_E_ARG), an empty range -------------------------
    {
        Model m(12);
        m.end_bit = m.bnd[9];
        const Linked o = link_model(m, m.bnd[5], 7);
        check_chains(m, o, 5, 4, 7, m.bnd[9]);
        CHECK(o.L.n0 == 4);                                         // the start and the candidates strictly inside
        Model in(12);
        in.end_bit = in.bnd[9] - 3;
        CHECK(link_model(in, in.bnd[5], 0).code == NDFL_E_ARG);
        std::vector<uint64_t> none, one{5, 900, 1000, 1001, 1100, 1200};
        filter_range(none, 40, 40);
        CHECK(none.size() == 1 && none[0] == 40);
        filter_range(one, 1000, 1000);
        CHECK(one.size() == 1 && one[0] == 1000);
        CHECK(count_order({}, 0).empty());
        CHECK(first_sync({40}, {ChainRes{}}) == NONE);
        const Outcome e = first_error({}, {}, 0, true, 0, 40);
        CHECK(e.code == 0 && e.produced == 0 && e.consumed_bits == 40);
    }
    // ---- the count order: longest first by 32-Kibit buckets when sorted, as given when not ------------------------------
    {
        std::vector<uint64_t> st{0, 40000, 40100, 200000, 200001, 1200000, 1200008};
        const uint64_t end = 3000000;
        const std::vector<uint32_t> o = count_order(st, end);
        std::vector<uint64_t> len;
        for (uint32_t k : o) len.push_back(std::min<uint64_t>(23, ((k + 1 < st.size() ? st[k + 1] : end) - st[k]) >> 15));
        CHECK(std::set<uint32_t>(o.begin(), o.end()).size() == st.size() && std::is_sorted(len.rbegin(), len.rend()));
        CHECK(o[0] == 4 && o[1] == 6);                              // 30 and 54 buckets: clamped to 23, in list order
        const std::vector<uint64_t> todo{900000, 17, 40000, 40000, 5};
        const std::vector<uint32_t> u = count_order(todo, end);
        for (uint32_t k = 0; k < u.size(); k++) CHECK(u[k] == k);
        CHECK(count_order({7}, 5) == std::vector<uint32_t>{0});     // (a start past end_bit: length 0)
    }
    // ---- the first error: in the first, a middle and the last chain, with and without partial -----------------------
    {
        std::vector<EmitChain> ch(5);
        for (size_t k = 0; k < 5; k++) ch[k] = EmitChain{100 * k, 100 * k + 100, 32768 + 50 * k, 50, k};
        for (size_t bad : {(size_t)0, (size_t)2, (size_t)4})
            for (int reason : {(int)R_UEOS, (int)R_RESERVED_LEN_HI})
                for (bool partial : {false, true}) {
                    std::vector<ChainRes> er(5);
                    for (size_t k = 0; k < 5; k++) er[k] = ChainRes{100 * k + 100, 50, ST_BOUNDARY, 0, 0, 0, 0, 0};
                    er[bad] = ChainRes{100 * bad + 77, 31, ST_ERROR, (uint32_t)reason, 0, 0, 100 * bad + 40, 20};
                    if (bad < 4) er[4] = ChainRes{444, 1, ST_ERROR, R_NO_PREV, 0, 0, 0, 0};     // a later one loses
                    const Outcome o = first_error(er, ch, 32768, partial, 250, 500);
                    if (partial && reason == R_UEOS)
                        CHECK(o.code == NDFL_NEED_INPUT && o.produced == 50 * bad + 20 && o.consumed_bits == 100 * bad + 40);
                    else
                        CHECK(o.code == reason && o.produced == 50 * bad + 31 && o.consumed_bits == 100 * bad + 77);
                }
        std::vector<ChainRes> fine(5, ChainRes{0, 50, ST_BOUNDARY, 0, 0, 0, 0, 0});
        fine[4].status = ST_FINAL;
        const Outcome o = first_error(fine, ch, 32768, true, 250, 500);
        CHECK(o.code == 0 && o.produced == 250 && o.consumed_bits == 500);
    }
    // ---- the sync probe: the first candidate a linked chain ends at whose own chain links on (or is final) ---------
    {
        const std::vector<uint64_t> st{1, 50, 120, 300, 410};
        std::vector<ChainRes> r(5);
        r[0] = ChainRes{50, 0, ST_BOUNDARY, 0, 1, 0, 0, 0};             // (slot 0, the probe's start, is never taken)
        r[1] = ChainRes{120, 0, ST_BOUNDARY, 0, 2, 0, 0, 0};            // links to 120, whose chain stops off the list
        r[2] = ChainRes{299, 0, ST_BOUNDARY, 0, 3, 0, 0, 0};
        r[3] = ChainRes{410, 0, ST_BOUNDARY, 0, 4, 0, 0, 0};            // links to 410, whose chain is final
        r[4] = ChainRes{500, 0, ST_FINAL, 0, 0, 0, 0, 0};
        CHECK(first_sync(st, r) == 410);
        r[2].end_bit = 300;
        CHECK(first_sync(st, r) == 120);
        r[3].next = 9;                                                  // (an index past the list)
        r[1].status = ST_ERROR;
        CHECK(first_sync(st, r) == NONE);
    }
    // ---- argument errors of the entry points: `ctx` is only compared with null on these paths ----------------------
    {
        alignas(16) static unsigned char fake_ctx[16];
        ndfl_ctx* c = (ndfl_ctx*)fake_ctx;
        std::vector<uint8_t> in(100, 7), out(256, 0xA5);
        uint64_t n = 77, bits = 77;
        CHECK(ndfl_inflate(nullptr, in.data(), 100, out.data(), 256, &n, &bits, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate(c, in.data(), 100, out.data(), 256, nullptr, &bits, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate(c, in.data(), 100, out.data(), 256, &n, nullptr, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate(c, nullptr, 100, out.data(), 256, &n, &bits, 0) == NDFL_E_ARG);
        auto range = [&](ndfl_ctx* ctx, const uint8_t* i, uint64_t s, uint64_t e, uint8_t* o, uint64_t dl, uint64_t cap, uint32_t f) {
            return ndfl_inflate_range(ctx, i, 100, s, e, o, dl, cap, &n, &bits, f);
        };
        CHECK(range(nullptr, in.data(), 0, UINT64_MAX, out.data(), 0, 256, 0) == NDFL_E_ARG);
        CHECK(range(c, nullptr, 0, UINT64_MAX, out.data(), 0, 256, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, UINT64_MAX, nullptr, 1, 0, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, UINT64_MAX, nullptr, 0, 1, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, UINT64_MAX, out.data(), 32769, 0, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 801, UINT64_MAX, out.data(), 0, 256, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 8, 8, out.data(), 0, 256, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 8, 7, out.data(), 0, 256, 0) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, UINT64_MAX, out.data(), 0, 256, NDFL_DICT_DEFERRED) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, UINT64_MAX, out.data(), 0, 256, NDFL_IN_PARTIAL | NDFL_DICT_DEFERRED | NDFL_OUT_DEVICE) == NDFL_E_ARG);
        CHECK(range(c, in.data(), 0, 800, out.data(), 0, 256, NDFL_IN_PARTIAL) == NDFL_E_ARG);
        CHECK(ndfl_inflate_range(c, in.data(), 100, 0, UINT64_MAX, out.data(), 0, 256, nullptr, &bits, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate_range(c, in.data(), 100, 0, UINT64_MAX, out.data(), 0, 256, &n, nullptr, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate_sync(nullptr, in.data(), 100, 0, 800, &bits, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate_sync(c, in.data(), 100, 0, 800, nullptr, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate_sync(c, nullptr, 100, 0, 800, &bits, 0) == NDFL_E_ARG);
        CHECK(ndfl_inflate_sync(c, in.data(), 100, 801, 800, &bits, 0) == NDFL_E_ARG);
        uint64_t heads[4] = {0, 0, 0, 0};
        CHECK(ndfl_inflate_headers(nullptr, in.data(), 100, 0, heads, 4, &n, nullptr, 0, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_headers(c, in.data(), 100, 0, heads, 4, nullptr, nullptr, 0, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_headers(c, nullptr, 100, 0, heads, 4, &n, nullptr, 0, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_headers(c, in.data(), 100, 0, nullptr, 4, &n, nullptr, 0, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_headers(c, in.data(), 100, 0, heads, 4, &n, nullptr, 1, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_resolve(nullptr, &n) == NDFL_E_ARG && ndfl_inflate_resolve(c, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_tail(nullptr, 1, out.data()) == NDFL_E_ARG && ndfl_inflate_tail(c, 1, nullptr) == NDFL_E_ARG);
        CHECK(ndfl_inflate_tail_map(nullptr, 1, (uint32_t*)heads) == NDFL_E_ARG);
        CHECK(ndfl_inflate_tail_map(c, 1, nullptr) == NDFL_E_ARG);
        for (uint8_t b : out) CHECK(b == 0xA5);
        CHECK(n == 77 && bits == 77);
    }
    puts("ok");
    return 0;
}
