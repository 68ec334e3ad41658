// Host code of ndfl_deflate_batch_binsplit under AddressSanitizer and UBSan, on the CPU, no GPU needed:
// the argument checks (every error path returns before the first HIP call), the search parameters and
// the wave's ring and token list sizes with the grid lowered to the budget.  A stand-alone program:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Wno-unused-function -Wno-unused-result -Wno-unused-value -Wno-pass-failed \
//         -o sanitize_batch_binsplit_host scripts/sanitize_batch_binsplit_host.cpp && ./sanitize_batch_binsplit_host
//
// It prints "ok" and returns 0; a sanitizer report or a failed check ends it with another status.
#include "../deflate-library-java_amd/csrc/capi/ndfl_capi.cpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

int main() {
    // ---- argument errors: `ctx` is only compared with null on these paths ----------------------------
    alignas(16) static unsigned char fake_ctx[16];
    ndfl_ctx* c = (ndfl_ctx*)fake_ctx;
    std::vector<uint8_t> in(100, 7), out(256, 0xA5);
    ndfl_member_item item{0, 100, 0, 200, NDFL_FMT_RAW, NDFL_SUM_NONE};
    ndfl_deflate_result res{};
    const ndfl_strategy_desc fd{NDFL_KIND_LZ77, 1, 3, 258, 1, 32768}, stored{NDFL_KIND_UNCOMPRESSED, 0, 0, 0, 0, 0};
    const ndfl_strategy_desc seven{7, 1, 3, 258, 1, 32768}, bad{NDFL_KIND_LZ77, 1, 2, 258, 1, 32768};
    auto call = [&](ndfl_ctx* ctx, const ndfl_member_item* it, ndfl_deflate_result* r, uint32_t n, const ndfl_strategy_desc* sub,
                    int32_t m, uint32_t chunk_len, uint32_t hist_limit) {
        return ndfl_deflate_batch_binsplit(ctx, in.data(), in.size(), out.data(), out.size(), it, r, n, sub, m, chunk_len,
                                           hist_limit, 0);
    };
    CHECK(call(nullptr, &item, &res, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, nullptr, nullptr, 0, nullptr, 0, 0, 99999) == NDFL_OK);
    CHECK(call(c, &item, &res, 1, nullptr, 100, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &fd, 0, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &fd, -1, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &fd, 100, 0, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &fd, 100, 65537, 32768) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, &item, &res, 1, &fd, 100, 65536, 32769) == NDFL_E_ARG);
    CHECK(call(c, nullptr, &res, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, nullptr, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &stored, 100, 65536, 32768) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, &item, &res, 1, &stored, 100, 65537, 32768) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, &item, &res, 1, &stored, 0, 65537, 32768) == NDFL_E_ARG);
    CHECK(call(c, &item, &res, 1, &seven, 100, 65536, 32768) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, &item, &res, 1, &bad, 100, 65536, 32768) == NDFL_E_ARG);
    {
        ndfl_member_item two[2] = {{0, 100, 0, 100, 0, 0}, {0, 100, 99, 100, 0, 0}};       // overlapping outputs
        ndfl_deflate_result r2[2] = {};
        CHECK(call(c, two, r2, 2, &fd, 100, 65536, 32768) == NDFL_E_ARG);
        ndfl_member_item far = {0, 101, 0, 100, 0, 0}, fmt = {0, 100, 0, 100, 3, 0}, huge = {0, 100, 1ull << 63, 1ull << 63, 0, 0};
        CHECK(call(c, &far, &res, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &fmt, &res, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &huge, &res, 1, &fd, 100, 65536, 32768) == NDFL_E_ARG);
    }
    for (uint8_t b : out) CHECK(b == 0xA5);
    CHECK(res.status == 0 && res.out_len == 0 && res.end_bits == 0);

    // ---- the search parameters ----------------------------------------------------------------------
    BatchLzScratch Z;
    Knobs knobs{};
    {
        BatchBinsplitLaunch l{Z, knobs, &item, dbsp::Args{}};
        l.set_search(fd);
        CHECK(l.a.dynamic == 1 && l.a.min_run == 3 && l.a.max_run == 258 && l.a.min_dist == 1 && l.a.max_dist == 32768 && l.a.link);
        l.set_search(ndfl_strategy_desc{NDFL_KIND_LZ77, 0, 0, 0, 0, 0});
        CHECK(l.a.dynamic == 0 && l.a.min_run == 3 && l.a.max_run == 258 && l.a.min_dist == 1 && l.a.max_dist == 0 && !l.a.link);
        l.set_search(ndfl_strategy_desc{NDFL_KIND_LZ77, 1, 3, 258, 1, 1});
        CHECK(l.a.link && l.a.max_dist == 1);
    }
    // ---- the wave's memory: the ring holds the chunk and its window, the list the chunk's tokens; the grid
    // that fits the budget (batch_grid's rule) never leaves a wave's part past the allocation -------------
    const uint64_t longests[] = {0, 1, 63, 64, 65, 4096, 4329, 65535, 65536, 65537, 98304, 98305, 131072, 131073, 1ull << 20,
                                 1ull << 32, ~0ull};
    const uint32_t chunks[] = {1, 2, 63, 64, 65, 1000, 4096, 65535, 65536};
    const uint32_t hists[] = {0, 1, 100, 32767, 32768};
    for (uint64_t longest : longests)
        for (uint32_t chunk_len : chunks)
            for (uint32_t hist : hists) {
                uint32_t ring = 0, tok_cap = 0;
                batch_binsplit_sizes(longest, chunk_len, hist, &ring, &tok_cap);
                const uint64_t span = std::min<uint64_t>(longest, (uint64_t)hist + chunk_len);
                CHECK(ring >= 64 && ring <= dbm::RING_MAX && (ring & (ring - 1)) == 0 && ring >= span);
                CHECK(ring == 64 || ring / 2 < span);
                CHECK(tok_cap >= 64 && tok_cap >= std::min<uint64_t>(chunk_len, longest) && tok_cap <= 65536);
                const size_t per_wave = (size_t)ring * 2 + (size_t)tok_cap * 4;
                CHECK(per_wave <= (size_t)512 << 10);
                for (uint32_t want : {1u, 7u, 511u, 512u, 513u, 1792u, 4096u}) {
                    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>(want, BATCH_LZ_BUDGET / per_wave));
                    CHECK(grid >= std::min(want, 512u) && (size_t)grid * per_wave <= BATCH_LZ_BUDGET);
                    // the last wave's token list and ring end inside grid * per_wave bytes
                    const size_t toks_end = ((size_t)(grid - 1) * tok_cap + tok_cap) * 4;
                    const size_t ring_end = (size_t)grid * tok_cap * 4 + ((size_t)(grid - 1) * ring + ring) * 2;
                    CHECK(toks_end <= (size_t)grid * tok_cap * 4 && ring_end == (size_t)grid * per_wave);
                }
            }
    puts("ok");
    return 0;
}
