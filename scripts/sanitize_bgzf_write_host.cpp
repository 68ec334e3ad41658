// Host code of ndfl_deflate_bgzf under AddressSanitizer and UBSan, on the CPU, no GPU needed: the argument
// paths that return before the first HIP call, the plan of a call (bgzw_plan,
// csrc/capi/ndfl_deflate_bgzf.cpp: blocks, members, tiles, slot and staged sizes, the limits refused before
// anything is allocated) and ndfl_bgzf_bound against a member-by-member sum.
// A stand-alone program:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Wno-unused-function -Wno-unused-result -Wno-unused-value -Wno-pass-failed \
//         -o sanitize_bgzf_write_host scripts/sanitize_bgzf_write_host.cpp && ./sanitize_bgzf_write_host
//
// It prints "ok" and returns 0; a sanitizer report or a failed check ends it with another status.
#include "../deflate-library-java_amd/csrc/capi/ndfl_capi.cpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// The bound, one member at a time.
static uint64_t bound_by_members(uint64_t in_len, uint32_t block_len) {
    uint64_t sum = 28;
    for (uint64_t at = 0; at < in_len; at += block_len) {
        const uint64_t len = std::min<uint64_t>(block_len, in_len - at);
        sum += 18 + 5 * std::max<uint64_t>(1, (len + 65534) / 65535) + len + 8;
    }
    return sum;
}

int main() {
    // ---- the bound ---------------------------------------------------------------------------------------
    for (uint32_t bl : {1u, 2u, 29u, 4096u, 65280u, 65505u, 65535u, 65536u})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)bl - 1, (uint64_t)bl, (uint64_t)bl + 1, 3 * (uint64_t)bl + 7,
                           (uint64_t)70001})
            CHECK(ndfl_bgzf_bound(n, bl) == bound_by_members(n, bl));
    CHECK(ndfl_bgzf_bound(65505, 65505) == 65536 + 28 && ndfl_bgzf_bound(65536, 65536) == 65572 + 28);
    for (uint32_t bl : {0u, 65537u, 0x80000000u, 0xFFFFFFFFu}) CHECK(ndfl_bgzf_bound(12345, bl) == 0 && ndfl_bgzf_bound(0, bl) == 0);
    CHECK(ndfl_bgzf_bound(8ull << 30, 1) == (8ull << 30) * 32 + 28);

    // ---- the plan ----------------------------------------------------------------------------------------
    for (uint32_t bl : {1u, 16u, 255u, 65280u, 65536u})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)bl - 1, (uint64_t)bl, (uint64_t)bl + 1, 255 * (uint64_t)bl,
                           256 * (uint64_t)bl, 256 * (uint64_t)bl + 1, 1000 * (uint64_t)bl + 3}) {
            BgzwPlan P;
            CHECK(bgzw_plan(n, bl, P) == NDFL_OK);
            CHECK(P.nblk == (n + bl - 1) / bl && P.n_members == P.nblk + 1);
            CHECK((uint64_t)P.ntiles * bgzw::SIZE_TILE >= P.n_members && (uint64_t)(P.ntiles - 1) * bgzw::SIZE_TILE < P.n_members);
            CHECK(P.staged == (uint64_t)P.nblk * bl && P.staged >= n && P.staged - n < bl);
            CHECK(P.slot % 4 == 0 && P.slot >= ndfl_deflate_bound(bl, bl) + 16 && P.out_bytes == P.nblk * P.slot);
        }
    {
        BgzwPlan P;
        CHECK(bgzw_plan(100, 0, P) == NDFL_E_ARG && bgzw_plan(100, 65537, P) == NDFL_E_UNSUPPORTED);
        CHECK(bgzw_plan((8ull << 30) + 1, 65280, P) == NDFL_E_UNSUPPORTED && bgzw_plan(8ull << 30, 65280, P) == NDFL_OK);
        CHECK(bgzw_plan(0x7FFFFFFFull, 1, P) == NDFL_E_UNSUPPORTED);           // 2^31 - 1 blocks
        CHECK(bgzw_plan(0x7FFFFFFEull, 1, P) == NDFL_OK && P.n_members == 0x7FFFFFFFu && P.ntiles == 0x800000u);
        CHECK(bgzw_plan(8ull << 30, 4, P) == NDFL_E_UNSUPPORTED);              // 2^31 blocks
        CHECK(bgzw_plan(8ull << 30, 5, P) == NDFL_OK && P.nblk == 1717986919u && P.staged == 5ull * 1717986919u);
    }

    // ---- argument errors: `ctx` is only compared with null on these paths --------------------------------
    alignas(16) static unsigned char fake_ctx[16];
    ndfl_ctx* c = (ndfl_ctx*)fake_ctx;
    std::vector<uint8_t> in(100, 7), out(256, 0xA5);
    ndfl_bgzf_write_result res;
    ndfl_bgzf_member table[4];
    auto call = [&](ndfl_ctx* ctx, const uint8_t* i, uint64_t n, uint8_t* o, uint64_t cap, ndfl_bgzf_write_result* r,
                    ndfl_bgzf_member* t, uint32_t tc, int min_run, uint32_t block_len) {
        return ndfl_deflate_bgzf(ctx, i, n, o, cap, r, t, tc, 1, min_run, 258, 1, 32768, block_len, 0);
    };
    memset(&res, 0x5A, sizeof res);
    CHECK(call(nullptr, in.data(), 100, out.data(), 256, &res, table, 4, 3, 65280) == NDFL_E_ARG);
    CHECK(call(c, in.data(), 100, out.data(), 256, nullptr, table, 4, 3, 65280) == NDFL_E_ARG);
    CHECK(call(c, nullptr, 100, out.data(), 256, &res, table, 4, 3, 65280) == NDFL_E_ARG);
    CHECK(call(c, in.data(), 100, nullptr, 256, &res, table, 4, 3, 65280) == NDFL_E_ARG);
    CHECK(call(c, in.data(), 100, out.data(), 256, &res, nullptr, 4, 3, 65280) == NDFL_E_ARG);
    CHECK(res.status == 0x5A5A5A5A);                                            // (untouched so far)
    CHECK(call(c, in.data(), 100, out.data(), 256, &res, table, 4, 2, 65280) == NDFL_E_ARG);     // the tuple first ...
    CHECK(call(c, in.data(), 100, out.data(), 256, &res, table, 4, 2, 65537) == NDFL_E_ARG);
    CHECK(call(c, in.data(), 100, out.data(), 256, &res, table, 4, 3, 0) == NDFL_E_ARG);         // ... then block_len
    CHECK(call(c, in.data(), 100, out.data(), 256, &res, table, 4, 3, 65537) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, in.data(), (8ull << 30) + 1, out.data(), 256, &res, table, 4, 3, 65280) == NDFL_E_UNSUPPORTED);
    CHECK(call(c, in.data(), 0x7FFFFFFFull, out.data(), 256, &res, table, 4, 3, 1) == NDFL_E_UNSUPPORTED);
    CHECK(res.status == 0 && res.n_members == 0 && res.bad_member == 0 && res.n_stored == 0 && res.out_len == 0);
    for (uint8_t b : out) CHECK(b == 0xA5);
    puts("ok");
    return 0;
}
