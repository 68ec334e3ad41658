// Host code of ndfl_deflate_batch_chunked under AddressSanitizer and UBSan, on the CPU, no GPU needed: the
// argument paths that return before the first HIP call, and the chunk and stream table builder
// (seg_build_tables, csrc/capi/ndfl_deflate_batch_chunked.cpp), which makes no HIP call -- empty streams,
// lengths around the multiples of chunk_len, chunk_len 1 and 65536, 70,000 streams, and a chunk count that
// does not fit 32 bits (NDFL_E_UNSUPPORTED, before anything is allocated).
// A stand-alone program:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Wno-unused-function -Wno-unused-result -Wno-unused-value -Wno-pass-failed \
//         -o sanitize_chunked_host scripts/sanitize_chunked_host.cpp && ./sanitize_chunked_host
//
// It prints "ok" and returns 0; a sanitizer report or a failed check ends it with another status.
#include "../deflate-library-java_amd/csrc/capi/ndfl_capi.cpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// Every rule of the tables for `lens` at chunk_len.
static void check_tables(const std::vector<uint64_t>& lens, uint32_t chunk_len) {
    std::vector<ndfl_member_item> items;
    uint64_t in_off = 3;
    for (size_t i = 0; i < lens.size(); i++) {
        items.push_back(ndfl_member_item{in_off, lens[i], 0, 0, (uint32_t)(i % 3), (uint32_t)((i / 3) % 3)});
        in_off += lens[i] + (i & 1);
    }
    SegTables T;
    CHECK(seg_build_tables(items.data(), (uint32_t)items.size(), chunk_len, T) == NDFL_OK);
    CHECK(T.streams.size() == items.size());
    CHECK(T.staged == (uint64_t)T.chunks.size() * chunk_len);
    uint64_t k = 0, obase = 0;
    bool any = false;
    for (size_t i = 0; i < items.size(); i++) {
        const uint64_t len = lens[i];
        const uint64_t cnt = len == 0 ? 1 : (len + chunk_len - 1) / chunk_len;
        const SegStream& s = T.streams[i];
        CHECK(s.first_chunk == k && s.nchunks == cnt && s.obase == obase && s.obase % 4 == 0);
        const uint32_t kind = items[i].format == NDFL_FMT_ZLIB ? NDFL_SUM_ADLER32 : items[i].format == NDFL_FMT_GZIP ? NDFL_SUM_CRC32
                                                                                                               : items[i].sum;
        any = any || kind != NDFL_SUM_NONE;
        uint64_t sum = 0;
        for (uint64_t j = 0; j < cnt; j++) {
            const SegChunk& c = T.chunks[k + j];
            CHECK(c.stream == i && c.start == k * chunk_len && c.src == items[i].in_off + j * chunk_len && c.pad == 0);
            CHECK(c.len <= chunk_len && (j + 1 == cnt || c.len == chunk_len) && (c.len > 0 || len == 0));
            CHECK(((c.flags & SEG_FIRST) != 0) == (j == 0) && ((c.flags & SEG_LAST) != 0) == (j + 1 == cnt));
            CHECK(((c.flags >> SEG_SUM_SHIFT) & 3u) == kind && (c.flags >> (SEG_SUM_SHIFT + 2)) == 0);
            sum += c.len;
        }
        CHECK(sum == len);
        // the stream's DEFLATE bytes, a trailer and the two words the encoders and the copy may touch past them
        CHECK(seg_out_slot(len, chunk_len) >= ndfl_deflate_bound(len, chunk_len) + 8 + 8 && seg_out_slot(len, chunk_len) % 4 == 0);
        obase += seg_out_slot(len, chunk_len);
        k += cnt;
    }
    CHECK(k == T.chunks.size() && obase == T.out_bytes && any == T.any_sum);
}

int main() {
    // ---- argument errors: `ctx` is only compared with null on these paths ----------------------------
    alignas(16) static unsigned char fake_ctx[16];
    ndfl_ctx* c = (ndfl_ctx*)fake_ctx;
    std::vector<uint8_t> in(100, 7), out(256, 0xA5);
    ndfl_member_item item{0, 100, 0, 200, NDFL_FMT_RAW, NDFL_SUM_NONE};
    ndfl_deflate_result res{};
    struct Tup { int dyn, a, b, c, d; };
    const Tup full{1, 3, 258, 1, 32768}, rle{0, 3, 258, 1, 1}, lit{1, 0, 0, 0, 0};
    auto call = [&](ndfl_ctx* ctx, const ndfl_member_item* it, ndfl_deflate_result* r, uint32_t n, Tup t, uint32_t chunk_len,
                    uint32_t hist_limit) {
        return ndfl_deflate_batch_chunked(ctx, in.data(), in.size(), out.data(), out.size(), it, r, n, t.dyn, t.a, t.b, t.c, t.d,
                                          chunk_len, hist_limit, 0);
    };
    for (const Tup& t : {full, rle, lit}) {
        CHECK(call(nullptr, &item, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(nullptr, nullptr, nullptr, 0, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, nullptr, nullptr, 0, t, 0, 99999) == NDFL_OK);
        CHECK(call(c, &item, &res, 1, t, 0, 32768) == NDFL_E_ARG);
        CHECK(call(c, &item, &res, 1, t, 65537, 32768) == NDFL_E_UNSUPPORTED);
        CHECK(call(c, &item, &res, 1, t, 65536, 32769) == NDFL_E_ARG);
        CHECK(call(c, &item, &res, 1, t, 0, 32769) == NDFL_E_ARG);
        CHECK(call(c, nullptr, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &item, nullptr, 1, t, 65536, 32768) == NDFL_E_ARG);
        ndfl_member_item two[2] = {{0, 100, 0, 100, 0, 0}, {0, 100, 99, 100, 0, 0}};       // overlapping outputs
        ndfl_deflate_result r2[2] = {};
        CHECK(call(c, two, r2, 2, t, 65536, 32768) == NDFL_E_ARG);
        ndfl_member_item far = {0, 101, 0, 100, 0, 0}, fmt = {0, 100, 0, 100, 3, 0}, sum = {0, 100, 0, 100, 0, 3};
        ndfl_member_item huge = {0, 100, 1ull << 63, 1ull << 63, 0, 0};
        CHECK(call(c, &far, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &fmt, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &sum, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &huge, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
    }
    // the six invalid tuples, refused before the frame is looked at (chunk_len 65537 would be NDFL_E_UNSUPPORTED)
    for (const Tup& t : {Tup{1, 2, 258, 1, 32768}, Tup{1, 3, 259, 1, 32768}, Tup{1, 5, 4, 1, 10}, Tup{1, 3, 258, 0, 10},
                         Tup{1, 3, 258, 1, 32769}, Tup{1, 3, 258, 10, 9}}) {
        CHECK(call(c, &item, &res, 1, t, 65536, 32768) == NDFL_E_ARG);
        CHECK(call(c, &item, &res, 1, t, 65537, 32768) == NDFL_E_ARG);
    }
    for (uint8_t b : out) CHECK(b == 0xA5);
    CHECK(res.status == 0 && res.out_len == 0 && res.end_bits == 0);

    // ---- the tables ----------------------------------------------------------------------------------------
    for (uint32_t cl : {1u, 2u, 64u, 1000u, 65535u, 65536u}) {
        const uint64_t c64 = cl;
        check_tables({0}, cl);
        check_tables({0, 0, 0}, cl);
        check_tables({0, 1, 2, c64 - 1, c64, c64 + 1, 2 * c64 - 1, 2 * c64, 2 * c64 + 1, 5 * c64 + 7, 0, c64, 0}, cl);
    }
    check_tables({70000, 1, 0, 65537}, 1);                      // a chunk per byte
    {
        std::vector<uint64_t> lens(70000);
        for (size_t i = 0; i < lens.size(); i++) lens[i] = (i * 2654435761u) % 300;
        check_tables(lens, 64);
        check_tables(lens, 65536);
    }
    // a chunk count that does not fit 32 bits: refused, nothing allocated
    {
        SegTables T;
        const ndfl_member_item big1{0, 1ull << 32, 0, 0, 0, 0};                             // 2^32 chunks of one byte
        CHECK(seg_build_tables(&big1, 1, 1, T) == NDFL_E_UNSUPPORTED && T.chunks.empty() && T.streams.empty());
        const ndfl_member_item big2[2] = {{0, (1ull << 32) - 1, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};   // ... the empty stream's chunk
        CHECK(seg_build_tables(big2, 2, 1, T) == NDFL_E_UNSUPPORTED && T.chunks.empty());
        const ndfl_member_item big3{0, ~0ull, 0, 0, 0, 0};
        CHECK(seg_build_tables(&big3, 1, 65536, T) == NDFL_E_UNSUPPORTED && T.chunks.empty());
        CHECK(seg_build_tables(&big3, 1, 1, T) == NDFL_E_UNSUPPORTED && T.chunks.empty());
        // through the call: the input need not exist, the refusal comes before it is read
        std::vector<uint8_t> o(16, 0xA5);
        const ndfl_member_item it{0, 1ull << 32, 0, 16, 0, 0};
        ndfl_deflate_result r{};
        CHECK(ndfl_deflate_batch_chunked(c, in.data(), 1ull << 32, o.data(), 16, &it, &r, 1, 1, 3, 258, 1, 32768, 1, 0, 0) ==
              NDFL_E_UNSUPPORTED);
        for (uint8_t b : o) CHECK(b == 0xA5);
        CHECK(r.status == 0 && r.out_len == 0);
    }
    puts("ok");
    return 0;
}
