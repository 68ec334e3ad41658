// ndfl_capi.cpp -- host side of the C ABI declared in include/ndfl.h.
// Compiled as HIP for gfx950 together with the kernels (single translation unit).
#include "../../../include/ndfl.h"
#include "../hip/deflate_kernels.hip"
#include "../hip/deflate_split.hip"
#include "../hip/lz77_kernels.hip"
#include "../hip/strategy_kernels.hip"
#include "../hip/deflate_seg.hip"
#include "../hip/inflate_kernels.hip"
#include "ndfl_inflate.cpp"
#include "../hip/inflate_batch.hip"
#include "../hip/inflate_bgzf.hip"
#include "../hip/deflate_bgzf.hip"
#include "../hip/deflate_batch.hip"
#include "../hip/deflate_batch_lz.hip"
#include "../hip/deflate_batch_multi.hip"
#include "../hip/deflate_batch_binsplit.hip"

#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <stdlib.h>
#include <vector>
#include <functional>
#include <map>
#include <memory>
#include <new>

namespace {

// A call's own temporary buffer: released on every return path.  (The context's members are plain
// DevBufs, released by ndfl_ctx_destroy.)
struct ScopedBuf : DevBuf {
    ScopedBuf() = default;
    ScopedBuf(ScopedBuf&& o) noexcept : DevBuf(o) { o.p = nullptr; o.cap = 0; }    // (so: not copyable)
    ~ScopedBuf() { release(); }
};

uint32_t host_crc_tab[1024];
uint32_t host_crc_x[64 + 1024];
uint32_t host_crc_p2[64];          // x^(8 * 2^k)
bool host_tabs_ready = false;

void init_host_tables() {
    if (host_tabs_ready) return;
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ NDFL_CRC_POLY : c >> 1;
        host_crc_tab[i] = c;
    }
    for (int t = 1; t < 4; t++)
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = host_crc_tab[(t - 1) * 256 + i];
            host_crc_tab[t * 256 + i] = (c >> 8) ^ host_crc_tab[c & 0xFF];
        }
    for (uint32_t k = 0; k < 64; k++) host_crc_x[k] = crc_x8n(k);
    for (uint32_t k = 0; k < 1024; k++) host_crc_x[64 + k] = crc_x8n((uint64_t)k * 64);
    host_crc_p2[0] = 1u << 23;
    for (int k = 1; k < 64; k++) host_crc_p2[k] = crc_multmodp(host_crc_p2[k - 1], host_crc_p2[k - 1]);
    host_tabs_ready = true;
}

}  // namespace

struct ndfl_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    bool user_stream = false;       // ndfl_ctx_set_stream named the caller's stream
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_order = nullptr;
    double last_ms = 0;
    double deflate_ms = 0;
    DevBuf d_in, d_out, d_status, d_ticket, d_edge_w, d_edge_v, d_crc, d_crc1, d_tabs, d_hostio;
    DevBuf d_hist, d_codes, d_off;  // split RLE/LITERAL pipeline: histograms, code records, offsets
    DevBuf d_lz, d_link, d_match;   // LZ77 path: staging [pad|hist|data], hash links, per-position matches
    DevBuf d_segtab;                // ndfl_deflate_batch_chunked: the chunk table, then the stream table
    DevBuf d_bgzw;                  // ndfl_deflate_bgzf: the head, the member lengths, the tile sums, the items, the table
    DevBuf d_mdata, d_mstreams[16], d_mbits[16], d_masm;   // strategy composition
    int ncu = 0;                    // the device's compute units (0: unknown)
    InflateScratch inf;
    BatchScratch batch;             // ndfl_inflate_batch: items / results / host-output staging
    BgzfScratch bgzf;               // ndfl_inflate_bgzf: the candidate list, the member table
    BatchLzScratch batch_lz;        // ndfl_deflate_batch_lz77 / _multi: the waves' link rings and token lists
    uint32_t* h_pinned = nullptr;   // small pinned area for results
    Knobs knobs;                    // switches read once at ndfl_ctx_create (ndfl_common.hpp)
    int err_sym = -1;               // the last decode's reserved symbol (ndfl_ctx_error_symbol), or -1
};

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return NDFL_E_DEVICE; } while (0)

// The ordering contract of include/ndfl.h: unless the caller named its stream (ndfl_ctx_set_stream),
// a call's device work starts only after everything queued before the call on the device's default
// stream -- e.g. the torch kernel that produced an NDFL_IN_DEVICE buffer, or the torch kernel still
// using a block the caching allocator has just handed out again as an NDFL_OUT_DEVICE buffer.  (The
// context's own stream is also a blocking stream, which the null stream orders implicitly; the
// event makes the wait explicit.)  Every call synchronizes its stream before returning, so results
// are complete when the call returns.
static hipStream_t ordered_stream(ndfl_ctx* c) {
    if (!c->user_stream) {
        hipEventRecord(c->ev_order, nullptr);
        hipStreamWaitEvent(c->stream, c->ev_order, 0);
    }
    return c->stream;
}

// Raw CRC of `len` bytes from the raw CRCs of its consecutive parts of `part_len` bytes into *out.
static hipError_t launch_crc_combine(ndfl_ctx* c, hipStream_t s, const uint32_t* parts, uint32_t nparts,
                                     uint32_t part_len, uint64_t len, uint32_t* out) {
    hipError_t e = hipMemsetAsync(out, 0, 4, s);
    if (e != hipSuccess) return e;
    const uint32_t* p2 = c->d_tabs.as<uint32_t>() + 1024 + 64 + 1024;
    const uint32_t grid = std::max(1u, std::min(1024u, (nparts + 255) / 256));
    hipLaunchKernelGGL(ndfl_crc_combine_kernel, dim3(grid), dim3(256), 0, s, parts, nparts, part_len, len, p2, out);
    return hipGetLastError();
}

extern "C" {

uint32_t ndfl_abi_version(void) { return NDFL_ABI_VERSION; }

const char* ndfl_error_string(int code) {
    static const char* reasons[] = {
        "Unexpected end of stream", "Reserved block type", "len/nlen mismatch in uncompressed block",
        "This canonical code produces an under-full Huffman code tree",
        "This canonical code produces an over-full Huffman code tree", "No code length value to copy",
        "Run exceeds number of codes", "End-of-block symbol has zero code length", "Reserved run length symbol",
        "Reserved distance symbol", "Length symbol encountered with empty distance code",
        "Attempting to copy from before start of dictionary", "Header checksum mismatch",
        "Unsupported compression method", "Decompression checksum mismatch", "Decompressed size mismatch",
        "Invalid GZIP magic number", "Reserved flags are set", "Unsupported operating system value"};
    if (code == 0) return "ok";
    if (code >= 1 && code <= 19) return reasons[code - 1];
    switch (code) {
        case NDFL_E_ARG: return "invalid argument";
        case NDFL_E_UNSUPPORTED: return "configuration not supported on the GPU path";
        case NDFL_E_CAPACITY: return "output buffer too small";
        case NDFL_E_DEVICE: return "HIP device error";
        case NDFL_E_STATE: return "invalid state";
        default: return "internal error";
    }
}

int ndfl_ctx_create(ndfl_ctx** out, int device, uint32_t flags) {
    (void)flags;
    if (!out) return NDFL_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) return NDFL_E_DEVICE;
    HIPCHK(hipSetDevice(device));
    init_host_tables();
    ndfl_ctx* c = new ndfl_ctx();
    c->device = device;
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) c->ncu = 0;
    c->knobs.read();
    c->inf.knobs = c->knobs;
    if (c->knobs.stats) c->knobs.print(stderr);
    if (hipStreamCreateWithFlags(&c->own, hipStreamDefault) != hipSuccess) { delete c; return NDFL_E_DEVICE; }
    c->stream = c->own;
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    if (hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming) != hipSuccess) { delete c; return NDFL_E_DEVICE; }
    if (c->d_tabs.ensure(sizeof(host_crc_tab) + sizeof(host_crc_x) + sizeof(host_crc_p2)) != hipSuccess) { delete c; return NDFL_E_DEVICE; }
    hipMemcpy(c->d_tabs.p, host_crc_tab, sizeof(host_crc_tab), hipMemcpyHostToDevice);
    hipMemcpy((char*)c->d_tabs.p + sizeof(host_crc_tab), host_crc_x, sizeof(host_crc_x), hipMemcpyHostToDevice);
    hipMemcpy((char*)c->d_tabs.p + sizeof(host_crc_tab) + sizeof(host_crc_x), host_crc_p2, sizeof(host_crc_p2),
              hipMemcpyHostToDevice);
    if (hipHostMalloc((void**)&c->h_pinned, 4096, 0) != hipSuccess) { delete c; return NDFL_E_DEVICE; }
    *out = c;
    return NDFL_OK;
}

int ndfl_ctx_destroy(ndfl_ctx* c) {
    if (!c) return NDFL_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&c->d_in, &c->d_out, &c->d_status, &c->d_ticket, &c->d_edge_w, &c->d_edge_v,
                      &c->d_crc, &c->d_crc1, &c->d_tabs, &c->d_hostio, &c->d_lz, &c->d_link, &c->d_match,
                      &c->d_mdata, &c->d_masm, &c->d_hist, &c->d_codes, &c->d_off, &c->d_segtab, &c->d_bgzw};
    for (DevBuf* b : bufs) b->release();
    for (int k = 0; k < 16; k++) { c->d_mstreams[k].release(); c->d_mbits[k].release(); }
    c->inf.release();
    c->batch.release();
    c->bgzf.release();
    c->batch_lz.release();
    if (c->h_pinned) hipHostFree(c->h_pinned);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->ev_order) hipEventDestroy(c->ev_order);
    if (c->own) hipStreamDestroy(c->own);
    delete c;
    return NDFL_OK;
}

int ndfl_ctx_set_stream(ndfl_ctx* c, void* s) {
    if (!c) return NDFL_E_ARG;
    c->stream = s ? (hipStream_t)s : c->own;
    c->user_stream = s != nullptr;
    return NDFL_OK;
}

double ndfl_ctx_last_kernel_ms(ndfl_ctx* c) { return c ? c->last_ms : 0.0; }

int ndfl_ctx_timings(ndfl_ctx* c, double* ms, int n) {
    if (!c || !ms) return NDFL_E_ARG;
    double v[10] = {c->deflate_ms, c->inf.last_ms_find, c->inf.last_ms_count, c->inf.last_ms_emit,
                    c->inf.last_ms_wall, (double)c->inf.chains, (double)c->inf.repairs, (double)c->inf.candidates,
                    (double)c->inf.flat_chains, (double)c->inf.pending_after_dev};
    for (int i = 0; i < n && i < 10; i++) ms[i] = v[i];
    return n < 10 ? n : 10;
}

uint64_t ndfl_deflate_bound(uint64_t len, uint32_t chunk_len) {
    if (chunk_len == 0) return 0;
    uint64_t nch = len / chunk_len + 1;
    // per chunk: <= 9 bits per byte (+ EOB) + header (<= 4,500 bits) + word alignment slack
    return (9 * len + nch * 4640) / 8 + 64;
}

uint32_t ndfl_crc32_combine(uint32_t a, uint32_t b, uint64_t len_b) {
    return crc_multmodp(crc_x8n(len_b), a) ^ b;
}

}  // extern "C"

#include "ndfl_deflate_chunks.cpp"

extern "C" {

int ndfl_crc32(ndfl_ctx* c, uint32_t* crc_inout, const uint8_t* data, uint64_t len, uint32_t flags) {
    if (!c || !crc_inout || (!data && len)) return NDFL_E_ARG;
    if (len == 0) return NDFL_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = ordered_stream(c);
    const uint8_t* d = data;
    if (!(flags & NDFL_IN_DEVICE)) {
        HIPCHK(c->d_in.ensure(len));
        HIPCHK(hipMemcpyAsync(c->d_in.p, data, len, hipMemcpyHostToDevice, s));
        d = c->d_in.as<uint8_t>();
    }
    const uint64_t nseg = (len + 65535) / 65536;
    HIPCHK(c->d_crc.ensure(nseg * 4));
    HIPCHK(c->d_crc1.ensure(64));
    HIPCHK(hipEventRecord(c->ev0, s));
    hipLaunchKernelGGL(ndfl_crc_segments_kernel, dim3((uint32_t)nseg), dim3(1024), 0, s, d, len,
                       (const uint32_t*)c->d_tabs.as<uint32_t>(), (const uint32_t*)(c->d_tabs.as<uint32_t>() + 1024),
                       c->d_crc.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, s));
    HIPCHK(launch_crc_combine(c, s, (const uint32_t*)c->d_crc.as<uint32_t>(), (uint32_t)nseg, 65536u, len,
                              c->d_crc1.as<uint32_t>()));
    HIPCHK(hipMemcpyAsync(c->h_pinned, c->d_crc1.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->last_ms = ms;
    uint32_t raw = c->h_pinned[0];
    uint32_t dc = ~(crc_multmodp(crc_x8n(len), 0xFFFFFFFFu) ^ raw);
    *crc_inout = ndfl_crc32_combine(*crc_inout, dc, len);
    return NDFL_OK;
}

int ndfl_adler32(ndfl_ctx* c, uint32_t* adler_inout, const uint8_t* data, uint64_t len, uint32_t flags) {
    if (!c || !adler_inout || (!data && len)) return NDFL_E_ARG;
    if (len == 0) return NDFL_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = ordered_stream(c);
    const uint8_t* d = data;
    if (!(flags & NDFL_IN_DEVICE)) {
        HIPCHK(c->d_in.ensure(len));
        HIPCHK(hipMemcpyAsync(c->d_in.p, data, len, hipMemcpyHostToDevice, s));
        d = c->d_in.as<uint8_t>();
    }
    const uint64_t nseg = (len + 65535) / 65536;
    HIPCHK(c->d_crc.ensure(nseg * 8));
    HIPCHK(hipEventRecord(c->ev0, s));
    hipLaunchKernelGGL(ndfl_adler_segments_kernel, dim3((uint32_t)nseg), dim3(1024), 0, s, d, len, c->d_crc.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, s));
    std::vector<uint32_t> st(nseg * 2);
    HIPCHK(hipMemcpyAsync(st.data(), c->d_crc.p, nseg * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->last_ms = ms;
    uint64_t a = *adler_inout & 0xFFFF, b = *adler_inout >> 16;
    for (uint64_t k = 0; k < nseg; k++) {
        const uint64_t sl = std::min<uint64_t>(65536, len - k * 65536);
        b = (b + sl % 65521 * a + st[2 * k + 1]) % 65521;
        a = (a + st[2 * k]) % 65521;
    }
    *adler_inout = (uint32_t)(b << 16 | a);
    return NDFL_OK;
}

// A decode's Reason as it leaves the library: the decoder reports the second reserved symbol of each
// alphabet (length 287, distance 31) with an internal code; both become the reference's Reason, and
// the symbol -- which the reference puts in its message, "Reserved run length symbol: " + sym
// (D/decomp/Open.java:516, 659) and "Reserved distance symbol: " + sym (:550, 674) -- is kept for
// ndfl_ctx_error_symbol.
static int public_reason(ndfl_ctx* c, int r) {
    c->err_sym = -1;
    switch (r) {
        case inf::R_RESERVED_LEN: c->err_sym = 286; break;
        case inf::R_RESERVED_LEN_HI: c->err_sym = 287; r = inf::R_RESERVED_LEN; break;
        case inf::R_RESERVED_DIST: c->err_sym = 30; break;
        case inf::R_RESERVED_DIST_HI: c->err_sym = 31; r = inf::R_RESERVED_DIST; break;
        case inf::R_INTERNAL: r = NDFL_E_INTERNAL; break;   // (a failed consistency check, not the data)
        default: break;
    }
    return r;
}

int ndfl_ctx_error_symbol(ndfl_ctx* c) { return c ? c->err_sym : -1; }

// One decode of a filled-in frame, its results to the caller.
static int run_decode(ndfl_ctx* c, Decode& d, const uint8_t* in, uint64_t in_len, uint64_t* out_len, uint64_t* consumed_bits) {
    d.last_ms = &c->last_ms;
    const int r = d.run(in, in_len);
    *out_len = d.out_len;
    *consumed_bits = d.consumed_bits;
    return public_reason(c, r);
}

int ndfl_inflate(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                 uint64_t* out_len, uint64_t* consumed_bits, uint32_t flags) {
    if (!c || !out_len || !consumed_bits || (!in && in_len)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    Decode d{c->inf, ordered_stream(c)};
    d.out = out; d.out_cap = out_cap; d.flags = flags;
    return run_decode(c, d, in, in_len, out_len, consumed_bits);
}

}  // extern "C"

// The call-level rules of ndfl_inflate_batch and ndfl_inflate_members (n > 0): the pointers, every
// item inside its buffers, no two non-empty output regions overlapping.
template <class Item>
static bool batch_regions_valid(const uint8_t* in, uint64_t in_size, const uint8_t* out, uint64_t out_size,
                                const Item* items, const void* results, uint32_t n) {
    if (!items || !results || (!in && in_size) || (!out && out_size)) return false;
    std::vector<std::pair<uint64_t, uint64_t>> regions;          // non-empty output regions [off, end)
    regions.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        const Item& it = items[i];
        if (it.in_off > in_size || it.in_len > in_size - it.in_off) return false;
        if (it.out_off > out_size || it.out_cap > out_size - it.out_off) return false;
        if (it.out_cap) regions.emplace_back(it.out_off, it.out_off + it.out_cap);
    }
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); k++)
        if (regions[k].first < regions[k - 1].second) return false;
    return true;
}

// public_reason per stream: the kernel's internal codes become the Reason and the stream's symbol.
template <class Result>
static void batch_public_reasons(Result* results, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        Result& q = results[i];
        q.error_symbol = -1;
        switch (q.status) {
            case inf::R_RESERVED_LEN: q.error_symbol = 286; break;
            case inf::R_RESERVED_LEN_HI: q.error_symbol = 287; q.status = inf::R_RESERVED_LEN; break;
            case inf::R_RESERVED_DIST: q.error_symbol = 30; break;
            case inf::R_RESERVED_DIST_HI: q.error_symbol = 31; q.status = inf::R_RESERVED_DIST; break;
            case inf::R_INTERNAL: q.status = NDFL_E_INTERNAL; break;
            default: break;
        }
    }
}

// The per-item rule of the calls that take ndfl_member_item: a known format and checksum kind.
static bool member_items_valid(const ndfl_member_item* items, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (items[i].format > NDFL_FMT_GZIP || items[i].sum > NDFL_SUM_ADLER32) return false;
    return true;
}

// What the batched deflate calls check of their frame, in this order: chunk_len and
// hist_limit, the call-level rules, the items.
static int deflate_batch_args(const uint8_t* in, uint64_t in_size, const uint8_t* out, uint64_t out_size,
                              const ndfl_member_item* items, const void* results, uint32_t n, uint32_t chunk_len,
                              uint32_t hist_limit) {
    if (chunk_len == 0 || hist_limit > 32768) return NDFL_E_ARG;
    if (chunk_len > (uint32_t)MAX_CHUNK) return NDFL_E_UNSUPPORTED;
    if (!batch_regions_valid(in, in_size, out, out_size, items, results, n) || !member_items_valid(items, n))
        return NDFL_E_ARG;
    return NDFL_OK;
}

// A batch runner's (or inflate_headers') return code as the C ABI's: 0, the device error, else an internal one.
static int batch_status(int r) { return !r ? NDFL_OK : r == NDFL_E_DEVICE ? r : NDFL_E_INTERNAL; }

// How the four batched deflate calls end once their arguments are checked: the frame's arguments and the
// checksum tables into the launcher, which holds what is the call's own already, and the run.
template <class Launch>
static int deflate_batch_launch(ndfl_ctx* c, Launch& launch, const uint8_t* in, uint8_t* out, const ndfl_member_item* items,
                                ndfl_deflate_result* results, uint32_t n, uint32_t chunk_len, uint32_t flags) {
    HIPCHK(hipSetDevice(c->device));
    launch.a.n = n; launch.a.chunk_len = chunk_len; launch.a.crc_tab = c->d_tabs.as<uint32_t>();
    return batch_status(deflate_batch_run(c->batch, c->d_in, ordered_stream(c), c->ev0, c->ev1, in, out,
                                          items, results, n, flags, launch, &c->last_ms));
}

#include "ndfl_deflate_batch_chunked.cpp"
#include "ndfl_deflate_bgzf.cpp"

extern "C" {

int ndfl_inflate_batch(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                       const ndfl_batch_item* items, ndfl_batch_result* results, uint32_t n, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    if (!batch_regions_valid(in, in_size, out, out_size, items, results, n)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    const int r = batch_status(inflate_batch_run<false>(c->inf, c->batch, ordered_stream(c), c->ev0, c->ev1, in, in_size, out,
                                                        items, results, n, flags, &c->last_ms));
    if (r == NDFL_OK) batch_public_reasons(results, n);
    return r;
}

int ndfl_inflate_members(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                         const ndfl_member_item* items, ndfl_member_result* results, uint32_t n, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    if (!batch_regions_valid(in, in_size, out, out_size, items, results, n) || !member_items_valid(items, n))
        return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    const int r = batch_status(inflate_batch_run<true>(c->inf, c->batch, ordered_stream(c), c->ev0, c->ev1, in, in_size, out,
                                                       items, results, n, flags, &c->last_ms,
                                                       c->d_tabs.as<uint32_t>() + 1024));
    if (r == NDFL_OK) batch_public_reasons(results, n);
    return r;
}

int ndfl_inflate_bgzf(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                      ndfl_bgzf_result* result, ndfl_bgzf_member* table, uint32_t table_cap, uint32_t flags) {
    if (!c || !result || (!in && in_len) || (!out && out_cap) || (!table && table_cap)) return NDFL_E_ARG;
    if (in_len > (8ull << 30)) return NDFL_E_UNSUPPORTED;       // (candidate indices are 32-bit)
    HIPCHK(hipSetDevice(c->device));
    BgzfOutcome o;
    const int r = batch_status(inflate_bgzf_run(c->inf, c->batch, c->bgzf, ordered_stream(c), c->ev0, c->ev1, in, in_len,
                                                out, out_cap, &o, table, table_cap, flags, &c->last_ms,
                                                c->d_tabs.as<uint32_t>() + 1024));
    if (r != NDFL_OK) return r;
    ndfl_member_result one{};
    one.status = o.status;
    batch_public_reasons(&one, 1);
    result->status = one.status;
    result->error_symbol = one.error_symbol;
    result->n_members = o.n_members;
    result->bad_member = o.bad_member;
    result->out_len = o.out_len;
    result->consumed_bytes = o.consumed;
    return result->status;
}

int ndfl_deflate_batch(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                       const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n, int strategy,
                       uint32_t chunk_len, uint32_t hist_limit, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    BatchRleLaunch launch{c->knobs, dbat::Args{}};
    switch (strategy) {
        case NDFL_LITERAL_STATIC: launch.a.rle = 0; launch.a.dynamic = 0; break;
        case NDFL_LITERAL_DYNAMIC: launch.a.rle = 0; launch.a.dynamic = 1; break;
        case NDFL_RLE_STATIC: launch.a.rle = 1; launch.a.dynamic = 0; break;
        case NDFL_RLE_DYNAMIC: launch.a.rle = 1; launch.a.dynamic = 1; break;
        case NDFL_FULL_STATIC: case NDFL_FULL_DYNAMIC: case NDFL_UNCOMPRESSED: return NDFL_E_UNSUPPORTED;
        default: return NDFL_E_ARG;
    }
    if (const int e = deflate_batch_args(in, in_size, out, out_size, items, results, n, chunk_len, hist_limit)) return e;
    launch.a.hist_enabled = hist_limit > 0; launch.a.crc_x = c->d_tabs.as<uint32_t>() + 1024;
    return deflate_batch_launch(c, launch, in, out, items, results, n, chunk_len, flags);
}

int ndfl_deflate_batch_lz77(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                            const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n, int dynamic,
                            int min_run, int max_run, int min_dist, int max_dist, uint32_t chunk_len,
                            uint32_t hist_limit, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    const LzTuple t{min_run, max_run, min_dist, max_dist};
    if (!lz77_tuple_valid(t)) return NDFL_E_ARG;
    // the literal-only and the distance-1 forms are ndfl_deflate_batch's presets, as in ndfl_deflate_chunks_lz77
    const int preset = lz77_preset(t, dynamic);
    if (preset >= 0)
        return ndfl_deflate_batch(c, in, in_size, out, out_size, items, results, n, preset, chunk_len, hist_limit, flags);
    if (const int e = deflate_batch_args(in, in_size, out, out_size, items, results, n, chunk_len, hist_limit)) return e;
    BatchLzLaunch launch{c->batch_lz, c->knobs, items, dblz::Args{}};
    launch.a.hist_limit = hist_limit; launch.a.dynamic = dynamic != 0;
    launch.a.min_run = (uint32_t)min_run; launch.a.max_run = (uint32_t)max_run;
    launch.a.min_dist = (uint32_t)min_dist; launch.a.max_dist = (uint32_t)max_dist;
    return deflate_batch_launch(c, launch, in, out, items, results, n, chunk_len, flags);
}

int ndfl_deflate_batch_multi(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                             const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                             const ndfl_strategy_desc* strats, uint32_t n_strats, uint32_t chunk_len,
                             uint32_t hist_limit, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    if (!strats || n_strats == 0) return NDFL_E_ARG;                                            // (D/comp/MultiStrategy.java:25-26)
    if (n_strats > dbm::MAXC) return NDFL_E_UNSUPPORTED;
    for (uint32_t k = 0; k < n_strats; k++) {                       // as ndfl_deflate_chunks_multi
        if (strats[k].kind == NDFL_KIND_UNCOMPRESSED) continue;
        if (strats[k].kind != NDFL_KIND_LZ77 || !lz77_tuple_valid(desc_tuple(strats[k]))) return NDFL_E_ARG;
    }
    BatchMultiLaunch launch{{c->batch_lz, c->knobs, items, dbm::Args{}}};
    // one Lz77Huffman alone, or several equal ones: nothing to choose, ndfl_deflate_batch_lz77's stream
    if (launch.set_candidates(strats, n_strats) == 1 && !(launch.a.c_flags[0] & dbm::C_STORED)) {
        const ndfl_strategy_desc& d = strats[launch.a.c_flags[0] >> 8];
        return ndfl_deflate_batch_lz77(c, in, in_size, out, out_size, items, results, n, d.dynamic, d.min_run, d.max_run,
                                       d.min_dist, d.max_dist, chunk_len, hist_limit, flags);
    }
    if (const int e = deflate_batch_args(in, in_size, out, out_size, items, results, n, chunk_len, hist_limit)) return e;
    launch.a.hist_limit = hist_limit;
    return deflate_batch_launch(c, launch, in, out, items, results, n, chunk_len, flags);
}

int ndfl_deflate_batch_binsplit(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                                const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                                const ndfl_strategy_desc* sub, int32_t min_block_len, uint32_t chunk_len,
                                uint32_t hist_limit, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    if (!sub || min_block_len < 1) return NDFL_E_ARG;                                           // (D/comp/BinarySplit.java:23-24)
    // as ndfl_deflate_chunks_binsplit: the frame's checks, then the substrategy
    if (const int e = deflate_batch_args(in, in_size, out, out_size, items, results, n, chunk_len, hist_limit)) return e;
    if (sub->kind != NDFL_KIND_LZ77) return NDFL_E_UNSUPPORTED;     // position-independent substrategies only
    if (!lz77_tuple_valid(desc_tuple(*sub))) return NDFL_E_ARG;
    BatchBinsplitLaunch launch{{c->batch_lz, c->knobs, items, dbsp::Args{}}};
    launch.set_search(*sub);
    launch.a.hist_limit = hist_limit; launch.a.min_block = (uint32_t)min_block_len;
    return deflate_batch_launch(c, launch, in, out, items, results, n, chunk_len, flags);
}

int ndfl_inflate_range(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint64_t start_bit, uint64_t end_bit,
                       uint8_t* out, uint64_t dict_len, uint64_t out_cap, uint64_t* out_len, uint64_t* consumed_bits,
                       uint32_t flags) {
    if (!c || !out_len || !consumed_bits || (!in && in_len) || (!out && (dict_len || out_cap))) return NDFL_E_ARG;
    if (dict_len > 32768 || start_bit > in_len * 8 || end_bit <= start_bit) return NDFL_E_ARG;
    const bool deferred = (flags & NDFL_DICT_DEFERRED) != 0;
    const bool partial = (flags & NDFL_IN_PARTIAL) != 0;
    if (deferred && !(flags & NDFL_OUT_DEVICE)) return NDFL_E_ARG;
    if (partial && (deferred || end_bit != UINT64_MAX)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    Decode d{c->inf, ordered_stream(c)};
    d.start_bit = start_bit; d.end_bit = end_bit; d.out = out; d.dict_len = dict_len; d.out_cap = out_cap;
    d.flags = flags; d.deferred = deferred; d.partial = partial;
    return run_decode(c, d, in, in_len, out_len, consumed_bits);
}

int ndfl_inflate_sync(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint64_t from_bit, uint64_t window_bits,
                      uint64_t* sync_bit, uint32_t flags) {
    if (!c || !sync_bit || (!in && in_len) || from_bit > in_len * 8) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    Decode d{c->inf, ordered_stream(c)};                        // at or past from_bit, at most window_bits ahead
    d.start_bit = from_bit; d.end_bit = std::min(in_len * 8, from_bit + window_bits); d.flags = flags;
    return d.sync_probe(in, in_len, sync_bit);
}

int ndfl_inflate_headers(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint32_t flags, uint64_t* headers,
                         uint64_t cap, uint64_t* n_headers, uint64_t* survivors, uint64_t surv_cap, uint64_t* stats) {
    if (!c || !n_headers || (!in && in_len) || (!headers && cap) || (!survivors && surv_cap)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return batch_status(inflate_headers(c->inf, ordered_stream(c), in, in_len, flags, headers, cap, n_headers, survivors,
                                        surv_cap, stats));
}

int ndfl_inflate_resolve(ndfl_ctx* c, uint64_t* n_reemitted) {
    if (!c || !n_reemitted) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return inflate_resolve(c->inf, ordered_stream(c), n_reemitted);
}

int ndfl_inflate_tail(ndfl_ctx* c, uint64_t tail_len, uint8_t* dst) {
    if (!c || (!dst && tail_len)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return inflate_tail(c->inf, ordered_stream(c), tail_len, dst);
}

int ndfl_inflate_tail_map(ndfl_ctx* c, uint64_t tail_len, uint32_t* dst) {
    if (!c || (!dst && tail_len)) return NDFL_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return inflate_tail_map(c->inf, ordered_stream(c), tail_len, dst);
}

int ndfl_bits_shift(ndfl_ctx* c, const uint8_t* in, uint64_t nbits, uint32_t shift, uint8_t* out, uint64_t out_cap,
                    uint32_t flags) {
    if (!c || (!in && nbits) || !out || shift > 7) return NDFL_E_ARG;
    if ((flags & (NDFL_IN_DEVICE | NDFL_OUT_DEVICE)) != (NDFL_IN_DEVICE | NDFL_OUT_DEVICE)) return NDFL_E_ARG;
    const uint64_t nout = (nbits + shift + 7) / 8;
    if (nout > out_cap) return NDFL_E_CAPACITY;
    const uint64_t nin = (nbits + 7) / 8;
    if (nout && in < out + nout && out < in + nin) return NDFL_E_ARG;     // no in-place shifting
    if (nout == 0) return NDFL_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t nthr = (nout + 3) / 4;
    hipLaunchKernelGGL(ndfl_bits_shift_kernel, dim3((uint32_t)((nthr + 255) / 256)), dim3(256), 0, ordered_stream(c), in,
                       nbits, shift, out, nout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return NDFL_OK;
}

}  // extern "C"

#include "ndfl_plugin.cpp"
