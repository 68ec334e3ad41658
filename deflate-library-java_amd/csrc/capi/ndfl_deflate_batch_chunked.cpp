// ndfl_deflate_batch_chunked.cpp -- ndfl_deflate_batch_chunked of include/ndfl.h (included by
// ndfl_capi.cpp): many medium buffers through the chunk encoders, one 1024-thread workgroup per chunk,
// in a number of launches that does not depend on the number of buffers.
//
// Every stream gets a slot of whole chunks in the staged input (behind the LZ_DS lead the LZ kernels
// expect) and a word-aligned base in the staged output; a chunk table and a stream table
// (seg_tables.hpp), built on the host and uploaded once each, tell the segmented kernels what a chunk's
// index no longer does.  RLE/LITERAL tuples run hist -> codes -> offsets (scanned over all chunks, then
// restarted at each stream's base) -> emit; every other tuple runs parse-driven match -> encode per slab
// of staged data, the look-back restarting at each stream's first chunk.  Then the checksum partials of
// all chunks, their combination per stream, and the finishing pass (deflate_seg.hip); batch_run
// (inflate_batch.hip) carries the items, the results and host output as for the wave batches.
// seg_prepare and seg_encode are those stages up to the finishing pass; ndfl_deflate_bgzf
// (ndfl_deflate_bgzf.cpp) runs them too, with tables of its own and its own last passes.

// The tables of a batch.
struct SegTables {
    std::vector<SegChunk> chunks;
    std::vector<SegStream> streams;
    uint64_t staged = 0;                // bytes of the slots: chunks * chunk_len
    uint64_t out_bytes = 0;             // bytes of the staged output
    bool any_sum = false;               // some stream asks for a checksum
};

// A stream's bytes in the staged output: its bound, a trailer, and the words the encoders and the
// finishing pass may touch past them.
static uint64_t seg_out_slot(uint64_t len, uint32_t chunk_len) {
    return ((ndfl_deflate_bound(len, chunk_len) + 8 + 3) / 4 + 2) * 4;
}

// Builds the tables of n valid items (no HIP call: scripts/sanitize_chunked_host.cpp drives it on the
// CPU).  NDFL_E_UNSUPPORTED when the chunks do not fit 32 bits, before anything is allocated.
static int seg_build_tables(const ndfl_member_item* items, uint32_t n, uint32_t chunk_len, SegTables& T) {
    uint64_t nch = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = items[i].in_len;
        nch += len == 0 ? 1 : len / chunk_len + (len % chunk_len != 0);
        if (nch > 0xFFFFFFFFull) return NDFL_E_UNSUPPORTED;
    }
    T.chunks.resize(nch);
    T.streams.resize(n);
    T.staged = nch * chunk_len;
    T.any_sum = false;
    uint64_t k = 0, obase = 0;
    for (uint32_t i = 0; i < n; i++) {
        const ndfl_member_item& it = items[i];
        const uint64_t len = it.in_len;
        const uint32_t cnt = (uint32_t)(len == 0 ? 1 : len / chunk_len + (len % chunk_len != 0));
        const uint32_t kind = it.format == NDFL_FMT_ZLIB ? NDFL_SUM_ADLER32 : it.format == NDFL_FMT_GZIP ? NDFL_SUM_CRC32 : it.sum;
        T.any_sum = T.any_sum || kind != NDFL_SUM_NONE;
        T.streams[i] = SegStream{obase, (uint32_t)k, cnt};
        obase += seg_out_slot(len, chunk_len);
        for (uint32_t j = 0; j < cnt; j++) {
            const uint64_t at = (uint64_t)j * chunk_len;
            SegChunk& c = T.chunks[k + j];
            c.start = k * chunk_len;
            c.src = it.in_off + at;
            c.stream = i;
            c.len = (uint32_t)std::min<uint64_t>(chunk_len, len - at);
            c.flags = (j == 0 ? SEG_FIRST : 0u) | (j + 1 == cnt ? SEG_LAST : 0u) | kind << SEG_SUM_SHIFT;
            c.pad = 0;
        }
        k += cnt;
    }
    T.out_bytes = obase;
    return NDFL_OK;
}

// The RLE / LITERAL presets over all chunks (chunks_rle's split pipeline, segmented).
static int seg_launch_rle(ndfl_ctx* c, hipStream_t s, const SegTab tab, const uint8_t* slots, uint32_t nch, uint64_t staged,
                          uint32_t chunk_len, uint32_t hist_limit, int rle, int dyn, uint32_t* two_walks) {
    HIPCHK(c->d_hist.ensure((size_t)nch * HREC * 4));
    HIPCHK(c->d_codes.ensure((size_t)nch * CREC * 4));
    const uint32_t ntile = (nch + SCAN_TILE - 1) / SCAN_TILE;
    HIPCHK(c->d_off.ensure(((size_t)2 * nch + 8 + ntile) * 8));
    uint64_t* d_offs = c->d_off.as<uint64_t>();            // [nch] per stream | [nch] over all chunks | total | tile sums
    uint64_t* d_raw = d_offs + nch;
    uint64_t* d_total = d_raw + nch;
    uint64_t* d_part = d_total + 8;
    Args a;
    a.in = slots; a.n = staged; a.chunk_len = chunk_len; a.nchunks = nch;
    a.prev_byte = -1; a.hist_enabled = hist_limit > 0; a.final_last = 1;
    a.rle = rle; a.dynamic = dyn; a.base_bit = 0; a.parent_len = chunk_len;
    a.out = c->d_out.as<uint32_t>(); a.status = c->d_status.as<uint64_t>(); a.ticket = c->d_ticket.as<uint32_t>();
    a.edge_w = c->d_edge_w.as<uint64_t>(); a.edge_v = c->d_edge_v.as<uint32_t>();
    a.chunk_bits = nullptr; a.crc_raw = nullptr;
    a.crc_tab = c->d_tabs.as<uint32_t>(); a.crc_x = c->d_tabs.as<uint32_t>() + 1024;
    a.prof = nullptr;
    a.hist_out = c->d_hist.as<uint32_t>(); a.codes = c->d_codes.as<uint32_t>(); a.chunk_off = d_offs;
    a.c0 = 0;
    a.pf_dist = c->knobs.deflate_pf ? 2u * (uint32_t)c->ncu : 0u;
    a.onewalk = c->knobs.deflate_onewalk ? 1u : 0u;
    a.two_walks = two_walks;
    hipLaunchKernelGGL(ndfl_deflate_hist_seg_kernel, dim3(nch), dim3(1024), 0, s, a, tab);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_deflate_codes_seg_kernel, dim3(nch), dim3(64), 0, s, a, tab);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_deflate_offsets_sum_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint64_t*)a.status, nch, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_deflate_offsets_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint64_t*)a.status, nch,
                       (uint64_t)0, d_raw, d_total, (const uint64_t*)d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_deflate_offsets_seg_kernel, dim3((nch + 255) / 256), dim3(256), 0, s, (const uint64_t*)d_raw,
                       a.status, nch, tab, d_offs);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ndfl_deflate_emit_seg_kernel, dim3(nch), dim3(1024), 0, s, a, tab);
    HIPCHK(hipGetLastError());
    return NDFL_OK;
}

// Lz77Huffman over all chunks (chunks_lz's parse-driven search and encode, segmented), a slab of whole
// chunks at a time: matches take 4 bytes per staged byte.
static int seg_launch_lz(ndfl_ctx* c, hipStream_t s, const SegTab tab, const uint8_t* buf, uint32_t nch, uint64_t staged,
                         uint32_t chunk_len, uint32_t hist_limit, const LzTuple& t, int dyn) {
    const uint64_t total = LZ_DS + staged;
    const uint32_t slab_ch = (uint32_t)std::min<uint64_t>(nch, std::max<uint64_t>(1, c->knobs.seg_slab / chunk_len));
    HIPCHK(c->d_match.ensure((size_t)slab_ch * chunk_len * 4));
    LzArgs la;
    la.buf = buf; la.total = total; la.vstart = LZ_DS; la.chunk_len = chunk_len; la.parent_len = chunk_len;
    la.hist_limit = hist_limit; la.min_run = (uint32_t)t.min_run; la.max_run = (uint32_t)t.max_run;
    la.min_dist = (uint32_t)t.min_dist; la.max_dist = (uint32_t)t.max_dist;
    la.link = nullptr; la.L0 = 0; la.match = c->d_match.as<uint32_t>(); la.stats = nullptr;
    LzEncArgs ea;
    ea.match = c->d_match.as<uint32_t>(); ea.n = staged; ea.chunk_len = chunk_len; ea.nchunks = nch;
    ea.final_last = 1; ea.dynamic = dyn; ea.base_bit = 0;
    ea.out = c->d_out.as<uint32_t>(); ea.status = c->d_status.as<uint64_t>(); ea.ticket = c->d_ticket.as<uint32_t>();
    ea.edge_w = c->d_edge_w.as<uint64_t>(); ea.edge_v = c->d_edge_v.as<uint32_t>();
    ea.chunk_bits = nullptr; ea.match_rw = c->d_match.as<uint32_t>();
    ea.g.buf = buf; ea.g.total = total; ea.g.vstart = LZ_DS; ea.g.chunk_len = chunk_len; ea.g.parent_len = chunk_len;
    ea.g.hist_limit = hist_limit; ea.g.min_run = la.min_run; ea.g.max_run = la.max_run; ea.g.min_dist = la.min_dist;
    ea.g.max_dist = la.max_dist;
    ea.stats = nullptr;
    const uint32_t lead_on = c->knobs.lz_lead == 0 ? 0u : 1u;
    for (uint32_t cb = 0; cb < nch; cb += slab_ch) {
        const uint32_t ce = (uint32_t)std::min<uint64_t>(nch, (uint64_t)cb + slab_ch);
        const uint64_t x0 = (uint64_t)cb * chunk_len, x1 = (uint64_t)ce * chunk_len;
        la.p_begin = LZ_DS + x0; la.p_end = LZ_DS + x1;
        hipLaunchKernelGGL(ndfl_lz_parse_match_seg_kernel, dim3((uint32_t)((x1 - x0 + LZP_TILE - 1) / LZP_TILE)), dim3(1024), 0,
                           s, la, lead_on, tab);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(c->d_ticket.p, 0, 64, s));
        ea.batch_x0 = x0; ea.chunk_base = cb; ea.nchunks_batch = ce - cb;
        hipLaunchKernelGGL(ndfl_lz_encode_seg_kernel, dim3(ce - cb), dim3(1024), 0, s, ea, tab);
        HIPCHK(hipGetLastError());
    }
    return NDFL_OK;
}

// The context's buffers of a segmented run over nch chunks of n streams, grown to its sizes, and the staged
// input's frame [LZ_DS zero bytes | the slots, `staged` bytes, not written here | 64 zero bytes]: *buf.
static int seg_prepare(ndfl_ctx* c, hipStream_t s, uint32_t nch, uint32_t n, uint64_t staged, uint64_t out_bytes,
                       uint8_t** buf) {
    HIPCHK(c->d_lz.ensure(LZ_DS + staged + 64));
    *buf = c->d_lz.as<uint8_t>();
    HIPCHK(hipMemsetAsync(*buf, 0, LZ_DS, s));
    HIPCHK(hipMemsetAsync(*buf + LZ_DS + staged, 0, 64, s));
    HIPCHK(c->d_out.ensure(out_bytes));
    HIPCHK(c->d_status.ensure(std::max<size_t>(8, nch * sizeof(uint64_t))));
    HIPCHK(c->d_ticket.ensure(64));
    HIPCHK(c->d_edge_w.ensure(2ull * nch * sizeof(uint64_t)));
    HIPCHK(c->d_edge_v.ensure(2ull * nch * sizeof(uint32_t)));
    HIPCHK(c->d_crc.ensure(2ull * nch * sizeof(uint32_t)));
    HIPCHK(c->d_crc1.ensure(std::max<size_t>(64, (size_t)n * sizeof(uint32_t))));
    return NDFL_OK;
}

// The launches of a segmented run on stream q, the slots filled and the tables on the device: the encoders
// of the tuple over all chunks, the edge fix-up, and the streams' checksums into c->d_crc1 (zeros without
// any_sum; d_items: the streams' lengths, on the device).  What is left is the pass that takes every stream
// out of the staged output: its end is its last chunk's status word.
static int seg_encode(ndfl_ctx* c, hipStream_t q, const SegTab tab, uint8_t* buf, uint32_t nch, uint64_t staged,
                      uint32_t chunk_len, uint32_t hist_limit, const LzTuple& t, int dynamic, bool any_sum,
                      const ndfl_member_item* d_items, uint32_t n, uint32_t* two_walks) {
    uint8_t* slots = buf + LZ_DS;
    const int preset = lz77_preset(t, dynamic);
    HIPCHK(hipMemsetAsync(c->d_status.p, 0, nch * sizeof(uint64_t), q));
    if (two_walks) HIPCHK(hipMemsetAsync(two_walks, 0, 64, q));
    if (preset >= 0)
        TRY(seg_launch_rle(c, q, tab, slots, nch, staged, chunk_len, hist_limit,
                           preset == NDFL_RLE_STATIC || preset == NDFL_RLE_DYNAMIC, dynamic != 0, two_walks));
    else
        TRY(seg_launch_lz(c, q, tab, buf, nch, staged, chunk_len, hist_limit, t, dynamic != 0));
    const uint32_t ne = 2 * nch;
    hipLaunchKernelGGL(ndfl_edge_fixup_kernel, dim3((ne + 255) / 256), dim3(256), 0, q, (const uint64_t*)c->d_edge_w.p,
                       (const uint32_t*)c->d_edge_v.p, ne, c->d_out.as<uint32_t>());
    HIPCHK(hipGetLastError());
    uint32_t* d_sums = c->d_crc1.as<uint32_t>();
    if (any_sum) {
        hipLaunchKernelGGL(ndfl_seg_sums_kernel, dim3(nch), dim3(1024), 0, q, (const uint8_t*)slots, chunk_len, tab,
                           (const uint32_t*)c->d_tabs.as<uint32_t>(), (const uint32_t*)(c->d_tabs.as<uint32_t>() + 1024),
                           c->d_crc.as<uint32_t>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ndfl_seg_sums_combine_kernel, dim3((uint32_t)(((uint64_t)n * 64 + 255) / 256)), dim3(256), 0, q,
                           (const uint32_t*)c->d_crc.p, chunk_len, tab, d_items, n,
                           (const uint32_t*)(c->d_tabs.as<uint32_t>() + 1024 + 64 + 1024), d_sums);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemsetAsync(d_sums, 0, (size_t)n * sizeof(uint32_t), q));
    }
    return NDFL_OK;
}

// The call, its arguments checked: tables, staged input, then everything else between batch_run's events.
static int deflate_batch_chunked_run(ndfl_ctx* c, const uint8_t* in, uint8_t* out, const ndfl_member_item* items,
                                     ndfl_deflate_result* results, uint32_t n, const LzTuple& t, int dynamic,
                                     uint32_t chunk_len, uint32_t hist_limit, uint32_t flags) {
    SegTables T;
    TRY(seg_build_tables(items, n, chunk_len, T));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = ordered_stream(c);
    if (T.chunks.size() > 0x7FFFFFFFull) return NDFL_E_UNSUPPORTED;   // (the edge list holds two entries per chunk)
    const uint32_t nch = (uint32_t)T.chunks.size();
    const size_t chunks_b = (size_t)nch * sizeof(SegChunk), streams_b = (size_t)n * sizeof(SegStream);
    HIPCHK(c->d_segtab.ensure(chunks_b + streams_b));
    HIPCHK(hipMemcpyAsync(c->d_segtab.p, T.chunks.data(), chunks_b, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((char*)c->d_segtab.p + chunks_b, T.streams.data(), streams_b, hipMemcpyHostToDevice, s));
    SegTab tab;
    tab.chunks = c->d_segtab.as<SegChunk>();
    tab.streams = (const SegStream*)((char*)c->d_segtab.p + chunks_b);

    uint8_t* buf = nullptr;
    TRY(seg_prepare(c, s, nch, n, T.staged, T.out_bytes, &buf));
    uint8_t* slots = buf + LZ_DS;
    std::unique_ptr<uint8_t[]> pack;                        // host input, packed: alive until batch_run has waited
    if (flags & NDFL_IN_DEVICE) {
        hipLaunchKernelGGL(ndfl_seg_gather_kernel, dim3(nch), dim3(256), 0, s, in, slots, tab, chunk_len);
        HIPCHK(hipGetLastError());
    } else {
        pack.reset(new (std::nothrow) uint8_t[T.staged]);
        if (!pack) return NDFL_E_INTERNAL;
        for (uint32_t k = 0; k < nch; k++) {
            const SegChunk& ch = T.chunks[k];
            uint8_t* dst = pack.get() + (uint64_t)k * chunk_len;
            if (ch.len) memcpy(dst, in + ch.src, ch.len);
            if (ch.len < chunk_len) memset(dst + ch.len, 0, chunk_len - ch.len);
        }
        HIPCHK(hipMemcpyAsync(slots, pack.get(), T.staged, hipMemcpyHostToDevice, s));
    }

    ScopedBuf two_walks;                // NDFL_STATS: the emit pass's chunks that took two walks
    if (c->knobs.stats && lz77_preset(t, dynamic) >= 0) HIPCHK(two_walks.ensure(64));

    auto launch = [&](hipStream_t q, uint8_t* d_out, const ndfl_member_item* d_items, ndfl_deflate_result* d_res,
                      uint32_t*) -> int {
        TRY(seg_encode(c, q, tab, buf, nch, T.staged, chunk_len, hist_limit, t, dynamic, T.any_sum, d_items, n,
                       two_walks.as<uint32_t>()));
        hipLaunchKernelGGL(ndfl_seg_finish_kernel, dim3(n), dim3(1024), 0, q, c->d_out.as<uint8_t>(),
                           (const uint64_t*)c->d_status.p, tab, d_items, (const uint32_t*)c->d_crc1.p, d_out, d_res);
        return NDFL_OK;
    };
    const int rc = batch_status(batch_run(c->batch, s, c->ev0, c->ev1, out, items, results, n, flags, &c->last_ms, launch));
    if (two_walks.p && rc == NDFL_OK) {                     // (batch_run has waited for the launches)
        uint32_t tw = 0;
        HIPCHK(hipMemcpy(&tw, two_walks.p, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "[ndfl] deflate emit: %u chunks, %u took two walks\n", nch, tw);
    }
    return rc;
}

extern "C" int ndfl_deflate_batch_chunked(ndfl_ctx* c, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                                          const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                                          int dynamic, int min_run, int max_run, int min_dist, int max_dist,
                                          uint32_t chunk_len, uint32_t hist_limit, uint32_t flags) {
    if (!c) return NDFL_E_ARG;
    if (n == 0) return NDFL_OK;
    const LzTuple t{min_run, max_run, min_dist, max_dist};
    if (!lz77_tuple_valid(t)) return NDFL_E_ARG;
    if (const int e = deflate_batch_args(in, in_size, out, out_size, items, results, n, chunk_len, hist_limit)) return e;
    return deflate_batch_chunked_run(c, in, out, items, results, n, t, dynamic, chunk_len, hist_limit, flags);
}
