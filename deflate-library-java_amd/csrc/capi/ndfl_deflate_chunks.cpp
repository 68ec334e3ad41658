// ndfl_deflate_chunks.cpp -- the four chunked deflate calls of include/ndfl.h (included by
// ndfl_capi.cpp).  Every call is a Frame; chunks_rle and chunks_lz write a frame's stream and
// encode_chunks picks one of them; MultiStrategy and BinarySplit run it on sub-frames.
#define TRY(x) do { if (const int _rc = (x)) return _rc; } while (0)

// The Lz77Huffman parameters, of the C ABI's arguments or of a strategy descriptor.
struct LzTuple {
    int min_run, max_run, min_dist, max_dist;
    bool literal_only() const { return min_run == 0 && max_run == 0 && min_dist == 0 && max_dist == 0; }   // (:29-31)
};
static LzTuple desc_tuple(const ndfl_strategy_desc& d) { return LzTuple{d.min_run, d.max_run, d.min_dist, d.max_dist}; }

// The record's rule (D/comp/Lz77Huffman.java:28-38).
static bool lz77_tuple_valid(const LzTuple& t) {
    const int min_run = t.min_run, max_run = t.max_run, min_dist = t.min_dist, max_dist = t.max_dist;
    return t.literal_only() || (3 <= min_run && min_run <= max_run && max_run <= 258 && 1 <= min_dist &&
                                min_dist <= max_dist && max_dist <= 32768);
}

// The preset a valid tuple is -- literals only, or every run at distance 1: the RLE/LITERAL
// encoders take those -- else -1.
static int lz77_preset(const LzTuple& t, int dynamic) {
    if (t.literal_only()) return dynamic ? NDFL_LITERAL_DYNAMIC : NDFL_LITERAL_STATIC;
    if (t.min_run == 3 && t.max_run == 258 && t.min_dist == 1 && t.max_dist == 1)
        return dynamic ? NDFL_RLE_DYNAMIC : NDFL_RLE_STATIC;
    return -1;
}

// What an encoder does for the strategy above it.
struct BlockOpts {
    uint64_t* chunk_bits = nullptr;     // device, optional: per chunk, the bits of its block
    uint32_t parent_len = 0;            // BinarySplit's sub-blocks: their history starts at their parent's (0: chunk_len)
};

// One chunked deflate call, or one sub-encode of one: its arguments, its stream, its output.
struct Frame {
    ndfl_ctx* c;
    const uint8_t* hist; uint32_t hist_len, hist_limit;
    const uint8_t* data; uint64_t len; uint32_t chunk_len;
    int final_flag; uint32_t start_bitpos;
    uint8_t* out; uint64_t out_cap; uint64_t* out_end_bits; uint32_t* crc_inout; uint32_t flags;
    hipStream_t s = nullptr;            // begin()
    uint32_t nch = 0;                   // count_chunks()
    uint32_t* d_out = nullptr;          // place(): where the kernels write the stream
    bool direct = false;                //          ... which is the caller's buffer itself
    uint64_t end_bits = 0;              // set_end()

    bool pointers_ok() const { return c && out_end_bits && (data || !len) && (hist || !hist_len) && out; }
    // The argument rules the four calls share: NDFL_E_ARG for a broken one, then the kernels' chunk length.
    int check() const {
        if (!pointers_ok()) return NDFL_E_ARG;
        if (start_bitpos > 7 || hist_limit > 32768 || hist_len > hist_limit || chunk_len == 0) return NDFL_E_ARG;
        if (!final_flag && (len == 0 || len % chunk_len != 0)) return NDFL_E_ARG;
        if (chunk_len > (uint32_t)MAX_CHUNK) return NDFL_E_UNSUPPORTED;
        return NDFL_OK;
    }

    int begin() { HIPCHK(hipSetDevice(c->device)); s = ordered_stream(c); return NDFL_OK; }
    int count_chunks() {
        const uint64_t n = final_flag ? (len == 0 ? 1 : (len + chunk_len - 1) / chunk_len) : len / chunk_len;
        if (n > 0xFFFFFFFFull) return NDFL_E_UNSUPPORTED;
        nch = (uint32_t)n;
        return NDFL_OK;
    }

    // A sub-encode (MultiStrategy's candidates, BinarySplit's levels and nodes): device in and out, bit 0, no CRC.
    Frame sub(const uint8_t* h, uint32_t hl, uint32_t hlim, const uint8_t* d, uint64_t n, uint32_t blk, int fin,
              uint8_t* dst, uint64_t cap) const {
        Frame f{c, h, hl, hlim, d, n, blk, fin, 0, dst, cap, nullptr, nullptr, NDFL_IN_DEVICE | NDFL_OUT_DEVICE};
        f.s = s;
        return f;
    }

    // The words an encoder of whole chunks may write: ndfl_deflate_bound plus the edge words.
    uint64_t bound_words() const { return (ndfl_deflate_bound(len, chunk_len) + 3) / 4 + 2; }
    // The output of `words` 32-bit words: the caller's device buffer where it is aligned and holds
    // them all -- the kernels then write the stream in place -- else the context's staging buffer.
    int place(uint64_t words, bool zeroed) {
        direct = (flags & NDFL_OUT_DEVICE) && (((uintptr_t)out & 3) == 0) && out_cap >= words * 4;
        if (direct) d_out = (uint32_t*)out;
        else { HIPCHK(c->d_out.ensure(words * 4)); d_out = c->d_out.as<uint32_t>(); }
        if (zeroed) HIPCHK(hipMemsetAsync(d_out, 0, words * 4, s));
        return NDFL_OK;
    }

    // place() for an encoder of whole chunks, with the chunks' look-back status and edge records.
    int place_chunks() {
        TRY(place(bound_words(), false));
        HIPCHK(c->d_status.ensure(nch * sizeof(uint64_t)));
        HIPCHK(c->d_ticket.ensure(64));
        HIPCHK(c->d_edge_w.ensure(2ull * nch * sizeof(uint64_t)));
        HIPCHK(c->d_edge_v.ensure(2ull * nch * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(c->d_status.p, 0, nch * sizeof(uint64_t), s));
        return NDFL_OK;
    }

    // The encode kernels run between these two (ndfl_ctx_last_kernel_ms, ndfl_ctx_timings[0]).
    int start_timing() { HIPCHK(hipEventRecord(c->ev0, s)); return NDFL_OK; }
    int stop_timing() { HIPCHK(hipEventRecord(c->ev1, s)); return NDFL_OK; }
    void set_end(uint64_t bits) { end_bits = bits; if (out_end_bits) *out_end_bits = bits; }

    // A timed encode's end: waits for the work, takes the kernels' time, reads the end from status word `d_word`.
    int read_end(const uint64_t* d_word) {
        HIPCHK(hipMemcpyAsync(c->h_pinned, d_word, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0;
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        c->last_ms = c->deflate_ms = ms;
        uint64_t st;
        memcpy(&st, c->h_pinned, 8);
        set_end(st & ST_VAL);
        return NDFL_OK;
    }

    // CRC-32 of the call's data, which is on the device at `d` (the encoders that do not fuse it).
    int crc_of(const uint8_t* d) { return crc_inout ? ndfl_crc32(c, crc_inout, d, len, NDFL_IN_DEVICE) : NDFL_OK; }

    // The tail, after set_end: a staged stream must fit the caller's buffer and is copied there.
    int finish() {
        if (direct) return NDFL_OK;
        const uint64_t nbytes = (end_bits + 7) / 8;
        if (nbytes > out_cap) return NDFL_E_CAPACITY;
        HIPCHK(hipMemcpyAsync(out, d_out, nbytes,
                              (flags & NDFL_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return NDFL_OK;
    }
};

// The RLE / LITERAL presets over the frame's chunks (deflate_kernels.hip, deflate_split.hip), the CRC
// fused into the first pass.
static int chunks_rle(Frame& f, int rle, int dyn, BlockOpts o) {
    ndfl_ctx* c = f.c;
    hipStream_t s = f.s;
    const uint32_t nch = f.nch;
    const uint8_t* d_data = f.data;
    int prev_byte = -1;
    if (f.hist_len > 0 && (f.flags & NDFL_IN_DEVICE)) {
        uint8_t pb = 0;
        HIPCHK(hipMemcpyAsync(&pb, f.hist + f.hist_len - 1, 1, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        prev_byte = pb;
    } else if (f.hist_len > 0) {
        prev_byte = f.hist[f.hist_len - 1];
    }
    if (!(f.flags & NDFL_IN_DEVICE) && f.len) {
        HIPCHK(c->d_in.ensure(f.len));
        HIPCHK(hipMemcpyAsync(c->d_in.p, f.data, f.len, hipMemcpyHostToDevice, s));
        d_data = c->d_in.as<uint8_t>();
    }
    TRY(f.place_chunks());
    if (f.crc_inout) { HIPCHK(c->d_crc.ensure(nch * sizeof(uint32_t))); HIPCHK(c->d_crc1.ensure(64)); }
    HIPCHK(hipMemsetAsync(c->d_ticket.p, 0, 64, s));

    Args a;
    a.in = d_data; a.n = f.len; a.chunk_len = f.chunk_len; a.nchunks = nch;
    a.prev_byte = prev_byte; a.hist_enabled = f.hist_limit > 0; a.final_last = f.final_flag ? 1 : 0;
    a.rle = rle; a.dynamic = dyn; a.base_bit = f.start_bitpos;
    a.parent_len = o.parent_len ? o.parent_len : f.chunk_len;
    a.out = f.d_out; a.status = c->d_status.as<uint64_t>(); a.ticket = c->d_ticket.as<uint32_t>();
    a.edge_w = c->d_edge_w.as<uint64_t>(); a.edge_v = c->d_edge_v.as<uint32_t>();
    a.chunk_bits = o.chunk_bits;
    a.crc_raw = f.crc_inout ? c->d_crc.as<uint32_t>() : nullptr;
    a.crc_tab = c->d_tabs.as<uint32_t>();
    a.crc_x = c->d_tabs.as<uint32_t>() + 1024;
    ScopedBuf prof;                     // NDFL_DEFLATE_PROFILE: per-chunk phase timestamps
    if (c->knobs.deflate_profile) {
        HIPCHK(prof.ensure((size_t)nch * 64));
        HIPCHK(hipMemsetAsync(prof.p, 0, (size_t)nch * 64, s));
    }
    a.prof = prof.as<uint64_t>();
    a.hist_out = nullptr; a.codes = nullptr; a.chunk_off = nullptr;
    // next generation of resident split-pass workgroups: 2 per CU (1024 threads, <= 75 KB LDS)
    a.pf_dist = c->knobs.deflate_pf ? 2u * (uint32_t)c->ncu : 0u;      // (NDFL_DEFLATE_PF=0: no L2 touch)
    // split pipeline by default (deflate_split.hip); NDFL_DEFLATE_FUSED=1 (or the per-phase profile)
    // selects the one-kernel encoder
    const bool split = !c->knobs.deflate_fused && !prof.p;
    uint64_t* d_total = nullptr;
    if (split) {
        HIPCHK(c->d_hist.ensure((size_t)nch * HREC * 4));
        HIPCHK(c->d_codes.ensure((size_t)nch * CREC * 4));
        HIPCHK(c->d_off.ensure((size_t)nch * 8 + 64 + (size_t)((nch + SCAN_TILE - 1) / SCAN_TILE) * 8));
        a.hist_out = c->d_hist.as<uint32_t>();
        a.codes = c->d_codes.as<uint32_t>();
        a.chunk_off = c->d_off.as<uint64_t>();
        d_total = c->d_off.as<uint64_t>() + nch;
    }
    a.c0 = 0;
    a.onewalk = c->knobs.deflate_onewalk ? 1u : 0u;
    ScopedBuf two_walks;                // NDFL_STATS: the emit pass's chunks that took two walks
    if (c->knobs.stats && split) {
        HIPCHK(two_walks.ensure(64));
        HIPCHK(hipMemsetAsync(two_walks.p, 0, 64, s));
    }
    a.two_walks = two_walks.as<uint32_t>();
    TRY(f.start_timing());
    if (split) {
        hipLaunchKernelGGL(ndfl_deflate_hist_kernel, dim3(nch), dim3(1024), 0, s, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ndfl_deflate_codes_kernel, dim3(nch), dim3(64), 0, s, a);
        HIPCHK(hipGetLastError());
        const uint32_t ntile = (nch + SCAN_TILE - 1) / SCAN_TILE;
        uint64_t* d_part = c->d_off.as<uint64_t>() + nch + 8;
        hipLaunchKernelGGL(ndfl_deflate_offsets_sum_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint64_t*)a.status,
                           nch, d_part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ndfl_deflate_offsets_kernel, dim3(ntile), dim3(SCAN_T), 0, s, (const uint64_t*)a.status, nch,
                           (uint64_t)f.start_bitpos, c->d_off.as<uint64_t>(), d_total, (const uint64_t*)d_part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ndfl_deflate_emit_kernel, dim3(nch), dim3(1024), 0, s, a);
    } else {
        hipLaunchKernelGGL(ndfl_deflate_chunks_kernel, dim3(nch), dim3(1024), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    TRY(f.stop_timing());
    const uint32_t ne = 2 * nch;
    hipLaunchKernelGGL(ndfl_edge_fixup_kernel, dim3((ne + 255) / 256), dim3(256), 0, s,
                       (const uint64_t*)a.edge_w, (const uint32_t*)a.edge_v, ne, f.d_out);
    HIPCHK(hipGetLastError());
    if (f.crc_inout) {
        HIPCHK(launch_crc_combine(c, s, (const uint32_t*)a.crc_raw, nch, f.chunk_len, f.len, c->d_crc1.as<uint32_t>()));
        HIPCHK(hipMemcpyAsync(c->h_pinned + 4, c->d_crc1.p, 4, hipMemcpyDeviceToHost, s));
    }
    TRY(f.read_end(split ? d_total : a.status + (nch - 1)));
    if (two_walks.p) {
        uint32_t tw = 0;
        HIPCHK(hipMemcpy(&tw, two_walks.p, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "[ndfl] deflate emit: %u chunks, %u took two walks\n", nch, tw);
    }
    if (prof.p) {
        std::vector<uint64_t> h((size_t)nch * 8);
        HIPCHK(hipMemcpy(h.data(), prof.p, (size_t)nch * 64, hipMemcpyDeviceToHost));
        double sum[7] = {0}, tmin = 1e300, tmax = 0;
        for (uint32_t k = 0; k < nch; k++) {
            const uint64_t* q = &h[k * 8];
            for (int p = 0; p < 7; p++) sum[p] += (double)(q[p + 1] - q[p]);
            tmin = std::min(tmin, (double)q[0]); tmax = std::max(tmax, (double)q[7]);
        }
        // wall_clock64 runs at 100 MHz
        fprintf(stderr, "[ndfl] deflate phases (us/chunk): load+crc %.2f hist %.2f codes %.2f bits+scan %.2f emit %.2f "
                "lookback %.2f store %.2f; span %.2f ms\n", sum[0] / nch / 100, sum[1] / nch / 100, sum[2] / nch / 100,
                sum[3] / nch / 100, sum[4] / nch / 100, sum[5] / nch / 100, sum[6] / nch / 100, (tmax - tmin) / 1e5);
    }
    if (f.crc_inout) {
        uint32_t raw = c->h_pinned[4];
        uint32_t dc = ~(crc_multmodp(crc_x8n(f.len), 0xFFFFFFFFu) ^ raw);
        *f.crc_inout = ndfl_crc32_combine(*f.crc_inout, dc, f.len);
    }
    return f.finish();
}

// Lz77Huffman(dynamic, minRun, maxRun, minDist, maxDist) over the frame's chunks
// (D/comp/Lz77Huffman.java:20-130): staging copy, then per batch of chunks links -> matches ->
// parse/encode; edges and CRC at the end.
static int chunks_lz(Frame& f, const LzTuple& t, int dyn, BlockOpts o) {
    ndfl_ctx* c = f.c;
    hipStream_t s = f.s;
    const uint32_t nch = f.nch, chunk_len = f.chunk_len;
    const uint64_t len = f.len;
    // staging buffer: data at LZ_DS, the history right before it
    const uint64_t total = LZ_DS + len;
    HIPCHK(c->d_lz.ensure(total + 64));
    uint8_t* buf = c->d_lz.as<uint8_t>();
    const hipMemcpyKind kin = (f.flags & NDFL_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (f.hist_len) HIPCHK(hipMemcpyAsync(buf + LZ_DS - f.hist_len, f.hist, f.hist_len, kin, s));
    if (len) HIPCHK(hipMemcpyAsync(buf + LZ_DS, f.data, len, kin, s));
    HIPCHK(hipMemsetAsync(buf + total, 0, 64, s));

    TRY(f.place_chunks());

    // batches of whole chunks, <= 256 MiB of data each (matches: 4 B per byte, links: 2 B)
    const uint32_t batch_ch = std::max<uint32_t>(1, (uint32_t)((256ull << 20) / chunk_len));
    const uint64_t batch_bytes = std::min<uint64_t>((uint64_t)batch_ch * chunk_len, std::max<uint64_t>(len, 1));
    HIPCHK(c->d_match.ensure(batch_bytes * 4));
    HIPCHK(c->d_link.ensure((batch_bytes + LZ_SEG) * 2));

    LzArgs la;
    la.buf = buf; la.total = total; la.vstart = LZ_DS - f.hist_len; la.chunk_len = chunk_len;
    la.parent_len = o.parent_len ? o.parent_len : chunk_len;
    la.hist_limit = f.hist_limit; la.min_run = (uint32_t)t.min_run; la.max_run = (uint32_t)t.max_run;
    la.min_dist = (uint32_t)t.min_dist; la.max_dist = (uint32_t)t.max_dist;
    la.link = c->d_link.as<uint16_t>(); la.match = c->d_match.as<uint32_t>();
    ScopedBuf stats;                    // NDFL_LZ_STATS: the kernels' counters
    if (c->knobs.lz_stats) {
        HIPCHK(stats.ensure(128));
        HIPCHK(hipMemsetAsync(stats.p, 0, 128, s));
    }
    la.stats = stats.as<unsigned long long>();
    LzEncArgs ea;
    ea.match = c->d_match.as<uint32_t>(); ea.n = len; ea.chunk_len = chunk_len; ea.nchunks = nch;
    ea.final_last = f.final_flag ? 1 : 0; ea.dynamic = dyn; ea.base_bit = f.start_bitpos;
    ea.out = f.d_out; ea.status = c->d_status.as<uint64_t>(); ea.ticket = c->d_ticket.as<uint32_t>();
    ea.edge_w = c->d_edge_w.as<uint64_t>(); ea.edge_v = c->d_edge_v.as<uint32_t>();
    ea.chunk_bits = o.chunk_bits;
    ea.match_rw = c->d_match.as<uint32_t>();
    ea.g.buf = buf; ea.g.total = total; ea.g.vstart = la.vstart; ea.g.chunk_len = chunk_len;
    ea.g.parent_len = la.parent_len; ea.g.hist_limit = f.hist_limit; ea.g.min_run = la.min_run;
    ea.g.max_run = la.max_run; ea.g.min_dist = la.min_dist; ea.g.max_dist = la.max_dist;
    ea.stats = la.stats;
    // match search: at the positions the greedy parse visits (default), or at every position by hash
    // chains (NDFL_LZ_SEARCH=chain, the round-3 search); NDFL_LZ_LEAD=0 drops the tiles' lead-in (so
    // the encode kernel's fallback search runs at most tile starts: a test of that path)
    const bool chain_search = c->knobs.lz_chain;
    const uint32_t lead_on = c->knobs.lz_lead == 0 ? 0u : 1u;

    TRY(f.start_timing());
    for (uint32_t cb = 0; cb < nch; cb += batch_ch) {
        const uint32_t ce = std::min(nch, cb + batch_ch);
        const uint64_t x0 = (uint64_t)cb * chunk_len, x1 = std::min<uint64_t>((uint64_t)ce * chunk_len, len);
        const uint64_t P0 = LZ_DS + x0, P1 = LZ_DS + x1;
        if (P1 > P0 && !chain_search) {
            la.L0 = P0; la.p_begin = P0; la.p_end = P1;
            hipLaunchKernelGGL(ndfl_lz_parse_match_kernel, dim3((uint32_t)((P1 - P0 + LZP_TILE - 1) / LZP_TILE)), dim3(1024),
                               0, s, la, lead_on);
            HIPCHK(hipGetLastError());
        } else if (P1 > P0) {
            const uint64_t L0 = std::max<uint64_t>(la.vstart, P0 - LZ_SEG);
            hipLaunchKernelGGL(ndfl_lz_links_kernel, dim3((uint32_t)((P1 - L0 + LZ_SEG - 1) / LZ_SEG)), dim3(1024), 0, s,
                               (const uint8_t*)buf, total, la.vstart, L0, P1, c->d_link.as<uint16_t>());
            HIPCHK(hipGetLastError());
            la.L0 = L0; la.p_begin = P0; la.p_end = P1;
            hipLaunchKernelGGL(ndfl_lz_match_kernel, dim3((uint32_t)((P1 - P0 + LZ_TILE - 1) / LZ_TILE)), dim3(1024), 0, s, la);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemsetAsync(c->d_ticket.p, 0, 64, s));
        ea.batch_x0 = x0; ea.chunk_base = cb; ea.nchunks_batch = ce - cb;
        hipLaunchKernelGGL(ndfl_lz_encode_kernel, dim3(ce - cb), dim3(1024), 0, s, ea);
        HIPCHK(hipGetLastError());
    }
    TRY(f.stop_timing());
    if (stats.p) {
        unsigned long long st[16];
        HIPCHK(hipMemcpyAsync(st, stats.p, 128, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (chain_search)
            fprintf(stderr, "[ndfl] lz match: %llu searched positions, %.2f hops/pos, %.2f trigram hits/pos, %.2f compare words/pos\n",
                    st[0], (double)st[1] / std::max(1ull, st[0]), (double)st[2] / std::max(1ull, st[0]),
                    (double)st[3] / std::max(1ull, st[0]));
        else
            fprintf(stderr, "[ndfl] lz parse-driven match: %llu searches for %llu positions (%.2f %%), %.2f bucket entries per search, "
                    "%llu fallback searches in the encode kernel\n",
                    st[0], (unsigned long long)len, 100.0 * (double)st[0] / std::max<double>(1.0, (double)len),
                    (double)st[1] / std::max(1ull, st[0]), st[2]);
        if (!chain_search)
            fprintf(stderr, "[ndfl] lz parse-driven tiles %llu: stage+sort %.1f us, paths %.1f us, entries %.1f us per tile\n",
                    st[6], st[3] / 100.0 / std::max(1ull, st[6]), st[4] / 100.0 / std::max(1ull, st[6]),
                    st[5] / 100.0 / std::max(1ull, st[6]));
        const double k = 100.0 * (double)std::max(1ull, st[13]);
        fprintf(stderr, "[ndfl] lz encode chunks %llu: fill+parse %.1f us (walks %.1f, true entries %.1f), histograms %.1f us, "
                "codes %.1f us, token bits %.1f us, look-back+store %.1f us per chunk\n", st[13], st[8] / k, st[14] / k,
                st[15] / k, st[9] / k, st[10] / k, st[11] / k, st[12] / k);
    }
    const uint32_t ne = 2 * nch;
    hipLaunchKernelGGL(ndfl_edge_fixup_kernel, dim3((ne + 255) / 256), dim3(256), 0, s,
                       (const uint64_t*)ea.edge_w, (const uint32_t*)ea.edge_v, ne, f.d_out);
    HIPCHK(hipGetLastError());
    TRY(f.read_end(ea.status + (nch - 1)));
    const double ms = c->last_ms;       // (ndfl_crc32 times its own kernel)
    const int rc = f.crc_of(buf + LZ_DS);
    c->last_ms = ms;
    if (rc) return rc;
    return f.finish();
}

// The dispatcher: the encoder of a valid tuple, over the frame's chunks.
static int encode_chunks(Frame& f, const LzTuple& t, int dynamic, BlockOpts o) {
    TRY(f.count_chunks());
    const int preset = lz77_preset(t, dynamic);
    if (preset < 0) return chunks_lz(f, t, dynamic != 0, o);
    return chunks_rle(f, preset == NDFL_RLE_STATIC || preset == NDFL_RLE_DYNAMIC, dynamic != 0, o);
}

// One ndfl_assemble_kernel launch, one entry per block it copies.  Either `choice` names each
// entry's stream among `streams` (a null stream: stored blocks of the entry's chunk of aa.data), or,
// with `setfin` given, streams[k] is entry k's own and setfin[k] sets its block's bfinal bit.
struct AsmTables {
    std::vector<uint64_t> src, dst, nb;          // per entry: its bits' offset in its stream and in the output, their number
    std::vector<const uint32_t*> streams;
    std::vector<uint8_t> choice, setfin;
};

// Packs the tables into one device block and launches; aa holds the data arguments and the output.
static int launch_assemble(ndfl_ctx* c, hipStream_t s, const AsmTables& t, AsmArgs aa) {
    const size_t ne = t.src.size();
    if (ne == 0) return NDFL_OK;
    const struct { const void* p; size_t n; } parts[6] = {
        {t.src.data(), ne * 8}, {t.dst.data(), ne * 8}, {t.nb.data(), ne * 8}, {t.streams.data(), t.streams.size() * 8},
        {t.setfin.data(), t.setfin.size()}, {t.choice.data(), ne}};
    size_t off[7] = {0};
    for (int k = 0; k < 6; k++) off[k + 1] = off[k] + parts[k].n;
    const size_t tb = off[6] + 64;
    HIPCHK(c->d_masm.ensure(tb));
    char* bp = (char*)c->d_masm.p;
    std::vector<char> host(tb);
    for (int k = 0; k < 6; k++)
        if (parts[k].n) memcpy(host.data() + off[k], parts[k].p, parts[k].n);
    HIPCHK(hipMemcpyAsync(bp, host.data(), tb, hipMemcpyHostToDevice, s));
    aa.nchunks = (uint32_t)ne;
    aa.src_bit = (const uint64_t*)(bp + off[0]); aa.dst_bit = (const uint64_t*)(bp + off[1]);
    aa.nbits = (const uint64_t*)(bp + off[2]); aa.streams = (const uint32_t* const*)(bp + off[3]);
    aa.per_entry_stream = t.setfin.empty() ? 0 : 1;
    aa.setfin = aa.per_entry_stream ? (const uint8_t*)(bp + off[4]) : nullptr;
    aa.choice = (const uint8_t*)(bp + off[5]);
    hipLaunchKernelGGL(ndfl_assemble_kernel, dim3((uint32_t)ne), dim3(256), 0, s, aa);
    HIPCHK(hipGetLastError());
    return NDFL_OK;
}

// MultiStrategy over Lz77Huffman / Uncompressed substrategies (D/comp/MultiStrategy.java:31-57,
// D/comp/Uncompressed.java:19-51): every Lz77Huffman substrategy encodes all chunks into its own
// stream; the host walks the chunks with the bit position mod 8 and keeps, per chunk, the first
// substrategy with the fewest bits at that position; ndfl_assemble_kernel writes the result.
static int deflate_multi(Frame& f, const ndfl_strategy_desc* strats, uint32_t n_strats) {
    if (!f.pointers_ok() || !strats || n_strats == 0) return NDFL_E_ARG;
    if (n_strats > 8) return NDFL_E_UNSUPPORTED;
    TRY(f.check());
    for (uint32_t k = 0; k < n_strats; k++) {
        if (strats[k].kind == NDFL_KIND_UNCOMPRESSED) continue;
        if (strats[k].kind != NDFL_KIND_LZ77 || !lz77_tuple_valid(desc_tuple(strats[k]))) return NDFL_E_ARG;
    }
    TRY(f.begin());
    TRY(f.count_chunks());
    ndfl_ctx* c = f.c;
    hipStream_t s = f.s;
    const uint32_t nch = f.nch, chunk_len = f.chunk_len;
    const uint64_t len = f.len;
    // device copies of the inputs (the sub-encodes take device pointers)
    const uint8_t* d_data = f.data;
    const uint8_t* d_hist = f.hist;
    if (!(f.flags & NDFL_IN_DEVICE)) {
        HIPCHK(c->d_mdata.ensure(len + f.hist_len + 16));
        if (f.hist_len) HIPCHK(hipMemcpyAsync(c->d_mdata.p, f.hist, f.hist_len, hipMemcpyHostToDevice, s));
        if (len) HIPCHK(hipMemcpyAsync(c->d_mdata.as<uint8_t>() + f.hist_len, f.data, len, hipMemcpyHostToDevice, s));
        d_hist = c->d_mdata.as<uint8_t>();
        d_data = d_hist + f.hist_len;
    }
    const uint64_t stream_cap = f.bound_words() * 4 + 64;
    std::vector<std::vector<uint64_t>> bits(n_strats);
    AsmTables t;
    t.streams.assign(n_strats, nullptr);
    for (uint32_t k = 0; k < n_strats; k++) {
        const ndfl_strategy_desc& d = strats[k];
        if (d.kind == NDFL_KIND_UNCOMPRESSED) continue;
        HIPCHK(c->d_mstreams[k].ensure(stream_cap));
        HIPCHK(c->d_mbits[k].ensure(nch * 8ull));
        Frame sf = f.sub(d_hist, f.hist_len, f.hist_limit, d_data, len, chunk_len, f.final_flag,
                         c->d_mstreams[k].as<uint8_t>(), stream_cap);
        TRY(encode_chunks(sf, desc_tuple(d), d.dynamic, BlockOpts{c->d_mbits[k].as<uint64_t>(), 0}));
        bits[k].resize(nch);
        HIPCHK(hipMemcpyAsync(bits[k].data(), c->d_mbits[k].p, nch * 8ull, hipMemcpyDeviceToHost, s));
        t.streams[k] = c->d_mstreams[k].as<uint32_t>();
    }
    HIPCHK(hipStreamSynchronize(s));
    // choose (D/comp/MultiStrategy.java:35-44: strictly fewer bits wins, so ties keep the earlier one)
    t.choice.resize(nch); t.src.resize(nch); t.dst.resize(nch); t.nb.resize(nch);
    std::vector<uint64_t> soff(n_strats, 0);
    uint64_t pos = f.start_bitpos;
    for (uint32_t ci = 0; ci < nch; ci++) {
        const uint64_t cl = std::min<uint64_t>(chunk_len, len - (uint64_t)ci * chunk_len);
        const uint32_t p8 = (uint32_t)(pos & 7);
        uint64_t best = UINT64_MAX;
        uint32_t bk = 0;
        for (uint32_t k = 0; k < n_strats; k++) {
            uint64_t b;
            if (strats[k].kind == NDFL_KIND_UNCOMPRESSED) {
                const uint64_t nblk = std::max<uint64_t>((cl + 65534) / 65535, 1);   // (:23-25)
                b = cl * 8 + nblk * 40 + (uint64_t)((int)((13 - p8) % 8) - 5);
            } else {
                b = bits[k][ci];
            }
            if (b < best) { best = b; bk = k; }
        }
        t.choice[ci] = (uint8_t)bk;
        t.dst[ci] = pos;
        t.nb[ci] = best;
        for (uint32_t k = 0; k < n_strats; k++)
            if (strats[k].kind != NDFL_KIND_UNCOMPRESSED) {
                if (k == bk) t.src[ci] = soff[k];
                soff[k] += bits[k][ci];
            }
        pos += best;
    }
    TRY(f.place((pos + 31) / 32 + 2, true));
    AsmArgs aa;
    aa.data = d_data; aa.n = len; aa.chunk_len = chunk_len; aa.final_last = f.final_flag ? 1 : 0; aa.out = f.d_out;
    TRY(launch_assemble(c, s, t, aa));
    HIPCHK(hipStreamSynchronize(s));
    f.set_end(pos);
    TRY(f.crc_of(d_data));
    return f.finish();
}

// BinarySplit(sub, minBlockLen) over an Lz77Huffman substrategy (D/comp/BinarySplit.java:21-82):
// each chunk is halved recursively while both halves are longer than minBlockLen, and a split is
// kept when the halves' decisions take fewer bits.  Every halving level of the full chunks is
// encoded by one sub-frame (block length L/2^k, history from the parent chunk -- the sub-decide keeps
// `off`, :44-45), a partial final chunk node by node; the host runs the reference's recursion on
// the bit counts and ndfl_assemble_kernel copies the chosen blocks (bfinal set on the last one).
extern "C" int ndfl_deflate_chunks_binsplit(ndfl_ctx* c, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                                            const uint8_t* data, uint64_t len, uint32_t chunk_len,
                                            const ndfl_strategy_desc* sub, int32_t min_block_len, int final_flag,
                                            uint32_t start_bitpos, uint8_t* out, uint64_t out_cap,
                                            uint64_t* out_end_bits, uint32_t* crc_inout, uint32_t flags) {
    Frame f{c, hist, hist_len, hist_limit, data, len, chunk_len, final_flag, start_bitpos, out, out_cap, out_end_bits,
            crc_inout, flags};
    if (!sub || min_block_len < 1) return NDFL_E_ARG;                               // (:23-24)
    TRY(f.check());
    if (sub->kind != NDFL_KIND_LZ77) return NDFL_E_UNSUPPORTED;     // position-independent substrategies only
    if (!lz77_tuple_valid(desc_tuple(*sub))) return NDFL_E_ARG;
    TRY(f.begin());
    hipStream_t s = f.s;
    const uint32_t M = (uint32_t)min_block_len;
    // device copy [hist | data]
    HIPCHK(c->d_mdata.ensure(len + hist_len + 16));
    const hipMemcpyKind kin = (f.flags & NDFL_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (hist_len) HIPCHK(hipMemcpyAsync(c->d_mdata.p, f.hist, hist_len, kin, s));
    if (len) HIPCHK(hipMemcpyAsync(c->d_mdata.as<uint8_t>() + hist_len, f.data, len, kin, s));
    const uint8_t* base = c->d_mdata.as<uint8_t>();            // base[hist_len + x] = data[x]
    // uniform halving levels of a full chunk
    std::vector<uint32_t> lv{chunk_len};
    while (true) {
        const uint32_t sz = lv.back();
        if (!(sz / 2 > M)) break;                               // min((n+1)/2, n/2) > minBlockLen (:41-42)
        if (sz & 1) return NDFL_E_UNSUPPORTED;                  // uneven halves: not on the GPU path
        lv.push_back(sz / 2);
    }
    const uint32_t nlev = (uint32_t)lv.size();
    if (nlev > 16) return NDFL_E_UNSUPPORTED;
    const bool partial = f.final_flag && (len == 0 || len % chunk_len != 0);
    const uint64_t nfull = len / chunk_len;
    TRY(f.place((ndfl_deflate_bound(len, chunk_len) + 64 + 3) / 4 + 4, true));

    // encode data [a, a + n) as blocks of `blk` into dst (device), block bits to `bits`.  `level`:
    // a is a chunk boundary and the blocks' history starts at their chunk's (parent_len = chunk_len);
    // otherwise one block whose history is that of the partial chunk starting at `pstart`
    auto encode = [&](uint64_t a, uint64_t n, uint32_t blk, bool level, uint64_t pstart, bool fin, uint8_t* dst,
                      uint64_t cap, uint64_t* d_bits, std::vector<uint64_t>& bits) -> int {
        const uint64_t off = hist_len + pstart - std::min<uint64_t>(hist_limit, hist_len + pstart);   // in base
        const uint64_t hl = level ? std::min<uint64_t>(hist_limit, hist_len + a)
                                  : std::min<uint64_t>(32768, hist_len + a - off);
        const uint64_t hlim = level ? hist_limit : hl;
        Frame sf = f.sub(base + hist_len + a - hl, (uint32_t)hl, (uint32_t)hlim, base + hist_len + a, n, blk, fin ? 1 : 0,
                         dst, cap);
        TRY(encode_chunks(sf, desc_tuple(*sub), sub->dynamic, BlockOpts{d_bits, level ? chunk_len : 0}));
        bits.resize(sf.nch);
        HIPCHK(hipMemcpyAsync(bits.data(), d_bits, sf.nch * 8ull, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    struct Ent { const uint32_t* st; uint64_t src, nb; uint8_t fin; };
    uint64_t pos = f.start_bitpos;
    // write a group of entries at pos (one assemble launch): one stream pointer per entry
    auto assemble = [&](const std::vector<Ent>& ents) -> int {
        if (ents.empty()) return 0;
        AsmTables t;
        for (const Ent& e : ents) {
            t.src.push_back(e.src); t.dst.push_back(pos); t.nb.push_back(e.nb); t.streams.push_back(e.st);
            t.setfin.push_back(e.fin); t.choice.push_back(0);
            pos += e.nb;
        }
        AsmArgs aa;
        aa.data = nullptr; aa.n = 0; aa.chunk_len = 1; aa.final_last = 0; aa.out = f.d_out;
        TRY(launch_assemble(c, s, t, aa));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    // recursion of BinarySplit.decide (:33-66) on bit counts (position-independent substrategy)
    std::vector<std::vector<uint64_t>> lb(nlev);
    std::function<uint64_t(uint32_t, uint64_t, std::vector<std::pair<uint32_t, uint64_t>>&)> decide_lv =
        [&](uint32_t k, uint64_t idx, std::vector<std::pair<uint32_t, uint64_t>>& leaves) -> uint64_t {
            const uint64_t cur = lb[k][idx];
            if (k + 1 < nlev) {
                const uint64_t d0 = lb[k + 1][2 * idx], d1 = lb[k + 1][2 * idx + 1];
                if (d0 + d1 < cur) {                            // improved: recurse into both halves
                    std::vector<std::pair<uint32_t, uint64_t>> l2;
                    const uint64_t t = decide_lv(k + 1, 2 * idx, l2) + decide_lv(k + 1, 2 * idx + 1, l2);
                    if (t < cur) { leaves.insert(leaves.end(), l2.begin(), l2.end()); return t; }
                }
            }
            leaves.push_back({k, idx});
            return cur;
        };
    const uint32_t BCH = std::max<uint32_t>(1, (uint32_t)((64ull << 20) / chunk_len));
    for (uint64_t cb = 0; cb < nfull; cb += BCH) {
        const uint64_t ce = std::min<uint64_t>(nfull, cb + BCH);
        const uint64_t a = cb * chunk_len, n = (ce - cb) * chunk_len;
        std::vector<uint64_t> soff[16];
        for (uint32_t k = 0; k < nlev; k++) {
            const uint64_t capk = (ndfl_deflate_bound(n, lv[k]) + 3) / 4 * 4 + 64;
            HIPCHK(c->d_mstreams[k].ensure(capk));
            HIPCHK(c->d_mbits[k].ensure((n / lv[k]) * 8 + 64));
            TRY(encode(a, n, lv[k], true, 0, false, c->d_mstreams[k].as<uint8_t>(), capk, c->d_mbits[k].as<uint64_t>(),
                       lb[k]));
            soff[k].resize(lb[k].size() + 1);
            soff[k][0] = 0;
            for (size_t q = 0; q < lb[k].size(); q++) soff[k][q + 1] = soff[k][q] + lb[k][q];
        }
        std::vector<Ent> ents;
        for (uint64_t j = 0; j < ce - cb; j++) {
            std::vector<std::pair<uint32_t, uint64_t>> leaves;
            decide_lv(0, j, leaves);
            for (auto& lf : leaves)
                ents.push_back({c->d_mstreams[lf.first].as<uint32_t>(), soff[lf.first][lf.second], lb[lf.first][lf.second], 0});
        }
        if (ce == nfull && !partial && final_flag && !ents.empty()) ents.back().fin = 1;
        TRY(assemble(ents));
    }
    if (partial) {
        const uint64_t P = nfull * chunk_len, lp = len - P;
        std::vector<ScopedBuf> bufs;                            // the nodes' blocks, released on every return
        int nenc = 0, err = 0;
        std::vector<uint64_t> tmpbits;
        HIPCHK(c->d_mbits[0].ensure(64));
        // node [a, a+n): bits and the buffer holding its block (encoded once, kept for assembly)
        std::map<std::pair<uint64_t, uint64_t>, std::pair<size_t, uint64_t>> memo;
        auto node = [&](uint64_t a2, uint64_t n2) -> std::pair<size_t, uint64_t> {
            auto it = memo.find({a2, n2});
            if (it != memo.end()) return it->second;
            if (++nenc > 8192) { err = NDFL_E_UNSUPPORTED; return {0, 0}; }
            bufs.emplace_back();
            const uint64_t capn = (ndfl_deflate_bound(n2, (uint32_t)std::max<uint64_t>(n2, 1)) + 3) / 4 * 4 + 64;
            if (bufs.back().ensure(capn) != hipSuccess) { err = NDFL_E_DEVICE; return {0, 0}; }
            const int rc = encode(P + (a2 - P), n2, (uint32_t)std::max<uint64_t>(n2, 1), false, P, n2 == 0,
                                  bufs.back().as<uint8_t>(), capn, c->d_mbits[0].as<uint64_t>(), tmpbits);
            if (rc) { err = rc; return {0, 0}; }
            auto r = std::make_pair(bufs.size() - 1, tmpbits[0]);
            memo[{a2, n2}] = r;
            return r;
        };
        std::vector<std::pair<uint64_t, uint64_t>> leaves;     // (a, n)
        std::function<uint64_t(uint64_t, uint64_t, std::vector<std::pair<uint64_t, uint64_t>>&)> decide_node =
            [&](uint64_t a2, uint64_t n2, std::vector<std::pair<uint64_t, uint64_t>>& out_l) -> uint64_t {
                const uint64_t cur = node(a2, n2).second;
                const uint64_t h1 = (n2 + 1) / 2, h2 = n2 - h1;
                if (!err && std::min(h1, h2) > M) {
                    const uint64_t d0 = node(a2, h1).second, d1 = node(a2 + h1, h2).second;
                    if (!err && d0 + d1 < cur) {
                        std::vector<std::pair<uint64_t, uint64_t>> l2;
                        const uint64_t t = decide_node(a2, h1, l2) + decide_node(a2 + h1, h2, l2);
                        if (t < cur) { out_l.insert(out_l.end(), l2.begin(), l2.end()); return t; }
                    }
                }
                out_l.push_back({a2, n2});
                return cur;
            };
        decide_node(P, lp, leaves);
        if (err) return err;
        std::vector<Ent> ents;
        for (auto& lf : leaves) {
            auto nd = memo[lf];
            ents.push_back({bufs[nd.first].as<uint32_t>(), 0, nd.second, 0});
        }
        if (!ents.empty() && lp > 0) ents.back().fin = 1;     // (an empty final block was encoded final)
        TRY(assemble(ents));
    }
    f.set_end(pos);
    TRY(f.crc_of(base + hist_len));
    return f.finish();
}

// One Lz77Huffman over the call's chunks: ndfl_deflate_chunks_lz77, and ndfl_deflate_chunks' presets.
static int deflate_lz(Frame& f, const LzTuple& t, int dynamic) {
    TRY(f.check());
    TRY(f.begin());
    return encode_chunks(f, t, dynamic, BlockOpts{});
}

extern "C" int ndfl_deflate_chunks(ndfl_ctx* c, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                                   const uint8_t* data, uint64_t len, uint32_t chunk_len, int strategy, int final_flag,
                                   uint32_t start_bitpos, uint8_t* out, uint64_t out_cap, uint64_t* out_end_bits,
                                   uint32_t* crc_inout, uint32_t flags) {
    Frame f{c, hist, hist_len, hist_limit, data, len, chunk_len, final_flag, start_bitpos, out, out_cap, out_end_bits,
            crc_inout, flags};
    static const ndfl_strategy_desc stored = {NDFL_KIND_UNCOMPRESSED, 0, 0, 0, 0, 0};
    switch (strategy) {          // the presets (D/comp/Lz77Huffman.java:298-305); the odd ids are the dynamic ones
        case NDFL_LITERAL_STATIC: case NDFL_LITERAL_DYNAMIC: return deflate_lz(f, {0, 0, 0, 0}, strategy & 1);
        case NDFL_RLE_STATIC: case NDFL_RLE_DYNAMIC: return deflate_lz(f, {3, 258, 1, 1}, strategy & 1);
        case NDFL_FULL_STATIC: case NDFL_FULL_DYNAMIC: return deflate_lz(f, {3, 258, 1, 32768}, strategy & 1);
        case NDFL_UNCOMPRESSED: return deflate_multi(f, &stored, 1);
        default: return NDFL_E_ARG;
    }
}

extern "C" int ndfl_deflate_chunks_lz77(ndfl_ctx* c, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                                        const uint8_t* data, uint64_t len, uint32_t chunk_len, int dynamic, int min_run,
                                        int max_run, int min_dist, int max_dist, int final_flag, uint32_t start_bitpos,
                                        uint8_t* out, uint64_t out_cap, uint64_t* out_end_bits, uint32_t* crc_inout,
                                        uint32_t flags) {
    const LzTuple t{min_run, max_run, min_dist, max_dist};
    if (!lz77_tuple_valid(t)) return NDFL_E_ARG;
    Frame f{c, hist, hist_len, hist_limit, data, len, chunk_len, final_flag, start_bitpos, out, out_cap, out_end_bits,
            crc_inout, flags};
    return deflate_lz(f, t, dynamic);
}

extern "C" int ndfl_deflate_chunks_multi(ndfl_ctx* c, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                                         const uint8_t* data, uint64_t len, uint32_t chunk_len,
                                         const ndfl_strategy_desc* strats, uint32_t n_strats, int final_flag,
                                         uint32_t start_bitpos, uint8_t* out, uint64_t out_cap, uint64_t* out_end_bits,
                                         uint32_t* crc_inout, uint32_t flags) {
    Frame f{c, hist, hist_len, hist_limit, data, len, chunk_len, final_flag, start_bitpos, out, out_cap, out_end_bits,
            crc_inout, flags};
    return deflate_multi(f, strats, n_strats);
}
