// ndfl_deflate_bgzf.cpp -- ndfl_deflate_bgzf and ndfl_bgzf_bound of include/ndfl.h (included by
// ndfl_capi.cpp): a buffer as a blocked gzip (BGZF) file, every block one stream of one chunk of the
// segmented chunk encoders (seg_prepare, seg_encode: ndfl_deflate_batch_chunked.cpp), then the writer's own
// passes (csrc/hip/deflate_bgzf.hip): member sizes, their scan, the table, and the pack into `out`.

// The geometry of a call, from its two numbers alone.
struct BgzwPlan {
    uint32_t nblk = 0;                  // data members: ceil(in_len / block_len)
    uint32_t n_members = 0;             // nblk + the closing empty member
    uint32_t ntiles = 0;                // tiles of bgzw::SIZE_TILE members
    uint64_t slot = 0;                  // a block's bytes in the staged output (a multiple of 4)
    uint64_t staged = 0;                // nblk * block_len: the slots
    uint64_t out_bytes = 0;             // nblk * slot
};

// A member's length with its block stored: header, the stored block or blocks, trailer.
static uint64_t bgzw_stored_member(uint64_t len) {
    return 26 + len + 5 * std::max<uint64_t>(1, (len + bgzw::STORED_BLOCK - 1) / bgzw::STORED_BLOCK);
}

// block_len and in_len against the call's limits, then the plan (no HIP call, nothing allocated).
static int bgzw_plan(uint64_t in_len, uint32_t block_len, BgzwPlan& P) {
    if (block_len == 0) return NDFL_E_ARG;
    if (block_len > (uint32_t)MAX_CHUNK) return NDFL_E_UNSUPPORTED;
    if (in_len > (8ull << 30)) return NDFL_E_UNSUPPORTED;
    const uint64_t nblk = in_len / block_len + (in_len % block_len != 0);
    if (nblk > 0x7FFFFFFEull) return NDFL_E_UNSUPPORTED;              // (the edge list holds two entries per chunk)
    P.nblk = (uint32_t)nblk;
    P.n_members = P.nblk + 1;
    P.ntiles = (P.n_members + bgzw::SIZE_TILE - 1) / bgzw::SIZE_TILE;
    P.slot = seg_out_slot(block_len, block_len);
    P.staged = nblk * block_len;
    P.out_bytes = nblk * P.slot;
    return NDFL_OK;
}

extern "C" uint64_t ndfl_bgzf_bound(uint64_t in_len, uint32_t block_len) {
    if (block_len == 0 || block_len > (uint32_t)MAX_CHUNK) return 0;
    const uint64_t tail = in_len % block_len;
    return in_len / block_len * bgzw_stored_member(block_len) + (tail ? bgzw_stored_member(tail) : 0) + bgzw::EOF_LEN;
}

// The call, its arguments checked.  One sync when the file stays on the device, else one for the sizes
// and one for the file's bytes.
static int deflate_bgzf_run(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                            ndfl_bgzf_write_result* result, ndfl_bgzf_member* table, uint32_t table_cap, const LzTuple& t,
                            int dynamic, uint32_t block_len, const BgzwPlan& P, uint32_t flags) {
    using namespace bgzw;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = ordered_stream(c);
    const uint32_t nblk = P.nblk, nm = P.n_members;
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t o_head = 0, o_mlen = up(sizeof(Head)), o_tcnt = o_mlen + up((size_t)nm * 4),
                 o_tsum = o_tcnt + up((size_t)P.ntiles * 4), o_items = o_tsum + up((size_t)P.ntiles * 8),
                 o_table = o_items + up((size_t)nblk * sizeof(ndfl_member_item)),
                 o_end = o_table + up(((size_t)nm + 1) * sizeof(ndfl_bgzf_member));
    HIPCHK(c->d_bgzw.ensure(o_end));
    char* z = (char*)c->d_bgzw.p;
    Head* d_head = (Head*)(z + o_head);
    uint32_t* d_mlen = (uint32_t*)(z + o_mlen);
    uint32_t* d_tcnt = (uint32_t*)(z + o_tcnt);
    uint64_t* d_tsum = (uint64_t*)(z + o_tsum);
    ndfl_member_item* d_items = (ndfl_member_item*)(z + o_items);
    ndfl_bgzf_member* d_table = (ndfl_bgzf_member*)(z + o_table);
    HIPCHK(hipMemsetAsync(d_head, 0xFF, sizeof(Head), s));

    const size_t chunks_b = (size_t)nblk * sizeof(SegChunk);
    HIPCHK(c->d_segtab.ensure(chunks_b + (size_t)nblk * sizeof(SegStream)));
    SegChunk* d_chunks = c->d_segtab.as<SegChunk>();
    SegStream* d_streams = (SegStream*)((char*)c->d_segtab.p + chunks_b);
    SegTab tab;
    tab.chunks = d_chunks;
    tab.streams = d_streams;
    uint8_t* buf = nullptr;
    if (nblk) {
        // the slots are the input as it lies: block k at k * block_len, the last slot's rest zeroed
        TRY(seg_prepare(c, s, nblk, nblk, P.staged, P.out_bytes, &buf));
        HIPCHK(hipMemcpyAsync(buf + LZ_DS, in, in_len, (flags & NDFL_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        if (P.staged > in_len) HIPCHK(hipMemsetAsync(buf + LZ_DS + in_len, 0, P.staged - in_len, s));
    }
    const bool out_dev = (flags & NDFL_OUT_DEVICE) != 0;
    uint8_t* d_out = out;
    if (!out_dev && out_cap) {          // (a file that fits out_cap fits the bound too)
        const uint64_t room = std::min<uint64_t>(out_cap, ndfl_bgzf_bound(in_len, block_len));
        HIPCHK(c->batch.d_out.ensure(room));
        d_out = c->batch.d_out.as<uint8_t>();
    }

    HIPCHK(hipEventRecord(c->ev0, s));
    if (nblk) {
        hipLaunchKernelGGL(ndfl_bgzw_tables_kernel, dim3((nblk + SIZE_TILE - 1) / SIZE_TILE), dim3(SIZE_TILE), 0, s, in_len,
                           block_len, nblk, P.slot, d_chunks, d_streams, d_items);
        HIPCHK(hipGetLastError());
        TRY(seg_encode(c, s, tab, buf, nblk, P.staged, block_len, 32768u, t, dynamic, true, d_items, nblk, nullptr));
    }
    hipLaunchKernelGGL(ndfl_bgzw_size_kernel, dim3(P.ntiles), dim3(SIZE_TILE), 0, s, (const uint64_t*)c->d_status.p, in_len,
                       block_len, nblk, P.slot, d_mlen, d_tcnt, d_tsum, d_head);
    hipLaunchKernelGGL(ndfl_bgzf_sum_kernel, dim3(1), dim3(bgzf::SUM_BLOCK), 0, s, d_tcnt, d_tsum, P.ntiles, &d_head->n_stored,
                       &d_head->total);
    hipLaunchKernelGGL(ndfl_bgzw_offsets_kernel, dim3(P.ntiles), dim3(SIZE_TILE), 0, s, (const uint32_t*)d_mlen,
                       (const uint64_t*)d_tsum, (const Head*)d_head, in_len, block_len, nblk, d_table);
    hipLaunchKernelGGL(ndfl_bgzw_pack_kernel, dim3(nm), dim3(PACK_THREADS), 0, s, (const uint8_t*)c->d_out.p,
                       (const uint8_t*)(buf ? buf + LZ_DS : nullptr), (const uint32_t*)d_mlen, (const ndfl_bgzf_member*)d_table,
                       (const uint32_t*)c->d_crc1.p, (const Head*)d_head, in_len, block_len, nblk, P.slot, d_out, out_cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, s));
    Head h;
    HIPCHK(hipMemcpyAsync(&h, d_head, sizeof(Head), hipMemcpyDeviceToHost, s));
    const uint32_t nt = (uint32_t)std::min<uint64_t>(table_cap, (uint64_t)nm + 1);
    if (nt) HIPCHK(hipMemcpyAsync(table, d_table, (size_t)nt * sizeof(ndfl_bgzf_member), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_ms = ms;
    result->n_members = nm;
    result->n_stored = h.n_stored;
    result->bad_member = h.bad == NO_BAD ? nm : h.bad;
    result->out_len = h.total;
    result->status = h.bad != NO_BAD ? NDFL_E_UNSUPPORTED : h.total > out_cap ? NDFL_E_CAPACITY : NDFL_OK;
    if (result->status == NDFL_OK && !out_dev) {
        HIPCHK(hipMemcpyAsync(out, d_out, h.total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return result->status;
}

extern "C" int ndfl_deflate_bgzf(ndfl_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                                 ndfl_bgzf_write_result* result, ndfl_bgzf_member* table, uint32_t table_cap,
                                 int dynamic, int min_run, int max_run, int min_dist, int max_dist,
                                 uint32_t block_len, uint32_t flags) {
    if (!c || !result || (!in && in_len) || (!out && out_cap) || (!table && table_cap)) return NDFL_E_ARG;
    *result = ndfl_bgzf_write_result{};
    const LzTuple t{min_run, max_run, min_dist, max_dist};
    if (!lz77_tuple_valid(t)) return NDFL_E_ARG;
    BgzwPlan P;
    TRY(bgzw_plan(in_len, block_len, P));
    return deflate_bgzf_run(c, in, in_len, out, out_cap, result, table, table_cap, t, dynamic, block_len, P, flags);
}
