// inflate_batch_loop.inc -- the stream loop of the two batch kernels (inflate_batch.hip): the BODY of
// a kernel, included once in each with NDFL_BATCH_MEMBERS defined.
//   0: ndfl_inflate_batch_kernel -- raw DEFLATE streams; ndfl_batch_item / ndfl_batch_result.
//   1: ndfl_inflate_members_kernel -- each item's container header before the DEFLATE data, the
//      checksum in flush_to (q is an OutM), the trailer after the final block; ndfl_member_item /
//      ndfl_member_result, and the extra kernel argument crc_x.
// It is text and not a function template on purpose: a function around the loop, inlined into the
// kernels, changes the code the compiler makes of the plain kernel (other instruction order, 154
// instead of 171 VGPRs), and that kernel's code is to stay exactly what it was.
//
// results[i].status: the decoder's internal Reason (R_*, the host maps it and derives the symbol), a
// container's Reason, NDFL_E_CAPACITY, NDFL_E_ARG (members: zlib CINFO > 7) or 0; the other fields as
// the C ABI documents them.
    using namespace bat;
    typedef Io<NDFL_BATCH_MEMBERS != 0>::Item Item;
    typedef Io<NDFL_BATCH_MEMBERS != 0>::Result Result;
    __shared__ __attribute__((aligned(16))) Shared S;
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ uint32_t inw[IW];
    __shared__ uint32_t s_ticket;
    const int lane = threadIdx.x;
    // The table build gets the lane index read back from LDS (S.kind_, which this kernel does not use
    // otherwise): computed from threadIdx, the build's many lane masks and lane-derived constants are
    // hoisted out of the stream loop and held -- spilled, 88 SGPRs -- across the token loop.
    S.kind_[lane] = (uint8_t)lane;
    uint32_t* scr = S.exit_;                    // the build's 64 words (this kernel has no rounds)
    w = (const uint32_t*)to_v((uint64_t)(uintptr_t)w);
    out = (uint8_t*)to_v((uint64_t)(uintptr_t)out);
    items = (const Item*)to_v((uint64_t)(uintptr_t)items);
    results = (Result*)to_v((uint64_t)(uintptr_t)results);
    ticket = (uint32_t*)to_v((uint64_t)(uintptr_t)ticket);
    n = to_v(n);
#if NDFL_BATCH_MEMBERS
    crc_x = (const uint32_t*)to_v((uint64_t)(uintptr_t)crc_x);
#endif
    for (;;) {
        __syncthreads();
        if (lane == 0) s_ticket = atomicAdd(ticket, 1u);
        __syncthreads();
        // (the stream's constants -- its index, item, input view and region -- are parked in vector
        // registers too, like the kernel's arguments: none of them is needed in the token loop's scalars)
        const uint32_t si = to_v((uint32_t)s_ticket);
        if (to_s(si) >= to_s(n)) break;
        Item it = items[si];
        it.in_off = to_v(it.in_off); it.in_len = to_v(it.in_len);
        it.out_off = to_v(it.out_off); it.out_cap = to_v(it.out_cap);
#if NDFL_BATCH_MEMBERS
        // The container header (lane 0).  The DEFLATE data is the item less its first hl bytes, so every
        // position check of the decode is the DEFLATE data's own, at any byte alignment of in_off + hl.
        const uint32_t fmt = to_v(it.format);
        uint64_t hl = 0;
        int32_t hstat = 0;
        if (lane == 0 && fmt != NDFL_FMT_RAW) {
            const In all = stream_in(w, it.in_off, it.in_len);
            hstat = fmt == NDFL_FMT_ZLIB ? parse_zlib_header(all, it.in_off & 3, it.in_len, hl)
                                         : parse_gzip_header(all, it.in_off & 3, it.in_len, hl);
        }
        hstat = (int32_t)to_v(to_s((uint32_t)hstat));
        hl = to_v(to_s(hl));
        const In in = stream_in(w, it.in_off + hl, it.in_len - hl);
        const uint64_t p0 = ((it.in_off + hl) & 3) * 8;
        OutM q;
        q.sum = to_v(fmt == NDFL_FMT_ZLIB ? NDFL_SUM_ADLER32 : fmt == NDFL_FMT_GZIP ? NDFL_SUM_CRC32 : it.sum);
        q.ck = to_v(q.sum == NDFL_SUM_CRC32 ? 0xFFFFFFFFu : q.sum == NDFL_SUM_ADLER32 ? 1u : 0u);
        q.crc_x = crc_x;
#else
        const In in = stream_in(w, it.in_off, it.in_len);
        const uint64_t p0 = (it.in_off & 3) * 8;
        Out q;
#endif
        q.ring = ring;
        q.obeg = (uint64_t)(uintptr_t)out + it.out_off;
        q.oend = q.obeg + it.out_cap;
        q.o = q.obeg; q.fl = q.obeg; q.npend = 0;
        uint32_t pend = 0;                      // this lane's pending literal
        uint64_t iw0 = NO_STAGE;                // first input word staged in inw
        uint64_t cur = p0;
        uint32_t reason = 0;
        for (;;) {
#if NDFL_BATCH_MEMBERS
            if (to_s((uint32_t)hstat)) break;   // no DEFLATE data behind a refused header
#endif
            park(q, cur, iw0);
            for (uint32_t s = (uint32_t)lane; s < 320; s += 64) S.lens[s] = 0;
            __syncthreads();
            if (lane == 0) {
                Hdr h;
                parse_hdr_core(in, cur, S.lens, S.cl_tab, h);
                hdr_to_shared(h, S);
            }
            __syncthreads();
            reason = __builtin_amdgcn_readfirstlane(S.h_err);
            if (reason) break;
            const uint32_t btype = __builtin_amdgcn_readfirstlane(S.h_btype);
            if (btype == 0) {
                unpark(q, cur, iw0);
                const uint64_t d0 = to_s(S.h_d0);
                const bool bfinal = __builtin_amdgcn_readfirstlane(S.h_bfinal) != 0;
                // stored: a wave-wide copy of the bytes the input still has, then the length check
                flush_pending(q, pend, lane);
                const uint64_t avail = (in.nbits - d0) / 8, ln = to_s(S.h_len);
                const uint64_t take = min(avail, ln), ib = d0 >> 3;
                for (uint64_t done = 0; done < take;) {
                    const uint32_t chunk = (uint32_t)min(take - done, (uint64_t)STORED_STEP);
                    make_room(q, chunk, lane);
                    for (uint32_t i = (uint32_t)lane * 4; i < chunk; i += 256) {
                        const uint64_t b = ib + done + i;
                        const uint64_t two = ((uint64_t)in.ld((b >> 2) + 1) << 32) | in.ld(b >> 2);
                        const uint32_t v = (uint32_t)(two >> (8 * (uint32_t)(b & 3)));
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++)
                            if (i + k < chunk) q.ring[(q.o + i + k) & RMASK] = (uint8_t)(v >> (8 * k));
                    }
                    q.o += chunk;
                    done += chunk;
                    wsync();
                }
                if (take < ln) { reason = R_UEOS; break; }
                cur = d0 + 8 * ln;
                if (bfinal) break;
                continue;
            }
            const int bt = build_block_tables((LShared*)&S, (int)S.kind_[lane], (lu32*)scr);
            reason = __builtin_amdgcn_readfirstlane((uint32_t)bt & 0xFFu);
            if (reason) break;
            const bool ed = __builtin_amdgcn_readfirstlane((uint32_t)bt & 0x100u) != 0;
            unpark(q, cur, iw0);
            const uint64_t d0 = to_s(S.h_d0);
            const bool bfinal = __builtin_amdgcn_readfirstlane(S.h_bfinal) != 0;
            // the wave-uniform token loop
            uint64_t pos = d0;
            bool eob = false;
            while (!eob && !reason) {
                const uint64_t wi = pos >> 5;
                if (wi < iw0 || wi + 3 > iw0 + IW) {
                    wsync();                    // the reads of the words staged before
                    iw0 = wi;
#pragma unroll
                    for (uint32_t k = 0; k < IW / 64; k++) inw[k * 64 + lane] = in.ld(iw0 + k * 64 + lane);
                    wsync();
                }
                const uint32_t r = (uint32_t)(wi - iw0), sh = (uint32_t)pos & 31;
                const uint32_t wa = inw[r], wb = inw[r + 1], wc = inw[r + 2];
                const uint32_t lo = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(wb, wa, sh));
                const uint32_t hi = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(wc, wb, sh));
                const uint32_t e = __builtin_amdgcn_readfirstlane(S.t.lit[lo & ((1u << LB) - 1u)]);
                const uint32_t nb = (uint32_t)min(in.nbits - pos, (uint64_t)0xFFFFFFFFu);
                uint32_t adv = 0;
                Tok tk;
                tok_e<true>(lo, hi, e, adv, S.t, ed, 0xFFFFFFFFu, nb, tk);
                const uint32_t kind = __builtin_amdgcn_readfirstlane(tk.kind);
                const uint32_t val = __builtin_amdgcn_readfirstlane(tk.val);
                const uint32_t tn = __builtin_amdgcn_readfirstlane(tk.n);
                const uint32_t dist = __builtin_amdgcn_readfirstlane(tk.dist);
                pos += to_s(adv);
                if (kind == K_LIT) {
                    add_literal(q, pend, val & 0xFFu, lane);
                    if (tn == 2) add_literal(q, pend, (val >> 8) & 0xFFu, lane);
                } else if (kind == K_LEN) {
                    flush_pending(q, pend, lane);
                    if (dist > q.o - q.obeg) reason = R_COPY_BEFORE;
                    else copy_run(q, tn, dist, lane);
                } else if (kind == K_EOB) {
                    eob = true;
                } else {
                    reason = val;
                }
            }
            if (reason) break;
            cur = pos;
            if (bfinal) break;
        }
        unpark(q, cur, iw0);
        flush_pending(q, pend, lane);
        flush_to(q, q.o, lane);
        if (lane == 0) {
            const uint64_t total = q.o - q.obeg;
            Result rr;
            rr.status = reason ? (int32_t)reason : total > it.out_cap ? NDFL_E_CAPACITY : 0;
            rr.error_symbol = -1;
            rr.out_len = total;
            rr.consumed_bits = reason ? 0 : cur - p0;
#if NDFL_BATCH_MEMBERS
            {
                // the finished checksum; the trailer once the final block has ended without a Reason
                const uint32_t kind = to_s(q.sum);
                const uint32_t sum = kind == NDFL_SUM_CRC32 ? ~q.ck : q.ck;
                int32_t st = hstat ? hstat : (int32_t)reason;
                bool have_sum = !st;            // also on the trailer's two mismatch Reasons
                // (the format through to_v again: compared anew here, not a lane mask of the header's
                // test held in two scalar registers -- spilled -- across the whole decode)
                const uint32_t tfmt = to_v(fmt);
                if (!st && tfmt != NDFL_FMT_RAW) {
                    const uint64_t t = hl + ((cur - p0 + 7) >> 3);
                    uint32_t tl;
                    st = check_trailer(stream_in(w, it.in_off, it.in_len), it.in_off & 3, it.in_len, tfmt, t, sum,
                                       total, tl);
                    rr.consumed_bits = 8 * (t + tl);            // the whole member
                    have_sum = st != NDFL_UNEXPECTED_END_OF_STREAM;
                }
                if (st) rr.consumed_bits = 0;
                rr.status = st ? st : total > it.out_cap ? NDFL_E_CAPACITY : 0;
                rr.checksum = have_sum ? sum : 0u;
                rr.header_len = hstat ? 0u : (uint32_t)hl;
            }
#endif
            results[si] = rr;
        }
    }
