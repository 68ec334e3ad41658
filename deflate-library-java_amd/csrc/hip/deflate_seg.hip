// deflate_seg.hip -- what ndfl_deflate_batch_chunked launches around the segmented chunk encoders
// (deflate_kernels.hip, deflate_split.hip, lz77_kernels.hip: the *_seg_kernel entry points): the
// gather of the streams into their slots, the per-chunk checksum partials and their combination per
// stream, and the finishing pass that moves every stream from the staged output to its region of the
// caller's `out`, appends its trailer and fills its result.  Tables: seg_tables.hpp.
#include "seg_tables.hpp"

// Chunk k's bytes from the caller's (device) `in` to slot position k * chunk_len, the rest of the
// chunk's slot zeroed: a kernel may read a slot's padding, so it is defined.  One workgroup per chunk.
extern "C" __global__ void __launch_bounds__(256)
ndfl_seg_gather_kernel(const uint8_t* in, uint8_t* slots, SegTab t, uint32_t chunk_len) {
    const uint32_t k = blockIdx.x;
    const uint32_t len = t.chunks[k].len;
    const uint8_t* src = in + t.chunks[k].src;
    uint8_t* dst = slots + (uint64_t)k * chunk_len;
    for (uint32_t i = threadIdx.x * 16; i < chunk_len; i += 256 * 16) {
        if (i + 16 <= len) {
            u32x4 v;
            __builtin_memcpy(&v, src + i, 16);
            __builtin_memcpy(dst + i, &v, 16);
        } else {
            for (uint32_t j = i; j < min(i + 16, chunk_len); j++) dst[j] = j < len ? src[j] : (uint8_t)0;
        }
    }
}

// One pass over all chunks: chunk k's checksum partial as its stream asks (its record's flags), the
// raw CRC-32 to part[2k] or Adler-32's (S, T) to part[2k], part[2k + 1].  A chunk of a stream that asks
// for no checksum leaves at the first, workgroup-uniform branch.
extern "C" __global__ void __launch_bounds__(1024)
ndfl_seg_sums_kernel(const uint8_t* slots, uint32_t chunk_len, SegTab t, const uint32_t* crc_tab, const uint32_t* crc_x,
                     uint32_t* part) {
    __shared__ unsigned long long rs[16], rt[16];
    __shared__ uint32_t red[16];
    const uint32_t k = blockIdx.x;
    const uint32_t kind = (t.chunks[k].flags >> SEG_SUM_SHIFT) & 3u;
    if (kind == NDFL_SUM_NONE) return;
    const uint8_t* seg = slots + (uint64_t)k * chunk_len;
    const uint32_t len = t.chunks[k].len;
    if (kind == NDFL_SUM_CRC32) {
        const uint32_t x = crc_segment_raw(seg, len, crc_tab, crc_x, red);
        if (threadIdx.x == 0) part[2 * k] = x;
    } else {
        adler_segment(seg, len, rs, rt, part + 2 * k);
    }
}

// The partials of a stream's chunks into its checksum, one wave per stream, a lane per chunk at a time.
// CRC-32: raw = XOR of crc_c * x^(8 * bytes after chunk c) (ndfl_crc_combine_kernel's arithmetic), then
// the initial and final complement.  Adler-32: every byte weighs its distance to the stream's end in
// b, so a = 1 + sum S_c and b = len + sum (T_c + S_c * bytes after chunk c), mod 65521.
extern "C" __global__ void __launch_bounds__(256)
ndfl_seg_sums_combine_kernel(const uint32_t* part, uint32_t chunk_len, SegTab t, const ndfl_member_item* items, uint32_t n,
                             const uint32_t* x8p2, uint32_t* sums) {
    const uint32_t s = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    if (s >= n) return;
    const SegStream st = t.streams[s];
    const uint32_t kind = (t.chunks[st.first_chunk].flags >> SEG_SUM_SHIFT) & 3u;
    const uint64_t len = items[s].in_len;
    if (kind == NDFL_SUM_NONE) {
        if (lane == 0) sums[s] = 0;
        return;
    }
    auto x8 = [&](uint64_t nb) -> uint32_t {                    // x^(8 * nb)
        uint32_t p = 1u << 31;
        for (int k = 0; nb; k++, nb >>= 1)
            if (nb & 1) p = crc_multmodp(x8p2[k], p);
        return p;
    };
    if (kind == NDFL_SUM_CRC32) {
        uint32_t acc = 0;
        for (uint32_t j = lane; j < st.nchunks; j += 64) {
            const uint64_t end = min((uint64_t)(j + 1) * chunk_len, len);
            acc ^= crc_multmodp(x8(len - end), part[2 * (uint64_t)(st.first_chunk + j)]);
        }
        acc = wave_xor(acc);
        if (lane == 0) sums[s] = ~(crc_multmodp(x8(len), 0xFFFFFFFFu) ^ acc);
    } else {
        unsigned long long a = 0, b = 0;
        for (uint32_t j = lane; j < st.nchunks; j += 64) {
            const uint64_t end = min((uint64_t)(j + 1) * chunk_len, len);
            const unsigned long long S = part[2 * (uint64_t)(st.first_chunk + j)], T = part[2 * (uint64_t)(st.first_chunk + j) + 1];
            a = (a + S) % 65521u;
            b = (b + T + S * ((len - end) % 65521u)) % 65521u;
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) sums[s] = (uint32_t)((b + len % 65521u) % 65521u) << 16 | (uint32_t)((a + 1) % 65521u);
    }
}

// One workgroup per stream: its end from its last chunk's status word (the inclusive prefix, in bits of
// the staged output), the container's trailer behind its byte-aligned DEFLATE data (the slot has room),
// min(out_len, out_cap) bytes to out[out_off ..] -- byte stores up to the first aligned word of `out` and
// after the last whole one, so no byte outside the stream's region is written -- and its result.
extern "C" __global__ void __launch_bounds__(1024)
ndfl_seg_finish_kernel(uint8_t* staged, const uint64_t* status, SegTab t, const ndfl_member_item* items,
                       const uint32_t* sums, uint8_t* out, ndfl_deflate_result* results) {
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const SegStream st = t.streams[s];
    const ndfl_member_item it = items[s];
    const uint64_t end_bits = (status[st.first_chunk + st.nchunks - 1] & ST_VAL) - 8 * st.obase;
    const uint64_t nbytes = (end_bits + 7) / 8;
    const uint32_t sum = sums[s];
    const uint32_t tl = it.format == NDFL_FMT_ZLIB ? 4u : it.format == NDFL_FMT_GZIP ? 8u : 0u;
    uint8_t* src = staged + st.obase;
    if (tid < tl) {
        uint32_t v;
        if (it.format == NDFL_FMT_ZLIB) v = sum >> (8 * (3 - tid));                        // big-endian Adler-32
        else v = tid < 4 ? sum >> (8 * tid) : (uint32_t)it.in_len >> (8 * (tid - 4));      // CRC-32, ISIZE: little-endian
        src[nbytes + tid] = (uint8_t)v;
    }
    __syncthreads();
    const uint64_t out_len = nbytes + tl;
    const uint64_t ncopy = min(out_len, it.out_cap);
    uint8_t* dst = out + it.out_off;
    const uint64_t head = min(ncopy, (uint64_t)((0 - (uintptr_t)dst) & 3));
    const uint64_t nw = (ncopy - head) / 4;
    if (tid < head) dst[tid] = src[tid];
    {
        const uint32_t r = (uint32_t)head;                  // (src is word-aligned: word w of dst starts at byte r of a word)
        const uint32_t* sw = (const uint32_t*)src;
        uint32_t* dw = (uint32_t*)(dst + head);
        for (uint64_t w = tid; w < nw; w += 1024)
            dw[w] = r ? __builtin_amdgcn_alignbyte(sw[w + 1], sw[w], r) : sw[w];
    }
    for (uint64_t i = head + 4 * nw + tid; i < ncopy; i += 1024) dst[i] = src[i];
    if (tid == 0) {
        ndfl_deflate_result rr;
        rr.status = out_len > it.out_cap ? NDFL_E_CAPACITY : 0;
        rr.checksum = sum;
        rr.out_len = out_len;
        rr.end_bits = end_bits;
        results[s] = rr;
    }
}
