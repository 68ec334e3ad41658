// deflate_split.hip -- the split RLE/LITERAL encoder pipeline (gfx950).
//
// The fused ndfl_deflate_chunks_kernel holds a 1024-thread workgroup (and the chunk's bytes in its
// registers) through the whole per-chunk Huffman build, which is a few hundred items of work at a
// time: two chunks per CU spend most of their life in barriers.  The split pipeline gives each
// phase the shape it wants:
//   1. ndfl_deflate_hist_kernel     1024 threads / chunk: load, CRC-32, closed-form RLE parse into
//                                   histograms (hist_out)
//   2. ndfl_deflate_codes_kernel    ONE WAVE / chunk: package-merge code lengths, canonical codes,
//                                   code-length RLE + its code, the header bits, the block size
//                                   (D/comp/Lz77Huffman.java:134-265,309-410) into a code record
//   3. ndfl_deflate_offsets_kernel  exclusive scan of the block sizes -> each chunk's global bit offset
//   4. ndfl_deflate_emit_kernel     1024 threads / chunk: reload, token bits at the known offset
// The codes come from the same builder as the fused kernel's (huffman_build.hpp, here on 64
// threads) and every other step yields the same bits as the fused kernel; the block size is computed from the histograms (every token's code length plus its
// extra bits -- the extra-bit count is a function of the symbol).
// D/ = /root/reference/src/io/nayuki/deflate/

#include "deflate_kernels.hip"       // Args, the record layouts
#include "huffman_build.hpp"

namespace {

// extra bits of literal/length symbol s (257..285) and distance symbol d (:92-127)
__device__ __forceinline__ uint32_t len_extra(uint32_t s) { return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0u; }
__device__ __forceinline__ uint32_t dist_extra(uint32_t d) { return d >= 4 ? (d >> 1) - 1 : 0u; }

}  // namespace

// Pass 2: one wave builds one chunk's codes and header from its histograms (build_block_codes<64>,
// huffman_build.hpp).  Writes the code record (codes, header bits, hdrBits) and the block size in
// bits to a.status[c] (+ chunk_bits).  SEG: the chunk's length and BFINAL from its record.
namespace {
template <bool SEG>
__device__ __forceinline__ void deflate_codes(const Args& a, HuffScr& S, const SegTab t = SegTab{}) {
    const uint32_t c = a.c0 + blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t cs = (uint64_t)c * a.chunk_len;
    const uint32_t len_c = SEG ? t.chunks[c].len : (uint32_t)min((uint64_t)a.chunk_len, a.n - cs);
    const bool is_final = SEG ? (t.chunks[c].flags & SEG_LAST) != 0 : a.final_last && (c + 1 == a.nchunks);
    const uint32_t* h = a.hist_out + (uint64_t)c * HREC;
    uint32_t* rec = (uint32_t*)a.codes + (uint64_t)c * CREC;
    for (int i = lane; i < 288; i += 64) S.hlit[i] = h[i];
    if (lane < 32) { const uint32_t v = h[288 + lane]; S.hdist[lane] = v; S.hdist0[lane] = v; }
    __syncthreads();
    const uint32_t hdrBits = build_block_codes<64>(S, a.dynamic != 0, is_final, rec + CREC_LIT, rec + CREC_DIST);
    // token bits incl. the end-of-block code: code length + extra bits per symbol occurrence; the
    // dummy literal of an empty block (:146-147) is in the histogram but never written
    const int ln = (int)S.misc[0], dn = (int)S.misc[1];
    uint64_t tok = 0;
    for (int t = lane; t < ln; t += 64) tok += (uint64_t)S.hlit[t] * (S.lens[t] + len_extra((uint32_t)t));
    if (lane < dn) tok += (uint64_t)S.hdist0[lane] * (S.lens[ln + lane] + dist_extra((uint32_t)lane));
    if (lane == 0 && a.dynamic && len_c == 0) tok -= S.lens[0];
    for (int i = lane; i < HDRW; i += 64) rec[CREC_HDR + i] = S.hdr()[i];
    tok = wave_sum(tok);
    if (lane == 0) {
        rec[CREC_META] = hdrBits;
        const uint64_t Sz = (uint64_t)hdrBits + tok;
        a.status[c] = Sz;
        if (a.chunk_bits) a.chunk_bits[c] = Sz;
    }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_codes_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) HuffScr S;
    deflate_codes<false>(a, S);
}
extern "C" __global__ void __launch_bounds__(64)
ndfl_deflate_codes_seg_kernel(Args a, SegTab t) {
    __shared__ __attribute__((aligned(16))) HuffScr S;
    deflate_codes<true>(a, S, t);
}

// Pass 3: chunk c's global bit offset = base + sum of the sizes before it; total[0] = end bit.  Two
// launches (ndfl_common.hpp scan_tile_*): the tile sums, then each tile's scan; grid = tiles.
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_deflate_offsets_sum_kernel(const uint64_t* sizes, uint32_t n, uint64_t* part) {
    scan_tile_sum([&](uint32_t i) { return sizes[i]; }, n, part);
}
extern "C" __global__ void __launch_bounds__(SCAN_T)
ndfl_deflate_offsets_kernel(const uint64_t* sizes, uint32_t n, uint64_t base, uint64_t* off, uint64_t* total,
                            const uint64_t* part) {
    scan_tile_apply([&](uint32_t i) { return sizes[i]; }, [&](uint32_t i, uint64_t v) { off[i] = v; }, n, part, base,
                    total);
}

// Pass 3 under SEG, after the two launches above have scanned all chunks' sizes into `raw` (base 0):
// the scan restarts at every stream's base.  Chunk k of stream s starts at bit 8 * obase[s] + raw[k] -
// raw[first chunk of s] of the staged output; sizes[k] becomes the chunk's inclusive prefix there, as
// a look-back would have published it (a stream's end is its last chunk's).
extern "C" __global__ void __launch_bounds__(256)
ndfl_deflate_offsets_seg_kernel(const uint64_t* raw, uint64_t* sizes, uint32_t n, SegTab t, uint64_t* off) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const SegStream st = t.streams[t.chunks[k].stream];
    const uint64_t o = 8 * st.obase + (raw[k] - raw[st.first_chunk]);
    off[k] = o;
    sizes[k] = ST_PRE | (o + sizes[k]);
}
