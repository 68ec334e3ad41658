// seg_tables.hpp -- the tables of the segmented (SEG = true) chunk encoders: chunk k of the launch
// belongs to stream `stream` (ndfl_deflate_batch_chunked, csrc/capi/ndfl_deflate_batch_chunked.cpp).
//
// The staged input gives every stream a slot of whole chunks: the stream's first byte sits at a
// multiple of chunk_len of the staged data, so chunk k still starts at k * chunk_len and the tile,
// chunk and parent arithmetic of the chunk encoders holds.  What a chunk no longer derives from its
// index comes from its record: its length (a stream's last chunk is short, an empty stream's only
// chunk is empty), where its stream starts (the window stops there), and whether it is the stream's
// first chunk (no history, no look-back, the stream's own output base) or its last (BFINAL).
#pragma once
#include <stdint.h>

enum : uint32_t {
    SEG_FIRST = 1u,                   // the stream's first chunk
    SEG_LAST = 2u,                    // the stream's last chunk: its block is final
    SEG_SUM_SHIFT = 4                 // bits 4..5: the stream's checksum kind (NDFL_SUM_*)
};

struct SegChunk {
    uint64_t start;                   // staged position of the stream's first byte (a multiple of chunk_len)
    uint64_t src;                     // the chunk's first byte in the caller's `in`
    uint32_t stream;
    uint32_t len;                     // chunk_len, the stream's tail, or 0
    uint32_t flags;                   // SEG_*
    uint32_t pad;
};                                    // 32 bytes

struct SegStream {
    uint64_t obase;                   // the stream's first byte in the staged output (a multiple of 4)
    uint32_t first_chunk, nchunks;
};                                    // 16 bytes

// What a segmented kernel gets next to its sibling's arguments.  SEG = false kernels pass SegTab{}:
// nothing of it is read.
struct SegTab {
    const SegChunk* chunks = nullptr;
    const SegStream* streams = nullptr;
};
