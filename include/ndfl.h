/*
 * ndfl.h -- C ABI of the MI355X-native DEFLATE codec (libndfl.so).
 *
 * This is the drop-in boundary for nayuki/DEFLATE-library-Java's encode/decode hot path.  Each
 * entry point names the reference interface it replaces (D/ = src/io/nayuki/deflate/ in the
 * reference).  Plain pointers and sizes only; no torch types.  Buffers are caller-owned; the
 * library never keeps a pointer past return.  A context owns device scratch and one HIP stream;
 * calls on one context are not reentrant, calls on different contexts are.
 *
 * Return convention (all int-returning calls):
 *     0                 success
 *     1 .. 19           DataFormatException.Reason ordinal + 1 (D/DataFormatException.java:61-83)
 *     < 0               NDFL_E_* (usage / device errors; map to IllegalArgument/IOException)
 */
#ifndef NDFL_H
#define NDFL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NDFL_ABI_VERSION 1u

/* error codes */
#define NDFL_OK               0
#define NDFL_E_ARG          (-1)   /* IllegalArgumentException / NullPointerException */
#define NDFL_E_UNSUPPORTED  (-2)   /* configuration not implemented on the GPU path */
#define NDFL_E_CAPACITY     (-3)   /* output buffer too small; required size reported */
#define NDFL_E_DEVICE       (-4)   /* HIP runtime error (IOException) */
#define NDFL_E_STATE        (-5)   /* IllegalStateException (use after finish/close) */
#define NDFL_E_INTERNAL     (-6)

/* DataFormatException.Reason ordinal + 1 */
enum ndfl_reason {
    NDFL_UNEXPECTED_END_OF_STREAM = 1, NDFL_RESERVED_BLOCK_TYPE, NDFL_UNCOMPRESSED_BLOCK_LENGTH_MISMATCH,
    NDFL_HUFFMAN_CODE_UNDER_FULL, NDFL_HUFFMAN_CODE_OVER_FULL, NDFL_NO_PREVIOUS_CODE_LENGTH_TO_COPY,
    NDFL_CODE_LENGTH_CODE_OVER_FULL, NDFL_END_OF_BLOCK_CODE_ZERO_LENGTH, NDFL_RESERVED_LENGTH_SYMBOL,
    NDFL_RESERVED_DISTANCE_SYMBOL, NDFL_LENGTH_ENCOUNTERED_WITH_EMPTY_DISTANCE_CODE,
    NDFL_COPY_FROM_BEFORE_DICTIONARY_START, NDFL_HEADER_CHECKSUM_MISMATCH, NDFL_UNSUPPORTED_COMPRESSION_METHOD,
    NDFL_DECOMPRESSED_CHECKSUM_MISMATCH, NDFL_DECOMPRESSED_SIZE_MISMATCH, NDFL_GZIP_INVALID_MAGIC_NUMBER,
    NDFL_GZIP_RESERVED_FLAGS_SET, NDFL_GZIP_UNSUPPORTED_OPERATING_SYSTEM
};

/* Strategy ids: the Lz77Huffman presets (D/comp/Lz77Huffman.java:298-305) and Uncompressed. */
enum ndfl_strategy {
    NDFL_LITERAL_STATIC = 0, NDFL_LITERAL_DYNAMIC = 1, NDFL_RLE_STATIC = 2, NDFL_RLE_DYNAMIC = 3,
    NDFL_FULL_STATIC = 4, NDFL_FULL_DYNAMIC = 5, NDFL_UNCOMPRESSED = 6
};

/* memory flags */
#define NDFL_IN_DEVICE   1u    /* input pointers (data, hist) are device memory */
#define NDFL_OUT_DEVICE  2u    /* output pointer is device memory */
#define NDFL_DICT_DEFERRED 4u  /* ndfl_inflate_range: window bytes are written later (see resolve) */
#define NDFL_IN_PADDED   8u    /* ndfl_inflate / ndfl_inflate_range with NDFL_IN_DEVICE: the input is
                                 16-byte aligned and followed by NDFL_IN_PAD_BYTES readable zero bytes,
                                 so it is decoded in place (no staging copy); otherwise ignored */
#define NDFL_IN_PAD_BYTES 256u
#define NDFL_IN_PARTIAL  16u   /* ndfl_inflate_range: `in` is a prefix of the stream (more input may
                                 follow); see NDFL_NEED_INPUT */

/* ndfl_inflate_range with NDFL_IN_PARTIAL: the decode ran out of input inside a block.  Nothing is
 * reported for that block: *consumed_bits is its start (the last block boundary reached) and
 * *out_len the bytes decoded before it.  The caller continues from there with more input and the
 * last <= 32 KiB of output as the window -- Open.read's incremental refill
 * (D/decomp/Open.java:137-192) at block granularity.  Not a Reason: at true end of input the
 * caller decodes without the flag and gets UNEXPECTED_END_OF_STREAM. */
#define NDFL_NEED_INPUT  64

typedef struct ndfl_ctx ndfl_ctx;

uint32_t ndfl_abi_version(void);
const char* ndfl_error_string(int code);

/* Create a context on HIP device `device`.  Fails with NDFL_E_DEVICE if no GPU.
 * The NDFL_* environment switches (test hand-over paths, statistics, A/B alternatives: the Knobs of
 * csrc/hip/ndfl_common.hpp; none is needed in production) are read ONCE, here: setting or changing
 * one after a context exists has no effect on it -- create a new context to measure another
 * setting.  A switch is on when set to anything but "0".  With NDFL_STATS on, the context prints its
 * effective switches once to stderr, so a profiling run shows which path it measured. */
int ndfl_ctx_create(ndfl_ctx** out, int device, uint32_t flags);
int ndfl_ctx_destroy(ndfl_ctx* ctx);
/*
 * Stream ordering (every call that reads or writes device memory: NDFL_IN_DEVICE / NDFL_OUT_DEVICE
 * buffers, ndfl_bits_shift, the deferred-window resolve).  By default a call's device work is
 * ordered after all work queued earlier on the device's default (NULL) stream, so a buffer just
 * produced there -- or a freed block a caching allocator hands out again while a kernel on that
 * stream still uses it -- is safe to pass without a host synchronize.  A caller that works on
 * another stream names it with ndfl_ctx_set_stream: the calls then run on that stream, in order
 * with the caller's own work (NULL restores the default).  Every call completes its device work
 * before it returns, so its outputs may be used right away on any stream.
 */
int ndfl_ctx_set_stream(ndfl_ctx* ctx, void* hip_stream);
/* Average device time (ms) of the last call's dominant kernel, measured with HIP events. */
double ndfl_ctx_last_kernel_ms(ndfl_ctx* ctx);
/* Device-time breakdown of the last calls (ms): [0] deflate kernel, [1] inflate finder,
 * [2] inflate count, [3] inflate emit, [4] inflate device span, [5] linked chains, [6] repaired
 * boundaries, [7] header candidates, [8] chains whose first block the count pass decoded one lane
 * per block (escape-prefix literal codes), [9] 32-byte output groups still pending after the six
 * device-queued resolve rounds of the last ndfl_inflate / ndfl_inflate_range (> 0: the host-checked
 * rounds ran; 0 on the host-link path and for NDFL_DICT_DEFERRED decodes).  Returns the number of
 * entries written (<= 10). */
int ndfl_ctx_timings(ndfl_ctx* ctx, double* ms, int n);
/* The reserved symbol behind the last ndfl_inflate / ndfl_inflate_range that returned
 * NDFL_RESERVED_LENGTH_SYMBOL (286 or 287) or NDFL_RESERVED_DISTANCE_SYMBOL (30 or 31), else -1:
 * the reference's message names it -- "Reserved run length symbol: " + sym,
 * "Reserved distance symbol: " + sym (D/decomp/Open.java:516, 550, 659, 674). */
int ndfl_ctx_error_symbol(ndfl_ctx* ctx);

/*
 * Compress K consecutive chunks of one DEFLATE stream.
 * Replaces K iterations of DeflaterOutputStream.writeBuffer (D/DeflaterOutputStream.java:119-137),
 * i.e. Strategy.decide(b, off, historyLen, dataLen) + Decision.compressTo(bitOut, isFinal)
 * (D/comp/Strategy.java:14, D/comp/Decision.java:16-19, D/comp/Lz77Huffman.java:42-286) and the
 * BitOut packing (D/DeflaterOutputStream.java:141-171).  Batching is exact because the default
 * decisions depend only on raw input, never on earlier output.
 *   hist/hist_len   the min(historyLookbehindLimit, pos) raw bytes preceding `data`
 *   data/len        K chunks: chunk_len bytes each, the last one 0..chunk_len bytes
 *   final_flag      1 if the last chunk is the stream's final chunk (bfinal=1); if 0, every
 *                   chunk must be full (len % chunk_len == 0, len > 0)
 *   hist_limit      historyLookbehindLimit (0..32768) -- decides whether history exists
 *   start_bitpos    BitOutputStream.getBitPosition() before the first block (0..7): the output
 *                   begins at that bit of out[0]; bits below it are written as 0 (caller ORs)
 *   out/out_cap     output bytes; on success *out_end_bits = start_bitpos + bits written
 *   crc_inout       optional: java.util.zip.CRC32 value updated with `data` (GzipOutputStream)
 * Returns 0, NDFL_E_UNSUPPORTED (chunk_len > 65536), NDFL_E_CAPACITY
 * (*out_end_bits = bits required), ...  FULL_STATIC / FULL_DYNAMIC run ndfl_deflate_chunks_lz77
 * with (3, 258, 1, 32768).
 */
int ndfl_deflate_chunks(ndfl_ctx* ctx, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                        const uint8_t* data, uint64_t len, uint32_t chunk_len, int strategy,
                        int final_flag, uint32_t start_bitpos, uint8_t* out, uint64_t out_cap,
                        uint64_t* out_end_bits, uint32_t* crc_inout, uint32_t flags);

/*
 * Same as ndfl_deflate_chunks for an explicit Lz77Huffman(useDynamicHuffmanCodes,
 * searchMinimumRunLength, searchMaximumRunLength, searchMinimumDistance, searchMaximumDistance)
 * strategy (D/comp/Lz77Huffman.java:20-39 record + validation, :62-130 greedy longest-match parse
 * with the smallest distance on ties).  (0,0,0,0) is the literal-only form; parameters outside
 * 3 <= minRun <= maxRun <= 258, 1 <= minDist <= maxDist <= 32768 give NDFL_E_ARG
 * (IllegalArgumentException, :37-38).  The FULL_* presets are (3, 258, 1, 32768).
 */
int ndfl_deflate_chunks_lz77(ndfl_ctx* ctx, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                             const uint8_t* data, uint64_t len, uint32_t chunk_len, int dynamic, int min_run,
                             int max_run, int min_dist, int max_dist, int final_flag, uint32_t start_bitpos,
                             uint8_t* out, uint64_t out_cap, uint64_t* out_end_bits, uint32_t* crc_inout,
                             uint32_t flags);

/* A substrategy of ndfl_deflate_chunks_multi: an Lz77Huffman record or Uncompressed.SINGLETON. */
#define NDFL_KIND_LZ77          0
#define NDFL_KIND_UNCOMPRESSED  1
typedef struct {
    int32_t kind;                                     /* NDFL_KIND_* */
    int32_t dynamic, min_run, max_run, min_dist, max_dist;   /* Lz77Huffman components (kind LZ77) */
} ndfl_strategy_desc;

/*
 * Same as ndfl_deflate_chunks for a MultiStrategy(strats...) (D/comp/MultiStrategy.java:31-57)
 * over up to 8 Lz77Huffman / Uncompressed substrategies (n_strats = 1 gives that strategy alone):
 * per chunk, the first substrategy with the fewest bits at the current output bit position
 * (Decision.getBitLengths, D/comp/Decision.java:16-19; Uncompressed's depend on the position,
 * D/comp/Uncompressed.java:22-26).  NDFL_UNCOMPRESSED in ndfl_deflate_chunks runs this with the
 * single Uncompressed substrategy.
 */
int ndfl_deflate_chunks_multi(ndfl_ctx* ctx, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                              const uint8_t* data, uint64_t len, uint32_t chunk_len, const ndfl_strategy_desc* strats,
                              uint32_t n_strats, int final_flag, uint32_t start_bitpos, uint8_t* out,
                              uint64_t out_cap, uint64_t* out_end_bits, uint32_t* crc_inout, uint32_t flags);

/*
 * Same as ndfl_deflate_chunks for BinarySplit(sub, minBlockLen) (D/comp/BinarySplit.java:21-82) over
 * an Lz77Huffman substrategy: each chunk halves recursively while both halves exceed
 * min_block_len (>= 1, else NDFL_E_ARG), keeping a split when it takes fewer bits; the sub-blocks'
 * history starts at their chunk's.  NDFL_E_UNSUPPORTED for other substrategies, for halvings of
 * an odd length inside full chunks, or for more than 8192 node encodes in a partial final chunk.
 */
int ndfl_deflate_chunks_binsplit(ndfl_ctx* ctx, const uint8_t* hist, uint32_t hist_len, uint32_t hist_limit,
                                 const uint8_t* data, uint64_t len, uint32_t chunk_len, const ndfl_strategy_desc* sub,
                                 int32_t min_block_len, int final_flag, uint32_t start_bitpos, uint8_t* out,
                                 uint64_t out_cap, uint64_t* out_end_bits, uint32_t* crc_inout, uint32_t flags);

/*
 * The compressor plugin API (D/comp/Strategy.java:14, D/comp/Decision.java:16-19): one chunk,
 * any strategy tree.  A strategy is an array of nodes; node `root` is the strategy:
 *   NDFL_KIND_LZ77          Lz77Huffman(dynamic, min_run, max_run, min_dist, max_dist)
 *   NDFL_KIND_UNCOMPRESSED  Uncompressed.SINGLETON
 *   NDFL_KIND_MULTI         MultiStrategy(nodes[first_child .. first_child + n_children))
 *   NDFL_KIND_BINSPLIT      BinarySplit(nodes[first_child], min_block_len)
 * ndfl_decide = Strategy.decide(b, off, historyLen, dataLen) on the GPU encoders: the data is
 * b[off + history_len, + data_len) (host memory, <= 65536 bytes), preceded by its history;
 * bit_lengths[i] = Decision.getBitLengths()[i], the block's bits when it starts at bit position
 * i (mod 8).  The decision keeps a pointer to `b` (as the Java Decision closes over it): keep b
 * valid until the decision is freed.  NDFL_E_ARG for the constructors' IllegalArgumentExceptions
 * (Lz77Huffman parameters, empty MultiStrategy, minBlockLen < 1) and malformed trees.
 * ndfl_compress_to = Decision.compressTo(out, isFinal): writes the block(s) at bit start_bitpos of
 * out[0] (lower bits kept), *out_end_bits = start_bitpos + bits written.
 */
#define NDFL_KIND_MULTI         2
#define NDFL_KIND_BINSPLIT      3
typedef struct {
    int32_t kind;                                        /* NDFL_KIND_* */
    int32_t dynamic, min_run, max_run, min_dist, max_dist;   /* LZ77 */
    int32_t first_child, n_children;                     /* MULTI / BINSPLIT (n_children unused) */
    int32_t min_block_len;                               /* BINSPLIT */
} ndfl_strategy_node;
typedef struct ndfl_decision ndfl_decision;
int ndfl_decide(ndfl_ctx* ctx, const ndfl_strategy_node* nodes, uint32_t n_nodes, uint32_t root, const uint8_t* b,
                uint64_t off, uint32_t history_len, uint32_t data_len, uint64_t* bit_lengths, ndfl_decision** out);
int ndfl_compress_to(ndfl_ctx* ctx, const ndfl_decision* dec, int is_final, uint32_t start_bitpos, uint8_t* out,
                     uint64_t out_cap, uint64_t* out_end_bits);
int ndfl_decision_free(ndfl_decision* dec);

/* Upper bound of output bytes of ndfl_deflate_chunks for `len` bytes. */
uint64_t ndfl_deflate_bound(uint64_t len, uint32_t chunk_len);

/*
 * Decompress one raw DEFLATE stream held entirely in `in`.
 * Replaces InflaterInputStream.read / Open.read (D/InflaterInputStream.java:147-164,
 * D/decomp/Open.java:83-124) run to end of stream.  Trailing bytes after the final block are
 * ignored; *consumed_bits is the bit position just after the final block (endExactly
 * repositioning uses ceil(consumed_bits/8), D/decomp/Open.java:113-124).
 * Returns 0, a Reason code (with *out_len = bytes decoded before the error), NDFL_E_CAPACITY
 * (*out_len = bytes required), or a negative error.
 */
int ndfl_inflate(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                 uint64_t* out_len, uint64_t* consumed_bits, uint32_t flags);

/*
 * Decompress n independent raw DEFLATE streams in one call: one kernel launch and one host sync
 * whatever n is (ndfl_inflate costs several launches and two syncs per stream).  Each stream is
 * decoded as ndfl_inflate decodes it -- InflaterInputStream.read / Open.read run to the end of the
 * stream, the reference's checks in the reference's order, trailing bytes after the final block
 * ignored -- by one wave, serially: the call is for MANY SMALL streams (zip entries, PNG IDAT
 * payloads, per-record zlib bodies).
 * Crossover (measured on one MI355X, DESIGN.md §4 "Batched inflate"): a wave decodes about 4 MB/s
 * of output on 4 KiB streams and 7.6 MB/s on 1 MiB streams, and up to 1,024 waves run at once;
 * ndfl_inflate costs about 0.57 ms per call plus 4 ns per output byte up to 1 MiB.  So one stream
 * alone is faster through ndfl_inflate above about 4.5 KiB of output, ten streams above about 47 KiB
 * each, and from about 34 streams on the batch is never slower for streams up to 1 MiB (256 x 1 MiB:
 * 136 ms in a batch, 1,201 ms in a loop).  Streams of hundreds of MiB, which ndfl_inflate decodes at
 * tens of GB/s by working inside the stream, belong there whatever their number.
 *   in/in_size, out/out_size   the two buffers all items point into; NDFL_IN_DEVICE, NDFL_OUT_DEVICE
 *               and NDFL_IN_PADDED (for the whole `in`) exactly as for ndfl_inflate
 *   items       host memory.  Stream i is in[in_off, in_off + in_len): its input ends there (it never
 *               sees its neighbour's bytes), and its dictionary starts empty at its own out_off (a
 *               distance that reaches before it is COPY_FROM_BEFORE_DICTIONARY_START whatever lies
 *               there in `out`).  Input regions may overlap or repeat; output regions must not overlap.
 *   results     host memory, one per stream.  Status precedence: a Reason wins -- out_len is then
 *               the bytes decoded before the error, of which the first min(out_len, out_cap) are
 *               stored; otherwise a stream that decodes to more than out_cap bytes has status
 *               NDFL_E_CAPACITY and out_len = the bytes required (the decode goes on without storing
 *               past out_cap, so a later Reason still wins); otherwise 0.  consumed_bits (status 0) is
 *               relative to the stream's own first bit.  error_symbol is this stream's
 *               ndfl_ctx_error_symbol value (ndfl_ctx_error_symbol itself is not changed by the call).
 * No byte of `out` outside [out_off, out_off + min(out_len, out_cap)) of some stream is written,
 * whatever the statuses.
 * Returns 0 when the batch ran (per-stream outcomes are in `results` only; n == 0 returns 0 and
 * touches nothing); NDFL_E_ARG for null pointers with n > 0, an item outside in_size / out_size, or
 * overlapping output regions (nothing is decoded); NDFL_E_DEVICE on HIP errors.
 * ndfl_ctx_last_kernel_ms reports the batch kernel's time.
 */
typedef struct {
    uint64_t in_off, in_len;     /* stream i is in[in_off, in_off + in_len) */
    uint64_t out_off, out_cap;   /* its output region is out[out_off, out_off + out_cap) */
} ndfl_batch_item;
typedef struct {
    int32_t  status;             /* 0, Reason+1 (1..19), or NDFL_E_CAPACITY */
    int32_t  error_symbol;       /* as ndfl_ctx_error_symbol for this stream, else -1 */
    uint64_t out_len;            /* as ndfl_inflate; with NDFL_E_CAPACITY: bytes required */
    uint64_t consumed_bits;      /* relative to the stream's own first bit */
} ndfl_batch_result;
int ndfl_inflate_batch(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                       const ndfl_batch_item* items, ndfl_batch_result* results, uint32_t n, uint32_t flags);

/*
 * ndfl_inflate_batch for container members, with the checksum taken in the same launch: item i is a
 * zlib member (ZlibInputStream: D/ZlibInputStream.java, header D/ZlibMetadata.java:47-80), ONE gzip
 * member (GzipInputStream: D/GzipInputStream.java, header D/GzipMetadata.java:73-146), or a raw
 * DEFLATE stream whose CRC-32 or Adler-32 the caller wants (a zip entry: its CRC-32 is in the
 * directory).  Still one kernel launch and one host sync whatever n is: the header is parsed, the
 * output checksummed on its way out of the decoder, and the trailer compared, by the wave that
 * decodes the stream.  Buffers, items' regions, flags, stream ordering, ndfl_ctx_last_kernel_ms and
 * the "no byte of `out` outside a stream's stored bytes is written" rule are ndfl_inflate_batch's.
 *
 * NDFL_FMT_RAW   status, error_symbol, out_len, consumed_bits and the stored bytes are exactly
 *                ndfl_inflate_batch's for the same item.  checksum = the java.util.zip.CRC32 value
 *                (NDFL_SUM_CRC32; initial 0) or the Adler-32 (NDFL_SUM_ADLER32; initial 1) of ALL out_len
 *                decoded bytes, those past out_cap included: valid when status is 0 or NDFL_E_CAPACITY,
 *                0 on a Reason and with NDFL_SUM_NONE.  header_len = 0.
 * NDFL_FMT_ZLIB  the header checks are ZlibMetadata.read's, in its order (D/ZlibMetadata.java:47-80):
 *                fewer than 2 bytes: UNEXPECTED_END_OF_STREAM; (CMF << 8 | FLG) % 31 != 0:
 *                HEADER_CHECKSUM_MISMATCH; a method other than 8 or 15: UNSUPPORTED_COMPRESSION_METHOD
 *                (15 is accepted and decoded as DEFLATE, as the reference does); FDICT: 4 more bytes
 *                are skipped (UNEXPECTED_END_OF_STREAM if absent; the dictionary stays empty); method 8
 *                with CINFO > 7 is the record constructor's IllegalArgumentException: this stream's
 *                status is NDFL_E_ARG, its out_len 0.  The DEFLATE data is decoded as for RAW; the 4
 *                trailer bytes follow at header_len + ceil(bits / 8) (fewer: UNEXPECTED_END_OF_STREAM)
 *                and hold the big-endian Adler-32 of the output, else DECOMPRESSED_CHECKSUM_MISMATCH
 *                (D/ZlibInputStream.java:57-79).
 * NDFL_FMT_GZIP  the header checks are GzipMetadata.read's, in its order (D/GzipMetadata.java:73-146):
 *                magic (GZIP_INVALID_MAGIC_NUMBER), method != 8 (UNSUPPORTED_COMPRESSION_METHOD),
 *                flags & 0xE0 (GZIP_RESERVED_FLAGS_SET), MTIME (4 bytes), XFL, an OS byte that is neither
 *                < 14 nor 255 (GZIP_UNSUPPORTED_OPERATING_SYSTEM), FEXTRA (2-byte little-endian length,
 *                then that many bytes), FNAME and FCOMMENT (each to a 0 byte), FHCRC (the low 16 bits of
 *                the CRC-32 of all header bytes before it, else HEADER_CHECKSUM_MISMATCH); a missing byte
 *                anywhere is UNEXPECTED_END_OF_STREAM.  The DEFLATE data is decoded as for RAW; 8 trailer
 *                bytes follow (fewer: UNEXPECTED_END_OF_STREAM): a CRC-32 that differs from the output's
 *                is DECOMPRESSED_CHECKSUM_MISMATCH, otherwise (uint32_t)out_len != ISIZE is
 *                DECOMPRESSED_SIZE_MISMATCH -- the checksum is tested first (D/GzipInputStream.java:76-87).
 * Both containers: `sum` is not read.  checksum = the value computed over the output, valid as for RAW
 * and on the two mismatch Reasons.  header_len = the bytes before the DEFLATE data once the header is
 * accepted, else 0.  On status 0 consumed_bits = 8 x the member's length in bytes (header,
 * ceil(bits / 8), trailer), so in_off + consumed_bits / 8 is the next member of a concatenation; bytes
 * after the trailer are ignored.  out_len is 0 on a header error; on a trailer error it is the whole
 * decoded length, and those bytes are stored.  DEFLATE errors report as for RAW, with error_symbol.
 * Precedence as in ndfl_inflate_batch: a Reason, or the per-stream NDFL_E_ARG, wins over
 * NDFL_E_CAPACITY -- the checksum covers the bytes past out_cap, so a member that overflows its region
 * AND has a bad trailer reports the mismatch.
 * Returns as ndfl_inflate_batch; in addition NDFL_E_ARG when an item's format > 2 or sum > 2 (nothing
 * is decoded).
 * Against ndfl_inflate_batch followed by one ndfl_crc32 / ndfl_adler32 call per stream (measured on
 * one MI355X, DESIGN.md §4 "Batched inflate of container members"): 65,536 x 512 B take 13.0 to 13.9 ms
 * instead of 4.7 to 5.3 s, 4,096 x 4 KiB 4.2 to 4.3 ms instead of 290 to 347 ms, 256 x 1 MiB 136 to
 * 137 ms instead of 155 to 164 ms.  The kernel's time against ndfl_inflate_batch's on the same streams:
 * Adler-32 within +-1.6 %, CRC-32 +0.3 to +0.6 % from 4 KiB streams up and +4.7 to +5.5 % on 512-byte
 * streams.  The crossover to ndfl_inflate is ndfl_inflate_batch's.
 */
#define NDFL_FMT_RAW   0u   /* raw DEFLATE, as ndfl_inflate_batch */
#define NDFL_FMT_ZLIB  1u   /* ZlibInputStream (D/ZlibInputStream.java, D/ZlibMetadata.java:47-80) */
#define NDFL_FMT_GZIP  2u   /* GzipInputStream, one member (D/GzipInputStream.java, D/GzipMetadata.java:73-146) */
#define NDFL_SUM_NONE    0u
#define NDFL_SUM_CRC32   1u
#define NDFL_SUM_ADLER32 2u
typedef struct {
    uint64_t in_off, in_len, out_off, out_cap;   /* as ndfl_batch_item */
    uint32_t format;                             /* NDFL_FMT_* */
    uint32_t sum;                                /* NDFL_SUM_*: read for NDFL_FMT_RAW only */
} ndfl_member_item;                              /* 40 bytes */
typedef struct {
    int32_t  status, error_symbol;               /* as ndfl_batch_result (status also NDFL_E_ARG: zlib CINFO > 7) */
    uint64_t out_len, consumed_bits;
    uint32_t checksum, header_len;
} ndfl_member_result;                            /* 32 bytes */
int ndfl_inflate_members(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                         const ndfl_member_item* items, ndfl_member_result* results, uint32_t n, uint32_t flags);

/*
 * Decompress a blocked gzip file (BGZF: bgzip, BAM, tabix-indexed VCF / BED) in one call.  Such a file is
 * a concatenation of gzip members of at most 64 KiB, each carrying its own length in a `BC` subfield of
 * its extra field (BSIZE) and its output length in its trailer (ISIZE), so the members are found and
 * the output laid out on the device without decoding a bit; ndfl_inflate_members' kernel then decodes
 * them all in one launch.  The number of launches grows only with the logarithm of the file's size (the
 * rounds that mark the chain), not with the number of members, and the host syncs twice: once for the
 * sizes, once at the end.
 *
 * Member start: p is one when in[p, p + 3) = 1f 8b 08, FLG (in[p + 3]) has bit 2, the 12 fixed bytes and
 *   all XLEN extra bytes lie inside in_len, the walk over the extra field's subfields (SI1, SI2, 2-byte
 *   LEN, LEN bytes) meets SI1 = 66, SI2 = 67, LEN = 2 with its two bytes inside the field, and BSIZE + 1
 *   >= 12 + XLEN + 8.  Nothing else of the header is looked at here: reserved flags, the OS byte, FNAME /
 *   FCOMMENT and FHCRC are checked by the decode, in the reference's order, as that member's Reason.
 * Chain:  member 0 is at byte 0 and member k + 1 at off[k] + BSIZE[k] + 1.  The chain ends at in_len or
 *   at the first position that is not a member start; that position is consumed_bytes, and the bytes
 *   after it are ignored, as ndfl_inflate ignores trailing bytes (a missing EOF marker is no error).
 *   Byte 0 not a member start: n_members = 0, status 0, out_len 0, consumed_bytes 0.  A member whose
 *   BSIZE runs past in_len gets the in_len - off[k] bytes there are and fails in the decode
 *   (UNEXPECTED_END_OF_STREAM) like any truncated member.  Look-alike headers off the chain -- inside
 *   a stored block, say -- are not members.
 * Layout: ISIZE[k] is the little-endian u32 in the member's last 4 bytes; out_off[k] is the exclusive
 *   64-bit sum of the ISIZEs and member k's region is ISIZE[k] bytes.  A total above out_cap returns
 *   NDFL_E_CAPACITY with out_len = the total: nothing is decoded and no byte of `out` is written.  So
 *   out = NULL, out_cap = 0 is the sizing and index call -- which TRUSTS the ISIZE fields: the size it
 *   reports is what a well-formed file decodes to, and a file that lies fails in the decoding call.
 *   table (host memory, may be NULL with table_cap = 0) receives min(table_cap, n_members + 1)
 *   entries, in every case; entry n_members is (consumed_bytes, total).
 * Decode: every member as an NDFL_FMT_GZIP item of ndfl_inflate_members, its dictionary empty.  A wrong
 *   ISIZE, too small or too large, is therefore DECOMPRESSED_SIZE_MISMATCH, the checksum is tested
 *   first, and a Reason wins over capacity.  (Bytes between a member's trailer and off + BSIZE + 1 are
 *   ignored by the decode; the layout still reads ISIZE from the member's last 4 bytes, and a member
 *   that decodes without a Reason to another length is DECOMPRESSED_SIZE_MISMATCH too.)
 * Result: the failing member with the LOWEST index decides, whatever order the members were decoded
 *   in.  On a Reason out_len = out_off[bad] + the bytes member `bad` decoded before the error, of which
 *   the first min(that, ISIZE[bad]) are stored, as ndfl_inflate_batch stores min(out_len, out_cap): out
 *   holds the file's bytes up to out_off[bad] + min(the member's out_len, ISIZE[bad]) -- with an ISIZE
 *   that is too small out_len lies past that, in the next member's region.  The bytes from there to the
 *   total are unspecified; no byte at or past the total is ever written.
 * Returns result->status, or NDFL_E_ARG (null ctx / result, null buffers with a size), NDFL_E_UNSUPPORTED
 * (in_len above 8 GiB), NDFL_E_DEVICE.  flags (NDFL_IN_DEVICE, NDFL_OUT_DEVICE, NDFL_IN_PADDED) and stream
 * ordering as for ndfl_inflate_members.  ndfl_ctx_last_kernel_ms covers all the call's kernels; of
 * ndfl_ctx_timings, [1] is the part up to the layout's end and [3] the decode with the reduction.
 */
typedef struct { uint64_t in_off, out_off; } ndfl_bgzf_member;
typedef struct {
    int32_t  status;          /* 0, Reason+1 of the FIRST failing member in file order, or NDFL_E_CAPACITY */
    int32_t  error_symbol;    /* that member's, else -1 */
    uint32_t n_members;       /* members on the chain from byte 0 */
    uint32_t bad_member;      /* index of the failing member, else n_members */
    uint64_t out_len;         /* status 0: total output; Reason: out_off[bad] + that member's out_len;
                                 NDFL_E_CAPACITY: bytes required */
    uint64_t consumed_bytes;  /* offset just past the last member of the chain */
} ndfl_bgzf_result;
int ndfl_inflate_bgzf(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                      ndfl_bgzf_result* result, ndfl_bgzf_member* table, uint32_t table_cap, uint32_t flags);

/*
 * Compress n independent buffers in one call: one kernel launch and one host sync whatever n is
 * (ndfl_deflate_chunks costs about eight launches and a sync per buffer).  The encoder's counterpart of
 * ndfl_inflate_batch / ndfl_inflate_members, with their items read the other way round: item i's raw
 * bytes are in[in_off, in_off + in_len), its compressed member goes to out[out_off, out_off + out_cap).
 * Stream i is exactly DeflaterOutputStream(out, chunk_len, hist_limit, strategy): write all bytes, then
 * finish() (D/DeflaterOutputStream.java:119-171).  Its DEFLATE bytes are bit-identical to
 * ndfl_deflate_chunks(ctx, NULL, 0, hist_limit, data_i, len_i, chunk_len, strategy, 1, 0, ...): the
 * stream starts at bit 0 of out[out_off], the unused high bits of its last DEFLATE byte are 0, an empty
 * buffer gives the one empty final block, and a stream never sees a neighbour's bytes (chunk 0 has no
 * history; a later chunk has its own stream's previous byte, and only when hist_limit > 0).  One wave
 * encodes a stream, chunk by chunk: the call is for MANY SMALL buffers (per-record zlib bodies, PNG IDAT
 * payloads, zip entries, small gzip members).
 *   strategy    NDFL_LITERAL_STATIC, NDFL_LITERAL_DYNAMIC, NDFL_RLE_STATIC or NDFL_RLE_DYNAMIC.
 *               NDFL_FULL_* and NDFL_UNCOMPRESSED return NDFL_E_UNSUPPORTED for the call and nothing is
 *               written: the LZ77 search is ndfl_deflate_batch_lz77's, Uncompressed and a per-chunk choice
 *               among several strategies ndfl_deflate_batch_multi's.
 *   chunk_len   1..65536 (0: NDFL_E_ARG; above 65536: NDFL_E_UNSUPPORTED, as ndfl_deflate_chunks)
 *   hist_limit  0..32768, else NDFL_E_ARG
 *   format      NDFL_FMT_*.  A container's header does not depend on the data and is the caller's, written
 *               in front of out_off before or after the call; the trailer does, and the kernel appends it
 *               after the byte-aligned DEFLATE data:
 *                 NDFL_FMT_RAW   no trailer; checksum = the java.util.zip CRC-32 (initial 0) or Adler-32
 *                                (initial 1) of the input bytes as `sum` asks, 0 with NDFL_SUM_NONE
 *                 NDFL_FMT_ZLIB  4 bytes: the big-endian Adler-32 of the input (D/ZlibOutputStream.java);
 *                                checksum = the Adler-32; `sum` is not read
 *                 NDFL_FMT_GZIP  8 bytes: the CRC-32, then (uint32_t)in_len, both little-endian
 *                                (D/GzipOutputStream.java); checksum = the CRC-32; `sum` is not read
 *               The checksum is taken from the bytes on their way through the encoder, in the same launch.
 *   results     host memory, one per stream.  out_len = ceil(end_bits / 8) + the trailer's bytes.  A
 *               member longer than out_cap has status NDFL_E_CAPACITY and out_len = the bytes required;
 *               its first out_cap bytes are stored, and the other streams are unaffected.
 * No byte of `out` outside [out_off, out_off + min(out_len, out_cap)) of some stream is written, whatever
 * the statuses, at any byte alignment of `out` and out_off, with regions that touch: a stream's first
 * and last partial words go out as byte stores.
 * Buffers, NDFL_IN_DEVICE / NDFL_OUT_DEVICE (host buffers are staged through the context), stream
 * ordering and ndfl_ctx_last_kernel_ms as for ndfl_inflate_batch.  Input regions may overlap or repeat;
 * output regions must not overlap.
 * Returns 0 when the batch ran (n == 0 returns 0 and touches nothing); NDFL_E_ARG, with nothing encoded,
 * for null pointers with n > 0, an item outside in_size / out_size, overlapping output regions, or an
 * item's format > 2 or sum > 2; NDFL_E_DEVICE on HIP errors.
 * Crossover to ndfl_deflate_chunks (measured on one MI355X, RLE_DYNAMIC with a CRC-32, DESIGN.md §4 "Batched
 * deflate"): a loop of ndfl_deflate_chunks calls costs 0.16 to 0.27 ms per buffer up to 1 MiB, nearly all of it
 * per-call cost; the batch costs about 0.1 ms per call, a wave about 0.1 ms per stream plus 24 us per KiB (41 MB/s),
 * and up to 3,072 waves run at once.  65,536 x 512 B take 2.7 to 2.9 ms in a batch and 10.6 to 12.0 s in a loop,
 * 4,096 x 4 KiB 0.50 to 0.55 ms and 661 to 871 ms, 256 x 1 MiB 25 to 28 ms and 48 to 69 ms.  So one buffer alone
 * goes through ndfl_deflate_chunks; two buffers are faster in a batch below about 5 KB each, ten below about
 * 57 KB, a hundred below about 650 KB, 256 below about 1.7 MB.  A buffer of many MiB, which ndfl_deflate_chunks
 * encodes at tens of GB/s by working inside the stream, belongs there whatever the count.
 */
typedef struct {
    int32_t  status;             /* 0 or NDFL_E_CAPACITY */
    uint32_t checksum;           /* see above */
    uint64_t out_len;            /* bytes of the member; with NDFL_E_CAPACITY: bytes required */
    uint64_t end_bits;           /* DEFLATE bits written, from the stream's own bit 0 */
} ndfl_deflate_result;           /* 24 bytes */
int ndfl_deflate_batch(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                       const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                       int strategy, uint32_t chunk_len, uint32_t hist_limit, uint32_t flags);

/*
 * ndfl_deflate_batch with the LZ77 search: stream i is DeflaterOutputStream(out, chunk_len, hist_limit,
 * Lz77Huffman(dynamic, min_run, max_run, min_dist, max_dist)): write all bytes, then finish().  Still one
 * kernel launch and one host sync whatever n is (ndfl_deflate_chunks_lz77 costs three kernels of 1024-thread
 * workgroups and a sync per buffer).  Items, results, formats, `sum`, trailers, NDFL_E_CAPACITY with the
 * required size, the rule that no byte of `out` outside [out_off, out_off + min(out_len, out_cap)) is
 * written, flags, stream ordering, ndfl_ctx_last_kernel_ms, n == 0, overlapping or repeated input regions
 * and the argument errors are ndfl_deflate_batch's, word for word.
 *   dynamic, min_run, max_run, min_dist, max_dist
 *               as ndfl_deflate_chunks_lz77: (0, 0, 0, 0) is the literal-only form, anything else outside
 *               3 <= min_run <= max_run <= 258, 1 <= min_dist <= max_dist <= 32768 is NDFL_E_ARG;
 *               (3, 258, 1, 32768) is FULL_STATIC / FULL_DYNAMIC.  The literal-only and the (3, 258, 1, 1)
 *               forms run as ndfl_deflate_batch's LITERAL_* and RLE_* presets.
 *   chunk_len   1..65536 (0: NDFL_E_ARG; above 65536: NDFL_E_UNSUPPORTED)
 *   hist_limit  0..32768, else NDFL_E_ARG
 * A stream's DEFLATE bytes and end_bits are bit-identical to ndfl_deflate_chunks_lz77(ctx, NULL, 0,
 * hist_limit, data_i, len_i, chunk_len, ..., 1, 0, ...).  Chunk 0 has no history; a chunk that starts at
 * stream offset cs has the min(hist_limit, cs) bytes before it, the stream's own and never a neighbour's,
 * whatever lies next to it in `in`.  At position q the candidates are the distances min_dist ..
 * min(max_dist, q - (cs - min(hist_limit, cs))); a run is capped at max_run and at the chunk's end; the
 * longest run wins, the smallest distance among equal runs (D/comp/Lz77Huffman.java:68-90); a run below
 * min_run is a literal.
 * One wave encodes a stream, and keeps its hash-chain links and its chunk's tokens in device memory the
 * context owns: at most 384 KiB per wave, sized from the batch's longest in_len and chunk_len, grown on
 * first use, and never more than 256 MiB (the grid is lowered to fit).
 * Crossover to a loop of ndfl_deflate_chunks_lz77 calls (measured on one MI355X, FULL_DYNAMIC with a CRC-32,
 * DESIGN.md §4 "Batched LZ77 deflate"): the loop costs 0.42 to 0.63 ms per buffer up to 1 MiB, nearly all of it
 * per-call cost; the batch costs about 0.1 ms per call, a wave about 0.08 ms per stream plus 0.12 ms per KiB
 * while the stream is a few KiB, 0.6 ms per KiB (1.7 MB/s) once its window is full, and up to 1,792 waves run
 * at once.  65,536 x 512 B take 5.8 to 7.3 ms in a batch and 27 to 33 s in a loop, 4,096 x 4 KiB 1.8 to 3.4 ms
 * and 1.8 to 2.2 s; 256 x 1 MiB take 625 to 808 ms in a batch and 133 to 162 ms in a loop: the batch loses
 * there (buffers of that size go through ndfl_deflate_batch_chunked, below).  So one buffer alone is faster here
 * below about 2.5 KB, ten below about 8 KB each, a hundred below about 80 KB, 256 below about 220 KB; larger buffers, which ndfl_deflate_chunks_lz77 searches with whole workgroups
 * and the window in LDS, belong there whatever the count.  Against ndfl_deflate_batch's RLE_DYNAMIC the kernel
 * takes 2.5 to 7 times as long on these small buffers, and 4 KiB text buffers come out at 56 % of their size
 * instead of 99 %.
 */
int ndfl_deflate_batch_lz77(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                            const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                            int dynamic, int min_run, int max_run, int min_dist, int max_dist,
                            uint32_t chunk_len, uint32_t hist_limit, uint32_t flags);

/*
 * ndfl_deflate_batch with a per-chunk choice of block: stream i is DeflaterOutputStream(out, chunk_len,
 * hist_limit, MultiStrategy(strats...)): write all bytes, then finish() (D/comp/MultiStrategy.java:31-57,
 * D/comp/Uncompressed.java:19-51).  Per chunk, the substrategy with the fewest bits at the current output bit
 * position (mod 8) gives the block, the first such one on a tie; the stream starts at bit 0.  So a batch
 * whose buffers want different block types -- a stored block for 64 random bytes, a fixed-code block for
 * 512 bytes of text, a dynamic one for 4 KiB -- gets each of them, never pays for a dynamic header that does
 * not pay back, and no stream is longer than under any one of its substrategies alone.  Still one kernel launch
 * and one host sync whatever n and n_strats are (ndfl_deflate_chunks_multi costs one ndfl_deflate_chunks_lz77
 * call per substrategy, an assemble kernel and several host waits per buffer).  Items, results, formats,
 * `sum`, trailers, NDFL_E_CAPACITY with the required size, the rule that no byte of `out` outside
 * [out_off, out_off + min(out_len, out_cap)) is written, flags, stream ordering, ndfl_ctx_last_kernel_ms,
 * n == 0, overlapping or repeated input regions and the argument errors are ndfl_deflate_batch's, word for
 * word.
 *   strats      1..8 entries of NDFL_KIND_LZ77 (any tuple ndfl_deflate_chunks_lz77 accepts, the literal-only
 *               form (0, 0, 0, 0) and the RLE form (3, 258, 1, 1) among them) or NDFL_KIND_UNCOMPRESSED.
 *               n_strats == 0 or a null strats: NDFL_E_ARG; n_strats > 8: NDFL_E_UNSUPPORTED; another kind,
 *               or invalid Lz77Huffman parameters: NDFL_E_ARG (all as ndfl_deflate_chunks_multi).  One
 *               Lz77Huffman entry alone (or several equal ones) runs as ndfl_deflate_batch_lz77, one
 *               Uncompressed entry alone gives the stored-only stream.
 *   chunk_len   1..65536 (0: NDFL_E_ARG; above 65536: NDFL_E_UNSUPPORTED)
 *   hist_limit  0..32768, else NDFL_E_ARG
 * On any error nothing is written to `out` or `results`.
 * A stream's DEFLATE bytes and end_bits are bit-identical to ndfl_deflate_chunks_multi(ctx, NULL, 0,
 * hist_limit, data_i, len_i, chunk_len, strats, n_strats, 1, 0, ...).  A stored block is 3 header bits, zero
 * bits up to the byte, LEN, NLEN and at most 65,535 bytes, so a 65,536-byte chunk is two of them; BFINAL is
 * set on the stream's last block only; an empty buffer under Uncompressed alone is one empty stored block.
 * The search's window, run and distance rules are ndfl_deflate_batch_lz77's, per substrategy.
 * One wave encodes a stream.  It links a chunk's positions once, searches it once per distinct (min_run,
 * max_run, min_dist, max_dist) among the substrategies (a static and a dynamic one with the same tuple share
 * their tokens), sizes every candidate exactly from its histograms and codes, and keeps the best so far
 * (tokens, codes, header) while it tries the rest.  Device memory the context owns: a link ring that holds a
 * chunk and its window (at most 256 KiB) and two token lists (at most 256 KiB each) per wave, 768 KiB at
 * most, sized from the batch's longest in_len, chunk_len and hist_limit, grown on first use, and never more
 * than 256 MiB (the grid is lowered to fit: never below 341 waves).
 * Crossover to a loop of ndfl_deflate_chunks_multi calls (measured on one MI355X, MultiStrategy(Uncompressed,
 * FULL_STATIC, FULL_DYNAMIC) with a CRC-32, DESIGN.md §4 "Batched MultiStrategy deflate"): the loop costs 0.8 to
 * 1.2 ms per buffer up to 1 MiB, nearly all of it per-call cost; the batch costs about 0.1 ms per call, a wave
 * about 0.08 ms per stream plus 0.13 ms per KiB while the stream is a few KiB, 0.6 ms per KiB once its window is
 * full, and up to 1,792 waves run at once.  65,536 x 512 B take 6.0 to 7.5 ms in a batch and 53 to 65 s in a
 * loop, 4,096 x 4 KiB 1.9 to 3.5 ms and 3.7 to 4.3 s; 256 x 1 MiB take 619 to 824 ms in a batch and 268 to
 * 318 ms in a loop: the batch loses there (for one Lz77Huffman alone, buffers of that size go through
 * ndfl_deflate_batch_chunked, below).  So one buffer alone is faster here below about 6 KB (0.18 ms + 0.13 ms
 * per KiB against 1.0 ms), and with the full-window rate ten are below about 16 KB each, a hundred below about
 * 170 KB, 256 below about 430 KB (0.18 ms + 0.6 ms per KiB against n x 1.0 ms).  Against ndfl_deflate_batch_lz77's
 * FULL_DYNAMIC on the same buffers the kernel takes 5 to 11 % longer, and 512-byte text buffers come out at 92 %
 * of their size instead of 101 %.
 */
int ndfl_deflate_batch_multi(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                             const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                             const ndfl_strategy_desc* strats, uint32_t n_strats,
                             uint32_t chunk_len, uint32_t hist_limit, uint32_t flags);

/*
 * ndfl_deflate_batch with split blocks: stream i is DeflaterOutputStream(out, chunk_len, hist_limit,
 * BinarySplit(Lz77Huffman(sub's dynamic, min_run, max_run, min_dist, max_dist), min_block_len)): write all
 * bytes, then finish() (D/comp/BinarySplit.java:21-82).  A record with mixed content -- header then body,
 * digits then text, text then binary -- gets a block and a code of its own for each part where that is
 * shorter, and no stream is longer than under `sub` alone.  Still one kernel launch and one host sync whatever
 * n is (ndfl_deflate_chunks_binsplit costs one sub-frame per halving level, a host recursion and an assemble
 * kernel per buffer).  Items, results, formats, `sum`, trailers, NDFL_E_CAPACITY with the required size, the
 * rule that no byte of `out` outside [out_off, out_off + min(out_len, out_cap)) is written, flags, stream
 * ordering, ndfl_ctx_last_kernel_ms, n == 0, overlapping or repeated input regions and the chunk_len and
 * hist_limit checks are ndfl_deflate_batch's, word for word.
 *   sub, min_block_len
 *               checked in ndfl_deflate_chunks_binsplit's order: a null sub or min_block_len < 1 is NDFL_E_ARG
 *               (D/comp/BinarySplit.java:23-24); then chunk_len, hist_limit, the pointers and the items as
 *               ndfl_deflate_batch; then sub->kind other than NDFL_KIND_LZ77 is NDFL_E_UNSUPPORTED (Uncompressed
 *               and MultiStrategy size a block by the bit position it starts at, which no fixed tree answers);
 *               then an invalid Lz77Huffman tuple is NDFL_E_ARG.  The literal-only form (0, 0, 0, 0) and the
 *               RLE form (3, 258, 1, 1) are valid tuples.
 *   chunk_len   1..65536 (0: NDFL_E_ARG; above 65536: NDFL_E_UNSUPPORTED)
 *   hist_limit  0..32768, else NDFL_E_ARG
 * On any error nothing is written to `out` or `results`.
 * The decision rule.  Lz77Huffman's bit lengths do not depend on the bit position, so the reference's recursion
 * (D/comp/BinarySplit.java:36-69) is: a block [a, a + n) of a chunk has the halves f = (n + 1) / 2 and
 * s = n - f; it is split iff min(f, s) > min_block_len and bits(a, f) + bits(a + f, s) < bits(a, n), where
 * bits() is the size of the range as one Lz77Huffman block; each half is then treated the same way.  A
 * sub-block's window starts where its chunk's does (:44-46): at position q of a chunk that starts at stream
 * offset cs the candidates are the distances min_dist .. min(max_dist, q - (cs - min(hist_limit, cs))), and a
 * run is capped at the sub-block's end.  BFINAL is set on the stream's last block only; an empty buffer gives
 * the one empty final block.  dynamic == 0 runs the same rule: two fresh greedy parses can be shorter than one.
 * Unlike ndfl_deflate_chunks_binsplit the call has no restriction on odd lengths or on the number of nodes: any
 * in_len, any chunk_len in 1..65536 and any min_block_len >= 1 is encoded.  Where that call accepts the input
 * (ctx, NULL, 0, hist_limit, data_i, len_i, chunk_len, sub, min_block_len, 1, 0, ...) the DEFLATE bytes and
 * end_bits are bit-identical.
 * One wave encodes a stream.  It links a chunk's positions once and walks the split tree depth-first, the left
 * half first, with the waiting right halves on a stack in LDS (at most 15): every node is searched and sized
 * once, exactly, from its histograms and codes, and a leaf is emitted as soon as it is known to be one --
 * without another search when its tokens and codes are still the ones in place, as for a chunk too short to
 * split, which costs the one search of ndfl_deflate_batch_lz77.  Device memory the context owns: a link ring that
 * holds a chunk and its window (at most 256 KiB) and one token list (at most 256 KiB) per wave, sized from the
 * batch's longest in_len, chunk_len and hist_limit, grown on first use, and never more than 256 MiB (the grid is
 * lowered to fit: never below 512 waves).
 * Cost: a chunk is searched once per level of the tree that is tried, plus once more for the leaves that are
 * built again: up to log2(chunk_len / min_block_len) + 2 searches of the chunk's bytes.
 * Crossover to a loop of ndfl_deflate_chunks_binsplit calls (measured on one MI355X, BinarySplit(FULL_DYNAMIC, 256)
 * with a CRC-32, chunk_len = min(the buffer, 65536), DESIGN.md §4 "Batched BinarySplit deflate"; "mixed" buffers
 * are a quarter each of digits, text, random bytes and 16-valued bytes, which split, "text" ones never do): the
 * loop costs 0.56 ms per 512-byte buffer (no level to try), 1.9 to 2.1 ms per 4 KiB buffer (three levels), 4.8 to
 * 6.8 ms per 1 MiB buffer; the batch costs about 0.1 ms per call, a wave 0.15 ms per 512-byte stream, 1.6 (text)
 * to 2.6 ms (mixed) per 4 KiB stream, and 1.8 to 2.3 ms per KiB of a 1 MiB stream, seven levels tried with the
 * window full; up to 1,792 waves run at once.  65,536 x 512 B take 5.7 to 6.0 ms in a batch and 37 s in a loop
 * (2,048 of them measured: 1.15 to 1.17 s), 4,096 x 4 KiB 4.9 to 8.0 ms and 7.6 to 8.7 s; 256 x 1 MiB take 1.81
 * to 2.36 s in a batch and 1.22 to 1.74 s in a loop: the batch loses there, as the LZ77 and MultiStrategy batches
 * do (for an Lz77Huffman without the split, buffers of that size go through ndfl_deflate_batch_chunked, below).  So
 * one buffer alone is faster here below about 4 KB (at 4 KiB: 1.7 to 2.7 ms against 1.9 to 2.1 ms), and
 * with the full-window rate, which overstates the batch below some tens of KiB, ten are below about 10 KB each, a
 * hundred below about 115 KB, 256 below about 470 KB (0.1 ms + 2.3 ms per KiB against n x (2.1 ms + 0.0046 ms per
 * KiB)).  Against ndfl_deflate_batch_lz77's
 * FULL_DYNAMIC on the same buffers the kernel takes 4 % longer on 512-byte buffers, which are too short to split
 * (one search per stream), 2.9 (text) to 4.9 (mixed) times as long on 4 KiB buffers and 3.2 times on 1 MiB ones;
 * mixed 4 KiB buffers come out at 72.3 % of their size instead of 77.8 %, text ones gain nothing.
 */
int ndfl_deflate_batch_binsplit(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                                const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                                const ndfl_strategy_desc* sub, int32_t min_block_len,
                                uint32_t chunk_len, uint32_t hist_limit, uint32_t flags);

/*
 * ndfl_deflate_batch_lz77 for MEDIUM buffers, one to a few dozen chunks each (64 KiB pages, column chunks,
 * HTTP bodies, zip entries of 100 KiB to a few MiB): the chunks of all streams go through the chunk encoders of
 * ndfl_deflate_chunks / ndfl_deflate_chunks_lz77, one 1024-thread workgroup per chunk, and the number of kernel
 * launches and host waits does not depend on n (it grows with the staged bytes: one pair of LZ launches per
 * 256 MiB of them).  Stream i is DeflaterOutputStream(out, chunk_len, hist_limit, Lz77Huffman(dynamic, min_run,
 * max_run, min_dist, max_dist)): write all bytes, then finish().  Signature, items, results, formats, `sum`,
 * trailers, NDFL_E_CAPACITY with the required size and the first out_cap bytes stored, the rule that no byte of
 * `out` outside [out_off, out_off + min(out_len, out_cap)) of some stream is written (any alignment, regions
 * that touch), NDFL_IN_DEVICE / NDFL_OUT_DEVICE, stream ordering, ndfl_ctx_last_kernel_ms (here: every launch from
 * the first encoder pass to the finishing pass), n == 0, overlapping or repeated input regions and the argument errors
 * and their order are ndfl_deflate_batch_lz77's, word for word; on any error nothing is written to `out` or
 * `results`.
 *   dynamic, min_run, max_run, min_dist, max_dist
 *               every valid tuple is accepted.  The literal-only form (0, 0, 0, 0) and the RLE form
 *               (3, 258, 1, 1) run on the RLE / LITERAL chunk encoders, every other tuple on the LZ77 ones.
 *   chunk_len   1..65536 (0: NDFL_E_ARG; above 65536: NDFL_E_UNSUPPORTED)
 *   hist_limit  0..32768, else NDFL_E_ARG
 * More than 2^31 - 1 chunks in all (an empty buffer has one) is NDFL_E_UNSUPPORTED.
 * A stream's DEFLATE bytes and end_bits are bit-identical to ndfl_deflate_chunks_lz77(ctx, NULL, 0, hist_limit,
 * data_i, len_i, chunk_len, ..., 1, 0, ...).  Chunk 0 of a stream has no history; a chunk that starts at stream
 * offset cs sees the min(hist_limit, cs) bytes before it, its own stream's and never a neighbour's, whatever lies
 * next to it in `in` or in the staged copy; an empty buffer gives the one empty final block.  A stream's CRC-32 or
 * Adler-32 is combined on the device from per-chunk partials taken in one pass over all chunks; a batch that asks
 * for no checksum skips that pass.
 * Memory the context owns, grown on first use: the staged input gives every stream a slot of
 * max(1, ceil(in_len / chunk_len)) whole chunks, so it costs the SUM OF THE SLOTS, plus 4 bytes per staged byte
 * (of at most 256 MiB at a time) for the LZ77 matches, and the staged output costs the sum of
 * ndfl_deflate_bound(in_len, chunk_len) + 16 per stream.  A batch of many buffers far smaller than chunk_len
 * pays a whole slot for each: it belongs in ndfl_deflate_batch_lz77, or needs a smaller chunk_len.
 * NDFL_DEFLATE_FUSED and NDFL_LZ_SEARCH=chain have no effect on this call.
 * Crossover (measured on one MI355X, a CRC-32 per buffer, device buffers, chunk_len 65536, DESIGN.md §4
 * "Chunk-parallel batched deflate"; FULL_DYNAMIC on text .. mixed data, RLE_DYNAMIC on text .. runs):
 *   4,096 x 4 KiB    FULL_DYNAMIC 43.6 to 53.3 ms here, 1.69 to 1.79 ms in ndfl_deflate_batch_lz77, 2.2 to 2.4 s in
 *                    a loop of ndfl_deflate_chunks_lz77 calls; RLE_DYNAMIC 0.90 to 1.22 ms here, 0.50 to 0.56 ms
 *                    in ndfl_deflate_batch, 0.7 to 0.9 s in a loop of ndfl_deflate_chunks calls: the wave batch
 *                    wins (a 4 KiB buffer pays a 64 KiB slot here)
 *   4,096 x 64 KiB   FULL_DYNAMIC 38.4 to 66.0 ms here, 171 to 249 ms and 2.5 to 3.6 s; RLE_DYNAMIC 1.24 to 1.71 ms
 *                    here, 3.55 to 4.00 ms and 0.8 to 1.0 s: this call wins
 *   256 x 1 MiB      FULL_DYNAMIC 24.0 to 43.8 ms here, 613 to 755 ms and 156 to 257 ms; RLE_DYNAMIC 1.25 to 1.66 ms
 *                    here, 26.1 to 29.3 ms and 48.5 to 65.7 ms: this call wins
 * Downwards: this call's time follows the staged bytes, the slots (4,096 slots of 64 KiB cost what 256 buffers of
 * 1 MiB do, whatever the buffers hold), a wave batch's the longest streams; with chunk_len 65536 and a few thousand
 * buffers the wave batch is faster below about 15 to 20 KB per buffer (both searches; interpolated linearly between
 * the 4 KiB and the 64 KiB shape).  Upwards: no buffer count or size was found at which one
 * ndfl_deflate_chunks_lz77 call per buffer is faster.  At 1 MiB a buffer costs 0.09 ms here against 0.6 to 1.0 ms
 * in the loop, nearly all of it per-call cost; the rate here, 11 GB/s of text, is what ndfl_deflate_chunks_lz77
 * reaches inside one large stream (1 GiB in about 108 ms), so larger buffers do not turn it round.  What bounds
 * this call is the memory above; one buffer of many chunks alone goes through ndfl_deflate_chunks_lz77, which
 * needs no slots and no second copy of the output.
 */
int ndfl_deflate_batch_chunked(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
                               const ndfl_member_item* items, ndfl_deflate_result* results, uint32_t n,
                               int dynamic, int min_run, int max_run, int min_dist, int max_dist,
                               uint32_t chunk_len, uint32_t hist_limit, uint32_t flags);

/*
 * Compress a buffer to a blocked gzip file (BGZF: bgzip, BAM, tabix) in one call: the counterpart of
 * ndfl_inflate_bgzf.  The input is cut into blocks of block_len bytes, every block becomes one gzip member with
 * its own length in a `BC` subfield (BSIZE), the members lie back to back from out[0], and the 28-byte empty
 * member closes the file.  The blocks run through ndfl_deflate_batch_chunked's encoders, one workgroup per
 * block; three passes of this call's own then size the members, scan their lengths and pack them, all on the
 * device.  The number of launches does not depend on the number of members (but for the LZ77 encoders' loop
 * over slabs of staged data, as in ndfl_deflate_batch_chunked); with NDFL_OUT_DEVICE the host syncs once, else
 * twice (the sizes, then the file's bytes).
 *
 * Blocks: member k holds in[k * block_len, min((k + 1) * block_len, in_len)).  block_len is 1..65536 (0:
 *   NDFL_E_ARG; above: NDFL_E_UNSUPPORTED); the tuple is checked first, as ndfl_deflate_batch_chunked checks
 *   it (an invalid one: NDFL_E_ARG).  Empty input gives the closing member alone.  in_len above 8 GiB, or more
 *   than 2^31 - 2 blocks, is NDFL_E_UNSUPPORTED, before anything is allocated.
 * Member: exactly what GzipOutputStream (D/GzipOutputStream.java) writes for that block alone with
 *   GzipMetadata(operatingSystem = UNKNOWN, extraField = 'B' 'C' 02 00 <BSIZE>) and MultiStrategy(
 *   Lz77Huffman(dynamic, min_run, max_run, min_dist, max_dist), Uncompressed.SINGLETON): the 18 header bytes
 *   1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 42 43 02 00 | BSIZE = the member's length - 1; the DEFLATE
 *   data; CRC-32 and ISIZE.  The DEFLATE data is one chunk that starts at bit 0, where MultiStrategy
 *   (D/comp/MultiStrategy.java:19-57: the first substrategy with the fewest bits) reduces to one rule: the
 *   stored form (D/comp/Uncompressed.java:19-47: 8 * len + 40 * nblk bits at bit 0, nblk = max(1, ceil(len /
 *   65535))) is taken if and only if it has FEWER bits than the tuple's single final block, whose bytes and
 *   bit count are ndfl_deflate_batch_chunked's for that block; a tie goes to the tuple.
 * Size: a member's length must fit BSIZE.  With block_len <= 65505 none can exceed 65,536 bytes (26 + 65505 +
 *   5 stored); above that an incompressible block can, and the call then returns NDFL_E_UNSUPPORTED with
 *   bad_member = the lowest such index; nothing of `out` is specified.
 * Layout: member k starts where member k - 1 ends (a 64-bit exclusive scan on the device).  table (host
 *   memory, may be NULL with table_cap = 0) receives min(table_cap, n_members + 1) entries (file offset, data
 *   offset), the last one (out_len, in_len): exactly what ndfl_inflate_bgzf reports for the file written.
 * Capacity: a file longer than out_cap returns NDFL_E_CAPACITY with out_len = its length, and no byte of `out`
 *   is written (the pack pass reads the total on the device), so out = NULL, out_cap = 0 sizes the file.  In
 *   every case no byte at or past out + out_len is written, at any byte alignment of `out`: whole aligned
 *   words are stored as words, a member's first and last bytes that share a word with a neighbour as bytes.
 * ndfl_bgzf_bound (host only, no context): every member in its stored form, 26 + len + 5 * nblk, plus 28; 0
 *   for a block_len outside 1..65536.  An upper bound of every file the call can write, exact when every
 *   member is stored.
 * Returns result->status, or NDFL_E_ARG (null ctx / result, null buffers with a size, block_len 0, an invalid
 * tuple), NDFL_E_UNSUPPORTED (block_len or in_len past the limits; *result is then all zero), NDFL_E_DEVICE.
 * NDFL_IN_DEVICE, NDFL_OUT_DEVICE and stream ordering as for the other batch calls; ndfl_ctx_last_kernel_ms
 * covers every launch from the tables to the pack.  Memory the context owns: the staged input (in_len), 4
 * bytes per staged byte (of at most 256 MiB at a time) for LZ77 matches, and per block the staged output's
 * ndfl_deflate_bound(block_len, block_len) + 16 and about 110 bytes of tables; a block_len of a few bytes pays
 * some 1,200 bytes a member.
 * Crossover (measured on one MI355X, blocks of 65,280 bytes, FULL_DYNAMIC against stored, DESIGN.md §4 "BGZF
 * writer"; against the composition this call replaces, as of commit 6ff466b: the blocks through the wave batch
 * ndfl_deflate_batch_multi, BSIZE patched and the members joined on the host, host bytes to host bytes):
 *   16 MiB, 257 members     1.8 ms (text, runs) to 3.0 ms (mixed data) device to device, 3.9 to 5.4 ms host to host;
 *                           the composition 50 to 91 ms
 *   256 MiB, 4,097 members  24 to 43 ms device to device, 366 to 420 ms host to host (host copies, not kernels);
 *                           the composition 1.43 to 1.55 s
 * No shape was measured at which the composition is faster; the smallest input measured is 16 MiB.
 */
typedef struct {
    int32_t  status;      /* 0, NDFL_E_CAPACITY, or NDFL_E_UNSUPPORTED (a member longer than 65,536 bytes) */
    uint32_t n_members;   /* members of the file written, the closing empty member included */
    uint32_t bad_member;  /* lowest index of a member longer than 65,536 bytes, else n_members */
    uint32_t n_stored;    /* members written as stored blocks */
    uint64_t out_len;     /* the file's length; with NDFL_E_CAPACITY: the bytes required */
} ndfl_bgzf_write_result;
int ndfl_deflate_bgzf(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                      ndfl_bgzf_write_result* result, ndfl_bgzf_member* table, uint32_t table_cap,
                      int dynamic, int min_run, int max_run, int min_dist, int max_dist,
                      uint32_t block_len, uint32_t flags);
uint64_t ndfl_bgzf_bound(uint64_t in_len, uint32_t block_len);

/*
 * Decompress the block-aligned bit range [start_bit, end_bit) of one raw DEFLATE stream: one GPU's
 * shard of a stream decoded across GPUs, or one batch of a stream read incrementally
 * (NDFL_IN_PARTIAL, end_bit UINT64_MAX: InflaterInputStream's bounded input buffer,
 * D/InflaterInputStream.java:96-106).  For the multi-GPU case: one GPU's
 * shard of a stream decoded across GPUs.  Same decoder as ndfl_inflate, i.e.
 * Open.read (D/decomp/Open.java:83-124), started at a block boundary with the reference's
 * dictionary state (the 32 KiB ring, :592-603) given by the caller instead of built up.
 *   out         window start: out[0, dict_len) holds the dict_len (<= 32768) output bytes preceding
 *               the range; decoded bytes are written to out[dict_len, dict_len + *out_len)
 *   end_bit     stop at the block boundary == end_bit (UINT64_MAX: run to the final block);
 *               NDFL_E_ARG if a block straddles it
 *   flags       NDFL_DICT_DEFERRED (requires NDFL_OUT_DEVICE): the window is not written yet.  The
 *               call decodes everything, records which chains of blocks read the window (directly
 *               or through other chains), and ndfl_inflate_resolve re-emits exactly those after the
 *               caller has written it; so all GPUs decode in parallel and only the window (32 KiB)
 *               is passed along.  `in` and `out` must stay valid until the resolve call.
 * Returns as ndfl_inflate (COPY_FROM_BEFORE_DICTIONARY_START counts the window as dictionary).
 */
int ndfl_inflate_range(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint64_t start_bit, uint64_t end_bit,
                       uint8_t* out, uint64_t dict_len, uint64_t out_cap, uint64_t* out_len,
                       uint64_t* consumed_bits, uint32_t flags);
/*
 * Multi-GPU decode of a stream WITHOUT a seam index (SURVEY §8e decompress): a block boundary
 * at or past from_bit that the decoder has confirmed -- the end of a chain of blocks, decoded from
 * a header candidate (the reference's own header checks, D/decomp/Open.java:322-435), that lands
 * exactly on another candidate whose own chain links on (or is final) -- looking at most
 * window_bits ahead;
 * *sync_bit = UINT64_MAX if there is none.  GPU r of N takes [sync(r*C/N), sync((r+1)*C/N)) and
 * decodes it with ndfl_inflate_range (deferred window); ndfl_inflate_range's exact-boundary
 * check (NDFL_E_ARG when a block straddles end_bit) proves each seam, starting from bit 0.
 * flags: NDFL_IN_DEVICE / NDFL_IN_PADDED as for ndfl_inflate.
 */
int ndfl_inflate_sync(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint64_t from_bit, uint64_t window_bits,
                      uint64_t* sync_bit, uint32_t flags);
/*
 * Diagnostics (no reference counterpart; used by the parity tests): the decoder's chain starts in
 * the raw DEFLATE stream `in` -- the bit positions at which the header finder and the strict stage
 * accept a block header, by the reference's own header checks (UncompressedBlock ctor
 * D/decomp/Open.java:232-241, HuffmanBlock(true) :336-431) restricted to headers a chain may start
 * at (BFINAL = 0; stored with zero padding, its LEN bytes in the input and a plausible next
 * header; dynamic with HLIT, HDIST < 30).  headers[0, min(cap, *n_headers)) = the positions in
 * ascending order, at most 256 per 64 KiB of input (the decoder's per-segment cap); survivors
 * (optional) = the finder's survivors before the strict stage (bit 63 set: dynamic); stats
 * (optional, 4 entries) = survivors found, headers accepted before the cap, segments over the cap,
 * survivors dropped past the survivor list's capacity.  flags: NDFL_IN_DEVICE / NDFL_IN_PADDED.
 */
int ndfl_inflate_headers(ndfl_ctx* ctx, const uint8_t* in, uint64_t in_len, uint32_t flags, uint64_t* headers,
                         uint64_t cap, uint64_t* n_headers, uint64_t* survivors, uint64_t surv_cap, uint64_t* stats);
/* Finish the last NDFL_DICT_DEFERRED range decode on this context (NDFL_E_STATE if none). */
int ndfl_inflate_resolve(ndfl_ctx* ctx, uint64_t* n_reemitted);
/*
 * Multi-GPU window chain: once the caller has written the window of the last
 * NDFL_DICT_DEFERRED range decode, dst[0, tail_len) (device memory) = the final values of the last
 * tail_len bytes of out[0, dict_len + out_len), without resolving the rest -- the next GPU's window,
 * passed on before this GPU's own resolve (ndfl_inflate_resolve still finishes the decode).  In the
 * reference this is the 32 KiB dictionary that Open carries from one block to the next
 * (D/decomp/Open.java:592-603).  NDFL_E_STATE if no deferred decode is pending, NDFL_E_UNSUPPORTED if
 * a byte's back-reference chain is too long to follow (resolve first, then take the bytes from out).
 */
int ndfl_inflate_tail(ndfl_ctx* ctx, uint64_t tail_len, uint8_t* dst);
/*
 * The window chain in one step: the same last tail_len bytes of the pending
 * NDFL_DICT_DEFERRED decode as a map of its window, before the window is written: dst[k] (device
 * memory, u32) = the window byte index (< dict_len) byte k's value comes from, or
 * NDFL_TAIL_LITERAL | value for a byte that does not depend on the window.  Every GPU computes its
 * map at once; an all-gather of the maps lets GPU r compose those of GPUs 0..r-1 into its window
 * (Open's 32 KiB dictionary, D/decomp/Open.java:592-603, carried across all earlier shards)
 * without waiting for GPU r-1.  Errors as ndfl_inflate_tail.
 */
#define NDFL_TAIL_LITERAL 0x80000000u
int ndfl_inflate_tail_map(ndfl_ctx* ctx, uint64_t tail_len, uint32_t* dst);

/*
 * Multi-GPU seam step for compression: place the first `nbits` bits of `in` at bit
 * `shift` (0..7) of out[0] (lower bits 0, bits past the end 0).  A shard compressed at bit 0 by
 * ndfl_deflate_chunks is thereby moved to its global bit offset mod 8; the byte shared with the
 * previous shard is ORed when the stream is assembled -- BitOut's byte packing
 * (D/DeflaterOutputStream.java:147-156) across GPUs.  Device pointers only (NDFL_IN_DEVICE |
 * NDFL_OUT_DEVICE), not in place.
 */
int ndfl_bits_shift(ndfl_ctx* ctx, const uint8_t* in, uint64_t nbits, uint32_t shift, uint8_t* out,
                    uint64_t out_cap, uint32_t flags);

/* java.util.zip.CRC32.update over a buffer, on the GPU (flags: NDFL_IN_DEVICE). */
int ndfl_crc32(ndfl_ctx* ctx, uint32_t* crc_inout, const uint8_t* data, uint64_t len, uint32_t flags);
/* java.util.zip.Adler32.update over a buffer, on the GPU (flags: NDFL_IN_DEVICE): the zlib
 * container's checksum (D/ZlibOutputStream.java:22,48, D/ZlibInputStream.java:25,57-69).
 * *adler_inout = (b << 16) | a, 1 for a fresh checksum. */
int ndfl_adler32(ndfl_ctx* ctx, uint32_t* adler_inout, const uint8_t* data, uint64_t len, uint32_t flags);
/* crc of A||B from crc(A), crc(B), |B| (host arithmetic). */
uint32_t ndfl_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

#ifdef __cplusplus
}
#endif
#endif
