/*
 * dint_hip.h — C ABI of the MI355X (gfx950) DINT decode path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types. Each entry point names the reference interface (jermp/dint) it
 * replaces; the C++ adaptors that give these calls the reference's static
 * `Coder::decode(dict, in, out, sum, n) -> in_end` shape live in
 * dint_amd/csrc/host/dint/coders.hpp, and INTEGRATION.md shows the
 * reference-side binding.
 *
 * Threading: a dint_dict is immutable after creation and may be used from
 * several host threads with distinct streams (its launch bookkeeping — queue
 * slots, timing events — sits behind the handle's own `launch_mutex`). One
 * dint_dict lives on one device; multi-GPU = one dint_dict per device (the
 * dictionary is replicated, posting lists are partitioned, there is no
 * data-path collective). A dint_query_index may be called from several host
 * threads, each with its own stream: its calls SERIALISE on the handle's own
 * lock (`dint_query_index::mutex`, taken inside dint_and_queries /
 * dint_and_queries_freqs for the whole call — the handle's workspaces are one
 * set); two query indexes, or two dint_block_tables over one index and one
 * pair of dictionaries, share nothing mutable and run side by side. A
 * dint_block_table (and a dint_unit_table) belongs to one caller at a time:
 * its decodes are ordered on the stream they are enqueued on
 * (tests/test_gpu_queries.py::test_one_query_index_under_two_host_threads,
 * tests/test_gpu_index.py::test_two_block_tables_over_one_index_on_two_threads).
 *
 * All functions return DINT_OK (0) or a negative dint_status; none throws.
 */
#ifndef DINT_HIP_H
#define DINT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINT_ABI_VERSION 6

/* A unit decodes to at most this many integers (the kernels address a unit's output with 32-bit byte
 * offsets); dint_index_stream never cuts larger ones, dint_decode_units skips them. */
#define DINT_MAX_UNIT_INTS (1u << 28)

typedef enum dint_status {
    DINT_OK = 0,
    DINT_ERR_ARG = -1,       /* null pointer, bad enum, capacity too small          */
    DINT_ERR_FORMAT = -2,    /* dictionary file or encoded stream is malformed      */
    DINT_ERR_HIP = -3,       /* a HIP runtime call failed (see dint_last_hip_error) */
    DINT_ERR_NO_DEVICE = -4, /* no gfx950 device / device index out of range        */
    DINT_ERR_NOMEM = -5
} dint_status;

/* Dictionary flavours of the decode path (reference include/dint/dictionary_types.hpp:8-21). */
typedef enum dint_dict_kind {
    DINT_DICT_RECTANGULAR = 0,   /* single_rect_dint   */
    DINT_DICT_SINGLE_PACKED = 1, /* single_packed_dint */
    DINT_DICT_MULTI_PACKED = 2   /* multi_packed_dint  */
} dint_dict_kind;

/* Opaque device-resident dictionary.
 * Replaces: Dictionary::builder::load + builder.build(dict)
 *           (vroom_env/decode.cpp:116-123; single_dictionary.hpp:88-107,177-181;
 *            rectangular_dictionary.hpp:79-92; multi_dictionary.hpp:93-121). */
typedef struct dint_dict dint_dict;

/* One unit of decode work: a run of codewords that starts on a codeword
 * boundary and decodes to exactly `n` integers. The vroom stream has no sync
 * points (lists are `vbyte(n) vbyte(universe) payload` back to back,
 * vroom_env/jobs.hpp:89-91), so this table is the sidecar that makes the
 * stream parallel; it is produced by dint_index_stream() or by the encoder. */
typedef struct dint_unit {
    uint64_t in_off;  /* byte offset of the unit's first codeword in the encoded buffer */
    uint64_t out_off; /* index of the unit's first integer in the output buffer         */
    uint32_t n;       /* integers this unit decodes to (> 0)                             */
    uint32_t list;    /* ordinal of the posting list the unit belongs to                 */
} dint_unit;

typedef struct dint_dict_info {
    int32_t kind;           /* dint_dict_kind                                  */
    int32_t device;         /* HIP device ordinal                              */
    uint32_t num_dicts;     /* 1, or 6 for multi                               */
    uint32_t entries;       /* m_size of the file                              */
    uint32_t hot_entries;   /* codewords whose payload is staged in LDS        */
    uint32_t lds_bytes;     /* LDS image size in bytes                         */
    uint32_t table_words;   /* device table size in u32                        */
    uint32_t compute_units; /* CUs of the device the kernels are sized for     */
} dint_dict_info;

int dint_abi_version(void);

/* Process-wide switches for tests and measurements (the library reads no environment variable). Defaults are what a
 * caller wants; every entry point reads them with one relaxed atomic load, so a change takes effect from the next call
 * on and is safe against concurrent calls. dint_set_option refuses values outside an option's range (DINT_ERR_ARG). */
typedef enum dint_option {
    DINT_OPT_BUNDLES = 0,             /* 1 (default): tiny units share tiles (bundle schedule); 0: every unit on its own           */
    DINT_OPT_INDEX_CONCURRENT = 1,    /* 1 (default): dint_decode_block_table runs its launches side by side; 0: one stream      */
    DINT_OPT_QUERY_LEAN_PAGES = 2,    /* page decodes of at least this many pages take the three-launch form; -1 (default): none */
    DINT_OPT_QUERY_TAIL_PAGES = 3,    /* calls of at most this many candidate pages run a round per launch; default 4            */
    DINT_OPT_QUERY_FUSED_PAGES = 4,   /* ... of at most this many run as ONE launch; default 2, 0: never                         */
    DINT_OPT_INDEX_INLINE_TAILS = 5,  /* 1 (default): a created block table's short blocks are decoded inside its docs launch;   */
                                      /* 0: by a launch of their own                                                             */
    DINT_OPT_CHUNK_SPLIT = 6,         /* the bundle path hands out 1/2^n of a 64-unit chunk per ticket, n = 0..4; -1 (default):  */
                                      /* by the launch's size                                                                   */
    DINT_OPT_INDEX_PAIR = 7,          /* 1 (default): once a table's schedules are known, docs parts, short blocks and freqs     */
                                      /* parts of a decode are ONE launch; 0: a launch each                                      */
    DINT_OPT_QUERY_FUSED_COPY = 8,    /* 1 (default): the one-launch query form's workgroup fetches the call's inputs from the   */
                                      /* host's pinned memory itself; 0: a copy on the stream in front of the launch            */
    DINT_OPT_QUERY_BATCH_FUSED = 9,   /* 1 (default): a call whose queries all have few candidate pages runs as ONE launch, a      */
                                      /* workgroup per query; 0: the round-per-launch batch form                                */
    DINT_OPT_SPLIT_UNITS = 10,        /* 1 (default): a prepared multi-dictionary unit table cuts the units that fit no tile in two */
                                      /* records each (a second launch of the bundles kernel); 0: the general kernel decodes them */
    DINT_OPT_REFINE_UNITS = 11,       /* 1 (default): a prepared multi-dictionary unit table whose units hold several 256-integer  */
                                      /* blocks (at most 131072 integers each) finds the blocks once and decodes a table of      */
                                      /* blocks; 0: the units as they came (a wavefront decodes a unit's blocks one after another) */
    DINT_OPT_COUNT_ = 12,
    /* Workspace bounds, numbered apart from the switches above (dint_option_name enumerates those from 0 up to the first
     * NULL; a bound's name is asked for by its number): */
    DINT_OPT_QUERY_OR_PASS_PAGES = 32 /* an OR call decodes at most this many pages (256 docIDs each) at a time, whole queries */
                                      /* per pass; a larger query runs alone. Default 1048576 (1 GiB of docIDs), 1 .. 2^32-1 */
} dint_option;
int dint_set_option(int option, long long value);
int dint_get_option(int option, long long* value);
const char* dint_option_name(int option); /* "bundles", "index_concurrent", ... ; NULL past the last */
int dint_reset_options(void);             /* every option back to its default */

const char* dint_strerror(int status);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char* dint_last_hip_error(void);
int dint_device_count(int* count);

/* Parse a dictionary file image (the bytes the reference's builder::write
 * produced) and stage it on `device`. */
int dint_dict_create(int kind, const void* file_bytes, size_t len, int device, dint_dict** out);
void dint_dict_destroy(dint_dict* dict);
int dint_dict_info_get(const dint_dict* dict, dint_dict_info* info);

/* Untimed host pre-pass over a whole vroom stream in host memory: reads every
 * list header, walks the codewords WITHOUT copying dictionary payloads, and
 * cuts each list into units of about `unit_ints` integers at codeword
 * boundaries (multi: at 256-integer block boundaries).
 * unit_ints = 0: one unit per list (a list of more than DINT_MAX_UNIT_INTS integers is still cut).
 * Replaces: the per-list framing loop of vroom_env/decode.cpp:139-150.
 * `*units` is malloc'ed; release with dint_free. */
int dint_index_stream(const dint_dict* dict, const uint8_t* enc, size_t enc_bytes,
                      uint32_t unit_ints, dint_unit** units, size_t* n_units,
                      uint64_t* total_ints, uint64_t* n_lists);
void dint_free(void* p);

/* Decode `n_units` units. All pointers except `dict` are DEVICE pointers on the
 * dictionary's device; `stream` is a hipStream_t (NULL = default stream). The
 * call is asynchronous. Exactly unit.n integers are written at
 * d_out[unit.out_off ...]; nothing else is touched (no pre-zeroed output, no
 * overflow area — unlike the reference, dint_codecs.hpp:11). If d_end_off is
 * not NULL, d_end_off[u] receives the byte offset one past unit u's last
 * consumed byte (the reference's returned `in` pointer).
 * Units may come in any order and any subset: a permutation or a subset of
 * dint_index_stream's table, units repeated (one in_off in several entries),
 * outputs anywhere in d_out (holes between them are left as they were; the
 * outputs of two entries must not overlap). A unit's stream bytes are bounded
 * by where the NEXT table entry starts when that lies above the unit's own
 * start, so no unit may begin strictly inside an earlier table entry's bytes
 * (a whole list followed by its own later pieces): such a table returns
 * DINT_OK and writes every unit only inside its own [out_off, out_off + n),
 * but the unit it cuts into may decode wrong, its end offset too. Tables of
 * dint_index_stream, and every subset or permutation of them, satisfy this.
 * Runs of table-consecutive tiny units (<= 256 integers, <= 256 stream bytes
 * up to the next unit's start, consecutive outputs — the long tail of short
 * posting lists) are decoded several to a wavefront tile, which changes the
 * speed, never the result.
 * Replaces: single_dint::decode / multi_opt_dint::decode
 *           (vroom_env/dint_codecs.hpp:37-107, :521-619). */
int dint_decode_units(const dint_dict* dict, const uint8_t* d_enc, size_t enc_bytes,
                      const dint_unit* d_units, size_t n_units, uint32_t* d_out,
                      size_t out_capacity, uint64_t* d_end_off, void* stream);

/* A unit table prepared for decoding. What depends on the unit table and the stream alone — which tiny units
 * share a wavefront tile, the work items of the unit queue, the selector bytes of a multi-dictionary stream's
 * blocks (the "bundle schedule": three small kernels and a read of 22 bytes per unit that dint_decode_units
 * runs before EVERY launch) — is computed once, here, like the sidecar itself (it is a property of the encoded
 * collection, not of a decode). The handle borrows `dict`, `d_enc` and `d_units`: they must outlive it and keep
 * their contents. `out_capacity` is the smallest output capacity later decodes may pass (the schedule's bounds
 * checks are made against it). The table may be shaped as dint_decode_units allows — any order, subsets, repeats, outputs
 * with holes — under the same rule: no unit begins strictly inside an earlier entry's bytes. Synchronises `stream`.
 * A multi-dictionary table whose units hold SEVERAL 256-integer blocks (at most 131072 integers each) is refined here: blocks
 * carry no length, so a unit of several is one wavefront's sequential work (242 G ints/s on the bench stream), where a table of
 * blocks packs three blocks into a tile (472-526 G). A lane per unit walks the unit's codewords once and the handle keeps a
 * unit record per block (24 bytes per 256 integers, + 22 bytes of schedule); decodes then run over the blocks, and d_end_off
 * still has one entry per unit of the CALLER's table. DINT_OPT_REFINE_UNITS = 0: the units as they came. Results are identical
 * either way. (Decodes of ONE table are ordered on one stream: its counters and, refined, its per-block end offsets are the
 * table's own.)
 * Replaces: nothing in the reference (its decode loop is sequential); it is the set-up half of
 * dint_decode_units, i.e. of vroom_env/decode.cpp:139-150. */
typedef struct dint_unit_table dint_unit_table;
int dint_unit_table_create(const dint_dict* dict, const uint8_t* d_enc, size_t enc_bytes, const dint_unit* d_units,
                           size_t n_units, size_t out_capacity, void* stream, dint_unit_table** out);
void dint_unit_table_destroy(dint_unit_table* table);
/* dint_decode_units over a prepared table: one kernel launch, asynchronous. out_capacity must be at least the
 * table's (DINT_ERR_ARG otherwise). Results are identical to dint_decode_units'. */
int dint_decode_unit_table(const dint_dict* dict, dint_unit_table* table, uint32_t* d_out, size_t out_capacity,
                           uint64_t* d_end_off, void* stream);
/* Where to put the output. The decode kernels run 10-17 % faster or slower depending on where the driver put the
 * stream they read relative to the output they write — a property of the PAIR of buffers, stable while both live,
 * which nothing but the decode kernel itself can see. A caller whose
 * output buffer lives for many decodes allocates a few candidates and lets this rank them: the table is decoded into
 * every candidate three times, kernel_ms[i] = the faster of the last two launches' kernel times, *fastest = the index
 * of the smallest. Synchronises `stream`; every candidate holds the decoded integers afterwards.
 * Replaces: nothing in the reference. */
int dint_unit_table_rank_outputs(const dint_dict* dict, dint_unit_table* table, uint32_t* const* d_outs, size_t n_outs,
                                 size_t out_capacity, void* stream, float* kernel_ms, size_t* fastest);
/* The same question for the price of a SAMPLE (round 6): which (stream copy, output buffer) pair do the decode kernels run
 * fastest on? Every candidate pair — n_encs copies of ONE encoded stream at different addresses, n_outs output buffers —
 * decodes the same evenly spread sample of the unit table (runs of 4 units, about `sample_ints` integers in all, 0: the
 * smallest launch that fills the device; the units keep their own places in stream and output, so the sample touches all of
 * both buffers) four times; kernel_ms[i * n_outs + j] = the fastest of the last three launches' kernel times on copy i and
 * output j. The slow / fast level of a pair is a property of where the driver put the two buffers and
 * shows in a sample as it does in the full decode (profiles/r06_placement_probe.txt); the stream is the small buffer of the
 * two (an eighth of the output), so a caller tries a few COPIES of it — allocated at different points of its set-up — against
 * the one output buffer it has: INTEGRATION.md section 6. Synchronises `stream`; the outputs hold the sample's integers.
 * Replaces: nothing in the reference. */
int dint_probe_placement(const dint_dict* dict, const uint8_t* const* d_encs, size_t n_encs, size_t enc_bytes,
                         const dint_unit* d_units, size_t n_units, uint32_t* const* d_outs, size_t n_outs, size_t out_capacity,
                         uint64_t sample_ints, void* stream, float* kernel_ms);

/* Host-pointer convenience with the reference's call shape: decode ONE
 * sequence of n integers starting at in[0]; *consumed = bytes read. Uploads,
 * runs one unit on the device, downloads, synchronises. n <= DINT_MAX_UNIT_INTS
 * (DINT_ERR_ARG beyond: index the stream and batch); a single wavefront wide:
 * batch through dint_decode_units for throughput.
 * Replaces: Coder::decode(dict, in, out, universe, n) at vroom_env/decode.cpp:143. */
int dint_decode_list_host(const dint_dict* dict, const uint8_t* in, size_t in_bytes,
                          uint32_t* out, size_t n, size_t* consumed);

/* ---- in-index path: posting lists in the dict_posting_list layout --------------------------- */

/* Host-pointer call with the reference's in-index BLOCK Coder shape: decode ONE block of n <= 256
 * integers starting at in[0]; *consumed = bytes read. n == 256: a DINT block — 16-bit codewords
 * (single dictionaries), or a selector byte and 16- / 8-bit codewords (multi) — through the DINT
 * kernels; n < 256: binary interpolative, `sum_of_values` being the sum of the block's integers or
 * 0xFFFFFFFF for "a vbyte of it comes first" (what the reference passes for freqs blocks), through
 * the interpolative kernel. Uploads, runs one block on the device, downloads, waits for the
 * dictionary's own stream (pinned staging and a device workspace kept by the dictionary: no
 * allocation after the first call of a size, no device-wide synchronisation): the reference's
 * granularity, one block per call — dint_list_cache_* decodes a list's blocks at once,
 * dint_decode_posting_blocks many lists'. Nothing past out[n - 1] is written and `out` need not be zeroed (the reference needs
 * both: block_size + overflow zeroed words, dict_posting_list.hpp:104-105, :296).
 * Pinned by tests/test_gpu_short_blocks.py for every n = 1 .. 255: a docs part without bits (n = 1: out[0] = sum_of_values;
 * a sum of zero: n zeros) reads nothing and *consumed = 0; the freqs part of n = 1 is its vbyte alone; sums up to
 * 0xFFFFFFFE on either side (a 5-byte vbyte); `in + in_bytes` may be the block's last byte.
 * Replaces: dint_block::decode / opt_dint_single_dict_block::decode /
 *           opt_dint_multi_dict_block::decode (include/dint/dint_codecs.hpp:13-49, :269-274,
 *           :460-510) and interpolative_block::decode (include/ds2i/block_codecs.hpp:130-150), as
 *           called from dict_posting_list.hpp:298-301 and :313-315. */
int dint_decode_block_host(const dint_dict* dict, const uint8_t* in, size_t in_bytes, uint32_t* out,
                           uint32_t sum_of_values, size_t n, size_t* consumed);

/* A whole posting list (host pointer, the dict_posting_list layout below) decoded ONCE, its blocks then served from host
 * memory: what makes the block Coder usable under a document_enumerator, which calls Coder::decode per touched block
 * (dict_posting_list.hpp:298-301, :313-315) — one launch sequence per 256 postings otherwise. `create` uploads the
 * list, decodes every block's docs part (as the Coder returns it: d-gaps) and — freqs_dict not NULL — freqs part (as
 * stored: freq - 1) through the batched kernels on the dictionary's own stream, and downloads; it synchronises that
 * stream only. `decode` = the Coder call for the block part that starts `in_offset` bytes into the list: a memcpy;
 * *consumed = the part's bytes. DINT_ERR_ARG if no part of n integers starts there.
 * A docs part without bits — a block of one posting, or of consecutive docIDs (a sum of zero) — has NO bytes: *consumed = 0,
 * and the freqs part of that block starts at the same offset. dint_list_cache_decode, which has the offset alone, answers
 * with the docs part there; dint_list_cache_decode_part takes the Coder call's sum_of_values as well (0xFFFFFFFF: the freqs
 * part, anything else: the docs part) and serves the part asked for, DINT_ERR_ARG if that part does not start at in_offset.
 * A cache made without a freqs dictionary refuses every freqs part (DINT_ERR_ARG: the caller decodes that block itself).
 * Pinned by tests/test_gpu_short_blocks.py over lists of one posting, of consecutive docIDs, with tails of 1, 128 and 255
 * postings behind full blocks and without a tail.
 * Replaces: dint_block::decode / interpolative_block::decode as called from dict_posting_list.hpp:298-301, :313-315,
 *           for a list at a time. */
typedef struct dint_list_cache dint_list_cache;
int dint_list_cache_create(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* list, size_t list_bytes,
                           dint_list_cache** out);
int dint_list_cache_decode(const dint_list_cache* cache, size_t in_offset, uint32_t* out, size_t n, size_t* consumed);
int dint_list_cache_decode_part(const dint_list_cache* cache, size_t in_offset, uint32_t sum_of_values, uint32_t* out, size_t n,
                                size_t* consumed);
void dint_list_cache_destroy(dint_list_cache* cache);

/* One 256-posting block (the last block of a list may be shorter) of a posting list laid out as
 * reference include/dint/dict_posting_list.hpp:10-56:
 *   vbyte(n) | u32 block_max[B] | u32 block_endpoint[B-1] | { docs part, freqs part } x B
 * The block-max / endpoint arrays already make every block independently addressable, so no
 * sidecar is needed here: this table is just those arrays flattened over many lists.
 * dint_decode_posting_blocks and dint_block_table_create take any table of such refs, each carrying
 * its own in_off / out_off / base / max: blocks and lists in any order, any subset of them (the lists
 * a query touches), a block repeated in several entries, outputs anywhere below out_capacity (holes
 * between them are left as they were; the outputs of two entries must not overlap). */
typedef struct dint_block_ref {
    uint64_t in_off;  /* byte offset of the block's docs part in the index buffer            */
    uint64_t out_off; /* index of the block's first posting in the output arrays             */
    uint32_t n;       /* postings in the block, 1..256                                        */
    uint32_t base;    /* docID base: previous block's max + 1 (0 for a list's first block)    */
    uint32_t max;     /* largest docID of the block                                           */
    uint32_t list;    /* ordinal of the list                                                  */
} dint_block_ref;

/* Host: flatten the block directories of n_lists posting lists (list i starts at byte
 * list_offsets[i] of `index`) into a block table. Replaces the pointer set-up of
 * document_enumerator's constructor (dict_posting_list.hpp:90-107). Release with dint_free. */
int dint_index_posting_lists(const uint8_t* index, size_t index_bytes, const uint64_t* list_offsets,
                             size_t n_lists, dint_block_ref** blocks, size_t* n_blocks,
                             uint64_t* total_postings);

/* A block table prepared for decoding. What depends on the table alone — the docs parts' unit table and
 * docID bases, the list of short (interpolative) blocks — is computed once, here; the workspace of a
 * decode lives in the handle too. `blocks` is the HOST table (dint_index_posting_lists); the handle keeps a
 * device copy. One decode at a time per handle (calls on one stream are ordered anyway). */
typedef struct dint_block_table dint_block_table;
int dint_block_table_create(const dint_dict* docs_dict, const dint_block_ref* blocks, size_t n_blocks,
                            size_t index_bytes, dint_block_table** out);
void dint_block_table_destroy(dint_block_table* table);

/* The sizing pass over the index, done at set-up instead of under the caller's first decodes: everything a table learns as
 * it is used — where each block's docs part ends (nothing in the index says: dict_posting_list.hpp:42-53 records the end of
 * docs + freqs only), the freqs parts' units, both bundle schedules, how many blocks they left to the unit queue — learnt
 * here by decoding the index on the device into a scratch output of the table's own (4 B x 2 per posting, released before
 * the call returns). SYNCHRONOUS (it is set-up): synchronises `stream`. After it the FIRST dint_decode_block_table of the
 * table is already the one launch. freqs_dict NULL: a table that will decode docIDs only. Optional: a table not taught
 * learns under its first two decodes, as before. The CONTENT STABILITY rule of dint_decode_block_table starts here. */
int dint_block_table_learn(dint_block_table* table, const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index,
                           size_t index_bytes, void* stream);
/* 1 when the next complete dint_decode_block_table of this table (with freqs iff with_freqs) takes the one-launch form. */
int dint_block_table_ready(const dint_block_table* table, int with_freqs);
/* What a table has learnt so far. */
typedef struct dint_block_table_info {
    uint64_t n_blocks, n_short_blocks;   /* blocks; those of fewer than 256 postings (binary-interpolative) */
    uint32_t complete_decodes;           /* decodes that covered every block (learning ones included) */
    uint32_t spans_exact;                /* 1: where every docs part ends is known */
    uint32_t freqs_units_ready;          /* 1: the freqs parts' units are built */
    uint32_t docs_schedule, freqs_schedule;        /* 1: the bundle schedule is kept and its work-item count read back */
    uint32_t docs_queue_items, freqs_queue_items;  /* full blocks that fit no tile (the unit queue's: a small second launch) */
    uint32_t short_block_tickets;        /* tickets the short blocks are dealt in inside the docs launch (0: a launch of their own) */
} dint_block_table_info;
int dint_block_table_info_get(const dint_block_table* table, dint_block_table_info* info);

/* Device: decode every block of the prepared table to docIDs (and, if d_freqs is not NULL, term
 * frequencies). ASYNCHRONOUS: enqueues on `stream` and returns — except that the ONE decode that builds a table's kept
 * schedules (the second complete decode of a table not taught by dint_block_table_learn, or the first after a decode with a
 * smaller out_capacity invalidated them) reads a 4-byte count back and synchronises `stream` (and the table's side stream)
 * once before it returns: do not capture that call into a graph; call dint_block_table_learn at set-up to have none. Full blocks go through the DINT kernels —
 * the docID prefix sums are formed in the expansion, one wave scan per block, the gaps never reach memory;
 * freq = value + 1 is added where the values are stored — blocks shorter than 256 through the
 * binary-interpolative decoder (whose code is the prefix sums already). A table learns as it is used: its first decode
 * finds where the docs parts end, its second builds the bundle schedules, and from the third on a decode is ONE launch
 * for the docs parts, the short blocks (inside it, by the waves' first lanes) and the freqs parts
 * (DINT_OPT_INDEX_PAIR, DINT_OPT_INDEX_INLINE_TAILS; plus a small launch for the few blocks that fit no tile). Before
 * that — and with those options off — the freqs launch and the short blocks' decoder run on streams the table owns,
 * beside the docs launch, forked from and joined to `stream` inside the call; to the caller everything is ordered on
 * `stream` either way (dint_set_option(DINT_OPT_INDEX_CONCURRENT, 0): one stream, one launch after the other).
 * ONE STREAM AT A TIME: a table's decodes share its launch counters (two sets, taken in turn: the one-launch decode clears
 * the set of the decode after it instead of a fill per call) — successive decodes of one table must be ordered on the GPU
 * (the same stream, or streams the caller orders); two tables over one index are independent.
 * CONTENT STABILITY: what the table learns in its first complete decode (exact byte spans, the freqs parts' units, both
 * bundle schedules — which bake in the blocks' selector bytes of a multi-dictionary index) is kept and keyed by the
 * dictionaries, the index POINTER and its size, not by the bytes: while the table lives, the index at d_index must keep
 * its contents, like the stream under a dint_unit_table. An index shard reloaded into the same buffer needs a new table.
 * Replaces: see dint_decode_posting_blocks. */
int dint_decode_block_table(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index,
                            size_t index_bytes, dint_block_table* table, uint32_t* d_docids, uint32_t* d_freqs,
                            size_t out_capacity, void* stream);

/* One-shot form of the two calls above over a DEVICE block table: prepares, decodes, synchronises
 * `stream`, releases. d_index / d_blocks / outputs are device pointers on the dictionaries' device;
 * both dictionaries must be of the same kind and live on the same device.
 * Replaces: document_enumerator::decode_docs_block / decode_freqs_block + the docid
 * accumulation of next() (dict_posting_list.hpp:111-124, 284-318), i.e. dint_block::decode /
 * opt_dint_multi_dict_block::decode (include/dint/dint_codecs.hpp:13-49, 460-510) and
 * interpolative_block::decode (include/ds2i/block_codecs.hpp:130-150), for many blocks per launch. */
int dint_decode_posting_blocks(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index,
                               size_t index_bytes, const dint_block_ref* d_blocks, size_t n_blocks,
                               uint32_t* d_docids, uint32_t* d_freqs, size_t out_capacity, void* stream);

/* ---- conjunctive queries over the in-index layout ------------------------------------------
 * Replaces: the index + and_query<false> pair of the reference's query path
 * (include/ds2i/queries.hpp:34-84, driven by src/queries.cpp:15-61 op_perftest), for a batch of
 * queries per call. The query index keeps a device copy of the block table (with its block
 * maxima packed for the block-max search of next_geq, dict_posting_list.hpp:126-147) and the
 * workspaces of the query rounds; it borrows d_index and docs_dict, which must outlive it. */
typedef struct dint_query_index dint_query_index;

/* blocks: HOST block table of ALL lists as produced by dint_index_posting_lists (lists in order,
 * each list's blocks contiguous); d_index: the index bytes on docs_dict's device. DocIDs must be
 * below 0xFFFFFFFF (the reference's num_docs is a u32 and docIDs < num_docs; the query kernels use
 * 0xFFFFFFFF as their dead-slot mark): a block whose max is 0xFFFFFFFF is DINT_ERR_FORMAT. */
int dint_query_index_create(const dint_dict* docs_dict, const uint8_t* d_index, size_t index_bytes,
                            const dint_block_ref* blocks, size_t n_blocks, size_t n_lists,
                            dint_query_index** out);
void dint_query_index_destroy(dint_query_index* qi);

/* counts[q] = number of documents that contain every term of query q (duplicate terms count
 * once, queries.hpp:28-31; an empty query counts 0, :38). terms/query_offsets/counts are HOST
 * arrays: query q is terms[query_offsets[q] .. query_offsets[q+1]). A term >= n_lists is
 * DINT_ERR_ARG. The call enqueues on `stream` and returns after synchronising it: ONE launch for a single query of a
 * page or two of candidates and for a call whose queries all have at most 16 candidate pages (a workgroup per query); a
 * round per launch for a single query of a few pages; one copy in and two launches per round for a batch of larger
 * queries; a mixed call is split into its small and its other queries. Which form a call takes is moved,
 * for tests and measurements, by dint_set_option: DINT_OPT_QUERY_LEAN_PAGES, DINT_OPT_QUERY_TAIL_PAGES,
 * DINT_OPT_QUERY_FUSED_PAGES, DINT_OPT_QUERY_FUSED_COPY, DINT_OPT_QUERY_BATCH_FUSED. The batch form keeps two hashed
 * claim tables per workgroup (160 KB each workgroup, 40 MB in all, whatever the index's size), allocated at the first such call. */
int dint_and_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets,
                     size_t n_queries, uint64_t* counts, void* stream);

/* and_query<true> (queries.hpp:72-76): the same counts, and freq_sums[q] = the sum, over the matches of query q and
 * over its (distinct) terms, of the term's frequency in the matching document — what the reference reads through
 * document_enumerator::freq() at every match. Lazy like the reference (dict_posting_list.hpp:164-169, :311-318): a
 * freqs part is decoded only for the blocks that hold a match; *freq_blocks_decoded (nullable) = how many that were. */
int dint_and_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms,
                           const uint64_t* query_offsets, size_t n_queries, uint64_t* counts, uint64_t* freq_sums,
                           uint64_t* freq_blocks_decoded, void* stream);

/* ---- disjunctive queries over the same query index --------------------------------------------
 * counts[q] = number of distinct documents that contain at least one term of query q: or_query<false>
 * (include/ds2i/queries.hpp:86-130, driven by src/queries.cpp:15-61 op_perftest), for a batch of queries per call.
 * Duplicate terms count once (queries.hpp:29-32, :92); an empty query counts 0 (:90-91). Arguments, host arrays, the
 * handle's lock and the stream are as for dint_and_queries: the call enqueues on `stream` and returns after
 * synchronising it. A term >= n_lists is DINT_ERR_ARG. A single-term query is answered from the list's length, with no
 * launch. Otherwise every block of every distinct term is decoded (the reference's loop reads every posting), in
 * passes of whole queries of at most DINT_OPT_QUERY_OR_PASS_PAGES pages, and ONE probe launch per pass counts every
 * posting that no earlier (longer) list of its query holds. The workspaces are the AND calls' own;
 * OR calls leave their claim tables as they found them. */
int dint_or_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets,
                    size_t n_queries, uint64_t* counts, void* stream);

/* or_query<true> (queries.hpp:86-130 with_freqs: freq() is read for every posting of every distinct term, :110-122):
 * the same counts, and freq_sums[q] = the sum, over the distinct terms of q and over every posting of the term's list,
 * of the posting's frequency. *freq_blocks_decoded (nullable) = the blocks whose freqs part was decoded: every block of
 * every distinct term of every query of the call (a block in the lists of several queries counts once per list).
 * freqs_dict: of the same kind and device as the query index's docs dictionary. */
int dint_or_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms,
                          const uint64_t* query_offsets, size_t n_queries, uint64_t* counts, uint64_t* freq_sums,
                          uint64_t* freq_blocks_decoded, void* stream);

/* ---- ranked conjunctive queries (BM25 top-k) over the same query index ---------------------------
 * Replaces: wand_data's norm_lens (include/ds2i/wand_data.hpp:18-57) on the device, and ranked_and_query
 * (include/ds2i/queries.hpp:309-385, src/queries.cpp:106-108) for a batch of queries per call.
 * dint_wand_data_create uploads norm_lens (HOST, num_docs floats: dinth_wand_data of include/dint_host.h) to `device` once;
 * the handle owns its copy. */
typedef struct dint_wand_data dint_wand_data;
int dint_wand_data_create(int device, const float* norm_lens, uint64_t num_docs, dint_wand_data** out);
void dint_wand_data_destroy(dint_wand_data* wd);

#define DINT_RANKED_MAX_K 1024 /* the largest k the ranked calls (AND, OR, pruned OR) take */

/* For query q — its distinct terms t with multiplicity qf_t (query_freqs, queries.hpp:135-148) — every document d of the
 * intersection of their lists scores sum_t q_weight_t * doc_term_weight(freq_t(d), norm_lens[d]) (bm25.hpp), with
 * q_weight_t = query_term_weight(qf_t, df_t = the list's length, wd's num_docs), the sum taken over the terms in order of
 * increasing list length, equal lengths by increasing term id, every operation a binary32 one, uncontracted, in the
 * reference's source order. counts[q] = min(k, size of the intersection); scores[q * k + i] /
 * docids[q * k + i] for i < counts[q]: the best documents, by descending score, equal scores by ascending docID; past
 * counts[q]: 0.0f / 0xFFFFFFFF. scores (and docids, nullable) are HOST arrays of n_queries * k. Terms, query_offsets,
 * counts, the handle's lock and the stream are as for dint_and_queries_freqs; an empty query counts 0. DINT_ERR_ARG: k == 0
 * or k > DINT_RANKED_MAX_K, a term >= n_lists, a freqs_dict of another kind or device than the docs dictionary, a wand
 * handle on another device, or one whose num_docs does not exceed the index's largest docID — checked before anything is
 * launched. Every query takes the round-per-launch form (never the workgroup-per-query batch form of dint_and_queries). */
int dint_ranked_and_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                            const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts,
                            float* scores, uint32_t* docids, void* stream);

/* ---- ranked boolean queries (required, optional and excluded terms; BM25 top-k) over the same query index ----
 * Replaces: ranked_and_query (include/ds2i/queries.hpp:309-385) generalised to the mix a caller of a BM25 index asks for —
 * documents that contain ALL of the required terms and NONE of the excluded ones, ranked with the optional terms counted
 * where they occur (Lucene's MUST / MUST_NOT / SHOULD) — over the cursor primitive next_geq + freq()
 * (include/dint/dict_posting_list.hpp:126-169), for a batch of queries per call. dint_ranked_and_queries ignores optional
 * terms and excludes nothing; dint_ranked_or_queries with a large k, filtered by the caller, decodes every block and is
 * capped at DINT_RANKED_MAX_K; re-scoring dint_ranked_and_queries' top k (dint_score_documents) ranks a top k that was chosen
 * without the optional terms.
 * The three clauses are HOST terms / offsets pairs laid out as in every query call (offsets: n_queries + 1 entries); a
 * pair may be null when the clause is empty for every query. Within a clause repeated terms are one term with multiplicity
 * qf (query_freqs, queries.hpp:135-148); the clauses are independent: a term in both `must` and `should` is scored once in
 * each phase, a term in both `must` and `not` matches nothing.
 * The matches of query q: the documents in every list of must[q] and in no list of not[q]. A QUERY WITHOUT A REQUIRED TERM
 * SELECTS NOTHING (count 0, outputs empty): the union-driven query, with exclusions and a minimum number of optional terms,
 * is dint_ranked_or_bool_queries'. The score of a match d starts at 0.0f; the required terms are added in dint_ranked_and_queries' order
 * (increasing list length, equal lengths by increasing term id), then the optional terms whose list holds d, in ascending
 * term id; every addend is q_weight_t * doc_term_weight(freq_t(d), norm_lens[d]), q_weight_t = query_term_weight(qf_t within
 * its clause, the list's length, wd's num_docs), every operation a binary32 one, uncontracted, as in
 * dint_ranked_and_queries. An optional term whose list is empty, or ends before d, adds nothing.
 * matches[q] (HOST, nullable) = the number of matches; counts[q] = min(k, matches); scores, docids (nullable), their order
 * (descending score, equal scores by ascending docID) and their filler (0.0f / 0xFFFFFFFF) are dint_ranked_and_queries'.
 * With empty `should` and `not` clauses the call returns dint_ranked_and_queries' answer for the `must` clause, bit for bit.
 * Lazy: behind the AND rounds of the required terms, the excluded terms — in ascending term id — decode docs parts only,
 * and only of the blocks the candidates still alive (the intersection's documents no earlier excluded term removed) fall
 * in; exclusion runs before any scoring, and the required and optional terms decode docs and freqs parts only of the
 * blocks the MATCHES fall in. A candidate past a list's last docID claims nothing.
 * *blocks_decoded (nullable) = the block claims of these steps behind the AND rounds. For a call of one query it is exact:
 * the sum over the excluded, required and optional terms of the distinct blocks just described. In a batch a block that
 * several queries claim in the same step counts once, so the batch's value is at most the sum of the one-query values.
 * DINT_ERR_ARG, before anything is launched: what dint_ranked_and_queries refuses (k == 0 or k > DINT_RANKED_MAX_K, a
 * freqs_dict of another kind or device, a wand handle on another device or one whose num_docs does not exceed the index's
 * largest docID, null counts or scores), and decreasing offsets or a term >= n_lists in any clause. The handle's lock and
 * the stream are as for dint_ranked_and_queries; every query takes the round-per-launch form. */
int dint_ranked_bool_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                             const uint32_t* must_terms, const uint64_t* must_offsets, const uint32_t* should_terms,
                             const uint64_t* should_offsets, const uint32_t* not_terms, const uint64_t* not_offsets, size_t n_queries,
                             uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream);

/* ---- union-driven ranked boolean queries (optional terms, a minimum of them, excluded terms; BM25 top-k) ----
 * Replaces: ranked_or_query (include/ds2i/queries.hpp:387-457) with the two filters a free-text query asks for — "some of
 * these words, at least m of them, and none of those" (Lucene's pure SHOULD with MUST_NOT and minimum_should_match) — for a
 * batch of queries per call; the excluded terms run over next_geq (include/dint/dict_posting_list.hpp:126-169).
 * dint_ranked_or_queries excludes nothing and asks for one term; filtering its output needs a k above DINT_RANKED_MAX_K as
 * soon as an excluded term is frequent; dint_ranked_bool_queries selects nothing without a required term.
 * Clauses: `should` and `not` are HOST terms / offsets pairs laid out as in dint_ranked_bool_queries (offsets: n_queries + 1
 * entries); the `not` pair may be null: no exclusions. Repeated terms within `should` are one term with multiplicity qf
 * (query_freqs, queries.hpp:135-148); repeats in `not` are one term. The clauses are independent: a term in both matches
 * nothing through that term's list (every document of the list is excluded).
 * m: min_should_match is a HOST array of n_queries (null: all 1); m_q = max(1, min_should_match[q]) counts the DISTINCT
 * optional terms whose list holds the document. m_q above the query's number of distinct optional terms selects nothing.
 * The matches of query q: the documents held by at least m_q of the distinct should[q] lists and by no not[q] list.
 * The score of a match is exactly dint_ranked_or_queries' score over should[q]: from 0.0f, the terms whose list holds the
 * document in ascending term id, q_weight_t * doc_term_weight(freq_t(d), norm_lens[d]) each (bm25_add), every operation a
 * binary32 one, uncontracted. Excluded terms never score. With no exclusions and every m_q <= 1 the call returns
 * dint_ranked_or_queries' counts, scores and docIDs bit for bit. With m_q equal to the number of distinct terms the
 * documents are the intersection's, but the sums keep dint_ranked_or_queries' order (ascending term id), not
 * dint_ranked_and_queries' (increasing list length): the scores of the two calls may differ in the last place.
 * matches[q] (HOST, nullable) = the number of matches; counts[q] = min(k, matches); scores, docids (nullable), their order
 * (descending score, equal scores by ascending docID) and their filler (0.0f / 0xFFFFFFFF) are the other ranked calls'.
 * *blocks_decoded (nullable) = an eager and a lazy part. Eager, dint_ranked_or_queries' unit: every block of every distinct
 * optional term of every query that can match (a query with no block in its lists, or with m_q above its distinct terms,
 * decodes nothing and returns zeros). Lazy, the claims of the exclusion steps: per excluded term, in ascending term id, the
 * blocks whose docs part was decoded because a candidate that survived the m-filter and the earlier exclusions falls in
 * them; a candidate past a list's last docID claims nothing. The value is exact for a call of one query; in a batch a block
 * that several queries claim in the same step counts once, so the batch's value is at most the sum of the one-query values.
 * DINT_ERR_ARG, before anything is launched (no output is written): everything dint_ranked_or_queries refuses (k == 0 or
 * k > DINT_RANKED_MAX_K, a freqs_dict of another kind or device, a wand handle on another device or one whose num_docs does
 * not exceed the index's largest docID, null counts or scores), decreasing offsets, and a term >= n_lists in either clause.
 * The handle's lock, the stream and the passes (DINT_OPT_QUERY_OR_PASS_PAGES: whole queries, sized by their optional
 * terms' blocks) are dint_ranked_or_queries'; there is no option of its own. */
int dint_ranked_or_bool_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                const uint32_t* should_terms, const uint64_t* should_offsets, const uint32_t* not_terms,
                                const uint64_t* not_offsets, const uint32_t* min_should_match, size_t n_queries, uint64_t* counts,
                                uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream);

/* ---- ranked disjunctive queries (BM25 top-k of the union) over the same query index --------------
 * Replaces: ranked_or_query (include/ds2i/queries.hpp:387-457) for a batch of queries per call. (Not a query type of
 * the reference's driver, src/queries.cpp:93-111.)
 * For query q — its distinct terms t with multiplicity qf_t — every document d of the union of their lists scores
 *     score = 0.0f; for t in ascending term id, if d is in L_t: score = score + q_weight_t * doc_term_weight(freq_t(d), norm_lens[d])
 * with q_weight_t as for dint_ranked_and_queries, every operation a binary32 one, uncontracted, in the reference's source
 * order. The sum runs in ascending term id, the order of query_freqs (queries.hpp:135-148) and so
 * of ranked_or_query, unlike dint_ranked_and_queries, which sums in list-length order. wand_query and maxscore_query
 * (queries.hpp:190-307, :459-575) return the same documents, but add the same terms in data-dependent orders and may
 * differ from these scores in the last bits. counts[q] = min(k, size of the union); the arguments, outputs, errors
 * (all checked before anything is launched), the handle's lock and the stream are exactly those of
 * dint_ranked_and_queries. The call runs in passes of whole queries of at most DINT_OPT_QUERY_OR_PASS_PAGES pages, as
 * dint_or_queries_freqs does, and every document of a union is scored by one thread, at its first occurrence. */
int dint_ranked_or_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                           const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts,
                           float* scores, uint32_t* docids, void* stream);

/* ---- MaxScore-pruned ranked disjunctive queries over the same query index ---------------------------
 * Replaces: the dynamic pruning of maxscore_query (include/ds2i/queries.hpp:459-573), with ranked_or_query's sums.
 * dint_wand_data_create_with_max_weights is dint_wand_data_create plus a HOST copy of wand_data's max_term_weight[n_lists]
 * (dinth_wand_data / dinth_read_wand_data of include/dint_host.h); max_term_weight may be null only if n_lists is 0.
 * A NaN or negative maximum is DINT_ERR_ARG, checked before the device is touched (*out is null then); -0.0f, +inf and
 * FLT_MAX are accepted.
 * dint_ranked_or_maxscore_queries returns exactly what dint_ranked_or_queries returns — counts, scores and docIDs, bit for
 * bit — but does not decode the blocks of the low-weight lists that no candidate able to reach the top k falls in
 * (DESIGN.md 4d-maxscore): per query a threshold from its shortest list of at least k postings, the terms whose summed
 * maxima stay below it left out of the candidates, each candidate's upper bound checked, and the blocks of those terms
 * claimed by the surviving candidates only. SAFETY ASSUMPTION: max_term_weight[t] >= f / (f + k1 * ((1 - b) + b * norm_len))
 * of every posting of list t, as the kernels compute it in binary32; dinth_wand_data and dint_create_wand_data compute
 * max_term_weight with that very expression, so their files and arrays hold it. Any larger maxima (up to +inf) give the same
 * answer and only read more blocks; with +inf nothing is left out and every block is read. Smaller maxima may drop
 * documents and nothing else: the call still returns DINT_OK, every (docID, score) it returns is a document of the union
 * with its exact dint_ranked_or_queries score, in that call's order, and counts[q] is at most that call's.
 * *blocks_read (nullable) = the sum over the call's queries of the distinct index blocks whose docs and freqs parts the
 * query's evaluation decoded (the unit of dint_or_queries_freqs' freq_blocks_decoded; dint_ranked_or_queries reads every
 * block of every distinct term). Arguments, outputs, errors, lock, stream and passes are those of dint_ranked_or_queries;
 * besides, DINT_ERR_ARG before anything is launched: a wand handle without maxima (dint_wand_data_create), or with fewer
 * than the index's n_lists of them. */
int dint_wand_data_create_with_max_weights(int device, const float* norm_lens, uint64_t num_docs, const float* max_term_weight,
                                           size_t n_lists, dint_wand_data** out);
int dint_ranked_or_maxscore_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts,
                                    float* scores, uint32_t* docids, uint64_t* blocks_read, void* stream);

/* ---- docID-range ranked queries (BM25 top-k of the union / the intersection within a docID interval) ----
 * Replaces: ranked_or_query / ranked_and_query (include/ds2i/queries.hpp:309-457) with a restriction of every query to a
 * half-open docID interval — a site or host of a URL-ordered collection, a date range of a time-ordered one, a document
 * shard of a shared index, a page of a walk through the docID space past DINT_RANKED_MAX_K — for a batch of queries per
 * call. dint_ranked_or_queries / dint_ranked_and_queries with a large k, filtered by the caller, are capped at
 * DINT_RANKED_MAX_K and decode every block of every term (OR) or seed from the whole rarest list (AND).
 * ranges (HOST, n_queries entries; null: every query unrestricted): query q ranks over the docIDs lo <= d < hi.
 * The matches of query q: the documents of the unranged call's match set (the union of its lists for
 * dint_ranked_or_range_queries, the intersection for dint_ranked_and_range_queries) with lo_q <= d < hi_q. lo_q >= hi_q
 * selects nothing and decodes nothing. [0, 0xFFFFFFFF) is unrestricted (docIDs are below 0xFFFFFFFF); with it, or with
 * null ranges, counts, scores and docids are the unranged call's, bit for bit.
 * The score of a match is EXACTLY the unranged call's — the same terms in the same order (OR: ascending term id; AND:
 * increasing list length, equal lengths by increasing term id), the same binary32 operations, and q_weight_t still from the
 * WHOLE list's length and wd's num_docs: the range filters, it does not re-weight. Merging the answers of ranges that tile
 * the docID space (by descending score, equal scores by ascending docID) therefore reproduces the unranged answer.
 * matches[q] (HOST, nullable) = the number of matches in range; counts[q] = min(k, matches[q]); scores, docids (nullable),
 * their order (descending score, equal scores by ascending docID) and their filler (0.0f / 0xFFFFFFFF) are the other
 * ranked calls'.
 * Skipping: of a list only the blocks that can hold a docID of the range are decoded. A block with dint_block_ref fields
 * base and max is in range iff max >= lo && base < hi; as positions of a list with block maxima M[0 .. nb) these are
 * [p0, p1), p0 = lower_bound(M, lo), p1 = min(nb, lower_bound(M, hi - 1) + 1). At most two blocks a term (the first and the
 * last in range) hold documents outside the range; those are dropped on the device before they are scored or probe anything.
 * *blocks_decoded (nullable), exact for any batch — OR: the sum over the queries and over their distinct terms of the
 * list's blocks in range (dint_or_queries_freqs' unit: a block in the lists of several queries counts once per query; on
 * the unrestricted range, every block of every distinct term); AND: the candidate pages, i.e. the blocks in range of each
 * query's rarest list (shortest, equal lengths by term id), summed over the queries. The blocks the AND rounds and its
 * scoring claim behind that are the unranged call's lazy ones, for in-range candidates only, and are not counted.
 * DINT_ERR_ARG, before anything is launched (no output is written): what the unranged calls refuse — k == 0 or
 * k > DINT_RANKED_MAX_K, a term >= n_lists, decreasing offsets, null counts or scores, a freqs_dict of another kind or
 * device than the docs dictionary, a wand handle on another device or one whose num_docs does not exceed the index's
 * largest docID. Any lo / hi pair is legal. Terms, query_offsets, the handle's lock and the stream are as for the unranged
 * calls. The OR call runs in dint_ranked_or_queries' passes (DINT_OPT_QUERY_OR_PASS_PAGES), sized by the blocks IN RANGE, so a
 * batch of narrow ranges packs more queries into a pass; the AND call takes the round-per-launch form with the first
 * round's search as a launch of its own (never the one-launch forms: DESIGN.md 4d-range). */
typedef struct dint_doc_range {
    uint32_t lo, hi; /* [lo, hi) */
} dint_doc_range;
int dint_ranked_or_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                 const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges,
                                 size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids,
                                 uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges,
                                  size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids,
                                  uint64_t* blocks_decoded, void* stream);

/* ---- document-filter ranked queries (BM25 top-k of the union / the intersection within a set of documents) ----
 * Replaces: ranked_or_query / ranked_and_query (include/ds2i/queries.hpp:309-457) with a restriction of a whole call to an
 * arbitrary set of documents, given as a bitmap over the docID space — the documents not deleted, a category, a language, a
 * tenant, an access list — for a batch of queries per call under ONE filter. The unfiltered calls with a large k, filtered
 * by the caller, are capped at DINT_RANKED_MAX_K and decode every block for nothing; the range calls take one interval a
 * query.
 * A filter handle (dint_doc_filter_create): bits is a HOST array of ceil(num_docs / 64) words, document d in the filter iff
 * d < num_docs and bit (d & 63) of word (d >> 6) is set. The handle keeps its own copy (bits may be released at once) and
 * ignores the bits at and past num_docs of the last word. num_docs may be smaller or larger than the index's largest
 * docID: docIDs at or past it are not in the filter. num_docs == 0: the empty filter, bits may be null.
 * num_docs > 0xFFFFFFFF, a null qi or out: DINT_ERR_ARG. The handle belongs to the query index it was created for — it
 * holds, for that index's block table, which blocks are LIVE: a block with dint_block_ref fields base and max is live iff
 * the filter holds a document d with base <= d <= max (and d < num_docs). These are found on the device at creation (a rank
 * directory of the bitmap, a thread per block, a prefix count of the live blocks), under the index's lock, which the handle
 * takes at no other time. It is immutable afterwards, usable from several host threads at once, and must be destroyed
 * before its index. dint_doc_filter_info_get: n_set = the documents in the filter, n_blocks = the index's blocks,
 * live_blocks = the live ones.
 * The filtered calls, filter one handle for the whole call: the matches of query q are the documents of the unfiltered
 * call's match set (the union of its lists for dint_ranked_or_filtered_queries, the intersection for
 * dint_ranked_and_filtered_queries) that are in the filter. An empty filter selects nothing and decodes nothing. A null
 * filter is unrestricted — the range calls on null ranges — and a filter with every bit set up to at least the index's
 * largest docID + 1 gives the same: counts, scores and docids are the unfiltered call's, bit for bit. A filter that holds
 * exactly the docIDs [lo, hi) gives the range call's counts, matches, scores, docids and *blocks_decoded on that range
 * (live and in range are one rule for an interval).
 * The score of a match is EXACTLY the unfiltered call's — the same terms in the same order (OR: ascending term id; AND:
 * increasing list length, equal lengths by increasing term id), the same binary32 operations, and q_weight_t still from the
 * WHOLE list's length and wd's num_docs: the filter filters, it does not re-weight.
 * matches[q] (HOST, nullable) = the number of matches in the filter; counts[q] = min(k, matches[q]); scores, docids
 * (nullable), their order (descending score, equal scores by ascending docID) and their filler (0.0f / 0xFFFFFFFF) are the
 * other ranked calls'.
 * Skipping: of a list only the live blocks are decoded, wherever they lie in the list. What a live block holds outside the
 * filter is dropped on the device before it is scored or probes anything. A scattered filter leaves almost every block
 * live (a block of 256 postings is dead only if none of the docIDs it spans is in the filter): there the drop is what
 * pays, the skipping pays for clustered filters.
 * *blocks_decoded (nullable), exact for any batch — OR: the sum over the queries and over their distinct terms of the
 * list's live blocks; AND: the candidate pages, i.e. the live blocks of each query's rarest list (shortest, equal lengths
 * by term id), summed over the queries. The blocks the AND rounds and its scoring claim behind that are the unfiltered
 * call's lazy ones, for candidates in the filter only, and are not counted.
 * DINT_ERR_ARG, before anything is launched (no output is written): what the unfiltered calls refuse — k == 0 or
 * k > DINT_RANKED_MAX_K, a term >= n_lists, decreasing offsets, null counts or scores, a freqs_dict of another kind or
 * device than the docs dictionary, a wand handle on another device or one whose num_docs does not exceed the index's
 * largest docID — and a filter created for another query index. Terms, query_offsets, the handle's lock and the stream
 * are as for the unfiltered calls. The OR call runs in dint_ranked_or_queries' passes (DINT_OPT_QUERY_OR_PASS_PAGES), sized by
 * the LIVE blocks; the AND call takes the round-per-launch form with the first round's search as a launch of its own, as
 * the range call does. A filter per query, and a filter combined with a range, are out of scope. */
typedef struct dint_doc_filter dint_doc_filter;
typedef struct dint_doc_filter_info {
    uint64_t num_docs;    /* as given to dint_doc_filter_create                  */
    uint64_t n_set;       /* documents in the filter                             */
    uint64_t n_blocks;    /* blocks of the query index                           */
    uint64_t live_blocks; /* ... whose [base, max] holds a document of the filter */
} dint_doc_filter_info;
int dint_doc_filter_create(dint_query_index* qi, const uint64_t* bits, uint64_t num_docs, dint_doc_filter** out);
int dint_doc_filter_info_get(const dint_doc_filter* f, dint_doc_filter_info* info);
void dint_doc_filter_destroy(dint_doc_filter* f);
int dint_ranked_or_filtered_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                    size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids,
                                    uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_filtered_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                     const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                     size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids,
                                     uint64_t* blocks_decoded, void* stream);

/* ---- facet counts of the ranked queries (how many matches each document group holds) -----------------------------
 * Adds: what a cursor engine computes with a facet collector beside its top-k collector (ranked_or_query / ranked_and_query,
 * include/ds2i/queries.hpp:309-457, have none) — per query and per group of documents (a category, a site, a tenant, a
 * date) the number of the query's matches in the group, for a batch of queries, in the call that ranks them. One filtered
 * call per group answers the same, and decodes and scores everything once per group.
 * A facets handle (dint_doc_facets_create): group_of is a HOST array of num_docs words; document d belongs to group
 * group_of[d], or to no group if that word is DINT_FACET_NONE or d >= num_docs. The handle takes its device as
 * dint_wand_data_create does and belongs to no query index: it describes documents, not blocks, and survives an index
 * rebuild. It keeps its own copy of the map on the device, 4 BYTES PER DOCUMENT (group_of may be released at once), is
 * immutable and usable from several host threads at once. DINT_ERR_ARG (no handle): n_groups == 0,
 * n_groups > DINT_FACETS_MAX_GROUPS, num_docs > 0xFFFFFFFF, a null array with num_docs > 0, a null out, or any entry that
 * is neither below n_groups nor DINT_FACET_NONE — found on the device: creation copies the map and runs one launch over
 * it, which also counts the group sizes (the whole collection's histogram) with the device function the queries count
 * with. dint_doc_facets_info_get: n_grouped = the documents in some group; dint_doc_facets_group_sizes: sizes[g] (HOST,
 * n_groups words) = the documents of group g; both from the host, no device work.
 * The faceted calls: counts, matches, scores, docids and *blocks_decoded are bit for bit what
 * dint_ranked_or_filtered_queries / dint_ranked_and_filtered_queries return for the same arguments (filter null: the
 * unfiltered answer with the matches counted). facet_counts (HOST, n_queries * n_groups words):
 * facet_counts[q * n_groups + g] = the number of matches of query q whose group is g — over EVERY match, not over the top
 * k — so the row's sum plus the matches in no group equals matches[q]; an empty query, or one without a match, has a row
 * of zeros. The counts are integer sums: exact and the same from run to run.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse, a null facets or facet_counts,
 * a facets handle on another device than the index, n_queries * n_groups > 2^28 (the caller batches). The rows are a
 * workspace of the query index (4 bytes * n_queries * n_groups, grow-only), cleared once per call. Terms, query_offsets,
 * the handle's lock and the stream are as for the filtered calls; besides their launches a call runs one counting launch
 * per OR pass / per AND call, which reads the candidate slots once more. Facets on the other query
 * forms, several maps per call and score sums are out of scope; the best document per group: the collapsed
 * calls below. */
#define DINT_FACET_NONE 0xFFFFFFFFu   /* a document in no group */
#define DINT_FACETS_MAX_GROUPS 65536u
typedef struct dint_doc_facets dint_doc_facets;
typedef struct dint_doc_facets_info {
    uint64_t num_docs;  /* as given to dint_doc_facets_create */
    uint64_t n_groups;  /* as given to dint_doc_facets_create */
    uint64_t n_grouped; /* documents in some group            */
} dint_doc_facets_info;
int dint_doc_facets_create(int device, const uint32_t* group_of, uint64_t num_docs, uint32_t n_groups, dint_doc_facets** out);
int dint_doc_facets_info_get(const dint_doc_facets* f, dint_doc_facets_info* info);
int dint_doc_facets_group_sizes(const dint_doc_facets* f, uint32_t* sizes);
void dint_doc_facets_destroy(dint_doc_facets* f);
int dint_ranked_or_faceted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                   const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                   const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores,
                                   uint32_t* docids, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_faceted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                    const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores,
                                    uint32_t* docids, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);

/* ---- collapsed ranked queries (the best document of every document group) ------------------------------------------
 * Adds: what a cursor engine computes with a collapsing collector in place of its top-k collector (ranked_or_query /
 * ranked_and_query, include/ds2i/queries.hpp:309-457, have none) — at most one hit per group of documents (a site, a
 * product, a thread): the k best GROUPS of every query, each shown by its best document, for a batch of queries, in the call
 * that ranks them. One filtered call per group answers the same and decodes and scores everything once per group; fetching
 * more than k hits and collapsing on the host is wrong as soon as one group holds more than the over-fetch.
 * A document's key is the one the selection sorts by: the score's bits, then the inverted docID — a higher score wins, equal
 * scores go to the smaller docID. A query's KEPT documents are, for every group with at least one match, the match of that
 * group with the largest key, and every match that is in no group (DINT_FACET_NONE, or a docID at or past the map's
 * num_docs): such a document stands for itself. Arguments as the faceted calls take them; the outputs (HOST):
 *   counts, scores, docids  the top k of the kept documents in key order, filled as the other ranked calls fill them
 *                           (0.0f / 0xFFFFFFFF past the count); every kept hit carries exactly the score the unfiltered
 *                           call gives that document
 *   matches[q]              (nullable) every match, exactly as the faceted call reports it
 *   collapsed[q]            the kept documents: groups with a match plus ungrouped matches; counts[q] = min(collapsed[q], k)
 *   hit_groups[q * k + i]   the group of hit i, DINT_FACET_NONE for an ungrouped hit and past the count
 *   hit_group_matches[q * k + i]  the matches of query q in that group (the faceted row's entry), 1 for an ungrouped hit,
 *                           0 past the count
 *   facet_counts            (nullable, n_queries * n_groups words) the faceted call's rows, bit for bit; the rows are counted
 *                           on the device either way and copied only when asked for
 *   *blocks_decoded         (nullable) the filtered / faceted call's value
 * The reduction is a 64-bit maximum per (query, group): order-independent, so the answer is exact and the same from run to
 * run (a float sum per group would not be: score sums stay out).
 * DINT_ERR_ARG, before anything is written or launched: whatever the faceted calls refuse except a null facet_counts; a null
 * collapsed, hit_groups or hit_group_matches; n_queries * n_groups > 2^27 — the per-call table of best keys is 8 BYTES PER
 * (QUERY, GROUP), a grow-only workspace of the query index cleared once per call, so this is 1 GiB; the caller batches.
 * Besides the faceted call's launches a call runs two launches over the candidate slots in front of the selection and one
 * over the selected keys behind it, per OR pass / per AND call. Several hits per group and collapsing
 * on the boolean and pruned forms are out of scope; the hits behind the first k: the paged calls below. */
int dint_ranked_or_collapsed_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                     const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                     const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                     uint64_t* collapsed, float* scores, uint32_t* docids, uint32_t* hit_groups,
                                     uint32_t* hit_group_matches, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_collapsed_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                      uint64_t* collapsed, float* scores, uint32_t* docids, uint32_t* hit_groups,
                                      uint32_t* hit_group_matches, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);

/* ---- search_after paging of the ranked queries (the hits behind a cursor) ------------------------------------------
 * Adds: what a front end needs for page 2 of a result list and a cursor engine's top-k queue cannot give (ranked_or_query /
 * ranked_and_query, include/ds2i/queries.hpp:309-457, return one queue of k) — the best k matches BEHIND a position of the
 * ranking, for a batch of queries with a position each. Asking with a larger k ends at DINT_RANKED_MAX_K; the range calls page
 * the docID order, not the ranking.
 * A cursor is a position in the order the selection sorts by: the score's bits, then the inverted docID. A match (s, d) of
 * query q lies AFTER after[q] = (cs, cd) iff s < cs, or s == cs and d > cd: its key bits(s) << 32 | (0xFFFFFFFF - d) is
 * strictly below the cursor's. The comparison is on bits and takes no tolerance. The last hit of one page is the cursor of
 * the next; the cursor need not be a match — any docID and any finite score give a well-defined cut. Special values:
 *   after == NULL, or score == +inf   from the start: the query's outputs are the un-paged call's, bit for bit, skipped 0
 *   score <= 0 (-0.0f, -inf)          nothing lies after it (every score is > 0): count 0, skipped = every match
 *   score NaN                         DINT_ERR_ARG
 * dint_ranked_or_paged_queries / dint_ranked_and_paged_queries take the arguments of the filtered calls (filter nullable:
 * unrestricted) and after (HOST, nullable, n_queries entries); the outputs (HOST):
 *   matches[q]       (nullable) every match, as the filtered call reports it: the cursor does not change it
 *   skipped[q]       (nullable) the matches that are NOT after the cursor: the rank of the page's first hit
 *   counts[q]        min(k, matches[q] - skipped[q])
 *   scores, docids   the best k of the matches after the cursor; order and filler are the other ranked calls'
 *   *blocks_decoded  (nullable) the filtered call's value: the plan does not depend on the cursor
 * dint_ranked_or_collapsed_paged_queries / dint_ranked_and_collapsed_paged_queries take the collapsed calls' arguments, after
 * and skipped. The cursor applies to the KEPT documents, after the best of every group is taken — a group's best does not
 * depend on the page, so walking the pages shows every group once. collapsed[q] is the collapsed call's; skipped[q] counts the
 * kept documents not after the cursor; counts[q] = min(k, collapsed[q] - skipped[q]); hit_groups, hit_group_matches, the rows
 * and matches are defined as the collapsed call defines them.
 * What a page costs: the whole query. Nothing is kept on the device between pages; every page decodes and scores again, and
 * one launch over the candidate slots in front of the selection (per OR pass / per AND call) kills and counts what is not
 * after the cursor — the selection then sees fewer live slots. The cursor keys and the counters are a grow-only workspace of
 * the query index (16 bytes per query), sent and cleared once per call. The counts are integer sums: exact and the same from
 * run to run.
 * A match whose score has underflowed to 0.0f (a norm_len so large that every addend rounds to zero) cannot be paged past: a
 * cursor at such a hit has score <= 0 and ends the walk.
 * DINT_ERR_ARG, before anything is written or launched: exactly what the filtered / collapsed calls refuse, and a NaN cursor
 * score. A scroll that keeps scored slots on the device between pages, paging on the boolean and pruned forms and backwards
 * paging are out of scope. */
typedef struct dint_rank_cursor {
    float score;
    uint32_t docid;
} dint_rank_cursor;
int dint_ranked_or_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                 const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                 const dint_rank_cursor* after, size_t n_queries, uint64_t* counts, uint64_t* matches, uint64_t* skipped,
                                 float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                  const dint_rank_cursor* after, size_t n_queries, uint64_t* counts, uint64_t* matches, uint64_t* skipped,
                                  float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream);
int dint_ranked_or_collapsed_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                           const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                           const dint_doc_facets* facets, const dint_rank_cursor* after, size_t n_queries, uint64_t* counts,
                                           uint64_t* matches, uint64_t* collapsed, uint64_t* skipped, float* scores, uint32_t* docids,
                                           uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* facet_counts,
                                           uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_collapsed_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                            const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                            const dint_doc_facets* facets, const dint_rank_cursor* after, size_t n_queries, uint64_t* counts,
                                            uint64_t* matches, uint64_t* collapsed, uint64_t* skipped, float* scores, uint32_t* docids,
                                            uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* facet_counts,
                                            uint64_t* blocks_decoded, void* stream);

/* ---- group-limited ranked queries (up to n hits of every document group) --------------------------------------------
 * Adds: what a front end most often needs from grouping and the all-or-one collapse cannot give — "at most two results per
 * site", "three offers per product", "the top five messages per thread". One filtered call per group decodes and scores the
 * query once per group; over-fetching and cutting on the host ends at DINT_RANKED_MAX_K and is wrong as soon as one group
 * fills the over-fetch.
 * dint_ranked_or_group_limit_queries / dint_ranked_and_group_limit_queries take the collapsed paged calls' arguments and
 * per_group, 1 .. DINT_GROUP_LIMIT_MAX. A document's key is the selection's: the score's bits, then the inverted docID. A
 * query's KEPT documents are, for every group with at least one match, its min(per_group, matches in the group) matches
 * with the largest keys — equal scores: the smaller docID first — and every match in no group (DINT_FACET_NONE, or a docID
 * at or past the map's num_docs), which stands for itself as in the collapsed call. The outputs (HOST):
 *   kept[q]               the kept documents
 *   skipped[q]            (nullable) the kept documents that are NOT after after[q]: the cursor applies to the kept documents,
 *                         AFTER the groups' best are taken, exactly as the collapsed paged calls apply it (NULL or +inf: from
 *                         the start; a score <= 0 leaves nothing after it; NaN: DINT_ERR_ARG)
 *   counts[q]             min(k, kept[q] - skipped[q])
 *   scores, docids        the best k kept documents after the cursor; order and filler are the other ranked calls'
 *   hit_groups, hit_group_matches   [q * k + i] as the collapsed call defines them
 *   hit_group_ranks       [q * k + i] the hit's 0-based position among ALL matches of its group in key order: 0 is the
 *                         group's best, always < per_group; 0 for an ungrouped hit and past the count
 *   matches, facet_counts, *blocks_decoded   (nullable) the faceted call's, bit for bit: the plan depends on neither
 *                         per_group nor the cursor
 * Every kept hit carries exactly the score the unfiltered call gives that document. per_group == 1 is the collapsed paged
 * call byte for byte, with every rank 0; a per_group of at least the largest group's matches keeps every match, and the hits
 * are the paged call's.
 * What it costs: the whole query, the faceted call's launches, and per OR pass / per AND call per_group + 2 more — one pass
 * over the candidate slots per place (place r of a group is the largest key strictly below its place r - 1: a 64-bit
 * maximum of integers, exact and the same from run to run), one that kills what lies below a group's last place, and one
 * over the selected keys. The table of places is a grow-only workspace of the query index, 8 BYTES PER (QUERY, GROUP,
 * PLACE), cleared once per call; n_queries * n_groups * per_group is capped at 2^27 (1 GiB): the caller batches.
 * DINT_ERR_ARG, before anything is written or launched: what the collapsed paged calls refuse, a null kept, hit_groups,
 * hit_group_matches or hit_group_ranks, per_group == 0 or > DINT_GROUP_LIMIT_MAX, and n_queries * n_groups * per_group > 2^27.
 * A grouped response (k groups with n hits each), a per_group per query, the boolean, pruned and sorted forms and a one-pass
 * in-register top-n are out of scope. */
#define DINT_GROUP_LIMIT_MAX 16 /* the largest per_group the group-limited calls take */
int dint_ranked_or_group_limit_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_facets* facets, uint32_t per_group, const dint_rank_cursor* after, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, uint64_t* kept, uint64_t* skipped, float* scores,
                                       uint32_t* docids, uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* hit_group_ranks,
                                       uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_group_limit_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_facets* facets, uint32_t per_group, const dint_rank_cursor* after, size_t n_queries,
                                        uint64_t* counts, uint64_t* matches, uint64_t* kept, uint64_t* skipped, float* scores,
                                        uint32_t* docids, uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* hit_group_ranks,
                                        uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);

/* ---- document values: ranked hits sorted by a per-document number, value-range filters ------------------------------
 * Adds: what a cursor engine computes with a field-sort collector in place of its top-k queue (ranked_or_query /
 * ranked_and_query, include/ds2i/queries.hpp:309-457, order by score only) — "the matches of this query, newest first" (or
 * cheapest first, or by any per-document number) — and the filter "only the documents whose value lies in [lo, hi]". A ranked
 * call with a large k, re-sorted by the caller, ends at DINT_RANKED_MAX_K and is wrong as soon as a query has more matches.
 * A values handle (dint_doc_values_create): values is a HOST array of num_docs words, one u32 per document, every 32-bit
 * value legal (signed, 64-bit or float columns: the caller maps them to order-preserving u32). The handle takes its device as
 * dint_doc_facets_create does and belongs to no query index. It keeps its own copy on the device, 4 BYTES PER DOCUMENT (values
 * may be released at once), is immutable and usable from several host threads at once. num_docs == 0 is legal. A document at
 * or past num_docs has value 0 wherever a value is read for sorting. DINT_ERR_ARG (no handle): num_docs > 0xFFFFFFFF, a null
 * out, a null array with num_docs > 0. dint_doc_values_info_get: num_docs as given.
 * dint_ranked_or_sorted_queries / dint_ranked_and_sorted_queries take the arguments of the filtered calls (filter nullable:
 * unrestricted), the column, order (DINT_SORT_DESC: larger value first; DINT_SORT_ASC) and after (HOST, nullable, n_queries
 * entries; set == 0: from the start). The matches are the filtered call's match set; the plan depends neither on the column,
 * nor on the order, nor on the cursor. The order is by value; EQUAL VALUES GO BY ASCENDING docID IN BOTH ORDERS. As a key,
 * sorted descending: K(d) = (order == ASC ? ~v(d) : v(d)) << 32 | (0xFFFFFFFF - d). A match lies AFTER a set cursor (cv, cd)
 * iff K(d) < (ASC ? ~cv : cv) << 32 | (0xFFFFFFFF - cd), compared as integers; the cursor need not be a match. The last hit
 * of one page, as (hit_value, docid), is the cursor of the next. The outputs (HOST):
 *   matches[q]       (nullable) every match, as the filtered call reports it: bit for bit
 *   skipped[q]       (nullable) the matches that are NOT after the cursor: the rank of the page's first hit
 *   counts[q]        min(k, matches[q] - skipped[q])
 *   docids, hit_values[q * k + i]  the i-th match after the cursor in the order above, and its value (hit_values nullable)
 *   scores[q * k + i]  (nullable) EXACTLY the BM25 score the filtered call gives that document
 *   past the count   0xFFFFFFFF, 0 and 0.0f
 *   *blocks_decoded  (nullable) the filtered call's value
 * What a page costs: the whole query, as a paged call's, and besides the filtered call's launches, per OR pass / per AND call,
 * one launch over the candidate slots that cuts at the cursor (only if some query has one), the selection's first stage with
 * one gathered word per live slot, and one launch over the slots behind the selection that finds the hits' scores (only if
 * scores are asked for). The cursor keys, flags, counters and hit scores are grow-only workspaces of the query index
 * (20 + 4 k bytes per query), sent and cleared once per call. Integer comparisons throughout: exact, the same from run to run.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse (scores may be null here, docids may
 * not), a null values or one on another device than the index, order > 1.
 * dint_doc_filter_create_from_values: the filter of the documents d < the column's num_docs with lo <= v(d) <= hi (closed;
 * lo > hi: the empty filter), built on the device — the bitmap never exists on the host. In its info and under every filtered
 * call it equals what dint_doc_filter_create makes of the same bitmap with num_docs the column's. DINT_ERR_ARG: a null qi,
 * values or out, a column on another device than the index.
 * Sorting the collapsed, faceted, boolean and pruned forms, several sort keys, an order per query, a value range combined
 * with a bitmap in one handle, backwards paging and narrower columns are out of scope. */
#define DINT_SORT_DESC 0u
#define DINT_SORT_ASC 1u
typedef struct dint_doc_values dint_doc_values;
typedef struct dint_doc_values_info {
    uint64_t num_docs; /* as given to dint_doc_values_create */
} dint_doc_values_info;
typedef struct dint_value_cursor {
    uint32_t value;
    uint32_t docid;
    uint32_t set; /* 0: from the start */
} dint_value_cursor;
int dint_doc_values_create(int device, const uint32_t* values, uint64_t num_docs, dint_doc_values** out);
int dint_doc_values_info_get(const dint_doc_values* v, dint_doc_values_info* info);
void dint_doc_values_destroy(dint_doc_values* v);
int dint_doc_filter_create_from_values(dint_query_index* qi, const dint_doc_values* values, uint32_t lo, uint32_t hi, dint_doc_filter** out);
int dint_ranked_or_sorted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                  const dint_doc_values* values, uint32_t order, const dint_value_cursor* after, size_t n_queries,
                                  uint64_t* counts, uint64_t* matches, uint64_t* skipped, uint32_t* hit_values, uint32_t* docids, float* scores,
                                  uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_sorted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                   const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                   const dint_doc_values* values, uint32_t order, const dint_value_cursor* after, size_t n_queries,
                                   uint64_t* counts, uint64_t* matches, uint64_t* skipped, uint32_t* hit_values, uint32_t* docids, float* scores,
                                   uint64_t* blocks_decoded, void* stream);

/* ---- value statistics and range histograms of the ranked queries (how the matches are distributed over a column) ----
 * Adds: what a cursor engine computes with a stats / range-aggregation collector beside its top-k collector (ranked_or_query /
 * ranked_and_query, include/ds2i/queries.hpp:309-457, have none) — per query the number, the sum, the minimum and the maximum
 * of a column's values over the query's matches and how many of them fall between caller-given bucket boundaries ("under 10,
 * 10-50, 50-200, above", a date histogram, the newest and the oldest match), for a batch of queries, in the call that ranks
 * them. Quantising the column into a facets map costs a 4-byte-per-document map per choice of boundaries and gives no min, max
 * or sum; aggregating fetched hits on the host is wrong as soon as a query has more than DINT_RANKED_MAX_K matches.
 * dint_ranked_or_value_stats_queries / dint_ranked_and_value_stats_queries take the arguments of the filtered calls (filter
 * nullable: unrestricted), the column (a dint_doc_values), edges (HOST, n_edges strictly ascending bucket boundaries;
 * n_edges == 0: no histogram, edges and bucket_counts are ignored and may be null) and the outputs (HOST):
 *   counts, matches, scores, docids, *blocks_decoded   bit for bit what dint_ranked_or_filtered_queries /
 *                    dint_ranked_and_filtered_queries return for the same arguments (filter null: the unfiltered answer with
 *                    the matches counted); the plan depends neither on the column nor on the edges; docids is nullable
 *   stats[q]         over EVERY match of query q that has a value, not over the top k. A match d HAS A VALUE iff d < the
 *                    column's num_docs, and the value is v(d); a match at or past the column has none and enters neither the
 *                    statistics nor any bucket — UNLIKE the sorted calls above, which give such a document the value 0 because
 *                    they must order it. So matches[q] - stats[q].n is the number of matches without a value. The sum is
 *                    64-bit and cannot overflow (fewer than 2^32 matches, each value below 2^32). An empty query, or one
 *                    without a valued match: {0, 0, 0xFFFFFFFF, 0}
 *   bucket_counts[q * (n_edges + 1) + b]  the valued matches of q in bucket b, bucket(v) = the number of edges e with e <= v:
 *                    bucket b holds edges[b - 1] <= v < edges[b], bucket 0 the values below edges[0], bucket n_edges the values
 *                    at or above the last edge. The row's sum equals stats[q].n
 *   hit_values[q * k + i]  (nullable) v(docids[q * k + i]) for i < counts[q] where that document has a value; 0 past the count
 *                    and for a hit at or past the column. Gathered on the device behind the selection; docids may be null
 *                    while hit_values is not
 * Every quantity is an integer sum, minimum or maximum: exact, order-independent and the same from run to run.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse; a null values or one on another
 * device than the index; a null stats; n_edges > DINT_VALUE_STATS_MAX_EDGES; n_edges > 0 with a null edges or bucket_counts;
 * edges that are not strictly ascending; n_queries * (n_edges + 1) > 2^28 (the caller batches). Terms, query_offsets, the
 * handle's lock and the stream are as for the filtered calls. The records (24 bytes per query, initialised to the empty
 * record), and the edges, the rows and the hit values (4 bytes * (n_edges + n_queries * (n_edges + 1 + k))) are grow-only
 * workspaces of the query index, sent and cleared once per call and copied back once. Besides the filtered call's launches a
 * call runs one launch over the candidate slots in front of the selection per OR pass / per AND call, which gathers one word
 * of the column per live slot and reduces in LDS — at most one global add per bucket present in a page and four atomics on the
 * query's record — and, if hit_values is given, one over the selected keys behind it.
 * Sums or means of scores (float sums are not order-independent), several columns per call and the boolean, pruned, collapsed
 * and paged forms are out of scope; statistics per facet group are the group-stats calls and exact percentiles
 * the percentile calls below. */
#define DINT_VALUE_STATS_MAX_EDGES 1023u
typedef struct dint_value_stats { /* 24 bytes: offsets 0, 8, 16, 20 */
    uint64_t n;   /* matches that have a value */
    uint64_t sum; /* the sum of their values   */
    uint32_t min; /* 0xFFFFFFFF if n == 0      */
    uint32_t max; /* 0 if n == 0               */
} dint_value_stats;
int dint_ranked_or_value_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* stats,
                                       uint32_t* bucket_counts, uint32_t* hit_values, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_value_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, size_t n_queries,
                                        uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* stats,
                                        uint32_t* bucket_counts, uint32_t* hit_values, uint64_t* blocks_decoded, void* stream);

/* ---- per-group value statistics of the ranked queries (facets x values: a column reduced per document group) --------
 * Adds: what a cursor engine computes with a stats collector nested under a terms collector — the average price per brand of
 * the results, the newest document per site, the revenue per tenant of what matched — for a batch of queries, in the call that
 * ranks them. Without it a caller runs one filtered value-stats call per group, each of which decodes and scores the query again.
 * dint_ranked_or_group_stats_queries / dint_ranked_and_group_stats_queries take the arguments of the filtered calls (filter
 * nullable: unrestricted), a facets map and a column (both belong to a device, neither to the index, and their num_docs need
 * not agree with each other or with the index) and the outputs (HOST):
 *   counts, matches, scores, docids, *blocks_decoded   bit for bit what dint_ranked_or_filtered_queries /
 *                    dint_ranked_and_filtered_queries return for the same arguments; the plan depends neither on the map nor on
 *                    the column; matches, docids and blocks_decoded are nullable
 *   group_stats[q * n_groups + g]   over EVERY match d of query q, not over the top k, that is in group g (d < the map's
 *                    num_docs and group_of[d] == g) and has a value (d < the column's num_docs): their number, the 64-bit sum of
 *                    their values, the minimum and the maximum. A match in no group contributes nowhere, and so does a match in
 *                    a group but at or past the column. A (query, group) without such a match: {0, 0, 0xFFFFFFFF, 0}
 *   facet_counts[q * n_groups + g]  (nullable) the faceted call's row, bit for bit: EVERY match of q in group g, valued or
 *                    not; so group_stats[..].n <= facet_counts[..], with equality where the column covers the index
 * Every quantity is an integer sum, minimum or maximum: exact, order-independent and the same from run to run.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse; a null facets, values or
 * group_stats; a map or a column on another device than the index; n_queries * n_groups > DINT_GROUP_STATS_MAX_RECORDS (384 MiB
 * of records: the caller batches). Terms, query_offsets, the handle's lock and the stream are as for the filtered calls. The
 * records are a grow-only workspace of the query index of their own (24 bytes per (query, group)), sent as the empty record
 * once per call and copied back once. Besides the filtered call's launches a call runs one launch over the candidate slots in
 * front of the selection per OR pass / per AND call, which gathers one word of the map and one of the column per live slot and
 * reduces runs of equal groups in registers and, up to 256 groups, the page's records in LDS — at most one set of four global
 * atomics per group present in a page — and, if facet_counts is given, the faceted call's launch.
 * The hits' groups and values (the collapsed and value-stats calls give them), bucket histograms per group, several columns per
 * call and sorting groups by a statistic are out of scope. */
#define DINT_GROUP_STATS_MAX_RECORDS (1ull << 24)
int dint_ranked_or_group_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_facets* facets, const dint_doc_values* values, size_t n_queries, uint64_t* counts,
                                       uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* group_stats,
                                       uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_group_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_facets* facets, const dint_doc_values* values, size_t n_queries, uint64_t* counts,
                                        uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* group_stats,
                                        uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream);

/* ---- exact percentiles of a column over the matches of the ranked queries (the median and the tail of what matched) ----
 * Adds: what a cursor engine computes with a percentiles collector beside its top-k collector — the median price of the
 * results, the p90 / p99 age of what matched — for a batch of queries, in the call that ranks them, EXACTLY: a histogram needs
 * its edges in advance and answers only to a bucket's width, and percentiles of fetched hits are wrong as soon as a query has
 * more than DINT_RANKED_MAX_K matches.
 * dint_ranked_or_percentile_queries / dint_ranked_and_percentile_queries take the arguments of the filtered calls (filter
 * nullable: unrestricted), the column (a dint_doc_values), per_million (HOST, n_percentiles ranks in parts per million, each
 * <= 1000000, in any order, repeats allowed) and the outputs (HOST):
 *   counts, matches, scores, docids, *blocks_decoded   bit for bit what dint_ranked_or_filtered_queries /
 *                    dint_ranked_and_filtered_queries return for the same arguments (filter null: the unfiltered answer with
 *                    the matches counted); the plan depends neither on the column nor on the percentiles; matches, docids and
 *                    blocks_decoded are nullable
 *   value_counts[q]  n_q, the matches of query q that have a value, over EVERY match, not over the top k. As for the
 *                    value-stats calls a match d HAS A VALUE iff d < the column's num_docs
 *   percentile_values[q * n_percentiles + j] = s[((n_q - 1) * per_million[j]) / 1000000], s the ascending sort of those n_q
 *                    values, duplicates kept, the division a 64-bit integer division that rounds down (the "lower" nearest
 *                    rank: no interpolation, the answer is always a value of the column); 0 if n_q == 0. per_million 0 gives
 *                    the minimum, 1000000 the maximum, 500000 the lower median
 *   stats[q]         (nullable) exactly what the value-stats call with n_edges == 0 writes: {n, sum, min, max}, the empty record
 *                    {0, 0, 0xFFFFFFFF, 0}. Null: nothing of the value-stats machinery is launched
 * Every quantity is an integer count or a value of the column: exact, order-independent and the same from run to run.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse; a null values or one on another
 * device than the index; a filter of another index; a null per_million, value_counts or percentile_values; n_percentiles == 0
 * or > DINT_PERCENTILES_MAX; a per_million[j] > 1000000; n_queries * n_percentiles > DINT_PERCENTILES_MAX_RECORDS (a counter row
 * is 1 KiB: 64 MiB of rows; the caller batches). Terms, query_offsets, the handle's lock and the stream are as for the filtered
 * calls. The rows (1 KiB per (query, percentile)) and the select's words (4 bytes * (n_percentiles + n_queries * (3 *
 * n_percentiles + 1))) are grow-only workspaces of the query index. Besides the filtered call's launches a call runs, per OR
 * pass / per AND call and in front of the selection, an MSB-first radix select of four rounds over the candidate slots: per
 * round one launch that gathers one word of the column per live slot and counts a byte of it in LDS, and one of a wave per
 * (query, percentile) that scans the 256 counters and fixes that byte of the answer. A round reads the round before it from
 * device memory; nothing returns to the host in between.
 * Interpolated percentiles, percentiles per facet group, the rank of a given value and the boolean, pruned, collapsed and paged
 * forms are out of scope. */
#define DINT_PERCENTILES_MAX 16u
#define DINT_PERCENTILES_MAX_RECORDS (1ull << 16)
int dint_ranked_or_percentile_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles, size_t n_queries,
                                      uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* value_counts,
                                      uint32_t* percentile_values, dint_value_stats* stats, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_percentile_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* value_counts,
                                       uint32_t* percentile_values, dint_value_stats* stats, uint64_t* blocks_decoded, void* stream);

/* ---- the most frequent values of a column over the matches of the ranked queries, and how many different ones there are ----
 * Adds: what a cursor engine computes with a terms collector and a cardinality collector beside its top-k collector — the top
 * 10 authors, hosts or prices of the results, the number of distinct sellers — for a batch of queries, in the call that ranks
 * them, EXACTLY. Facet counts need the column mapped to at most DINT_FACETS_MAX_GROUPS dense group ids in advance and return a
 * row of n_groups counters per query; a column is an arbitrary u32 per document and may have as many values as documents.
 * dint_ranked_or_top_values_queries / dint_ranked_and_top_values_queries take the arguments of the filtered calls (filter
 * nullable: unrestricted), the column (a dint_doc_values), n_top (0 .. DINT_TOP_VALUES_MAX) and the outputs (HOST):
 *   counts, matches, scores, docids, *blocks_decoded   bit for bit what dint_ranked_or_filtered_queries /
 *                    dint_ranked_and_filtered_queries return for the same arguments (filter null: the unfiltered answer with
 *                    the matches counted); the plan depends neither on the column nor on n_top; matches, docids and
 *                    blocks_decoded are nullable
 *   value_counts[q]  the matches of query q that have a value, over EVERY match, not over the top k: the number the
 *                    percentile and value-stats calls report. A match d HAS A VALUE iff d < the column's num_docs
 *   distinct_counts[q]  the number of different values among them
 *   top_n[q]         min(n_top, distinct_counts[q])
 *   top_values[q * n_top + i], top_counts[q * n_top + i], i < top_n[q]: the values in the order COUNT DESCENDING, THEN VALUE
 *                    ASCENDING, and how many valued matches have each; 0 past top_n[q]. n_top == 0 asks for the counts only:
 *                    top_values and top_counts may then be null, and no selection is launched
 * Every quantity is an integer count: exact, order-independent, the same from run to run and equal to a sort-and-count on the
 * host.
 * DINT_ERR_ARG, before anything is written or launched: whatever the filtered calls refuse; a null values or one on another
 * device than the index; a filter of another index; n_top > DINT_TOP_VALUES_MAX; a null value_counts, distinct_counts or top_n;
 * a null top_values or top_counts with n_top > 0. Terms, query_offsets, the handle's lock and the stream are as for the
 * filtered calls. Besides the filtered call's launches a call runs, per OR pass / per AND call and in front of the selection:
 * a clear of the pass's hash tables — per query 16 bytes per candidate slot, 64-bit words `value << 32 | count` at a load of
 * at most 1/2 —, one launch that gathers one word of the column per live slot, merges equal values in a page-local LDS table
 * and inserts each of the page's distinct values into its query's table once, and — n_top > 0 — a selection over the tables
 * in the ranked selection's manner (runs sorted, merged pairwise) with workspaces of its own. The tables, the selection's
 * tasks and keys, the counters (8 bytes a query) and the selected keys (8 bytes * n_queries * n_top) are grow-only workspaces of
 * the query index; everything returns once, in front of the call's last wait. Every probe sequence
 * on the device is bounded by its table's capacity; a table that ran full all the same — a mistake of the library's, never of
 * the caller's — ends the call with DINT_ERR_NOMEM behind its last wait.
 * Approximate sketches, top values per facet group, strings (the caller maps them to u32, as for every column), merging top
 * lists across shards and the boolean, pruned, collapsed and paged forms are out of scope. */
#define DINT_TOP_VALUES_MAX 1024u /* = DINT_RANKED_MAX_K */
int dint_ranked_or_top_values_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_values* values, uint32_t n_top, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                      float* scores, uint32_t* docids, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n,
                                      uint32_t* top_values, uint32_t* top_counts, uint64_t* blocks_decoded, void* stream);
int dint_ranked_and_top_values_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, uint32_t n_top, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                       float* scores, uint32_t* docids, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n,
                                       uint32_t* top_values, uint32_t* top_counts, uint64_t* blocks_decoded, void* stream);

/* ---- the wand data's BM25 maxima from the index, on the device; block maxima for the pruned call --------------
 * Replaces: the max_term_weight half of wand_data's constructor (include/ds2i/wand_data.hpp:18-57, src/create_wand_data.cpp),
 * which walks the uncompressed collection posting by posting, by one decode of the INDEX: a caller that has only what this
 * library serves from (the index and the document sizes, for norm_lens) can build the maxima.
 * block_max_weight[b] (HOST, nullable: not wanted; one per block of the block table the query index was created from, in
 * that table's order) = the largest f / (f + k1 * ((1 - b) + b * norm_lens[d])) over the postings (d, f) of block b, every
 * operation a binary32 one, uncontracted: the expression of the scoring kernels without the query weight, and of
 * dinth_wand_data. max_term_weight[t] (HOST, n_lists of the query index) = the largest block_max_weight over list t's
 * blocks, 0.0f for a list without a block. Every maximum starts at 0.0f and takes a value only if it is larger, as the
 * host's std::max(max, score) does: a NaN (a norm_len of 0 under a freq that wrapped to 0), a negative value or -0.0f never
 * enters it. A maximum of binary32 values does not depend on the order they are taken in, so max_term_weight equals
 * dinth_wand_data's array bit for bit (include/dint_host.h; wd's norm_lens being that call's).
 * Every block's docs and freqs parts are decoded once, in passes of consecutive blocks of at most
 * DINT_OPT_QUERY_OR_PASS_PAGES pages (a list may span passes), into the query index's workspaces, under the handle's lock
 * like the query calls; the results come back in one copy and the call returns after synchronising `stream`.
 * DINT_ERR_ARG, before anything is launched: a null handle, a null max_term_weight with n_lists != 0, a freqs_dict of another
 * kind or device than the docs dictionary, a wand handle on another device or one whose num_docs does not exceed the index's
 * largest docID. An index of zero blocks returns DINT_OK and writes zeros. */
int dint_index_max_weights(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, float* max_term_weight,
                           float* block_max_weight, void* stream);

/* Gives a wand handle block maxima (HOST, n_blocks floats: dint_index_max_weights' block_max_weight for the query index the
 * handle will be used with): a device copy on the handle's device, owned by the handle; calling it again replaces the copy.
 * A NaN or negative value is DINT_ERR_ARG, checked before the device is touched, and the handle is left as it was; -0.0f,
 * +inf and FLT_MAX are accepted (the rule of dint_wand_data_create_with_max_weights). NOT thread-safe against calls running
 * on the same handle: set the maxima before the handle is shared.
 * With block maxima dint_ranked_or_maxscore_queries bounds the non-essential terms per candidate: the sum of their term
 * maxima gives way to the candidate's own sum — from 0.0 in double over those terms in ascending term id, (double) of the
 * binary32 product q_weight_t * block_max_weight[the first block of t whose last docID is >= the candidate], nothing for a
 * term whose list ends before the candidate — wherever that sum is the smaller of the two (it is, for block maxima no
 * larger than their list's max_term_weight); the comparison, its margin, the seed, theta, the split by TERM maxima, the
 * claims, the scores and the selection are unchanged. A handle whose n_blocks differs from the query index's block
 * count is DINT_ERR_ARG there, before anything is launched; a handle without block maxima behaves as it always did.
 * SAFETY ASSUMPTION, beside the one on max_term_weight: block_max_weight[b] >= the doc_term_weight of every posting of
 * block b. Then the call still returns dint_ranked_or_queries' answer bit for bit, and *blocks_read can only fall: any
 * larger block maxima give the same answer, and +inf reads exactly the blocks the handle read without block maxima. Smaller block maxima do what smaller term maxima do: documents may
 * be missing, never wrong (every returned pair is a document of the union with its exact score, in order). */
int dint_wand_data_set_block_max_weights(dint_wand_data* wd, const float* block_max_weight, size_t n_blocks);

/* ---- an index checked against its collection, on the device ------------------------------------------------------
 * Replaces: verify_collection (include/ds2i/verify_collection.hpp:7-52), the walk behind `create_freq_index --check` and
 * the check_index tool (src/check_index.cpp): every list of the collection beside the index's enumerator, stopping at the
 * first wrong length, docID or freq. Here the whole index is compared and the mismatches are counted; the one the
 * reference would have stopped at is reported.
 * view (HOST): the collection as its files hold it, nothing copied: list i is docs[docs_at[i] .. + list_len[i]) and, with
 * freqs, freqs[freqs_at[i] .. + list_len[i]).
 * Lengths are compared on the host (:18-24): list i's length in the query index against view->list_len[i]. A list of wrong
 * length counts as ONE mismatch and none of its postings is compared. Of every other list each posting is compared with
 * the decoded docID (:30-37) and, when view->freqs and freqs_dict are given, with the decoded freq() (:39-46); pass both or
 * neither. A posting whose docID or freq (or both) differs counts once. *n_mismatches = wrong lengths + wrong postings.
 * *first (nullable) = the mismatch the reference would have stopped at: the lowest list; within it LENGTH before any
 * posting, otherwise the lowest position; at that position DOCID before FREQ. `expected` is the collection's value (LENGTH:
 * its length), `got` the index's; position is 0 for LENGTH. No mismatch: kind DINT_CHECK_OK, every other field 0.
 * Both outputs are a function of (index, view) alone: a sum and a minimum over the postings, independent of the pass size,
 * the order of the passes and the timing of the atomics that form them. `got` is read from that one block decoded again.
 * DINT_OK whether or not there are mismatches: a mismatch is a result, not an error.
 * Every block is decoded once, in dint_index_max_weights' passes (consecutive blocks, at most DINT_OPT_QUERY_OR_PASS_PAGES
 * pages and at most 16384), under the handle's lock; the collection's postings of a pass are staged through two pinned
 * buffers of the handle (32.25 MiB each at most) by a copy stream of the call's own, beside the pass before it. The call
 * returns after synchronising `stream`.
 * DINT_ERR_ARG, before anything is launched: a null qi, view or n_mismatches; view->n_lists different from the index's list
 * count; null docs / docs_at / list_len (freqs_at with freqs) when n_lists != 0; freqs without freqs_dict or freqs_dict
 * without freqs; a freqs_dict of another kind or device than the docs dictionary; a query index created from a block table
 * in which a block that is not its list's last holds fewer than 256 postings (not the in-index layout: block j of a list
 * would not be its positions [256 j, 256 j + n)). An index of zero blocks returns DINT_OK with the length comparisons only. */
#define DINT_CHECK_OK 0
#define DINT_CHECK_LENGTH 1 /* verify_collection.hpp:18-24 */
#define DINT_CHECK_DOCID 2  /* :30-37 */
#define DINT_CHECK_FREQ 3   /* :39-46 */

typedef struct dint_collection_view {
    const uint32_t* docs;     /* words of the .docs file (or any array)                */
    const uint32_t* freqs;    /* words of the .freqs file; null: docIDs only           */
    const uint64_t* docs_at;  /* [n_lists] word offset in docs of list i's first docID */
    const uint64_t* freqs_at; /* [n_lists] word offset in freqs of list i's first freq */
    const uint64_t* list_len; /* [n_lists] postings of list i                          */
    size_t n_lists;
} dint_collection_view;

typedef struct dint_index_mismatch {
    uint32_t kind;     /* DINT_CHECK_* */
    uint32_t list;
    uint64_t position; /* within the list; 0 for LENGTH */
    uint64_t expected; /* the collection's value (LENGTH: its length) */
    uint64_t got;      /* the index's */
} dint_index_mismatch;

int dint_check_index(dint_query_index* qi, const dint_dict* freqs_dict, const dint_collection_view* view, uint64_t* n_mismatches,
                     dint_index_mismatch* first, void* stream);

/* ---- BM25 scores and term frequencies of caller-given documents over the same query index -----------
 * Replaces: the cursor primitive under every query, document_enumerator::next_geq(d) then freq()
 * (include/dint/dict_posting_list.hpp:126-169), with ranked_or_query's sums (include/ds2i/queries.hpp:387-457), for a batch
 * of (query, document set) pairs per call: "is document d in list t, with what frequency, and what does d score?".
 * terms / query_offsets are as in every query call (repeated terms give qf; an empty query is legal). Query q's documents
 * are docids[doc_offsets[q] .. doc_offsets[q + 1]) (HOST; doc_offsets has n_queries + 1 entries, non-decreasing): in any
 * order, repeated or not, any u32 — a docID above the index's largest, 0xFFFFFFFF included, is in no list.
 * scores (HOST, laid out like docids: scores[i] belongs to docids[i]): dint_ranked_or_queries' score of that document for
 * that query, bit for bit — from 0.0f, for each distinct term in ascending term id whose list holds d,
 * score = score + q_weight_t * doc_term_weight(freq_t(d), norm_lens[d]), binary32, uncontracted. A
 * document in none of the query's lists scores 0.0f; norm_lens[d] is read only after a hit, so the wand handle need only
 * cover the index's largest docID, as for the ranked calls (one created without max_term_weight will do).
 * freqs (HOST, nullable: not wanted): for query q with T_q distinct terms, a row-major matrix [documents of q][T_q], the
 * terms in ascending term id, 0 for "not in the list", otherwise freq(); the queries' matrices back to back in query order.
 * *blocks_read (nullable) = the sum over the queries of the distinct (term, block) pairs whose docs and freqs parts the call
 * decoded: a document claims, in each term of its query, the first block whose last docID is >= it, if there is one. No
 * other block is read. The call runs in passes of whole queries of at most DINT_OPT_QUERY_OR_PASS_PAGES pages of the bound
 * sum_t min(blocks of t, documents of q) (a larger query alone); a query without documents launches nothing. The handle's
 * lock and the stream are as for dint_and_queries. DINT_ERR_ARG, before any device is touched: a null handle, null scores,
 * null offsets with n_queries != 0, decreasing doc_offsets, more than 2^30 documents for one query, null docids with a
 * document to score; then, before anything is launched: a freqs_dict of another kind or device than the docs dictionary, a
 * wand handle on another device or one whose num_docs does not exceed the index's largest docID, decreasing
 * query_offsets, a term >= n_lists. */
int dint_score_documents(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, const uint32_t* terms,
                         const uint64_t* query_offsets, size_t n_queries, const uint32_t* docids, const uint64_t* doc_offsets,
                         float* scores, uint32_t* freqs, uint64_t* blocks_read, void* stream);

/* ---- block statistics on the device (dictionary construction, counting half) ----------------------------
 * Counts every aligned 16/8/4/2/1-gram of the given lists — multi != 0: of their whole 256-integer blocks, per block
 * context — keyed by the MurmurHash64A of its integers, as the reference's collectors do.
 * Replaces: adjusted::collect, include/dint/statistics_collectors.hpp:90-118 (context: :21-40), the per-thread
 * maps of block_statistics.hpp:82-106. The selection (filter, sort, DSF, packing: dictionary_builders.hpp:40-76) stays
 * on the host: dinth_build_dictionary_from_ngrams (include/dint_host.h) takes these entries.
 * d_gaps: device, n_ints u32 (d-gaps minus one, lists back to back); list_starts: host, n_lists + 1 offsets into d_gaps.
 * *entries (malloc'ed, release with dint_free): one per distinct (context, n-gram) — position of its first
 * occurrence in d_gaps, length, context, number of occurrences — in no particular order (see top_k below). */
typedef struct dint_ngram {
    uint64_t pos;
    uint32_t freq;
    uint8_t len;
    uint8_t ctx;
    uint16_t pad;
} dint_ngram;
int dint_count_ngrams(int device, int multi, const uint32_t* d_gaps, uint64_t n_ints, const uint64_t* list_starts,
                      uint64_t n_lists, uint32_t top_k, dint_ngram** entries, size_t* n_entries, float* kernel_ms);
/* top_k = 0: every distinct n-gram. top_k > 0 (65536 for DSF-65536-16): only those that can be among the first top_k
 * of their context in the selection's order (occurrences first) — per context the entries whose count reaches the
 * top_k-th largest count among the n-grams the reference's filter keeps (dictionary_builders.hpp:15-38), ties
 * included: the dictionary built from them is the same, the host sorts tens of thousands of entries instead of
 * tens of millions. The filter's total is the sum of the lists' lengths (in the multi flavour the integers past a
 * list's last whole block count too). A context with fewer than top_k kept n-grams comes back whole; entries the
 * filter drops come back as well where their count reaches their context's threshold (the selection drops them);
 * and when there are no more than top_k distinct n-grams in all, every one comes back.
 * DINT_ERR_ARG (*entries = NULL, *n_entries = 0): entries or n_entries NULL, list_starts not ascending or past n_ints.
 * No list, or no list with a chunk to count: DINT_OK with *entries = NULL and *n_entries = 0. */

/* The selection half on the device too: of `entries` (dint_count_ngrams' output; in place), the n-grams the reference's
 * filter keeps (dictionary_builders.hpp:15-38), every context's in dictionary order — most frequent first, then the
 * longer, then by their integers (block_statistics.hpp:246-276 freq_length sorter; ties made deterministic) — and of
 * those the first top_k (decreasing_static_frequencies::build, dictionary_builders.hpp:55-75: 65536). A filter kernel, one
 * rocPRIM merge sort whose comparator reads the integers in d_gaps, one scatter. *n_selected entries come back; the
 * host only packs them (dinth_pack_dictionary, include/dint_host.h).
 * The filter: count * (48 * len - 16) / total_ints > 0.0001 / 1000 in double (one ulp above the literal 1e-7: a saving
 * equal to the quotient is dropped), or len == 1; total_ints is the caller's claim and is not checked against d_gaps. The
 * integers compare as unsigned. The counts are the caller's too: any value is taken.
 * DINT_ERR_ARG, with `entries` untouched: top_k == 0, n_selected NULL, an entry with len 0 or above 16, ctx >= 8, or
 * integers that do not lie inside d_gaps (pos + len > n_ints). */
int dint_select_ngrams(int device, const uint32_t* d_gaps, uint64_t n_ints, uint64_t total_ints, dint_ngram* entries,
                       size_t n_entries, uint32_t top_k, size_t* n_selected);

/* Device time (ms) between the two events the library records around the decode kernel of the most
 * recent dint_decode_units on this dictionary (one event pair per in-flight launch: launches on
 * different streams do not disturb each other's); synchronises that launch. */
int dint_last_kernel_ms(const dint_dict* dict, float* ms);

/* The same for the most recent launches, oldest first: up to max_n of the last 64 (the library keeps
 * that many event pairs); *n = how many were written. Synchronises them. What bench.py reports its
 * per-launch kernel time from: the events of the timed launches themselves. */
int dint_recent_kernel_ms(const dint_dict* dict, float* ms, size_t max_n, size_t* n);
/* The shader clock the most recent decode kernel ran at, MHz: cycles counted by the launch's first wavefront
 * (s_memtime at both ends) over the kernel's duration from its event pair. (Boxes of a pool differ.) The count is read from
 * where that launch's counters live — a block table's launches keep theirs in the table: call while it exists — and is 0 for a
 * launch that recorded none (the small launch behind an in-index decode for the blocks that fit no tile). */
int dint_last_kernel_clock_mhz(const dint_dict* dict, float* mhz);

/* What a vroom stream is made of, by the dictionary's device layout (host pre-pass, like
 * dint_index_stream): codewords, exceptions, how many codewords find their integers on chip. */
typedef struct dint_stream_stats {
    uint64_t lists, ints, payload_bytes;
    uint64_t codewords;        /* dictionary codewords (runs included), exceptions not */
    uint64_t run_codewords;
    uint64_t exceptions16, exceptions32;
    uint64_t hot_codewords;    /* dictionary codewords whose integers are in the LDS image (runs included) */
    uint64_t hot_ints;         /* integers they decode to */
    uint64_t wide_blocks;      /* multi: blocks of 16-bit slots; narrow_blocks: of 8-bit slots */
    uint64_t narrow_blocks;
} dint_stream_stats;
int dint_stream_stats_get(const dint_dict* dict, const uint8_t* enc, size_t enc_bytes, dint_stream_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* DINT_HIP_H */
