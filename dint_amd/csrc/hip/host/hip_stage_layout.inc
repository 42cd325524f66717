// Part of dint_hip.hip (one translation unit; included from there, in order): the staged input areas of the query calls and the decode launch's two schedule workspaces, each laid out ONCE.
// Plain C++, no HIP call and no allocation (tests/test_stage_layout.py compiles this file alone). A call stages what its
// kernels read from the host in dint_query_index::h_stage and sends it to ::inputs in one copy: a layout takes the area's
// fields in order and records each one's word offset; the host fills the field at h(at), the kernel's argument struct
// gets d(at) (hip_query_handle.inc) — one offset, both addresses.
struct stage_layout {
    size_t words = 0;  // the total so far
    // the next field: n words, at a multiple of `align` words (2: the field holds 8-byte values)
    size_t take(size_t n, size_t align = 1) {
        words = (words + align - 1) / align * align;
        words += n;
        return words - n;
    }
    // ... and a run of fields of n words each, in order
    void take_each(std::initializer_list<size_t*> fields, size_t n) {
        for (size_t* f : fields) *f = take(n);
    }
};
// the field at word `at` of an area that begins at `base`
template <class T = uint32_t>
static inline T* staged(void* base, size_t at) {
    return reinterpret_cast<T*>(static_cast<uint32_t*>(base) + at);
}

// The AND forms' tables: page -> block, page -> query, then per round and query the first block and the block count of
// the round's list (n_tab = max(1, rounds * n_queries) each).
struct and_tables_layout : stage_layout {
    size_t page_block, page_query, term_first, term_blocks;
    and_tables_layout(size_t n_pages, size_t n_tab) {
        take_each({&page_block, &page_query}, n_pages);
        take_each({&term_first, &term_blocks}, n_tab);
    }
};
// The workgroup-per-query batch form: the tables; the result counters (u64 each; zeros, copied in with the tables); per
// active query {query, first page, pages, steps}, then per active query {probe page, control word}.
struct and_batch_layout : and_tables_layout {
    size_t counts, qrec, qrec2;
    and_batch_layout(size_t n_pages, size_t n_tab, size_t n_queries, size_t n_active) : and_tables_layout(n_pages, n_tab) {
        counts = take(2 * n_queries, 4);
        qrec = take(4 * n_active, 4);
        qrec2 = take(2 * n_active);
    }
};
// The general form: the tables and behind them — zeros, copied in with them: one copy instead of a copy and a clear —
// every counter the call's launches count in (ctrl_words for the candidates and for every round) and the result counters
// (u64 each); then the one-launch form's steps, 8-byte aligned (step_bytes = sizeof(fused_step)).
struct and_general_layout : and_tables_layout {
    size_t ctrl, counts, steps;
    and_general_layout(size_t n_pages, size_t n_tab, size_t n_queries, size_t rounds, size_t ctrl_words, size_t step_bytes)
        : and_tables_layout(n_pages, n_tab) {
        ctrl = take((rounds + 1) * ctrl_words, 32);
        counts = take(2 * n_queries);  // (ctrl_words is even: 8-byte aligned)
        steps = take((rounds + 1) * ((step_bytes + 7) / 8 * 2), 2);
    }
};
// The general form with a ranked boolean call's extra steps behind it (with none of them: and_general_layout itself, word
// for word): per excluded step and query {first block, blocks} (n_not_tab = steps * n_queries each), per optional step and
// query {first block, blocks, q_weight}, then a claim counter per step (zeros, copied in with the rest).
struct and_bool_layout : and_general_layout {
    size_t not_first, not_blocks, should_first, should_blocks, should_weight, step_count;
    and_bool_layout(size_t n_pages, size_t n_tab, size_t n_queries, size_t rounds, size_t ctrl_words, size_t step_bytes, size_t n_not_tab,
                    size_t n_should_tab, size_t n_steps)
        : and_general_layout(n_pages, n_tab, n_queries, rounds, ctrl_words, step_bytes) {
        take_each({&not_first, &not_blocks}, n_not_tab);
        take_each({&should_first, &should_blocks, &should_weight}, n_should_tab);
        step_count = take(n_steps);
    }
};
// An OR pass (and the pruned ranked call's seeds): page -> block, page -> term record, then per term record {first
// block, blocks, first page, query, from} and, ranked, {the records of its query by term id, its query's terms, q_weight}.
struct or_pass_layout : stage_layout {
    size_t page_block, page_term, term_first, term_blocks, term_page, term_query, term_from, term_order = 0, term_n = 0, term_weight = 0;
    or_pass_layout(size_t n_pages, size_t n_terms, bool ranked) {
        take_each({&page_block, &page_term}, n_pages);
        take_each({&term_first, &term_blocks, &term_page, &term_query, &term_from}, n_terms);
        if (ranked) take_each({&term_order, &term_n, &term_weight}, n_terms);
    }
};
// What a ranked OR pass with a minimum and exclusions (dint_ranked_or_bool_queries) stages besides, from word `base` on —
// behind the pass's or_pass_layout, which keeps its words: page -> query of the pass, per term record its query's m, per
// excluded step and query of the pass {first block, blocks} (n_not_tab = steps * queries each), then a claim counter per
// step (zeros, copied in with the rest).
struct or_bool_layout : stage_layout {
    size_t page_query, term_m, not_first, not_blocks, step_count;
    or_bool_layout(size_t base, size_t n_pages, size_t n_terms, size_t n_not_tab, size_t n_steps) {
        words = base;
        page_query = take(n_pages);
        term_m = take(n_terms);
        take_each({&not_first, &not_blocks}, n_not_tab);
        step_count = take(n_steps);
    }
};
// What a ranged ranked OR pass (dint_ranked_or_range_queries) stages besides, from word `base` on — behind the pass's
// or_pass_layout, which keeps its words: per term record its query's range {lo, hi}.
struct or_range_layout : stage_layout {
    size_t term_lo, term_hi;
    or_range_layout(size_t base, size_t n_terms) {
        words = base;
        take_each({&term_lo, &term_hi}, n_terms);
    }
};
// What a faceted ranked OR pass (dint_ranked_or_faceted_queries) stages besides, from word `base` on — behind the pass's
// other layouts, which keep their words: page -> query of the pass (facet_count_kernel's; the selection has the host's copy).
struct or_facet_layout : stage_layout {
    size_t page_query;
    or_facet_layout(size_t base, size_t n_pages) {
        words = base;
        page_query = take(n_pages);
    }
};
// The pruned ranked call's main stage: per record {first, blocks, page, claimed, q_weight, order, E, query}, per query
// {from, n, n_E, theta}, per candidate page {page, record}, the other E terms' blocks, then (8-byte aligned) per query
// {rest, margin} (doubles).
struct maxscore_layout : stage_layout {
    size_t term_first, term_blocks, term_page, term_claimed, term_weight, term_order, term_e, rec_query;
    size_t q_from, q_n, q_ne, q_theta, cpage_page, cpage_rec, rest_blocks, q_rest, q_margin;
    maxscore_layout(size_t n_rec, size_t nq, size_t n_cpages, size_t n_rest) {
        take_each({&term_first, &term_blocks, &term_page, &term_claimed, &term_weight, &term_order, &term_e, &rec_query}, n_rec);
        take_each({&q_from, &q_n, &q_ne, &q_theta}, nq);
        take_each({&cpage_page, &cpage_rec}, n_cpages);
        rest_blocks = take(n_rest);
        q_rest = take(2 * nq, 2);
        q_margin = take(2 * nq);
    }
};
// A pass of dint_score_documents: per record {first, blocks, flag, q_weight, order}, per query {from, n}, per document
// {query, docID}, then (8-byte aligned, u64) per query where its freqs matrix begins.
struct score_documents_layout : stage_layout {
    size_t term_first, term_blocks, term_flag, term_weight, term_order, q_from, q_n, doc_query, doc_id, q_freq_at;
    score_documents_layout(size_t n_rec, size_t nq, size_t n_docs) {
        take_each({&term_first, &term_blocks, &term_flag, &term_weight, &term_order}, n_rec);
        take_each({&q_from, &q_n}, nq);
        take_each({&doc_query, &doc_id}, n_docs);
        q_freq_at = take(2 * nq, 2);
    }
};
// ranked_topk: the tasks (3 words each), per query {first page, pages}, then (8-byte aligned, u64) the key bases.
struct topk_layout : stage_layout {
    size_t tasks, page_first, pages, key_base;
    topk_layout(size_t n_tasks, size_t nq) {
        tasks = take(3 * n_tasks);
        take_each({&page_first, &pages}, nq);
        key_base = take(2 * nq, 2);
    }
};

// ---- the two schedule workspaces of a decode launch (hip_api_vroom.inc), as byte offsets into one allocation -----------------
// (what the kernels size them by comes in as arguments — chunk_units: kChunkUnits, kernels/bundles.inc; counter_bytes: a
// launch's kQueueLines counter lines of kQueueStride words, dint_kernels.hpp — so that this file still compiles alone)
template <class T>
static inline T* at_byte(void* base, size_t off) {
    return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off);
}
// A bundle schedule of n units (sched_cache::d_mem, dint_dict::d_sched): per unit a 16-byte record, per chunk of chunk_units
// units a 16-byte base, per unit its work item (u32), per 256 units their count / offset (u32), the number of work items
// (u32), then per unit the schedule byte and the item count byte.
struct sched_layout {
    size_t n_units, n_blocks, n_chunks;
    size_t urec = 0, cbase, items, block, n_items, sch, item_cnt, need;
    sched_layout(size_t n, size_t chunk_units) : n_units(n), n_blocks((n + 255) / 256), n_chunks((n + chunk_units - 1) / chunk_units) {
        cbase = urec + 16 * n_units;
        items = cbase + 16 * n_chunks;
        block = items + 4 * n_units;
        n_items = block + 4 * n_blocks;
        sch = n_items + 4;
        item_cnt = sch + n_units;
        need = item_cnt + n_units;
    }
};
// The cut units of a kept schedule (sched_cache::d_split) that left `items` units to the queue: two 16-byte records each,
// their chunks' bases, two end offsets each (u64), the units that could not be cut (u32), a 256-byte line — their number,
// and 8 bytes on the clock word of the cut units' launch — then a launch's counter lines.
struct split_layout {
    size_t n_items, n_sub, n_chunks;
    size_t urec = 0, cbase, end, left, n_left, clock, counters, need;
    split_layout(size_t items, size_t chunk_units, size_t counter_bytes)
        : n_items(items), n_sub(2 * items), n_chunks((2 * items + chunk_units - 1) / chunk_units) {
        cbase = urec + 16 * n_sub;
        end = cbase + 16 * n_chunks;
        left = end + 8 * n_sub;
        n_left = left + 4 * n_items;
        clock = n_left + 8;
        counters = n_left + 256;
        need = counters + counter_bytes;
    }
};
