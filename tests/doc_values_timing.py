#!/usr/bin/env python3
"""Sorted ranked query timing: dint_ranked_or_sorted_queries and dint_ranked_and_sorted_queries at k = 10
without a filter, descending, under a random, a clustered (the value follows the docID in runs of 4 096) and a constant
column, with every query's cursor from the start and at rank 10 000 — the cursors taken from a first walk (pages of 1 000: the
last hit of the tenth) — each workload as one batch, beside the FILTERED entry on a null filter (the same plan and scoring
launches, the selection by score) in the same process: the baseline, timed in alternation with the sorted rows so that all see
the same clocks, and its round-to-round spread reported as the noise the rows are to be read against. µs per query per row and
each row's ratio to the baseline's median; the sorted answer's matches and blocks_decoded are checked against the filtered
entry's and skipped against the cursor's rank. Also dint_doc_filter_create_from_values against dint_doc_filter_create of the
same bitmap (the host's packing of the mask timed with the latter: it is what the device kernel replaces), ms per creation.

    python tests/doc_values_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/sorted_queries_1e8.json]

A query with fewer matches than the rank has no hit there: its cursor is its last hit, and nothing lies behind it. Lives under
tests/ because it uses the test helpers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

RANK = 10000
WALK_K = 1000  # the first walk's page


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    n_lists = len(coll.lens)
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    workloads = {
        "reference_log_mod_lists": reference_queries(n_lists),
        "longest_lists": heavy_queries(coll.lens, 500, pool=256, max_terms=5),
    }
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)
    rng = np.random.default_rng(4)
    columns = {"random": rng.integers(0, 1 << 32, num_docs, dtype=np.uint32), "clustered": np.arange(num_docs, dtype=np.uint32) >> 12,
               "constant": np.full(num_docs, 7, dtype=np.uint32)}
    handles = {name: device.DocValues(0, v) for name, v in columns.items()}

    def timed(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0), out

    def us(t, n):
        return {"min": min(t) * 1e6 / n, "median": float(np.median(t)) * 1e6 / n, "max": max(t) * 1e6 / n}

    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "rank": RANK}
    entries = {"or": (qi.ranked_or_sorted_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_sorted_queries, qi.ranked_and_filtered_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs)}
        for entry, (sorted_call, filtered) in entries.items():
            want = filtered(fdd, wand, qs, None, k=10, with_stats=True)  # (warm-up, and the answer)
            rows = {}
            for cname, col in handles.items():
                # the first walk: every query's last hit of the page that ends at the rank (or its last hit before)
                last, seen = [None] * len(qs), np.zeros(len(qs), dtype=np.uint64)
                for ids, counts, hv, docs, _, _ in qi.ranked_pages(entry + "_sorted", fdd, wand, qs, k=WALK_K, values=col, max_pages=RANK // WALK_K):
                    for j, i in enumerate(ids.tolist()):
                        if counts[j]:
                            last[i] = (int(hv[j, int(counts[j]) - 1]), int(docs[j, int(counts[j]) - 1]))
                            seen[i] += counts[j]
                for rname, after, rank_of in (("start", None, np.zeros(len(qs), dtype=np.uint64)), (f"rank {RANK}", last, seen)):
                    got = sorted_call(fdd, wand, qs, col, after=after, k=10, with_stats=True)
                    assert np.array_equal(got[4], want[3]) and got[5] == want[4] and np.array_equal(got[6], rank_of)
                    rows[(cname, rname)] = dict(t=[], after=after, col=col, hits=int(got[0].sum()), skipped=int(got[6].sum()))
            t_filtered = []
            for _ in range(args.rounds):
                t_filtered.append(timed(lambda: filtered(fdd, wand, qs, None, k=10, with_stats=True))[0])
                for r in rows.values():
                    r["t"].append(timed(lambda: sorted_call(fdd, wand, qs, r["col"], after=r["after"], k=10, with_stats=True))[0])
            base = float(np.median(t_filtered))
            out[wname]["ranked_" + entry] = dict(
                filtered_us_per_query=us(t_filtered, len(qs)), noise_rel=(max(t_filtered) - min(t_filtered)) / base, matches=int(want[3].sum()),
                sorted={f"{cname}, {rname}": dict(us_per_query=us(r["t"], len(qs)), over_filtered_median=float(np.median(r["t"])) / base,
                                                 hits=r["hits"], skipped=r["skipped"]) for (cname, rname), r in rows.items()})
    # the value-range filter against the bitmap filter of the same documents
    v = columns["random"]
    lo, hi = 1 << 30, 3 << 30
    mask = (v >= lo) & (v <= hi)
    t_values, t_bitmap = [], []
    for _ in range(args.rounds + 1):
        t, f2 = timed(lambda: qi.doc_filter_from_values(handles["random"], lo, hi))
        t_values.append(t)
        t, f1 = timed(lambda: qi.doc_filter(mask))
        t_bitmap.append(t)
        i1, i2 = f1.info, f2.info
        assert (i1.num_docs, i1.n_set, i1.live_blocks) == (i2.num_docs, i2.n_set, i2.live_blocks)
        f1.close()
        f2.close()
    out["value_range_filter"] = dict(num_docs=num_docs, n_set=int(mask.sum()), from_values_ms=us(t_values[1:], 1000),
                                     from_host_bitmap_ms=us(t_bitmap[1:], 1000))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
