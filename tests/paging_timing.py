#!/usr/bin/env python3
"""Paged ranked query timing: dint_ranked_or_paged_queries and dint_ranked_and_paged_queries at k = 10
without a filter, with every query's cursor from the start, at rank 1 000 and at rank 10 000 — the cursors taken from a first
walk (pages of 1 000: the last hit of the first page, and of the tenth) — each workload as one batch, beside the FILTERED
entry on a null filter (the same plan and launches but page_after_kernel, the upload of the keys and the clear of the
counters) in the same process: the baseline, timed in alternation with the paged rows so that all see the same clocks, and its
round-to-round spread reported as the noise the rows are to be read against. µs per query per row and each row's ratio to the
baseline's median; the paged answer's matches and blocks_decoded are checked against the filtered entry's, the from-the-start
answer against its hits bit for bit, and skipped against the cursor's rank.

    python tests/paging_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/paging_queries_1e8.json]

A query with fewer matches than a rank has no hit there: its cursor is its last hit, and nothing lies behind it. Lives under
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

RANKS = (1000, 10000)
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

    def timed(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0), out

    def us(t, n):
        return {"min": min(t) * 1e6 / n, "median": float(np.median(t)) * 1e6 / n, "max": max(t) * 1e6 / n}

    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "ranks": list(RANKS)}
    entries = {"or": (qi.ranked_or_paged_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_paged_queries, qi.ranked_and_filtered_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs)}
        for entry, (paged, filtered) in entries.items():
            want = filtered(fdd, wand, qs, None, k=10, with_stats=True)  # (warm-up, and the answer)
            # the first walk: every query's last hit of the page that ends at each rank (or its last hit before)
            cursors, rank_of = {"start": None}, {"start": np.zeros(len(qs), dtype=np.uint64)}
            last, seen = [None] * len(qs), np.zeros(len(qs), dtype=np.uint64)
            for page, (ids, counts, scores, docs, _) in enumerate(qi.ranked_pages(entry, fdd, wand, qs, k=WALK_K, max_pages=max(RANKS) // WALK_K)):
                for j, i in enumerate(ids.tolist()):
                    if counts[j]:
                        last[i] = (scores[j, int(counts[j]) - 1], int(docs[j, int(counts[j]) - 1]))
                        seen[i] += counts[j]
                if (page + 1) * WALK_K in RANKS:
                    cursors[f"rank {(page + 1) * WALK_K}"] = list(last)
                    rank_of[f"rank {(page + 1) * WALK_K}"] = seen.copy()
            for r in RANKS:  # (every query ran out before a rank: the walk ended early)
                cursors.setdefault(f"rank {r}", list(last))
                rank_of.setdefault(f"rank {r}", seen.copy())
            rows = {}
            for cname, after in cursors.items():
                got = paged(fdd, wand, qs, after=after, k=10, with_stats=True)
                assert np.array_equal(got[3], want[3]) and got[4] == want[4] and np.array_equal(got[5], rank_of[cname])
                if after is None:
                    assert all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got[:3], want[:3]))
                rows[cname] = dict(t=[], hits=int(got[0].sum()), skipped=int(got[5].sum()))
            t_filtered = []
            for _ in range(args.rounds):
                t_filtered.append(timed(lambda: filtered(fdd, wand, qs, None, k=10, with_stats=True))[0])
                for cname, after in cursors.items():
                    rows[cname]["t"].append(timed(lambda: paged(fdd, wand, qs, after=after, k=10, with_stats=True))[0])
            base = float(np.median(t_filtered))
            out[wname]["ranked_" + entry] = dict(
                filtered_us_per_query=us(t_filtered, len(qs)), noise_rel=(max(t_filtered) - min(t_filtered)) / base, matches=int(want[3].sum()),
                paged={cname: dict(us_per_query=us(r["t"], len(qs)), over_filtered_median=float(np.median(r["t"])) / base, hits=r["hits"],
                                   skipped=r["skipped"]) for cname, r in rows.items()})
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
