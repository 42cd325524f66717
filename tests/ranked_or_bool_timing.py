#!/usr/bin/env python3
"""Union-driven ranked boolean query timing on tests/ranked_query_timing.py's index: the reference's log
and the 500 heaviest queries, the whole set as one call and every query on its own (avg/q50/q90/q95 in µs), measured in ONE
process with the three calls alternating run by run:
  ranked_or    dint_ranked_or_queries of the queries
  (a) plain    dint_ranked_or_bool_queries of the same queries with m = 1 and no exclusion — the same passes with one count
               launch more: the ratio to ranked_or is reported
  (b) bool     m = 2 and one excluded term, the query's most frequent term (the others stay optional) — the ratio to (a) is
               reported
Only queries of at least three distinct terms are taken, so that (b) leaves two optional terms for m = 2; (a) and ranked_or run
(b)'s optional terms.

    python tests/ranked_or_bool_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 5] [--single-queries 0]
                                          [--out profiles/ranked_or_bool_1e8.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--single-queries", type=int, default=0, help="one query per call: only the first N of a workload (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranked_or_bool_1e8.json"))
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
    lens = coll.lens
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, lens)
    workloads = {
        "reference_log_mod_lists": reference_queries(len(lens)),
        "longest_lists": heavy_queries(lens, 500, pool=256, max_terms=5),
    }
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)
    out = {"postings": coll.num_postings, "lists": len(lens), "blocks": int(len(qi.blocks)), "type": args.type, "k": 10,
           "device": torch.cuda.get_device_name(0)}
    pct = lambda a, p: float(a[min(len(a) - 1, int(p * len(a) / 100))])  # noqa: E731
    for name, qs in workloads.items():
        should, exclude = [], []
        for q in qs:
            u = sorted(set(int(t) for t in q), key=lambda t: (int(lens[t]), t))
            if len(u) >= 3:
                should.append([int(t) for t in q if int(t) != u[-1]]), exclude.append([u[-1]])
        n = len(should)
        calls = {"ranked_or": lambda i: qi.ranked_or_queries(fdd, wand, should[i], k=10)[0],
                 "plain": lambda i: qi.ranked_or_bool_queries(fdd, wand, should[i], k=10)[0],
                 "bool": lambda i: qi.ranked_or_bool_queries(fdd, wand, should[i], exclude[i], [2] * len(should[i]), k=10)}
        whole = slice(0, n)
        counts = {what: call(whole) for what, call in calls.items()}  # (warm-up)
        blocks = counts["bool"][4]
        counts["bool"] = counts["bool"][0]
        assert np.array_equal(counts["ranked_or"], counts["plain"])
        batch = {what: [] for what in calls}
        single = {what: [] for what in calls}
        for _ in range(args.runs):  # the calls alternate: what drifts over the run drifts under all three
            for what, call in calls.items():
                t0 = time.perf_counter()
                call(whole)
                batch[what].append(time.perf_counter() - t0)
        n_single = min(n, args.single_queries) if args.single_queries else n
        for run in range(args.runs):
            for i in range(n_single):
                for what, call in calls.items():
                    t0 = time.perf_counter()
                    c = call(slice(i, i + 1))
                    if run:  # (the first pass over the queries is not timed)
                        single[what].append((time.perf_counter() - t0) * 1e6)
                    assert int(c[0][0] if what == "bool" else c[0]) == int(counts[what][i])
        res = {"queries": n, "single_queries": n_single, "bool_blocks_decoded_batch": int(blocks),
               "optional_blocks": int(sum(-(-int(lens[t]) // 256) for s in should for t in set(s)))}
        for what in calls:
            us = np.sort(np.array(single[what]))
            res[what] = {"results": int(counts[what].sum()), "gpu_batch_us_per_query": min(batch[what]) * 1e6 / max(1, n),
                         "gpu_batch_us_per_query_runs": [t * 1e6 / max(1, n) for t in batch[what]],
                         "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
        res["plain_over_ranked_or"] = {"batch": res["plain"]["gpu_batch_us_per_query"] / res["ranked_or"]["gpu_batch_us_per_query"],
                                       "single_q50": res["plain"]["gpu_single"]["q50"] / res["ranked_or"]["gpu_single"]["q50"]}
        res["bool_over_plain"] = {"batch": res["bool"]["gpu_batch_us_per_query"] / res["plain"]["gpu_batch_us_per_query"],
                                  "single_q50": res["bool"]["gpu_single"]["q50"] / res["plain"]["gpu_single"]["q50"]}
        out[name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
