#!/usr/bin/env python3
"""Ranked boolean query timing on tests/ranked_query_timing.py's index: the reference's log and the 500
heaviest queries, the whole set as one call and every query on its own (avg/q50/q90/q95 in µs), measured in ONE process with
the three calls alternating run by run:
  ranked_and   dint_ranked_and_queries of the queries' required terms
  (a) must     dint_ranked_bool_queries with only the required terms — the same launches: the ratio to ranked_and is reported
  (b) bool     the required terms + one optional + one excluded term (tests/ranked_bool.py's split: the rarest two required,
               the next optional, the most frequent excluded) — the ratio to (a) is reported
Every query of (b) has all three clauses: only queries of at least four distinct terms are taken.

    python tests/ranked_bool_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 5] [--out profiles/ranked_bool_1e8.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranked_bool_1e8.json"))
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
        must, should, exclude = [], [], []
        for q in qs:
            u = sorted(set(int(t) for t in q), key=lambda t: (int(lens[t]), t))
            if len(u) >= 4:
                must.append(u[:2]), should.append([u[2]]), exclude.append([u[-1]])
        n = len(must)
        calls = {"ranked_and": lambda i: qi.ranked_and_queries(fdd, wand, must[i], k=10)[0],
                 "must": lambda i: qi.ranked_bool_queries(fdd, wand, must[i], k=10)[0],
                 "bool": lambda i: qi.ranked_bool_queries(fdd, wand, must[i], should[i], exclude[i], k=10)[0]}
        whole = slice(0, n)
        counts = {what: call(whole) for what, call in calls.items()}  # (warm-up)
        assert np.array_equal(counts["ranked_and"], counts["must"])
        batch = {what: [] for what in calls}
        single = {what: [] for what in calls}
        for _ in range(args.runs):  # the calls alternate: what drifts over the run drifts under all three
            for what, call in calls.items():
                t0 = time.perf_counter()
                call(whole)
                batch[what].append(time.perf_counter() - t0)
        for run in range(args.runs):
            for i in range(n):
                for what, call in calls.items():
                    t0 = time.perf_counter()
                    c = call(slice(i, i + 1))
                    if run:  # (the first pass over the queries is not timed)
                        single[what].append((time.perf_counter() - t0) * 1e6)
                    assert int(c[0]) == int(counts[what][i])
        res = {"queries": n}
        for what in calls:
            us = np.sort(np.array(single[what]))
            res[what] = {"results": int(counts[what].sum()), "gpu_batch_us_per_query": min(batch[what]) * 1e6 / max(1, n),
                         "gpu_batch_us_per_query_runs": [t * 1e6 / max(1, n) for t in batch[what]],
                         "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
        res["must_over_ranked_and"] = {"batch": res["must"]["gpu_batch_us_per_query"] / res["ranked_and"]["gpu_batch_us_per_query"],
                                       "single_q50": res["must"]["gpu_single"]["q50"] / res["ranked_and"]["gpu_single"]["q50"]}
        res["bool_over_must"] = {"batch": res["bool"]["gpu_batch_us_per_query"] / res["must"]["gpu_batch_us_per_query"],
                                 "single_q50": res["bool"]["gpu_single"]["q50"] / res["must"]["gpu_single"]["q50"]}
        out[name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
