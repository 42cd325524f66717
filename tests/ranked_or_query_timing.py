#!/usr/bin/env python3
"""Ranked OR timing next to or_freq on the same index: the reference's op_perftest shape
(src/queries.cpp:15-61 — every query on its own, avg/q50/q90/q95 in µs) and the whole log as one call, for
dint_ranked_or_queries at k = 10 and dint_or_queries_freqs, plus one CPU core answering a sample of the same queries with
the binary32 model (tests/ranked_or.py: numpy over the builder's lists, the union and the scoring timed, no decode).

    python tests/ranked_or_query_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 3]

Lives under tests/ because it uses the test model, as tests/or_query_timing.py uses the CPU oracle.
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=30)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries
    import ranked
    import ranked_or

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    bounds = coll.list_bounds()
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
    lists = ranked.BuilderLists(docids, freqs, bounds)
    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "type": args.type, "k": 10,
           "device": torch.cuda.get_device_name(0)}
    pct = lambda a, p: float(a[min(len(a) - 1, int(p * len(a) / 100))])
    for name, qs in workloads.items():
        res = {"queries": len(qs)}
        calls = (("ranked_or", lambda q: qi.ranked_or_queries(fdd, wand, q, k=10)[0]),
                 ("or_freq", lambda q: qi.or_queries_with_freqs(fdd, q)[0]))
        for what, call in calls:
            counts = call(qs)  # (warm-up)
            t_batch = []
            for _ in range(max(args.runs, 5)):
                t0 = time.perf_counter()
                call(qs)
                t_batch.append(time.perf_counter() - t0)
            for q in qs:
                call([q])
            us = []
            for _ in range(args.runs - 1):
                for q, want in zip(qs, counts):
                    t0 = time.perf_counter()
                    c = call([q])
                    us.append((time.perf_counter() - t0) * 1e6)
                    assert int(c[0]) == int(want)
            us = np.sort(np.array(us))
            res[what] = {"results": int(counts.sum()), "gpu_batch_us_per_query": min(t_batch) * 1e6 / len(qs),
                         "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
            if what == "or_freq":
                assert np.array_equal(np.minimum(counts, 10), ranked_counts)
            else:
                ranked_counts = counts.copy()
        # one CPU core: the model over a sample, checked bit for bit against the device
        sample = qs[:: max(1, len(qs) // args.cpu_sample)][: args.cpu_sample]
        got = qi.ranked_or_queries(fdd, wand, sample, k=10)
        cpu = []
        for i, q in enumerate(sample):
            t0 = time.perf_counter()
            n, sc, ids = ranked_or.ranked_or(lists, q, norm_lens, num_docs, 10)
            cpu.append((time.perf_counter() - t0) * 1e6)
            assert n == got[0][i] and np.array_equal(sc.view(np.uint32), got[1][i].view(np.uint32)) and np.array_equal(ids, got[2][i])
        cpu = np.sort(np.array(cpu))
        res["cpu_one_core_model"] = {"queries": len(sample), "avg": float(cpu.mean()), "q50": pct(cpu, 50), "q90": pct(cpu, 90),
                                     "q95": pct(cpu, 95), "note": "tests/ranked_or.py (numpy, binary32) over the builder's lists: no decode"}
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
