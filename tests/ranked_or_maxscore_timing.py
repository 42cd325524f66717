#!/usr/bin/env python3
"""MaxScore-pruned ranked OR timing against ranked_or on the same index: dint_ranked_or_queries and
dint_ranked_or_maxscore_queries at k = 10, in one process, alternating call by call — the reference's op_perftest shape
(src/queries.cpp:15-61: every query on its own, avg/q50/q90/q95 in µs) and the whole set as one call — over the light
reference log, the heavy set and the mixed set (tests/maxscore.py), with the blocks each call reads. The results are
checked equal call by call.

    python tests/ranked_or_maxscore_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 3]

Lives under tests/ beside tests/ranked_or_query_timing.py, whose index it builds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from maxscore import mixed_queries
    from queries import heavy_queries, reference_queries

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/ranked_or_query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    n_lists = len(coll.lens)
    num_docs = int(docids.max()) + 1
    norm_lens, mtw = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    workloads = {
        "reference_log_mod_lists": reference_queries(n_lists),
        "longest_lists": heavy_queries(coll.lens, 500, pool=256, max_terms=5),
        "mixed": mixed_queries(coll.lens, 500),
    }
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens, max_term_weight=mtw)
    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "type": args.type, "k": 10,
           "device": torch.cuda.get_device_name(0)}
    pct = lambda a, p: float(a[min(len(a) - 1, int(p * len(a) / 100))])
    calls = {"ranked_or": lambda q: qi.ranked_or_queries(fdd, wand, q, k=10),
             "ranked_or_maxscore": lambda q: qi.ranked_or_maxscore_queries(fdd, wand, q, k=10)}
    same = lambda a, b: all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x,
                                           np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
                            for x, y in zip(a[:3], b[:3]))
    for name, qs in workloads.items():
        ref = calls["ranked_or"](qs)
        ms = calls["ranked_or_maxscore"](qs)  # (warm-ups)
        assert same(ref, ms)
        _, _, all_blocks = qi.or_queries_with_freqs(fdd, qs)
        res = {"queries": len(qs), "results": int(ref[0].sum()), "blocks_ranked_or": int(all_blocks), "blocks_maxscore": int(ms[3])}
        batch = {w: [] for w in calls}
        for _ in range(max(args.runs, 5)):
            for w, call in calls.items():
                t0 = time.perf_counter()
                call(qs)
                batch[w].append(time.perf_counter() - t0)
        single = {w: [] for w in calls}
        for run in range(args.runs):
            for q in qs:
                got = {}
                for w, call in calls.items():
                    t0 = time.perf_counter()
                    got[w] = call([q])
                    if run:  # (the first run is not timed)
                        single[w].append((time.perf_counter() - t0) * 1e6)
                assert same(got["ranked_or"], got["ranked_or_maxscore"])
        for w in calls:
            us = np.sort(np.array(single[w]))
            res[w] = {"gpu_batch_us_per_query": min(batch[w]) * 1e6 / len(qs),
                      "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
        out[name] = res
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
