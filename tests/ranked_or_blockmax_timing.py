#!/usr/bin/env python3
"""Block maxima timing (DESIGN.md 4d-wand, 4d-maxscore "block maxima") on the index of tests/ranked_or_query_timing.py, in one
process:

  build    dint_index_max_weights with and without block maxima against dinth_wand_data over the same postings on one core
           -> profiles/index_max_weights_1e8.json
  queries  dint_ranked_or_queries, dint_ranked_or_maxscore_queries on a handle with term maxima and the same call on a handle
           that also has block maxima, k = 10, alternating call by call, over the light reference log, the heavy set and the
           mixed set (tests/maxscore.py), as one batch and as one query per call, with the blocks each call reads; the answers
           are checked equal call by call -> profiles/ranked_or_blockmax_1e8.json

    python tests/ranked_or_blockmax_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 3] [--out-dir profiles]
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
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--queries", type=int, default=500)
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
    sizes = host.sizes_from_postings(docids, freqs, num_docs)
    t0 = time.perf_counter()
    norm_lens, mtw = host.wand_data(sizes, docids, freqs, coll.lens)
    host_s = time.perf_counter() - t0
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    plain = device.WandData(norm_lens)
    tag = f"{args.postings:.0e}".replace("+0", "").replace("+", "")
    head = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "type": args.type,
            "device": torch.cuda.get_device_name(0)}

    # ---- the build ----
    build = {w: [] for w in ("terms_only", "with_blocks")}
    bmw = None
    for _ in range(max(args.runs, 3) + 1):  # (the first of each is a warm-up: the workspaces are allocated there)
        for w in build:
            t0 = time.perf_counter()
            got = qi.max_weights(fdd, plain, with_blocks=w == "with_blocks")
            build[w].append(time.perf_counter() - t0)
            got_mtw = got[0] if w == "with_blocks" else got
            assert np.array_equal(got_mtw.view(np.uint32), mtw.view(np.uint32))
            if w == "with_blocks":
                bmw = got[1]
    out = dict(head, host_wand_data_one_core_s=host_s, **{f"device_{w}_s": min(v[1:]) for w, v in build.items()})
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, f"index_max_weights_{tag}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), file=sys.stderr, flush=True)

    # ---- the pruned call ----
    wand = device.WandData(norm_lens, max_term_weight=mtw)
    bwand = device.WandData(norm_lens, max_term_weight=mtw)
    bwand.set_block_max_weights(bmw)
    workloads = {
        "reference_log_mod_lists": reference_queries(n_lists)[:args.queries],
        "longest_lists": heavy_queries(coll.lens, args.queries, pool=256, max_terms=5),
        "mixed": mixed_queries(coll.lens, args.queries),
    }
    out = dict(head, k=10)
    pct = lambda a, p: float(a[min(len(a) - 1, int(p * len(a) / 100))])
    calls = {"ranked_or": lambda q: qi.ranked_or_queries(fdd, wand, q, k=10),
             "ranked_or_maxscore": lambda q: qi.ranked_or_maxscore_queries(fdd, wand, q, k=10),
             "ranked_or_blockmax": lambda q: qi.ranked_or_maxscore_queries(fdd, bwand, q, k=10)}
    same = lambda a, b: all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x,
                                           np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
                            for x, y in zip(a[:3], b[:3]))
    for name, qs in workloads.items():
        ref = calls["ranked_or"](qs)
        ms = calls["ranked_or_maxscore"](qs)  # (warm-ups)
        bm = calls["ranked_or_blockmax"](qs)
        assert same(ref, ms) and same(ref, bm) and bm[3] <= ms[3]
        _, _, all_blocks = qi.or_queries_with_freqs(fdd, qs)
        res = {"queries": len(qs), "results": int(ref[0].sum()), "blocks_ranked_or": int(all_blocks), "blocks_maxscore": int(ms[3]),
               "blocks_blockmax": int(bm[3])}
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
                assert same(got["ranked_or"], got["ranked_or_maxscore"]) and same(got["ranked_or"], got["ranked_or_blockmax"])
        for w in calls:
            us = np.sort(np.array(single[w]))
            res[w] = {"gpu_batch_us_per_query": min(batch[w]) * 1e6 / len(qs),
                      "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
        out[name] = res
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    with open(os.path.join(args.out_dir, f"ranked_or_blockmax_{tag}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
