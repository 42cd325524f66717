#!/usr/bin/env python3
"""dint_score_documents timing against ranked_or on the same index: the reference log and the 500
heaviest queries over tests/ranked_or_query_timing.py's index, 10 / 1 000 / 100 000 documents a query drawn from its union
(fewer where the union is smaller), as one batch and one query per call, alternating with dint_ranked_or_queries at k = 10
in the same process; the blocks read against all blocks; and the re-scoring of ranked_or's own k = 10 answer, whose scores
are checked equal bit for bit.

    python tests/score_documents_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 3] [--out file.json]
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
    ap.add_argument("--single", type=int, default=100, help="queries timed one per call (the first of each set)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/ranked_or_query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    n_lists = len(coll.lens)
    bounds = coll.list_bounds()
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    workloads = {"reference_log_mod_lists": reference_queries(n_lists),
                 "longest_lists": heavy_queries(coll.lens, 500, pool=256, max_terms=5)}
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)
    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "type": args.type, "k": 10,
           "device": torch.cuda.get_device_name(0)}
    r = np.random.default_rng(21)

    def best(call, runs):
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    for name, qs in workloads.items():
        unions = [np.unique(np.concatenate([docids[int(bounds[t]):int(bounds[t + 1])] for t in np.unique(q)])) for q in qs]
        ref = qi.ranked_or_queries(fdd, wand, qs, k=10)  # (warm-up, and the answer to re-score)
        _, _, all_blocks = qi.or_queries_with_freqs(fdd, qs)
        res = {"queries": len(qs), "blocks_ranked_or": int(all_blocks)}
        sets = {str(n): [r.choice(u, min(n, u.size), replace=False).astype(np.uint32) for u in unions] for n in (10, 1000, 100000)}
        sets["ranked_or_top10"] = [ref[2][i][:int(ref[0][i])] for i in range(len(qs))]
        top = qi.score_documents(fdd, wand, qs, sets["ranked_or_top10"])
        assert all(np.array_equal(top[0][i].view(np.uint32), ref[1][i][:int(ref[0][i])].view(np.uint32)) for i in range(len(qs)))
        n1 = min(args.single, len(qs))
        for label, docs in sets.items():
            got = qi.score_documents(fdd, wand, qs, docs)  # (warm-up)
            row = {"documents": int(sum(d.size for d in docs)), "blocks_read": int(got[2])}
            # alternating, call by call: ranked_or, score_documents
            t_or, t_sd = [], []
            for _ in range(max(args.runs, 5)):
                t_or.append(best(lambda: qi.ranked_or_queries(fdd, wand, qs, k=10), 1))
                t_sd.append(best(lambda: qi.score_documents(fdd, wand, qs, docs), 1))
            row["batch_us_per_query"] = {"ranked_or": min(t_or) * 1e6 / len(qs), "score_documents": min(t_sd) * 1e6 / len(qs)}
            one_or, one_sd = [], []
            for run in range(args.runs):
                for i in range(n1):
                    a = best(lambda: qi.ranked_or_queries(fdd, wand, [qs[i]], k=10), 1)
                    b = best(lambda: qi.score_documents(fdd, wand, [qs[i]], [docs[i]]), 1)
                    if run:  # (the first run is not timed)
                        one_or.append(a * 1e6)
                        one_sd.append(b * 1e6)
            row["single_us"] = {"ranked_or": {"avg": float(np.mean(one_or)), "q50": float(np.median(one_or))},
                                "score_documents": {"avg": float(np.mean(one_sd)), "q50": float(np.median(one_sd))}}
            res[label] = row
            print(json.dumps({name: {label: row}}), file=sys.stderr, flush=True)
        out[name] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
