#!/usr/bin/env python3
"""DocID-range ranked query timing: dint_ranked_or_range_queries and dint_ranked_and_range_queries at
k = 10 over ranges of 1/1, 1/8 and 1/64 of the docID space, each workload as one batch, beside the UNRANGED entry in the
same process — the baseline, timed in alternation with the full-range rows so that both see the same clocks, and its
round-to-round spread reported as the noise the full-range row is to be read against. µs per query and blocks_decoded per
row; blocks_decoded is checked against the blocks in range of the host block table, and the full-range answer against the
unranged entry's, bit for bit.

    python tests/ranked_range_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 7] [--out profiles/x.json]

Lives under tests/ because it uses the test helpers, as tests/ranked_or_query_timing.py does.
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries
    import ranked_range as RR

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
    first = np.searchsorted(qi.blocks["list"], np.arange(n_lists + 1))  # list t's records: [first[t], first[t + 1])
    maxima = qi.blocks["max"]

    def blocks_in(entry, qs, lo, hi):
        total = 0
        for q in qs:
            terms = sorted(set(int(t) for t in q))
            if entry == "and" and terms:
                terms = [min(terms, key=lambda t: (int(coll.lens[t]), t))]
            for t in terms:
                p0, p1 = RR.blocks_in_range(maxima[first[t]:first[t + 1]], lo, hi)
                total += p1 - p0
        return total

    def timed(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0), out

    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    fractions = {"1/1": (0, num_docs), "1/8": (3 * num_docs // 8, 3 * num_docs // 8 + num_docs // 8),
                 "1/64": (3 * num_docs // 8, 3 * num_docs // 8 + num_docs // 64)}
    for name, qs in workloads.items():
        res = {"queries": len(qs)}
        for entry in ("or", "and"):
            ranged = qi.ranked_or_range_queries if entry == "or" else qi.ranked_and_range_queries
            plain = qi.ranked_or_queries if entry == "or" else qi.ranked_and_queries
            full = np.array([fractions["1/1"]] * len(qs), dtype=np.uint32)
            want = plain(fdd, wand, qs, k=10)  # (warm-up, and the answer)
            got = ranged(fdd, wand, qs, full, k=10, with_stats=True)
            assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got[:3], want))
            # the baseline and the full-range row in alternation: A B A B ...
            t_plain, t_full = [], []
            for _ in range(args.rounds):
                t_plain.append(timed(lambda: plain(fdd, wand, qs, k=10))[0])
                t_full.append(timed(lambda: ranged(fdd, wand, qs, full, k=10, with_stats=True))[0])
            us = lambda ts: {"min": min(ts) * 1e6 / len(qs), "median": float(np.median(ts)) * 1e6 / len(qs),  # noqa: E731
                             "max": max(ts) * 1e6 / len(qs)}
            rows = {"unranged": dict(us_per_query=us(t_plain), results=int(want[0].sum()))}
            rows["unranged"]["noise_rel"] = (max(t_plain) - min(t_plain)) / float(np.median(t_plain))
            for frac, (lo, hi) in fractions.items():
                rg = np.array([(lo, hi)] * len(qs), dtype=np.uint32)
                if frac == "1/1":
                    ts, last = t_full, got
                else:
                    last = ranged(fdd, wand, qs, rg, k=10, with_stats=True)
                    ts = [timed(lambda: ranged(fdd, wand, qs, rg, k=10, with_stats=True))[0] for _ in range(args.rounds)]
                assert last[4] == blocks_in(entry, qs, lo, hi)
                rows[frac] = dict(us_per_query=us(ts), results=int(last[0].sum()), matches=int(last[3].sum()), blocks_decoded=int(last[4]))
            rows["full_range_over_unranged_median"] = rows["1/1"]["us_per_query"]["median"] / rows["unranged"]["us_per_query"]["median"]
            res["ranked_" + entry] = rows
        out[name] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
