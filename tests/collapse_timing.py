#!/usr/bin/env python3
"""Collapsed ranked query timing: dint_ranked_or_collapsed_queries and
dint_ranked_and_collapsed_queries at k = 10 without a filter and without the rows, under clustered, striped and random group
maps at n_groups 8, 256, 257 and 4096 — both sides of the threshold between the LDS form and the global form of
collapse_best_kernel — each workload as one batch, beside the FACETED entry (the same plan and launches but the three
collapse launches and the clear of the table) in the same process: the baseline, timed in alternation with the collapsed rows
so that all see the same clocks, and its round-to-round spread reported as the noise the rows are to be read against. µs per
query per row and the table's device bytes; the collapsed answer's matches and blocks_decoded are checked against the faceted
entry's, its hits against the rows (a hit's group matches are the row's entry) and collapsed against the groups hit.

    python tests/collapse_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/collapse_queries_1e8.json]

The maps are built on the fly, one at a time, as tests/facets_timing.py builds them: the 10^8-posting index spans 8.8e8
docIDs, so a map is 3.5 GB on the host and on the device. Lives under tests/ because it uses the test helpers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from facets_timing import GROUPS, MAPS, group_map  # noqa: E402


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
           "k": 10, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "map_device_bytes": 4 * num_docs, "maps": {}}
    entries = {"or": (qi.ranked_or_collapsed_queries, qi.ranked_or_faceted_queries),
               "and": (qi.ranked_and_collapsed_queries, qi.ranked_and_faceted_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs), "ranked_or": {}, "ranked_and": {}}
    # a map at a time (3.5 GB each at 1e8 postings); per map, every workload and entry: baseline and collapsed row in alternation
    for n_groups in GROUPS:
        for mname in MAPS:
            g = group_map(mname, num_docs, n_groups)
            facets = device.DocFacets(0, g, n_groups)
            key = f"{mname} {n_groups}"
            out["maps"][key] = dict(n_grouped=facets.n_grouped)
            for wname, qs in workloads.items():
                for entry, (collapsed, faceted) in entries.items():
                    want = faceted(fdd, wand, qs, facets, k=10, with_stats=True)  # (warm-up, and the answer)
                    got = collapsed(fdd, wand, qs, facets, k=10, with_stats=True, with_rows=True)
                    assert np.array_equal(got[3], want[3]) and got[4] == want[4] and np.array_equal(got[8], want[5])
                    assert np.array_equal(got[5], np.count_nonzero(got[8], axis=1).astype(np.uint64))  # (every document is in a group)
                    shown = got[6] != 0xFFFFFFFF
                    rows_at_hits = np.take_along_axis(got[8], np.where(shown, got[6], 0).astype(np.int64), axis=1)
                    assert np.array_equal(got[7][shown], rows_at_hits[shown]) and not got[7][~shown].any()
                    t_faceted, t_collapsed = [], []
                    for _ in range(args.rounds):
                        t_faceted.append(timed(lambda: faceted(fdd, wand, qs, facets, k=10, with_stats=True))[0])
                        t_collapsed.append(timed(lambda: collapsed(fdd, wand, qs, facets, k=10, with_stats=True))[0])
                    out[wname]["ranked_" + entry][key] = dict(
                        faceted_us_per_query=us(t_faceted, len(qs)), collapsed_us_per_query=us(t_collapsed, len(qs)),
                        noise_rel=(max(t_faceted) - min(t_faceted)) / float(np.median(t_faceted)),
                        collapsed_over_faceted_median=float(np.median(t_collapsed) / np.median(t_faceted)),
                        matches=int(got[3].sum()), collapsed=int(got[5].sum()), table_device_bytes=8 * len(qs) * n_groups)
            facets.close()
            del g
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
