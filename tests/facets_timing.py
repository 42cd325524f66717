#!/usr/bin/env python3
"""Faceted ranked query timing: dint_ranked_or_faceted_queries and dint_ranked_and_faceted_queries at
k = 10 without a filter, under clustered, striped and random group maps at n_groups 8, 256, 257 and 4096 — both sides of the
threshold between the LDS form and the global form of the counting kernel — each workload as one batch, beside the UNFACETED
entry (the filtered entry on a null filter: the same plan and launches but the counting one) in the same process: the
baseline, timed in alternation with the faceted rows so that all see the same clocks, and its round-to-round spread reported
as the noise the rows are to be read against. For n_groups = 8 also the eight filtered calls, one per group, that answer the
same question without facets. µs per query per row, the map's device bytes and its creation time; the faceted answer is
checked against the unfaceted entry's, bit for bit, the rows' sums against matches, and at n_groups = 8 the rows against the
eight filtered calls' matches.

    python tests/facets_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/x.json]

The maps are built on the fly, one at a time: the 10^8-posting index spans 8.8e8 docIDs, so a map is 3.5 GB on the host and
on the device. Lives under tests/ because it uses the test helpers, as tests/doc_filter_timing.py does.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

GROUPS = (8, 256, 257, 4096)
MAPS = ("clustered", "striped", "random")


def group_map(name, num_docs, n_groups, seed=7):
    """tests/facets.py's named maps as u32, built in place (no int64 temporaries of the docID space)"""
    if name == "random":
        return np.random.default_rng(seed).integers(0, n_groups, num_docs, dtype=np.uint32)
    g = np.arange(num_docs, dtype=np.uint32)
    if name == "striped":
        g %= np.uint32(n_groups)
        return g
    g //= np.uint32(max(1, -(-num_docs // n_groups)))
    np.minimum(g, np.uint32(n_groups - 1), out=g)
    return g


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
    entries = {"or": (qi.ranked_or_faceted_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_faceted_queries, qi.ranked_and_filtered_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs), "ranked_or": {}, "ranked_and": {}}
    # a map at a time (3.5 GB each at 1e8 postings); per map, every workload and entry: baseline and faceted row in alternation
    for n_groups in GROUPS:
        for mname in MAPS:
            g = group_map(mname, num_docs, n_groups)
            t_create, facets = timed(lambda: device.DocFacets(0, g, n_groups))
            key = f"{mname} {n_groups}"
            out["maps"][key] = dict(create_us=t_create * 1e6, n_grouped=facets.n_grouped)
            masks = [g == np.uint32(i) for i in range(n_groups)] if n_groups == 8 else None
            filters = [qi.doc_filter(m) for m in masks] if masks else None
            for wname, qs in workloads.items():
                for entry, (faceted, plain) in entries.items():
                    want = plain(fdd, wand, qs, None, k=10, with_stats=True)  # (warm-up, and the answer)
                    got = faceted(fdd, wand, qs, facets, k=10, with_stats=True)
                    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[:4], want[:4])) and got[4] == want[4]
                    assert np.array_equal(got[5].sum(axis=1, dtype=np.uint64), got[3])  # (every document is in a group)
                    t_plain, t_faceted, t_eight = [], [], []
                    for _ in range(args.rounds):
                        t_plain.append(timed(lambda: plain(fdd, wand, qs, None, k=10, with_stats=True))[0])
                        t_faceted.append(timed(lambda: faceted(fdd, wand, qs, facets, k=10, with_stats=True))[0])
                        if filters:
                            t, per_group = timed(lambda: [plain(fdd, wand, qs, f, k=10, with_stats=True)[3] for f in filters])
                            t_eight.append(t)
                            assert np.array_equal(np.stack(per_group, axis=1), got[5].astype(np.uint64))
                    row = dict(unfaceted_us_per_query=us(t_plain, len(qs)), faceted_us_per_query=us(t_faceted, len(qs)),
                               noise_rel=(max(t_plain) - min(t_plain)) / float(np.median(t_plain)),
                               faceted_over_unfaceted_median=float(np.median(t_faceted) / np.median(t_plain)),
                               matches=int(got[3].sum()), groups_hit=int(np.count_nonzero(got[5])))
                    if filters:
                        row["eight_filtered_calls_us_per_query"] = us(t_eight, len(qs))
                    out[wname]["ranked_" + entry][key] = row
            for f in filters or []:
                f.close()
            facets.close()
            del g, masks
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
