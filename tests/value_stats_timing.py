#!/usr/bin/env python3
"""Value-stats ranked query timing: dint_ranked_or_value_stats_queries and
dint_ranked_and_value_stats_queries at k = 10 without a filter, over a clustered column (v = d >> 6: docID order is value
order, long runs of equal buckets) and a random one (the whole u32 range), with 0, 16 and 1023 edges spread evenly over the
column's values — each workload as one batch and, for its first queries, one query per call — beside the PLAIN entry (the
filtered entry on a null filter: the same plan and launches but the reducing one) and beside the FACETED entry under clustered
maps of 17 and 1024 groups (as many counters a query as 16 and 1023 edges give buckets), all in the same process and timed in
alternation so that all see the same clocks; the plain entry's round-to-round spread is reported as the noise the rows are to be
read against. µs per query per row; every answer is checked against the plain entry's, bit for bit, and the rows' sums against
the records' n.

    python tests/value_stats_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--singles 100] [--out profiles/x.json]

A column and a map are 4 bytes per document each, built one at a time. Lives under tests/ because it uses the test helpers, as
tests/facets_timing.py does.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

EDGE_COUNTS = (0, 16, 1023)
GROUPS = (17, 1024)


def column(name, num_docs, seed=7):
    if name == "random":
        return np.random.default_rng(seed).integers(0, 1 << 32, num_docs, dtype=np.uint64).astype(np.uint32)
    v = np.arange(num_docs, dtype=np.uint32)
    v >>= np.uint32(6)
    return v


def edges_over(values, n):
    """n edges spread evenly over [the column's smallest value + 1, its largest]"""
    if n == 0:
        return None
    lo, hi = int(values.min()) + 1, int(values.max())
    return np.unique(np.linspace(lo, hi, n).astype(np.uint64)).astype(np.uint32)


def clustered_map(num_docs, n_groups):
    g = np.arange(num_docs, dtype=np.uint32)
    g //= np.uint32(max(1, -(-num_docs // n_groups)))
    np.minimum(g, np.uint32(n_groups - 1), out=g)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--singles", type=int, default=100)
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
    print("index built:", coll.num_postings, "postings,", num_docs, "documents", file=sys.stderr, flush=True)
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

    def one_by_one(call, qs):
        t0 = time.perf_counter()
        for q in qs:
            call([q])
        return time.perf_counter() - t0

    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "singles": args.singles, "device": torch.cuda.get_device_name(0), "column_device_bytes": 4 * num_docs}
    entries = {"or": (qi.ranked_or_value_stats_queries, qi.ranked_or_faceted_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_value_stats_queries, qi.ranked_and_faceted_queries, qi.ranked_and_filtered_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs), "ranked_or": {}, "ranked_and": {}}

    def measure(wname, qs, entry, key, call, plain, check):
        """one row: `call` against `plain`, both as a batch and (the first --singles queries) one query per call, in alternation"""
        want = plain(qs)  # (warm-up, and the answer)
        got = call(qs)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[:4], want[:4])) and got[4] == want[4]
        check(got)
        first = qs[:args.singles]
        t_plain, t_call, s_plain, s_call = [], [], [], []
        for _ in range(args.rounds):
            t_plain.append(timed(lambda: plain(qs))[0])
            t_call.append(timed(lambda: call(qs))[0])
            s_plain.append(one_by_one(plain, first))
            s_call.append(one_by_one(call, first))
        out[wname]["ranked_" + entry][key] = dict(
            plain_batch_us_per_query=us(t_plain, len(qs)), batch_us_per_query=us(t_call, len(qs)),
            batch_noise_rel=(max(t_plain) - min(t_plain)) / float(np.median(t_plain)),
            batch_over_plain_median=float(np.median(t_call) / np.median(t_plain)),
            plain_single_us_per_query=us(s_plain, len(first)), single_us_per_query=us(s_call, len(first)),
            single_noise_rel=(max(s_plain) - min(s_plain)) / float(np.median(s_plain)),
            single_over_plain_median=float(np.median(s_call) / np.median(s_plain)), matches=int(got[3].sum()))
        print(wname, entry, key, "batch x%.3f single x%.3f" % (out[wname]["ranked_" + entry][key]["batch_over_plain_median"],
                                                             out[wname]["ranked_" + entry][key]["single_over_plain_median"]),
              file=sys.stderr, flush=True)

    for cname in ("clustered", "random"):
        values = column(cname, num_docs)
        col = device.DocValues(0, values)
        for n_edges in EDGE_COUNTS:
            edges = edges_over(values, n_edges)
            for wname, qs in workloads.items():
                for entry, (stats_call, _, plain) in entries.items():
                    def check(got):
                        assert np.array_equal(got[5]["n"], got[3])  # (the column covers every document)
                        assert got[6] is None or np.array_equal(got[6].sum(axis=1, dtype=np.uint64), got[5]["n"])

                    measure(wname, qs, entry, f"stats {cname} {n_edges} edges",
                            lambda q, c=stats_call: c(fdd, wand, q, col, edges=edges, k=10, with_stats=True),
                            lambda q, p=plain: p(fdd, wand, q, None, k=10, with_stats=True), check)
        col.close()
        del values
    for n_groups in GROUPS:
        g = clustered_map(num_docs, n_groups)
        facets = device.DocFacets(0, g, n_groups)
        for wname, qs in workloads.items():
            for entry, (_, faceted, plain) in entries.items():
                measure(wname, qs, entry, f"faceted clustered {n_groups} groups",
                        lambda q, c=faceted: c(fdd, wand, q, facets, k=10, with_stats=True),
                        lambda q, p=plain: p(fdd, wand, q, None, k=10, with_stats=True),
                        lambda got: np.array_equal(got[5].sum(axis=1, dtype=np.uint64), got[3]))
        facets.close()
        del g
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
