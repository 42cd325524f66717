#!/usr/bin/env python3
"""Group-stats ranked query timing: dint_ranked_or_group_stats_queries and
dint_ranked_and_group_stats_queries at k = 10 without a filter and without facet counts, over the heavy log of the other timing
scripts (the longest lists), under clustered maps of 8, 256, 300 and 65 536 groups (and a striped one of 8) and a random column
(the whole u32 range) — each as one batch, cut into calls of 256 queries where 65 536 groups would pass the call's 2^24 records —
beside the FACETED entry on the same arguments (the difference is the new launch against facet_count_kernel: the faceted entry
is the filtered entry plus that launch) and beside the PLAIN entry (the filtered entry on a null filter), all in the same
process and timed in alternation so that all see the same clocks; the plain entry's round-to-round spread is reported as the
noise the rows are to be read against. With 8 groups also the only alternative without the entries: eight filtered value-stats
calls, one per group, each under the filter of the group's documents — every one decodes and scores the batch again, though
under a clustered map a group's filter leaves only its own blocks alive; under the striped map it leaves all. µs per query per
row; every answer is checked against the plain entry's, bit for bit, the records' n against the faceted entry's rows (the column
covers every document), and with 8 groups the records against the eight calls'.

    python tests/group_stats_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/x.json]

A column and a map are 4 bytes per document each. Lives under tests/ because it uses the test helpers, as
tests/value_stats_timing.py does. It is not a test and sets no threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

GROUPS = (8, 256, 300, 65536)
MAX_RECORDS = 1 << 24  # DINT_GROUP_STATS_MAX_RECORDS: a call takes n_queries * n_groups records, the caller batches


def clustered_map(num_docs, n_groups):
    g = np.arange(num_docs, dtype=np.uint32)
    g //= np.uint32(max(1, -(-num_docs // n_groups)))
    np.minimum(g, np.uint32(n_groups - 1), out=g)
    return g


def striped_map(num_docs, n_groups):
    g = np.arange(num_docs, dtype=np.uint32)
    g %= np.uint32(n_groups)
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
    from queries import heavy_queries

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    print("index built:", coll.num_postings, "postings,", num_docs, "documents", file=sys.stderr, flush=True)
    qs = heavy_queries(coll.lens, 500, pool=256, max_terms=5)
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)
    values = np.random.default_rng(7).integers(0, 1 << 32, num_docs, dtype=np.uint64).astype(np.uint32)
    col = device.DocValues(0, values)

    def timed(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0), out

    def us(t):
        return {"min": min(t) * 1e6 / len(qs), "median": float(np.median(t)) * 1e6 / len(qs), "max": max(t) * 1e6 / len(qs)}

    out = {"postings": coll.num_postings, "lists": len(coll.lens), "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "queries": len(qs), "device": torch.cuda.get_device_name(0), "ranked_or": {}, "ranked_and": {}}
    entries = {"or": (qi.ranked_or_group_stats_queries, qi.ranked_or_faceted_queries, qi.ranked_or_filtered_queries, qi.ranked_or_value_stats_queries),
               "and": (qi.ranked_and_group_stats_queries, qi.ranked_and_faceted_queries, qi.ranked_and_filtered_queries, qi.ranked_and_value_stats_queries)}

    def in_chunks(call, step):
        """the batch in calls of at most `step` queries -> the outputs joined (blocks_decoded summed)"""
        parts = [call(qs[i:i + step]) for i in range(0, len(qs), step)]
        return tuple(sum(p[j] for p in parts) if j == 4 else np.concatenate([p[j] for p in parts]) for j in range(len(parts[0])))

    for n_groups, map_name in [(n, "clustered") for n in GROUPS] + [(8, "striped")]:
        g = (clustered_map if map_name == "clustered" else striped_map)(num_docs, n_groups)
        facets = device.DocFacets(0, g, n_groups)
        filters = [qi.doc_filter(g == i) for i in range(n_groups)] if n_groups == 8 else []
        step = min(len(qs), MAX_RECORDS // n_groups)  # (65 536 groups: 256 queries a call; every entry is cut the same way)
        for entry, (grouped, faceted, plain, vstats) in entries.items():
            calls = {"plain": lambda: in_chunks(lambda q: plain(fdd, wand, q, None, k=10, with_stats=True), step),
                     "faceted": lambda: in_chunks(lambda q: faceted(fdd, wand, q, facets, k=10, with_stats=True), step),
                     "group_stats": lambda: in_chunks(lambda q: grouped(fdd, wand, q, facets, col, k=10)[:6], step)}
            if filters:
                calls["value_stats_per_group"] = lambda: [vstats(fdd, wand, qs, col, filter=f, k=10, with_stats=True) for f in filters]
            got = {name: call() for name, call in calls.items()}  # (warm-up, and the answers)
            want = got["plain"]
            for name in ("faceted", "group_stats"):
                assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[name][:4], want[:4])) and got[name][4] == want[4]
            recs = got["group_stats"][5]
            assert np.array_equal(recs["n"], got["faceted"][5])  # (the column covers every document)
            if filters:
                per_group = np.stack([o[5] for o in got["value_stats_per_group"]], axis=1)
                assert per_group.tobytes() == recs.tobytes()
            times = {name: [] for name in calls}
            for _ in range(args.rounds):
                for name, call in calls.items():
                    times[name].append(timed(call)[0])
            row = {name + "_us_per_query": us(t) for name, t in times.items()}
            row["noise_rel"] = (max(times["plain"]) - min(times["plain"])) / float(np.median(times["plain"]))
            for name in times:
                if name != "plain":
                    row[name + "_over_plain_median"] = float(np.median(times[name]) / np.median(times["plain"]))
            row["group_stats_minus_faceted_us_per_query"] = (float(np.median(times["group_stats"])) - float(np.median(times["faceted"]))) * 1e6 / len(qs)
            row["matches"] = int(want[3].sum())
            row["queries_per_call"] = step
            out["ranked_" + entry][f"{n_groups} groups, {map_name}"] = row
            print(entry, n_groups, map_name, {k: round(v, 3) for k, v in row.items() if k.endswith("_median")}, file=sys.stderr, flush=True)
        for f in filters:
            f.close()
        facets.close()
        del g
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
