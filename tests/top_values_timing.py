#!/usr/bin/env python3
"""Top-values ranked query timing: dint_ranked_or_top_values_queries and
dint_ranked_and_top_values_queries at k = 10 without a filter, with n_top 0 (the count alone: no selection is launched), 10 and
1024, over a column of about 100 distinct values (v = d % 101: no two neighbours equal, the page-local tables do the merging)
and a column whose values are all distinct (v = d: every table at its densest) — each workload as one batch and, for its first
queries, one query per call — beside the PLAIN entry (the filtered entry on a null filter: the same plan and launches but the
aggregation's) and beside the PERCENTILE entry with one percentile (four rounds over the slots), all in the same process and
timed in alternation so that all see the same clocks; the plain entry's round-to-round spread is reported as the noise the rows
are to be read against. µs per query per row; every answer is checked against the plain entry's, bit for bit, the counts of
valued matches against the matches, and the listed counts against the n_top 0 call's counts.

    python tests/top_values_timing.py [--postings 2e7] [--type single_packed_dint] [--rounds 5] [--singles 100] [--out profiles/x.json]

A column is 4 bytes per document, built one at a time. Lives under tests/ because it uses the test helpers, as
tests/percentile_timing.py does.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

N_TOPS = (0, 10, 1024)


def column(name, num_docs):
    v = np.arange(num_docs, dtype=np.uint32)
    return v % np.uint32(101) if name == "101 values" else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=2e7)
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
        call()
        return time.perf_counter() - t0

    def us(t, n):
        return {"min": min(t) * 1e6 / n, "median": float(np.median(t)) * 1e6 / n, "max": max(t) * 1e6 / n}

    def one_by_one(call, qs):
        t0 = time.perf_counter()
        for q in qs:
            call([q])
        return time.perf_counter() - t0

    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "singles": args.singles, "device": torch.cuda.get_device_name(0), "column_device_bytes": 4 * num_docs,
           "n_tops": list(N_TOPS)}
    entries = {"or": (qi.ranked_or_top_values_queries, qi.ranked_or_percentile_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_top_values_queries, qi.ranked_and_percentile_queries, qi.ranked_and_filtered_queries)}
    for wname, qs in workloads.items():
        out[wname] = {"queries": len(qs), "ranked_or": {}, "ranked_and": {}}

    def measure(wname, qs, entry, key, call, plain, extra):
        """one row: `call` against `plain`, both as a batch and (the first --singles queries) one query per call, in alternation"""
        want = plain(qs)  # (warm-up, and the answer)
        got = call(qs)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[:3], want[:3]))
        first = qs[:args.singles]
        t_plain, t_call, s_plain, s_call = [], [], [], []
        for _ in range(args.rounds):
            t_plain.append(timed(lambda: plain(qs)))
            t_call.append(timed(lambda: call(qs)))
            s_plain.append(one_by_one(plain, first))
            s_call.append(one_by_one(call, first))
        out[wname]["ranked_" + entry][key] = dict(
            plain_batch_us_per_query=us(t_plain, len(qs)), batch_us_per_query=us(t_call, len(qs)),
            batch_noise_rel=(max(t_plain) - min(t_plain)) / float(np.median(t_plain)),
            batch_over_plain_median=float(np.median(t_call) / np.median(t_plain)),
            plain_single_us_per_query=us(s_plain, len(first)), single_us_per_query=us(s_call, len(first)),
            single_noise_rel=(max(s_plain) - min(s_plain)) / float(np.median(s_plain)),
            single_over_plain_median=float(np.median(s_call) / np.median(s_plain)), **extra)
        print(wname, entry, key, "batch x%.3f single x%.3f" % (out[wname]["ranked_" + entry][key]["batch_over_plain_median"],
                                                             out[wname]["ranked_" + entry][key]["single_over_plain_median"]),
              file=sys.stderr, flush=True)
        if args.out:  # (every row as it comes: a run that is cut short leaves what it has measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")

    for cname in ("101 values", "all distinct"):
        values = column(cname, num_docs)
        col = device.DocValues(0, values)
        for wname, qs in workloads.items():
            for entry, (top_call, pct_call, plain) in entries.items():
                # the timed plain form asks for what the plain entry gives and no more: no matches
                plain_call = lambda q, p=plain: p(fdd, wand, q, None, k=10)  # noqa: E731
                same = plain(fdd, wand, qs, None, k=10, with_stats=True)
                extra = {"matches": int(same[3].sum())}
                measure(wname, qs, entry, f"percentiles {cname} 1", lambda q, c=pct_call: c(fdd, wand, q, col, [50.0], k=10), plain_call, extra)
                counts_only = None
                for n_top in N_TOPS:
                    full = top_call(fdd, wand, qs, col, n_top, k=10)
                    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(full[:4], same[:4])) and full[4] == same[4]
                    assert np.array_equal(full[5], full[3])  # (the column covers every document)
                    assert np.array_equal(full[7], np.minimum(full[6], n_top)) and full[8].shape == (len(qs), n_top)
                    if n_top == 0:
                        counts_only = full
                    else:
                        assert full[5].tobytes() == counts_only[5].tobytes() and full[6].tobytes() == counts_only[6].tobytes()
                        assert (np.diff(full[9].astype(np.int64), axis=1) <= 0).all()  # (counts descend; 0 past top_n)
                        if cname == "all distinct":
                            assert np.array_equal(full[6], full[5]) and int(full[9].max(initial=0)) <= 1
                        if n_top == 1024 and cname == "101 values":  # (every value is listed)
                            assert np.array_equal(full[9].sum(axis=1, dtype=np.uint64), full[5])
                    measure(wname, qs, entry, f"top values {cname} {n_top}", lambda q, c=top_call, n=n_top: c(fdd, wand, q, col, n, k=10),
                            plain_call, dict(extra, distinct=int(full[6].sum())))
        col.close()
        del values
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
