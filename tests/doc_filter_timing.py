#!/usr/bin/env python3
"""Document-filter ranked query timing: dint_ranked_or_filtered_queries and
dint_ranked_and_filtered_queries at k = 10 under five filters — all ones, random densities 1/2, 1/8 and 1/64, and one run
covering 1/8 of the docID space — each workload as one batch, beside the UNFILTERED entry in the same process: the baseline,
timed in alternation with the filtered rows so that all see the same clocks, and its round-to-round spread reported as the
noise the all-ones row is to be read against. µs per query, matches and blocks_decoded per row; the filters' creation timed
by itself, with their live_blocks; blocks_decoded is checked against the live blocks of the host block table, and the
all-ones answer against the unfiltered entry's, bit for bit.

    python tests/doc_filter_timing.py [--postings 1e8] [--type single_packed_dint] [--rounds 5] [--out profiles/x.json]

Lives under tests/ because it uses the test helpers, as tests/ranked_range_timing.py does.
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries
    import doc_filter as DF

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

    def timed(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0), out

    # the filters as bitmap words (the index spans ~9e8 docIDs: a byte per document is too much). A random word is density
    # 1/2; the AND of j of them 2^-j. The last word is masked here, so that the popcounts below are the filter's.
    r = np.random.default_rng(7)
    n_words = (num_docs + 63) // 64
    random_words = lambda j: np.bitwise_and.reduce([r.integers(0, 1 << 64, n_words, dtype=np.uint64) for _ in range(j)])  # noqa: E731
    run = np.zeros(n_words, dtype=np.uint64)
    run[3 * n_words // 8:3 * n_words // 8 + n_words // 8] = ~np.uint64(0)
    masks = {"all ones": np.full(n_words, ~np.uint64(0)), "random 1/2": random_words(1), "random 1/8": random_words(3),
             "random 1/64": random_words(6), "one run of 1/8": run}
    if num_docs & 63:
        for words in masks.values():
            words[-1] &= (np.uint64(1) << np.uint64(num_docs & 63)) - np.uint64(1)
    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "filters": {}}
    filters, live_before = {}, {}
    for name, words in masks.items():
        n = num_docs
        qi.doc_filter(words, n).close()  # (warm-up)
        ts = []
        for _ in range(args.rounds):
            t, f = timed(lambda: qi.doc_filter(words, n))
            ts.append(t)
            if len(ts) != args.rounds:
                f.close()
        filters[name] = f
        live = DF.live_blocks_words(qi.blocks, words, n)
        live_before[name] = np.concatenate([[0], np.cumsum(live)])
        info = f.info
        assert (info.n_set, info.live_blocks) == (int(DF.popcount64(words).sum()), int(live.sum()))
        out["filters"][name] = dict(n_set=int(info.n_set), live_blocks=int(info.live_blocks),
                                    create_us=dict(min=min(ts) * 1e6, median=float(np.median(ts)) * 1e6, max=max(ts) * 1e6))

    def blocks_in(entry, qs, name):
        total = 0
        for q in qs:
            terms = sorted(set(int(t) for t in q))
            if entry == "and" and terms:
                terms = [min(terms, key=lambda t: (int(coll.lens[t]), t))]
            total += sum(int(live_before[name][first[t + 1]] - live_before[name][first[t]]) for t in terms)
        return total

    for wname, qs in workloads.items():
        res = {"queries": len(qs)}
        for entry in ("or", "and"):
            filtered = qi.ranked_or_filtered_queries if entry == "or" else qi.ranked_and_filtered_queries
            plain = qi.ranked_or_queries if entry == "or" else qi.ranked_and_queries
            want = plain(fdd, wand, qs, k=10)  # (warm-up, and the answer)
            last = {name: filtered(fdd, wand, qs, f, k=10, with_stats=True) for name, f in filters.items()}  # (warm-up, and the answers)
            assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(last["all ones"][:3], want))
            # the baseline and the filtered rows in alternation: A B C D E F A B ...
            t_plain, ts = [], {name: [] for name in filters}
            for _ in range(args.rounds):
                t_plain.append(timed(lambda: plain(fdd, wand, qs, k=10))[0])
                for name, f in filters.items():
                    ts[name].append(timed(lambda: filtered(fdd, wand, qs, f, k=10, with_stats=True))[0])
            us = lambda t: {"min": min(t) * 1e6 / len(qs), "median": float(np.median(t)) * 1e6 / len(qs),  # noqa: E731
                            "max": max(t) * 1e6 / len(qs)}
            rows = {"unfiltered": dict(us_per_query=us(t_plain), results=int(want[0].sum()))}
            rows["unfiltered"]["noise_rel"] = (max(t_plain) - min(t_plain)) / float(np.median(t_plain))
            for name in filters:
                got = last[name]
                assert got[4] == blocks_in(entry, qs, name)
                rows[name] = dict(us_per_query=us(ts[name]), results=int(got[0].sum()), matches=int(got[3].sum()), blocks_decoded=int(got[4]))
            rows["all_ones_over_unfiltered_median"] = rows["all ones"]["us_per_query"]["median"] / rows["unfiltered"]["us_per_query"]["median"]
            res["ranked_" + entry] = rows
        out[wname] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
