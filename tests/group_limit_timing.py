#!/usr/bin/env python3
"""Group-limited ranked query timing: dint_ranked_or_group_limit_queries and
dint_ranked_and_group_limit_queries at k = 10 without a filter and without facet counts, over the reference log and the 500
heaviest queries of the other timing scripts (the longest lists), each as one batch and one query per call, under clustered and
striped maps of 8, 256, 257 and 4 096 groups, at per_group 1, 2, 4 and 16, from the start and with a cursor at rank 1 000 (a
query's 1 000-th match of the ungrouped ranking, its last one where it has fewer). The baseline is the COLLAPSED entry on the
same arguments, for the cursor rows the collapsed paged entry: it is timed in alternation with every row in the same process,
so that both see the same clocks, and its round-to-round spread (max - min) / median is reported as the noise the row is to be
read against. µs per query per row, medians over the rounds; the per_group = 1 answer is checked against the baseline's, byte
for byte, and a larger per_group's kept against it (never fewer documents).

    python tests/group_limit_timing.py [--postings 2e7] [--type single_packed_dint] [--rounds 5] [--single-queries N]
                                       [--logs heavy,reference] [--groups 8,256,257,4096] [--per-group 1,2,4,16] [--out profiles/x.json]

--single-queries N asks only the first N queries of a log one per call (default: all of them); the JSON says how many. A map
is 4 bytes per document. Lives under tests/ because it uses the test helpers, as tests/group_stats_timing.py does. It is not a
test and sets no threshold.
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
PER_GROUPS = (1, 2, 4, 16)
CURSOR_RANK = 1000


def clustered_map(num_docs, n_groups):
    g = np.arange(num_docs, dtype=np.uint32)
    g //= np.uint32(max(1, -(-num_docs // n_groups)))
    np.minimum(g, np.uint32(n_groups - 1), out=g)
    return g


def striped_map(num_docs, n_groups):
    g = np.arange(num_docs, dtype=np.uint32)
    g %= np.uint32(n_groups)
    return g


CELL = ("log", "entry", "map", "n_groups", "cursor", "mode", "queries", "collapsed")  # what the rows of one cell share
PER_PLACE = ("per_group", "group_limit_us_per_query", "collapsed_us_per_query", "over_collapsed", "noise_rel", "kept")


def profile_text(out):
    """The profile as it is committed: the run's description, the columns once, then a line per cell — a (log, entry, map,
    n_groups, cursor, mode) — with, behind what its rows share, a list per PER_PLACE column over the cell's per_group values."""
    head = {k: v for k, v in out.items() if k != "rows"}
    head["columns"] = list(CELL) + [c + "[]" for c in PER_PLACE]
    cells = {}
    for row in out["rows"]:
        cells.setdefault(tuple(row[c] for c in CELL), []).append(row)
    lines = [json.dumps(list(key) + [[r[c] for r in rows] for c in PER_PLACE]) for key, rows in cells.items()]
    text = json.dumps(head)
    return text[:-1] + ',\n "rows": [\n  ' + ",\n  ".join(lines) + "\n ]\n}\n"


def profile_rows(profile):
    """a committed profile -> its measured rows as dictionaries, one per (cell, per_group)"""
    out = []
    for line in profile["rows"]:
        shared = dict(zip(CELL, line))
        lists = dict(zip(PER_PLACE, line[len(CELL):]))
        out += [dict(shared, **{c: lists[c][i] for c in PER_PLACE}) for i in range(len(lists["per_group"]))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=2e7)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--single-queries", type=int, default=0)
    ap.add_argument("--logs", default="heavy,reference")
    ap.add_argument("--groups", default=",".join(str(n) for n in GROUPS))
    ap.add_argument("--per-group", default=",".join(str(n) for n in PER_GROUPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    groups = tuple(int(x) for x in args.groups.split(","))
    per_groups = tuple(int(x) for x in args.per_group.split(","))

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
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    print("index built:", coll.num_postings, "postings,", num_docs, "documents", file=sys.stderr, flush=True)
    logs = {"heavy": heavy_queries(coll.lens, 500, pool=256, max_terms=5), "reference": reference_queries(len(coll.lens))}
    logs = {name: logs[name] for name in args.logs.split(",")}
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)

    out = {"postings": coll.num_postings, "lists": len(coll.lens), "blocks": int(len(qi.blocks)), "num_docs": num_docs, "type": args.type,
           "k": 10, "rounds": args.rounds, "cursor_rank": CURSOR_RANK, "device": torch.cuda.get_device_name(0),
           "queries": {name: len(qs) for name, qs in logs.items()}, "rows": []}
    entries = {"or": (qi.ranked_or_group_limit_queries, qi.ranked_or_collapsed_queries, qi.ranked_or_collapsed_paged_queries, qi.ranked_or_filtered_queries),
               "and": (qi.ranked_and_group_limit_queries, qi.ranked_and_collapsed_queries, qi.ranked_and_collapsed_paged_queries,
                       qi.ranked_and_filtered_queries)}

    def one_by_one(call, qs, after):
        """one query per call -> the outputs joined"""
        parts = [call([q], None if after is None else [after[i]]) for i, q in enumerate(qs)]
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(len(parts[0])))

    for log_name, qs in logs.items():
        n_single = min(len(qs), args.single_queries) if args.single_queries else len(qs)
        cursors = {}
        for entry, (_, _, _, plain) in entries.items():  # the cursor at rank 1 000 of the ungrouped ranking
            counts, scores, ids = plain(fdd, wand, qs, None, k=CURSOR_RANK)
            cursors[entry] = [(scores[i, int(c) - 1], int(ids[i, int(c) - 1])) if c else None for i, c in enumerate(counts)]
        for map_name, make in (("clustered", clustered_map), ("striped", striped_map)):
            for n_groups in groups:
                g = make(num_docs, n_groups)
                facets = device.DocFacets(0, g, n_groups)
                for entry, (limited, collapsed, collapsed_paged, _) in entries.items():
                    for paged in (False, True):
                        after = cursors[entry] if paged else None
                        for mode in ("batch", "single"):
                            sub = qs if mode == "batch" else qs[:n_single]
                            sub_after = after if after is None or mode == "batch" else after[:n_single]

                            def base_call(q, a):
                                return collapsed_paged(fdd, wand, q, facets, after=a, k=10) if paged else collapsed(fdd, wand, q, facets, k=10)

                            def run(call):
                                return call(sub, sub_after) if mode == "batch" else one_by_one(call, sub, sub_after)

                            want = run(base_call)  # (warm-up, and the answer)
                            for per_group in per_groups:
                                def row_call(q, a, n=per_group):
                                    return limited(fdd, wand, q, facets, n, after=a, k=10)

                                got = run(row_call)  # (counts, scores, docids, kept, hit_groups, hit_group_matches, hit_group_ranks, skipped)
                                if per_group == 1:
                                    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[:6] + got[7:], want))
                                    assert not got[6].any()
                                assert (got[3] >= want[3]).all() and (got[6] < per_group).all()
                                t_base, t_row = [], []
                                for _ in range(args.rounds):
                                    t0 = time.perf_counter()
                                    run(base_call)
                                    t1 = time.perf_counter()
                                    run(row_call)
                                    t2 = time.perf_counter()
                                    t_base.append(t1 - t0)
                                    t_row.append(t2 - t1)
                                scale = 1e6 / len(sub)
                                row = {"log": log_name, "entry": "ranked_" + entry, "map": map_name, "n_groups": n_groups, "per_group": per_group,
                                       "cursor": paged, "mode": mode, "queries": len(sub),
                                       "group_limit_us_per_query": round(float(np.median(t_row)) * scale, 3),
                                       "collapsed_us_per_query": round(float(np.median(t_base)) * scale, 3),
                                       "over_collapsed": round(float(np.median(t_row) / np.median(t_base)), 4),
                                       "noise_rel": round((max(t_base) - min(t_base)) / float(np.median(t_base)), 4),
                                       "kept": int(got[3].sum()), "collapsed": int(want[3].sum())}
                                out["rows"].append(row)
                                print(json.dumps(row), file=sys.stderr, flush=True)
                facets.close()
                del g
        if args.out:  # (after every log: a run that is cut short leaves what it has measured)
            with open(args.out, "w") as f:
                f.write(profile_text(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
