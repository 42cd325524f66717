"""dint_queries answers `ranked_or_group_stats` and `ranked_and_group_stats` over a plain query log with a wand file, --facets
FILE and --values FILE, with --filter FILE or --value-range lo:hi as options. The tool prints totals, so what is compared is the
total of counts and the JSON line's "matches", "n_groups", "group_n", "group_sum", "group_min" and "group_max" with the model's
records (tests/group_stats.py) merged over the log — and with the binding's, themselves held to the model by
tests/test_gpu_group_stats.py. A group-stats type beside another type, without --facets or without --values, and with --pages,
--order or --edges is refused with a clear error and an empty stdout; --facets still does not go with the value-stats types."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import facets as FA
import group_stats as GS
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k
N_GROUPS = 6


def _merged(recs):
    """STATS_DTYPE[n, n_groups] of a log -> what the tool prints: (group_n, group_sum, group_min, group_max)"""
    return (recs["n"].sum(axis=0, dtype=np.uint64).tolist(), recs["sum"].sum(axis=0, dtype=np.uint64).tolist(),
            recs["min"].min(axis=0).tolist(), recs["max"].max(axis=0).tolist())


def test_group_stats_types_through_the_tools(tmp_path):
    from dint_amd import device

    coll = host.synth_collection(60_000, universe=30_000, seed=47)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 9)
    b = coll.list_bounds()
    base = str(tmp_path / "c")
    num_docs = int(docids.max()) + 1
    lists = [docids[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))]
    fr = [freqs[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))]
    sizes = host.sizes_from_postings(docids, freqs, num_docs)
    host.write_collection(base, lists, fr, num_docs=num_docs)
    host.write_sizes(base + ".sizes", sizes)
    t = "single_packed_dint"
    bin_ = lambda name: os.path.join(ROOT, "dint_amd", "bin", name)  # noqa: E731
    run = lambda *a, **kw: subprocess.run(list(a), cwd=tmp_path, capture_output=True, text=True, timeout=900, **kw)  # noqa: E731
    r = run(bin_("dint_create_freq_index"), t, base, str(tmp_path / "c.index"), "--threads", "4")
    assert r.returncode == 0, r.stderr
    r = run(bin_("dint_create_wand_data"), base, str(tmp_path / "c.wand"))
    assert r.returncode == 0, r.stderr
    index, wand = str(tmp_path / "c.index"), str(tmp_path / "c.wand")
    qs = reference_queries(len(coll.lens))[:40]
    log = "\n".join(" ".join("%d" % x for x in q) for q in qs) + "\n"
    # the values file: thirty price-like runs over nine tenths of the docID space, one document far above them, and the top of
    # the space unset — the column is shorter than the index
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 31)).astype(np.int64)
    top = int(cuts[-1])
    values = np.zeros(top, dtype=np.uint32)
    text = []
    for g in range(30):
        v = int(rs.integers(1, 300))
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], v))
        values[cuts[g]:cuts[g + 1]] = v
    text.append("%d 4000000000" % held[5])
    values[held[5]] = 4000000000
    (tmp_path / "v.txt").write_text("\n".join(text) + "\n")
    assert top < num_docs
    # the facets file: five groups of consecutive documents, a fifth of the postings each, the first forty documents of each
    # stretch in no group, and a sixth group that no document is in
    edges = np.quantile(docids, np.linspace(0, 1, N_GROUPS)).astype(np.int64)
    edges[-1] = num_docs
    group_of = np.full(num_docs, FA.NONE, dtype=np.int64)
    text = []
    for g in range(N_GROUPS - 1):
        text.append("%d:%d %d" % (edges[g] + 40, edges[g + 1], g))
        group_of[edges[g] + 40:edges[g + 1]] = g
    text.append("%d:%d %d" % (0, 0, N_GROUPS - 1))  # (an empty interval: the map has six groups)
    (tmp_path / "g.txt").write_text("\n".join(text) + "\n")
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, top // 3, 12))]
    (tmp_path / "f.txt").write_text("\n".join("%d:%d" % x for x in runs) + "\n")
    members = set()
    for lo, hi in runs:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)
    range_mask = DV.values_mask(values, 10, 200)

    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    col, x = device.DocValues(0, values), device.DocFacets(0, group_of, N_GROUPS)
    f = qi.doc_filter(mask)
    f_range = qi.doc_filter_from_values(col, 10, 200)
    bl = ranked.BuilderLists(docids, freqs, b)
    for name, conjunctive in (("ranked_or_group_stats", False), ("ranked_and_group_stats", True)):
        call = qi.ranked_and_group_stats_queries if conjunctive else qi.ranked_or_group_stats_queries
        every = [DF.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        for filt, m, filter_args in ((None, None, []), (f, mask, ["--filter", "f.txt"]), (f_range, range_mask, ["--value-range", "10:200"])):
            what = (name, filter_args)
            got = call(fdd, wd, qs, x, col, filter=filt, k=K)
            want = GS.stacked([GS.group_stats(e, m, group_of, N_GROUPS, values) for e in every], N_GROUPS)
            assert _merged(got[5]) == _merged(want) and int(want["n"].sum()) > 0 and not want["n"][:, N_GROUPS - 1].any(), what
            r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--facets", "g.txt", "--values", "v.txt", *filter_args,
                    input=log)
            assert r.returncode == 0, r.stderr
            out = r.stdout.strip().splitlines()
            assert len(out) == 2 and int(out[0]) == 3 * int(got[0].sum()), what
            line = json.loads(out[1])
            assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "matches", "n_groups", "group_n", "group_sum", "group_min", "group_max"}, what
            assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
            assert line["matches"] == int(got[3].sum()) and line["n_groups"] == N_GROUPS, what
            assert (line["group_n"], line["group_sum"], line["group_min"], line["group_max"]) == _merged(want), what
            assert line["group_min"][N_GROUPS - 1] == 0xFFFFFFFF and line["group_max"][N_GROUPS - 1] == 0  # the empty record of the empty group
        # the same hits as the filtered type
        mine = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--facets", "g.txt", "--values", "v.txt", "--filter", "f.txt", input=log)
        same = run(bin_("dint_queries"), t, name.replace("group_stats", "filtered"), index, wand, "--runs", "2", "--filter", "f.txt", input=log)
        assert mine.returncode == 0 and same.returncode == 0, mine.stderr + same.stderr
        assert mine.stdout.strip().splitlines()[0] == same.stdout.strip().splitlines()[0] and int(same.stdout.split()[0]) > 0

        # the refusals: nothing answered
        def refused(args, words, query=name):
            r = run(bin_("dint_queries"), t, query, index, wand, "--runs", "2", *args, input=log)
            assert r.returncode != 0 and words in r.stderr and r.stdout.strip() == "", (query, args, r.stderr)

        both = ["--facets", "g.txt", "--values", "v.txt"]
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_group_stats:ranked_and_group_stats"):
            refused(both, "only query type", query=mixed)
        refused(["--values", "v.txt"], "needs --facets FILE")
        refused(["--facets", "g.txt"], "needs --values FILE")
        refused([], "needs --facets FILE")
        refused(both + ["--pages", "2"], "--pages goes with")
        refused(both + ["--order", "asc"], "--order goes with")
        refused(both + ["--edges", "1,2"], "--edges goes with")
        refused(both + ["--filter", "f.txt", "--value-range", "1:2"], "exclude each other")
        # ... and what the tool refused before, word for word
        refused(both, "--facets does not go with the ranked_*_value_stats types", query=name.replace("group_stats", "value_stats"))
        refused(["--values", "v.txt"], "--values, --order and --value-range go with ranked_or_sorted and ranked_and_sorted only", query="ranked_or")
        refused(["--facets", "g.txt"], "--facets goes with the ranked_*_faceted, ranked_*_collapsed and ranked_*_paged types only", query="ranked_or")
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", *both, input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    for h in (f_range, f, x, col, qi, wd):
        h.close()
