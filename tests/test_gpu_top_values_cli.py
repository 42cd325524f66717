"""dint_queries answers `ranked_or_top_values` and `ranked_and_top_values` over a plain query log with a wand file,
--values FILE and --top-values N, with --filter FILE or --value-range lo:hi as options. The tool prints totals, so what is
compared is the total of counts and the JSON line's "matches", "value_n", "distinct", "top_count_sum" and "n_top" with the
binding's outputs (QueryIndex.ranked_*_top_values_queries, themselves held to the model by tests/test_gpu_top_values.py) summed
over the log, and those with the model's (tests/top_values.py). A top-values type beside another type, without --values or
--top-values, with --pages, --order, --facets, --edges or --percentiles, a bad --top-values and --top-values with another type
are refused with a clear error and an empty stdout."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import ranked
import top_values as TV
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k


def _totals(value_counts, distinct_counts, top_n, top_counts):
    """the binding's (or the model's stacked) outputs of a log -> what the tool prints"""
    listed = np.arange(top_counts.shape[1])[None, :] < top_n[:, None]
    return int(value_counts.sum()), int(distinct_counts.sum()), int(top_counts[listed].sum(dtype=np.uint64))


def test_top_values_types_through_the_tools(tmp_path):
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
    # the values file: a hundred and fifty seller-like runs over nine tenths of the docID space, some sellers holding several runs,
    # one document far above them, and the top of the space unset — the column is shorter than the index
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 151)).astype(np.int64)
    top = int(cuts[-1])
    values = np.zeros(top, dtype=np.uint32)
    text = []
    for g in range(150):
        v = int(rs.integers(1, 60))
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], v))
        values[cuts[g]:cuts[g + 1]] = v
    text.append("%d 4000000000" % held[5])
    values[held[5]] = 4000000000
    (tmp_path / "v.txt").write_text("\n".join(text) + "\n")
    assert top < num_docs
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, top // 3, 12))]
    (tmp_path / "f.txt").write_text("\n".join("%d:%d" % x for x in runs) + "\n")
    members = set()
    for lo, hi in runs:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)
    range_mask = DV.values_mask(values, 10, 40)

    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    col = device.DocValues(0, values)
    f = qi.doc_filter(mask)
    f_range = qi.doc_filter_from_values(col, 10, 40)
    bl = ranked.BuilderLists(docids, freqs, b)
    for name, conjunctive in (("ranked_or_top_values", False), ("ranked_and_top_values", True)):
        call = qi.ranked_and_top_values_queries if conjunctive else qi.ranked_or_top_values_queries
        every = [DF.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        none, by_file, by_range = (None, None, []), (f, mask, ["--filter", "f.txt"]), (f_range, range_mask, ["--value-range", "10:40"])
        for (filt, m, filter_args), n_top in ((none, 3), (by_file, 0), (by_range, 1024)):
            what = (name, filter_args, n_top)
            got = call(fdd, wd, qs, col, n_top, filter=filt, k=K)
            want = TV.stacked([TV.top_values(e, m, values, n_top) for e in every], n_top)
            assert _totals(got[5], got[6], got[7], got[9]) == _totals(want[0], want[1], want[2], want[4]), what
            assert int(got[6].sum()) > 0 and int(got[3].sum()) >= int(got[5].sum()) >= int(got[6].sum()), what
            r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--values", "v.txt", "--top-values", str(n_top), *filter_args,
                    input=log)
            assert r.returncode == 0, r.stderr
            out = r.stdout.strip().splitlines()
            assert len(out) == 2 and int(out[0]) == 3 * int(got[0].sum()), what
            line = json.loads(out[1])
            assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "matches", "value_n", "distinct", "top_count_sum", "n_top"}, what
            assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
            assert line["matches"] == int(got[3].sum()) and line["n_top"] == n_top, what
            assert (line["value_n"], line["distinct"], line["top_count_sum"]) == _totals(got[5], got[6], got[7], got[9]), what
            if n_top == 1024:  # (more than any query has values: every valued match is listed)
                assert line["top_count_sum"] == line["value_n"], what
        # the same hits as the filtered type
        mine = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--values", "v.txt", "--top-values", "5", "--filter", "f.txt", input=log)
        same = run(bin_("dint_queries"), t, name.replace("top_values", "filtered"), index, wand, "--runs", "2", "--filter", "f.txt", input=log)
        assert mine.returncode == 0 and same.returncode == 0, mine.stderr + same.stderr
        assert mine.stdout.strip().splitlines()[0] == same.stdout.strip().splitlines()[0] and int(same.stdout.split()[0]) > 0
        # the refusals: nothing answered
        def refused(args, words, query=name):
            r = run(bin_("dint_queries"), t, query, index, wand, "--runs", "2", *args, input=log)
            assert r.returncode != 0 and words in r.stderr and r.stdout.strip() == "", (query, args, r.stderr)

        both = ["--values", "v.txt", "--top-values", "5"]
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_top_values:ranked_and_top_values"):
            refused(both, "only query type", query=mixed)
        refused(["--top-values", "5"], "needs --values FILE")
        refused(["--values", "v.txt"], "needs --top-values")
        refused(both + ["--pages", "2"], "--pages goes with")
        refused(both + ["--order", "asc"], "--order goes with")
        refused(both + ["--facets", "f.txt"], "--facets")
        refused(both + ["--edges", "1,2"], "--edges goes with")
        refused(both + ["--percentiles", "50"], "--percentiles goes with")
        refused(both + ["--filter", "f.txt", "--value-range", "1:2"], "exclude each other")
        for bad in ("", "1025", "-1", "1e1", "5.", "ten", "99999"):
            refused(["--values", "v.txt", "--top-values", bad], "--top-values")
        refused(["--top-values", "5"], "--top-values goes with", query="ranked_or")
        refused(["--values", "v.txt", "--top-values", "5"], "--top-values goes with", query=name.replace("top_values", "value_stats"))
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--values", "v.txt", "--top-values", "5", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    f_range.close()
    f.close()
    col.close()
    qi.close()
    wd.close()
