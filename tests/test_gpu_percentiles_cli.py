"""dint_queries answers `ranked_or_percentiles` and `ranked_and_percentiles` over a plain query log with a wand file,
--values FILE and --percentiles p1,p2,..., with --filter FILE or --value-range lo:hi as options. The tool prints totals, so what
is compared is the total of counts and the JSON line's "matches", "value_n", "per_million" and "percentile_sum" with the
binding's outputs (QueryIndex.ranked_*_percentile_queries, themselves held to the model by tests/test_gpu_percentiles.py) summed
over the log, and those with the model's (tests/percentiles.py). A percentile type beside another type, without --values or
--percentiles, with --pages, --order, --facets or --edges, a bad --percentiles list and --percentiles with another type are
refused with a clear error and an empty stdout."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import percentiles as PC
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k


def _totals(value_counts, values):
    """the binding's (or the model's stacked) counts and answers of a log -> what the tool prints"""
    return int(value_counts.sum()), values.sum(axis=0, dtype=np.uint64).tolist()


def test_percentile_types_through_the_tools(tmp_path):
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
    col = device.DocValues(0, values)
    f = qi.doc_filter(mask)
    f_range = qi.doc_filter_from_values(col, 10, 200)
    bl = ranked.BuilderLists(docids, freqs, b)
    for name, conjunctive in (("ranked_or_percentiles", False), ("ranked_and_percentiles", True)):
        call = qi.ranked_and_percentile_queries if conjunctive else qi.ranked_or_percentile_queries
        every = [DF.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        none, by_file, by_range = (None, None, []), (f, mask, ["--filter", "f.txt"]), (f_range, range_mask, ["--value-range", "10:200"])
        for (filt, m, filter_args), lists_ in ((none, ("50,90,99.9", "100,0,50,50")), (by_file, ("0.0001,99.9999,25",)), (by_range, ("50",))):
            for text_ in lists_:
                what = (name, filter_args, text_)
                percents = [float(x) for x in text_.split(",")]
                per_million = [int(round(p * 10000)) for p in percents]
                got = call(fdd, wd, qs, col, percents, filter=filt, k=K, with_stats=True)
                want = PC.stacked([PC.percentiles(e, m, values, per_million) for e in every], len(per_million))
                assert _totals(got[5], got[6]) == _totals(*want), what
                assert int(got[5].sum()) > 0 and int(got[3].sum()) >= int(got[5].sum()), what
                r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--values", "v.txt", "--percentiles", text_, *filter_args,
                        input=log)
                assert r.returncode == 0, r.stderr
                out = r.stdout.strip().splitlines()
                assert len(out) == 2 and int(out[0]) == 3 * int(got[0].sum()), what
                line = json.loads(out[1])
                assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "matches", "value_n", "per_million", "percentile_sum"}, what
                assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
                assert line["matches"] == int(got[3].sum()) and line["per_million"] == per_million, what
                assert (line["value_n"], line["percentile_sum"]) == _totals(got[5], got[6]), what
        # the same hits as the filtered type
        mine = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--values", "v.txt", "--percentiles", "50", "--filter", "f.txt", input=log)
        same = run(bin_("dint_queries"), t, name.replace("percentiles", "filtered"), index, wand, "--runs", "2", "--filter", "f.txt", input=log)
        assert mine.returncode == 0 and same.returncode == 0, mine.stderr + same.stderr
        assert mine.stdout.strip().splitlines()[0] == same.stdout.strip().splitlines()[0] and int(same.stdout.split()[0]) > 0
        # the refusals: nothing answered
        def refused(args, words, query=name):
            r = run(bin_("dint_queries"), t, query, index, wand, "--runs", "2", *args, input=log)
            assert r.returncode != 0 and words in r.stderr and r.stdout.strip() == "", (query, args, r.stderr)

        both = ["--values", "v.txt", "--percentiles", "50"]
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_percentiles:ranked_and_percentiles"):
            refused(both, "only query type", query=mixed)
        refused(["--percentiles", "50"], "needs --values FILE")
        refused(["--values", "v.txt"], "needs --percentiles")
        refused(both + ["--pages", "2"], "--pages goes with")
        refused(both + ["--order", "asc"], "--order goes with")
        refused(both + ["--facets", "f.txt"], "--facets")
        refused(both + ["--edges", "1,2"], "--edges goes with")
        refused(both + ["--filter", "f.txt", "--value-range", "1:2"], "exclude each other")
        for bad in ("", "100.0001", "1.23456", "1,,2", "-1", "1e1", ".5", "5.", "101", ",".join(str(i) for i in range(17))):
            refused(["--values", "v.txt", "--percentiles", bad], "--percentiles")
        refused(["--percentiles", "50"], "--percentiles goes with", query="ranked_or")
        refused(["--values", "v.txt", "--percentiles", "50"], "--percentiles goes with", query=name.replace("percentiles", "value_stats"))
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--values", "v.txt", "--percentiles", "50", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    f_range.close()
    f.close()
    col.close()
    qi.close()
    wd.close()
