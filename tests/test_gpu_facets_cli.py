"""dint_queries answers `ranked_or_faceted` and `ranked_and_faceted` over a plain query log under the group map of
--facets FILE (lines `d g` or `lo:hi g`, later lines win), with a wand file and, as an option, --filter FILE: the tool prints
totals, so what is compared is the total of counts with the Python entry's (QueryIndex.ranked_*_faceted_queries, itself
held to the model by tests/test_gpu_facets.py), and the JSON line's "matches", "n_groups" and "facet_totals" with the model's
(tests/facets.py) summed over the log. A faceted type without --facets is a usage error, and one beside another type is
refused with a clear error."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_faceted_types_through_the_tools(tmp_path):
    from dint_amd import device

    coll = host.synth_collection(120_000, universe=60_000, seed=43)
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
    qs = reference_queries(len(coll.lens))[:110]
    log = "\n".join(" ".join("%d" % x for x in q) for q in qs) + "\n"
    # the facets file: intervals (seven site-like runs, each a tenth and more of the postings), single documents that
    # override them, a later interval that overrides both, blank and empty lines; the top of the space is in no group
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 8)).astype(np.int64)  # (the synthetic docIDs thin out towards the top)
    top = int(cuts[-1])
    group_of = np.full(top + 40, FA.NONE, dtype=np.int64)
    text = []
    for g in range(7):
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], g))
        group_of[cuts[g]:cuts[g + 1]] = g
    for d in rs.choice(held[held < top], 200, replace=False).tolist():
        text.append("%d 8" % d)
        group_of[d] = 8
    text += ["", "  ", "7:7 3", "%d:%d 2" % (cuts[1] - 10, cuts[1] + 10), "%d 9" % (top + 39)]
    group_of[cuts[1] - 10:cuts[1] + 10] = 2
    group_of[top + 39] = 9
    n_groups = 10
    (tmp_path / "g.txt").write_text("\n".join(text) + "\n")
    # ... and a filter file: runs that begin at documents the index holds
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, top // 40, 12))]
    (tmp_path / "f.txt").write_text("\n".join("%d:%d" % x for x in runs) + "\n")
    members = set()
    for lo, hi in runs:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)

    # the Python entry and the model over the same index, norm_lens, map and filter
    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    facets = device.DocFacets(0, group_of, n_groups)
    f = qi.doc_filter(mask)
    bl = ranked.BuilderLists(docids, freqs, b)
    for name, fn, conjunctive in (("ranked_or_faceted", qi.ranked_or_faceted_queries, False),
                                  ("ranked_and_faceted", qi.ranked_and_faceted_queries, True)):
        every = [FA.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        for filt, m, extra in ((None, None, []), (f, mask, ["--filter", "f.txt"])):
            inside = [FA.matches_in(e, m) for e in every]
            want_rows = np.sum([FA.row_of(group_of, n_groups, ids)[0].astype(np.int64) for ids in inside], axis=0)
            want_matches = sum(int(ids.size) for ids in inside)
            assert np.count_nonzero(want_rows) >= 2 and want_matches > want_rows.sum(), (name, want_rows)  # (several groups, and matches in none)
            want = int(fn(fdd, wd, qs, facets, filter=filt, k=10)[0].sum())
            r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--facets", "g.txt", *extra, input=log)
            assert r.returncode == 0, r.stderr
            out = r.stdout.strip().splitlines()
            assert len(out) == 2 and int(out[0]) == 3 * want, name
            line = json.loads(out[1])
            assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "matches", "n_groups", "facet_totals"}
            assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
            assert line["n_groups"] == n_groups and line["facet_totals"] == want_rows.tolist() and line["matches"] == want_matches, (name, extra)
        # without --facets: a usage error, nothing answered
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input=log)
        assert r.returncode != 0 and "needs --facets" in r.stderr and r.stdout.strip() == ""
        # beside another type: refused, nothing answered
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_faceted:ranked_and_faceted"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", "--facets", "g.txt", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        # a line that is not `d g` or `lo:hi g`; a file that is not there
        (tmp_path / "bad.txt").write_text("5 1\n7\n")
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--facets", "bad.txt", input=log)
        assert r.returncode != 0 and "not a `d g` or `lo:hi g` line" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--facets", "none.txt", input=log)
        assert r.returncode != 0 and "could not open the facets file" in r.stderr
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--facets", "g.txt", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    # --facets with another type
    r = run(bin_("dint_queries"), t, "ranked_or", index, wand, "--runs", "2", "--facets", "g.txt", input=log)
    assert r.returncode != 0 and "--facets goes with" in r.stderr
    f.close()
    facets.close()
    qi.close()
    wd.close()
