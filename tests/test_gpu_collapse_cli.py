"""dint_queries answers `ranked_or_collapsed` and `ranked_and_collapsed` over a plain query log under the group map of
--facets FILE (lines `d g` or `lo:hi g`, later lines win), with a wand file and, as an option, --filter FILE: the tool prints
totals, so what is compared is the total of counts — the hits: at most one per group — and the JSON line's "matches" and
"collapsed" with the Python entry's (QueryIndex.ranked_*_collapsed_queries, itself held to the model by
tests/test_gpu_collapse.py) summed over the log, and those with the model's (tests/collapse.py). A collapsed type without
--facets is a usage error, and one beside another type is refused with a clear error."""
import json
import os
import subprocess

import numpy as np
import pytest

import collapse as CO
import doc_filter as DF
import facets as FA
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_collapsed_types_through_the_tools(tmp_path):
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
    # the facets file: forty site-like runs over nine tenths of the postings, single documents in a group of their own kind;
    # the top of the space is in no group
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 41)).astype(np.int64)  # (the synthetic docIDs thin out towards the top)
    top = int(cuts[-1])
    group_of = np.full(top + 40, FA.NONE, dtype=np.int64)
    text = []
    for g in range(40):
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], g))
        group_of[cuts[g]:cuts[g + 1]] = g
    for d in rs.choice(held[held < top], 200, replace=False).tolist():
        text.append("%d 41" % d)
        group_of[d] = 41
    text += ["", "%d 42" % (top + 39)]
    group_of[top + 39] = 42
    n_groups = 43
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
    for name, fn, conjunctive in (("ranked_or_collapsed", qi.ranked_or_collapsed_queries, False),
                                  ("ranked_and_collapsed", qi.ranked_and_collapsed_queries, True)):
        every = [CO.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        for filt, m, extra in ((None, None, []), (f, mask, ["--filter", "f.txt"])):
            model = [CO.collapse(e, m, group_of, n_groups, 10) for e in every]
            want_hits, want_matches, want_collapsed = (sum(int(w[j]) for w in model) for j in (0, 3, 4))
            assert 0 < want_collapsed < want_matches and want_hits > 0, (name, extra)  # (collapsing removes something)
            got = fn(fdd, wd, qs, facets, filter=filt, k=10, with_stats=True)
            assert (int(got[0].sum()), int(got[3].sum()), int(got[5].sum())) == (want_hits, want_matches, want_collapsed)
            r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--facets", "g.txt", *extra, input=log)
            assert r.returncode == 0, r.stderr
            out = r.stdout.strip().splitlines()
            assert len(out) == 2 and int(out[0]) == 3 * want_hits, name
            line = json.loads(out[1])
            assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "matches", "collapsed", "n_groups"} and "facet_totals" not in line
            assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
            assert (line["n_groups"], line["matches"], line["collapsed"]) == (n_groups, want_matches, want_collapsed), (name, extra)
        # without --facets: a usage error, nothing answered
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input=log)
        assert r.returncode != 0 and "needs --facets" in r.stderr and r.stdout.strip() == ""
        # beside another type: refused, nothing answered
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_collapsed:ranked_and_collapsed", name + ":ranked_or_faceted"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", "--facets", "g.txt", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--facets", "g.txt", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    f.close()
    facets.close()
    qi.close()
    wd.close()
