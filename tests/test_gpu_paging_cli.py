"""dint_queries answers `ranked_or_paged` and `ranked_and_paged` over a plain query log with a wand file: --pages N pages of
10 hits per query, each page behind the last hit of the one before, under --filter FILE as an option and, with --facets FILE,
through the collapsed paged entries. The tool prints totals, so what is compared is the total of counts — the hits summed over
the pages — and the JSON line's "pages", "hits", "matches" (and "collapsed") with the binding's walk
(QueryIndex.ranked_pages, itself held to the model by tests/test_gpu_paging.py) summed over the log, and those with the
model's (tests/paging.py). --pages 1 answers what the filtered type answers: the same total and the shared keys. A paged type
beside another type, and --pages with another type, are refused with a clear error."""
import json
import os
import subprocess

import numpy as np
import pytest

import collapse as CO
import doc_filter as DF
import facets as FA
import paging as PG
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k


def _model_walk(every, mask, pages, group_of=None, n_groups=0):
    """-> (hits over `pages` pages of K chained by the last hit, matches, collapsed) of one query, from the model"""
    cur, hits = None, 0
    for _ in range(pages):
        if group_of is None:
            n, sc, ids, matches, _ = PG.page_after(every, mask, cur, K)
            collapsed = 0
        else:
            n, sc, ids, matches, collapsed = PG.collapsed_page_after(every, mask, group_of, n_groups, cur, K)[:5]
        hits += n
        if n < K:
            break
        cur = PG.last_hit(n, sc, ids)
    return hits, matches, collapsed


def test_paged_types_through_the_tools(tmp_path):
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
    qs = reference_queries(len(coll.lens))[:60]
    log = "\n".join(" ".join("%d" % x for x in q) for q in qs) + "\n"
    # the facets file: forty site-like runs over nine tenths of the postings; the top of the space is in no group
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 41)).astype(np.int64)
    top = int(cuts[-1])
    group_of = np.full(top, FA.NONE, dtype=np.int64)
    text = []
    for g in range(40):
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], g))
        group_of[cuts[g]:cuts[g + 1]] = g
    n_groups = 40
    (tmp_path / "g.txt").write_text("\n".join(text) + "\n")
    # ... and a filter file: runs that begin at documents the index holds, wide enough to hold some of the log's 40
    # conjunctive matches
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, top // 3, 12))]
    (tmp_path / "f.txt").write_text("\n".join("%d:%d" % x for x in runs) + "\n")
    members = set()
    for lo, hi in runs:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)

    # the binding and the model over the same index, norm_lens, map and filter
    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    facets = device.DocFacets(0, group_of, n_groups)
    f = qi.doc_filter(mask)
    bl = ranked.BuilderLists(docids, freqs, b)
    pages = 3
    for name, entry, conjunctive in (("ranked_or_paged", "or", False), ("ranked_and_paged", "and", True)):
        every = [CO.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        for filt, m, filter_args in ((None, None, []), (f, mask, ["--filter", "f.txt"])):
            for x, g, facet_args in ((None, None, []), (facets, group_of, ["--facets", "g.txt"])):
                what = (name, filter_args, facet_args)
                model = [_model_walk(e, m, pages, g, n_groups) for e in every]
                want_hits, want_matches, want_collapsed = (sum(int(w[j]) for w in model) for j in range(3))
                one_page = sum(_model_walk(e, m, 1, g, n_groups)[0] for e in every)
                assert want_hits >= one_page > 0 and (conjunctive or want_hits > one_page), what  # (OR: the later pages hold something)
                walk = qi.ranked_pages(entry + ("_collapsed" if x is not None else ""), fdd, wd, qs, k=K, filter=filt, facets=x, max_pages=pages)
                assert sum(int(counts.sum()) for _, counts, _, _, _ in walk) == want_hits, what
                r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--pages", str(pages), *filter_args, *facet_args,
                        input=log)
                assert r.returncode == 0, r.stderr
                out = r.stdout.strip().splitlines()
                assert len(out) == 2 and int(out[0]) == 3 * want_hits, what
                line = json.loads(out[1])
                assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "pages", "hits", "matches"}, what
                assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
                assert (line["pages"], line["hits"], line["matches"]) == (pages, want_hits, want_matches), what
                if x is not None:
                    assert (line["collapsed"], line["n_groups"]) == (want_collapsed, n_groups), what
                    assert want_collapsed <= want_matches and (conjunctive or want_collapsed < want_matches), what  # (OR: collapsing removes something)
                else:
                    assert "collapsed" not in line and "n_groups" not in line
        # --pages 1 equals the filtered type's line on the shared keys: the same total, type and the same keys besides its own
        paged = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--pages", "1", "--filter", "f.txt", input=log)
        same = run(bin_("dint_queries"), t, name.replace("paged", "filtered"), index, wand, "--runs", "2", "--filter", "f.txt", input=log)
        assert paged.returncode == 0 and same.returncode == 0, paged.stderr + same.stderr
        p_out, s_out = paged.stdout.strip().splitlines(), same.stdout.strip().splitlines()
        assert p_out[0] == s_out[0] and int(p_out[0]) > 0
        p_line, s_line = json.loads(p_out[1]), json.loads(s_out[1])
        assert set(p_line) - set(s_line) == {"pages", "hits", "matches"} and set(s_line) <= set(p_line)
        assert (p_line["type"], p_line["device"], p_line["pages"]) == (s_line["type"], s_line["device"], 1) and 2 * p_line["hits"] == int(s_out[0])
        # beside another type: refused, nothing answered; --pages with another type too
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_paged:ranked_and_paged"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, "ranked_or", index, wand, "--runs", "2", "--pages", "2", input=log)
        assert r.returncode != 0 and "--pages goes with" in r.stderr and r.stdout.strip() == ""
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    f.close()
    facets.close()
    qi.close()
    wd.close()
