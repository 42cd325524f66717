"""dint_queries answers `ranked_or_group_limit` and `ranked_and_group_limit` over a plain query log with a wand file, under
--facets FILE and --per-group N, with --filter FILE and --pages P as options. The tool prints totals, so what is compared is
the total of counts — the hits summed over the pages — and the JSON line's "pages", "hits", "matches", "kept", "per_group" and
"n_groups" with the binding's walk (QueryIndex.ranked_pages, itself held to the model by tests/test_gpu_group_limit.py) summed
over the log, and those with the model's (tests/group_limit.py). --per-group 1 answers what the collapsed paged type answers.
A group-limit type beside another type, without --facets or --per-group, with a --per-group out of range, and --per-group with
another type are refused with a clear error and an empty stdout."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import group_limit as GL
import paging as PG
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k


def _model_walk(every, mask, pages, group_of, n_groups, per_group):
    """-> (hits over `pages` pages of K chained by the last hit, matches, kept) of one query, from the model"""
    cur, hits = None, 0
    for _ in range(pages):
        n, sc, ids, matches, kept = GL.group_limit(every, mask, group_of, n_groups, K, per_group, cur)[:5]
        hits += n
        if n < K:
            break
        cur = PG.last_hit(n, sc, ids)
    return hits, matches, kept


def test_group_limit_types_through_the_tools(tmp_path):
    from dint_amd import device

    coll = host.synth_collection(120_000, universe=60_000, seed=47)
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
    keys = {"type", "query", "avg", "q50", "q90", "q95", "pages", "hits", "matches", "kept", "per_group", "n_groups"}
    for name, entry, conjunctive in (("ranked_or_group_limit", "or", False), ("ranked_and_group_limit", "and", True)):
        every = [GL.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        for filt, m, per_group, pages, args in ((None, None, 2, 1, []), (f, mask, 3, 3, ["--filter", "f.txt", "--pages", "3"])):
            what = (name, args)
            model = [_model_walk(e, m, pages, group_of, n_groups, per_group) for e in every]
            want_hits, want_matches, want_kept = (sum(int(w[j]) for w in model) for j in range(3))
            assert want_hits > 0 and want_kept <= want_matches and (conjunctive or want_kept < want_matches), what  # (OR: the limit cuts something)
            walk = qi.ranked_pages(entry + "_group_limit", fdd, wd, qs, k=K, filter=filt, facets=facets, per_group=per_group, max_pages=pages)
            assert sum(int(counts.sum()) for _, counts, _, _, _ in walk) == want_hits, what
            r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--facets", "g.txt", "--per-group", str(per_group), *args,
                    input=log)
            assert r.returncode == 0, r.stderr
            out = r.stdout.strip().splitlines()
            assert len(out) == 2 and int(out[0]) == 3 * want_hits, what
            line = json.loads(out[1])
            assert set(line) >= keys and "collapsed" not in line, what
            assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
            assert (line["pages"], line["hits"], line["matches"], line["kept"], line["per_group"], line["n_groups"]) == \
                (pages, want_hits, want_matches, want_kept, per_group, n_groups), what
        # --per-group 1 equals the collapsed paged type's line: the same total, and "kept" is its "collapsed"
        one = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--pages", "2", "--facets", "g.txt", "--per-group", "1", "--filter", "f.txt",
                  input=log)
        same = run(bin_("dint_queries"), t, name.replace("group_limit", "paged"), index, wand, "--runs", "2", "--pages", "2", "--facets", "g.txt",
                   "--filter", "f.txt", input=log)
        assert one.returncode == 0 and same.returncode == 0, one.stderr + same.stderr
        o_out, s_out = one.stdout.strip().splitlines(), same.stdout.strip().splitlines()
        assert o_out[0] == s_out[0] and int(o_out[0]) > 0
        o_line, s_line = json.loads(o_out[1]), json.loads(s_out[1])
        assert set(o_line) - set(s_line) == {"kept", "per_group"} and set(s_line) - set(o_line) == {"collapsed"}
        assert all(o_line[key] == s_line[key] for key in ("type", "device", "pages", "hits", "matches", "n_groups")) and o_line["kept"] == s_line["collapsed"]
        # the refusals: nothing is answered
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_group_limit:ranked_and_group_limit"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", "--facets", "g.txt", "--per-group", "2", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--per-group", "2", input=log)
        assert r.returncode != 0 and "needs --facets FILE" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--facets", "g.txt", input=log)
        assert r.returncode != 0 and "needs --per-group N" in r.stderr and r.stdout.strip() == ""
        for bad in ("0", "17"):
            r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--facets", "g.txt", "--per-group", bad, input=log)
            assert r.returncode != 0 and "--per-group is 1 to 16" in r.stderr and r.stdout.strip() == ""
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--facets", "g.txt", "--per-group", "2", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    # --per-group with another type; the refusals the tool made before stay: --pages with a type that does not page
    r = run(bin_("dint_queries"), t, "ranked_or_collapsed", index, wand, "--runs", "2", "--facets", "g.txt", "--per-group", "2", input=log)
    assert r.returncode != 0 and "--per-group goes with" in r.stderr and r.stdout.strip() == ""
    r = run(bin_("dint_queries"), t, "ranked_or", index, wand, "--runs", "2", "--pages", "2", input=log)
    assert r.returncode != 0 and "--pages goes with ranked_or_paged, ranked_and_paged, ranked_or_sorted and ranked_and_sorted only" in r.stderr
    f.close()
    facets.close()
    qi.close()
    wd.close()
