"""dint_queries answers `ranked_or_sorted` and `ranked_and_sorted` over a plain query log with a wand file and --values FILE:
--pages N pages of 10 hits per query in --order asc|desc, each page behind the last hit of the one before, under --filter FILE
or --value-range lo:hi as an option. The tool prints totals, so what is compared is the total of counts — the hits summed over
the pages — and the JSON line's "pages", "hits", "matches" and "order" with the binding's walk (QueryIndex.ranked_pages, itself
held to the model by tests/test_gpu_doc_values.py) summed over the log, and those with the model's (tests/doc_values.py). A
sorted type beside another type, --value-range beside --filter and a sorted type without --values are refused with a clear
error."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import ranked
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10  # the tool's top k


def _model_walk(every, mask, values, descending, pages):
    """-> (hits over `pages` pages of K chained by the last hit, matches) of one query, from the model"""
    cur, hits = None, 0
    for _ in range(pages):
        n, hv, ids, _, matches, _ = DV.sorted_page(every, mask, values, descending, cur, K)
        hits += n
        if n < K:
            break
        cur = DV.last_hit(n, hv, ids)
    return hits, matches


def test_sorted_types_through_the_tools(tmp_path):
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
    # the values file: thirty date-like runs over nine tenths of the docID space with few distinct values (ties abound), a
    # single document that a later line overrides, and the top of the space unset (value 0)
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    cuts = np.quantile(docids, np.linspace(0, 0.9, 31)).astype(np.int64)
    top = int(cuts[-1])
    values = np.zeros(top, dtype=np.uint32)
    text = []
    for g in range(30):
        v = int(rs.integers(1, 9))
        text.append("%d:%d %d" % (cuts[g], cuts[g + 1], v))
        values[cuts[g]:cuts[g + 1]] = v
    text.append("%d 4000000000" % held[5])
    values[held[5]] = 4000000000
    (tmp_path / "v.txt").write_text("\n".join(text) + "\n")
    assert top < num_docs  # (a column shorter than the index)
    # ... and a filter file: runs that begin at documents the index holds
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, top // 3, 12))]
    (tmp_path / "f.txt").write_text("\n".join("%d:%d" % x for x in runs) + "\n")
    members = set()
    for lo, hi in runs:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)
    range_mask = DV.values_mask(values, 3, 6)

    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    col = device.DocValues(0, values)
    f = qi.doc_filter(mask)
    f_range = qi.doc_filter_from_values(col, 3, 6)
    bl = ranked.BuilderLists(docids, freqs, b)
    pages = 3
    for name, entry, conjunctive in (("ranked_or_sorted", "or_sorted", False), ("ranked_and_sorted", "and_sorted", True)):
        every = [DF.every_match(bl, q, nl, num_docs, conjunctive) for q in qs]
        none, by_file, by_range = (None, None, []), (f, mask, ["--filter", "f.txt"]), (f_range, range_mask, ["--value-range", "3:6"])
        default, desc_, asc = (True, []), (True, ["--order", "desc"]), (False, ["--order", "asc"])
        for (filt, m, filter_args), orders in ((none, (default, asc)), (by_file, (desc_,)), (by_range, (asc, default))):
            for desc, order_args in orders:
                what = (name, filter_args, order_args)
                model = [_model_walk(e, m, values, desc, pages) for e in every]
                want_hits, want_matches = (sum(int(w[j]) for w in model) for j in range(2))
                one_page = sum(_model_walk(e, m, values, desc, 1)[0] for e in every)
                assert want_hits >= one_page > 0 and (conjunctive or want_hits > one_page), what
                walk = qi.ranked_pages(entry, fdd, wd, qs, k=K, filter=filt, values=col, descending=desc, max_pages=pages)
                assert sum(int(out[1].sum()) for out in walk) == want_hits, what
                r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--pages", str(pages), "--values", "v.txt",
                        *filter_args, *order_args, input=log)
                assert r.returncode == 0, r.stderr
                out = r.stdout.strip().splitlines()
                assert len(out) == 2 and int(out[0]) == 3 * want_hits, what
                line = json.loads(out[1])
                assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95", "pages", "hits", "matches", "order"}, what
                assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["batch_us_per_query"] > 0
                assert (line["pages"], line["hits"], line["matches"], line["order"]) == (pages, want_hits, want_matches, "desc" if desc else "asc"), what
        # --pages defaults to 1: as many hits as the filtered type returns
        paged = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--values", "v.txt", "--filter", "f.txt", input=log)
        same = run(bin_("dint_queries"), t, name.replace("sorted", "filtered"), index, wand, "--runs", "2", "--filter", "f.txt", input=log)
        assert paged.returncode == 0 and same.returncode == 0, paged.stderr + same.stderr
        p_out, s_out = paged.stdout.strip().splitlines(), same.stdout.strip().splitlines()
        assert p_out[0] == s_out[0] and int(p_out[0]) > 0 and json.loads(p_out[1])["pages"] == 1
        # beside another type: refused, nothing answered; the options with another type, both filters, no --values, a bad order
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_sorted:ranked_and_sorted"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", "--values", "v.txt", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, "ranked_or", index, wand, "--runs", "2", "--values", "v.txt", input=log)
        assert r.returncode != 0 and "go with ranked_or_sorted" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--values", "v.txt", "--filter", "f.txt", "--value-range", "1:2", input=log)
        assert r.returncode != 0 and "exclude each other" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input=log)
        assert r.returncode != 0 and "needs --values FILE" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--values", "v.txt", "--order", "up", input=log)
        assert r.returncode != 0 and "--order is asc or desc" in r.stderr and r.stdout.strip() == ""
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--values", "v.txt", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    f_range.close()
    f.close()
    col.close()
    qi.close()
    wd.close()
