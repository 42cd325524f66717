"""dint_queries answers `ranked_or_filtered` and `ranked_and_filtered` over a plain query log under the document filter of
--filter FILE (lines `d` or `lo:hi`, their union), with a wand file: the tool prints totals, not documents, so what is
compared is the total of counts with the Python entry's over the same filter (QueryIndex.ranked_*_filtered_queries, itself
held to the model by tests/test_gpu_doc_filter.py); the stats line carries ranked_or's keys; a filtered type without
--filter is a usage error, and one beside another type is refused with a clear error."""
import json
import os
import subprocess

import numpy as np
import pytest

import doc_filter as DF
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filtered_types_through_the_tools(tmp_path):
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
    # the filter file: single docIDs, intervals, overlapping, empty and blank lines — documents the index holds and runs
    # that begin at one (the synthetic docIDs thin out towards the top of their space: a uniform draw would match little)
    rs = np.random.default_rng(8)
    held = np.unique(docids)
    singles = rs.choice(held, 300, replace=False).tolist()
    runs = [(int(lo), int(lo) + int(w)) for lo, w in zip(rs.choice(held, 12), rs.integers(1, num_docs // 150, 12))]
    text = [str(d) for d in singles[:150]] + ["%d:%d" % x for x in runs] + ["", "7:7", "9:3"] + [str(d) for d in singles[150:]]
    text += ["%d:%d" % (runs[0][0] + 1, runs[0][1] + 5), str(singles[0])]
    (tmp_path / "f.txt").write_text("\n".join(text) + "\n")
    members = set(singles)
    for lo, hi in runs + [(runs[0][0] + 1, runs[0][1] + 5)]:
        members.update(range(lo, hi))
    mask = DF.as_mask(sorted(members), max(members) + 1)

    # the Python entry over the same index, norm_lens and filter
    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    dd = host.build_dictionary(host.SINGLE_PACKED, coll)
    fd = host.build_dictionary(host.SINGLE_PACKED, host.Collection(freqs - 1, coll.lens))
    idx, offs = host.build_index(host.SINGLE_PACKED, dd, fd, docids, freqs, coll.lens)
    qi, fdd, wd = device.QueryIndex(device.Dictionary(host.SINGLE_PACKED, dd), idx, offs), device.Dictionary(host.SINGLE_PACKED, fd), device.WandData(nl)
    f = qi.doc_filter(mask)
    assert f.info.n_set == len(members)
    for name, fn, plain in (("ranked_or_filtered", qi.ranked_or_filtered_queries, qi.ranked_or_queries),
                            ("ranked_and_filtered", qi.ranked_and_filtered_queries, qi.ranked_and_queries)):
        want = int(fn(fdd, wd, qs, f, k=10)[0].sum())
        unfiltered = int(plain(fdd, wd, qs, k=10)[0].sum())
        assert 20 < want < unfiltered, (name, want, unfiltered)  # (the filter takes documents out of the top 10s, and leaves some)
        r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", "--filter", "f.txt", input=log)
        assert r.returncode == 0, r.stderr
        out = r.stdout.strip().splitlines()
        assert len(out) == 2 and int(out[0]) == 3 * want, name
        line = json.loads(out[1])
        assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95"}
        assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["q50"] <= line["q95"]
        assert line["batch_us_per_query"] > 0
        # an empty filter file: nothing matches
        (tmp_path / "empty.txt").write_text("\n")
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--filter", "empty.txt", input=log)
        assert r.returncode == 0 and int(r.stdout.strip().splitlines()[0]) == 0, r.stderr
        # without --filter: a usage error, nothing answered
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input=log)
        assert r.returncode != 0 and "needs --filter" in r.stderr and r.stdout.strip() == ""
        # beside another type: refused, nothing answered
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_filtered:ranked_and_filtered"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", "--filter", "f.txt", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        # a line that is neither a docID nor an interval; a file that is not there
        (tmp_path / "bad.txt").write_text("5\nx7\n")
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--filter", "bad.txt", input=log)
        assert r.returncode != 0 and "not a docID or a lo:hi interval" in r.stderr and r.stdout.strip() == ""
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", "--filter", "none.txt", input=log)
        assert r.returncode != 0 and "could not open the filter file" in r.stderr
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", "--filter", "f.txt", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    # --filter with another type
    r = run(bin_("dint_queries"), t, "ranked_or", index, wand, "--runs", "2", "--filter", "f.txt", input=log)
    assert r.returncode != 0 and "--filter goes with" in r.stderr
    f.close()
    qi.close()
    wd.close()
