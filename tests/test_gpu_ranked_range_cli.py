"""dint_queries answers `ranked_or_range` and `ranked_and_range` over a query log of term ids and at most one @lo:hi token a
line, with a wand file: the tool prints totals, not documents, so what is compared is the total of counts — the sum of the
model's min(10, matches in range) (tests/ranked_range.py) over the log; the stats line carries ranked_or's keys; a second
range token on a line and a ranged type beside another type are refused with a clear error."""
import json
import os
import subprocess

import numpy as np
import pytest

import ranked
import ranked_range as RR
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranged_types_through_the_tools(tmp_path):
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
    qs, ranges = RR.ranged_batch(reference_queries(len(coll.lens))[:110], num_docs)
    ranges = ranges.tolist()
    # every fourth line has no token (unrestricted); the token stands first, last or between the terms
    lines = []
    for i, (q, (lo, hi)) in enumerate(zip(qs, ranges)):
        terms = ["%d" % x for x in q]
        if i % 4 == 3:
            ranges[i] = [0, 0xFFFFFFFF]
        else:
            terms.insert((i * 7) % (len(terms) + 1), "@%d:%d" % (lo, hi))
        lines.append(" ".join(terms))
    lines += ["@5:5 1 2", "@9:3 1"]  # an empty and an inverted range
    qs, ranges = qs + [[1, 2], [1]], ranges + [[5, 5], [9, 3]]
    log = "\n".join(lines) + "\n"
    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    bl = ranked.BuilderLists(docids, freqs, b)
    index, wand = str(tmp_path / "c.index"), str(tmp_path / "c.wand")
    for name, conjunctive in (("ranked_or_range", False), ("ranked_and_range", True)):
        r = run(bin_("dint_queries"), t, name, index, wand, "--batch", "--runs", "3", input=log)
        assert r.returncode == 0, r.stderr
        want = sum(RR.top_in_range(RR.every_match(bl, q, nl, num_docs, conjunctive), lo, hi, 10)[0] for q, (lo, hi) in zip(qs, ranges))
        unranged = sum(RR.top_in_range(RR.every_match(bl, q, nl, num_docs, conjunctive), 0, 1 << 32, 10)[0] for q in qs)
        assert 20 < want < unranged, (name, want, unranged)  # (the ranges take documents out of the top 10s, and leave some)
        out = r.stdout.strip().splitlines()
        assert len(out) == 2 and int(out[0]) == 3 * want, name
        line = json.loads(out[1])
        assert set(line) >= {"type", "query", "avg", "q50", "q90", "q95"}
        assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["q50"] <= line["q95"]
        assert line["batch_us_per_query"] > 0
        # two range tokens on a line
        r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input="1 @0:10 2 @5:9\n")
        assert r.returncode != 0 and "more than one @lo:hi range" in r.stderr and r.stdout.strip() == ""
        # beside another type: refused, nothing answered
        for mixed in (name + ":or", "ranked_or:" + name, "ranked_or_range:ranked_and_range"):
            r = run(bin_("dint_queries"), t, mixed, index, wand, "--runs", "2", input=log)
            assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
        # a token that is neither, and a range without its colon
        for bad in ("1 x2\n", "1 @7\n", "1 @7:\n", "1 @:7\n", "1 @1:2:3\n", "1 @1:4294967296\n"):
            r = run(bin_("dint_queries"), t, name, index, wand, "--runs", "2", input=bad)
            assert r.returncode != 0 and "not a term id or an @lo:hi range" in r.stderr, bad
        # without a wand file: refused as ranked_or is
        r = run(bin_("dint_queries"), t, name, index, "--runs", "2", input=log)
        assert r.returncode == 0 and "Unsupported query type: " + name in r.stderr
    assert np.asarray(ranges).shape == (len(qs), 2)
