"""dint_queries answers `ranked_or_bool` over a query log of tokens (t optional, -t excluded, ~m the line's minimum) with a wand
file: the tool prints totals, not documents, so what is compared is the total of counts — it equals the sum of the model's
counts (min(10, matches), tests/ranked_or_bool.py) over the log; the stats line carries ranked_and's keys, and a required term
(+t), the type beside another type and a second ~m are refused."""
import json
import os
import subprocess

import pytest

import ranked
import ranked_or_bool as ROB
from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranked_or_bool_through_the_tools(tmp_path):
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
    should, exclude, mins = ROB.derive_clauses(reference_queries(len(coll.lens))[:120], coll.lens)
    should, exclude, mins = should + [[]], exclude + [[4]], mins + [1]  # a line of excluded terms only
    # (~m where the derivation sets one other than 1; a line without it: 1)
    log = "\n".join(" ".join(["%d" % x for x in s] + ["-%d" % x for x in e] + (["~%d" % m] if m != 1 else []))
                    for s, e, m in zip(should, exclude, mins)) + "\n"
    r = run(bin_("dint_queries"), t, "ranked_or_bool", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--batch", "--runs", "3",
            input=log)
    assert r.returncode == 0, r.stderr
    nl = host.wand_data(sizes, docids, freqs, coll.lens)[0]
    counts = ROB.model_batch(ranked.BuilderLists(docids, freqs, b), should, exclude, mins, nl, num_docs, 10)[0]
    want = int(counts.sum())
    assert want > 50 and any(exclude) and max(mins) >= 2
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and int(lines[0]) == 3 * want
    line = json.loads(lines[1])
    assert line["type"] == t and line["query"] == "ranked_or_bool" and line["avg"] > 0 and line["q50"] <= line["q95"]
    assert line["batch_us_per_query"] > 0
    # a required term: that query is ranked_bool's
    r = run(bin_("dint_queries"), t, "ranked_or_bool", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--runs", "2", input="1 +2\n")
    assert r.returncode != 0 and "no required terms" in r.stderr and r.stdout.strip() == ""
    # beside another type: refused, nothing answered
    r = run(bin_("dint_queries"), t, "ranked_or_bool:or", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--runs", "2", input=log)
    assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
    # without a wand file: refused as ranked_and is
    r = run(bin_("dint_queries"), t, "ranked_or_bool", str(tmp_path / "c.index"), "--runs", "2", input=log)
    assert r.returncode == 0 and "Unsupported query type: ranked_or_bool" in r.stderr
    # a token that is no term, and a second minimum
    for bad in ("1 x2\n", "1 2 ~1 ~2\n"):
        r = run(bin_("dint_queries"), t, "ranked_or_bool", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--runs", "2", input=bad)
        assert r.returncode != 0 and "not a term token" in r.stderr
