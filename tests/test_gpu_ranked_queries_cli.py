"""dint_queries answers `ranked_and` (src/queries.cpp:106-108) with a wand file written by dint_create_wand_data: the total is the
sum of min(10, matches) over the log, the stats line carries the reference's keys, and without a wand file the type is refused
as the reference refuses it."""
import json
import os
import subprocess

import pytest

from dint_amd import host
from queries import intersect, reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranked_and_through_the_tools(tmp_path):
    coll = host.synth_collection(400_000, universe=150_000, seed=43)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 9)
    b = coll.list_bounds()
    base = str(tmp_path / "c")
    num_docs = int(docids.max()) + 1
    host.write_collection(base, [docids[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))],
                          [freqs[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))], num_docs=num_docs)
    host.write_sizes(base + ".sizes", host.sizes_from_postings(docids, freqs, num_docs))
    t = "single_packed_dint"
    bin_ = lambda name: os.path.join(ROOT, "dint_amd", "bin", name)
    run = lambda *a, **kw: subprocess.run(list(a), cwd=tmp_path, capture_output=True, text=True, timeout=900, **kw)
    r = run(bin_("dint_create_freq_index"), t, base, str(tmp_path / "c.index"), "--threads", "4")
    assert r.returncode == 0, r.stderr
    r = run(bin_("dint_create_wand_data"), base, str(tmp_path / "c.wand"))
    assert r.returncode == 0, r.stderr
    qs = reference_queries(len(coll.lens))[:120]
    log = "\n".join(" ".join(str(int(x)) for x in q) for q in qs) + "\n"
    r = run(bin_("dint_queries"), t, "ranked_and:wand:maxscore", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--batch",
            "--runs", "3", input=log)
    assert r.returncode == 0, r.stderr
    assert "Unsupported query type: wand" in r.stderr and "Unsupported query type: maxscore" in r.stderr
    assert "Unsupported query type: ranked_and" not in r.stderr
    want = sum(min(10, intersect(docids, b, q)) for q in qs)
    assert want > 50
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and int(lines[0]) == 3 * want
    line = json.loads(lines[1])
    assert line["type"] == t and line["query"] == "ranked_and" and line["avg"] > 0 and line["q50"] <= line["q95"]
    assert line["batch_us_per_query"] > 0
    # without a wand file: refused, as the reference does
    r = run(bin_("dint_queries"), t, "ranked_and:and", str(tmp_path / "c.index"), "--runs", "2", input=log)
    assert r.returncode == 0, r.stderr
    assert "Unsupported query type: ranked_and" in r.stderr
    assert len(r.stdout.strip().splitlines()) == 2  # (the `and` total and its stats line)
