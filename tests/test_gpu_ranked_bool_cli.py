"""dint_queries answers `ranked_bool` over a query log of prefixed tokens (+t required, -t excluded, t optional) with a wand
file: the total is the sum of the binding's counts (min(10, matches)) over the log, the stats line carries ranked_and's keys,
and the type beside another type is refused — the other types' reader parses plain integers."""
import json
import os
import subprocess

import numpy as np
import pytest

import ranked_bool as RB
from dint_amd import host
from queries import reference_queries
from test_gpu_query_fuzz import HandIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranked_bool_through_the_tools(tmp_path):
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
    must, should, exclude = RB.split_clauses(reference_queries(len(coll.lens))[:120], coll.lens)
    must, should, exclude = must + [[]], should + [[3, 3]], exclude + [[4]]  # a line without a required term
    log = "\n".join(" ".join(["+%d" % x for x in m] + ["%d" % x for x in s] + ["-%d" % x for x in e])
                    for m, s, e in zip(must, should, exclude)) + "\n"
    r = run(bin_("dint_queries"), t, "ranked_bool", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--batch", "--runs", "3",
            input=log)
    assert r.returncode == 0, r.stderr
    h = HandIndex(device, host.SINGLE_PACKED, lists, fr, num_docs, host.wand_data(sizes, docids, freqs, coll.lens)[0])
    counts = h.qi.ranked_bool_queries(h.fd, h.wand, must, should, exclude, k=10)[0]
    h.close()
    want = int(counts.sum())
    assert want > 50 and any(should) and any(exclude)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and int(lines[0]) == 3 * want
    line = json.loads(lines[1])
    assert line["type"] == t and line["query"] == "ranked_bool" and line["avg"] > 0 and line["q50"] <= line["q95"]
    assert line["batch_us_per_query"] > 0
    # beside another type: refused, nothing answered
    r = run(bin_("dint_queries"), t, "ranked_bool:and", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--runs", "2", input=log)
    assert r.returncode != 0 and "only query type" in r.stderr and r.stdout.strip() == ""
    # without a wand file: refused as ranked_and is
    r = run(bin_("dint_queries"), t, "ranked_bool", str(tmp_path / "c.index"), "--runs", "2", input=log)
    assert r.returncode == 0 and "Unsupported query type: ranked_bool" in r.stderr
    # a token that is no term
    r = run(bin_("dint_queries"), t, "ranked_bool", str(tmp_path / "c.index"), str(tmp_path / "c.wand"), "--runs", "2", input="+1 x2\n")
    assert r.returncode != 0 and "not a term token" in r.stderr
