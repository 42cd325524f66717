"""dint_queries answers `or` and `or_freq` (src/queries.cpp:96-103) on an index the project's own tools wrote: the totals are
the set union's, the stats lines carry the reference's keys, and the ranked types are still refused."""
import json
import os
import subprocess

import numpy as np
import pytest

from dint_amd import host
from or_union import union
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {host.SINGLE_PACKED: ("single_packed_dint", "single_packed"), host.MULTI_PACKED: ("multi_packed_dint", "multi_packed")}


@pytest.mark.parametrize("kind", list(TYPES))
def test_or_query_types_through_the_tools(tmp_path, kind):
    coll = host.synth_collection(400_000, universe=150_000, seed=43)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 9)
    b = coll.list_bounds()
    base = str(tmp_path / "c")
    host.write_collection(base, [docids[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))],
                          [freqs[int(b[i]):int(b[i + 1])] for i in range(len(coll.lens))], num_docs=int(docids.max()) + 1)
    t, _ = TYPES[kind]
    bin_ = lambda name: os.path.join(ROOT, "dint_amd", "bin", name)
    run = lambda *a, **kw: subprocess.run(list(a), cwd=tmp_path, capture_output=True, text=True, timeout=900, **kw)
    r = run(bin_("dint_create_freq_index"), t, base, str(tmp_path / "c.index"), "--threads", "4")
    assert r.returncode == 0, r.stderr
    qs = reference_queries(len(coll.lens))[:120]
    log = "\n".join(" ".join(str(int(x)) for x in q) for q in qs) + "\n"
    r = run(bin_("dint_queries"), t, "or:or_freq:wand", str(tmp_path / "c.index"), "--runs", "3", "--batch", input=log)
    assert r.returncode == 0, r.stderr
    assert "Unsupported query type: wand" in r.stderr  # src/queries.cpp:108-110
    want = sum(union(docids, b, q) for q in qs)
    assert want > 10_000
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and int(lines[0]) == 3 * want and int(lines[2]) == 3 * want
    for text, name in ((lines[1], "or"), (lines[3], "or_freq")):
        line = json.loads(text)
        assert line["type"] == t and line["query"] == name and line["avg"] > 0 and line["q50"] <= line["q95"]
        assert set(("type", "query", "avg", "q50", "q90", "q95")) <= set(line) and line["batch_us_per_query"] > 0
