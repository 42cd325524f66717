"""dint_index_wand_data writes, from the index file and the .sizes file alone, the very bytes dint_create_wand_data writes from
the collection; and dint_queries' `ranked_or_blockmax` (the pruned call on a handle with block maxima computed from the
index at start-up) prints ranked_or's totals."""
import json
import os
import subprocess

import pytest

from dint_amd import host
from queries import reference_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_wand_file_from_the_index_and_ranked_or_blockmax(tmp_path):
    coll = host.synth_collection(400_000, universe=150_000, seed=53)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 13)
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
    r = run(bin_("dint_index_wand_data"), t, str(tmp_path / "c.index"), base + ".sizes", str(tmp_path / "i.wand"))
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["num_docs"] == num_docs and stats["sequences"] == len(coll.lens) and stats["postings"] == coll.num_postings
    want = open(tmp_path / "c.wand", "rb").read()
    assert len(want) == 24 + 4 * num_docs + 4 * len(coll.lens)
    assert open(tmp_path / "i.wand", "rb").read() == want
    # another index type than the file's, and a sizes file that is too short: refused
    r = run(bin_("dint_index_wand_data"), "multi_packed_dint", str(tmp_path / "c.index"), base + ".sizes", str(tmp_path / "x.wand"))
    assert r.returncode == 1 and "another index type" in r.stderr
    qs = reference_queries(len(coll.lens))[:120]
    log = "\n".join(" ".join(str(int(x)) for x in q) for q in qs) + "\n"
    r = run(bin_("dint_queries"), t, "ranked_or:ranked_or_blockmax", str(tmp_path / "c.index"), str(tmp_path / "i.wand"),
            "--batch", "--runs", "3", input=log)
    assert r.returncode == 0, r.stderr
    assert "Unsupported" not in r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4
    assert int(lines[0]) == int(lines[2]) > 300
    line = json.loads(lines[3])
    assert line["type"] == t and line["query"] == "ranked_or_blockmax" and line["avg"] > 0 and line["batch_us_per_query"] > 0
    # without a wand file: refused, as ranked_or_maxscore is
    r = run(bin_("dint_queries"), t, "ranked_or_blockmax:or", str(tmp_path / "c.index"), "--runs", "2", input=log)
    assert r.returncode == 0, r.stderr
    assert "Unsupported query type: ranked_or_blockmax" in r.stderr
    assert len(r.stdout.strip().splitlines()) == 2
