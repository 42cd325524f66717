"""dint_check_index, the reference's check_index tool: a written index against the collection files it was built from says
"Everything is OK!" and exits 0; against a collection with one freq changed it prints the reference's verdict for a freq
(sequence, position, GOT != EXPECTED, the sequence's length) and exits 1; another index type than the file's is refused."""
import json
import os
import subprocess

import pytest

from dint_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_tool_says_ok_and_names_the_first_wrong_freq(tmp_path):
    coll = host.synth_collection(400_000, universe=150_000, seed=53)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 13)
    b = coll.list_bounds()
    n_lists = len(coll.lens)
    num_docs = int(docids.max()) + 1
    base = str(tmp_path / "c")
    lists = [docids[int(b[i]):int(b[i + 1])] for i in range(n_lists)]
    host.write_collection(base, lists, [freqs[int(b[i]):int(b[i + 1])] for i in range(n_lists)], num_docs=num_docs)
    t = "single_packed_dint"
    bin_ = lambda name: os.path.join(ROOT, "dint_amd", "bin", name)
    run = lambda *a, **kw: subprocess.run(list(a), cwd=tmp_path, capture_output=True, text=True, timeout=900, **kw)
    index = str(tmp_path / "c.index")
    r = run(bin_("dint_create_freq_index"), t, base, index, "--threads", "4")
    assert r.returncode == 0, r.stderr

    r = run(bin_("dint_check_index"), t, index, base)
    assert r.returncode == 0, r.stderr
    assert "Everything is OK!" in r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["type"] == t and stats["sequences"] == n_lists and stats["postings"] == coll.num_postings
    assert stats["mismatches"] == 0 and "first" not in stats and stats["check_time"] > 0

    # a second collection, one freq changed in one list (a list of several blocks, behind its first block)
    seq = max(range(n_lists), key=lambda i: int(coll.lens[i]))
    assert int(coll.lens[seq]) > 600
    pos = 300
    g = int(b[seq]) + pos
    changed = freqs.copy()
    changed[g] += 5
    base2 = str(tmp_path / "d")
    host.write_collection(base2, lists, [changed[int(b[i]):int(b[i + 1])] for i in range(n_lists)], num_docs=num_docs)
    r = run(bin_("dint_check_index"), t, index, base2)
    assert r.returncode == 1
    assert "Everything is OK!" not in r.stderr
    lines = r.stderr.strip().splitlines()
    at = lines.index(f"freq in sequence {seq} differs at position {pos}!")
    assert lines[at + 1] == f"{int(freqs[g])} != {int(changed[g])}"       # GOT != EXPECTED
    assert lines[at + 2] == f"sequence length: {int(coll.lens[seq])}"
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["mismatches"] == 1
    assert stats["first"] == {"kind": "freq", "sequence": seq, "position": pos, "expected": int(changed[g]), "got": int(freqs[g])}

    # another index type than the file's
    r = run(bin_("dint_check_index"), "multi_packed_dint", index, base)
    assert r.returncode == 1 and "another index type" in r.stderr
