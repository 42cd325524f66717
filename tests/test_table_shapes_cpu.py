"""The reshaped tables of tests/table_shapes.py against the C oracle: every entry of every shape expects what the oracle
decodes at that entry's stream offset (integers and the bytes used; posting lists' docIDs and freqs at the block's place),
and every shape is really there — permuted, skipping bytes, repeating an in_off, overlapping — not silently empty."""
import json
import os

import numpy as np
import pytest

import fuzz_streams as F
import oracle
import table_shapes as TS

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_digests.json")))
VROOM = F.plan(*GOLDEN["vroom_plan"])
INDEX = F.index_plan(*GOLDEN["index_plan"])
QUERY = F.query_plan(*GOLDEN["query_plan"])
N_V, N_I, N_Q = GOLDEN["vroom_plan"][0], GOLDEN["index_plan"][0], GOLDEN["query_plan"][0]
# one case per dictionary kind (the GPU file runs two)
V_CASES = [VROOM[N_V * 0 + 3], VROOM[N_V * 1 + 3], VROOM[N_V * 2 + 4]]
B_CASES = [INDEX[N_I * 0 + 1], INDEX[N_I * 1 + 1], QUERY[N_Q * 2 + 1]]


def _build_blocks(case):
    return F.build_query_case(case) if case in QUERY else F.build_index_case(case)


@pytest.mark.parametrize("case", V_CASES, ids=lambda c: f"seed{c[0]}")
def test_unit_shapes_match_the_oracle(case):
    D, S = F.build_case(case)
    assert F.digest(D, S) == GOLDEN["vroom"][str(case[0])]["digest"]
    od = oracle.OracleDict(D.kind, D.file)
    shapes = TS.unit_shapes(S, D.kind, case[0])
    assert set(shapes) == set(TS.UNIT_SHAPES) | (set() if D.kind == F.MULTI else set(TS.OVERLAP_SHAPES))
    seen = {}
    for name, sh in shapes.items():
        u = sh.units
        assert len(u) >= 20, name
        assert np.array_equal(sh.want[sh.hole], np.zeros(int(sh.hole.sum()), np.uint32))
        assert sh.capacity == int(u["n"].sum()) + int(sh.hole.sum()), name
        for i, x in enumerate(u):
            key = (int(x["in_off"]), int(x["n"]))
            if key not in seen:
                seen[key] = od.decode_list(S.enc, *key)
            got, used = seen[key]
            o = int(x["out_off"])
            assert np.array_equal(sh.want[o:o + key[1]], got), f"{name}: unit {i}"
            assert int(sh.ends[i]) == key[0] + used, f"{name}: end of unit {i}"
    # the shapes are what they say
    perm = shapes["permuted"].units
    assert not np.all(np.diff(perm["in_off"].astype(np.int64)) > 0) and sorted(perm["in_off"]) == sorted(S.units["in_off"])
    assert np.all(np.diff(shapes["reversed"].units["in_off"].astype(np.int64)) < 0)
    for name in ("every_other_list", "random_subset"):
        sh = shapes[name]
        assert not sh.hole.any() and (sh.units["in_off"][1:] > sh.ends[:-1]).any(), f"{name} skips no stream bytes"
    sc = shapes["scattered"]
    assert sc.hole.sum() > len(sc.units) // 2
    after = sc.units["out_off"] + sc.units["n"]
    touching = np.isin(sc.units["out_off"], after)  # outputs that follow another unit's output without a hole ...
    order = np.argsort(sc.units["out_off"])
    prev = np.empty(len(order), np.int64)
    prev[order[1:]] = order[:-1]
    assert (touching & (prev != np.arange(len(prev)) - 1)).sum() >= 3  # ... that is not its stream neighbour
    rep = shapes["repeated"].units
    assert np.array_equal(rep["in_off"][0::2], rep["in_off"][1::2])
    assert np.array_equal(rep["out_off"][1::2], rep["out_off"][0::2] + rep["n"][0::2])
    mixed = shapes["mixed"].units
    whole = np.isin(mixed["in_off"], [l[0] for l in S.lists]) & np.isin(mixed["n"], [l[1] for l in S.lists])
    assert whole.sum() >= 20 and (~whole).sum() >= 20
    if D.kind != F.MULTI:
        sh = shapes["overlapping"]
        pairs = TS.overlap_pairs(sh)
        assert len(pairs) >= 10
        u = sh.units
        assert (u["n"][pairs] <= 256).all()
        true_len = sh.ends[pairs] - u["in_off"][pairs]
        assert (u["in_off"][pairs + 1] - u["in_off"][pairs] < true_len).all()
        assert np.array_equal(u["out_off"][pairs + 1], u["out_off"][pairs] + u["n"][pairs])
        # the one shape outside dint_decode_units' contract, and exactly at the whole lists of its pairs
        cut = TS.cut_into(sh)
        assert np.array_equal(np.flatnonzero(cut), pairs)
    for name, sh in shapes.items():
        assert name == "overlapping" or not TS.cut_into(sh).any(), name


@pytest.mark.parametrize("case", B_CASES, ids=lambda c: f"seed{c[0]}")
def test_block_shapes_match_the_oracle(case):
    Dd, Df, X = _build_blocks(case)
    od, of = oracle.OracleDict(Dd.kind, Dd.file), oracle.OracleDict(Df.kind, Df.file)
    lists = [oracle.posting_list_decode(od, of, X.index, int(X.offsets[i])) for i in range(len(X.offsets) - 1)]
    blocks = TS.block_table(X)
    assert int(blocks["n"].sum()) == len(X.docids) and np.array_equal(np.unique(blocks["list"]), np.arange(len(lists)))
    shapes = TS.block_shapes(X, blocks, case[0])
    assert set(shapes) == set(TS.BLOCK_SHAPES)
    for name, sh in shapes.items():
        t = sh.blocks
        assert len(t) >= 10, name
        assert sh.capacity == int(t["n"].sum()) + int(sh.hole.sum()), name
        for i, x in enumerate(t):
            d, f = lists[int(x["list"])]
            b = int(np.searchsorted(d[255::256] if len(d) >= 256 else d[:0], int(x["max"])))  # the block whose max this is
            lo, n, o = 256 * b, int(x["n"]), int(x["out_off"])
            assert d[min(len(d), lo + n) - 1] == x["max"] and (lo == 0 or d[lo - 1] + 1 == x["base"]) and (lo or x["base"] == 0)
            assert np.array_equal(sh.docids[o:o + n], d[lo:lo + n]), f"{name}: block {i}"
            assert np.array_equal(sh.freqs[o:o + n], f[lo:lo + n]), f"{name}: block {i}"
    # the shapes are what they say
    n_lists = len(lists)
    lp = shapes["lists_permuted"].blocks["list"]
    firsts = lp[np.r_[True, lp[1:] != lp[:-1]]]
    assert len(firsts) == n_lists and not np.all(np.diff(firsts.astype(np.int64)) > 0)
    sub = np.unique(shapes["lists_subset"].blocks["list"])
    assert 2 <= len(sub) < n_lists
    assert np.all(np.diff(shapes["blocks_reversed"].blocks["in_off"].astype(np.int64)) < 0)
    assert sorted(shapes["blocks_permuted"].blocks["in_off"]) == sorted(blocks["in_off"])
    rep = shapes["blocks_repeated"].blocks
    assert np.array_equal(rep["in_off"][0::2], rep["in_off"][1::2]) and (rep["out_off"][1::2] != rep["out_off"][0::2]).all()
    assert shapes["blocks_scattered"].hole.sum() > len(blocks) // 2
    assert (shapes["short_only"].blocks["n"] < 256).all() and (shapes["full_only"].blocks["n"] == 256).all()
