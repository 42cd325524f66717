"""Document-filter ranked queries without a GPU: the entries in the header, the library and the
binding; the model (tests/doc_filter.py) against a brute-force filter of the union / the intersection on tiny indexes;
live_blocks against a per-docID loop; the binding's three input forms; the parser of dint_queries' --filter files
(tools/doc_filter_file.hpp, compiled alone with g++); and the shares that tests/test_gpu_doc_filter_fuzz.py demands of its
committed seeds, from the model alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import doc_filter as DF
import ranked
import ranked_or
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER = os.path.join(ROOT, "tools", "doc_filter_file.hpp")
HANDLE = ("dint_doc_filter_create", "dint_doc_filter_info_get", "dint_doc_filter_destroy")
ENTRIES = ("dint_ranked_or_filtered_queries", "dint_ranked_and_filtered_queries")


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "typedef struct dint_doc_filter dint_doc_filter;" in header and "} dint_doc_filter_info;" in header
    for name in HANDLE + ENTRIES:
        assert f" {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
    for name in ENTRIES:
        assert hasattr(device.QueryIndex, name[len("dint_"):])
    assert hasattr(device.QueryIndex, "doc_filter") and hasattr(device.DocFilter, "info") and hasattr(device.DocFilter, "close")
    assert [f[0] for f in device.DocFilterInfo._fields_] == ["num_docs", "n_set", "n_blocks", "live_blocks"]


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    counts = np.full(1, 77, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for name in ENTRIES:
        call = getattr(device._lib, name)
        for qi, fd, w, k, cnt in ((None, fake, fake, 10, counts), (fake, None, fake, 10, counts), (fake, fake, None, 10, counts),
                                  (fake, fake, fake, 0, counts), (fake, fake, fake, 1025, counts), (fake, fake, fake, 10, None)):
            for filt in (None, fake):
                assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, filt, 1, cnt.ctypes.data if cnt is not None else None, None,
                            scores.ctypes.data, None, C.byref(blocks), None) == -1
                assert counts[0] == 77 and blocks.value == 77 and not scores.any()  # nothing is written
    h = C.c_void_p(77)
    word = np.zeros(1, dtype=np.uint64)
    assert device._lib.dint_doc_filter_create(None, word.ctypes.data, 10, C.byref(h)) == -1
    assert device._lib.dint_doc_filter_create(fake, word.ctypes.data, 10, None) == -1
    assert device._lib.dint_doc_filter_create(fake, None, 10, C.byref(h)) == -1
    assert device._lib.dint_doc_filter_create(fake, word.ctypes.data, 1 << 32, C.byref(h)) == -1
    assert device._lib.dint_doc_filter_info_get(None, C.byref(device.DocFilterInfo())) == -1
    device._lib.dint_doc_filter_destroy(None)


def test_the_binding_packs_masks_words_and_docids_alike():
    from dint_amd import device

    r = np.random.default_rng(2)
    for n in (0, 1, 63, 64, 65, 1000):
        mask = r.random(n) < 0.4
        words, num_docs = device.doc_filter_words(mask)
        assert num_docs == n and words.dtype == np.uint64 and words.size == (n + 63) // 64
        assert all(bool((int(words[d >> 6]) >> (d & 63)) & 1) == bool(mask[d]) for d in range(n))
        again, n2 = device.doc_filter_words(words, n)
        ids, n3 = device.doc_filter_words(np.flatnonzero(mask), n)
        assert n2 == n3 == n and np.array_equal(again, words) and np.array_equal(ids, words)
    assert device.doc_filter_words([3, 70, 3])[1] == 71 and device.doc_filter_words([])[1] == 0
    words, n = device.doc_filter_words([3, 70, 200], 100)  # (docIDs at or past num_docs are left out)
    assert n == 100 and words.tolist() == [8, 64]
    # docIDs that happen to be u64 are not taken for words: refused by their count, or named
    with pytest.raises(ValueError):
        device.doc_filter_words(np.array([3, 70, 99], dtype=np.uint64), 100)
    assert device.doc_filter_words(np.array([3, 70, 200], dtype=np.uint64), 100, form="docids")[0].tolist() == [8, 64]
    assert device.doc_filter_words(np.array([3, 70], dtype=np.uint64), form="docids")[1] == 71
    assert device.doc_filter_words([1, 0, 1], form="mask")[0].tolist() == [5]
    assert device.doc_filter_words(np.ones(10, dtype=bool), 4)[0].tolist() == [15]
    assert device.doc_filter_words(np.ones(4, dtype=bool), 70)[0].tolist() == [15, 0]


# ---- the model against brute force on tiny indexes --------------------------------------------------------------------
def _tiny(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 6, x.size).astype(np.uint32) for x in lists]
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    return r, ranked.BuilderLists(docids, fr, bounds), nl, num_docs, lists


@pytest.mark.parametrize("conjunctive", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_brute_force_filter(seed, conjunctive):
    r, lists, nl, num_docs, raw = _tiny(seed)
    model = ranked.ranked_and if conjunctive else ranked_or.ranked_or
    seen = 0
    for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], [2, 0]):
        sets = [set(raw[t].tolist()) for t in q]
        docs = set.intersection(*sets) if conjunctive else set.union(*sets)
        full = model(lists, q, nl, num_docs, max(1, len(docs)))
        score_of = dict(zip(full[2][:full[0]].tolist(), bits(full[1][:full[0]]).tolist()))
        assert set(score_of) == docs
        every = DF.every_match(lists, q, nl, num_docs, conjunctive)
        for n_mask in (num_docs, num_docs // 2, num_docs + 50, 0):  # the filter's num_docs: at, below, above, none
            for density in (0.5, 0.05, 1.0):
                mask = r.random(n_mask) < density
                inside = sorted(d for d in docs if d < n_mask and mask[d])
                for k in (1, 10, 1000):
                    n, sc, ids, matches = DF.top_in_filter(every, mask, k)
                    assert matches == len(inside) and n == min(k, matches)
                    order = sorted(inside, key=lambda d: (-float(np.uint32(score_of[d]).view(np.float32)), d))[:k]
                    assert ids[:n].tolist() == order and bits(sc[:n]).tolist() == [score_of[d] for d in order]
                    assert (ids[n:] == 0xFFFFFFFF).all() and not sc[n:].any()
                seen += matches
    assert seen > 100


def test_live_blocks_is_the_per_docid_rule():
    r = np.random.default_rng(9)
    table = np.zeros(0, dtype=[("base", "<u4"), ("max", "<u4"), ("list", "<u4")])
    for t in range(4):  # four lists of blocks that tile [0, the list's last docID]
        maxima = np.sort(r.choice(600, int(r.integers(1, 9)), replace=False))
        rec = np.zeros(maxima.size, dtype=table.dtype)
        rec["max"], rec["base"], rec["list"] = maxima, np.concatenate([[0], maxima[:-1] + 1]), t
        table = np.concatenate([table, rec])
    some_dead = some_live = 0
    for n_mask in (0, 1, 64, 300, 599, 600, 601, 900):
        for density in (0.0, 0.01, 0.1, 1.0):
            mask = r.random(n_mask) < density
            want = [any(d < n_mask and mask[d] for d in range(int(b["base"]), int(b["max"]) + 1)) for b in table]
            got = DF.live_blocks(table, mask)
            assert got.tolist() == want, (n_mask, density)
            words = np.packbits(np.concatenate([mask, np.ones(-n_mask % 64, dtype=bool)]), bitorder="little").view("<u8")  # (garbage past the end)
            assert DF.live_blocks_words(table, words, n_mask).tolist() == want, (n_mask, density)
            some_live += int(got.sum())
            some_dead += int((~got).sum())
            for t in range(4):  # ... and a query's blocks_decoded is their count, OR over the distinct terms, AND the rarest
                assert DF.planned_blocks(table, got, [5, 5, 2, 9], [t, t], False) == sum(w for w, b in zip(want, table) if b["list"] == t)
            assert DF.planned_blocks(table, got, [5, 5, 2, 9], [0, 1, 2], True) == sum(w for w, b in zip(want, table) if b["list"] == 2)
            assert DF.planned_blocks(table, got, [5, 5, 2, 9], [1, 0], True) == sum(w for w, b in zip(want, table) if b["list"] == 0)
    assert some_dead > 50 and some_live > 50
    assert DF.planned_blocks(table, None, [5, 5, 2, 9], [3], False) == int((table["list"] == 3).sum())


def test_an_interval_mask_is_the_range_rule(small_corpus):
    """live and in range are one rule for an interval: on a real block table, the live blocks under a mask of [lo, hi) are
    the blocks in range of tests/ranked_range.py"""
    import ranked_range as RR
    from dint_amd import device

    ix = get_index(small_corpus, host.SINGLE_PACKED)
    table, _ = device.index_posting_lists(ix.bytes, ix.offsets)
    num_docs = int(ix.docids.max()) + 1
    r = np.random.default_rng(1)
    terms = np.argsort(-ix.lens.astype(np.int64))[:30].tolist() + [0, 1, 2]
    for _ in range(12):
        lo, hi = sorted(int(x) for x in r.integers(0, num_docs + 1, 2))
        mask = np.zeros(num_docs, dtype=bool)
        mask[lo:hi] = True
        live = DF.live_blocks(table, mask)
        for t in terms:
            assert int(live[table["list"] == t].sum()) == RR.n_blocks_in_range(table, t, lo, hi), (t, lo, hi)


@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_the_gpu_batch_is_not_vacuous(request, corpus_name):
    """tests/test_gpu_doc_filter.py's batch, from the lists alone: under every one of its filters either entry matches
    something, over the five it matches thousands, and the clustered filter leaves blocks dead."""
    import functools

    from dint_amd import device

    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    num_docs = int(ix.docids.max()) + 1
    table, _ = device.index_posting_lists(ix.bytes, ix.offsets)
    qs = reference_queries(len(ix.lens))[::2] + heavy_queries(ix.lens, 30)
    term = int(np.argmax(ix.lens))
    of = lambda t: ix.docids[int(ix.bounds[t]):int(ix.bounds[t + 1])]  # noqa: E731
    docs = {False: [], True: []}
    for q in qs:
        own = [of(int(t)) for t in sorted(set(int(t) for t in q))]
        docs[False].append(np.unique(np.concatenate(own)))
        docs[True].append(functools.reduce(lambda a, b: np.intersect1d(a, b, assume_unique=True), own))
    matched = {False: 0, True: 0}
    for name in DF.BATCH_FILTERS:
        mask = DF.batch_filter(name, DF.batch_num_docs(num_docs), ix.docids, of(term))
        assert mask.size == min(num_docs, DF.BATCH_MAX_DOCS)
        for conjunctive in (False, True):
            n = sum(int(DF.holds(mask, d).sum()) for d in docs[conjunctive])
            assert n > 0, (name, conjunctive)
            matched[conjunctive] += n
        if name == "runs":
            per_list, every = DF.live_per_list(table, DF.live_blocks(table, mask), len(ix.lens)), DF.live_per_list(table, None, len(ix.lens))
            for conjunctive in (False, True):
                assert 0 < sum(DF.planned_of(per_list, ix.lens, q, conjunctive) for q in qs) < sum(DF.planned_of(every, ix.lens, q, conjunctive) for q in qs)
    assert matched[False] > 5000 and matched[True] > 500, matched


# ---- the --filter file parser -----------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include "%s"
int main() {
    try {
        const tool::doc_filter_bits f = tool::parse_doc_filter(std::cin);
        std::printf("%%llu %%zu", (unsigned long long)f.num_docs, f.words.size());
        for (uint64_t w : f.words) std::printf(" %%llu", (unsigned long long)w);
        std::printf("\n");
    } catch (std::exception const& e) {
        std::printf("error %%s\n", e.what());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def parser_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the filter file parser"
    tmp = tmp_path_factory.mktemp("doc_filter_file")
    src, exe = os.path.join(tmp, "parse.cpp"), os.path.join(tmp, "parse")
    with open(src, "w") as f:
        f.write(PROGRAM % PARSER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    return exe


def _parse(exe, text):
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    if out[0] == "error":
        return None
    num_docs, n_words = int(out[0]), int(out[1])
    words = np.array([int(x) for x in out[2:]], dtype=np.uint64)
    assert words.size == n_words == (num_docs + 63) // 64
    return num_docs, np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).tolist()


def test_filter_files(parser_exe):
    assert _parse(parser_exe, "") == (0, [])
    assert _parse(parser_exe, "\n\n") == (0, [])
    assert _parse(parser_exe, "5\n") == (6, [5])
    assert _parse(parser_exe, "0\n63\n64\n65") == (66, [0, 63, 64, 65])
    assert _parse(parser_exe, "3:7\n") == (7, [3, 4, 5, 6])
    assert _parse(parser_exe, "  3:7  \r\n\n10\n") == (11, [3, 4, 5, 6, 10])
    assert _parse(parser_exe, "7:7\n9:3\n") == (0, [])                        # empty and inverted intervals add nothing
    assert _parse(parser_exe, "2:70\n60:130\n64\n5\n100:101\n") == (130, list(range(2, 130)))  # overlapping lines: the union
    assert _parse(parser_exe, "0:64\n") == (64, list(range(64)))
    assert _parse(parser_exe, "63:65\n") == (65, [63, 64])
    assert _parse(parser_exe, "64:200\n") == (200, list(range(64, 200)))
    assert _parse(parser_exe, "0:1000\n5000\n")[1] == list(range(1000)) + [5000]
    r = np.random.default_rng(6)
    lines, want = [], set()
    for _ in range(200):
        lo = int(r.integers(0, 5000))
        if r.random() < 0.5:
            lines.append(str(lo)), want.add(lo)
        else:
            hi = lo + int(r.integers(-3, 200))
            lines.append(f"{lo}:{hi}"), want.update(range(lo, hi))
    got = _parse(parser_exe, "\n".join(lines))
    assert got == (max(want) + 1, sorted(want))
    for bad in ("x\n", "1 2\n", "1:2:3\n", ":5\n", "5:\n", "-1\n", "4294967295\n", "0:4294967296\n", "1.5\n"):
        assert _parse(parser_exe, bad) is None, bad
    # the top of the range, without a bitmap of it: the largest hi and lo are read, and an empty interval there adds nothing
    assert _parse(parser_exe, "4294967295:4294967295\n4294967294:4294967290\n7\n") == (8, [7])
    assert _parse(parser_exe, "4294967296:4294967296\n") is None


# ---- the fuzz's conditions, from the model alone ----------------------------------------------------------------------
def test_the_fuzz_seeds_meet_their_conditions():
    """tests/test_gpu_doc_filter_fuzz.py asserts, on the device's own outputs, that at least half of its (case, query) pairs
    match something and that at least a quarter decode strictly fewer blocks than the unfiltered call, for either entry
    (check_shares there). These are properties of the committed seeds: replayed here from the model, so that
    they are settled without a device."""
    import test_gpu_doc_filter_fuzz as Z
    from dint_amd import device

    totals = []
    for seed, kind, ds, fs in Z.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
        for i in range(Z.CASES_PER_DICTIONARY):
            case = Z.draw_filter_case(Dd, Df, 100 * seed + i)
            table, _ = device.index_posting_lists(case.X.index, case.X.offsets)
            totals.append(Z.model_shares(case, table))
    Z.check_shares(np.sum(totals, axis=0))
