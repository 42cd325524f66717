"""The ranked calls' shared sequence on the GPU ("the extras' five steps"): every family's entries — faceted,
collapsed, paged, collapsed paged, group-limited, sorted, value-stats, group-stats and percentile, OR and AND — run one
after another on ONE query index and must each give, byte for byte, what they give on an index nothing else has touched
(a workspace left uncleared between families would show), and on the calls that return before anything is launched every
output is what the step `begin` promises. The values themselves are the family tests' business (tests/test_gpu_<family>.py:
each against its model); here only the same bytes count. Inputs are fixed; nothing is drawn."""
import ctypes as C

import numpy as np
import pytest

from dint_amd import host
from test_gpu_facets import HAND_DOCS
from test_gpu_ranked_queries import _hand_made

pytestmark = pytest.mark.gpu

K = 3
NONE32 = 0xFFFFFFFF
N_GROUPS = 5
PER_GROUP = 2
# the hand-made index (test_gpu_ranked_range.py): a = 0 .. 2999, b = 5000 .. 8999, c = the evens, d = every doc, e = {10, 20, 30, 40}
BATCH = [[2, 3, 4],  # several terms, matches in both modes
         [0, 1],     # AND: a's pages are planned and nothing survives them; OR: two disjoint lists
         [],         # no terms
         [3, 4], [0, 2]]
NO_TERMS = [[], [], []]
PERCENTILES = [0, 50, 99.5, 100]
EDGES = [100, 500, 900]


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available()
    from dint_amd import device as dev

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


class World:
    """What every call here shares besides its query index: the hand-made index's bytes, the freqs dictionary, the wand data
    (norm_lens all 1), a map (document d in group d % 5, every 11th in none), a column, and fixed cursors."""

    def __init__(self, device):
        self.device = device
        self.kind = host.MULTI_PACKED
        self.ix = _hand_made(device, self.kind)
        self.fd = device.Dictionary(self.kind, self.ix.freqs_dict)
        self.wand = device.WandData(np.ones(HAND_DOCS, dtype=np.float32))
        d = np.arange(HAND_DOCS, dtype=np.int64)
        self.facets = device.DocFacets(0, np.where(d % 11 == 0, -1, d % N_GROUPS), N_GROUPS)
        self.values = device.DocValues(0, (d * 7919) % 1000)
        self.mask = (d % 3 != 1) | (d >= 6000)

    def index(self):
        return self.device.QueryIndex(self.device.Dictionary(self.kind, self.ix.docs_dict), self.ix.bytes, self.ix.offsets)

    def close(self):
        self.values.close()
        self.facets.close()
        self.wand.close()


@pytest.fixture(scope="module")
def world(device):
    w = World(device)
    yield w
    w.close()


def _value_stats_without_hit_values(w, mode, qi, qs, f):
    """the value-stats entry with a null hit_values (the Python method always takes them) -> (counts, scores, docids, matches,
    blocks_decoded, stats, buckets)"""
    from dint_amd import device as dev

    terms, offs = dev._pack_queries(qs)
    edges = np.asarray(EDGES, dtype=np.uint32)
    n = len(qs)
    counts, matches = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    scores, docids = np.zeros((n, K), dtype=np.float32), np.zeros((n, K), dtype=np.uint32)
    stats, buckets = np.zeros(n, dtype=dev._VALUE_STATS), np.zeros((n, edges.size + 1), dtype=np.uint32)
    blocks = C.c_uint64()
    fn = f"dint_ranked_{mode}_value_stats_queries"
    dev._check(getattr(dev._lib, fn)(qi._h, w.fd._h, w.wand._h, K, terms.ctypes.data, offs.ctypes.data, f._h if f is not None else None,
                                     w.values._h, edges.ctypes.data, edges.size, n, counts.ctypes.data, matches.ctypes.data,
                                     scores.ctypes.data, docids.ctypes.data, stats.ctypes.data, buckets.ctypes.data, None, C.byref(blocks),
                                     qi._stream()), fn)
    return counts, scores, docids, matches, blocks.value, stats, buckets


def entries(w, mode, cursors, value_cursors):
    """[(name, call(qi, qs, filter) -> the entry's outputs, the outputs' indices that hold hit groups)] of one mode; a call
    takes the cursors of its queries by their index in BATCH (any other batch: cursors[:len(qs)])"""
    def m(qi, family):
        return getattr(qi, f"ranked_{mode}_{family}_queries")

    def cur(c, qs):
        return c[:len(qs)]

    return [
        ("faceted", lambda qi, qs, f: m(qi, "faceted")(w.fd, w.wand, qs, w.facets, filter=f, k=K, with_stats=True), ()),
        ("collapsed", lambda qi, qs, f: m(qi, "collapsed")(w.fd, w.wand, qs, w.facets, filter=f, k=K, with_stats=True, with_rows=True), (6,)),
        ("paged", lambda qi, qs, f: m(qi, "paged")(w.fd, w.wand, qs, after=cur(cursors, qs), filter=f, k=K, with_stats=True), ()),
        ("collapsed paged", lambda qi, qs, f: m(qi, "collapsed_paged")(w.fd, w.wand, qs, w.facets, after=cur(cursors, qs), filter=f, k=K,
                                                                       with_stats=True, with_rows=True), (6,)),
        ("group limit", lambda qi, qs, f: m(qi, "group_limit")(w.fd, w.wand, qs, w.facets, PER_GROUP, after=cur(cursors, qs), filter=f, k=K,
                                                               with_stats=True, with_rows=True), (6,)),
        ("group limit from the start", lambda qi, qs, f: m(qi, "group_limit")(w.fd, w.wand, qs, w.facets, PER_GROUP, filter=f, k=K,
                                                                              with_stats=True), (6,)),
        ("sorted", lambda qi, qs, f: m(qi, "sorted")(w.fd, w.wand, qs, w.values, descending=False, after=cur(value_cursors, qs), filter=f,
                                                     k=K, with_stats=True), ()),
        ("value stats", lambda qi, qs, f: _value_stats_without_hit_values(w, mode, qi, qs, f), ()),
        ("value stats with hit values", lambda qi, qs, f: m(qi, "value_stats")(w.fd, w.wand, qs, w.values, edges=EDGES, filter=f, k=K,
                                                                              with_stats=True), ()),
        ("group stats", lambda qi, qs, f: m(qi, "group_stats")(w.fd, w.wand, qs, w.facets, w.values, filter=f, k=K, with_facet_counts=True), ()),
        ("percentile", lambda qi, qs, f: m(qi, "percentile")(w.fd, w.wand, qs, w.values, PERCENTILES, filter=f, k=K), ()),
        ("percentile with stats", lambda qi, qs, f: m(qi, "percentile")(w.fd, w.wand, qs, w.values, PERCENTILES, filter=f, k=K,
                                                                        with_stats=True), ()),
    ]


def all_entries(w, f=None):
    """both modes' entries, OR's first; the cursors are every query's first hit from the start (no hit: from the start), so
    a paged call skips something wherever there is something to skip"""
    qi = w.index()
    f = qi.doc_filter(w.mask) if f else None
    out = []
    for mode in ("or", "and"):
        counts, scores, docids, _ = getattr(qi, f"ranked_{mode}_paged_queries")(w.fd, w.wand, BATCH, filter=f, k=K)
        cursors = [(float(scores[q, 0]), int(docids[q, 0])) if counts[q] else None for q in range(len(BATCH))]
        counts, hit_values, docids, _, _ = getattr(qi, f"ranked_{mode}_sorted_queries")(w.fd, w.wand, BATCH, w.values, descending=False,
                                                                                         filter=f, k=K)
        value_cursors = [(int(hit_values[q, 0]), int(docids[q, 0])) if counts[q] else None for q in range(len(BATCH))]
        assert cursors[0] is not None and value_cursors[0] is not None and cursors[2] is None
        out += [(f"{mode} {name}", call, groups) for name, call, groups in entries(w, mode, cursors, value_cursors)]
    if f is not None:
        f.close()
    qi.close()
    return out


def _bytes(out):
    return [np.asarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in out]


def _alone(w, call, qs, filtered):
    """the call on a query index of its own"""
    qi = w.index()
    f = qi.doc_filter(w.mask) if filtered else None
    out = call(qi, qs, f)
    if f is not None:
        f.close()
    qi.close()
    return out


def _in_turn(w, es, qs, filtered, alone):
    """every entry on one shared index, forwards and then backwards: each the bytes it gave alone"""
    qi = w.index()
    f = qi.doc_filter(w.mask) if filtered else None
    for name, call, _ in es + es[::-1]:
        assert _bytes(call(qi, qs, f)) == _bytes(alone[name]), name
    if f is not None:
        f.close()
    qi.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["unrestricted", "under a filter"])
def test_entries_in_turn_on_one_index_give_what_they_give_alone(world, filtered):
    es = all_entries(world, filtered)
    alone = {name: _alone(world, call, BATCH, filtered) for name, call, _ in es}
    # (the batch is what it is said to be: matches for [2, 3, 4] in both modes, pages and no survivor for AND's [0, 1])
    assert alone["and faceted"][3].tolist()[:3] == [4 if not filtered else int(world.mask[[10, 20, 30, 40]].sum()), 0, 0]
    assert alone["and faceted"][4] > 0 and alone["or faceted"][3][1] > 0 and alone["or faceted"][3][2] == 0
    assert alone["or paged"][5][0] == 1 and alone["and paged"][5][0] == 1  # (the cursor is the first hit: one match is not after it)
    _in_turn(world, es, BATCH, filtered, alone)


def test_entries_in_turn_when_or_runs_in_many_passes(device, world):
    """query_or_pass_pages = 1: every query with pages is an OR pass of its own, so the launches in front of the selection and
    behind it run once per pass at the pass's query offset — the same bytes as in one pass, alone and in turn"""
    es = all_entries(world)
    one_pass = {name: _alone(world, call, BATCH, False) for name, call, _ in es}
    device.set_option("query_or_pass_pages", 1)
    alone = {name: _alone(world, call, BATCH, False) for name, call, _ in es}
    for name in alone:
        assert _bytes(alone[name]) == _bytes(one_pass[name]), name
    _in_turn(world, es, BATCH, False, alone)


def _begun(x, hit_groups):
    """an output of a call without a match as `begin` and the entries' outputs leave it"""
    if x is None or not isinstance(x, np.ndarray):
        return x in (None, 0)
    if x.dtype.names:  # (the value-stats record: nothing reduced)
        return bool((x["n"] == 0).all() and (x["sum"] == 0).all() and (x["min"] == NONE32).all() and (x["max"] == 0).all())
    return bool((x == (NONE32 if hit_groups else 0)).all())


def test_a_batch_without_a_term_returns_what_begin_promises(world):
    """no query has a term: AND returns at n_pages == 0, OR at op.all == 0, behind `begin` and in front of the lock — zeros,
    the empty record, no group for every hit (docids: no document) — alone, as a batch of one, and in turn on an index whose
    workspaces the batch with matches has just filled"""
    es = all_entries(world)
    alone = {name: _alone(world, call, NO_TERMS, False) for name, call, _ in es}
    for name, call, groups in es:
        out = alone[name]
        docids = 2  # (every entry: counts, scores or hit values, docids, ...)
        for j, x in enumerate(out):
            assert _begun(x, j in groups or j == docids), (name, j)
        one = _alone(world, call, NO_TERMS[:1], False)
        for j, x in enumerate(out):
            if isinstance(x, np.ndarray):
                assert all(x[q:q + 1].tobytes() == one[j].tobytes() for q in range(len(NO_TERMS))), (name, j)
            else:
                assert x == one[j], (name, j)
    qi = world.index()
    for name, call, _ in es + es[::-1]:
        call(qi, BATCH, None)
        assert _bytes(call(qi, NO_TERMS, None)) == _bytes(alone[name]), name
    qi.close()
