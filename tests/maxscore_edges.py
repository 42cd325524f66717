"""Hand-made indexes for the edges of the pruned ranked OR call: list lengths on k, the choice of the
seed, thresholds of 0.0 and of subnormal size, and the geometry of the claims in an N list. Every spec carries its lists,
norm_lens and queries with what is known about each query by construction — theta from the seed's addends, the blocks
read counted by hand — so that tests/test_ranked_or_maxscore_cpu.py holds the model (tests/maxscore.py) to it without a
GPU and tests/test_gpu_ranked_or_maxscore.py the device to the model."""
from dataclasses import dataclass, field

import numpy as np

import maxscore
import ranked

KS = (1, 2, 255, 256, 257, 1024)
LENGTH_CASES = [(k, False) for k in KS] + [(2, True), (256, True)]  # (k, equal norm_lens and freqs: the addends tie)
MAXIMA_FUZZ_CASES = (0, 10)  # of the query fuzz plan (tests/fuzz_streams.py's query_plan): a single- and a multi-dictionary case
FLT_MAX = np.finfo(np.float32).max


def upper_bounds(mtw: np.ndarray) -> dict:
    """Maxima that are upper bounds of every doc_term_weight (f / (f + kd) <= 1): the pruned call's answer is ranked_or's."""
    return {"x1.5": (mtw * np.float32(1.5)).astype(np.float32), "ones": np.ones_like(mtw), "flt_max": np.full_like(mtw, FLT_MAX),
            "inf": np.full_like(mtw, np.inf)}


def under_estimates(mtw: np.ndarray) -> dict:
    """Maxima below the true ones: the documented degradation (include/dint_hip.h), documents may be dropped."""
    return {"x0.5": (mtw * np.float32(0.5)).astype(np.float32), "zeros": np.zeros_like(mtw)}


@dataclass
class Query:
    terms: list
    k: int
    seed: object = None     # the term whose k-th best addend is theta; None: no list of k postings, theta = 0
    blocks: object = None   # blocks read, counted by hand (None: the model's word only)
    prunes: object = None   # True: N is non-empty and fewer blocks are read than ranked_or reads; False: every block is read
    what: str = ""


@dataclass
class Spec:
    lists: list
    freqs: list
    num_docs: int
    nl: np.ndarray
    queries: list = field(default_factory=list)

    def __post_init__(self):
        self.lens = np.array([x.size for x in self.lists], dtype=np.uint32)
        self.docids = np.concatenate(self.lists).astype(np.uint32)
        self.all_freqs = np.concatenate(self.freqs).astype(np.uint32)
        self.bounds = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.mtw = ranked.max_term_weights(self.docids, self.all_freqs, self.bounds, self.nl)
        self.model_lists = ranked.BuilderLists(self.docids, self.all_freqs, self.bounds)

    def addends(self, t: int, qf: int = 1) -> np.ndarray:
        """a_t(d) over list t, in binary32, from the BM25 pieces alone (no part of the pruned model)."""
        return ranked.query_term_weight(qf, int(self.lens[t]), self.num_docs) * ranked.doc_term_weight(self.freqs[t], self.nl[self.lists[t]])

    def theta(self, q: Query) -> np.float32:
        if q.seed is None:
            return np.float32(0)
        return np.sort(self.addends(q.seed, q.terms.count(q.seed)))[::-1][q.k - 1]

    def all_blocks(self, q: Query) -> int:
        return sum(maxscore.blocks_of(int(self.lens[t])) for t in set(q.terms))

    def model(self, q: Query) -> maxscore.Result:
        return maxscore.maxscore(self.model_lists, q.terms, self.nl, self.mtw, self.num_docs, q.k)

    def check_model(self, q: Query) -> maxscore.Result:
        """The model against what the query is known to do by construction."""
        m = self.model(q)
        n_terms = len(set(q.terms))
        assert np.float32(m.theta) == self.theta(q) and m.all_blocks == self.all_blocks(q), q
        if q.seed is None:
            assert m.theta == 0.0 and m.blocks_read == m.all_blocks and m.n_essential == n_terms, q
        if q.blocks is not None:
            assert m.blocks_read == q.blocks, (q, m.blocks_read)
        if q.prunes is True:
            assert m.n_essential < n_terms and m.blocks_read < m.all_blocks, q
        if q.prunes is False:
            assert m.blocks_read == m.all_blocks, q
        return m


def _pick(r, universe: int, n: int) -> np.ndarray:
    return np.sort(r.choice(universe, n, replace=False)).astype(np.uint32)


def lengths_on_k(k: int, equal: bool = False) -> Spec:
    """Lists of k - 1, k and k + 1 postings (0-4; two of each of the first two, for the seed's tie) of high freqs, rare in
    16000 documents and all among the first 2000 (so that they fall in few blocks of the dense lists), and two dense lists of 24 and 28 pages (5, 6) of freqs 1-3, whose maxima together stay below any addend
    of the rare ones. equal: every norm_len 1 and every freq of a rare list 7, so that a rare list's addends all tie."""
    r = np.random.default_rng(1000 + k)
    num_docs = 16000
    sizes = [max(k - 1, 1), k, k + 1, max(k - 1, 1), k, 6000, 7000]
    lists = [_pick(r, 2000, n) for n in sizes[:5]] + [_pick(r, num_docs, n) for n in sizes[5:]]
    freqs = [np.full(n, 7, dtype=np.uint32) if equal else r.integers(5, 30, n).astype(np.uint32) for n in sizes[:5]]
    freqs += [r.integers(1, 4, n).astype(np.uint32) for n in sizes[5:]]
    nl = np.ones(num_docs, dtype=np.float32) if equal else (r.random(num_docs) * 3 + 0.05).astype(np.float32)
    s = Spec(lists, freqs, num_docs, nl)
    below, at, above, below2, at2, a, b = range(7)
    long_seed = a  # of the two dense lists, the shorter
    s.queries = [
        Query([at, a, b], k, seed=at, prunes=True, what="a list of exactly k postings is the seed: theta is its smallest addend"),
        Query([above, a, b], k, seed=above, prunes=True, what="k + 1 postings: theta is its second smallest addend"),
        Query([at, above, a, b], k, seed=at, what="k and k + 1 postings: the shorter"),
        Query([at, at2, a, b], k, seed=at, what="two lists of k postings: the smaller term id"),
        Query([at2, at, at2, b], k, seed=at, what="... whatever the order and the multiplicity in the query"),
        Query([at2, a, b], k, seed=at2, prunes=True),
        Query([at], k, seed=at, blocks=maxscore.blocks_of(k)),
        Query([at, at], k, seed=at, blocks=maxscore.blocks_of(k)),
        Query([a, b], k, seed=long_seed),
    ]
    if k > 1:  # (k = 1: a list of k - 1 postings would be empty)
        s.queries += [
            Query([below, a, b], k, seed=long_seed, what="k - 1 postings are no seed: the shortest list of at least k is a dense one"),
            Query([below, below2], k, seed=None, prunes=False, what="no list of k postings: theta = 0 and every block is read"),
            Query([below], k, seed=None, prunes=False),
            Query([below, at, a], k, seed=at),
        ]
    return s


def seed_ties() -> Spec:
    """Two candidate seeds of equal length in one query, k = 256: the smaller term id wins, and the two choices are told apart
    by theta and the blocks read. hi lists have freqs 20-30 (every addend above the dense lists' summed maxima), lo lists
    freq 1 and norm_lens of 50 (their addends are below either dense list's maximum: nothing is pruned). Terms 0 = hi, 1 = lo, 2 = lo, 3 = hi; 4, 5 dense."""
    r = np.random.default_rng(77)
    num_docs, n = 16000, 256
    lists = [_pick(r, 2000, n) for _ in range(4)] + [_pick(r, num_docs, 6000), _pick(r, num_docs, 7000)]
    hi = lambda: r.integers(20, 31, n).astype(np.uint32)
    lo = lambda: np.ones(n, dtype=np.uint32)
    freqs = [hi(), lo(), lo(), hi(), r.integers(1, 4, 6000).astype(np.uint32), r.integers(1, 4, 7000).astype(np.uint32)]
    nl = (r.random(num_docs) * 3 + 0.05).astype(np.float32)
    nl[np.concatenate([lists[1], lists[2]])] = 50.0
    s = Spec(lists, freqs, num_docs, nl)
    s.queries = [Query([0, 1, 4, 5], n, seed=0, what="hi before lo: hi is the seed"),
                 Query([1, 0, 5, 4], n, seed=0),
                 Query([2, 3, 4, 5], n, seed=2, what="lo before hi: lo is the seed"),
                 Query([3, 2, 4, 5], n, seed=2),
                 Query([1, 2, 4, 5], n, seed=1), Query([0, 3, 4, 5], n, seed=0)]
    return s


def zero_theta() -> Spec:
    """A seed whose k-th best addend is exactly 0.0: a list of one full block with a posting of freq 0 (freq - 1 wraps to
    0xFFFFFFFF, legal in a full block). Nothing is pruned, and the document of score 0.0 is counted, last."""
    r = np.random.default_rng(78)
    num_docs = 16000
    lists = [_pick(r, num_docs, 256), _pick(r, num_docs, 6000), _pick(r, num_docs, 256)]
    freqs = [r.integers(5, 30, 256).astype(np.uint32), r.integers(1, 4, 6000).astype(np.uint32), r.integers(5, 30, 256).astype(np.uint32)]
    freqs[0][[3, 200]] = 0
    # (list 2's docID of freq 0 is in no other list: its score is 0.0)
    alone = int(np.flatnonzero(~np.isin(lists[2], np.concatenate([lists[0], lists[1]])))[0])
    freqs[2][alone] = 0
    nl = (r.random(num_docs) * 3 + 0.05).astype(np.float32)
    s = Spec(lists, freqs, num_docs, nl)
    s.zero_doc = int(lists[2][alone])
    s.queries = [Query([0], 256, seed=0, prunes=False), Query([0, 1], 256, seed=0, prunes=False),
                 Query([0, 1], 255, seed=0, prunes=False, what="two addends of 0.0: the 255th best is one of them"),
                 Query([2], 256, seed=2, prunes=False), Query([2, 1], 256, seed=2, prunes=False),
                 Query([0, 1], 254, seed=0, what="the 254th addend is positive")]
    return s


def subnormal_theta() -> Spec:
    """tests/test_gpu_query_fuzz.py's subnormal index: two thirds of the norm_lens are 1e36 .. 3e38, so most addends (and the
    k-th best of a long enough list) are subnormal binary32 numbers; the bound compares them in double."""
    r = np.random.default_rng(777)
    n_docs = 1200
    dense = np.arange(0, n_docs, dtype=np.uint32)
    half = _pick(r, n_docs, 700)
    rare = _pick(r, n_docs, 90)
    lists = [dense, half, rare]
    freqs = [r.integers(1, 20, x.size).astype(np.uint32) for x in lists]
    nl = (r.random(n_docs) + 0.5).astype(np.float32)
    large = r.random(n_docs) < 0.67
    nl[large] = (10.0 ** r.uniform(36, 38.5, int(large.sum()))).astype(np.float32)
    s = Spec(lists, freqs, n_docs, nl)
    s.queries = [Query([0], 1024, seed=0), Query([0, 1], 1024, seed=0), Query([0, 1, 2], 1024, seed=0), Query([0, 2], 1024, seed=0),
                 Query([1, 0], 512, seed=1), Query([1, 2], 512, seed=1), Query([0, 1, 2, 2], 512, seed=1), Query([2, 0], 80, seed=2),
                 Query([2, 1], 90, seed=2), Query([2], 91, seed=None)]
    return s


def claim_geometry() -> Spec:
    """Every norm_len 1. N lists of freq 1 (low maxima): 0 = 4 full blocks and a short one of 100, docIDs 1000, 1003, ...;
    1 = one block of 100; 2 = 80 full blocks, docIDs 0, 3, ... Rare lists of freq 50 from term 3 on, their addends all equal
    (so every candidate ties with theta and lives), placed against the N lists' blocks; k = 2 but where said."""
    num_docs = 70000
    n0 = np.arange(1000, 1000 + 3 * (4 * 256 + 100), 3, dtype=np.uint32)
    n1 = np.arange(30000, 30000 + 5 * 100, 5, dtype=np.uint32)
    n2 = np.arange(0, 3 * 80 * 256, 3, dtype=np.uint32)
    u = lambda *x: np.array(sorted(x), dtype=np.uint32)
    rare = {
        "block_last": u(n0[255], n0[511]),                    # a block's last docID exactly: that block, not the next
        "below_first": u(5, 10),                              # below the list's first docID: its first block is claimed
        "above_last": u(n0[-1] + 1, n0[-1] + 7),              # above its last docID: no claim
        "short_block": u(n0[1024 + 50], n0[1024 + 60] + 1),   # its short last block, a member and a non-member
        "between": u(n0[300] + 1, n0[600] + 1),               # blocks that do not contain them
        "wave": n0[512] + 1 + np.arange(200, dtype=np.uint32),  # 200 consecutive docIDs within one block: one claim
        "two_lists_a": u(n0[800], n0[810] + 1),               # the same block from two E lists' pages
        "two_lists_b": u(n0[790] + 2, n0[1000]),
        "one_block": u(n1[0], n1[50] + 1, n1[99]),            # an N list of one block
        "one_of_80": u(n2[256 * 40 + 7], n2[256 * 40 + 9] + 1),  # one block of 80
        "all_of_80": np.sort(np.concatenate([n2[100::256], n2[200::256] + 1])).astype(np.uint32),  # every block of 80
    }
    names = list(rare)
    lists = [n0, n1, n2] + [rare[x] for x in names]
    freqs = [np.ones(x.size, dtype=np.uint32) for x in lists[:3]] + [np.full(rare[x].size, 50, dtype=np.uint32) for x in names]
    s = Spec(lists, freqs, num_docs, np.ones(num_docs, dtype=np.float32))
    t = {x: 3 + i for i, x in enumerate(names)}
    s.term = t
    Q = lambda terms, blocks, what, k=2: Query(terms, k, seed=terms[0], blocks=blocks, prunes=blocks < sum(maxscore.blocks_of(lists[x].size) for x in set(terms)), what=what)
    s.queries = [
        Q([t["block_last"], 0], 1 + 2, "blocks 0 and 1"),
        Q([t["below_first"], 0], 1 + 1, "block 0"),
        Q([t["above_last"], 0], 1 + 0, "no block"),
        Q([t["short_block"], 0], 1 + 1, "the short last block"),
        Q([t["between"], 0], 1 + 2, "blocks 1 and 2"),
        Q([t["wave"], 0], 1 + 1, "200 candidates, one claim", k=200),
        Q([t["wave"], 0], 1 + 1, "... and with most of them tied behind the k-th place", k=3),
        Q([t["two_lists_a"], t["two_lists_b"], 0], 2 + 1, "block 3, claimed from two workgroups"),
        Q([t["one_block"], 1], 1 + 1, "a list of one block"),
        Q([t["above_last"], 1], 1 + 1, "below a one-block list's first docID"),
        Q([t["one_of_80"], 2], 1 + 1, "one block of 80 pages"),
        Q([t["all_of_80"], 2], 1 + 80, "every block of 80 pages: nothing saved", k=160),
        Q([t["block_last"], 0, 1, 2], 1 + 2 + 1 + 2, "three N lists: two blocks, the first block of a list above it, two of 80"),
    ]
    return s
