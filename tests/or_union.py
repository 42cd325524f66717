"""Expected values of the OR-query tests: or_query (include/ds2i/queries.hpp:86-130) counts the distinct docIDs of the
union of a query's lists and, with freqs, reads the freq of every posting of every distinct term."""
import numpy as np

import oracle


def union(docids: np.ndarray, bounds: np.ndarray, terms) -> int:
    """Plain set union of the lists' docIDs (the builder's input, no codec involved)."""
    cur = np.zeros(0, dtype=np.uint32)
    for t in np.unique(np.asarray(terms, dtype=np.int64)):
        cur = np.union1d(cur, docids[int(bounds[t]):int(bounds[t + 1])])
    return int(cur.size)


def union_freqs(docids: np.ndarray, freqs: np.ndarray, bounds: np.ndarray, terms):
    """-> (union size, sum of the freqs of every posting of every distinct term)."""
    total = 0
    for t in np.unique(np.asarray(terms, dtype=np.int64)):
        total += int(freqs[int(bounds[t]):int(bounds[t + 1])].astype(np.uint64).sum())
    return union(docids, bounds, terms), total


class OracleLists:
    """The lists as the CPU oracle decodes them from the index bytes (posting_list_decode), cached per term."""

    def __init__(self, kind, docs_dict: bytes, freqs_dict: bytes, index: np.ndarray, offsets: np.ndarray):
        self.docs = oracle.OracleDict(kind, docs_dict)
        self.freqs = oracle.OracleDict(kind, freqs_dict)
        self.index = np.ascontiguousarray(index, dtype=np.uint8)
        self.offsets = offsets
        self._lists = {}

    def postings(self, term: int):
        if term not in self._lists:
            self._lists[term] = oracle.posting_list_decode(self.docs, self.freqs, self.index, int(self.offsets[term]))
        return self._lists[term]

    def union(self, terms) -> int:
        cur = np.zeros(0, dtype=np.uint32)
        for t in np.unique(np.asarray(terms, dtype=np.int64)):
            cur = np.union1d(cur, self.postings(int(t))[0])
        return int(cur.size)


def oracle_lists(ix, kind) -> OracleLists:
    return OracleLists(kind, ix.docs_dict, ix.freqs_dict, ix.bytes, ix.offsets)
