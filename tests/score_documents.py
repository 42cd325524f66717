"""Expected values of the score-documents tests: a CPU model of dint_score_documents over the builder's
lists, built from the ranked-OR model's pieces (tests/ranked_or.py, tests/ranked.py), as tests/maxscore.py's _scores is.

Per query, over its distinct terms T in ascending term id, and per document d the caller names (any u32, in any order,
repeated or not): the freqs row [f_t(d) if list t holds d else 0 for t in T], the score 0.0f + for each t whose list holds d
q_weight_t * doc_term_weight(f_t(d), norm_lens[d]) in binary32, and the blocks read: per term the distinct blocks the
documents fall in, a document's block being the first whose last docID is >= it (none past the list's last docID)."""
from dataclasses import dataclass

import numpy as np

import ranked
import ranked_or
from maxscore import block_maxima, blocks_of


@dataclass
class Result:
    scores: np.ndarray  # f32[n_docs]
    freqs: np.ndarray   # u32[n_docs, T]
    held: np.ndarray    # bool[n_docs, T]: list t holds the document (a freq may be 0: freq - 1 wrapped)
    blocks_read: int
    all_blocks: int     # every block of every distinct term (what ranked_or reads)


def score_documents(lists, terms, docs, norm_lens_, num_docs: int) -> Result:
    docs = np.asarray(docs, dtype=np.uint32)
    if len(terms) == 0:
        return Result(np.zeros(docs.size, np.float32), np.zeros((docs.size, 0), np.uint32), np.zeros((docs.size, 0), bool), 0, 0)
    norm_lens_ = np.asarray(norm_lens_, dtype=np.float32)
    t, qf, post, _ = ranked_or._union(lists, terms)
    score = np.zeros(docs.size, dtype=np.float32)
    freqs = np.zeros((docs.size, t.size), dtype=np.uint32)
    held = np.zeros((docs.size, t.size), dtype=bool)
    read = all_blocks = 0
    for j in range(t.size):  # ascending term id
        d, f = post[j]
        all_blocks += blocks_of(d.size)
        if d.size == 0 or docs.size == 0:
            continue
        pos = np.minimum(np.searchsorted(d, docs), d.size - 1)
        hit = d[pos] == docs
        held[:, j] = hit
        freqs[hit, j] = f[pos][hit]
        nl = norm_lens_[docs[hit]]  # (read after a hit only: a document of no list may lie past norm_lens)
        w = ranked.query_term_weight(int(qf[j]), int(d.size), num_docs) * ranked.doc_term_weight(f[pos][hit], nl)
        score[hit] = score[hit] + w
        blk = np.searchsorted(block_maxima(d), docs, side="left")
        read += int(np.unique(blk[blk < blocks_of(d.size)]).size)
    return Result(score, freqs, held, read, all_blocks)


def model_batch(lists, queries, docs, norm_lens_, num_docs: int):
    return [score_documents(lists, q, d, norm_lens_, num_docs) for q, d in zip(queries, docs)]


def union_of(lists, terms) -> np.ndarray:
    if len(terms) == 0:
        return np.zeros(0, np.uint32)
    return ranked_or._union(lists, terms)[3]


def draw_from_union(r, lists, terms, n: int) -> np.ndarray:
    """n documents of the query's union, drawn with replacement only if it has fewer, in the draw's order."""
    u = union_of(lists, terms)
    if u.size == 0:
        return u
    return r.choice(u, n, replace=u.size < n).astype(np.uint32)
