"""Expected values of the document-filter ranked tests: the unfiltered models (tests/ranked_or.py,
tests/ranked.py) asked for EVERY match (tests/ranked_range.py's every_match), filtered by a mask over the docID space —
document d is in the filter iff d < len(mask) and mask[d] — and cut to the best k by descending score, equal scores by
ascending docID. The filter filters: a match keeps the score the unfiltered model gives it, bit for bit. Also the live blocks
of a host block table under a mask (what dint_doc_filter_info's live_blocks and the calls' blocks_decoded are held to), and
the seeded filters of the batch and fuzz tests, so that tests/test_doc_filter_cpu.py can replay them without a device."""
import numpy as np

import ranked_range as RR

every_match = RR.every_match


def as_mask(members, num_docs: int):
    """docIDs -> a bool mask of num_docs entries (members at or past num_docs are not in the filter)"""
    mask = np.zeros(int(num_docs), dtype=bool)
    m = np.asarray(members, dtype=np.int64).reshape(-1)
    mask[m[m < num_docs]] = True
    return mask


def holds(mask, ids):
    """mask[ids], False at and past len(mask)"""
    ids = np.asarray(ids).astype(np.int64)
    inside = ids < mask.size
    out = np.zeros(ids.shape, dtype=bool)
    out[inside] = mask[ids[inside]]
    return out


def top_in_filter(matches, mask, k: int):
    """every_match's pair filtered by the mask -> (count, scores f32[k], docids u32[k], matches in the filter), the outputs
    filled as the device fills them: 0.0 / 0xFFFFFFFF past the count."""
    sc, ids = matches
    keep = holds(mask, ids)
    sc, ids = sc[keep], ids[keep]
    best = np.lexsort((ids, -sc))[:k]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    scores[:best.size] = sc[best]
    docids[:best.size] = ids[best]
    return best.size, scores, docids, int(keep.sum())


def ranked_or_filtered(lists, terms, norm_lens_, num_docs: int, k: int, mask):
    return top_in_filter(every_match(lists, terms, norm_lens_, num_docs, False), mask, k)


def ranked_and_filtered(lists, terms, norm_lens_, num_docs: int, k: int, mask):
    return top_in_filter(every_match(lists, terms, norm_lens_, num_docs, True), mask, k)


def live_blocks(block_table, mask):
    """-> bool per block of a host block table (dint_index_posting_lists' records): live iff the mask holds a document d
    with base <= d <= max (and d < len(mask)). One prefix sum of the mask, two reads a block."""
    below = np.concatenate([[0], np.cumsum(np.asarray(mask, dtype=np.int64))])  # below[x] = the filter's documents < x
    n = int(np.asarray(mask).size)
    lo = block_table["base"].astype(np.int64)
    hi = np.minimum(block_table["max"].astype(np.int64), n - 1)
    ok = lo <= hi
    live = np.zeros(len(block_table), dtype=bool)
    live[ok] = below[hi[ok] + 1] > below[lo[ok]]
    return live


def popcount64(words):
    """the set bits of each u64 word"""
    w = np.asarray(words, dtype=np.uint64).copy()
    m1, m2, m4, h = (np.uint64(x) for x in (0x5555555555555555, 0x3333333333333333, 0x0F0F0F0F0F0F0F0F, 0x0101010101010101))
    w -= (w >> np.uint64(1)) & m1
    w = (w & m2) + ((w >> np.uint64(2)) & m2)
    w = (w + (w >> np.uint64(4))) & m4
    return ((w * h) >> np.uint64(56)).astype(np.int64)


def live_blocks_words(block_table, words, num_docs: int):
    """live_blocks for a filter given as its bitmap words (bit d & 63 of word d >> 6; the bits at and past num_docs are
    ignored) — for filters over docID spaces where a byte per document is too much (tests/doc_filter_timing.py). The
    device's own rule: a directory of the words' prefix popcounts, two entries and two words a block."""
    words = np.asarray(words, dtype=np.uint64)
    rank = np.concatenate([[0], np.cumsum(popcount64(words))])

    def below(x):  # the filter's documents < x, x <= num_docs
        w, r = x >> 6, (x & 63).astype(np.uint64)
        inside = r != 0
        part = np.zeros(x.shape, dtype=np.int64)
        part[inside] = popcount64(words[w[inside]] & ((np.uint64(1) << r[inside]) - np.uint64(1)))
        return rank[w] + part

    lo = block_table["base"].astype(np.int64)
    hi = np.minimum(block_table["max"].astype(np.int64), int(num_docs) - 1)
    ok = lo <= hi
    live = np.zeros(len(block_table), dtype=bool)
    live[ok] = below(hi[ok] + 1) > below(lo[ok])
    return live


def live_per_list(block_table, live, n_lists: int):
    """-> per list, its live blocks. live: live_blocks' flags, or None (unfiltered: every block)."""
    weights = None if live is None else np.asarray(live, dtype=np.int64)
    return np.bincount(block_table["list"], weights=weights, minlength=n_lists).astype(np.int64)


def planned_of(per_list, lens, terms, conjunctive: bool) -> int:
    """A query's blocks_decoded from live_per_list's counts — OR: the live blocks of every distinct term; AND: of the rarest
    list (shortest, equal lengths by term id)."""
    terms = sorted(set(int(t) for t in terms))
    if conjunctive and terms:
        terms = [min(terms, key=lambda t: (int(lens[t]), t))]
    return sum(int(per_list[t]) for t in terms)


def planned_blocks(block_table, live, lens, terms, conjunctive: bool) -> int:
    """planned_of over live_blocks' flags (None: unfiltered, every block)"""
    return planned_of(live_per_list(block_table, live, len(lens)), lens, terms, conjunctive)


# ---- the filters of the batch test: densities 1/2 and 1/64, clustered runs, one term's documents, their complement ----
BATCH_FILTERS = ("half", "one in 64", "runs", "one term", "all but one term")


BATCH_MAX_DOCS = 1 << 25  # (a mask is a byte per document here: the sparse corpus spans 1.3e9 docIDs)


def batch_num_docs(num_docs: int) -> int:
    """The batch filters' num_docs for an index of num_docs documents: its own, capped — on the sparse corpus the filters end
    far below the index's largest docID, and every document past them is outside."""
    return min(int(num_docs), BATCH_MAX_DOCS)


def batch_filter(name: str, num_docs: int, docids, term_docids, seed: int = 3):
    """-> a bool mask over [0, num_docs). docids: the index's postings (the runs begin at documents it holds: synthetic
    docIDs thin out towards the top of their space); term_docids: the documents of the term the last two kinds are about."""
    r = np.random.default_rng(seed)
    if name == "half":
        return r.random(num_docs) < 0.5
    if name == "one in 64":
        return r.random(num_docs) < 1.0 / 64
    if name == "runs":  # eight runs, together up to a tenth of the space
        mask = np.zeros(num_docs, dtype=bool)
        inside = docids[:1 << 20][docids[:1 << 20] < num_docs]
        for lo in r.choice(inside, 8):
            mask[int(lo):int(lo) + max(1, num_docs // 80)] = True
        return mask
    if name == "one term":
        return as_mask(term_docids, num_docs)
    if name == "all but one term":
        return ~as_mask(term_docids, num_docs)
    raise ValueError(name)


# ---- the filters of the fuzz cases ------------------------------------------------------------------------------------
FUZZ_KINDS = ("runs", "few postings", "interval", "one term", "all but one term", "half", "one in 64", "all", "empty")
FUZZ_WEIGHTS = (0.26, 0.2, 0.14, 0.08, 0.06, 0.1, 0.06, 0.06, 0.04)


def fuzz_filter(r, docids, bounds, anchors=None):
    """One seeded filter of a random kind for an index of the lists docids[bounds[t] : bounds[t + 1]] -> (kind, mask). The
    mask's length — the filter's num_docs — is drawn too: below, at and above the index's largest docID + 1. anchors: the
    documents the clustered kinds are drawn around (a document once per query of the case whose intersection holds it, so
    that a narrow filter still leaves the conjunctive queries something); none: the postings."""
    anchors = docids if anchors is None or len(anchors) == 0 else np.asarray(anchors)
    top = int(docids.max()) + 1
    num_docs = max(1, int(top * r.choice([0.4, 0.9, 1.0, 1.0, 1.0, 1.3])) + int(r.integers(0, 3)))
    kind = FUZZ_KINDS[int(r.choice(len(FUZZ_KINDS), p=FUZZ_WEIGHTS))]
    mask = np.zeros(num_docs, dtype=bool)
    t = int(r.integers(0, len(bounds) - 1))
    of_t = docids[int(bounds[t]):int(bounds[t + 1])]
    if kind == "runs":  # one to four runs around postings, each a few hundredths of the space
        for at in r.choice(anchors, int(r.integers(1, 5))):
            lo = max(0, int(at) - int(r.integers(0, max(1, top // 40))))
            mask[lo:int(at) + 1 + int(r.integers(0, max(1, top // 40)))] = True
    elif kind == "few postings":  # a handful of documents the index holds
        mask = as_mask(r.choice(anchors, int(r.integers(1, 17))), num_docs)
    elif kind == "interval":
        at = int(r.choice(anchors))  # one run, of any width, around an anchor
        a, b = max(0, at - int(r.integers(0, num_docs // 3 + 1))), at + 1 + int(r.integers(0, num_docs // 3 + 1))
        mask[a:b] = True
    elif kind == "one term":
        mask = as_mask(of_t, num_docs)
    elif kind == "all but one term":
        mask = ~as_mask(of_t, num_docs)
    elif kind == "half":
        mask = r.random(num_docs) < 0.5
    elif kind == "one in 64":
        mask = r.random(num_docs) < 1.0 / 64
    elif kind == "all":
        mask[:] = True
    return kind, mask
