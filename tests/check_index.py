"""Model of dint_check_index (include/dint_hip.h; the reference's verify_collection,
include/ds2i/verify_collection.hpp:7-52) in plain numpy: an index, given as the lists and freqs it holds, against a view of a
collection. Not a test."""
from collections import namedtuple

import numpy as np

OK, LENGTH, DOCID, FREQ = 0, 1, 2, 3

#: the fields of dint_index_mismatch
Mismatch = namedtuple("Mismatch", "kind list position expected got")

#: the arrays of dint_collection_view, as QueryIndex.check takes them (freqs / freqs_at None: docIDs only)
View = namedtuple("View", "docs freqs docs_at freqs_at list_len")


def view_of(lists, freqs=None):
    """The lists back to back, as a collection file holds them without its length words."""
    lens = np.array([len(x) for x in lists], dtype=np.uint64)
    at = (np.cumsum(lens) - lens).astype(np.uint64)
    docs = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists]) if len(lists) else np.zeros(0, np.uint32)
    if freqs is None:
        return View(docs, None, at, None, lens)
    return View(docs, np.concatenate([np.asarray(x, dtype=np.uint32) for x in freqs]), at, at.copy(), lens)


def check(index_lists, index_freqs, view, with_freqs=True):
    """(n_mismatches, first): a list of wrong length counts once and none of its postings is compared; a posting whose docID
    or freq (or both) differs counts once; first = the lowest list, LENGTH before any posting, the lowest position, DOCID
    before FREQ; None without a mismatch."""
    assert len(index_lists) == len(view.list_len)
    with_freqs = with_freqs and view.freqs is not None
    n, first = 0, None
    for l, got_docs in enumerate(index_lists):
        want_len = int(view.list_len[l])
        if want_len != len(got_docs):
            n += 1
            first = first or Mismatch(LENGTH, l, 0, want_len, len(got_docs))
            continue
        a = int(view.docs_at[l])
        want_docs = view.docs[a:a + want_len]
        wrong_doc = np.asarray(got_docs, dtype=np.uint32) != want_docs
        wrong = wrong_doc
        if with_freqs:
            f = int(view.freqs_at[l])
            want_freqs = view.freqs[f:f + want_len]
            wrong = wrong_doc | (np.asarray(index_freqs[l], dtype=np.uint32) != want_freqs)
        n += int(wrong.sum())
        if first is None and wrong.any():
            i = int(np.flatnonzero(wrong)[0])
            if wrong_doc[i]:
                first = Mismatch(DOCID, l, i, int(want_docs[i]), int(got_docs[i]))
            else:
                first = Mismatch(FREQ, l, i, int(want_freqs[i]), int(index_freqs[l][i]))
    return n, first
