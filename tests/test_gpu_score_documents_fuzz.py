"""Differential fuzzing of dint_score_documents on the GPU: the query plan of tests/fuzz_streams.py (random dictionary files,
random decoder-legal posting lists of up to 80 pages, wrapped freqs of 0 and freqs near 2^32) with the queries, norm_lens
and options of tests/query_fuzz_draws.py, and seeded document sets per case — against the model (tests/score_documents.py)
over the generator's postings and, on a sample, over the lists the CPU oracle decodes from the index bytes."""
import numpy as np
import pytest

import fuzz_streams as F
import ranked
import score_documents as S
from or_union import OracleLists
from query_fuzz_draws import draw_case
from test_gpu_query_fuzz import QUERY
from test_gpu_score_documents import assert_model, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


def draw_documents(r, lists, qs, num_docs):
    """Per query one of: documents of the union (1, 40 or 3 000 of them), the union itself, any u32, docIDs around num_docs,
    a shuffled set with repeats, nothing."""
    out = []
    for q in qs:
        u = S.union_of(lists, q)
        which = int(r.integers(0, 8))
        if which <= 2:
            d = S.draw_from_union(r, lists, q, (1, 40, 3000)[which])
        elif which == 3:
            d = u
        elif which == 4:
            d = r.integers(0, 1 << 32, 200).astype(np.uint32)
        elif which == 5:
            d = r.integers(max(0, num_docs - 300), num_docs + 300, 200).astype(np.uint32)
        elif which == 6:
            d = np.concatenate([S.draw_from_union(r, lists, q, 300), r.integers(0, num_docs, 100).astype(np.uint32)])
            d = r.permutation(np.concatenate([d, d[:150]]))
        else:
            d = np.zeros(0, np.uint32)
        out.append(np.asarray(d, dtype=np.uint32))
    return out


@pytest.mark.parametrize("case", QUERY, ids=lambda c: f"seed{c[0]}")
def test_score_documents_case(device, case):
    Dd, Df, X = F.build_query_case(case)
    setting, qs, nl, _ = draw_case(case[0], X)
    for k, v in setting.items():
        device.set_option(k, v)
    num_docs = int(X.docids.max()) + 1
    qi = device.QueryIndex(device.Dictionary(Dd.kind, Dd.file), X.index, X.offsets)
    fd = device.Dictionary(Df.kind, Df.file)
    wand = device.WandData(nl)
    lists = ranked.BuilderLists(X.docids, X.freqs, X.bounds)
    r = np.random.default_rng(case[0] + 4099)
    docs = draw_documents(r, lists, qs, num_docs)
    mods = S.model_batch(lists, qs, docs, nl, num_docs)
    got = qi.score_documents(fd, wand, qs, docs, with_freqs=True)
    assert_model(got, mods, setting)
    assert_model(qi.score_documents(fd, wand, qs, docs), mods, setting)
    assert_model(qi.score_documents(fd, wand, qs[::-1], docs[::-1], with_freqs=True), mods[::-1], ("reversed", setting))
    # the scores of the documents ranked_or returns are that call's
    k = 257
    counts, scores, ids = qi.ranked_or_queries(fd, wand, qs, k=k)
    top = qi.score_documents(fd, wand, qs, [ids[i][:int(counts[i])] for i in range(len(qs))])
    for i in range(len(qs)):
        assert np.array_equal(bits(top[0][i]), bits(scores[i][:int(counts[i])])), (i, setting)
    # one query per call and the lists as the oracle decodes them from the index bytes, on a sample
    ol = OracleLists(Dd.kind, Dd.file, Df.file, X.index, X.offsets)
    for i in range(0, len(qs), 7):
        one = qi.score_documents(fd, wand, [qs[i]], [docs[i]], with_freqs=True)
        assert_model(one, [mods[i]], (i, setting))
        assert_model(one, [S.score_documents(ol, qs[i], docs[i], nl, num_docs)], ("oracle", i))
    qi.close()
    wand.close()
