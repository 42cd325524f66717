"""docIDs at the top of the u32 range on the GPU: lists ending at 0xFFFFFFFE, straddling 2^31, {0, 0xFFFFFFFE}, lists of
more than 16 pages high in the range among shorter ones, freqs near 2^32 - 1 in full blocks (the u64 freq sums pass
2^32), built with the project's encoder for the three kinds. The decoders and the AND / OR queries against numpy, under
the query forms' options. docID 0xFFFFFFFF is the query kernels' dead-slot mark, not a docID: an index holding it is
refused when the query index is created."""
import numpy as np
import pytest

from dint_amd import host
from or_union import union_freqs
from queries import intersect_freqs

pytestmark = pytest.mark.gpu

DINT_ERR_FORMAT = -2
TOP = 0xFFFFFFFE
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]


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


def _high_lists(r):
    """-> (lists of docIDs, their freqs): full blocks carry freqs near 2^32 - 1; a short (interpolative) block stores the
    sum of its freq - 1 as a u32, so the last block of a list keeps small freqs."""
    hi_pool = np.arange(TOP - 40_000, TOP + 1, dtype=np.uint64)
    lists = [
        np.arange(TOP - 999, TOP + 1, dtype=np.uint64),                                  # ends at 0xFFFFFFFE
        np.sort(r.choice(hi_pool, 6000, replace=False)),                                 # 24 pages, ends near the top
        np.array([0, TOP], dtype=np.uint64),
        np.sort(r.choice(np.arange((1 << 31) - 3000, (1 << 31) + 3000, dtype=np.uint64), 1500, replace=False)),  # 2^31
        np.sort(r.choice(hi_pool, 300, replace=False)),
        np.sort(r.choice(hi_pool, 4353, replace=False)),                                 # 17 pages + 1
        np.concatenate([np.arange(0, 700, 7, dtype=np.uint64), np.sort(r.choice(hi_pool, 900, replace=False))]),
        np.concatenate([np.arange((1 << 31) - 300, (1 << 31) + 300, dtype=np.uint64), [TOP]]),
        np.sort(r.choice(hi_pool, 2, replace=False)),
        np.sort(r.choice(hi_pool, 17 * 256, replace=False)),                             # 17 full pages
    ]
    lists = [np.unique(x).astype(np.uint32) for x in lists]
    freqs = []
    for x in lists:
        n = x.size
        f = r.integers(1, 50, n).astype(np.uint32)
        full = n - n % 256
        if full:
            f[:full] = (0xFFFFFFFF - r.integers(0, 4, full)).astype(np.uint32)
            f[:full][r.random(full) < 0.05] = 0  # freq - 1 wraps to 0xFFFFFFFF: a full block holds it
        freqs.append(f)
    return lists, freqs


class HighIndex:
    def __init__(self, device, kind, lists, freqs):
        self.lens = np.array([x.size for x in lists], dtype=np.uint32)
        self.docids = np.concatenate(lists)
        self.freqs = np.concatenate(freqs)
        self.bounds = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        gaps = np.concatenate([host.docids_to_gaps(x) for x in lists])
        self.dd_bytes = host.build_dictionary(kind, host.Collection(gaps, self.lens))
        self.fd_bytes = host.build_dictionary(kind, host.Collection(self.freqs - np.uint32(1), self.lens))
        self.index, self.offsets = host.build_index(kind, self.dd_bytes, self.fd_bytes, self.docids, self.freqs, self.lens)
        self.dd, self.fd = device.Dictionary(kind, self.dd_bytes), device.Dictionary(kind, self.fd_bytes)


@pytest.mark.parametrize("kind", KINDS)
def test_decoders_at_the_top_of_the_range(device, kind):
    import torch

    r = np.random.default_rng(31 + kind)
    h = HighIndex(device, kind, *_high_lists(r))
    assert int(h.docids.max()) == TOP
    blocks, total = device.index_posting_lists(h.index, h.offsets)
    assert total == h.docids.size and int(blocks["max"].max()) == TOP
    docids, freqs = device.decode_posting_lists(h.dd, h.fd, h.index, blocks, total)
    assert np.array_equal(docids, h.docids) and np.array_equal(freqs, h.freqs)
    dev = torch.device("cuda", 0)
    padded = np.concatenate([h.index, np.zeros(16, np.uint8)])
    index_dev = torch.from_numpy(padded).to(dev)
    taught, plain = device.BlockTable(h.dd, blocks, padded.size), device.BlockTable(h.dd, blocks, padded.size)
    taught.learn(h.dd, h.fd, index_dev, padded.size)
    for table in (taught, plain):
        docids_dev = torch.full((total + 64,), -1, dtype=torch.int32, device=dev)
        freqs_dev = torch.full((total + 64,), -1, dtype=torch.int32, device=dev)
        table.decode(h.dd, h.fd, index_dev, padded.size, docids_dev[:total], freqs_dev[:total])
        torch.cuda.synchronize()
        got_d, got_f = docids_dev.cpu().numpy().view(np.uint32), freqs_dev.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_d[:total], h.docids) and (got_d[total:] == 0xFFFFFFFF).all()
        assert np.array_equal(got_f[:total], h.freqs) and (got_f[total:] == 0xFFFFFFFF).all()
        table.close()


FORMS = [dict(), dict(query_batch_fused=0), dict(query_fused_pages=0, query_tail_pages=0), dict(query_lean_pages=0),
         dict(query_fused_copy=0, query_fused_pages=8, query_tail_pages=16), dict(query_or_pass_pages=1),
         dict(query_or_pass_pages=5, query_lean_pages=1)]


@pytest.mark.parametrize("kind", KINDS)
def test_and_or_queries_at_the_top_of_the_range(device, kind):
    r = np.random.default_rng(77 + kind)
    lists, freqs = _high_lists(r)
    h = HighIndex(device, kind, lists, freqs)
    n = len(lists)
    qs = [[0], [0, 1], [1, 5], [1, 9], [5, 9], [1, 5, 9], [2, 0], [2, 7], [3, 7], [3, 6], [4, 1, 5], [6, 1], [8, 1],
          [0, 2, 7], [9, 9, 1], [], [1, 4, 5, 6, 9], list(range(n)), [2, 3, 7], [3, 3]]
    qs += [r.integers(0, n, int(r.integers(2, 6))).tolist() for _ in range(20)]
    want_and = [intersect_freqs(h.docids, h.freqs, h.bounds, q) for q in qs]
    want_or = [union_freqs(h.docids, h.freqs, h.bounds, q) for q in qs]
    assert max(w[1] for w in want_and) > 1 << 40 and max(w[1] for w in want_or) > 1 << 40  # u64 sums past 2^32
    assert want_and[6][0] == 1 and want_and[13][0] == 1  # {0, 0xFFFFFFFE} meets the lists ending at 0xFFFFFFFE
    qi = device.QueryIndex(h.dd, h.index, h.offsets)
    for opts in FORMS:
        with device.options(**opts):
            assert qi.and_queries(qs).tolist() == [w[0] for w in want_and], opts
            counts, sums, _ = qi.and_queries_with_freqs(h.fd, qs)
            assert list(zip(counts.tolist(), sums.tolist())) == want_and, opts
            assert qi.or_queries(qs).tolist() == [w[0] for w in want_or], opts
            counts, sums, _ = qi.or_queries_with_freqs(h.fd, qs)
            assert list(zip(counts.tolist(), sums.tolist())) == want_or, opts
            for i in range(0, len(qs), 5):
                assert int(qi.and_queries([qs[i]])[0]) == want_and[i][0], (opts, i)
                assert int(qi.or_queries([qs[i]])[0]) == want_or[i][0], (opts, i)
    qi.close()


@pytest.mark.parametrize("kind", KINDS)
def test_docid_0xffffffff_is_refused(device, kind):
    """0xFFFFFFFF marks dead candidate slots in the query kernels (an AND match or a ranked-OR document there would be
    dropped): an index holding it is DINT_ERR_FORMAT at creation; the same lists one lower are answered."""
    for top, ok in ((0xFFFFFFFF, False), (TOP, True)):
        lists = [np.arange(top - 599, top + 1, dtype=np.uint64).astype(np.uint32),
                 np.array([0, 5, top], dtype=np.uint32),
                 np.arange(top - 298, top + 1, 2, dtype=np.uint64).astype(np.uint32)]
        freqs = [np.full(x.size, 2, dtype=np.uint32) for x in lists]
        h = HighIndex(device, kind, lists, freqs)
        if not ok:
            with pytest.raises(device.DintError) as e:
                device.QueryIndex(h.dd, h.index, h.offsets)
            assert e.value.status == DINT_ERR_FORMAT
            # (the decoders take it: docID 0xFFFFFFFF is no problem outside the query kernels)
            blocks, total = device.index_posting_lists(h.index, h.offsets)
            docids, _ = device.decode_posting_lists(h.dd, h.fd, h.index, blocks, total)
            assert np.array_equal(docids, h.docids)
            continue
        qi = device.QueryIndex(h.dd, h.index, h.offsets)
        qs = [[0, 1], [0, 2], [1, 2], [0, 1, 2], [0], [1, 2, 2]]
        assert qi.and_queries(qs).tolist() == [intersect_freqs(h.docids, h.freqs, h.bounds, q)[0] for q in qs]
        assert qi.and_queries(qs).tolist()[:4] == [1, 150, 1, 1]
        assert qi.or_queries(qs).tolist() == [union_freqs(h.docids, h.freqs, h.bounds, q)[0] for q in qs]
        qi.close()
