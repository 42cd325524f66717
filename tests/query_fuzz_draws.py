"""The seeded draws of a query-fuzz case (tests/test_gpu_query_fuzz.py's run_query_case, replayed without a GPU by
tests/test_ranked_or_maxscore_cpu.py): the query options, the query mix, the norm_lens class and array and the two k, all
from one generator seeded with the case seed + 17, in this order. Both files take them from draw_case, so that the CPU
replay sees exactly the queries, norm_lens and k the device is given."""
import numpy as np

KS = (1, 2, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024)
CHOICES = {"query_batch_fused": [0, 1, 1], "query_fused_pages": [0, 2, 8], "query_tail_pages": [0, 1, 4, 16],
           "query_lean_pages": [-1, -1, 0, 1, 3], "query_fused_copy": [0, 1],
           "query_or_pass_pages": [1, 2, 3, 5, 8, 64, 1 << 20]}
NORM_LENS = ("random", "equal", "zeros", "large")


def query_mix(r, lens):
    """Empty and single-term queries, repeated terms (qf > 1), small queries of any lists (the workgroup-per-query form)
    and large ones over the longest lists in the same call (the mixed-call split), queries of 8 to 32 terms; shuffled."""
    n = len(lens)
    big = np.argsort(-lens.astype(np.int64), kind="stable")[:14]
    qs = [[], []]
    qs += [[int(t)] for t in r.choice(n, 6, replace=False)] + [[int(t)] for t in r.choice(big, 3)]
    for _ in range(6):
        a, b = (int(t) for t in r.choice(big, 2))
        qs.append([a, b, a] if r.random() < 0.5 else [a, a])
    qs += [r.integers(0, n, int(r.integers(2, 5))).tolist() for _ in range(24)]
    qs += [r.choice(big, int(r.integers(2, 5))).tolist() for _ in range(10)]
    qs += [r.choice(big[:6], int(r.integers(8, 33))).tolist() for _ in range(5)]
    qs += [r.integers(0, n, int(r.integers(8, 33))).tolist() for _ in range(4)]
    return [qs[i] for i in r.permutation(len(qs))]


def draw_norm_lens(r, num_docs, cls):
    nl = (r.random(num_docs) * 3 + 0.05).astype(np.float32)
    if cls == "equal":  # mass ties
        nl[:] = 1.0
    elif cls == "zeros":
        nl[r.random(num_docs) < 0.3] = 0.0
    elif cls == "large":  # q_weight * w down to subnormal floats
        big = r.random(num_docs) < 0.02
        nl[big] = (10.0 ** r.uniform(30, 38.4, int(big.sum()))).astype(np.float32)
    return nl


def draw_case(seed: int, X, setting=None):
    """-> (the query options, the queries, norm_lens over every docID of the case, the two k). A given `setting` (the soak's
    --random-options) takes the place of the options' draw."""
    r = np.random.default_rng(seed + 17)
    if setting is None:
        setting = {k: int(r.choice(v)) for k, v in CHOICES.items()}
    qs = query_mix(r, np.diff(X.bounds))
    num_docs = int(X.docids.max()) + 1
    nl = draw_norm_lens(r, num_docs, NORM_LENS[int(r.integers(0, len(NORM_LENS)))])
    ks = [int(k) for k in r.choice(KS, 2, replace=False)]
    return setting, qs, nl, ks
