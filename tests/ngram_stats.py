"""A plain model of the device's n-gram statistics (dint_count_ngrams, dint_select_ngrams: include/dint_hip.h "block
statistics on the device"), written from the header's and the kernels' contracts in Python and numpy alone; the named
cases and the seeded fuzz draws that tests/test_ngram_stats_cpu.py (model against the oracle and the host library) and
tests/test_gpu_ngram_stats.py (device against the model) share.

An entry is one distinct (context, n-gram): count() gives them as a dict, entries_of() as the C struct (NGRAM_DTYPE =
dint_ngram = dinth_ngram) that select() and cut() take and return."""
import numpy as np

BLOCK = 256                      # a chunk of a list; a block of the multi-dictionary flavour
WIDTHS = (16, 8, 4, 2, 1)        # the aligned n-grams counted in a chunk: 16 + 32 + 64 + 128 + 256 = 496 at most
NGRAMS_PER_CHUNK = 496
M32 = 0xFFFFFFFF
NGRAM_DTYPE = np.dtype([("pos", "<u8"), ("freq", "<u4"), ("len", "u1"), ("ctx", "u1"), ("pad", "<u2")])
# a block's maximum on either side of every context boundary, and where the 32-bit `max + 1` wraps
CONTEXT_EDGES = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 15: 2, 16: 3, 255: 3, 256: 4, 65535: 4, 65536: 5, 0xFFFFFFFE: 5, 0xFFFFFFFF: 0}


def ceil_log2(x: int) -> int:
    return 0 if x <= 1 else (x - 1).bit_length()


def context_of(max_value: int) -> int:
    """the context of a block whose largest integer is max_value: the 1 is added in 32 bits, so 0xFFFFFFFF is context 0"""
    return 0 if max_value <= 1 else ceil_log2(ceil_log2((max_value + 1) % 2**32))


def chunks_of(list_starts, multi: bool):
    """(start, length) of every chunk that is counted: 256 integers aligned to their list's start, the last one of a list
    shorter; with multi only the whole ones"""
    out = []
    for a, b in zip(list_starts[:-1], list_starts[1:]):
        for at in range(int(a), int(b), BLOCK):
            n = min(BLOCK, int(b) - at)
            if not multi or n == BLOCK:
                out.append((at, n))
    return out


def total_of(list_starts) -> int:
    """the integers of the collection, as the filter's total counts them: every list's, the multi tails too"""
    return sum(int(b) - int(a) for a, b in zip(list_starts[:-1], list_starts[1:]))


def count(gaps, list_starts, multi: bool) -> dict:
    """-> {(ctx, n-gram): (freq, first_pos)}"""
    g = [int(x) for x in gaps]
    table = {}
    for start, n in chunks_of(list_starts, multi):
        ctx = context_of(max(g[start:start + n])) if multi else 0
        for w in WIDTHS:
            for pos in range(start, start + n - w + 1, w):
                key = (ctx, tuple(g[pos:pos + w]))
                freq, first = table.get(key, (0, pos))
                table[key] = (freq + 1, min(first, pos))
    return table


def entries_of(counts: dict) -> np.ndarray:
    e = np.zeros(len(counts), dtype=NGRAM_DTYPE)
    for i, ((ctx, ngram), (freq, pos)) in enumerate(sorted(counts.items())):
        e[i] = (pos, freq, len(ngram), ctx, 0)
    return e


def kept(freq: int, length: int, total_ints: int) -> bool:
    """the saving filter, in double and in ngram_kept's order: one multiplication, one division, one comparison"""
    codeword_bits = 16.0
    initial_bpi = 3 * codeword_bits
    saving = float(freq) * (initial_bpi * float(length) - codeword_bits) / float(total_ints)
    return saving > 0.0001 / 1000 or length == 1


def _ngram(gaps, e) -> tuple:
    return tuple(int(x) for x in gaps[int(e["pos"]):int(e["pos"]) + int(e["len"])])


def select(entries: np.ndarray, gaps, total_ints: int, top_k: int) -> np.ndarray:
    """the kept entries of every context in dictionary order — most frequent first, then the longer, then by their integers
    (unsigned) —, the first top_k of each"""
    mine = [e for e in entries if kept(int(e["freq"]), int(e["len"]), total_ints)]
    mine.sort(key=lambda e: (int(e["ctx"]), -int(e["freq"]), -int(e["len"]), _ngram(gaps, e)))
    out, taken = [], {}
    for e in mine:
        c = int(e["ctx"])
        if taken.get(c, 0) < top_k:
            taken[c] = taken.get(c, 0) + 1
            out.append(e)
    return np.array(out, dtype=NGRAM_DTYPE) if out else np.zeros(0, dtype=NGRAM_DTYPE)


def cut_thresholds(entries: np.ndarray, total_ints: int, top_k: int) -> dict:
    """per context that has entries: the top_k-th largest freq among its kept entries, 1 where fewer are kept"""
    t = {}
    for c in sorted({int(x) for x in entries["ctx"]}):
        f = sorted((int(e["freq"]) for e in entries if int(e["ctx"]) == c and kept(int(e["freq"]), int(e["len"]), total_ints)),
                   reverse=True)
        t[c] = f[top_k - 1] if len(f) >= top_k else 1
    return t


def cut(entries: np.ndarray, total_ints: int, top_k: int) -> np.ndarray:
    """what dint_count_ngrams(top_k) returns of `entries` (all of the collection's): everything when there are no more than
    top_k in all; else per context the entries whose freq reaches the threshold, those the filter drops included"""
    if len(entries) <= top_k:
        return entries.copy()
    t = cut_thresholds(entries, total_ints, top_k)
    return entries[[int(e["freq"]) >= t[int(e["ctx"])] for e in entries]]


def cut_profile(entries: np.ndarray, total_ints: int, top_k: int):
    """-> (contexts whose threshold is above 1, those of them with a tie at the threshold — more than top_k come back —,
    contexts that come back whole), all empty where the call cuts nothing because there are no more than top_k entries"""
    if len(entries) <= top_k:
        return set(), set(), set()
    t = cut_thresholds(entries, total_ints, top_k)
    back = cut(entries, total_ints, top_k)
    n_back = {c: int((back["ctx"] == c).sum()) for c in t}
    n_all = {c: int((entries["ctx"] == c).sum()) for c in t}
    above = {c for c in t if t[c] > 1}
    return above, {c for c in above if n_back[c] > top_k}, {c for c in t if n_back[c] == n_all[c]}


def as_set(entries: np.ndarray) -> set:
    return {(int(e["ctx"]), int(e["len"]), int(e["freq"]), int(e["pos"])) for e in entries}


def as_list(entries: np.ndarray) -> list:
    return [(int(e["ctx"]), int(e["len"]), int(e["freq"]), int(e["pos"])) for e in entries]


# ---- the named cases -------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, gaps, lens, multi):
        self.name, self.multi = name, bool(multi)
        self.gaps = np.ascontiguousarray(gaps, dtype=np.uint32)
        self.lens = [int(n) for n in lens]
        self.starts = np.zeros(len(self.lens) + 1, dtype=np.uint64)
        np.cumsum(self.lens, out=self.starts[1:])
        assert int(self.starts[-1]) == self.gaps.size
        self._counts = None

    @property
    def total(self) -> int:
        return total_of(self.starts)

    @property
    def counts(self) -> dict:
        if self._counts is None:
            self._counts = count(self.gaps, self.starts, self.multi)
        return self._counts

    @property
    def entries(self) -> np.ndarray:
        return entries_of(self.counts)

    def ngram(self, e) -> tuple:
        return _ngram(self.gaps, e)


# the lengths around the n-gram widths and around 256; the last list, a second one of 1 integer, makes the chunks 25
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 255, 256, 257, 511, 512, 513)
LENGTHS_LISTS = (0, 1, 2, 0, 3, 4, 5, 0, 0, 7, 8, 9, 15, 16, 0, 17, 31, 33, 255, 0, 256, 257, 0, 511, 512, 513, 0, 1)
CONTEXT_MAXIMA = (0, 1, 2, 3, 4, 15, 16, 255, 256, 65535, 65536, 0xFFFFFFFE, 0xFFFFFFFF)
CONTEXT_MAX_AT = 37                                   # where in its block the maximum stands
TIE_VALUES = (0x80000000, 5, 0xFFFFFFFE, 1, 0x7FFFFFFF, 0x80000001, 2, 0xFFFFFFFD, 0x7FFFFFFE, 3, 0x90000000, 4, 0x70000000,
              0xF0000000, 6, 0x60000000)              # 16 different integers on both sides of 2^31, not in order
TIE_TOP_KS = (1, 2, 7, 8, 9)
FIRST_NGRAMS = ((7,), (8, 7))                         # "first occurrence": last in chunk 0, first in 40 later chunks


def context_filler() -> np.ndarray:
    f = np.zeros(BLOCK, dtype=np.uint32)
    f[3::7] = 1
    return f


def _lengths(multi):
    r = np.random.default_rng(11)
    return Case("multi tails" if multi else "lengths", r.integers(0, 3, sum(LENGTHS_LISTS)), LENGTHS_LISTS, multi)


def _contexts():
    blocks = []
    for m in CONTEXT_MAXIMA:
        b = context_filler() if m else np.zeros(BLOCK, dtype=np.uint32)   # (a block whose maximum is 0 holds no 1)
        b[CONTEXT_MAX_AT] = m
        blocks.append(b)
    return Case("contexts", np.concatenate(blocks), (5 * BLOCK, BLOCK, 7 * BLOCK), True)


def _all_distinct(multi):
    chunk = (np.arange(1, BLOCK + 1, dtype=np.uint64) * 2654435761 % 2**32).astype(np.uint32)  # 256 different integers
    return Case("all distinct, multi" if multi else "all distinct", np.concatenate([chunk, chunk]), (BLOCK, BLOCK), multi)


def _first_occurrence():
    r = np.random.default_rng(12)
    head = r.integers(0, 3, BLOCK).astype(np.uint32)
    head[-2:] = (8, 7)                                   # the pair is n-gram 239 of its chunk, the 7 n-gram 495
    gaps, lens = [head], [BLOCK]
    for i in range(40):
        n = (2, 3, 5)[i % 3]
        later = r.integers(0, 3, n).astype(np.uint32)
        later[:2] = (8, 7)
        gaps.append(later)
        lens.append(n)
    return Case("first occurrence", np.concatenate(gaps), lens, False)


def _ties():
    """one context; in selection order: 3 entries of freq 7, 5 of freq 6, 31 of freq 5, then the 31 n-grams of TIE_VALUES
    with freq 3 — 1 of 16 integers, 2 of 8, 4 of 4, 8 of 2, 16 of 1 —, then 31 of freq 1"""
    lists = [(100, 101)] * 7 + [(200, 201)] * 6 + [(300,)] * 6 + [(301,)] * 6
    lists += [tuple(range(1000, 1016))] * 5 + [TIE_VALUES] * 3 + [tuple(range(2000, 2016))]
    order = np.random.default_rng(13).permutation(len(lists))
    lists = [lists[i] for i in order]
    return Case("ties", np.concatenate([np.array(x, dtype=np.uint32) for x in lists]), [len(x) for x in lists], False)


def _gaps_in_contexts():
    r = np.random.default_rng(14)
    gaps = r.integers(0, 2, 5 * BLOCK).astype(np.uint32)
    for block, m in ((1, 9), (2, 70000), (3, 4)):        # contexts 0, 2, 5, 2, 0
        gaps[block * BLOCK + 100] = m
    return Case("gaps in contexts", gaps, (2 * BLOCK, 3 * BLOCK), True)


def _no_whole_block():
    r = np.random.default_rng(15)
    lens = [n for n in LENGTHS_LISTS if n < BLOCK]
    return Case("multi, no whole block", r.integers(0, 3, sum(lens)), lens, True)


_CASES = None


def cases() -> dict:
    """the named cases, made once"""
    global _CASES
    if _CASES is None:
        made = [_lengths(False), _lengths(True), _no_whole_block(), _contexts(), _all_distinct(False), _all_distinct(True),
                _first_occurrence(), _ties(), _gaps_in_contexts()]
        _CASES = {c.name: c for c in made}
    return _CASES


CASE_NAMES = ("lengths", "multi tails", "multi, no whole block", "contexts", "all distinct", "all distinct, multi",
              "first occurrence", "ties", "gaps in contexts")


# ---- the fuzz draws --------------------------------------------------------------------------------------------------
FUZZ_DRAWS = 48
FUZZ_MAX_INTS = 2048
FUZZ_TOP_KS = (1, 2, 3, 5, 17, 100)
FUZZ_SEED = 20269   # chosen so that the floors of tests/test_ngram_stats_cpu.py hold: 41 draws cut, 13 with a tie, 12 mixed
_POOL = (0, 1, 2, 3, 7, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE)
_MULTI_POOL = (0, 1, 2, 3, 5, 7)                                   # (the blocks' own maxima: contexts 0, 1 and 2)
_SPREAD = (2, 3, 9, 200, 70000, 0xFFFFFFFE, 0xFFFFFFFF)            # block maxima of contexts 1, 1, 2, 3, 5, 5 and 0
_LONELY = 40000                                                    # context 4: held by one block of few n-grams, or by none
_MULTI_TOP_K_WEIGHTS = (1, 1, 1, 1, 5, 3)                          # (a context comes back whole under the larger ones)


class Draw(Case):
    def __init__(self, i):
        r = np.random.default_rng([FUZZ_SEED, i])
        multi = i % 2 == 1
        pool = _MULTI_POOL if multi else _POOL
        letters = r.choice(len(pool), size=int(r.integers(2, 7)), replace=False)
        alphabet = np.array([pool[j] for j in letters], dtype=np.uint32)
        skew = r.dirichlet(np.full(alphabet.size, 0.6))
        lens, room = [], int(r.choice((300, 700, FUZZ_MAX_INTS))) if not multi else FUZZ_MAX_INTS
        while room > 0 and len(lens) < 12:
            if multi and r.random() < 0.6:
                n = int(r.choice((256, 257, 300, 512, 513, 600)))
            else:
                n = int(r.integers(0, 601)) if r.random() < 0.5 else int(r.integers(0, 40))
            n = min(n, room)
            lens.append(n)
            room -= n
        parts = []
        for n in lens:  # a list is independent draws of the alphabet, or a short motif over and over (few n-grams, equal counts)
            if r.random() < 0.4:
                motif = alphabet[r.choice(alphabet.size, size=int(r.choice((1, 2, 3, 4, 8, 16))))]
                parts.append(np.resize(motif, n))
            else:
                parts.append(alphabet[r.choice(alphabet.size, size=n, p=skew)])
        gaps = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        if multi:  # a maximum into some blocks, so that the collection spreads over contexts
            starts = np.concatenate([[0], np.cumsum(lens)])
            for at, _ in chunks_of(starts, True):
                if r.random() < 0.5:
                    gaps[at + int(r.integers(0, BLOCK))] = _SPREAD[int(r.integers(0, len(_SPREAD)))]
            whole = chunks_of(starts, True)
            if whole and r.random() < 0.8:  # one block alone in its context, a pair over and over: 11 n-grams
                at = whole[int(r.integers(0, len(whole)))][0]
                gaps[at:at + BLOCK] = np.resize(alphabet[:2], BLOCK)
                gaps[at + int(r.integers(0, BLOCK))] = _LONELY
        super().__init__("draw %d" % i, gaps, lens, multi)
        self.alphabet = [int(v) for v in alphabet]
        w = np.array(_MULTI_TOP_K_WEIGHTS if multi else (1,) * len(FUZZ_TOP_KS), dtype=float)
        self.top_k = int(r.choice(FUZZ_TOP_KS, p=w / w.sum()))


_DRAWS = None


def draws() -> list:
    global _DRAWS
    if _DRAWS is None:
        _DRAWS = [Draw(i) for i in range(FUZZ_DRAWS)]
    return _DRAWS


# ---- the filter's boundary -------------------------------------------------------------------------------------------
# freq * (48 * len - 16) / total against 0.0001 / 1000 = 1.0000000000000001e-07 (one ulp above the literal 1e-7): with freq 1
# the saving of a pair is 80 / total, of 4, 8, 16 integers 176, 368, 752 / total; at total = 1e7 times that it is the double
# 1e-07 exactly, which is not above the threshold
FILTER_TOTALS = tuple(m * 10**7 + d for m in (80, 176, 368, 752) for d in (-1, 0, 1))
# savings that ARE the threshold, (freq, len, total): N / (1e7 N - 1) with N = freq * (48 len - 16) near 7e8 is one ulp above
# N / (1e7 N). `>` drops them; `>=`, or a threshold written 1e-7, keeps them. No freq <= 1000 has one (exact_triples below).
EXACT_TRIPLES = ((9_500_000, 2, 7_599_999_999_999_999), (868_388, 16, 6_530_277_759_999_999))


def exact_triples(max_freq: int, lengths=(2, 4, 8, 16), around=2):
    """every (freq, len, total) with freq <= max_freq whose saving in double equals 0.0001 / 1000: the total has to be within
    a few integers of 1e7 * freq * (48 len - 16), everything further away misses by far more than an ulp"""
    t = 0.0001 / 1000
    for length in lengths:
        m = 48 * length - 16
        for freq in range(1, max_freq + 1):
            for total in range(freq * m * 10**7 - around, freq * m * 10**7 + around + 1):
                if float(freq) * float(m) / float(total) == t:
                    yield freq, length, total


def boundary_collection():
    """-> (gaps, entries) with every width once (16 different integers), a pair twice and a single integer three times"""
    lens = [16, 2, 2, 1, 1, 1]
    gaps = np.array(TIE_VALUES + (50, 51, 50, 51, 60, 60, 60), dtype=np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return gaps, starts, entries_of(count(gaps, starts, False))


def with_freq(entries: np.ndarray, length: int, freq: int) -> np.ndarray:
    """the entries with the first one of `length` integers given another count"""
    e = entries.copy()
    e["freq"][np.flatnonzero(e["len"] == length)[0]] = freq
    return e
