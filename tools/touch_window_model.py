#!/usr/bin/env python3
"""Development aid (CPU only): how well a stream-touch window rule (dint_stream_touch.hpp) fits the streams bench.py decodes —
the numbers behind DESIGN.md section 4e's "window sized by each unit's bytes". For `gov2`, `gov2-bpi59` and `gov2-freqs` it builds the
bench's dictionary (from the collection's first lists, as bench.py does), encodes a sample of the bench's collection — runs of
consecutive lists spaced evenly over all of it, --postings in all — with host.encode_vroom at the bench's unit length, and lays
every rule over the unit table:
  * shipped-before: stream_touch(in_off, n, enc_bytes) — n * 19 / 32 bytes expected, 64 lines at the most;
  * exact spans (a unit's bytes = up to the next unit's first byte, as the kernel reads it from the table) at 64, 96 and 128
    lines, and at 128 lines with 1536 bytes past the unit's end (the next unit's first three tiles).
Per rule, over the stream's bytes: `uncovered` — bytes of units above 12000 integers behind their third tile that no window
holds (they still come through HBM-latency pair requests); `over` — bytes touched behind the touching unit's last byte;
`touched` — all bytes touched; and the share of the units above 12000 integers that reach past their window.
(The freqs sample draws its values with the bench's law from a generator of its own per run of lists: the same distribution,
not the bench's very integers — bench.py seeds one generator per 1e9-posting piece.)

usage: tools/touch_window_model.py [--postings 1.5e8] [--runs 48] [--workloads gov2,gov2-bpi59,gov2-freqs] > profiles/r09_touch_window_model.txt"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
from dint_amd import host

# bench.py's WORKLOADS (the rows this tool knows), its seed, unit length and dictionary sample
WORKLOADS = {
    "gov2": dict(universe=25_000_000, postings=5.0e9),
    "gov2-bpi59": dict(universe=25_000_000, postings=2.0e9, synth=dict(stay_cluster=0.78, p_cluster_min=0.38, p_cluster_max=0.88)),
    "gov2-freqs": dict(universe=25_000_000, postings=1.0e9, values="freqs", freq_p=(0.17, 0.5)),
}
SEED, UNIT_INTS, DICT_SAMPLE = 12345, 16384, 20_000_000
LINE, PROLOGUE, LONG_N = 128, 1536, 12000

ap = argparse.ArgumentParser()
ap.add_argument("--postings", type=float, default=1.5e8)
ap.add_argument("--runs", type=int, default=48)
ap.add_argument("--workloads", default="gov2,gov2-bpi59,gov2-freqs")
args = ap.parse_args()


def window_by_n(in_off, n, enc_bytes, cap=64):
    """stream_touch, vectorised: -> (first line's byte offset, lines)."""
    tile3 = in_off + PROLOGUE
    est = np.minimum(n, 1 << 20) * 19 // 32
    line = tile3 // LINE * LINE
    want = -(-(tile3 - line + est - PROLOGUE) // LINE)
    fit = np.where(enc_bytes - line >= 4, (enc_bytes - line - 4) // LINE + 1, 0)
    lines = np.minimum(np.minimum(want, cap), fit)
    lines = np.where((tile3 >= enc_bytes) | (est <= PROLOGUE), 0, lines)
    return line, lines


def window_by_span(in_off, span, enc_bytes, cap, past=0):
    """stream_touch_span, vectorised."""
    tile3 = in_off + PROLOGUE
    line = tile3 // LINE * LINE
    want = (in_off + span + past - 1) // LINE - line // LINE + 1
    fit = np.where(enc_bytes - line >= 4, (enc_bytes - line - 4) // LINE + 1, 0)
    lines = np.minimum(np.minimum(want, cap), fit)
    lines = np.where((tile3 >= enc_bytes) | (span <= PROLOGUE), 0, lines)
    return line, lines


def sample(name, w):
    """-> (stream bytes, in_off, n, span) of the sample's units."""
    p = host.synth_params(universe=w["universe"], seed=SEED, **w.get("synth", {}))
    lens_all = host.synth_lengths(p, int(w["postings"]))
    cum = np.cumsum(lens_all, dtype=np.uint64)
    total = int(cum[-1])

    def lists(a, b):
        if w.get("values") == "freqs":
            r = np.random.default_rng([SEED, a])
            p_lo, p_span = w["freq_p"]
            p_list = np.repeat(p_lo + p_span * r.random(b - a), lens_all[a:b])
            return (r.geometric(p_list) - 1).astype(np.uint32)
        return host.synth_gaps(p, lens_all[a:b], first_list_id=a)

    # the dictionary: bench.py builds it from a prefix sample of DICT_SAMPLE integers of its first piece — the lists up to that
    # many postings give the same file (freqs: the same law, see above)
    j = max(1, int(np.searchsorted(cum, DICT_SAMPLE, side="right")))
    j = min(j, len(lens_all))
    dict_file = host.build_dictionary(host.SINGLE_PACKED, host.Collection(lists(0, j), lens_all[:j]), max_sample_ints=DICT_SAMPLE)

    per_run = args.postings / args.runs
    in_offs, ns, spans, stream_bytes, postings = [], [], [], 0, 0
    for k in range(args.runs):
        a = int(np.searchsorted(cum, total * k // args.runs, side="left"))
        a = min(a + (1 if k else 0), len(lens_all) - 1)
        b = int(np.searchsorted(cum, int(cum[a]) - int(lens_all[a]) + per_run, side="left")) + 1
        b = min(max(b, a + 1), len(lens_all))
        coll = host.Collection(lists(a, b), lens_all[a:b])
        enc, units = host.encode_vroom(host.SINGLE_PACKED, dict_file, coll, unit_ints=UNIT_INTS)
        off = units["in_off"].astype(np.int64)
        in_offs.append(off + stream_bytes)
        ns.append(units["n"].astype(np.int64))
        spans.append(np.diff(np.concatenate([off, [enc.size]])))
        stream_bytes += enc.size
        postings += coll.num_postings
    return postings, stream_bytes, np.concatenate(in_offs), np.concatenate(ns), np.concatenate(spans)


def report(label, in_off, n, span, stream_bytes, line, lines):
    end = in_off + span                               # one past the unit's last byte (the next unit's list header included)
    covered_to = np.where(lines > 0, line + LINE * lines, 0)
    covered_to = np.maximum(covered_to, in_off + PROLOGUE)
    long_ = n > LONG_N
    uncovered = np.maximum(0, end - covered_to)
    over = np.where(lines > 0, np.maximum(0, line + LINE * lines - np.maximum(end, line)), 0)
    past = long_ & (uncovered > 0)
    print(f"  {label:34s} uncovered {uncovered[long_].sum() / stream_bytes:6.3f} ({uncovered[long_].sum() / 1024 / max(1, long_.sum()):5.2f} KB a long unit)"
          f"   over {over.sum() / stream_bytes:6.3f}   touched {LINE * lines.sum() / stream_bytes:6.3f}   long units past the window {past.sum() / max(1, long_.sum()):6.3f}"
          f"   with a second load {np.mean(lines[long_] > 64):6.3f}")


for name in args.workloads.split(","):
    t = time.time()
    postings, stream_bytes, in_off, n, span = sample(name, WORKLOADS[name])
    long_ = n > LONG_N
    print(f"{name}: {postings} postings of {int(WORKLOADS[name]['postings'])} in {args.runs} runs of lists, {stream_bytes} B = {8 * stream_bytes / postings:.3f} bits/int, "
          f"{len(n)} units, {int(long_.sum())} above {LONG_N} integers holding {n[long_].sum() / postings:.3f} of the integers and "
          f"{span[long_].sum() / stream_bytes:.3f} of the bytes ({time.time() - t:.0f} s)")
    q = np.percentile(span[long_], [1, 5, 25, 50, 75, 95, 99, 100]) / 1024
    print("  span of a long unit, KB: percentile 1 / 5 / 25 / 50 / 75 / 95 / 99 / max  " + " / ".join(f"{v:.1f}" for v in q) + f"   mean {span[long_].mean() / 1024:.1f}")
    report("sized from n, 64 lines (before)", in_off, n, span, stream_bytes, *window_by_n(in_off, n, stream_bytes))
    for cap in (64, 96, 128):
        report(f"exact spans, {cap} lines", in_off, n, span, stream_bytes, *window_by_span(in_off, span, stream_bytes, cap))
    report("exact spans, 128 lines, 1536 past", in_off, n, span, stream_bytes, *window_by_span(in_off, span, stream_bytes, 128, 1536))
    sys.stdout.flush()
