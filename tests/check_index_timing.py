#!/usr/bin/env python3
"""dint_check_index timing: a synthetic index checked against the collection it was built from, in one
process and on one stream, alternating call by call — postings/s of QueryIndex.check (docIDs and freqs), of
QueryIndex.max_weights (the same decode passes with nothing uploaded) and of the check with docIDs only — and the time the
reference's CPU walk of the same index would take at the oracle's measured 2.3 G ints/s.

    python tests/check_index_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 5] [--pass-pages N] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ORACLE_INTS_PER_S = 2.3e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pass-pages", type=int, default=0, help="query_or_pass_pages (0: the default; the check caps a pass at 16384 pages)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, 13)
    dd = host.build_dictionary(kind, coll, max_sample_ints=20_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs - np.uint32(1), coll.lens), max_sample_ints=20_000_000)
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    num_docs = int(docids.max()) + 1
    norm_lens, _ = host.wand_data(host.sizes_from_postings(docids, freqs, num_docs), docids, freqs, coll.lens)
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    fdd = device.Dictionary(kind, fd)
    wand = device.WandData(norm_lens)
    lens = coll.lens.astype(np.uint64)
    at = (np.cumsum(lens) - lens).astype(np.uint64)  # the lists back to back: the view of the collection's two arrays
    if args.pass_pages:
        device.set_option("query_or_pass_pages", args.pass_pages)

    calls = {"check": lambda: qi.check(fdd, docids, freqs, at, at, lens),
             "max_weights": lambda: qi.max_weights(fdd, wand),
             "check_docids_only": lambda: qi.check(None, docids, None, at, None, lens)}
    for name in ("check", "check_docids_only"):
        for _ in range(4):  # (warm-up: the workspaces, the dictionaries' four schedule slots)
            assert calls[name]() == (0, None), name
    calls["max_weights"]()
    times = {name: [] for name in calls}
    for _ in range(args.runs):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times[name].append(time.perf_counter() - t0)
    n = coll.num_postings
    out = {"postings": n, "lists": len(lens), "blocks": int(len(qi.blocks)), "type": args.type, "device": torch.cuda.get_device_name(0),
           "hip_lib": os.path.basename(os.environ.get("DINT_HIP_LIB") or "libdint_hip.so"),
           "pass_pages": min(device.get_option("query_or_pass_pages"), 16384), "runs": args.runs,
           "seconds": {k: {"best": min(v), "median": float(np.median(v))} for k, v in times.items()},
           "postings_per_s": {k: n / min(v) for k, v in times.items()},
           "reference_cpu_walk_seconds_at_2.3_Gints_per_s": 2 * n / ORACLE_INTS_PER_S}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
