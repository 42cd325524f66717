#!/usr/bin/env python3
"""OR-query timing next to AND on the same index: the reference's op_perftest shape (src/queries.cpp:15-61 —
every query on its own, avg/q50/q90/q95 in µs) and the whole log as one call, for dint_or_queries and dint_and_queries, plus
one CPU core answering the same unions (tools/or_union_cpu.cpp: the reference's or_query loop over lists the CPU oracle
decoded beforehand — the union alone, no decode in the timed region).

    python tests/or_query_timing.py [--postings 1e8] [--type single_packed_dint] [--runs 3]

Lives under tests/ because it decodes the lists with the CPU oracle (test infrastructure), as tests/query_timing.py does.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def _cpu_union_lib(tmp):
    so = os.path.join(tmp, "libor_union_cpu.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "or_union_cpu.cpp")], check=True)
    lib = C.CDLL(so)
    lib.or_union_count.restype = C.c_uint64
    lib.or_union_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--postings", type=float, default=1e8)
    ap.add_argument("--type", default="single_packed_dint")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch
    from dint_amd import device, host
    from queries import heavy_queries, reference_queries
    import oracle

    kind = host.KIND_BY_TYPE[args.type]
    coll = host.synth_collection(int(args.postings), seed=11)  # (tests/query_timing.py's index)
    docids = host.gaps_to_docids(coll)
    freqs = np.ones(coll.num_postings, dtype=np.uint32)
    dd = host.build_dictionary(kind, coll, max_sample_ints=50_000_000)
    fd = host.build_dictionary(kind, host.Collection(freqs[:1000] - 1, np.array([1000], dtype=np.uint32)))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, coll.lens)
    bounds = coll.list_bounds()
    n_lists = len(coll.lens)
    workloads = {
        "reference_log_mod_lists": reference_queries(n_lists),
        "longest_lists": heavy_queries(coll.lens, 500, pool=256, max_terms=5),
    }
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    od, ofd = oracle.OracleDict(kind, dd), oracle.OracleDict(kind, fd)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"postings": coll.num_postings, "lists": n_lists, "blocks": int(len(qi.blocks)), "type": args.type,
           "device": torch.cuda.get_device_name(0)}
    pct = lambda a, p: float(a[min(len(a) - 1, int(p * len(a) / 100))])
    with tempfile.TemporaryDirectory() as tmp:
        lib = _cpu_union_lib(tmp)
        decoded = {}
        for name, qs in workloads.items():
            terms, qoffs = device._pack_queries(qs)
            res = {"queries": len(qs)}
            for what, call in (("or", qi.or_queries_packed), ("and", qi.and_queries_packed)):
                counts = np.zeros(len(qs), dtype=np.uint64)
                call(terms, qoffs, counts, stream)  # (warm-up)
                t_batch = []
                for _ in range(max(args.runs, 5)):
                    t0 = time.perf_counter()
                    call(terms, qoffs, counts, stream)
                    t_batch.append(time.perf_counter() - t0)
                packed = [(np.ascontiguousarray(q, dtype=np.uint32), np.array([0, len(q)], dtype=np.uint64), np.zeros(1, dtype=np.uint64))
                          for q in qs]
                for t, o, c in packed:
                    call(t, o, c, stream)
                us = []
                for _ in range(args.runs - 1):
                    for (t, o, c), want in zip(packed, counts):
                        t0 = time.perf_counter()
                        call(t, o, c, stream)
                        us.append((time.perf_counter() - t0) * 1e6)
                        assert int(c[0]) == int(want)
                us = np.sort(np.array(us))
                res[what] = {"results": int(counts.sum()), "gpu_batch_us_per_query": min(t_batch) * 1e6 / len(qs),
                             "gpu_single": {"avg": float(us.mean()), "q50": pct(us, 50), "q90": pct(us, 90), "q95": pct(us, 95)}}
                if what == "or":
                    or_counts = counts.copy()
            # one CPU core: the reference's or_query loop over the oracle-decoded lists (decode untimed)
            cpu, cpu_counts = [], []
            for q in qs:
                ts = [int(t) for t in np.unique(q)]
                for t in ts:
                    if t not in decoded:
                        decoded[t] = oracle.posting_list_decode(od, ofd, idx, int(offs[t]))[0]
                        assert np.array_equal(decoded[t], docids[int(bounds[t]):int(bounds[t + 1])])
                ptrs = (C.c_void_p * max(1, len(ts)))(*[decoded[t].ctypes.data for t in ts])
                lens = np.array([decoded[t].size for t in ts] or [0], dtype=np.uint64)
                t0 = time.perf_counter()
                n = lib.or_union_count(ptrs, lens.ctypes.data, len(ts))
                cpu.append((time.perf_counter() - t0) * 1e6)
                cpu_counts.append(n)
            assert np.array_equal(np.array(cpu_counts, dtype=np.uint64), or_counts)
            cpu = np.sort(np.array(cpu))
            res["cpu_one_core_or_union"] = {"avg": float(cpu.mean()), "q50": pct(cpu, 50), "q90": pct(cpu, 90), "q95": pct(cpu, 95),
                                            "note": "tools/or_union_cpu.cpp over the oracle-decoded lists: the union alone, no decode"}
            res["or_pages_q50_q90"] = [float(np.percentile([sum(-(-int(coll.lens[t]) // 256) for t in np.unique(q)) for q in qs], p))
                                       for p in (50, 90)]
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
