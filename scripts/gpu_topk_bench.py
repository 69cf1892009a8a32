#!/usr/bin/env python3
"""GPU box: ssw_gpu_search_topk at BASELINE config 5's full size (protein_config(0): 50 000 queries x 10 000 entries, BLOSUM50, gaps 3/1,
score only) against what a caller does today with ssw_gpu_search_db.  The queries and the database are uploaded once; the variants are
timed alternately, `reps` rounds in one process (wall clock of the call, plus its ssw_gpu_last_timing):
  (a)  search_db with a no-op chunk function (the 8 GB of compact records still cross PCIe);
  (b)  search_db with a numpy top-10 per query in the chunk function (what a user writes today);
  (c)  search_topk score-only, k = 10 and k = 100 (selection on the device, lists downloaded once);
  (d)  search_topk k = 10, flag 0x0f (filterd 32767): begin positions and CIGARs of the 500 000 selected pairs.
One JSON line (and the file `out` when given).  --only-topk: just (c), once each (for a rocprofv3 --kernel-trace --stats run).

usage: gpu_topk_bench.py [queries=50000] [reps=3] [out.json] [--only-topk]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
import ssw_amd           # noqa: E402
import workloads as W    # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ONLY_TOPK = "--only-topk" in sys.argv
NQ = int(args[0]) if len(args) > 0 else 50000
REPS = int(args[1]) if len(args) > 1 else 3
OUT = args[2] if len(args) > 2 else None


def numpy_top10(nq, k=10):
    """the caller-side selection of today: a running top-k per query merged in every chunk function call"""
    state = {"key": np.zeros((nq, k), dtype=np.int64)}

    def on_chunk(t0, hits):
        s = hits["score1"].astype(np.int64)
        ok = (hits["ref_end2"] != -2) & (s > 0)
        t = np.arange(t0, t0 + hits.shape[1], dtype=np.int64)
        key = np.where(ok, (s << 32) | (0xffffffff - t)[None, :], 0)
        kk = min(k, key.shape[1])
        top = np.take_along_axis(key, np.argpartition(-key, kk - 1, axis=1)[:, :kk], axis=1)
        both = np.concatenate([state["key"], top], axis=1)
        state["key"] = -np.sort(-both, axis=1)[:, :k]
        return 0
    return on_chunk, state


def main():
    db, qs, mat = W.protein_config(0, queries=NQ)
    ctx = ssw_amd.Context(0)
    ctx.set_exclusive()
    Q = ctx.upload(qs); T = ctx.upload(db)
    cells = float(sum(len(q) for q in qs)) * float(sum(len(t) for t in db))
    runs = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
        tm = ctx.timing()
        runs.setdefault(name, []).append({"wall_s": wall, "fill_ms": tm["fill_ms"], "reduce_ms": tm["reduce_ms"], "locate_ms": tm["locate_ms"],
                                          "trace_ms": tm["trace_ms"], "total_ms": tm["total_ms"]})
        print("%-24s %8.3f s  fill %8.1f ms  reduce/select %7.1f ms  locate %7.1f ms  trace %7.1f ms" % (
            name, wall, tm["fill_ms"], tm["reduce_ms"], tm["locate_ms"], tm["trace_ms"]), file=sys.stderr, flush=True)
        return out

    try:
        if ONLY_TOPK:
            timed("c_topk10", lambda: ctx.search_topk(Q, T, 10, mat, 24, gapO=3, gapE=1, want_cigar=False))
            timed("c_topk100", lambda: ctx.search_topk(Q, T, 100, mat, 24, gapO=3, gapE=1, want_cigar=False))
            return
        check = {}
        for rep in range(REPS):
            timed("a_search_db_noop", lambda: ctx.search_db(Q, T, mat, 24, 3, 1, -1, 2, 0, lambda t0, h: 0))
            fn, st = numpy_top10(len(qs))
            timed("b_search_db_numpy_top10", lambda: ctx.search_db(Q, T, mat, 24, 3, 1, -1, 2, 0, fn))
            ti10, r10, _ = timed("c_topk10", lambda: ctx.search_topk(Q, T, 10, mat, 24, gapO=3, gapE=1, want_cigar=False))
            timed("c_topk100", lambda: ctx.search_topk(Q, T, 100, mat, 24, gapO=3, gapE=1, want_cigar=False))
            tf, rf, cig = timed("d_topk10_flag15", lambda: ctx.search_topk(Q, T, 10, mat, 24, gapO=3, gapE=1, flag=0x0f, filterd=32767))
            if rep == 0:      # the device lists = the numpy lists of (b); flag 0x0f keeps them and adds CIGARs
                nk = st["key"]
                exp_t = np.where(nk > 0, 0xffffffff - (nk & 0xffffffff), -1).astype(np.int64)
                check = {"device_lists_equal_numpy_top10": bool((ti10 == exp_t).all()), "flag15_lists_equal": bool((tf == ti10).all()),
                         "cigar_words_k10": int(len(cig)), "hits_k10": int((ti10 >= 0).sum())}
    finally:
        Q.free(); T.free(); ctx.close()
    med = {k: float(np.median([r["wall_s"] for r in v])) for k, v in runs.items()}
    sel = {k: float(np.median([r["reduce_ms"] for r in v])) for k, v in runs.items() if k.startswith(("c_", "d_"))}
    fill = float(np.median([r["fill_ms"] for r in runs["c_topk10"]]))
    res = {"workload": "config 5 full size: %d protein queries x %d entries, BLOSUM50, gaps 3/1" % (NQ, len(db)), "reps": REPS,
           "median_wall_s": med, "gcups": {k: cells / v / 1e9 for k, v in med.items()},
           "k_topk_device_ms": sel, "fill_ms_c_topk10": fill, "k_topk_share_of_fill_k10": sel["c_topk10"] / fill if fill else None,
           "k_topk_share_of_fill_k100": sel["c_topk100"] / fill if fill else None,
           "ratio_c10_over_a": med["c_topk10"] / med["a_search_db_noop"], "ratio_c100_over_a": med["c_topk100"] / med["a_search_db_noop"],
           "ratio_c10_over_b": med["c_topk10"] / med["b_search_db_numpy_top10"], "ratio_d_over_c10": med["d_topk10_flag15"] / med["c_topk10"],
           "runs": runs, "check": check}
    line = json.dumps(res)
    print(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
