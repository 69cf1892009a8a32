#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_windows_best (the best candidate window of every read, selected on the device) next to the two ways a caller
reaches the same answer without it, on the same candidate list, in one process, the variants ALTERNATING inside every repeat.

Workload: 150-bp reads (gpu_windows_bench.py's: ~2 % substitutions, an indel in one of five), `--cands` candidates per read -- the true
window at a random position of the group plus decoys elsewhere, windows of 300..700 bp of one resident 100 Mb target.

Variants (flag 0, and flag 2 with CIGARs):
  a  best          Context.align_windows_best                                                      -- this library
  b  two_calls     align_windows flag 0 over all candidates + numpy segmented top-2 (reported on its own) + align_windows with the flag
                   over the winners                                                                -- `--baseline-lib`, else this library
  c  all_flagged   ONE align_windows with the flag over all candidates + the same numpy selection  -- `--baseline-lib`, else this library
The outputs of a and b must be equal (selection, records, CIGAR words) or the script fails.  Every figure is the median of `--reps` timed
repeats after one warm-up, with min and max.  The yardstick is b on the BASELINE library (a build of the commit before this entry
point): a is faster when the difference exceeds twice b's max - min; nothing else is tuned.

usage: gpu_windows_best_bench.py [--reads 1000000] [--cands 4] [--reps 5] [--baseline-lib PATH] [--out out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssw_amd          # noqa: E402
from gpu_windows_bench import GENOME, stats, upload, workload   # noqa: E402
from sswutil import dna_matrix   # noqa: E402

PHASES = ("total_ms", "fill_ms", "reduce_ms", "locate_ms", "trace_ms")
MAT = dna_matrix(2, 2)


def candidates(nreads, ncand, tbeg, tlen, seed=2):
    rng = np.random.default_rng(seed)
    n = nreads * ncand
    cb = rng.integers(0, GENOME - 700, size=n).astype(np.int64)
    cl = rng.integers(300, 701, size=n).astype(np.int32)
    planted = rng.integers(0, ncand, size=nreads)
    at = np.arange(nreads, dtype=np.int64) * ncand + planted
    cb[at] = tbeg; cl[at] = tlen
    own = np.repeat(tbeg, ncand)                  # a decoy that comes near its read's own window moves half a target away
    clash = (np.abs(cb - own) < 1400) & (np.arange(n) != np.repeat(at, ncand))
    cb[clash] = (own[clash] + GENOME // 2) % (GENOME - 700)
    cand_off = np.arange(nreads + 1, dtype=np.int64) * ncand
    return cand_off, np.repeat(np.arange(nreads, dtype=np.int32), ncand), cb, cl, planted


def select_numpy(res, cand_off, min_score=0):
    """segmented top-2 over all candidates' records (no empty groups): score1 descending, then position ascending -> best, second, n_eligible"""
    ok = (res["status"] == 0) & (res["score1"] > 0) & (res["score1"] >= min_score)
    pos = np.arange(len(res), dtype=np.int64) - np.repeat(cand_off[:-1], np.diff(cand_off))
    key = np.where(ok, (res["score1"].astype(np.int64) << 32) | (0xffffffff - pos), 0)
    k1 = np.maximum.reduceat(key, cand_off[:-1])
    best = np.where(k1 > 0, 0xffffffff - (k1 & 0xffffffff), -1)
    key2 = key.copy()
    key2[(cand_off[:-1] + best)[best >= 0]] = 0
    k2 = np.maximum.reduceat(key2, cand_off[:-1])
    second = np.where(k2 > 0, 0xffffffff - (k2 & 0xffffffff), -1)
    return best, second, np.add.reduceat(ok.astype(np.int32), cand_off[:-1]), (k2 >> 32).astype(np.uint16)


def phases(ctx):
    t = ctx.timing()
    return {k: t.get(k, 0.0) for k in PHASES}


def run_best(ctx, Q, T, W, flag):
    t0 = time.perf_counter()
    sel, res, cig = ctx.align_windows_best(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=flag, want_cigar=flag != 0)
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    row = dict(wall_ms=wall, **{k: t[k] for k in PHASES})
    row["host_remainder_ms"] = wall - t["fill_ms"] - t["reduce_ms"] - t["locate_ms"] - t["trace_ms"]
    return row, (sel["best"].astype(np.int64), sel["second"].astype(np.int64), sel["n_eligible"], sel["second_score1"], res, cig), t["best_flagged"]


def run_two_calls(ctx, Q, T, W, flag):
    co = W["cand_off"]
    t0 = time.perf_counter()
    res, _ = ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=0, want_cigar=False)
    t1 = time.perf_counter()
    p1 = phases(ctx)
    best, second, ne, s2 = select_numpy(res, co)
    assert (best >= 0).all()      # (this workload: every read has a candidate that scores)
    win = co[:-1] + best
    t2 = time.perf_counter()
    p2 = {k: 0.0 for k in PHASES}
    if flag:
        wres, cig = ctx.align_windows(Q, T, W["qidx"][win], W["tidx"][win], W["tbeg"][win], W["tlen"][win], MAT, 5, flag=flag)
        p2 = phases(ctx)
    else:
        wres, cig = res[win], np.zeros(0, dtype=np.uint32)
    t3 = time.perf_counter()
    row = dict(wall_ms=(t3 - t0) * 1e3, call1_wall_ms=(t1 - t0) * 1e3, numpy_select_ms=(t2 - t1) * 1e3, call2_wall_ms=(t3 - t2) * 1e3,
               wall_without_numpy_ms=(t3 - t0 - (t2 - t1)) * 1e3, **{k: p1[k] + p2[k] for k in PHASES})
    return row, (best, second, ne, s2, wres, cig)


def run_all_flagged(ctx, Q, T, W, flag):
    co = W["cand_off"]
    t0 = time.perf_counter()
    res, cig = ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=flag)
    t1 = time.perf_counter()
    p1 = phases(ctx)
    best, second, ne, s2 = select_numpy(res, co)
    wres = res[co[:-1] + best]
    t2 = time.perf_counter()
    return dict(wall_ms=(t2 - t0) * 1e3, call_wall_ms=(t1 - t0) * 1e3, numpy_select_ms=(t2 - t1) * 1e3, **p1), None


def same(a, b):
    return bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all() and (a[4] == b[4]).all() and
                a[5].tobytes() == b[5].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    genome, rcodes, roff, tbeg, tlen = workload(args.reads)
    co, qidx, cb, cl, planted = candidates(args.reads, args.cands, tbeg, tlen)
    W = dict(cand_off=co, qidx=qidx, tidx=np.zeros(len(qidx), dtype=np.int32), tbeg=cb, tlen=cl)
    new = ssw_amd.Context(0, ssw_amd.load(None))
    base = new
    if args.baseline_lib:      # a second library in the same process: its own context, its own copy of the reads and the target
        base = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib))
    sets = {}
    for c in {id(new): new, id(base): base}.values():
        sets[id(c)] = (upload(c, rcodes, roff), upload(c, genome, np.array([0, GENOME], dtype=np.int64)))
    variants = [("a_best_flag0", lambda: run_best(new, *sets[id(new)], W, 0)), ("b_two_calls_flag0", lambda: run_two_calls(base, *sets[id(base)], W, 0)),
                ("a_best_flag2", lambda: run_best(new, *sets[id(new)], W, 2)), ("b_two_calls_flag2", lambda: run_two_calls(base, *sets[id(base)], W, 2)),
                ("c_all_flagged_flag2", lambda: run_all_flagged(base, *sets[id(base)], W, 2))]
    rows = {name: [] for name, _ in variants}
    equal = {}
    flagged = {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        outs = {}
        for name, fn in variants:
            r = fn()
            outs[name] = r[1]
            if name.startswith("a_"):
                flagged[name] = int(r[2])
            if rep > 0:
                rows[name].append(r[0])
        for f in ("flag0", "flag2"):
            equal[f] = same(outs["a_best_" + f], outs["b_two_calls_" + f])
            if not equal[f]:
                raise SystemExit("align_windows_best and the two-call path disagree at %s" % f)
        assert (outs["a_best_flag0"][0] == planted).all()
        sys.stderr.write("[gpu_windows_best_bench] repeat %d done\n" % rep); sys.stderr.flush()
    out = {"script": "gpu_windows_best_bench", "reads": args.reads, "candidates_per_read": args.cands, "reps": args.reps,
           "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)", "outputs_equal": equal, "best_flagged": flagged,
           "variants": {name: stats(v) for name, v in rows.items()}}
    cmpd = {}
    for f in ("flag0", "flag2"):
        a = out["variants"]["a_best_" + f]["wall_ms"]; b = out["variants"]["b_two_calls_" + f]
        for col in ("wall_ms", "wall_without_numpy_ms"):
            margin = 2 * (b[col]["max"] - b[col]["min"])
            cmpd[f + "_vs_b_" + col] = {"a_median": a["median"], "b_median": b[col]["median"], "difference": b[col]["median"] - a["median"],
                                        "margin_2x_b_spread": margin, "a_faster_beyond_margin": bool(b[col]["median"] - a["median"] > margin)}
    out["comparison"] = cmpd
    for c in {id(new): new, id(base): base}.values():
        for s in sets[id(c)]:
            s.free()
        c.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
