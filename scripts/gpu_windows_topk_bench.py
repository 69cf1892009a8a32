#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_windows_topk (the best k candidate windows of every read, selected on the device) next to the two-call recipe a
caller uses without it, on gpu_windows_best_bench.py's workload, in one process, the variants ALTERNATING inside every repeat.

Workload: 150-bp reads, `--cands` candidates per read -- the true window at a random position of the group plus decoys elsewhere,
windows of 300..700 bp of one resident 100 Mb target.  k = 1, 2 and 4 (`--ks`), flag 0 and flag 2 with CIGARs.

Variants:
  a  topk          Context.align_windows_topk                                                          -- this library
  b  two_calls     align_windows flag 0 over all candidates + numpy top-k (reported on its own) + align_windows with the flag over
                   the chosen pairs                                                                    -- `--baseline-lib`, else this library
  c  all_flagged   ONE align_windows with the flag over all candidates (k-independent, reported only)  -- `--baseline-lib`, else this library
  best             Context.align_windows_best on this library AND on the baseline library (the unchanged path; also the k = 1 comparison)
The outputs of a and b must be equal (positions, eligible counts, records, CIGAR words) or the script fails.  Every figure is the median of
`--reps` timed repeats after one warm-up, with min and max.  The yardstick is b on the BASELINE library (a build of the commit before
this entry point) at the same k: a is faster when the difference exceeds twice b's max - min; the unchanged path is within when the two
builds' medians differ by at most twice the baseline's max - min.  Nothing else is tuned.

usage: gpu_windows_topk_bench.py [--reads 1000000] [--cands 4] [--ks 1,2,4] [--reps 5] [--baseline-lib PATH] [--out out.json]"""
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
from gpu_windows_best_bench import MAT, PHASES, candidates, phases   # noqa: E402


def select_numpy(res, nreads, ncand, k):
    """top-k of every group of `ncand` candidates: score1 descending, then position ascending -> pos [nreads, k] (-1 past the last), n_eligible"""
    ok = (res["status"] == 0) & (res["score1"] > 0)
    p = np.tile(np.arange(ncand, dtype=np.int64), nreads)
    key = np.where(ok, (res["score1"].astype(np.int64) << 32) | (0xffffffff - p), 0).reshape(nreads, ncand)
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    pos = np.where(np.take_along_axis(key, order, axis=1) > 0, order, -1).astype(np.int32)
    if pos.shape[1] < k:
        pos = np.concatenate([pos, np.full((nreads, k - pos.shape[1]), -1, dtype=np.int32)], axis=1)
    return pos, ok.reshape(nreads, ncand).sum(axis=1).astype(np.int32)


def run_topk(ctx, Q, T, W, k, flag):
    t0 = time.perf_counter()
    pos, nel, res, cig = ctx.align_windows_topk(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, k, flag=flag, want_cigar=flag != 0)
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    row = dict(wall_ms=wall, **{f: t[f] for f in PHASES})
    row["host_remainder_ms"] = wall - t["fill_ms"] - t["reduce_ms"] - t["locate_ms"] - t["trace_ms"]
    return row, (pos, nel, res, cig), int(t["best_flagged"])


def run_two_calls(ctx, Q, T, W, k, flag, nreads, ncand):
    t0 = time.perf_counter()
    res, _ = ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=0, want_cigar=False)
    t1 = time.perf_counter()
    p1 = phases(ctx)
    pos, nel = select_numpy(res, nreads, ncand, k)
    hit = pos >= 0
    chosen = (W["cand_off"][:-1, None] + pos)[hit]          # (g, r) order
    out = np.zeros((nreads, k), dtype=ssw_amd.RESULT_DTYPE)
    out["ref_begin1"] = -1; out["read_begin1"] = -1; out["cigar_off"] = -1
    t2 = time.perf_counter()
    p2 = {f: 0.0 for f in PHASES}
    if flag:
        wres, cig = ctx.align_windows(Q, T, W["qidx"][chosen], W["tidx"][chosen], W["tbeg"][chosen], W["tlen"][chosen], MAT, 5, flag=flag)
        p2 = phases(ctx)
    else:
        wres, cig = res[chosen], np.zeros(0, dtype=np.uint32)
    out[hit] = wres
    t3 = time.perf_counter()
    row = dict(wall_ms=(t3 - t0) * 1e3, call1_wall_ms=(t1 - t0) * 1e3, numpy_select_ms=(t2 - t1) * 1e3, call2_wall_ms=(t3 - t2) * 1e3,
               wall_without_numpy_ms=(t3 - t0 - (t2 - t1)) * 1e3, **{f: p1[f] + p2[f] for f in PHASES})
    return row, (pos, nel, out, cig)


def run_all_flagged(ctx, Q, T, W, flag):
    t0 = time.perf_counter()
    ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=flag)
    return dict(wall_ms=(time.perf_counter() - t0) * 1e3, **phases(ctx))


def run_best(ctx, Q, T, W, flag):
    t0 = time.perf_counter()
    sel, res, cig = ctx.align_windows_best(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=flag, want_cigar=flag != 0)
    wall = (time.perf_counter() - t0) * 1e3
    return dict(wall_ms=wall, **phases(ctx)), (sel, res, cig)


def same(a, b):
    return bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3].tobytes() == b[3].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--ks", default="1,2,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [int(x) for x in args.ks.split(",")]
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
    rows, flagged, equal = {}, {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        def keep(name, row):
            if rep > 0:
                rows.setdefault(name, []).append(row)
        for flag in (0, 2):
            f = "flag%d" % flag
            for k in ks:
                ra, oa, nf = run_topk(new, *sets[id(new)], W, k, flag)
                rb, ob = run_two_calls(base, *sets[id(base)], W, k, flag, args.reads, args.cands)
                keep("a_topk_k%d_%s" % (k, f), ra); keep("b_two_calls_k%d_%s" % (k, f), rb)
                flagged["k%d_%s" % (k, f)] = nf
                equal["k%d_%s" % (k, f)] = same(oa, ob)
                if not equal["k%d_%s" % (k, f)]:
                    raise SystemExit("align_windows_topk and the two-call recipe disagree at k = %d, %s" % (k, f))
                assert (oa[0][:, 0] == planted).all()
                if k == 1:
                    rn, on = run_best(new, *sets[id(new)], W, flag)
                    keep("best_this_build_%s" % f, rn)
                    assert (on[0]["best"] == oa[0][:, 0]).all() and (on[1] == oa[2][:, 0]).all() and on[2].tobytes() == oa[3].tobytes()
                    if base is not new:
                        rp, _ = run_best(base, *sets[id(base)], W, flag)
                        keep("best_baseline_%s" % f, rp)
            if flag:
                keep("c_all_flagged_%s" % f, run_all_flagged(base, *sets[id(base)], W, flag))
        sys.stderr.write("[gpu_windows_topk_bench] repeat %d done\n" % rep); sys.stderr.flush()
    out = {"script": "gpu_windows_topk_bench", "reads": args.reads, "candidates_per_read": args.cands, "ks": ks, "reps": args.reps,
           "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)", "outputs_equal": equal, "best_flagged": flagged,
           "variants": {name: stats(v) for name, v in rows.items()}}
    cmpd = {}
    V = out["variants"]
    for flag in (0, 2):
        f = "flag%d" % flag
        for k in ks:
            a = V["a_topk_k%d_%s" % (k, f)]; b = V["b_two_calls_k%d_%s" % (k, f)]
            for col in ("wall_ms", "wall_without_numpy_ms"):
                margin = 2 * (b[col]["max"] - b[col]["min"])
                cmpd["k%d_%s_vs_b_%s" % (k, f, col)] = {"a_median": a["wall_ms"]["median"], "b_median": b[col]["median"], "difference": b[col]["median"] - a["wall_ms"]["median"],
                                                        "margin_2x_b_spread": margin, "a_faster_beyond_margin": bool(b[col]["median"] - a["wall_ms"]["median"] > margin)}
            cmpd["k%d_%s_reduce_over_fill" % (k, f)] = a["reduce_ms"]["median"] / a["fill_ms"]["median"]
        if "best_baseline_" + f in V:
            n = V["best_this_build_" + f]["wall_ms"]; p = V["best_baseline_" + f]["wall_ms"]
            margin = 2 * (p["max"] - p["min"])
            cmpd["best_%s_this_build_vs_baseline" % f] = {"this_build_median": n["median"], "baseline_median": p["median"], "margin_2x_baseline_spread": margin,
                                                          "within_margin": bool(n["median"] - p["median"] <= margin)}
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
