#!/usr/bin/env python3
"""GPU box: ssw_gpu_insert_hist (the insert-size histogram of a library, reduced on the device) next to the host recipe a caller uses
without it, and the mates call next to the parent commit's.

Workload: scripts/gpu_windows_mates_bench.py's list -- `--frags` fragments x 2 mates x `--cands` candidates, FR, inserts uniform in
300 .. 600, one resident 100 Mb target.  max_span 1000, min_margin 1.

Rows:
  a  insert_hist    Context.insert_hist of this library
  b  recipe         align_windows_best at flag 0 + the rule of include/ssw_gpu.h in numpy (reported on its own)
                                                     -- `--baseline-lib` (a build of the parent commit), in a CHILD process, which runs first
  c  mates          Context.align_windows_mates at flag 0, of this library and (in the child) of the parent's
a's histogram and counters must equal b's or the script fails.  Every figure is the median of `--reps` timed repeats after one warm-up,
with min and max.  a is faster when b's median exceeds a's by more than twice b's max - min, with and without b's numpy part; c is
unchanged when the medians differ by at most twice the parent's max - min.  reduce_ms of a is k_insertstat's device time, of c
k_matebest's.  Also reported: ssw_gpu_insert_fit of a's FR row against the generator's parameters, and the share of fragments
align_windows_mates finds proper under insert_model_normal of that fit.  With `--bench-alt N`, bench.py --gpus 1 --steps 20 --warmup 5 N
times with either library, alternating, each run a process of its own (the library through SSW_LIB).

usage: gpu_insert_hist_bench.py [--frags 1000000] [--cands 4] [--reps 5] [--bench-alt N] [--baseline-lib PATH] [--out out.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssw_amd          # noqa: E402
from gpu_windows_bench import GENOME, stats, upload   # noqa: E402
from gpu_windows_best_bench import MAT, PHASES   # noqa: E402
from gpu_windows_mates_bench import MAX_INS, MIN_INS, PENALTY, RL, workload   # noqa: E402

MAX_SPAN, MIN_MARGIN, MATCH, CAP = 1000, 1, 2, 17
COUNTS = ("n_both", "n_unique", "n_same", "n_in", "n_out")


def rule_numpy(sel, res, W, nf, nfwd):
    """the rule of include/ssw_gpu.h over align_windows_best's selections and winners' records -> (hist [3, MAX_SPAN + 1], counts)"""
    best = sel["best"].astype(np.int64).reshape(nf, 2)
    both = (best >= 0).all(axis=1)
    lead = res["score1"].astype(np.int64).reshape(nf, 2) - sel["second_score1"].astype(np.int64).reshape(nf, 2)
    unique = both & (lead >= MIN_MARGIN).all(axis=1)
    idx = W["cand_off"][:-1].reshape(nf, 2)[unique] + best[unique]
    same = W["tidx"][idx[:, 0]] == W["tidx"][idx[:, 1]]
    idx = idx[same]
    E = W["tbeg"][idx] + res["ref_end1"].astype(np.int64).reshape(nf, 2)[unique][same]
    B = E - RL + 1
    minus = W["qidx"][idx] >= nfwd
    opp = minus[:, 0] != minus[:, 1]
    a_minus = minus[:, 0]
    Ep = np.where(a_minus, E[:, 1], E[:, 0]); Bp = np.where(a_minus, B[:, 1], B[:, 0])      # the plus-strand one (strands differ)
    Em = np.where(a_minus, E[:, 0], E[:, 1]); Bm = np.where(a_minus, B[:, 0], B[:, 1])
    spans = ((Em - Bp + 1)[opp], (Ep - Bm + 1)[opp], np.where(a_minus, E[:, 0] - B[:, 1], E[:, 1] - B[:, 0])[~opp] + 1)
    hist = np.zeros((3, MAX_SPAN + 1), dtype=np.uint32)
    n_in, n_out = [], []
    for o, d in enumerate(spans):
        ok = (d >= 0) & (d <= MAX_SPAN)
        hist[o] = np.bincount(d[ok], minlength=MAX_SPAN + 1)
        n_in.append(int(ok.sum())); n_out.append(int((~ok).sum()))
    return hist, dict(n_both=int(both.sum()), n_unique=int(unique.sum()), n_same=int(same.sum()), n_in=n_in, n_out=n_out)


def timed(ctx, fn):
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    return dict(wall_ms=wall, **{f: t[f] for f in PHASES}), out


def measure(args, parent):
    genome, rcodes, roff, W, nfwd, planted = workload(args.frags, args.cands)
    nf = args.frags
    ctx = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib if parent else None))
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    cand = (W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"])
    rows, outs = {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        if parent:
            row, (sel, res, _) = timed(ctx, lambda: ctx.align_windows_best(Q, T, *cand, MAT, 5, flag=0))
            t1 = time.perf_counter()
            outs["hist"], outs["counts"] = rule_numpy(sel, res, W, nf, nfwd)
            row["numpy_rule_ms"] = (time.perf_counter() - t1) * 1e3
            row["wall_without_numpy_ms"] = row["wall_ms"]; row["wall_ms"] += row["numpy_rule_ms"]
            new = {"b_recipe": row}
        else:
            row, (outs["hist"], outs["counts"]) = timed(ctx, lambda: ctx.insert_hist(Q, T, *cand, nfwd, MAT, 5, MAX_SPAN, min_margin=MIN_MARGIN))
            new = {"a_insert_hist": row}
        new["c_mates_flag0"], (outs["sel"], _, _) = timed(ctx, lambda: ctx.align_windows_mates(Q, T, *cand, nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY, flag=0,
                                                                                              want_cigar=False))
        if rep > 0:
            for k, v in new.items():
                rows.setdefault(k, []).append(v)
        sys.stderr.write("[gpu_insert_hist_bench] %s: repeat %d done\n" % ("parent" if parent else "this build", rep)); sys.stderr.flush()
    fitted = None
    if not parent:
        st = ssw_amd.insert_fit(outs["hist"][0], ctx.lib)
        model = ssw_amd.insert_model_normal(st, MATCH, CAP)
        sel, _, _ = ctx.align_windows_mates(Q, T, *cand, nfwd, MAT, 5, unpaired_penalty=PENALTY, flag=0, want_cigar=False, **model)
        fitted = {"fr_row": {k: st[k] for k in ("n_total", "n_used", "p25", "p50", "p75", "mean", "sd", "min_insert", "max_insert")},
                  "generator": {"inserts": "uniform 300 .. 600", "mean": 450.0, "sd": float(np.sqrt((301 ** 2 - 1) / 12.0))},
                  "proper_rate_under_insert_model_normal": float((sel["proper"] == 1).mean()),
                  "proper_rate_flat_100_1000": float((outs["sel"]["proper"] == 1).mean())}
    Q.free(); T.free(); ctx.close()
    return {k: stats(v) for k, v in rows.items()}, outs, fitted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-alt", type=int, default=0, help="runs of bench.py with either library, alternating (0: none)")
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)      # internal: run the parent's rows, leave outputs in this .npz
    args = ap.parse_args()
    if args.parent_child:
        V, outs, _ = measure(args, True)
        np.savez(args.parent_child, stats=json.dumps(V), counts=json.dumps(outs["counts"]), hist=outs["hist"], sel=outs["sel"])
        return
    with tempfile.TemporaryDirectory() as tmp:      # the parent first, in a process of its own (this one has not touched the device yet)
        npz = os.path.join(tmp, "parent.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--frags", str(args.frags), "--cands", str(args.cands), "--reps", str(args.reps), "--parent-child", npz]
        if args.baseline_lib:
            cmd += ["--baseline-lib", args.baseline_lib]
        subprocess.run(cmd, check=True)
        with np.load(npz) as z:
            P = json.loads(str(z["stats"])); pcounts = json.loads(str(z["counts"])); phist = z["hist"]; psel = z["sel"]
    N, outs, fitted = measure(args, False)
    equal = {"hist": bool(outs["hist"].tobytes() == phist.tobytes()), "counts": bool({k: outs["counts"][k] for k in COUNTS} == pcounts),
             "mates_sel": bool(outs["sel"].tobytes() == psel.tobytes())}
    if not all(equal.values()):
        raise SystemExit("this build and the recipe on the parent disagree: %s (counts %s / %s)" % (equal, outs["counts"], pcounts))
    out = {"script": "gpu_insert_hist_bench", "fragments": args.frags, "candidates_per_mate": args.cands, "reps": args.reps,
           "max_span": MAX_SPAN, "min_margin": MIN_MARGIN, "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)",
           "outputs_equal": equal, "counts": outs["counts"], "this_build": N, "parent": P, "fit": fitted}
    a, b = N["a_insert_hist"], P["b_recipe"]
    cmpd = {}
    for col in ("wall_ms", "wall_without_numpy_ms"):
        margin = 2 * (b[col]["max"] - b[col]["min"])
        cmpd["a_vs_b_%s" % col] = {"a_median": a["wall_ms"]["median"], "b_median": b[col]["median"], "difference": b[col]["median"] - a["wall_ms"]["median"],
                                   "margin_2x_b_spread": margin, "a_faster_beyond_margin": bool(b[col]["median"] - a["wall_ms"]["median"] > margin)}
    for col in ("wall_ms", "reduce_ms", "fill_ms"):
        t, p = N["c_mates_flag0"][col], P["c_mates_flag0"][col]
        margin = 2 * (p["max"] - p["min"])
        cmpd["c_mates_%s_vs_parent" % col] = {"this_median": t["median"], "parent_median": p["median"], "this_minus_parent": t["median"] - p["median"],
                                              "margin_2x_parent_spread": margin, "within_margin": bool(abs(t["median"] - p["median"]) <= margin)}
    cmpd["d_reduce_ms"] = {"k_insertstat": a["reduce_ms"], "k_matebest": N["c_mates_flag0"]["reduce_ms"]}

    def emit():
        line = json.dumps(out)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return line

    out["comparison"] = cmpd
    emit()      # (the list's figures are on disk before the benchmark's runs start)
    if args.bench_alt > 0:      # the flagship benchmark, unchanged code paths: the parent's library and this one by turns
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_alt):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("SSW_LIB", None)
                if who == "parent" and args.baseline_lib:
                    env["SSW_LIB"] = args.baseline_lib
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], check=True, env=env,
                                   capture_output=True, text=True)
                runs[who].append(float(json.loads(r.stdout.strip().splitlines()[-1])["value"]))
                sys.stderr.write("[gpu_insert_hist_bench] bench.py, %s: %.1f GCUPS\n" % (who, runs[who][-1])); sys.stderr.flush()
        st = {w: stats([{"gcups": v} for v in runs[w]])["gcups"] for w in runs}
        margin = 2 * (st["parent"]["max"] - st["parent"]["min"])
        cmpd["e_bench_py_gcups"] = {"this": st["this"], "parent": st["parent"], "runs": runs, "margin_2x_parent_spread": margin,
                                    "within_margin": bool(abs(st["this"]["median"] - st["parent"]["median"]) <= margin)}
    print(emit())


if __name__ == "__main__":
    main()
