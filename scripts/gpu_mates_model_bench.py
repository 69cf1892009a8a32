#!/usr/bin/env python3
"""GPU box: the pair model's insert-size penalty table (ssw_gpu_align_windows_mates_model) next to the flat rule, and the flat rule next to
the parent commit's.

Workload: scripts/gpu_windows_mates_bench.py's list -- `--frags` fragments x 2 mates x `--cands` candidates, FR, one resident 100 Mb target,
min_insert 100, max_insert 1000, unpaired_penalty 17 -- and the table ssw_amd.insert_penalty_normal(450, 75, 100, 1000, 2, 17): the
fragments' inserts are uniform in 300 .. 600, the table is 0 at 450 and reaches 17 about 2.7 sd away.  Flag 0 and flag 2 with CIGARs.

Rows:
  parent_flat   Context.align_windows_mates on `--baseline-lib` (a build of the parent commit), in a CHILD process, which runs first
  this_flat     Context.align_windows_mates of this library (the old symbol: insert_penalty=None)
  this_model    Context.align_windows_mates(insert_penalty=table) of this library
this_flat's outputs must equal parent_flat's (selections, records, CIGAR words) or the script fails.  Every figure is the median of `--reps`
timed repeats after one warm-up, with min and max.  A row is "within margin" of the parent when its median differs from the parent's by at
most twice the parent's max - min over its repeats -- for the wall time and for reduce_ms (the device time of k_matebest).  Reported, not
gated: the fragments whose chosen pair differs between this_flat and this_model.  With `--bench-alt N`, bench.py --gpus 1 --steps 20
--warmup 5 N times with either library, alternating, each run a process of its own (the library through SSW_LIB).

usage: gpu_mates_model_bench.py [--frags 1000000] [--cands 4] [--reps 5] [--bench-alt N] [--baseline-lib PATH] [--out out.json]"""
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
from gpu_windows_mates_bench import MAX_INS, MIN_INS, PENALTY, workload   # noqa: E402

MEAN, SD, MATCH, CAP = 450, 75, 2, 17


def run(ctx, Q, T, W, nfwd, flag, table):
    kw = {} if table is None else {"insert_penalty": table}      # (the parent's binding has no such keyword)
    t0 = time.perf_counter()
    sel, res, cig = ctx.align_windows_mates(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                            flag=flag, want_cigar=flag != 0, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    row = dict(wall_ms=wall, **{f: t[f] for f in PHASES})
    row["host_remainder_ms"] = wall - t["fill_ms"] - t["reduce_ms"] - t["locate_ms"] - t["trace_ms"]
    return row, (sel, res, cig)


def measure(args, parent):
    genome, rcodes, roff, W, nfwd, planted = workload(args.frags, args.cands)
    ctx = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib if parent else None))
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    table = None if parent else ssw_amd.insert_penalty_normal(MEAN, SD, MIN_INS, MAX_INS, MATCH, CAP)
    rows, outs = {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        for flag in (0, 2):
            for name, tab in ((("parent_flat", None),) if parent else (("this_flat", None), ("this_model", table))):
                row, o = run(ctx, Q, T, W, nfwd, flag, tab)
                if rep > 0:
                    rows.setdefault(name, {}).setdefault("flag%d" % flag, []).append(row)
                outs[(name, flag)] = o
        sys.stderr.write("[gpu_mates_model_bench] %s: repeat %d done\n" % ("parent" if parent else "this build", rep)); sys.stderr.flush()
    Q.free(); T.free(); ctx.close()
    return {n: {k: stats(v) for k, v in d.items()} for n, d in rows.items()}, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-alt", type=int, default=0, help="runs of bench.py with either library, alternating (0: none)")
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)      # internal: run parent_flat, leave outputs in this .npz
    args = ap.parse_args()
    if args.parent_child:
        V, outs = measure(args, True)
        np.savez(args.parent_child, stats=json.dumps(V), **{"%s%d" % (n, f): outs[("parent_flat", f)][i] for f in (0, 2) for i, n in enumerate(("sel", "res", "cig"))})
        return
    with tempfile.TemporaryDirectory() as tmp:      # the parent first, in a process of its own (this one has not touched the device yet)
        npz = os.path.join(tmp, "parent.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--frags", str(args.frags), "--cands", str(args.cands), "--reps", str(args.reps), "--parent-child", npz]
        if args.baseline_lib:
            cmd += ["--baseline-lib", args.baseline_lib]
        subprocess.run(cmd, check=True)
        with np.load(npz) as z:
            P = json.loads(str(z["stats"])); pouts = {f: (z["sel%d" % f], z["res%d" % f], z["cig%d" % f]) for f in (0, 2)}
    N, outs = measure(args, False)
    equal = {"flag%d" % f: bool(outs[("this_flat", f)][0].tobytes() == pouts[f][0].tobytes() and (outs[("this_flat", f)][1] == pouts[f][1]).all() and
                                outs[("this_flat", f)][2].tobytes() == pouts[f][2].tobytes()) for f in (0, 2)}
    if not all(equal.values()):
        raise SystemExit("the flat call of this build and of the parent disagree: %s" % equal)
    table = ssw_amd.insert_penalty_normal(MEAN, SD, MIN_INS, MAX_INS, MATCH, CAP)
    fs, ms = outs[("this_flat", 0)][0], outs[("this_model", 0)][0]
    assert ms.tobytes() == outs[("this_model", 2)][0].tobytes()      # sel does not depend on the flag
    out = {"script": "gpu_mates_model_bench", "fragments": args.frags, "candidates_per_mate": args.cands, "reps": args.reps,
           "min_insert": MIN_INS, "max_insert": MAX_INS, "unpaired_penalty": PENALTY,
           "insert_penalty": {"helper": "insert_penalty_normal", "mean": MEAN, "sd": SD, "match": MATCH, "cap": CAP, "entries": int(len(table)),
                              "zero_entries": int((table == 0).sum()), "capped_entries": int((table == CAP).sum())},
           "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)", "flat_outputs_equal_parent": equal,
           "this_build": N, "parent": P["parent_flat"],
           "fragments_whose_chosen_pair_differs": int(((fs["pos1"] != ms["pos1"]) | (fs["pos2"] != ms["pos2"])).sum()),
           "fragments_whose_score_differs": int((fs["score"] != ms["score"]).sum()),
           "fragments_proper_flat_vs_model": [int(fs["proper"].sum()), int(ms["proper"].sum())]}
    cmpd = {}
    for f in ("flag0", "flag2"):
        b = P["parent_flat"][f]
        for name in ("this_flat", "this_model"):
            a = N[name][f]
            for col in ("wall_ms", "reduce_ms", "fill_ms"):
                margin = 2 * (b[col]["max"] - b[col]["min"])
                d = a[col]["median"] - b[col]["median"]
                cmpd["%s_%s_%s_vs_parent" % (name, f, col)] = {"this_median": a[col]["median"], "parent_median": b[col]["median"], "this_minus_parent": d,
                                                               "margin_2x_parent_spread": margin, "within_margin": bool(abs(d) <= margin)}
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
                sys.stderr.write("[gpu_mates_model_bench] bench.py, %s: %.1f GCUPS\n" % (who, runs[who][-1])); sys.stderr.flush()
        st = {w: stats([{"gcups": v} for v in runs[w]])["gcups"] for w in runs}
        margin = 2 * (st["parent"]["max"] - st["parent"]["min"])
        cmpd["bench_py_gcups"] = {"this": st["this"], "parent": st["parent"], "runs": runs, "margin_2x_parent_spread": margin,
                                  "within_margin": bool(abs(st["this"]["median"] - st["parent"]["median"]) <= margin)}
    print(emit())


if __name__ == "__main__":
    main()
