#!/usr/bin/env python3
"""GPU box: ssw_gpu_pool_align_windows_mates (the best candidate pair per read pair over a pool of workers) next to the single-context call
it is made of, on gpu_windows_mates_bench.py's list, the variants ALTERNATING inside every repeat.

Workload: `--frags` fragments of 2 x 150 bp (FR, inserts of 300..600 columns) of one resident 100 Mb target, `--cands` candidates per mate,
min_insert 100, max_insert 1000, unpaired_penalty 17; flag 0 and flag 2 with CIGARs.

Variants:
  ctx_resident   Context.align_windows_mates, reads and their reverse complements already on the device
  ctx_upload     the same with the upload of the reads and ssw_gpu_seqs_with_revcomp inside the timed region -- what a pool call does
  pool_1         Pool([0])       one worker: the blocks of the list one after the other
  pool_2_same    Pool([0, 0])    two workers on ONE device: one block's host planning and upload beside another block's kernels
  pool_all       Pool(None)      one worker per visible device
The pool calls use block = 0 (a few blocks per worker).  Every pool output must equal the single context's (selections, records, CIGAR
words) or the script fails.  Every figure is the median of `--reps` timed repeats after one warm-up, with min and max.  The pool figures are
reported beside the single context's with their spread; nothing is gated on a ratio.

With `--baseline-lib` (a build of the parent commit) a CHILD process first times ssw_gpu_align_windows_mates -- the symbol without an
orientation -- with the reads resident on that library, and leaves its selections and records in a file.  ctx_resident must give the same
output, and `unchanged` says per flag whether its wall time and reduce_ms (the device time of k_matebest) lie within twice the
baseline's max - min of the baseline's median.

usage: gpu_pool_mates_bench.py [--frags 1000000] [--cands 4] [--reps 5] [--baseline-lib PATH] [--out out.json]"""
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
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssw_amd          # noqa: E402
from gpu_windows_bench import GENOME, stats, upload   # noqa: E402
from gpu_windows_best_bench import MAT   # noqa: E402
from gpu_windows_mates_bench import MAX_INS, MIN_INS, PENALTY, workload   # noqa: E402


def same(a, b):
    return bool(a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes())


def old_symbol(ctx, Q, T, W, nfwd, flag):
    """ssw_gpu_align_windows_mates as the parent commit exports it, straight through the C ABI"""
    nf = (len(W["cand_off"]) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE); res = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE)
    pool = ssw_amd._u32p(); words = C.c_int64(0)
    rc = ctx.lib.ssw_gpu_align_windows_mates(ctx.h, Q.h, T.h, W["cand_off"].ctypes.data, nf, W["qidx"].ctypes.data, W["tidx"].ctypes.data,
                                             W["tbeg"].ctypes.data, W["tlen"].ctypes.data, nfwd, C.byref(p), 0, MIN_INS, MAX_INS, PENALTY,
                                             sel.ctypes.data, res.ctypes.data, C.byref(pool) if flag else None, C.byref(words))
    if rc != 0:
        raise SystemExit("ssw_gpu_align_windows_mates: " + ctx.error())
    cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if flag and words.value > 0 else np.zeros(0, dtype=np.uint32)
    if flag and pool:
        C.CDLL(None).free(pool)
    return sel, res, cig


def run_ctx(ctx, Q, T, W, nfwd, flag, reads=None, old=False):
    t0 = time.perf_counter()
    if reads is not None:
        base = upload(ctx, *reads); base.lengths = np.diff(reads[1])
        Q = base.with_revcomp(); base.free()
    if old:
        out = old_symbol(ctx, Q, T, W, nfwd, flag)
    else:
        out = ctx.align_windows_mates(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                      flag=flag, want_cigar=flag != 0)
    if reads is not None:
        Q.free()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    return dict(wall_ms=wall, device_total_ms=t["total_ms"], reduce_ms=t["reduce_ms"]), out


def run_pool(pool, reads, W, flag):
    t0 = time.perf_counter()
    out = pool.align_windows_mates(None, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                   with_revcomp=True, flag=flag, want_cigar=flag != 0, packed=reads)
    wall = (time.perf_counter() - t0) * 1e3
    st = pool.stats()
    return dict(wall_ms=wall, busy_ms_sum=sum(s["busy_ms"] for s in st), busy_ms_max=max(s["busy_ms"] for s in st),
                blocks=sum(s["blocks"] for s in st)), out


def baseline_child(args):
    """the parent commit's library: the old symbol with the reads resident -> stats and outputs in args.baseline_child (.npz)"""
    genome, rcodes, roff, W, nfwd, _ = workload(args.frags, args.cands)
    ctx = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib))
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    rows, outs = {}, {}
    for rep in range(args.reps + 1):
        for flag in (0, 2):
            r, outs[flag] = run_ctx(ctx, Q, T, W, nfwd, flag, old=True)
            if rep > 0:
                rows.setdefault("flag%d" % flag, []).append(r)
        sys.stderr.write("[gpu_pool_mates_bench] baseline: repeat %d done\n" % rep); sys.stderr.flush()
    Q.free(); T.free(); ctx.close()
    np.savez(args.baseline_child, stats=json.dumps({k: stats(v) for k, v in rows.items()}),
             **{"%s%d" % (n, f): outs[f][i] for f in (0, 2) for i, n in enumerate(("sel", "res", "cig"))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-child", default=None, help=argparse.SUPPRESS)      # internal: time the baseline library, leave outputs in this .npz
    args = ap.parse_args()
    if args.baseline_child:
        baseline_child(args)
        return
    B, bouts = None, None
    if args.baseline_lib:      # the yardstick first, in a process of its own (this one has not touched the device yet)
        with tempfile.TemporaryDirectory() as tmp:
            npz = os.path.join(tmp, "baseline.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--frags", str(args.frags), "--cands", str(args.cands), "--reps", str(args.reps),
                            "--baseline-lib", args.baseline_lib, "--baseline-child", npz], check=True)
            with np.load(npz) as z:
                B = json.loads(str(z["stats"])); bouts = {f: (z["sel%d" % f], z["res%d" % f], z["cig%d" % f]) for f in (0, 2)}
    genome, rcodes, roff, W, nfwd, planted = workload(args.frags, args.cands)
    reads = (rcodes, roff)
    lib = ssw_amd.load(None)
    ndev = int(lib.ssw_gpu_device_count())
    ctx = ssw_amd.Context(0, lib)
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    pools = {"pool_1": ssw_amd.Pool([0], lib), "pool_2_same": ssw_amd.Pool([0, 0], lib), "pool_all": ssw_amd.Pool(None, lib)}
    for p in pools.values():
        p.set_targets([genome])
    rows, equal = {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        def keep(name, row):
            if rep > 0:
                rows.setdefault(name, []).append(row)
        for flag in (0, 2):
            f = "flag%d" % flag
            r, want = run_ctx(ctx, Q, T, W, nfwd, flag)
            keep("ctx_resident_" + f, r)
            good = (want[0]["pos1"] == planted[0::2]) & (want[0]["pos2"] == planted[1::2]) & (want[0]["proper"] == 1)
            assert good.mean() > 0.999, good.mean()
            if bouts is not None:
                equal["baseline_" + f] = same(want, bouts[flag])
                if not equal["baseline_" + f]:
                    raise SystemExit("this library and the baseline library disagree at %s" % f)
            r, got = run_ctx(ctx, None, T, W, nfwd, flag, reads=reads)
            keep("ctx_upload_" + f, r)
            assert same(got, want)
            for name, p in pools.items():
                r, got = run_pool(p, reads, W, flag)
                keep(name + "_" + f, r)
                equal[name + "_" + f] = same(got, want)
                if not equal[name + "_" + f]:
                    raise SystemExit("%s and the single context disagree at %s" % (name, f))
        sys.stderr.write("[gpu_pool_mates_bench] repeat %d done\n" % rep); sys.stderr.flush()
    V = {name: stats(v) for name, v in rows.items()}
    cmpd = {}
    for flag in (0, 2):
        f = "flag%d" % flag
        up = V["ctx_upload_" + f]["wall_ms"]
        for name in pools:
            w = V[name + "_" + f]["wall_ms"]
            cmpd[name + "_" + f] = {"median": w["median"], "ctx_upload_median": up["median"], "ctx_resident_median": V["ctx_resident_" + f]["wall_ms"]["median"],
                                    "ratio_to_ctx_upload": w["median"] / up["median"], "spread": w["max"] - w["min"]}
    out = {"script": "gpu_pool_mates_bench", "fragments": args.frags, "candidates_per_mate": args.cands, "reps": args.reps,
           "min_insert": MIN_INS, "max_insert": MAX_INS, "unpaired_penalty": PENALTY, "visible_devices": ndev,
           "workers": {name: p.size() for name, p in pools.items()}, "outputs_equal": equal, "variants": V, "comparison": cmpd}
    if B is not None:
        out["baseline_lib"] = args.baseline_lib
        out["baseline"] = B
        unchanged = {}
        for f in ("flag0", "flag2"):
            for col in ("wall_ms", "reduce_ms"):
                b, a = B[f][col], V["ctx_resident_" + f][col]
                margin = 2 * (b["max"] - b["min"])
                unchanged["%s_%s" % (f, col)] = {"baseline_median": b["median"], "median": a["median"], "difference": a["median"] - b["median"],
                                                 "margin_2x_baseline_spread": margin, "within_margin": bool(a["median"] - b["median"] <= margin)}
        out["unchanged"] = unchanged
    for p in pools.values():
        p.close()
    Q.free(); T.free(); ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
