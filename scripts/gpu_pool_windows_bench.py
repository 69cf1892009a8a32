#!/usr/bin/env python3
"""GPU box: ssw_gpu_pool_align_windows_topk (the window lists over a pool of workers) next to the single-context call it is made of, on
gpu_windows_topk_bench.py's list, in one process, the variants ALTERNATING inside every repeat.

Workload: 150-bp reads, `--cands` candidates per read -- the true window at a random position of the group plus decoys elsewhere,
windows of 300..700 bp of one resident 100 Mb target --, k = 2, flag 0 and flag 2 with CIGARs.

Variants:
  ctx_resident   Context.align_windows_topk, reads already on the device (what gpu_windows_topk_bench.py times)
  ctx_upload     the same with the upload of the reads inside the timed region -- what a pool call does, since its reads come from the host
  pool_1         Pool([0])       one worker: the blocks of the list one after the other
  pool_2_same    Pool([0, 0])    two workers on ONE device: one block's host planning and upload beside another block's kernels
  pool_all       Pool(None)      one worker per visible device
The pool calls use block = 0 (a few blocks per worker).  Every pool output must equal the single context's (positions, eligible counts,
records, CIGAR words) or the script fails.  Every figure is the median of `--reps` timed repeats after one warm-up, with min and max.
Nothing is gated on a ratio: the single-context call is the baseline, the pool figures are reported beside it with their spread.

usage: gpu_pool_windows_bench.py [--reads 1000000] [--cands 4] [--k 2] [--reps 5] [--out out.json]"""
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
from gpu_windows_best_bench import MAT, candidates   # noqa: E402


def same(a, b):
    return bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3].tobytes() == b[3].tobytes())


def run_ctx(ctx, Q, T, W, k, flag, reads=None):
    t0 = time.perf_counter()
    if reads is not None:
        Q = upload(ctx, *reads)
    out = ctx.align_windows_topk(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, k, flag=flag, want_cigar=flag != 0)
    if reads is not None:
        Q.free()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    return dict(wall_ms=wall, device_total_ms=t["total_ms"]), out


def run_pool(pool, reads, W, k, flag):
    t0 = time.perf_counter()
    out = pool.align_windows_topk(None, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, k, flag=flag, want_cigar=flag != 0,
                                  packed=reads)
    wall = (time.perf_counter() - t0) * 1e3
    st = pool.stats()
    return dict(wall_ms=wall, busy_ms_sum=sum(s["busy_ms"] for s in st), busy_ms_max=max(s["busy_ms"] for s in st),
                blocks=sum(s["blocks"] for s in st)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    genome, rcodes, roff, tbeg, tlen = workload(args.reads)
    co, qidx, cb, cl, planted = candidates(args.reads, args.cands, tbeg, tlen)
    W = dict(cand_off=co, qidx=qidx, tidx=np.zeros(len(qidx), dtype=np.int32), tbeg=cb, tlen=cl)
    reads = (rcodes, roff)
    lib = ssw_amd.load(None)
    ndev = int(lib.ssw_gpu_device_count())
    ctx = ssw_amd.Context(0, lib)
    Q = upload(ctx, rcodes, roff); T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
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
            r, want = run_ctx(ctx, Q, T, W, args.k, flag)
            keep("ctx_resident_" + f, r)
            assert (want[0][:, 0] == planted).all()
            r, got = run_ctx(ctx, None, T, W, args.k, flag, reads=reads)
            keep("ctx_upload_" + f, r)
            assert same(got, want)
            for name, p in pools.items():
                r, got = run_pool(p, reads, W, args.k, flag)
                keep(name + "_" + f, r)
                equal[name + "_" + f] = same(got, want)
                if not equal[name + "_" + f]:
                    raise SystemExit("%s and the single context disagree at %s" % (name, f))
        sys.stderr.write("[gpu_pool_windows_bench] repeat %d done\n" % rep); sys.stderr.flush()
    V = {name: stats(v) for name, v in rows.items()}
    cmpd = {}
    for flag in (0, 2):
        f = "flag%d" % flag
        base = V["ctx_upload_" + f]["wall_ms"]
        for name in pools:
            w = V[name + "_" + f]["wall_ms"]
            cmpd[name + "_" + f] = {"median": w["median"], "ctx_upload_median": base["median"], "ctx_resident_median": V["ctx_resident_" + f]["wall_ms"]["median"],
                                    "ratio_to_ctx_upload": w["median"] / base["median"], "spread": w["max"] - w["min"]}
    out = {"script": "gpu_pool_windows_bench", "reads": args.reads, "candidates_per_read": args.cands, "k": args.k, "reps": args.reps,
           "visible_devices": ndev, "workers": {name: p.size() for name, p in pools.items()}, "outputs_equal": equal, "variants": V,
           "comparison": cmpd}
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
