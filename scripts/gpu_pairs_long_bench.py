#!/usr/bin/env python3
"""GPU box: long reads on the fused pair / window path (k_chainq<R,pairs,form>) next to the parent build, which answers every
such pair through the fallback (one internal batch call per distinct window), on the same list in the same session.

Workload: a resident 100 Mb random target; BASELINE config 4's read model (10 000 reads of 10 kb, tests/workloads.py: 1 % substitutions,
0.25 % insertions and deletions, 5 % unrelated reads); every read against its OWN window of read length + 20 % (12 000 columns, 1 000
columns ahead of the read's source); flag 0 and flag 2 with CIGARs, maskLen 5000.

Protocol: one warm-up, then the median of `reps` timed repeats with [min, max].  Measurements of the new build ("new"):
  align_windows          wall clock of the call + its phase times (fill_ms: the strip kernel's launches; total_ms also holds the reduction,
                         uploads and downloads)
  batch_one_target       ssw_gpu_align_batch of the same reads against ONE 12-kb target, flag 0: the batch path's k_chainq fill over the same
                         number of cells -- the fill rate of both (fill_cells / fill_ms) is reported, not gated
  parity                 records (and CIGARs) of a `--parity`-pair sample against the reference's (parity.expected): 0 mismatches required
The baseline runs in a child process on `--baseline-lib` (a build of the parent commit) over a `--sample`-pair subsample of the same list
(the head of the list) and is SCALED to the list -- on the parent this is the per-pair fallback, the full list would take minutes.
Acceptance: new median < scaled baseline median - 2 x scaled baseline (max - min), per flag.

usage: gpu_pairs_long_bench.py [--npairs 10000] [--reps 5] [--sample 500] [--parity 200] [--baseline-lib PATH] [--out out.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
import ssw_amd          # noqa: E402
from gpu_windows_bench import stats, upload   # noqa: E402
from parity import expected   # noqa: E402
from sswutil import RES_FIELDS, dna_matrix   # noqa: E402
from workloads import DNA_CONFIGS, make_reads_fast   # noqa: E402

GENOME = 100000000
PHASES = ("total_ms", "fill_ms", "reduce_ms", "locate_ms", "trace_ms")
CFG = DNA_CONFIGS[4]
MASK = CFG["mask_len"]


def workload(npairs, seed=4000):
    """-> genome, reads [npairs, 10 000], tbeg, tlen"""
    genome = np.random.default_rng(7).integers(0, 4, size=GENOME, dtype=np.int8)
    L = CFG["read_len"]
    reads = make_reads_fast(genome, npairs, L, seed=seed, sub=CFG["sub"], ins=CFG["indel"], dele=CFG["indel"])
    off = np.random.default_rng(seed).integers(0, GENOME - (L + 32), size=npairs)      # make_reads_fast's first draw: where every read comes from
    tlen = np.full(npairs, L + L // 5, dtype=np.int32)
    tbeg = np.clip(off - L // 10, 0, GENOME - int(tlen[0])).astype(np.int64)
    return genome, reads, tbeg, tlen


def run(ctx, Q, T, qidx, tidx, tbeg, tlen, flag, reps):
    mat = dna_matrix(2, 2)
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res, cig = ctx.align_windows(Q, T, qidx, tidx, tbeg, tlen, mat, 5, 3, 1, flag, maskLen=MASK, want_cigar=flag != 0)
        dt = time.perf_counter() - t0
        t = ctx.timing()
        if r > 0:
            rows.append(dict(wall_ms=dt * 1e3, **{k: t[k] for k in PHASES}))
        sys.stderr.write("[gpu_pairs_long_bench] flag %d run %d of %d: %.1f ms (%s)\n" % (flag, r, reps, dt * 1e3, t["fill_kernel"])); sys.stderr.flush()
    s = stats(rows)
    return dict(s, fill_kernel=t["fill_kernel"], fill_launches=t["fill_launches"], fill_cells=t["fill_cells"], cells=t["cells"], win_copied=t["win_copied"],
                n_word=t["n_word"], n_byte=t["n_byte"], fill_tcups=t["fill_cells"] / (s["fill_ms"]["median"] * 1e-3) / 1e12 if s["fill_ms"]["median"] > 0 else None,
                gcups_wall=t["cells"] / (s["wall_ms"]["median"] * 1e-3) / 1e9), res, cig


def child(args):
    lib = ssw_amd.load(args.lib)
    ctx = ssw_amd.Context(0, lib)
    ctx.set_exclusive()
    genome, reads, tbeg, tlen = workload(args.npairs)
    n = args.sub if args.sub else args.npairs
    L = reads.shape[1]
    out = {"lib": os.path.relpath(args.lib or ssw_amd.DEFAULT_LIB, ROOT), "pairs": n, "read_len": L, "window": int(tlen[0])}
    Q = upload(ctx, np.ascontiguousarray(reads[:n].reshape(-1)), np.arange(n + 1, dtype=np.int64) * L)
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    qidx = np.arange(n, dtype=np.int32); tidx = np.zeros(n, dtype=np.int32)
    mat = dna_matrix(2, 2)
    for flag in (0, 2):
        m, res, cig = run(ctx, Q, T, qidx, tidx, tbeg[:n], tlen[:n], flag, args.reps)
        bad = 0
        for i in range(min(args.parity, n)):
            exp, ecig = expected(reads[i], mat, 5, np.ascontiguousarray(genome[int(tbeg[i]):int(tbeg[i]) + int(tlen[i])]), 3, 1, flag, 0, 0, MASK, 2)
            g = res[i]
            o, ln = int(g["cigar_off"]), int(g["cigarLen"])
            ok = exp is not None and int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp and [int(x) for x in cig[o:o + ln]] == (ecig if ln > 0 else [])
            bad += 0 if ok else 1
        m["parity"] = {"pairs": min(args.parity, n), "mismatches": bad}
        out["flag%d" % flag] = {"align_windows": m}
    if not args.sub:      # the batch path's fill over the same number of cells: the same reads against ONE window as a target of its own
        T1 = ctx.upload([np.ascontiguousarray(genome[int(tbeg[0]):int(tbeg[0]) + int(tlen[0])])])
        rows = []
        for r in range(args.reps + 1):
            ctx.align_batch(Q, T1, mat, 5, 3, 1, 0, 0, 0, MASK, 2, want_cigar=False)
            t = ctx.timing()
            if r > 0:
                rows.append({k: t[k] for k in PHASES})
        s = stats(rows)
        out["batch_one_target"] = dict(s, fill_kernel=t["fill_kernel"], fill_cells=t["fill_cells"],
                                       fill_tcups=t["fill_cells"] / (s["fill_ms"]["median"] * 1e-3) / 1e12)
        T1.free()
    Q.free(); T.free(); ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npairs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=500)
    ap.add_argument("--parity", type=int, default=200)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sub", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"script": "gpu_pairs_long_bench", "npairs": args.npairs, "reps": args.reps, "sample": args.sample}
    for name, lib in (("new", None), ("baseline", args.baseline_lib)):      # fresh child processes, one after the other
        if name == "baseline" and lib is None:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--npairs", str(args.npairs), "--reps", str(args.reps)]
        cmd += ["--lib", lib, "--sub", str(args.sample), "--parity", "0"] if lib else ["--parity", str(args.parity)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=1100)      # (the child's progress lines go straight to stderr)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:])
            raise SystemExit("%s run failed (exit %d): nothing further is started" % (name, r.returncode))
        sys.stderr.write("[gpu_pairs_long_bench] %s run done\n" % name); sys.stderr.flush()
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    cmpd = {}
    for flag in ("flag0", "flag2"):
        w = out["new"][flag]["align_windows"]
        c = {"new_wall_ms": w["wall_ms"], "parity_mismatches": w["parity"]["mismatches"]}
        if "baseline" in out:
            b = out["baseline"][flag]["align_windows"]
            k = args.npairs / float(out["baseline"]["pairs"])
            c["baseline_scaled_wall_ms"] = {"median": b["wall_ms"]["median"] * k, "min": b["wall_ms"]["min"] * k, "max": b["wall_ms"]["max"] * k, "scaled": True,
                                            "scale": k, "fill_kernel": b["fill_kernel"], "win_copied_sample": b["win_copied"]}
            margin = 2 * (b["wall_ms"]["max"] - b["wall_ms"]["min"]) * k
            c["margin_2x_baseline_spread_ms"] = margin
            c["ratio"] = b["wall_ms"]["median"] * k / w["wall_ms"]["median"]
            c["accepted"] = bool(w["wall_ms"]["median"] < b["wall_ms"]["median"] * k - margin and w["parity"]["mismatches"] == 0)
        cmpd[flag] = c
    if "batch_one_target" in out["new"]:
        cmpd["fill_tcups"] = {"pairs_mode": out["new"]["flag0"]["align_windows"]["fill_tcups"],      # cells the kernels evaluated (padding rows included) per second of fill_ms
                              "batch_one_target": out["new"]["batch_one_target"]["fill_tcups"]}
    out["comparison"] = cmpd
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
