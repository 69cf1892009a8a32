#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_windows_mates (the best candidate pair of every read pair, selected on the device) next to the host recipe a
paired-end caller uses without it.

Workload: `--frags` fragments of 2 x 150 bp (FR, inserts of 300..600 columns) of one resident 100 Mb target, `--cands` candidates per mate
-- the true window on the right strand at a random position of the group plus decoys elsewhere on a random strand, windows of 300..700 bp.
The reads are uploaded with their reverse complements.  min_insert 100, max_insert 1000, unpaired_penalty 17; flag 0 and flag 2 with CIGARs.

Variants:
  a  mates     Context.align_windows_mates                                                                    -- this library, this process
  b  recipe    align_windows at flag 0 over all candidates + the pairing in numpy (reported on its own) + align_windows with the flag
               over the winners                              -- `--baseline-lib` (a build of the parent commit), in a CHILD process
The child runs first and leaves its selections and records in a file; a's outputs must equal them (selections, records, CIGAR words) or the
script fails.  Every figure is the median of `--reps` timed repeats after one warm-up, with min and max.  a is faster when the difference
exceeds twice b's max - min, with and without b's numpy part.  Nothing else is tuned.

usage: gpu_windows_mates_bench.py [--frags 1000000] [--cands 4] [--reps 5] [--baseline-lib PATH] [--out out.json]"""
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
from gpu_windows_best_bench import MAT, PHASES, phases   # noqa: E402

MIN_INS, MAX_INS, PENALTY, RL = 100, 1000, 17, 150


def workload(nf, ncand, seed=1):
    """-> genome, read codes (flat, 2 nf reads of 150), read offsets, and the candidate arrays (cand_off, qidx, tidx, tbeg, tlen), nfwd"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=GENOME, dtype=np.int8)
    ins = rng.integers(300, 601, size=nf)
    s = rng.integers(1000, GENOME - 2000, size=nf)
    flip = rng.random(nf) < 0.5                                   # mate 1 is the right end (reverse complement) of the fragment
    left, right = s, s + ins - RL
    R = np.empty((2 * nf, RL), dtype=np.int8)
    for a in range(0, nf, 100000):
        b = min(nf, a + 100000)
        L = genome[left[a:b, None] + np.arange(RL)[None, :]]
        Rt = 3 - genome[right[a:b, None] + np.arange(RL)[None, ::-1]]
        fl = flip[a:b, None]
        R[2 * a:2 * b:2] = np.where(fl, Rt, L); R[2 * a + 1:2 * b:2] = np.where(fl, L, Rt)
    sub = rng.random(R.shape) < 0.02
    R[sub] = (R[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
    nr = 2 * nf
    home = np.empty(nr, dtype=np.int64); home[0::2] = np.where(flip, right, left); home[1::2] = np.where(flip, left, right)
    rev = np.empty(nr, dtype=bool); rev[0::2] = flip; rev[1::2] = ~flip      # the read matches as its reverse complement
    n = nr * ncand
    cl = rng.integers(300, 701, size=n).astype(np.int32)
    cb = rng.integers(0, GENOME - 700, size=n).astype(np.int64)
    crev = rng.random(n) < 0.5
    planted = rng.integers(0, ncand, size=nr)
    at = np.arange(nr, dtype=np.int64) * ncand + planted
    cb[at] = np.clip(home - (rng.random(nr) * (cl[at] - RL)).astype(np.int64), 0, GENOME - 700)
    crev[at] = rev
    qidx = (np.repeat(np.arange(nr, dtype=np.int64), ncand) + np.where(crev, nr, 0)).astype(np.int32)
    off = np.arange(nr + 1, dtype=np.int64) * RL
    W = dict(cand_off=np.arange(nr + 1, dtype=np.int64) * ncand, qidx=qidx, tidx=np.zeros(n, dtype=np.int32), tbeg=cb, tlen=cl)
    return genome, np.ascontiguousarray(R.reshape(-1)), off, W, nr, planted


def pair_numpy(res, W, nf, nc, nfwd):
    """the rule of include/ssw_gpu.h over the flag-0 records of all candidates, every group holding nc candidates -> sel [nf] of MATES_DTYPE"""
    s = res["score1"].astype(np.int64).reshape(nf, 2, nc)
    ok = ((res["status"] == 0) & (res["score1"] > 0)).reshape(nf, 2, nc)
    E = (W["tbeg"] + res["ref_end1"]).reshape(nf, 2, nc)
    B = E - RL + 1
    minus = (W["qidx"] >= nfwd).reshape(nf, 2, nc)
    m1, m2 = minus[:, 0, :, None], minus[:, 1, None, :]
    ins = np.where(m1, E[:, 0, :, None] - B[:, 1, None, :], E[:, 1, None, :] - B[:, 0, :, None]) + 1
    proper = (m1 != m2) & (ins >= MIN_INS) & (ins <= MAX_INS)      # (one target)
    valid = ok[:, 0, :, None] & ok[:, 1, None, :]
    S = s[:, 0, :, None] + s[:, 1, None, :] - np.where(proper, 0, PENALTY)
    c = np.arange(nc * nc, dtype=np.int64)
    key = np.where(valid, ((S + 65536) << 32) | (0xffffffff - c.reshape(1, nc, nc)), 0).reshape(nf, nc * nc)
    order = np.argsort(-key, axis=1, kind="stable")[:, :2]
    k12 = np.take_along_axis(key, order, axis=1)
    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE)
    ne = ok.sum(axis=2)
    both = k12[:, 0] > 0
    sel["n_eligible1"] = ne[:, 0]; sel["n_eligible2"] = ne[:, 1]
    sel["pos1"] = np.where(both, order[:, 0] // nc, -1); sel["pos2"] = np.where(both, order[:, 0] % nc, -1)
    sel["score"] = np.where(both, (k12[:, 0] >> 32) - 65536, 0)
    sel["second_score"] = np.where(k12[:, 1] > 0, (k12[:, 1] >> 32) - 65536, 0)
    sel["n_proper"] = (proper & valid).sum(axis=(1, 2))
    sel["proper"] = np.where(both, np.take_along_axis((proper & valid).reshape(nf, nc * nc), order[:, :1], axis=1)[:, 0], 0)
    for f in np.nonzero(~both & (ne.sum(axis=1) > 0))[0]:          # one mate alone (rare): score1 descending, position ascending
        h = 0 if ne[f, 0] else 1
        o = sorted((i for i in range(nc) if ok[f, h, i]), key=lambda i: (-s[f, h, i], i))
        sel["pos1" if h == 0 else "pos2"][f] = o[0]
        sel["score"][f] = s[f, h, o[0]]; sel["second_score"][f] = s[f, h, o[1]] if len(o) > 1 else 0
    return sel


def run_mates(ctx, Q, T, W, nfwd, flag):
    t0 = time.perf_counter()
    sel, res, cig = ctx.align_windows_mates(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                            flag=flag, want_cigar=flag != 0)
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    row = dict(wall_ms=wall, **{f: t[f] for f in PHASES})
    row["host_remainder_ms"] = wall - t["fill_ms"] - t["reduce_ms"] - t["locate_ms"] - t["trace_ms"]
    return row, (sel, res, cig), int(t["best_flagged"])


def run_recipe(ctx, Q, T, W, nfwd, flag, nf, nc):
    t0 = time.perf_counter()
    res, _ = ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=0, want_cigar=False)
    t1 = time.perf_counter()
    p1 = phases(ctx)
    sel = pair_numpy(res, W, nf, nc, nfwd)
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    hit = pos >= 0
    chosen = (W["cand_off"][:-1].reshape(nf, 2) + pos)[hit]          # (fragment, mate) order
    out = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE)
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
    row = dict(wall_ms=(t3 - t0) * 1e3, call1_wall_ms=(t1 - t0) * 1e3, numpy_pairing_ms=(t2 - t1) * 1e3, call2_wall_ms=(t3 - t2) * 1e3,
               wall_without_numpy_ms=(t3 - t0 - (t2 - t1)) * 1e3, **{f: p1[f] + p2[f] for f in PHASES})
    return row, (sel, out, cig)


def measure(args, recipe):
    genome, rcodes, roff, W, nfwd, planted = workload(args.frags, args.cands)
    ctx = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib if recipe else None))
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    rows, outs, flagged = {}, {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        for flag in (0, 2):
            if recipe:
                row, o = run_recipe(ctx, Q, T, W, nfwd, flag, args.frags, args.cands)
            else:
                row, o, flagged["flag%d" % flag] = run_mates(ctx, Q, T, W, nfwd, flag)
            if rep > 0:
                rows.setdefault("flag%d" % flag, []).append(row)
            outs[flag] = o
        sys.stderr.write("[gpu_windows_mates_bench] %s: repeat %d done\n" % ("recipe" if recipe else "mates", rep)); sys.stderr.flush()
    Q.free(); T.free(); ctx.close()
    for flag in (0, 2):      # the planted windows win as a proper pair (but for the few decoys that fall on a read's own locus)
        sel = outs[flag][0]
        good = (sel["pos1"] == planted[0::2]) & (sel["pos2"] == planted[1::2]) & (sel["proper"] == 1)
        assert good.mean() > 0.999, good.mean()
    return {k: stats(v) for k, v in rows.items()}, outs, flagged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recipe-child", default=None, help=argparse.SUPPRESS)      # internal: run variant b, leave outputs in this .npz
    args = ap.parse_args()
    if args.recipe_child:
        V, outs, _ = measure(args, True)
        np.savez(args.recipe_child, stats=json.dumps(V), **{"%s%d" % (n, f): outs[f][i] for f in (0, 2) for i, n in enumerate(("sel", "res", "cig"))})
        return
    with tempfile.TemporaryDirectory() as tmp:      # the yardstick first, in a process of its own (this one has not touched the device yet)
        npz = os.path.join(tmp, "recipe.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--frags", str(args.frags), "--cands", str(args.cands), "--reps", str(args.reps), "--recipe-child", npz]
        if args.baseline_lib:
            cmd += ["--baseline-lib", args.baseline_lib]
        subprocess.run(cmd, check=True)
        with np.load(npz) as z:
            B = json.loads(str(z["stats"])); bouts = {f: (z["sel%d" % f], z["res%d" % f], z["cig%d" % f]) for f in (0, 2)}
    A, aouts, flagged = measure(args, False)
    equal = {"flag%d" % f: bool(aouts[f][0].tobytes() == bouts[f][0].tobytes() and (aouts[f][1] == bouts[f][1]).all() and
                                aouts[f][2].tobytes() == bouts[f][2].tobytes()) for f in (0, 2)}
    if not all(equal.values()):
        raise SystemExit("align_windows_mates and the host recipe disagree: %s" % equal)
    out = {"script": "gpu_windows_mates_bench", "fragments": args.frags, "candidates_per_mate": args.cands, "reps": args.reps,
           "min_insert": MIN_INS, "max_insert": MAX_INS, "unpaired_penalty": PENALTY,
           "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)", "outputs_equal": equal, "best_flagged": flagged,
           "variants": {"a_mates": A, "b_recipe": B}}
    cmpd = {}
    for f in ("flag0", "flag2"):
        a, b = A[f], B[f]
        for col in ("wall_ms", "wall_without_numpy_ms"):
            margin = 2 * (b[col]["max"] - b[col]["min"])
            cmpd["%s_vs_b_%s" % (f, col)] = {"a_median": a["wall_ms"]["median"], "b_median": b[col]["median"], "difference": b[col]["median"] - a["wall_ms"]["median"],
                                             "margin_2x_b_spread": margin, "a_faster_beyond_margin": bool(b[col]["median"] - a["wall_ms"]["median"] > margin)}
        cmpd["%s_reduce_over_fill" % f] = a["reduce_ms"]["median"] / a["fill_ms"]["median"]
    out["comparison"] = cmpd
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
