#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_windows_mates_rescue (mate rescue on the device) next to the recipe a caller needs without it.

Workload: gpu_windows_mates_bench's list -- `--frags` fragments of 2 x 150 bp (FR) of one resident 100 Mb target, `--cands` candidates per
mate.  In every tenth fragment mate 2's true candidate is REMOVED: a decoy takes its place, so that every group keeps `--cands` candidates
and the numpy part of the recipe stays vectorised.  max_anchors 2, anchor_min_score 100 (so that decoys are no anchors), rescue_pad 16, min_insert 100, max_insert 1000, unpaired_penalty 17.

Rows (flag 0, and flag 2 with CIGARs):
  i    the removed list: Context.align_windows_mates_rescue (this library) against the RECIPE on `--baseline-lib` (a build of the parent
       commit): align_windows at flag 0 over all candidates, the rescue windows in numpy (reported on its own), align_windows_mates over
       the augmented list (a group gets its rescue slots up to the last non-empty one).  The two must give the same selections, records and CIGAR words, or the script fails.
  ii   the full list (nothing removed, nothing to rescue): align_windows_mates_rescue against the parent's align_windows_mates.
       With nothing to rescue every slot is empty and the two answers must be equal as well.
  iii  the full list: align_windows_mates of this library against the parent's; with `--bench-alt N`, bench.py --gpus 1 --steps 20
       --warmup 5 N times with either library, alternating, each run a process of its own (the library through SSW_LIB).
Each library runs in a child process of its own; every figure is the median of `--reps` timed repeats after one warm-up, with min and max.
A difference counts when it exceeds twice the parent's max - min.  Also reported: rescue_windows, the share of removed mates that come
back in a proper pair, and the mismatches against the reference on a sample of 200 rescued winners.

`--mates-only` runs row iii alone, this build's process first (the rescue calls' large host allocations leave a process slower).

usage: gpu_mates_rescue_bench.py [--frags 1000000] [--cands 4] [--reps 5] [--bench-alt N] [--mates-only] [--baseline-lib PATH] [--out out.json]"""
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

ANCHORS, PAD, ANCHOR_MIN = 2, 16, 100      # (anchor_min_score 100: a read of 150 scores about 280 at its locus, about 30 against a decoy)


def remove_mate2(W, planted, nf, nc, seed=7):
    """-> a copy of the list in which the true candidate of mate 2 of every tenth fragment is replaced by a decoy, and those fragments"""
    rng = np.random.default_rng(seed)
    lost = np.arange(0, nf, 10)
    at = (2 * lost + 1) * nc + planted[2 * lost + 1]
    V = {k: v.copy() for k, v in W.items()}
    V["tbeg"][at] = rng.integers(0, GENOME - 700, size=len(at))
    return V, lost


def rescue_numpy(res, W, nf, nc, nfwd):
    """the rule of include/ssw_gpu.h (FR, one target, every group nc candidates, reads of RL) over the flag-0 records -> augmented list"""
    s = res["score1"].astype(np.int64).reshape(nf, 2, nc)
    ok = ((res["status"] == 0) & (res["score1"] > 0)).reshape(nf, 2, nc)
    E = (W["tbeg"] + res["ref_end1"]).reshape(nf, 2, nc)
    B = E - RL + 1
    minus = (W["qidx"] >= nfwd).reshape(nf, 2, nc)
    m1, m2 = minus[:, 0, :, None], minus[:, 1, None, :]
    ins = np.where(m1, E[:, 0, :, None] - B[:, 1, None, :], E[:, 1, None, :] - B[:, 0, :, None]) + 1
    proper = (m1 != m2) & (ins >= MIN_INS) & (ins <= MAX_INS) & ok[:, 0, :, None] & ok[:, 1, None, :]
    partner = np.stack([proper.any(axis=2), proper.any(axis=1)], axis=1)            # [nf, mate, candidate]: has a proper partner
    key = np.where(ok & (s >= ANCHOR_MIN), (s << 32) | (0xffffffff - np.arange(nc, dtype=np.int64)), 0)
    rank = np.argsort(-key, axis=2, kind="stable")[:, :, :ANCHORS]                  # anchors of either mate, best first
    rkey = np.take_along_axis(key, rank, axis=2)
    A = ANCHORS
    q = np.empty((nf, 2, nc + A), dtype=np.int32); t = np.zeros((nf, 2, nc + A), dtype=np.int32)
    b = np.zeros((nf, 2, nc + A), dtype=np.int64); ln = np.zeros((nf, 2, nc + A), dtype=np.int32)
    q[:, :, :nc] = W["qidx"].reshape(nf, 2, nc); b[:, :, :nc] = W["tbeg"].reshape(nf, 2, nc); ln[:, :, :nc] = W["tlen"].reshape(nf, 2, nc)
    mq = np.arange(2 * nf, dtype=np.int32).reshape(nf, 2)
    for h in (0, 1):
        o = 1 - h
        live = (rkey[:, o, :] > 0) & ~np.take_along_axis(partner[:, o, :], rank[:, o, :], axis=1)
        sa = np.take_along_axis(minus[:, o, :], rank[:, o, :], axis=1)
        Ea = np.take_along_axis(E[:, o, :], rank[:, o, :], axis=1); Ba = np.take_along_axis(B[:, o, :], rank[:, o, :], axis=1)
        down = ~sa                                                                   # FR: the rescued mate is on the other strand; the minus one lies downstream
        w0 = np.where(down, Ba + MIN_INS - RL - PAD, Ea + 1 - MAX_INS - PAD); w1 = np.where(down, Ba + MAX_INS - 1 + PAD, Ea - MIN_INS + RL + PAD)
        w0 = np.maximum(w0, 0); w1 = np.minimum(w1, GENOME - 1)
        live &= w1 >= w0
        q[:, h, nc:] = mq[:, h, None] + np.where(live & ~sa, nfwd, 0)
        b[:, h, nc:] = np.where(live, w0, 0); ln[:, h, nc:] = np.where(live, w1 - w0 + 1, 0)
    # a caller appends what it has to: a group keeps its slots up to the last non-empty one (positions as in the call's augmented group)
    keep = np.ones((nf, 2, nc + A), dtype=bool)
    keep[:, :, nc:] = np.cumsum((ln[:, :, :nc - 1:-1] > 0), axis=2)[:, :, ::-1] > 0
    off = np.concatenate([[0], np.cumsum(keep.sum(axis=2).reshape(-1))]).astype(np.int64)
    return dict(cand_off=off, qidx=q[keep], tidx=t[keep], tbeg=b[keep], tlen=ln[keep]), int((ln[:, :, nc:] > 0).sum())


def row_of(ctx, wall):
    t = ctx.timing()
    row = dict(wall_ms=wall, **{f: t[f] for f in PHASES})
    row["rescue_windows"] = int(t.get("rescue_windows", 0)); row["fill_launches"] = int(t["fill_launches"])
    return row


def run_rescue(ctx, Q, T, W, nfwd, flag):
    mq = np.arange(nfwd, dtype=np.int32)
    t0 = time.perf_counter()
    sel, res, org, cig = ctx.align_windows_mates_rescue(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], nfwd, mq, MAT, 5, MIN_INS, MAX_INS,
                                                        PENALTY, max_anchors=ANCHORS, anchor_min_score=ANCHOR_MIN, rescue_pad=PAD, flag=flag, want_cigar=flag != 0)
    return row_of(ctx, (time.perf_counter() - t0) * 1e3), (sel, res, cig, org)


def run_mates(ctx, Q, T, W, nfwd, flag):
    t0 = time.perf_counter()
    sel, res, cig = ctx.align_windows_mates(Q, T, W["cand_off"], W["qidx"], W["tidx"], W["tbeg"], W["tlen"], nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                            flag=flag, want_cigar=flag != 0)
    return row_of(ctx, (time.perf_counter() - t0) * 1e3), (sel, res, cig)


def run_recipe(ctx, Q, T, W, nfwd, flag, nf, nc):
    t0 = time.perf_counter()
    res, _ = ctx.align_windows(Q, T, W["qidx"], W["tidx"], W["tbeg"], W["tlen"], MAT, 5, flag=0, want_cigar=False)
    t1 = time.perf_counter()
    V, filled = rescue_numpy(res, W, nf, nc, nfwd)
    t2 = time.perf_counter()
    sel, out, cig = ctx.align_windows_mates(Q, T, V["cand_off"], V["qidx"], V["tidx"], V["tbeg"], V["tlen"], nfwd, MAT, 5, MIN_INS, MAX_INS, PENALTY,
                                            flag=flag, want_cigar=flag != 0)
    t3 = time.perf_counter()
    row = dict(wall_ms=(t3 - t0) * 1e3, call1_wall_ms=(t1 - t0) * 1e3, numpy_rescue_ms=(t2 - t1) * 1e3, call2_wall_ms=(t3 - t2) * 1e3,
               wall_without_numpy_ms=(t3 - t0 - (t2 - t1)) * 1e3, rescue_windows=filled)
    return row, (sel, out, cig)


def measure(args, parent):
    genome, rcodes, roff, W, nfwd, planted = workload(args.frags, args.cands)
    V, lost = remove_mate2(W, planted, args.frags, args.cands)
    ctx = ssw_amd.Context(0, ssw_amd.load(args.baseline_lib if parent else None))
    base = upload(ctx, rcodes, roff); base.lengths = np.diff(roff)
    Q = base.with_revcomp(); base.free()
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64))
    rows, outs = {}, {}
    for rep in range(args.reps + 1):      # repeat 0 is the warm-up
        for flag in (0, 2):
            k = "flag%d" % flag
            if args.mates_only:      # row iii alone: neither the recipe nor a rescue call runs in the process
                got = {"ii_iii_mates" if parent else "iii_mates": run_mates(ctx, Q, T, W, nfwd, flag)}
            elif parent:
                got = {"i_recipe": run_recipe(ctx, Q, T, V, nfwd, flag, args.frags, args.cands), "ii_iii_mates": run_mates(ctx, Q, T, W, nfwd, flag)}
            else:
                got = {"i_rescue": run_rescue(ctx, Q, T, V, nfwd, flag), "ii_rescue_full": run_rescue(ctx, Q, T, W, nfwd, flag),
                       "iii_mates": run_mates(ctx, Q, T, W, nfwd, flag)}
            for name, (row, o) in got.items():
                if rep > 0:
                    rows.setdefault(name, {}).setdefault(k, []).append(row)
                outs[(name, flag)] = o
        sys.stderr.write("[gpu_mates_rescue_bench] %s: repeat %d done\n" % ("parent" if parent else "this build", rep)); sys.stderr.flush()
    extra = {}
    if not parent and not args.mates_only:      # what the rescue brought back, and a sample of rescued winners against the reference
        from parity import expected
        from sswutil import RES_FIELDS
        sel, res, cig, org = outs[("i_rescue", 2)]
        extra["removed_fragments"] = int(len(lost)); extra["removed_recovered_proper"] = float(((sel["proper"][lost] == 1) & (org["anchor"][lost, 1] >= 0)).mean())
        resc = np.argwhere(org["anchor"] >= 0)
        pick = resc[np.random.default_rng(11).choice(len(resc), size=min(200, len(resc)), replace=False)]
        reads = rcodes.reshape(-1, RL)
        bad = 0
        for f, h in pick:
            o, rec = org[f, h], res[f, h]
            qi = int(o["qidx"])
            rd = reads[qi] if qi < nfwd else np.ascontiguousarray(3 - reads[qi - nfwd][::-1])
            rf = np.ascontiguousarray(genome[int(o["tbeg"]):int(o["tbeg"]) + int(o["tlen"])])
            exp, xcig = expected(np.ascontiguousarray(rd, dtype=np.int8), MAT, 5, rf, 3, 1, 2, 0, 0, RL // 2, 2)
            off, n = int(rec["cigar_off"]), int(rec["cigarLen"])
            bad += not (exp is not None and {x: int(rec[x]) for x in RES_FIELDS} == exp and [int(x) for x in cig[off:off + n]] == xcig)
        extra["reference_sample"] = int(len(pick)); extra["reference_mismatches"] = int(bad)
    Q.free(); T.free(); ctx.close()
    return {n: {k: stats(v) for k, v in d.items()} for n, d in rows.items()}, outs, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-alt", type=int, default=0, help="runs of bench.py with either library, alternating (0: none)")
    ap.add_argument("--mates-only", action="store_true", help="row iii alone, this build's process FIRST, then the parent's")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # internal: "parent" or "this", outputs left in --npz
    ap.add_argument("--npz", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        V, outs, extra = measure(args, args.child == "parent")
        keep = {"%s_%d_%s" % (n, f, w): o[i] for (n, f), o in outs.items() for i, w in enumerate(("sel", "res", "cig"))}
        np.savez(args.npz, stats=json.dumps(V), extra=json.dumps(extra), **keep)
        return
    got = {}
    with tempfile.TemporaryDirectory() as tmp:      # either library in a process of its own, the parent's first
        for who in (("this", "parent") if args.mates_only else ("parent", "this")):
            npz = os.path.join(tmp, who + ".npz")
            cmd = [sys.executable, os.path.abspath(__file__), "--frags", str(args.frags), "--cands", str(args.cands), "--reps", str(args.reps), "--child", who, "--npz", npz]
            if args.baseline_lib:
                cmd += ["--baseline-lib", args.baseline_lib]
            if args.mates_only:
                cmd += ["--mates-only"]
            subprocess.run(cmd, check=True)
            with np.load(npz) as z:
                got[who] = (json.loads(str(z["stats"])), json.loads(str(z["extra"])), {k: z[k] for k in z.files if k not in ("stats", "extra")})
    P, _, po = got["parent"]; N, extra, no = got["this"]
    equal = {}
    for a, b, name in ((("iii_mates", "ii_iii_mates", "iii"),) if args.mates_only else
                       (("i_rescue", "i_recipe", "i"), ("ii_rescue_full", "ii_iii_mates", "ii"), ("iii_mates", "ii_iii_mates", "iii"))):
        for f in (0, 2):
            x, y = [no["%s_%d_%s" % (a, f, w)] for w in ("sel", "res", "cig")], [po["%s_%d_%s" % (b, f, w)] for w in ("sel", "res", "cig")]
            equal["%s_flag%d" % (name, f)] = bool(x[0].tobytes() == y[0].tobytes() and x[1].shape == y[1].shape and (x[1] == y[1]).all() and x[2].tobytes() == y[2].tobytes())
    if not all(equal.values()):
        raise SystemExit("this build and the parent's recipe disagree: %s" % equal)
    out = {"script": "gpu_mates_rescue_bench", "fragments": args.frags, "candidates_per_mate": args.cands, "reps": args.reps, "max_anchors": ANCHORS, "anchor_min_score": ANCHOR_MIN,
           "rescue_pad": PAD, "min_insert": MIN_INS, "max_insert": MAX_INS, "unpaired_penalty": PENALTY,
           "baseline_lib": args.baseline_lib or "this library (no --baseline-lib)", "outputs_equal": equal, "this_build": N, "parent": P,
           "mates_only": bool(args.mates_only)}
    out.update(extra)
    cmpd = {}
    for f in ("flag0", "flag2"):
        for name, a, b, cols in ((("iii", N["iii_mates"][f], P["ii_iii_mates"][f], ("wall_ms",)),) if args.mates_only else
                                 (("i", N["i_rescue"][f], P["i_recipe"][f], ("wall_ms", "wall_without_numpy_ms")), ("ii", N["ii_rescue_full"][f], P["ii_iii_mates"][f], ("wall_ms",)),
                                  ("iii", N["iii_mates"][f], P["ii_iii_mates"][f], ("wall_ms",)))):
            for col in cols:
                margin = 2 * (b[col]["max"] - b[col]["min"])
                d = b[col]["median"] - a["wall_ms"]["median"]
                cmpd["%s_%s_vs_parent_%s" % (name, f, col)] = {"this_median": a["wall_ms"]["median"], "parent_median": b[col]["median"], "parent_minus_this": d,
                                                              "margin_2x_parent_spread": margin, "faster_beyond_margin": bool(d > margin), "within_margin": bool(abs(d) <= margin)}
        if not args.mates_only:
            cmpd["ii_%s_reduce_ms_rescue_vs_mates" % f] = {"rescue_call": N["ii_rescue_full"][f]["reduce_ms"]["median"], "mates_call": N["iii_mates"][f]["reduce_ms"]["median"],
                                                       "fill_ms": N["ii_rescue_full"][f]["fill_ms"]["median"]}
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
                sys.stderr.write("[gpu_mates_rescue_bench] bench.py, %s: %.1f GCUPS\n" % (who, runs[who][-1])); sys.stderr.flush()
        st = {w: stats([{"gcups": v} for v in runs[w]])["gcups"] for w in runs}
        margin = 2 * (st["parent"]["max"] - st["parent"]["min"])
        cmpd["bench_py_gcups"] = {"this": st["this"], "parent": st["parent"], "runs": runs, "margin_2x_parent_spread": margin,
                                  "within_margin": bool(abs(st["this"]["median"] - st["parent"]["median"]) <= margin)}
    out["comparison"] = cmpd
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
