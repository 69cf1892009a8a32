#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_windows (reads against windows of a RESIDENT target set) next to what a caller does without it -- cut the
windows out on the host, upload them as a set of their own, ssw_gpu_align_pairs, free -- on the same pair list, in the same session.

Workload: case (a) of gpu_pairs_bench.py (150-bp reads with ~2 % substitutions and an indel in one of five, windows of 300..700 bp,
flag 0 and flag 2 with CIGARs), the windows drawn from one resident 100 Mb target; and the same list against a resident set of
23 x 100 Mb (above 2^31 residues), half of the windows above absolute offset 2^31.

Every figure is the median of `reps` timed repeats after one warm-up, with min and max beside it.  Measurements:
  windows      Context.align_windows, wall clock of the call (the four index arrays come from the host every time) + its phase times
  cut_upload   wall clock of: host gather of the windows (numpy; reported on its own, a C caller's memcpy loop is faster), seqs_upload,
               align_pairs, seqs_free -- and the phase times of that align_pairs
The baseline runs in a child process on `--baseline-lib` (a build of the commit before this entry point; default: the same library),
so both sides run on the same box within minutes.  `above_2_31_flag2_baseline` is the baseline's align_pairs with flag 2 over a resident
set above 2^31 residues (it answers every pair with a batch call of its own there), timed on `--sample` pairs and SCALED to the list.

usage: gpu_windows_bench.py [--npairs 1000000] [--reps 5] [--sample 2000] [--baseline-lib PATH] [--out out.json] [--skip-big]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
import ssw_amd          # noqa: E402
from sswutil import dna_matrix   # noqa: E402

GENOME = 100000000
COPIES = 23               # 23 x 100 Mb = 2.3e9 >= 2^31 + 2^27 residues
PHASES = ("total_ms", "fill_ms", "locate_ms", "trace_ms")


def workload(npairs, seed=1):
    """-> genome, read codes (flat), read offsets, tbeg, tlen (windows of the ONE 100 Mb target)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=GENOME, dtype=np.int8)
    tlen = rng.integers(300, 701, size=npairs).astype(np.int32)
    tbeg = rng.integers(0, GENOME - 700, size=npairs).astype(np.int64)
    start = tbeg + (rng.random(npairs) * (tlen - 150)).astype(np.int64)
    R = np.empty((npairs, 151), dtype=np.int8)
    for a in range(0, npairs, 100000):
        b = min(npairs, a + 100000)
        R[a:b] = genome[start[a:b, None] + np.arange(151)[None, :]]
    sub = rng.random((npairs, 151)) < 0.02
    R[sub] = (R[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
    lens = np.full(npairs, 150, dtype=np.int64)
    kind = rng.random(npairs)                      # < 0.1: a deletion in the read, < 0.2: an insertion
    pos = rng.integers(10, 140, size=npairs)
    for i in np.nonzero(kind < 0.2)[0]:
        p = int(pos[i])
        if kind[i] < 0.1:
            R[i, p:150] = R[i, p + 1:151]; lens[i] = 149
        else:
            R[i, p + 1:151] = R[i, p:150]; R[i, p] = rng.integers(0, 4); lens[i] = 151
    off = np.zeros(npairs + 1, dtype=np.int64); off[1:] = np.cumsum(lens)
    keep = np.arange(151)[None, :] < lens[:, None]
    return genome, np.ascontiguousarray(R[keep]), off, tbeg, tlen


def upload(ctx, codes, off):
    h = ctx.lib.ssw_gpu_seqs_upload(ctx.h, codes.ctypes.data_as(C.POINTER(C.c_int8)), off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1)
    if not h:
        raise RuntimeError("ssw_gpu_seqs_upload: " + ctx.error())
    s = ssw_amd.Seqs.__new__(ssw_amd.Seqs)
    s.ctx = ctx; s.count = len(off) - 1; s.h = h
    return s


def stats(rows):
    out = {}
    for k in rows[0]:
        v = sorted(r[k] for r in rows)
        out[k] = {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0], "max": v[-1]}
    out["reps"] = len(rows)
    return out


def cut(flat, abs_start, tlen):
    """the windows as one packed set: what the caller gathers on the host for every batch"""
    woff = np.zeros(len(tlen) + 1, dtype=np.int64); woff[1:] = np.cumsum(tlen)
    return np.concatenate([flat[s:s + n] for s, n in zip(abs_start.tolist(), tlen.tolist())]), woff


def run_windows(ctx, Q, T, qidx, tidx, tbeg, tlen, flag, reps):
    mat = dna_matrix(2, 2)
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res, cig = ctx.align_windows(Q, T, qidx, tidx, tbeg, tlen, mat, 5, 3, 1, flag, want_cigar=flag != 0)
        dt = time.perf_counter() - t0
        t = ctx.timing()
        if r > 0:
            rows.append(dict(wall_ms=dt * 1e3, **{k: t[k] for k in PHASES}))
    assert t["win_copied"] == 0 and t["fill_kernel"].startswith("k_fillpairs<")
    return dict(stats(rows), fill_kernel=t["fill_kernel"], cells=t["cells"], gcups_wall=t["cells"] / (stats(rows)["wall_ms"]["median"] * 1e-3) / 1e9), res, cig


def run_cut_upload(ctx, Q, flat, abs_start, qidx, tlen, flag, reps):
    mat = dna_matrix(2, 2)
    rows = []
    ti = np.arange(len(qidx), dtype=np.int32)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        wcodes, woff = cut(flat, abs_start, tlen)
        t1 = time.perf_counter()
        W = upload(ctx, wcodes, woff)
        t2 = time.perf_counter()
        res, cig = ctx.align_pairs(Q, W, qidx, ti, mat, 5, 3, 1, flag, want_cigar=flag != 0)
        t3 = time.perf_counter()
        t = ctx.timing()
        W.free()
        t4 = time.perf_counter()
        if r > 0:
            rows.append(dict(host_cut_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, align_pairs_wall_ms=(t3 - t2) * 1e3, free_ms=(t4 - t3) * 1e3,
                             wall_without_cut_ms=(t4 - t1) * 1e3, wall_ms=(t4 - t0) * 1e3, **{k: t[k] for k in PHASES}))
    return dict(stats(rows), fill_kernel=t["fill_kernel"], window_bytes=int(woff[-1])), res, cig


def child(args):
    """one library, one context: every measurement that library can make -> one JSON line"""
    lib = ssw_amd.load(args.lib)
    ctx = ssw_amd.Context(0, lib)
    ctx.set_exclusive()
    has_windows = hasattr(lib, "ssw_gpu_align_windows")
    genome, rcodes, roff, tbeg, tlen = workload(args.npairs)
    npairs = args.npairs
    qidx = np.arange(npairs, dtype=np.int32); tidx = np.zeros(npairs, dtype=np.int32)
    out = {"lib": os.path.relpath(args.lib or ssw_amd.DEFAULT_LIB, ROOT), "npairs": npairs, "has_align_windows": has_windows}
    Q = upload(ctx, rcodes, roff)
    T = upload(ctx, genome, np.array([0, GENOME], dtype=np.int64)) if has_windows else None
    for flag in (0, 2):
        key = "flag%d" % flag
        base, bres, bcig = run_cut_upload(ctx, Q, genome, tbeg, qidx, tlen, flag, args.reps)
        out[key] = {"cut_upload_align_pairs": base}
        if has_windows:
            win, wres, wcig = run_windows(ctx, Q, T, qidx, tidx, tbeg, tlen, flag, args.reps)
            out[key]["align_windows"] = win
            out[key]["records_equal"] = bool((wres == bres).all() and wcig.tobytes() == bcig.tobytes())
    if T is not None:
        T.free()
    if not args.skip_big:
        flat = np.tile(genome, COPIES)
        toff = np.arange(COPIES + 1, dtype=np.int64) * GENOME
        Tbig = upload(ctx, flat, toff)
        tidx_b = (np.arange(npairs) % COPIES).astype(np.int32); tidx_b[::2] = COPIES - 1      # half of the windows above absolute offset 2^31
        assert (COPIES - 1) * GENOME >= 1 << 31
        if has_windows:
            for flag in (0, 2):
                win, wres, _ = run_windows(ctx, Q, Tbig, qidx, tidx_b, tbeg, tlen, flag, args.reps)
                win["resident_residues"] = int(toff[-1]); win["windows_above_2_31"] = int(((toff[tidx_b] + tbeg) >= (1 << 31)).sum())
                out["flag%d" % flag]["align_windows_above_2_31"] = win
        else:
            # what this library can do with a resident set above 2^31 residues and flag 2: the windows must be sequences of that set, and every
            # flagged pair then takes a batch call of its own.  A sample of windows is appended to the big set as sequences of their own.
            ns = min(args.sample, npairs)
            wcodes, woff = cut(genome, tbeg[:ns], tlen[:ns])
            codes = np.concatenate([flat, wcodes]); off = np.concatenate([toff, toff[-1] + woff[1:]])
            Tbig.free()
            Tbig = upload(ctx, codes, off)
            ti = (COPIES + np.arange(ns)).astype(np.int32)
            rows = []
            for r in range(3):
                t0 = time.perf_counter()
                ctx.align_pairs(Q, Tbig, qidx[:ns], ti, dna_matrix(2, 2), 5, 3, 1, 2)
                rows.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3))
            s = stats(rows[1:])
            out["flag2"]["align_pairs_above_2_31_sample"] = dict(s, sample_pairs=ns, fill_kernel=ctx.timing()["fill_kernel"],
                                                                 scaled_to_npairs_wall_ms=s["wall_ms"]["median"] * npairs / ns, scaled=True)
        Tbig.free()
    Q.free(); ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"script": "gpu_windows_bench", "npairs": args.npairs, "reps": args.reps}
    for name, lib in (("baseline", args.baseline_lib), ("new", None)):      # fresh child processes, one after the other: one context on the device at a time
        if name == "baseline" and lib is None:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--npairs", str(args.npairs), "--reps", str(args.reps), "--sample", str(args.sample)]
        if lib:
            cmd += ["--lib", lib]
        if args.skip_big:
            cmd.append("--skip-big")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("%s run failed (exit %d): nothing further is started" % (name, r.returncode))
        sys.stderr.write("[gpu_windows_bench] %s run done\n" % name); sys.stderr.flush()
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    base = out.get("baseline", out["new"])
    out["baseline_is"] = "baseline" if "baseline" in out else "new (same library)"
    cmpd = {}
    for flag in ("flag0", "flag2"):
        b = base[flag]["cut_upload_align_pairs"]; w = out["new"][flag]["align_windows"]
        c = {"end_to_end_ratio_without_host_cut": b["wall_without_cut_ms"]["median"] / w["wall_ms"]["median"],
             "end_to_end_ratio_with_numpy_cut": b["wall_ms"]["median"] / w["wall_ms"]["median"]}
        for ph in ("fill_ms", "locate_ms", "trace_ms"):
            margin = 2 * (b[ph]["max"] - b[ph]["min"])
            d = w[ph]["median"] - b[ph]["median"]
            c[ph] = {"baseline_median": b[ph]["median"], "windows_median": w[ph]["median"], "difference": d, "margin_2x_baseline_spread": margin,
                     "within_margin": bool(d <= margin)}
            if "baseline" in out:      # the new build's own align_pairs over uploaded windows: k_fillpairs and the window kernels gained an argument
                n = out["new"][flag]["cut_upload_align_pairs"][ph]
                c[ph]["new_align_pairs_median"] = n["median"]; c[ph]["new_align_pairs_within_margin"] = bool(n["median"] - b[ph]["median"] <= margin)
        cmpd[flag] = c
    out["comparison"] = cmpd
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
