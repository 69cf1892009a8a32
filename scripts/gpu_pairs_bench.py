#!/usr/bin/env python3
"""GPU box: ssw_gpu_align_pairs (explicit (query, target) pair lists) -- wall-clock GCUPS of the call with the sequences resident, its
phase split (ssw_gpu_last_timing), next to the same work as a 16-thread ssw_align loop and as the reference (oracle/_ref) on 16 threads,
both measured on a sample and scaled (scripts/pairs_loop.c: 16 native threads, compiled here with the system C compiler).  One JSON line (and profiles/<out>.json when given).

  (a)  one-to-one DNA: 150-bp reads (~2 % substitutions + indels), each against its own 300..700-bp window, flag 0; and flag 2 with
       CIGARs
  (b)  one-to-many proteins: 2 048 queries x 64 random entries each out of 10 000, BLOSUM50, flag 0

usage: gpu_pairs_bench.py [npairs_a=1000000] [npairs_a_flag2=1000000] [sample=4000] [out.json]"""
import concurrent.futures as cf
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "complete-striped-smith-waterman-library_amd"))
import ssw_amd          # noqa: E402
from sswutil import blosum50, dna_matrix, mutate   # noqa: E402

NA = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
NA2 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
SAMPLE = int(sys.argv[3]) if len(sys.argv) > 3 else 4000
OUT = sys.argv[4] if len(sys.argv) > 4 else None
THREADS = 16
WORK = tempfile.mkdtemp(prefix="pairs_bench_")
LOOP = os.path.join(WORK, "pairs_loop")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libssw_ref.so")


def case_a(npairs, seed=1):
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=4000000, dtype=np.int8)
    wins, reads = [], []
    for i in range(npairs):
        wl = int(rng.integers(300, 701)); ws = int(rng.integers(0, len(genome) - wl))
        w = genome[ws:ws + wl]
        s = int(rng.integers(0, wl - 150))
        r = w[s:s + 150].copy()
        k = rng.random(150) < 0.02
        r[k] = (r[k] + rng.integers(1, 4, size=int(k.sum()))) % 4
        if rng.random() < 0.2:      # an indel in one read of five
            p = int(rng.integers(10, 140))
            r = np.concatenate([r[:p], r[p + 1:]]) if rng.random() < 0.5 else np.concatenate([r[:p], rng.integers(0, 4, 1, dtype=np.int8), r[p:]])
        wins.append(w); reads.append(r.astype(np.int8))
    idx = np.arange(npairs, dtype=np.int32)
    return reads, wins, idx, idx.copy()


def case_b(seed=2):
    rng = np.random.default_rng(seed)
    db = [rng.integers(0, 20, size=int(rng.integers(100, 600)), dtype=np.int8) for _ in range(10000)]
    qs = []
    for i in range(2048):
        src = db[int(rng.integers(0, 10000))]
        L = min(len(src), int(rng.integers(80, 400)))
        qs.append(mutate(src[:L], rng, 0.25, 0.02, 0.02, 20) if rng.random() < 0.5 else rng.integers(0, 20, size=L, dtype=np.int8))
    qidx = np.repeat(np.arange(2048, dtype=np.int32), 64)
    tidx = rng.integers(0, 10000, size=2048 * 64).astype(np.int32)
    return qs, db, qidx, tidx


def loop_rate(libpath, reads, refs, qidx, tidx, mat, n, gapO, gapE, flag, sample, rng):
    """the loop "ssw_init + ssw_align per pair" on THREADS native threads (scripts/pairs_loop.c) over a sample of the list -> GCUPS"""
    pick = rng.choice(len(qidx), size=min(sample, len(qidx)), replace=False)
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    path = os.path.join(WORK, "pairs_%d.bin" % flag)
    with open(path, "wb") as f:
        f.write(np.array([n, gapO, gapE, len(pick)], dtype="<i4").tobytes()); f.write(mat.tobytes())
        for i in pick:
            rd = np.asarray(reads[qidx[i]], dtype=np.int8); rf = np.asarray(refs[tidx[i]], dtype=np.int8)
            f.write(np.array([len(rd), len(rf)], dtype="<i4").tobytes()); f.write(rd.tobytes()); f.write(rf.tobytes())
    out = subprocess.run([LOOP, libpath, path, str(THREADS), str(flag)], check=True, capture_output=True, text=True).stdout.split()
    dt, cells = float(out[0]), float(out[1])
    return {"sample_pairs": len(pick), "seconds": dt, "gcups": cells / dt / 1e9, "threads": THREADS}


def gpu_rate(ctx, Q, T, qidx, tidx, mat, n, gapO, gapE, flag, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        res, cig = ctx.align_pairs(Q, T, qidx, tidx, mat, n, gapO, gapE, flag, want_cigar=flag != 0)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, ctx.timing(), res, cig)
    dt, t, res, cig = best
    return {"seconds": dt, "gcups": t["cells"] / dt / 1e9, "cells": t["cells"],
            "timing": {k: t[k] for k in ("total_ms", "fill_ms", "reduce_ms", "locate_ms", "trace_ms", "fill_launches", "fill_cells", "fill_kernel")}}, res, cig


def parity(res, cig, reads, refs, qidx, tidx, mat, n, gapO, gapE, flag, sample, rng):
    from parity import expected
    from sswutil import RES_FIELDS
    bad = 0
    for i in rng.choice(len(qidx), size=min(sample, len(qidx)), replace=False):
        rd, rf = reads[qidx[i]], refs[tidx[i]]
        exp, ecig = expected(rd, mat, n, rf, gapO, gapE, flag, 0, 0, len(rd) // 2, 2)
        g = res[i]
        off, ln = int(g["cigar_off"]), int(g["cigarLen"])
        gc = [int(x) for x in cig[off:off + ln]] if ln > 0 else []
        if exp is None or {k: int(g[k]) for k in RES_FIELDS} != exp or gc != ecig:
            bad += 1
    return bad


def main():
    subprocess.run(["cc", "-O2", "-o", LOOP, os.path.join(ROOT, "scripts", "pairs_loop.c"), "-ldl", "-lpthread"], check=True)
    lib = ssw_amd.load()
    ctx = ssw_amd.Context(0, lib)
    ctx.set_exclusive()
    ref = REF_SO if os.path.exists(REF_SO) else None
    rng = np.random.default_rng(7)
    out = {"script": "gpu_pairs_bench", "threads_for_loops": THREADS}
    dna = dna_matrix(2, 2)

    reads, wins, qi, ti = case_a(NA)
    Q = ctx.upload(reads); T = ctx.upload(wins)
    g, res, cig = gpu_rate(ctx, Q, T, qi, ti, dna, 5, 3, 1, 0)
    g["parity_mismatches"] = parity(res, cig, reads, wins, qi, ti, dna, 5, 3, 1, 0, 2000, rng)
    g["ssw_align_loop"] = loop_rate(ssw_amd.DEFAULT_LIB, reads, wins, qi, ti, dna, 5, 3, 1, 0, SAMPLE, rng)
    if ref is not None:
        g["reference_16"] = loop_rate(ref, reads, wins, qi, ti, dna, 5, 3, 1, 0, SAMPLE, rng)
    out["a_flag0"] = dict(npairs=NA, **g)
    Q.free(); T.free()

    reads, wins, qi, ti = reads[:NA2], wins[:NA2], qi[:NA2], ti[:NA2]
    Q = ctx.upload(reads); T = ctx.upload(wins)
    g, res, cig = gpu_rate(ctx, Q, T, qi, ti, dna, 5, 3, 1, 2, reps=2)
    g["parity_mismatches"] = parity(res, cig, reads, wins, qi, ti, dna, 5, 3, 1, 2, 2000, rng)
    g["ssw_align_loop"] = loop_rate(ssw_amd.DEFAULT_LIB, reads, wins, qi, ti, dna, 5, 3, 1, 2, SAMPLE, rng)
    if ref is not None:
        g["reference_16"] = loop_rate(ref, reads, wins, qi, ti, dna, 5, 3, 1, 2, SAMPLE, rng)
    out["a_flag2_cigar"] = dict(npairs=NA2, **g)
    Q.free(); T.free()

    qs, db, qi, ti = case_b()
    b50 = blosum50()
    Q = ctx.upload(qs); T = ctx.upload(db)
    g, res, cig = gpu_rate(ctx, Q, T, qi, ti, b50, 24, 3, 1, 0)
    g["parity_mismatches"] = parity(res, cig, qs, db, qi, ti, b50, 24, 3, 1, 0, 2000, rng)
    g["ssw_align_loop"] = loop_rate(ssw_amd.DEFAULT_LIB, qs, db, qi, ti, b50, 24, 3, 1, 0, SAMPLE, rng)
    if ref is not None:
        g["reference_16"] = loop_rate(ref, qs, db, qi, ti, b50, 24, 3, 1, 0, SAMPLE, rng)
    out["b_protein_flag0"] = dict(npairs=len(qi), **g)
    Q.free(); T.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
