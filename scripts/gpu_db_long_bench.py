#!/usr/bin/env python3
"""GPU box: the long class of the database path (queries above k_filldb's 640 residues on the strip kernel's pair mode) next
to a build of the parent commit, which answers such rows on the per-target loop and takes a streamed search with one of them off the
streamed path.  Database: BASELINE config 5's 10 000 entries (workloads.protein_config), BLOSUM50, gaps 3/1, score only.

  (a) long queries alone: `--nlong` queries of 641..2 000 residues (uniform lengths, background residue frequencies, every 100th holds a
      mutated database entry): align_batch at flag 0 and search_topk with k = 10.  The baseline runs the first `--sample` of them
      against the first `--sample-db` entries only (there every target is a round trip of ~10 ms: the whole database would take minutes
      per call); its time is reported as measured AND scaled by (entries / sample-db) x (nlong / sample).  Its cost is one round trip per
      target for every call, so the factor for the queries overstates what the parent would need for the whole list in one call: the
      comparison that counts is the one scaled by the targets alone.
  (b) one long query among many: protein_config(queries = `--nq`) with query 17 replaced by a 700-residue one, against the first `--db-b`
      entries (both builds): search_topk with k = 10 and search_db with a no-op chunk function.
  (c) unchanged paths: (b) without the replacement.
  fill rates (fill_cells / fill_ms of ssw_gpu_last_timing, padding rows counted): the class in (a), k_filldb in (c).
  parity: `--parity` (query, target) pairs of (a) against the reference (parity.expected): 0 mismatches required.

Protocol: each library in a child process of its own, one after the other; per measurement one warm-up, then `--reps` timed repeats: median
[min, max] of the wall clock of the call.  Acceptance: (a), (b) faster than the baseline by more than twice its max - min; (c) within twice
its max - min.

usage: gpu_db_long_bench.py [--nlong 256] [--sample 16] [--sample-db 500] [--nq 5000] [--db-b 2000] [--reps 5] [--baseline-reps 3]
                            [--parity 200] [--baseline-lib PATH] [--out out.json]"""
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
import workloads as W   # noqa: E402
from gpu_windows_bench import stats   # noqa: E402
from parity import expected   # noqa: E402
from sswutil import RES_FIELDS, mutate   # noqa: E402

KEEP = ("fill_ms", "reduce_ms", "total_ms")


def long_queries(db, count, seed=6160):
    rng = np.random.default_rng(seed)
    lens = rng.integers(641, 2001, size=count)
    qs = [rng.choice(20, size=int(L), p=W._AA_FREQ).astype(np.int8) for L in lens]
    for i in range(0, count, 100):      # 1 % planted homologs: a mutated database entry inside the query
        m = np.asarray(mutate(db[int(rng.integers(0, len(db)))], rng, 0.15, 0.02, 0.02, 20), dtype=np.int8)[:600]
        qs[i][20:20 + len(m)] = m
    return qs


def measure(ctx, name, fn, reps, out):
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        val = fn()
        dt = time.perf_counter() - t0
        t = ctx.timing()
        if r > 0:
            rows.append(dict(wall_ms=dt * 1e3, **{k: t[k] for k in KEEP}))
        sys.stderr.write("[gpu_db_long_bench] %s run %d of %d: %.1f ms (%s)\n" % (name, r, reps, dt * 1e3, t["fill_kernel"])); sys.stderr.flush()
    s = stats(rows)
    out[name] = dict(s, fill_kernel=t["fill_kernel"], fill_launches=t["fill_launches"], fill_cells=t["fill_cells"], cells=t["cells"],
                     db_long_pairs=t.get("db_long_pairs", 0),
                     fill_tcups=t["fill_cells"] / (s["fill_ms"]["median"] * 1e-3) / 1e12 if s["fill_ms"]["median"] > 0 else None)
    sys.stderr.write("[gpu_db_long_bench] %s: %s\n" % (name, json.dumps(out[name]))); sys.stderr.flush()      # (kept if a later step runs out of time)
    return val


def child(args):
    ctx = ssw_amd.Context(0, ssw_amd.load(args.lib))
    ctx.set_exclusive()
    db, qs, mat = W.protein_config(0, queries=args.nq)
    lq = long_queries(db, args.nlong)
    n = args.sub if args.sub else args.nlong
    na = args.sub_db if args.sub_db else len(db)
    out = {"lib": os.path.relpath(args.lib or ssw_amd.DEFAULT_LIB, ROOT), "long_queries": n, "db_entries_a": na, "queries_b": args.nq, "db_entries_b": args.db_b}
    T = ctx.upload(db[:na])
    kw = dict(gapO=3, gapE=1)
    # (a)
    QL = ctx.upload(lq[:n])
    res, _ = measure(ctx, "a_align_batch", lambda: ctx.align_batch(QL, T, mat, 24, want_cigar=False, **kw), args.reps, out)
    measure(ctx, "a_search_topk10", lambda: ctx.search_topk(QL, T, 10, mat, 24, want_cigar=False, **kw), args.reps, out)
    if args.parity:
        rng = np.random.default_rng(1)
        bad = 0
        for _ in range(args.parity):
            q, t = int(rng.integers(0, n)), int(rng.integers(0, na))
            exp, _c = expected(lq[q], mat, 24, db[t], 3, 1, 0, 0, 0, len(lq[q]) // 2, 2)
            g = res[q, t]
            bad += 0 if exp is not None and int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp else 1
        out["parity"] = {"pairs": args.parity, "mismatches": bad}
    QL.free(); T.free()
    # (b), (c)
    T = ctx.upload(db[:args.db_b])
    for name, sub in (("b", True), ("c", False)):
        q2 = list(qs)
        if sub:
            q2[17] = lq[0][:700].copy()
        Q = ctx.upload(q2)
        measure(ctx, name + "_search_topk10", lambda: ctx.search_topk(Q, T, 10, mat, 24, want_cigar=False, **kw), args.reps, out)
        measure(ctx, name + "_search_db", lambda: ctx.search_db(Q, T, mat, 24, 3, 1, -1, 2, 0, lambda t0, h: 0), args.reps, out)
        Q.free()
    T.free(); ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlong", type=int, default=256)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--sample-db", type=int, default=500)
    ap.add_argument("--nq", type=int, default=5000)
    ap.add_argument("--db-b", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--parity", type=int, default=200)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sub", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--sub-db", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"script": "gpu_db_long_bench", "nlong": args.nlong, "sample": args.sample, "sample_db": args.sample_db, "nq": args.nq, "db_b": args.db_b,
           "reps": args.reps, "baseline_reps": args.baseline_reps}
    for name, lib in (("new", None), ("baseline", args.baseline_lib)):      # fresh child processes, one after the other
        if name == "baseline" and lib is None:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nlong", str(args.nlong), "--nq", str(args.nq), "--db-b", str(args.db_b)]
        cmd += ["--lib", lib, "--sub", str(args.sample), "--sub-db", str(args.sample_db), "--parity", "0", "--reps", str(args.baseline_reps)] if lib else \
               ["--parity", str(args.parity), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=1000)      # (the child's progress lines go straight to stderr)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:])
            raise SystemExit("%s run failed (exit %d): nothing further is started" % (name, r.returncode))
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    cmpd = {}
    if "baseline" in out:
        kt = out["new"]["db_entries_a"] / float(out["baseline"]["db_entries_a"])      # (a): the baseline's targets are a subsample too
        k = kt * args.nlong / float(out["baseline"]["long_queries"])
        for key in ("a_align_batch", "a_search_topk10", "b_search_topk10", "b_search_db", "c_search_topk10", "c_search_db"):
            w, b = out["new"][key]["wall_ms"], out["baseline"][key]["wall_ms"]
            f = kt if key.startswith("a_") else 1.0      # what the acceptance compares: (a) scaled by the targets alone
            margin = 2 * (b["max"] - b["min"]) * f
            c = {"new_ms": w, "baseline_ms": b, "margin_2x_baseline_spread_ms": margin, "ratio": b["median"] * f / w["median"]}
            if key.startswith("a_"):
                c["baseline_queries"] = out["baseline"]["long_queries"]; c["baseline_entries"] = out["baseline"]["db_entries_a"]
                c["baseline_scaled_by_targets_ms"] = b["median"] * kt; c["baseline_scaled_by_targets_and_queries_ms"] = b["median"] * k
            c["accepted"] = bool(abs(w["median"] - b["median"]) <= margin or w["median"] < b["median"]) if key.startswith("c_") else bool(w["median"] < b["median"] * f - margin)
            cmpd[key] = c
    cmpd["fill_tcups"] = {"long_class_a": out["new"]["a_align_batch"]["fill_tcups"], "k_filldb_c": out["new"]["c_search_db"]["fill_tcups"]}
    cmpd["parity_mismatches"] = out["new"].get("parity", {}).get("mismatches")
    out["comparison"] = cmpd
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
