"""Regime and boundary parity of the fused pair / window fill kernel (k_fillpairs) and of its host planner (pairs_core, csrc/ssw_host.c).

Every case goes three ways through ONE helper (_three_ways): (a) Context.align_pairs on the targets as sequences of their own, (b)
Context.align_windows with the same targets laid end to end inside one or two resident sequences (odd and even byte offsets, foreign
residues on both sides), (c) -- where the case asks for it: flag 0 and one flagged setting per family -- Context.align_windows_best with one
candidate per group.  (a) must equal parity.expected() -- the compiled reference -- for EVERY pair (all RES_FIELDS, the CIGAR words, status 1
exactly where the reference returns NULL); (b) and (c) must equal (a) in every field but cigar_off, and in the pool words of every pair.
The helper also asserts WHICH path answered: it splits the pair list by the envelope include/ssw_gpu.h documents (gapO > gapE, n <= 32,
max(mat) <= 49, queries of 1..640 residues with n x ceil(ceil(len/16)/4) x 256 <= 65535, targets of 1..65 000 columns), runs the two sides as
calls of their own, and wants fill_kernel "k_fillpairs<..." with win_copied 0 inside and the opposite outside.  Inside, n_word / n_byte of
the timing record must equal the counts that follow from the reference's scores (score1 >= 255 - bias decides, src/ssw.c:881-899).
Where a case is built to reach a value (a top score, a NULL, a score2, a last-column ref_end1) the assertion is made on the REFERENCE's answer.

Families: 1 length grid (15/16/17, the 32-column planner class, 640/641); 2 unbalanced and idle register halves (1 against T columns); 3 the
column limit 64 999 / 65 000 / 65 001 with the best cell in the last column; 4 the clipping regimes (R 38..40 x max(mat) 46..50, both
forms, forced renormalisation periods, the clipped protein matrix); 5 the 8-bit / 16-bit decision at 254/255/256 - bias and the
padded-length rule of the second best; 6 the alphabet gate n x ceil(R/4) x 256 at n = 24/25/26/32/33; 7 ties (homopolymers, period 2 and 3).
Every family runs on the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source; `not gpu`, small sizes) and on the
MI355X (`gpu`).

Running time, one session, same machine, emulator library already built, the two modules in turn: `pytest -m "not gpu" tests/test_pairs.py`
40.6 s, 57.0 s and 46.6 s; `pytest -m "not gpu" tests/test_pairs_regimes.py` 34.1 s and 34.7 s.  (Building libssw_emu.so, which the first
emulator test of a fresh checkout pays, takes 4 min 18 s more for either.)  That bound, not the case lists, sets the emulator sizes: an
emulated call costs 0.15 s before its first cell and a workgroup steps ALL its chains through its longest target, so the emulator half runs
a cover of each family -- what is left out there is named at each family below -- and the gpu half runs every case in full.
`pytest -m gpu tests/test_pairs_regimes.py` on an MI355X: 28 tests in 4 s (profiles/pairs_regimes_gpu_tests_mi355x.log)."""
import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix

FIELDS = [f for f in ssw_amd.RESULT_DTYPE.names if f != "cigar_off"]
FAST = "k_fillpairs<"
NCH_MAX = 16      # chains of a k_fillpairs workgroup: 256 threads / 16 lanes (small R and n: LDS does not cut it down)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the one helper

def in_envelope(qlen, tlen, n, mat, gapO, gapE):
    """the fast path as include/ssw_gpu.h states it (ssw_gpu_align_pairs, "Fast path")"""
    R = -(-qlen // 16)
    return bool(gapO > gapE and n <= 32 and int(np.max(mat)) <= 49 and 1 <= qlen <= 640 and 1 <= tlen <= 65000 and
                n * (-(-R // 4)) * 256 <= 65535)


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def _lay_out(targets, rng, ncodes):
    """the targets end to end inside one (a single target) or two resident sequences, each behind 1..6 foreign residues and the last one
    before 3..8 more; window starts alternate between odd and even byte offsets of the resident set -> (resident, seq, begin)"""
    nres = 1 if len(targets) < 2 else 2
    resident, seq, beg = [], [0] * len(targets), [0] * len(targets)
    base = 0
    for s in range(nres):
        parts, pos = [], 0
        for j, k in enumerate(range(s, len(targets), nres)):
            pad = int(rng.integers(1, 6))
            if (base + pos + pad) & 1 != (j + s) & 1:
                pad += 1
            parts.append(rng.integers(0, ncodes, size=pad, dtype=np.int8)); pos += pad
            seq[k], beg[k] = s, pos
            parts.append(np.asarray(targets[k], dtype=np.int8)); pos += len(targets[k])
        parts.append(rng.integers(0, ncodes, size=int(rng.integers(3, 9)), dtype=np.int8))
        resident.append(np.ascontiguousarray(np.concatenate(parts)))
        base += len(resident[-1])
    if len(targets) >= 2:
        start = [beg[k] + (len(resident[0]) if seq[k] else 0) for k in range(len(targets))]
        assert any(x & 1 for x in start) and not all(x & 1 for x in start)
    return resident, np.array(seq, dtype=np.int32), np.array(beg, dtype=np.int64)


def _same(tag, a, acig, g, gcig, i, bad):
    if any(int(a[f]) != int(g[f]) for f in FIELDS) or _cig(a, acig) != _cig(g, gcig):
        if len(bad) < 4:
            bad.append("%s pair %d: pairs %s %s, got %s %s" % (tag, i, a, cigar_str(_cig(a, acig)), g, cigar_str(_cig(g, gcig))))


def _three_ways(ctx, reads, targets, qidx, tidx, mat, n, best=False, ncodes=None, inside_budget=0, **kw):
    """every pair against the reference and the three entry points against each other, path asserted per side of the envelope.
    best: also way (c) -- True, or "inside" for the pairs inside the envelope only (the fallback runs twice for it).
    inside_budget: scratch budget (ssw_gpu_set_budget) of the calls inside the envelope, 0: the default
    -> (reference answers [(dict | None, cigar)] in pair order, {True / False: timing of align_pairs on that side})"""
    qidx = np.asarray(qidx, dtype=np.int32); tidx = np.asarray(tidx, dtype=np.int32)
    ncodes = ncodes if ncodes is not None else (4 if n == 5 else n)
    gapO, gapE, flag = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("flag", 0)
    filters, filterd, ml, ss = kw.get("filters", 0), kw.get("filterd", 0), kw.get("maskLen", -1), kw.get("score_size", 2)
    ref = []
    for q, t in zip(qidx, tidx):
        rd = reads[q]
        ref.append(expected(rd, mat, n, targets[t], gapO, gapE, flag, filters, filterd, ml if ml >= 0 else len(rd) // 2, ss))
    inside = np.array([in_envelope(len(reads[q]), len(targets[t]), n, mat, gapO, gapE) for q, t in zip(qidx, tidx)])
    rng = np.random.default_rng(len(targets) * 7919 + len(reads))
    resident, wseq, wbeg = _lay_out(targets, rng, ncodes)
    tlen = np.array([len(targets[t]) for t in tidx], dtype=np.int32)
    minmat = int(np.min(mat))
    bias = -minmat if minmat < 0 else 0
    timings = {}
    Q = ctx.upload(reads); T = ctx.upload(targets); W = ctx.upload(resident)
    try:
        for side in (True, False):
            ix = np.nonzero(inside == side)[0]
            if len(ix) == 0:
                continue
            q, t = qidx[ix], tidx[ix]
            bad = []
            ctx.lib.ssw_gpu_set_budget(ctx.h, inside_budget if side else 0)
            # (a) the targets as their own sequences, against the reference
            ares, acig = ctx.align_pairs(Q, T, q, t, mat, n, **kw)
            tms = [("pairs", ctx.timing())]
            timings[side] = tms[0][1]
            for k, i in enumerate(ix):
                exp, ecig = ref[i]
                g = ares[k]
                if exp is None:
                    ok = int(g["status"]) == 1
                else:
                    ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp and _cig(g, acig) == ecig
                if not ok and len(bad) < 4:
                    bad.append("pair %d (read %d x target %d columns): reference %s %s, pairs %s %s" % (
                        i, len(reads[qidx[i]]), len(targets[tidx[i]]), exp, cigar_str(ecig), g, cigar_str(_cig(g, acig))))
            # (b) the same targets as windows of the resident sequences
            bres, bcig = ctx.align_windows(Q, W, q, wseq[t], wbeg[t], tlen[ix], mat, n, **kw)
            tms.append(("windows", ctx.timing()))
            for k, i in enumerate(ix):
                _same("windows", ares[k], acig, bres[k], bcig, i, bad)
            # (c) one candidate per group
            if best is True or (best == "inside" and side):
                sel, cres, ccig = ctx.align_windows_best(Q, W, np.arange(len(ix) + 1), q, wseq[t], wbeg[t], tlen[ix], mat, n, **kw)
                tms.append(("windows_best", ctx.timing()))
                for k, i in enumerate(ix):
                    a = ares[k]
                    if int(a["status"]) == 0 and int(a["score1"]) > 0:      # eligible: the winner of its group
                        _same("windows_best", a, acig, cres[k], ccig, i, bad)
                        want = (0, -1, 1, 0)
                    else:                                                   # ssw_gpu_search_topk's padding record
                        pad = {f: 0 for f in FIELDS}; pad["ref_begin1"] = pad["read_begin1"] = -1
                        if {f: int(cres[k][f]) for f in FIELDS} != pad or int(cres[k]["cigar_off"]) != -1:
                            bad.append("windows_best pair %d: padding record expected, got %s" % (i, cres[k]))
                        want = (-1, -1, 0, 0)
                    if tuple(int(sel[k][f]) for f in ("best", "second", "n_eligible", "second_score1")) != want:
                        bad.append("windows_best pair %d: selection %s, expected %s" % (i, sel[k], want))
            assert not bad, "\n".join(bad[:6])
            # the path, and what the fill counted
            scored = [ref[i][0]["score1"] for i in ix if ref[i][0] is not None and ref[i][0]["score1"] > 0]
            n_word = sum(1 for s in scored if ss == 1 or (ss == 2 and s >= 255 - bias))
            for who, tm in tms:
                if side:
                    assert tm["fill_kernel"].startswith(FAST) and tm["win_copied"] == 0, (who, tm["fill_kernel"], tm["win_copied"])
                    assert (tm["n_word"], tm["n_byte"]) == (n_word, len(scored) - n_word), (who, tm["n_word"], tm["n_byte"], n_word, len(scored))
                else:
                    assert not tm["fill_kernel"].startswith(FAST), (who, tm["fill_kernel"])
                    assert (tm["win_copied"] > 0) == (who != "pairs"), (who, tm["win_copied"])
            if not side:      # identical windows are gathered once
                distinct = set((int(tidx[i]), int(tlen[i])) for i in ix)
                assert tms[1][1]["win_copied"] == sum(l for _, l in distinct)
    finally:
        ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        Q.free(); T.free(); W.free()
    return ref, timings


def _rand(rng, L, ncodes=4):
    return rng.integers(0, ncodes, size=int(L), dtype=np.int8)


def _subst(seq, rng, rate, ncodes=4, at_least=0):
    """substitutions only (lengths stay): every residue with probability `rate`, and at least `at_least` of them"""
    r = np.array(seq, dtype=np.int8)
    hit = np.nonzero(rng.random(len(r)) < rate)[0]
    if len(hit) < at_least:
        hit = rng.choice(len(r), size=at_least, replace=False)
    r[hit] = (r[hit] + 1 + rng.integers(0, ncodes - 1, size=len(hit))) % ncodes
    return r


def _mat(match, mismatch):
    m = np.zeros((5, 5), dtype=np.int64)      # (tests/test_saturation.py _mat: N scores 0)
    m[:4, :4] = -mismatch
    for i in range(4):
        m[i, i] = match
    return m.astype(np.int8).reshape(-1).copy()


# ------------------------------------------------------------------------------------------------------------------ 1 length grid

QL_EMU = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65]
QL_GPU = QL_EMU + [255, 256, 257, 447, 448, 449, 624, 625, 639, 640, 641]
TL_GRID = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]      # and one long target: 2 999 columns on the GPU, 299 on the emulator
GRID_ALL = [dict(flag=f, filters=0, filterd=32767 if f == 15 else 0, maskLen=m, score_size=s)
            for f in (0, 2, 15) for m in (0, 15, -1) for s in (1, 2)]
# emulator: three settings in which every flag, every maskLen and both score sizes occur, the long target 299 columns, windows_best at flag 0
# only; the whole cross, 2 999 columns and windows_best at flags 0 and 15 on the GPU
GRID_EMU = [GRID_ALL[k] for k in (5, 8, 13)]      # (flag, maskLen, score_size) = (0, -1, 2), (2, 15, 1), (15, 0, 2)


def _grid_case(qlens, tlong, seed):
    """every query length against every target length; the read from the END of its target in half the pairs where it fits, from the
    start in the other half, else the target plus a random tail; list order permuted"""
    rng = np.random.default_rng(seed)
    tlens = TL_GRID + [tlong]
    targets = [_rand(rng, L) for L in tlens]
    reads, qidx, tidx = [], [], []
    for ql in qlens:
        for ti, tl in enumerate(tlens):
            t = targets[ti]
            if ql <= tl:
                rd = t[tl - ql:].copy() if len(reads) % 2 == 0 else t[:ql].copy()
            else:
                rd = np.concatenate([t, _rand(rng, ql - tl)])
            qidx.append(len(reads)); tidx.append(ti); reads.append(np.ascontiguousarray(rd, dtype=np.int8))
    perm = rng.permutation(len(qidx))
    return reads, targets, np.array(qidx)[perm], np.array(tidx)[perm]


def _length_grid(ctx, qlens, tlong, kw):
    reads, targets, qidx, tidx = _grid_case(qlens, tlong, 8100)
    ref, tms = _three_ways(ctx, reads, targets, qidx, tidx, dna_matrix(2, 2), 5, best=kw["flag"] == 0 or (kw["flag"] == 15 and tlong > 299), **kw)
    fits = [i for i in range(len(qidx)) if len(reads[qidx[i]]) <= len(targets[tidx[i]])]
    assert all(ref[i][0]["score1"] == 2 * len(reads[qidx[i]]) for i in fits)      # the planted reads match end to end
    assert any(ref[i][0]["ref_end1"] == len(targets[tidx[i]]) - 1 for i in fits) and any(ref[i][0]["ref_end1"] < len(targets[tidx[i]]) - 1 for i in fits)
    assert True in tms and ((False in tms) == (641 in qlens))      # 641 residues: answered by the fallback, nothing else is


@pytest.mark.parametrize("kw", GRID_EMU, ids=lambda k: "f%d_m%d_s%d" % (k["flag"], k["maskLen"], k["score_size"]))
def test_emu_length_grid(ectx, kw):
    _length_grid(ectx, QL_EMU, 299, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", GRID_ALL, ids=lambda k: "f%d_m%d_s%d" % (k["flag"], k["maskLen"], k["score_size"]))
def test_gpu_length_grid(gpu_ctx, kw):
    _length_grid(gpu_ctx, QL_GPU, 2999, kw)


# ------------------------------------------------------------------------------------------------------------------ 2 unbalanced halves

def _unbalanced(ctx, T, emu):
    """one row class (R = 1) per call; the T-column target holds its 16-residue read in its last 16 columns.  Two pairs (1, T) in both list
    orders: one job, its halves 1 and T columns long; three pairs (1, 40, T): the long one alone in a job (idle high half, qb = -1);
    2 x 16 + 1 pairs: sixteen jobs of short targets -- a workgroup of 16 chains whose last job is the two 1-column pairs --, then the long one.
    Flags 0 and 15.  Emulator: T = 600, windows_best at flag 0 only"""
    rng = np.random.default_rng(8200 + T)
    long_t = _rand(rng, T)
    short = [_rand(rng, 1), _rand(rng, 40)] + [_rand(rng, int(L)) for L in rng.integers(20, 32, size=2 * NCH_MAX - 2)] + [_rand(rng, 1), _rand(rng, 1)]
    targets = [long_t] + short
    reads = [long_t[T - 16:].copy()] + [(s[-16:].copy() if len(s) >= 16 else np.concatenate([s, _rand(rng, int(rng.integers(8, 15)))])) for s in short]
    assert all(1 <= len(r) <= 16 for r in reads)
    many = list(range(3, 2 * NCH_MAX + 3))      # 30 targets of 20..31 columns, then the two 1-column ones: planner class 0, list order kept
    lists = [[1, 0], [0, 1], [1, 2, 0], many[:7] + [0] + many[7:]]
    for flag in (0, 15):
        for ids in lists:
            ref, tms = _three_ways(ctx, reads, targets, ids, ids, dna_matrix(2, 2), 5, best=not emu or flag == 0, flag=flag,
                                   filterd=32767 if flag else 0)
            k = ids.index(0)
            assert ref[k][0]["score1"] == 32 and ref[k][0]["ref_end1"] == T - 1 and ref[k][0]["read_end1"] == 15
            if flag:
                assert ref[k][0]["ref_begin1"] == T - 16
            assert list(tms) == [True]


def test_emu_unbalanced_halves(ectx):
    _unbalanced(ectx, 600, True)      # (T = 3 000 takes the emulator 15 s: every chain of the workgroup steps through the longest target)


@pytest.mark.gpu
def test_gpu_unbalanced_halves(gpu_ctx):
    _unbalanced(gpu_ctx, 65000, False)


# ------------------------------------------------------------------------------------------------------------------ 3 column limit

def _column_limit(ctx, Rs, emu):
    """targets of 64 999, 65 000 (fast path) and 65 001 columns (fallback); the read's exact copy ends on the LAST column, a copy with two
    substitutions lies at column 100 (maskLen 15: the second best is decided 64 900 columns away); and the same data mirrored.
    Emulator: the boundary itself stays -- R = 1 only, flag 2 only (the fill, then the reverse pass and the traceback), the mirrored
    65 001-column pair left out, windows_best inside the envelope only, and the calls inside the envelope under the 1 MiB scratch budget: one
    chain per workgroup instead of sixteen, most of them idle, that the emulator would step through 65 000 columns (8.5 s per call)"""
    rng = np.random.default_rng(8300)
    reads, targets, qidx, tidx, mirrored = [], [], [], [], []
    for L in (64999, 65000, 65001):
        for R in Rs:
            ql = 16 * R
            t = _rand(rng, L)
            rd = t[L - ql:].copy()
            t[100:100 + ql] = rd
            for p in (100 + ql // 3, 100 + 2 * ql // 3):      # (inside the copy: its best cell stays on its last column)
                t[p] = (t[p] + 1) % 4
            for mirror in (False, True):
                if emu and mirror and L > 65000:
                    continue
                qidx.append(len(reads)); tidx.append(len(targets)); mirrored.append(mirror)
                reads.append(np.ascontiguousarray(rd[::-1] if mirror else rd)); targets.append(np.ascontiguousarray(t[::-1] if mirror else t))
    perm = rng.permutation(len(qidx))
    qidx, tidx = np.array(qidx)[perm], np.array(tidx)[perm]
    for flag in (2,) if emu else (0, 2):
        ref, tms = _three_ways(ctx, reads, targets, qidx, tidx, dna_matrix(2, 2), 5, best="inside" if emu else True,
                               inside_budget=(1 << 20) if emu else 0, flag=flag, maskLen=15)
        for i, (q, t) in enumerate(zip(qidx, tidx)):
            e, ql, L = ref[i][0], len(reads[q]), len(targets[t])
            assert e["score1"] == 2 * ql and e["score2"] > 0 and e["ref_end1"] == (ql - 1 if mirrored[q] else L - 1), (i, e)
            if ql >= 48:      # (a 16-residue read: chance hits in 65 000 random columns rival its mutated copy)
                assert e["ref_end2"] == (L - 101 if mirrored[q] else 100 + ql - 1), (i, e)
        assert set(tms) == {True, False}


def test_emu_column_limit(ectx):
    _column_limit(ectx, (1,), True)


@pytest.mark.gpu
def test_gpu_column_limit(gpu_ctx):
    _column_limit(gpu_ctx, (1, 10, 40), False)


# ------------------------------------------------------------------------------------------------------------------ 4 clipping regimes

def _clip_reads(rng, tcols, R, nreads=4):
    """tests/test_saturation.py's reads for a row class: an exact copy of 16 R residues, one of 16 R - 1, 16 R - 9 with 1 % substitutions, and a
    2 %-substituted copy of 16 R -- each in a target of its own"""
    L = 16 * R
    plan = [(L, 0.0), (L - 9, 0.01), (L - 1, 0.0), (L, 0.02)][:nreads]
    reads, targets = [], []
    for ql, sub in plan:
        t = _rand(rng, tcols)
        off = int(rng.integers(0, tcols - ql + 1))
        reads.append(_subst(t[off:off + ql], rng, sub, at_least=1) if sub else t[off:off + ql].copy()); targets.append(t)
    return reads, targets


def _form(tm):
    name = tm["fill_kernel"]
    assert name.startswith(FAST) and name.endswith(">"), name
    return name[len(FAST):-1].split(",", 1)      # [R, form]


def _clip_case(ctx, rng, R, mm, gaps, flag, tcols, nreads, best):
    """-> the form name the host chose, None outside the envelope (mm = 50 must leave k_fillpairs: _three_ways asserts the path)"""
    reads, targets = _clip_reads(rng, tcols, R, nreads)
    ids = rng.permutation(len(reads))
    ref, tms = _three_ways(ctx, reads, targets, ids, ids, _mat(mm, 11), 5, best=best, gapO=gaps[0], gapE=gaps[1], flag=flag)
    assert ref[list(ids).index(0)][0]["score1"] == 16 * R * mm      # the top of the row class' range is reached
    assert list(tms) == [mm <= 49]
    if mm > 49:
        return None
    r, form = _form(tms[True])
    assert int(r) == R
    return form


def _protein_clipped(ctx, lengths, tcols, emu):
    """min(3 x BLOSUM50, 49) (its largest entry is 45), gaps 30 / 6, homologous reads (10 % substitutions); one row class per call -> the form
    names.  Emulator: one read of 624 residues at flag 0 and one of 625 at flag 2, no windows_best"""
    rng = np.random.default_rng(8450)
    mat = np.minimum(blosum50().astype(np.int64) * 3, 49).astype(np.int8)
    assert 40 < int(mat.max()) <= 49
    forms = set()
    by_R = {}
    for L in lengths:
        by_R.setdefault(-(-L // 16), []).append(L)
    for R, ls in sorted(by_R.items()):
        targets = [_rand(rng, tcols, 20) for _ in ls]
        reads = [_subst(t[7:7 + L], rng, 0.1, ncodes=20) for t, L in zip(targets, ls)]
        ids = np.arange(len(ls))
        for flag in ((0,) if R & 1 else (2,)) if emu else (0, 2):
            ref, tms = _three_ways(ctx, reads, targets, ids, ids, mat, 24, best=not emu and flag == 0, ncodes=20, gapO=30, gapE=6, flag=flag)
            assert all(e["score1"] > 2048 for e, _ in ref) and list(tms) == [True]
            r, form = _form(tms[True])
            assert int(r) == R
            forms.add(form)
    return forms


# the issue's set: R 38..40 x max(mat) 46..50 x gaps 11/3 and 7/2 x flags 0 and 2.  Emulator: R = 40 at mm 46 / 49 / 50 with both gap pairs and
# both flags between them, and one case each of R = 38 and 39 (two reads per case, windows_best at flag 0 only)
GPU_CLIP = [(R, mm, gaps, flag) for R in (38, 39, 40) for mm in (46, 47, 48, 49, 50) for gaps in ((11, 3), (7, 2)) for flag in (0, 2)]
EMU_CLIP = [(40, 46, (11, 3), 0), (40, 49, (7, 2), 2), (40, 50, (11, 3), 2), (39, 49, (7, 2), 0), (38, 47, (11, 3), 2)]
# beyond it: with gaps 30/6 the range limit of the frame form (ssw_frame_params: top + base + (K + 18) gapE < 31744, K >= 64) falls inside
# R 38..40 at max(mat) 49, so that the library without hooks stands on both sides of it
LIMIT_CLIP = [(R, 49, (30, 6), flag) for R in (38, 39, 40) for flag in (0, 2)]
EMU_LIMIT_CLIP = [(39, 49, (30, 6), 2), (40, 49, (30, 6), 0)]


def _clipping(ctx, emu):
    rng = np.random.default_rng(8400)
    forms = set()
    for R, mm, gaps, flag in (EMU_CLIP + EMU_LIMIT_CLIP) if emu else (GPU_CLIP + LIMIT_CLIP):
        f = _clip_case(ctx, rng, R, mm, gaps, flag, 660 if emu else 2600, 2 if emu else 4, best=gaps == (11, 3) and (flag == 0 or not emu))
        assert (f is None) == (mm == 50)
        if f:
            forms.add(f)
    forms |= _protein_clipped(ctx, (624, 625) if emu else (500, 560, 608, 624, 625, 633, 640), 660 if emu else 1500, emu)
    assert forms == {"frame", "int16+max3"}, forms      # both forms of the kernel ran, by the name the host reports


def _clipping_hooks(ctx, monkeypatch, emu):
    """R = 40 at mm 46 and 49 with the frame renormalised every 16 / 64 steps and with the plain int16 form forced (hooks library; the
    emulator library has the hooks too).  Emulator: mm 46 under K = 16, mm 49 under K = 64, both under the forced int16 form"""
    rng = np.random.default_rng(8460)
    forms = set()
    for env in ({"SSW_GPU_FRAME_K": "16"}, {"SSW_GPU_FRAME_K": "64"}, {"SSW_GPU_DB_FORM": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for mm in (46, 49):
                if emu and env.get("SSW_GPU_FRAME_K") == ("64" if mm == 46 else "16"):
                    continue      # emulator: one period per matrix
                f = _clip_case(ctx, rng, 40, mm, (11, 3) if mm == 46 else (7, 2), 2 if mm == 46 else 0, 660 if emu else 2600, 2 if emu else 4, best=False)
                if "SSW_GPU_DB_FORM" in env:
                    assert f == "int16+max3"
                forms.add(f)
    assert forms == {"frame", "int16+max3"}, forms


def test_emu_clipping_regimes(ectx):
    _clipping(ectx, True)


def test_emu_clipping_regimes_forced_forms(ectx, monkeypatch):
    _clipping_hooks(ectx, monkeypatch, True)


@pytest.mark.gpu
def test_gpu_clipping_regimes(gpu_ctx):
    _clipping(gpu_ctx, False)


@pytest.mark.gpu
def test_gpu_clipping_regimes_forced_forms(gpu_hctx, monkeypatch):
    _clipping_hooks(gpu_hctx, monkeypatch, False)


# ------------------------------------------------------------------------------------------------------------------ 5 byte / word decision

def _byte_word_decision(ctx, tcols, emu):
    """match 1, mismatch x: bias = x; exact copies of 255 - x - 1, 255 - x and 255 - x + 1 residues score their length.  score_size 0: NULL
    (status 1) from 255 - x on; the n_word / n_byte counts are asserted by _three_ways from the reference's scores (and spelt out here).
    Emulator: windows_best for x = 1 only"""
    rng = np.random.default_rng(8500)
    for x in (1, 3):
        lens = [255 - x - 1, 255 - x, 255 - x + 1]
        targets = [_rand(rng, tcols) for _ in lens]
        reads = [t[11 + k:11 + k + L].copy() for k, (t, L) in enumerate(zip(targets, lens))]
        ids = [2, 0, 1]
        for ss in (0, 1, 2):
            ref, tms = _three_ways(ctx, reads, targets, ids, ids, dna_matrix(1, x), 5, best=not emu or x == 1, flag=0, score_size=ss)
            for k, i in enumerate(ids):
                if ss == 0 and lens[i] >= 255 - x:
                    assert ref[k][0] is None
                else:
                    assert ref[k][0]["score1"] == lens[i]
            assert list(tms) == [True]
            assert (tms[True]["n_word"], tms[True]["n_byte"]) == {0: (0, 1), 1: (3, 0), 2: (2, 1)}[ss]


def _padded_second_best(ctx, emu):
    """word semantics (match 2: an exact copy of 256 residues and more overflows 8 bits); reads of 256 + {0, 1, 8, 9, 15} residues, len & 15
    = 0, 1, 8, 9, 15: for 1..8 the reference's second best comes from the padded segment length (the kernel's other tap).  Every target holds
    the exact copy and, behind it and outside the mask, a second copy with 5 % substitutions.  maskLen -1 and 15, flags 0 and 2.
    Emulator: (maskLen 15, flag 2) left out, windows_best at (maskLen -1, flag 0) only"""
    rng = np.random.default_rng(8550)
    reads, targets = [], []
    for d in (0, 1, 8, 9, 15):
        rd = _rand(rng, 256 + d)
        targets.append(np.concatenate([_rand(rng, 40 + d), rd, _rand(rng, 30), _subst(rd, rng, 0.05, at_least=5), _rand(rng, 20)]))
        reads.append(rd)
    ids = [3, 1, 4, 0, 2]
    for maskLen, flag in ((-1, 0), (15, 0), (-1, 2), (15, 2))[:3 if emu else 4]:
        ref, tms = _three_ways(ctx, reads, targets, ids, ids, dna_matrix(2, 2), 5, best=not emu or (flag == 0 and maskLen < 0), flag=flag, maskLen=maskLen)
        for k, i in enumerate(ids):
            e = ref[k][0]
            assert e["score1"] == 2 * len(reads[i]) and e["score2"] > 0, (i, e)
            if maskLen < 0:      # (maskLen 15: the shoulder of the best alignment, 15 columns behind its end, is the reference's second best)
                assert e["ref_end2"] > e["ref_end1"] + len(reads[i]) // 2, (i, e)
        assert list(tms) == [True] and tms[True]["n_word"] == 5


def test_emu_byte_word_decision(ectx):
    _byte_word_decision(ectx, 300, True)


def test_emu_padded_second_best(ectx):
    _padded_second_best(ectx, True)


@pytest.mark.gpu
def test_gpu_byte_word_decision(gpu_ctx):
    _byte_word_decision(gpu_ctx, 2000, False)


@pytest.mark.gpu
def test_gpu_padded_second_best(gpu_ctx):
    _padded_second_best(gpu_ctx, False)


# ------------------------------------------------------------------------------------------------------------------ 6 alphabet gate

# (n, query length) -> fast path?  n x ceil(R / 4) x 256 <= 65535 with R = ceil(len / 16), n <= 32 (include/ssw_gpu.h):
# 25 x 10 x 256 = 64 000; 26 x 9 x 256 = 59 904 (576) / 26 x 10 x 256 = 66 560 (577); 32 x 7 x 256 = 57 344 (448) / 32 x 8 x 256 = 65 536 (449)
GATE = {(24, 640): True, (25, 640): True, (26, 576): True, (26, 577): False, (32, 448): True, (32, 449): False, (33, 448): False, (33, 16): False}


def _alphabet_gate(ctx, ns, tcols):
    rng = np.random.default_rng(8600)
    for n in ns:
        mat = rng.integers(-12, 13, size=(n, n)).astype(np.int8)
        np.fill_diagonal(mat, rng.integers(1, 13, size=n))
        mat = np.ascontiguousarray(mat.reshape(-1))
        lens = [L for (m, L) in GATE if m == n]
        targets = [_rand(rng, tcols - 13 * k, n) for k in range(len(lens))]
        reads = [_subst(t[5:5 + L], rng, 0.05, ncodes=n) for t, L in zip(targets, lens)]
        ids = np.arange(len(lens))[::-1]
        for L in lens:
            assert in_envelope(L, tcols, n, mat, 10, 2) == GATE[(n, L)]
        for flag in (0, 2):
            ref, tms = _three_ways(ctx, reads, targets, ids, ids, mat, n, best=flag == 0, gapO=10, gapE=2, flag=flag)
            assert all(e is not None and e["score1"] > 0 for e, _ in ref)
            assert set(tms) == set(GATE[(n, L)] for L in lens)


def test_emu_alphabet_gate(ectx):
    _alphabet_gate(ectx, (32,), 600)


@pytest.mark.gpu
def test_gpu_alphabet_gate(gpu_ctx):
    _alphabet_gate(gpu_ctx, (24, 25, 26, 32, 33), 1500)


# ------------------------------------------------------------------------------------------------------------------ 7 ties

def _ties_case():
    """homopolymer, period-2 and period-3 reads against like targets (the period-3 target with one foreign residue in the middle): the
    maximum is reached in many cells, and the tie rules alone decide ref_end1, read_end1 and ref_end2 (emulator: windows_best at flag 0 only)"""
    reads, targets, qidx, tidx = [], [], [], []
    for period in (1, 2, 3):
        unit = np.arange(period, dtype=np.int8)
        r0, t0 = len(reads), len(targets)
        for ql in (1, 16, 17, 40, 150):
            reads.append(np.resize(unit, ql).astype(np.int8))
        for tl in (16, 64, 100, 333):
            t = np.resize(unit, tl).astype(np.int8)
            if period == 3:
                t[tl // 2] = 3
            targets.append(t)
        for q in range(5):
            for t in range(4):
                qidx.append(r0 + q); tidx.append(t0 + t)
    # beyond the issue's list: the same maximum in two different columns AND rows, held by different lanes of the chain -- a read of two runs
    # against a target that holds half of each run in the other order (the first COLUMN wins, whichever lane comes first)
    for run in (10, 24):
        a, c = np.zeros(2 * run, dtype=np.int8), np.ones(2 * run, dtype=np.int8)
        r0, t0 = len(reads), len(targets)
        reads += [np.concatenate([a, c]), np.concatenate([c, a])]
        targets += [np.concatenate([c[:run], [2], a[:run]]).astype(np.int8), np.concatenate([a[:run], [2, 2, 2], c[:run]]).astype(np.int8)]
        for q in range(2):
            for t in range(2):
                qidx.append(r0 + q); tidx.append(t0 + t)
    perm = np.random.default_rng(8700).permutation(len(qidx))
    return reads, targets, np.array(qidx)[perm], np.array(tidx)[perm]


def _ties(ctx, flag, emu):
    reads, targets, qidx, tidx = _ties_case()
    ref, tms = _three_ways(ctx, reads, targets, qidx, tidx, dna_matrix(2, 2), 5, best=flag == 0 or (flag == 15 and not emu), flag=flag, filters=0,
                           filterd=32767 if flag == 15 else 0)
    # the first column that holds the maximum wins: a homopolymer read inside a longer homopolymer target ends at column len - 1
    for i, (q, t) in enumerate(zip(qidx, tidx)):
        if q < 5 and len(reads[q]) <= len(targets[t]):
            assert ref[i][0]["score1"] == 2 * len(reads[q]) and ref[i][0]["ref_end1"] == len(reads[q]) - 1
    # (reads 15.., targets 12..: the pairs whose target holds the runs in the OTHER order tie; the reference ends on the target's first run)
    two_runs = [ref[i][0] for i, (q, t) in enumerate(zip(qidx, tidx)) if q >= 15 and (q - 15) % 2 == (t - 12) % 2]
    assert len(two_runs) == 4 and all(e["score1"] == 2 * (e["ref_end1"] + 1) and e["score1"] in (20, 48) for e in two_runs)
    assert any(e["score2"] > 0 for e, _ in ref) and list(tms) == [True]


@pytest.mark.parametrize("flag", [0, 2, 15])
def test_emu_ties(ectx, flag):
    _ties(ectx, flag, True)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 2, 15])
def test_gpu_ties(gpu_ctx, flag):
    _ties(gpu_ctx, flag, False)
