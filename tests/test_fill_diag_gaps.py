"""k_fill8 opens gaps from the diagonal candidate only where the scoring allows it (DESIGN.md "Gaps from the diagonal"):

    xc = x - (gapO - gapE)      h = max3(x, E, F)      E' = max3(xc, E, floor)      F' = max3(xc, F, floor)

instead of t = h - (gapO - gapE) in E' and F'.  That drops a vertical gap directly next to a horizontal one.  H is what it was when
gapO > gapE, -min(mat) <= 2 gapE and the target has no null column; E and F may come out lower.

The gate, in plain numpy: the full recurrence against the restricted one on random matrices on both sides of the gate, the boundary
-min(mat) = 2 gapE and 2 gapE + 1 included, and one committed case beyond the gate (1/-9 with gaps 2/1) where H differs.

What "an insertion directly next to a deletion" can mean under the gate.  The exchange argument is strict: a path with the adjacency scores
at least gapO - gapE LESS than the path that replaces it, so under the gate no best alignment has the adjacency and none ties with one that
has it -- such a read cannot be built.  What can be built, and is: reads that CARRY an insertion directly next to a deletion against the
target (g_ins foreign residues in the place of g_del residues of the target).  Around such a place the full recurrence's E and F are fed by
an H that is itself E or F -- the prefix path with the adjacency -- and the plain DP below checks per read that no case is vacuous: H is the
same everywhere, and there are cells where the full E or F is positive and HIGHER than the restricted one (the old form's register holds
another value: the restricted form reaches its H by another path) and cells where the prefix path with the adjacency TIES with one without
(the full E or F equals H - gapO of a cell whose H is E or F alone, and the restricted value is the same).  The places stand in mid-tile
and at a tile's first column, over the class seam and over the position seam of the row frame.

The calls (targets of 6 400 columns, one to four reads per call, as tests/test_fill_rowframe.py): every instance R8 = 1 .. 23 at one length
with flags 0, 1 and 2, N residues in every third target and calls of one read (dead chain B); the adjacency reads; tests/test_fill_rowframe.py's
second copies that end in the padded rows or are cut off in a row of each class (the plain DP checks that Ftop differs between the forms);
the three scorings of that file with SSW_GPU_FRAME_K 16 and 64; every record against the reference.  Under SSW_GPU_FILL_DG=0 the hooks
library runs the old form and its records are byte-identical.  Scorings beyond the gate (1/-4/6/1, the matrix with an entry of -100) and a
target with a residue code outside the alphabet run the old form by name.  At the planner's last match score the new form runs: it needs no
more of the frame's range than the old one (x - (gapO - gapE) >= 4 gapE + 8 at the old base: ssw_host.c, fill8_diag_gaps), so there is no
score at which only the old form fits, and the next match score falls to the int16 form as before.  Under the emulator pk_max3_fr asserts
the range of every operand, fr_add_pair its carry and fr_sub_pair / fr_sub_one that no borrow crosses a half or a word."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_batch, make_reads
from sswutil import dna_matrix, random_ref
from test_fill_half_flush import _halo
from test_fill_rowframe import (BOUND_SCORINGS, IDS, LENGTHS, SCORINGS, T_LEN, TILE, TILES, _cm_call, bound_match, calls_colmax, cm_cases)

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")
NEG = -10 ** 6


def _r8(L):
    return (L + 7) // 8


# ---- the two recurrences, cell by cell --------------------------------------------------------------------------------------------------------

def plain_dp(read, target, mat, n, gO, gE, rows, diag_only):
    """Smith-Waterman with affine gaps over `rows` rows (the read, then zero-score rows).  diag_only: gaps open from the diagonal candidate
    x = H(i-1, j-1) + s alone.  Returns H, E, F as [rows + 1][columns + 1] arrays: E(i, j) the horizontal gap that ENTERS cell (i, j), F(i, j) the
    vertical one; row 0 and column 0 are the boundary."""
    L, m = len(read), len(target)
    H = np.zeros((rows + 1, m + 1), dtype=np.int64)
    X = np.full((rows + 1, m + 1), NEG, dtype=np.int64)
    E = np.full((rows + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((rows + 1, m + 1), NEG, dtype=np.int64)
    for j in range(1, m + 1):
        b = int(target[j - 1])
        for i in range(1, rows + 1):
            s = int(mat[b * n + int(read[i - 1])]) if i <= L else 0
            src_e = X[i, j - 1] if diag_only else H[i, j - 1]
            src_f = X[i - 1, j] if diag_only else H[i - 1, j]
            E[i, j] = max(E[i, j - 1] - gE, src_e - gO)
            F[i, j] = max(F[i - 1, j] - gE, src_f - gO)
            X[i, j] = H[i - 1, j - 1] + s
            H[i, j] = max(0, X[i, j], E[i, j], F[i, j])
    return H, E, F


def adjacency_cells(read, target, mat, n, gO, gE, rows):
    """(H equal everywhere, cells where the full E or F is positive and higher than the restricted one, cells where a prefix path with the
    adjacency ties with one without)"""
    Hf, Ef, Ff = plain_dp(read, target, mat, n, gO, gE, rows, False)
    Hr, Er, Fr = plain_dp(read, target, mat, n, gO, gE, rows, True)
    strict = int(np.sum((Ef > Er) & (Ef > 0)) + np.sum((Ff > Fr) & (Ff > 0)))
    # H of the source cell is E or F alone (above its diagonal candidate and zero), the gap opened from it is the full value, and the restricted agrees
    only_e = (Hf == Ff) & (Ff > Ef) & (Hf > 0)      # the source's H comes from its vertical gap: E opened from it is F -> E
    only_f = (Hf == Ef) & (Ef > Ff) & (Hf > 0)
    Xf = np.full_like(Hf, NEG); Xf[1:, 1:] = Hf[:-1, :-1]
    L = len(read)
    for j in range(1, Hf.shape[1]):
        for i in range(1, rows + 1):
            Xf[i, j] += int(mat[int(target[j - 1]) * n + int(read[i - 1])]) if i <= L else 0
    only_e &= Hf > Xf; only_f &= Hf > Xf
    tie = int(np.sum(only_e[:, :-1] & (Ef[:, 1:] == Hf[:, :-1] - gO) & (Er[:, 1:] == Ef[:, 1:]) & (Ef[:, 1:] > 0)) +
              np.sum(only_f[:-1, :] & (Ff[1:, :] == Hf[:-1, :] - gO) & (Fr[1:, :] == Ff[1:, :]) & (Ff[1:, :] > 0)))
    return bool(np.array_equal(Hf, Hr)), strict, tie


def _random_matrix(rng, lo, hi):
    m = rng.integers(lo, hi + 1, size=(5, 5)).astype(np.int8)
    m = np.minimum(m, m.T)
    m[np.diag_indices(5)] = rng.integers(1, hi + 1, size=5)
    return m.reshape(-1)


GATE_CASES = [(3, 1, 2), (5, 2, 4), (10, 4, 8), (2, 1, 2), (6, 1, 1), (4, 3, 6)]      # gapO, gapE, -min(mat): the last entry at most 2 gapE


@pytest.mark.parametrize("gO,gE,low", GATE_CASES)
def test_restricted_recurrence_is_exact_under_the_gate(gO, gE, low):
    """random matrices whose smallest entry is exactly -low (low <= 2 gapE, with the boundary low = 2 gapE among the cases), random
    sequences with planted copies: H of the two recurrences is the same in every cell; E and F are lower somewhere (the forms do differ)"""
    assert low <= 2 * gE and gO > gE
    rng = np.random.default_rng(9100 + 100 * gO + gE)
    lower = 0
    for trial in range(40):
        mat = _random_matrix(rng, -low, 6)
        mat[rng.integers(0, 5) * 5 + rng.integers(0, 5)] = -low
        target = rng.integers(0, 5, size=26, dtype=np.int8)
        read = np.concatenate([target[3:9], rng.integers(0, 5, size=2, dtype=np.int8), target[10:19]]).astype(np.int8)
        Hf, Ef, Ff = plain_dp(read, target, mat, 5, gO, gE, len(read) + 3, False)
        Hr, Er, Fr = plain_dp(read, target, mat, 5, gO, gE, len(read) + 3, True)
        assert np.array_equal(Hf, Hr), (trial, mat.reshape(5, 5))
        assert np.all(Er <= Ef) and np.all(Fr <= Ff)
        lower += int(np.sum(Er < Ef) + np.sum(Fr < Ff))
    assert lower > 0


@pytest.mark.parametrize("gE", [1, 2, 3])
def test_one_past_the_boundary_breaks_it(gE):
    """-min(mat) = 2 gapE + 1 with gapO = gapE + 1: k substituted residues in a row cost k (2 gapE + 1) as mismatches and 2 k gapE + 2 as a
    vertical gap of k next to a horizontal one -- from k = 3 on the adjacency wins by k - 2, and H of the restricted recurrence is lower"""
    low, gO = 2 * gE + 1, gE + 1
    mat = dna_matrix(6, low)
    left = np.array([0, 1, 2, 3, 0, 2, 1, 3, 2], dtype=np.int8)
    right = np.array([2, 3, 1, 0, 3, 2, 0, 1, 3], dtype=np.int8)
    for k in range(1, 5):
        target = np.concatenate([left, np.zeros(k, dtype=np.int8), right])
        read = np.concatenate([left, np.ones(k, dtype=np.int8), right])
        Hf, _, _ = plain_dp(read, target, mat, 5, gO, gE, len(read), False)
        Hr, _, _ = plain_dp(read, target, mat, 5, gO, gE, len(read), True)
        assert np.all(Hr <= Hf)
        assert Hf.max() == 18 * 6 - min(k * low, 2 * k * gE + 2)
        assert (Hr.max() == Hf.max()) == (k < 3), k


def test_beyond_the_gate_h_differs():
    """1/-9 with gaps 2/1: one substituted residue between two flanks of eight is aligned as an insertion next to a deletion (-4) by the full
    recurrence and cannot be by the restricted one, whose best score is lower -- the gate is not decoration"""
    mat = dna_matrix(1, 9)
    target = np.array([0, 1, 2, 3, 0, 2, 1, 3, 0, 3, 1, 0, 2, 2, 3, 1, 0], dtype=np.int8)
    read = target.copy(); read[8] = 1
    Hf, _, _ = plain_dp(read, target, mat, 5, 2, 1, len(read), False)
    Hr, _, _ = plain_dp(read, target, mat, 5, 2, 1, len(read), True)
    assert Hf.max() == 8 - 4 + 8 and Hr.max() < Hf.max() and np.all(Hr <= Hf)
    assert 9 > 2 * 1      # (beyond the gate)


# ---- the calls: (name, reads, target, flag) ----------------------------------------------------------------------------------------------

def calls_instances(si):
    rng = np.random.default_rng(6200 + si)
    calls = []
    for j, L in enumerate([8 * r - (3 * r) % 8 for r in range(1, 24, 2)]):      # one length per instance, 8 R8 - 7 .. 8 R8
        target = random_ref(T_LEN, 6300 + 10 * j + si, 4)
        if j % 3 == 0:
            target[np.arange(57, T_LEN, 211)] = 4      # N residues
        reads = make_reads(rng, target, 1 + j % 4, [L], 4, frac_random=0.0)
        calls.append(("instance R8 %d, %d bp" % (_r8(L), L), reads, target, j % 3))
    return calls


ADJ = ((1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (1, 3))      # (inserted residues, deleted residues) side by side


def adj_cases(R8):
    """(row of the read at which the run stands, inserted, deleted, seam) in position 3 of the chain: the run's first row is the class-0 row of the
    seam, so that the vertical gap crosses it"""
    p0 = 3 * R8
    out = []
    for k, (gi, gd) in enumerate(ADJ):
        up = k % 2 if gi >= 2 else 0      # (a run of one row has to stand in the seam's second row)
        out.append((p0 + 4 - up, gi, gd, "class"))
        out.append((p0 + R8 - up, gi, gd, "position"))
    return out


def _adjacent(target, X, L, a, gi, gd):
    """rows 0 .. a - 1 are target[X : X + a], then gi residues that fit neither the deleted ones nor what follows, then the target from X + a + gd on"""
    seg = target[X:X + L - gi + gd]
    avoid = {int(x) for x in seg[a:a + gd + 1]}
    free = [c for c in range(4) if c not in avoid] or [(int(seg[a]) + 1) % 4]
    run = np.array([free[k % len(free)] for k in range(gi)], dtype=np.int8)
    return np.concatenate([seg[:a], run, seg[a + gd:]]).astype(np.int8)


def adj_calls(si):
    """(cases, reads, target, first columns): read j of a call has its run in mid-tile (j even) or at a tile's first column (j odd)"""
    out = []
    for R8, L in LENGTHS.items():
        cases = adj_cases(R8)
        k = shape = 0
        while k < len(cases):
            nr = min(2 + shape % 3, len(cases) - k); shape += 1
            target = random_ref(T_LEN, 6600 + 100 * R8 + k + 1000 * si, 4)
            reads, places = [], []
            for j in range(nr):
                a, gi, gd, _ = cases[k + j]
                col = TILE * TILES[j] + (0 if (j + shape) % 2 else 23 + 5 * j)      # the column of the run
                reads.append(_adjacent(target, col - a, L, a, gi, gd)); places.append(col - a)
            out.append((cases[k:k + nr], reads, target, places))
            k += nr
    return out


def calls_adjacent(si):
    return [("adjacent R8 %d: %s" % (_r8(len(reads[0])), cases), reads, target, 1 + i % 2) for i, (cases, reads, target, _) in enumerate(adj_calls(si))]


def build_calls(si):
    return calls_instances(si) + calls_adjacent(si) + calls_colmax(si)


# ---- the cases are what they claim to be (CPU) --------------------------------------------------------------------------------------------

def test_shapes_cover_every_instance_seam_and_place():
    for si in range(len(SCORINGS)):
        inst = calls_instances(si)
        assert [_r8(len(r[0])) for _, r, _, _ in inst] == list(range(1, 24, 2))
        assert all(1 <= len(r[0]) % 16 <= 8 for _, r, _, _ in inst)
        assert {len(r) for _, r, _, _ in inst} == {1, 2, 3, 4} and {f for _, _, _, f in inst} == {0, 1, 2}
        assert any((t == 4).any() for _, _, t, _ in inst)
        seen = set()
        for cases, reads, target, places in adj_calls(si):
            for (a, gi, gd, seam), rd, X in zip(cases, reads, places):
                R8 = _r8(len(rd))
                assert len(rd) == LENGTHS[R8]
                rows = range(a - 1, a + gi)      # the vertical gap is born in row a - 1 and runs to row a + gi - 1
                if seam == "class":
                    assert any(x % R8 % 4 == 3 and x + 1 in rows and (x + 1) % R8 for x in rows), (a, gi, R8)
                else:
                    assert any((x + 1) % R8 == 0 and x + 1 in rows for x in rows), (a, gi, R8)
                col = X + a
                seen.add((R8, seam, "first column" if col % TILE == 0 else "mid-tile"))
                assert col % TILE == 0 or 8 < col % TILE < TILE - 8
        assert seen == {(R8, s, p) for R8 in LENGTHS for s in ("class", "position") for p in ("first column", "mid-tile")}, seen


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_no_adjacency_case_is_vacuous(si):
    """the plain DP over the columns around each run: H is the same with the adjacency forbidden, and the full recurrence's E / F are fed through
    the adjacency -- strictly higher in some cells, tied with an adjacency-free prefix in others (both kinds in every scoring, one at least per read)"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    assert gO > gE and mism <= 2 * gE
    strict_all = tie_all = 0
    for cases, reads, target, places in adj_calls(si):
        for (a, gi, gd, seam), rd, X in zip(cases, reads, places):
            lo, hi = max(0, X + a - 24), min(T_LEN, X + a + gd + 24)
            r0 = max(0, a - 24)
            same, strict, tie = adjacency_cells(rd[r0:a + gi + 24], target[lo:hi], mat, 5, gO, gE, len(rd[r0:a + gi + 24]))
            assert same, (a, gi, gd, seam)
            assert strict + tie > 0, ("vacuous case: the adjacency feeds no E or F", a, gi, gd, seam)
            strict_all += strict; tie_all += tie
    assert strict_all > 0 and tie_all > 0, (strict_all, tie_all)


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_ftop_differs_between_the_forms(si):
    """second copies that end in row P8 - 1 (tests/test_fill_rowframe.py's): the F that enters the padded rows is lower in the restricted
    recurrence in some column behind the copy, H of row P8 - 1 and every column maximum are the same"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    lower = 0
    for idx, (L, m) in enumerate(cm_cases(si)):
        if m:
            continue
        reads, target, ends = _cm_call(si, idx, L, m, 1 + idx % 4)
        P8, P16 = (L + 7) // 8 * 8, (L + 15) // 16 * 16
        rd, X = reads[0], ends[0]
        lo, hi = max(0, X + 1 - L - 12), min(T_LEN, X + 12)
        Hf, _, Ff = plain_dp(rd, target[lo:hi], mat, 5, gO, gE, P16, False)
        Hr, _, Fr = plain_dp(rd, target[lo:hi], mat, 5, gO, gE, P16, True)
        assert np.array_equal(Hf, Hr)
        lower += int(np.sum((Fr[P8 + 1] < Ff[P8 + 1]) & (Ff[P8 + 1] > 0)))
    assert lower > 0


# ---- running the calls ----------------------------------------------------------------------------------------------------------------------

def _name(R8, dg):
    return "k_fill8<%d,frame>%s" % (R8, " dg" if dg and R8 not in (9, 17) else "")      # (the two instances that keep the old form)


def _run(ctx, calls, mat, gO, gE, dg, check=True, what=""):
    recs = []
    for name, reads, target, flag in calls:
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        R8 = _r8(len(reads[0]))
        assert tm["fill_kernel"] == _name(R8, dg), (tm["fill_kernel"], name, what)
        assert tm["fill_ops_per_row"] == 6.5 if R8 == 9 else 5.0 <= tm["fill_ops_per_row"] < 6.5, (tm["fill_ops_per_row"], name)
        recs.append(res.tobytes() + np.asarray(cig).tobytes())
        if check:
            bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, flag, 0, 0, -1, 2)
            assert not bad, "%s %s: " % (what, name) + "\n".join(bad)
    return recs


def run_calls(ctx, si, dg=True, check=True):
    """every call of scoring si through ctx (the new form by name unless dg is off), every record against the reference; returns the records"""
    match, mism, gO, gE = SCORINGS[si]
    return _run(ctx, build_calls(si), dna_matrix(match, mism), gO, gE, dg, check, IDS[si])


def _minus100():
    m = dna_matrix(2, 2)
    m[0 * 5 + 1] = m[1 * 5 + 0] = -100
    return m


def run_gate_off(ctx):
    """beyond the gate the old form runs, by name, and matches the reference: 1/-4/6/1 and the matrix with an entry of -100 (gaps 3/1)"""
    calls = [c for c in calls_instances(0) if _r8(len(c[1][0])) in (5, 19, 23)] + calls_adjacent(0)[:2]
    _run(ctx, calls, dna_matrix(1, 4), 6, 1, False, True, "1/-4/6/1")
    _run(ctx, calls, _minus100(), 3, 1, False, True, "minus100")


def run_bound(ctx, bi, frame_k):
    """perfect 184-bp copies at the planner's last match score: the new form still runs (it fits wherever the old one does), one score on the
    bucket takes the int16 form"""
    mism, gO, gE = BOUND_SCORINGS[bi]
    top = bound_match(bi, frame_k)
    assert mism <= 2 * gE
    target = random_ref(T_LEN, 6900 + bi, 4)
    reads = [target[3000:3184].copy(), target[70:254].copy(), target[5000:5184].copy()]
    for match, frame in ((top, True), (top + 1, False)):
        mat = dna_matrix(match, mism)
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, 1, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        assert tm["fill_kernel"] == ("k_fill8<23,frame> dg" if frame else "k_fill<12,int16>"), (tm["fill_kernel"], match, BOUND_SCORINGS[bi])
        assert int(res[0, 0]["score1"]) == 184 * match
        bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, 1, 0, 0, -1, 2)
        assert not bad, "bound %s match %d: " % (BOUND_SCORINGS[bi], match) + "\n".join(bad)


def run_null_column(ctx):
    """a residue code outside the alphabet makes a null column, whose cells have no diagonal: such a target keeps the old form.  (No input of
    the reference, which would read its profile out of bounds: the caller compares the records with the 16-lane kernel's)"""
    rng = np.random.default_rng(6950)
    target = random_ref(T_LEN, 6951, 4)
    reads = make_reads(rng, target, 3, [150], 4, frac_random=0.0)
    target[1700] = 9
    mat = dna_matrix(2, 2)
    return _run(ctx, [("null column", reads, target, 1)], mat, 3, 1, False, False)


_EMU_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill_diag_gaps as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
si = int(os.environ["DIAGGAP_SI"])
n = len(m.run_calls(ctx, si))
if si < 2:
    m.run_bound(ctx, si, int(os.environ["SSW_GPU_FRAME_K"]))
else:
    m.run_gate_off(ctx)
    m.run_null_column(ctx)
ctx.close()
print("ok", n)
'''


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_diag_gaps_on_the_emulator(emu_lib_path, K, si):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K, DIAGGAP_SI=str(si))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_diag_gaps_hooks_library_gpu(gpu_hctx, monkeypatch, si, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)      # (hooks of libssw_hooks.so, read at every call)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    recs = run_calls(gpu_hctx, si)
    monkeypatch.setenv("SSW_GPU_FILL_DG", "0")
    assert run_calls(gpu_hctx, si, dg=False, check=False) == recs      # the old form, by name: byte-identical records


@pytest.mark.gpu
@pytest.mark.parametrize("K", ["16", "64"])
def test_gate_off_and_null_column_hooks_library_gpu(gpu_hctx, monkeypatch, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    run_gate_off(gpu_hctx)
    recs = run_null_column(gpu_hctx)
    monkeypatch.setenv("SSW_GPU_FILL_HALF", "0")
    rng = np.random.default_rng(6950)
    target = random_ref(T_LEN, 6951, 4)
    reads = make_reads(rng, target, 3, [150], 4, frac_random=0.0)
    target[1700] = 9
    Q = gpu_hctx.upload(reads); T = gpu_hctx.upload([target])
    try:
        res, cig = gpu_hctx.align_batch(Q, T, dna_matrix(2, 2), 5, 3, 1, 1, 0, 0, -1, 2)
    finally:
        Q.free(); T.free()
    assert gpu_hctx.timing()["fill_kernel"].startswith("k_fill<")
    assert [res.tobytes() + np.asarray(cig).tobytes()] == recs


@pytest.mark.gpu
@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("K", ["16", "64"])
def test_bound_hooks_library_gpu(gpu_hctx, monkeypatch, bi, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    run_bound(gpu_hctx, bi, int(K))


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_diag_gaps_product_library_gpu(gpu_ctx, si):
    run_calls(gpu_ctx, si)
    if si < 2:
        run_bound(gpu_ctx, si, 0)
    else:
        run_gate_off(gpu_ctx)
        run_null_column(gpu_ctx)
