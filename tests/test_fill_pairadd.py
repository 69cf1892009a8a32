"""k_fill8 forms diag + score of rows 2j and 2j + 1 of a position in ONE 64-bit add (fr_add_pair, lanes.h): the profile words of the two rows
are one addend, and a live word of row 2j whose signed sum lo + hi x 65536 is negative borrows 1 from the word of row 2j + 1 when the profile
is built (build_profile8) -- the carry out of bit 31 gives it back at run time.  What can go wrong with that, and the shapes that reach it:

  * every instance: read lengths 8 R8 (the last row of the last position is a row of the read) and 8 R8 - 7 (seven zero-score rows at the end
    of the chain, one of them the upper word of a pair) for R8 = 1, 3, .. 23 -- R8 = 1 has no pair, R8 = 9 keeps its 32-bit adds, every other
    odd R8 ends on a row that is added alone;
  * the borrow: 2/-2/3/1 and 1/-3/5/2, where a class-0 row (profile entry: score - 2 gapE) borrows on every mismatch, and a matrix with one
    entry of -100 at gapE = 1, where lower words outside class 0 borrow too.  The census below computes the words from the profile's formula and fails
    if a scoring has no borrowing word, no borrowing word under a zero-score upper word, or no call with a dead chain: no case is vacuous;
  * dead and null words: calls of one and two reads (one pair: chain B of the workgroup is dead), of three (the second pair has no query B:
    its high halves are zero scores) and of four; target lengths that are no multiple of 16, so that null columns (every word FR_DEAD)
    follow live ones inside a trip, and N residues (score 0) in the target.  Codes outside the alphabet are no input of the reference -- it
    would read its profile out of bounds -- so the null columns are the ones past the target's end;
  * frame seams: reads with a soft-clipped prefix of r residues (tests/test_fill_rowframe.py's construction), whose alignment begins in row
    r, for the rows on both sides of every pair boundary and class-0 row of the first positions, and of the seam between two positions;
  * range: a perfect 184-bp copy at the largest match score the planner admits to the frame form.

Targets of 203 .. 600 columns; the small-call rule cuts them into tiles of 64 columns and more where the halo is shorter than the target
(checked below for the calls that claim it).  Every record is compared with the reference; the hooks library and the emulator renormalise
every 16 and every 64 steps (SSW_GPU_FRAME_K), and the hooks library's records are compared byte for byte with the 16-lane kernel's
(SSW_GPU_FILL_HALF=0).  Under the emulator pk_max3_fr asserts the range of every operand and fr_add_pair that the low word's carry is its
borrow, that is, that the pair add equals the two 32-bit adds of the words before the borrow."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_batch, make_reads
from sswutil import dna_matrix, random_ref
from test_fill_rowframe import BOUND_SCORINGS, _clipped, bound_match

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")


def _matrix(si):
    if si < 2:
        return dna_matrix(*SCORINGS[si][:2])
    m = dna_matrix(2, 2)
    m[0 * 5 + 1] = m[1 * 5 + 0] = -100
    return m


SCORINGS = ((2, 2, 3, 1), (1, 3, 5, 2), (2, 2, 3, 1))      # match, mismatch, gapO, gapE; the third with A x C = -100 (_matrix)
IDS = ["2_2_3_1", "1_3_5_2", "minus100"]
SEAM_LENGTHS = {5: 40, 19: 150}
SEAM_ROWS = {5: list(range(11)), 19: [0, 1, 2, 3, 4, 5, 7, 8, 9, 18, 19, 20, 21, 22, 23]}


def _r8(L):
    return (L + 7) // 8


# ---- the calls: (name, reads, target, flag) ----------------------------------------------------------------------------------------------

def _target(length, seed, with_n):
    t = random_ref(length, seed, 4)
    if with_n:
        t[length // 3] = t[length // 2 + 1] = 4
    return t


def calls_instances(si):
    rng = np.random.default_rng(7100 + si)
    calls = []
    for j, L in enumerate([8 * r for r in range(1, 24, 2)] + [8 * r - 7 for r in range(1, 24, 2)]):
        target = _target(203 + 37 * (j % 8) + (L > 100) * 130, 7200 + 10 * j + si, j % 3 == 0)
        reads = make_reads(rng, target, 1 + (j + j // 12) % 4, [L], 4, frac_random=0.0)
        calls.append(("instance R8 %d, %d bp" % (_r8(L), L), reads, target, j % 3))
    return calls


def calls_seams(si):
    rng = np.random.default_rng(7300 + si)
    calls = []
    for R8, L in SEAM_LENGTHS.items():
        rows = SEAM_ROWS[R8]
        for k in range(0, len(rows), 3):
            T = 333 if L < 100 else 600
            target = _target(T, 7400 + 100 * R8 + k + 1000 * si, False)
            places = ((5 * k + R8) % 16, T // 2 + 3, T - L - 9)      # first 16 columns, mid-target, near the end
            reads = [_clipped(rng, target, X, L, r) for r, X in zip(rows[k:k + 3], places)]
            calls.append(("seams R8 %d, alignments from rows %s" % (R8, rows[k:k + 3]), reads, target, 1))
    return calls


def build_calls(si):
    return calls_instances(si) + calls_seams(si)


# ---- the cases are what they claim to be (CPU) --------------------------------------------------------------------------------------------

def _words(mat, gapE, R8, qa, qb, b):
    """build_profile8's words of one live chain against residue b before the borrow, as signed sums: [position][row]"""
    P = 1 if R8 == 9 else 4
    KL = (R8 - 1) % P
    out = []
    for p in range(8):
        ws = []
        for r in range(R8):
            row = p * R8 + r
            lo = int(mat[b * 5 + qa[row]]) if row < len(qa) else 0
            hi = int(mat[b * 5 + qb[row]]) if qb is not None and row < len(qb) else 0
            fr = (1 + r % P - (KL if r == 0 else (r - 1) % P)) * gapE
            ws.append((lo + fr) + (hi + fr) * 65536)
        out.append(ws)
    return out


def census(si):
    """(borrowing lower words, of them under a zero-score upper word, calls with a dead chain B, calls whose last pair has no query B,
    calls whose trips hold null columns behind live ones, calls of two tiles and more) over the calls of a scoring"""
    match, mism, gO, gE = SCORINGS[si]
    mat = _matrix(si)
    borrow = zero_upper = dead_chain = no_qb = null_cols = tiled = 0
    for name, reads, target, flag in build_calls(si):
        L = len(reads[0]); R8 = _r8(L)
        assert all(len(r) == L for r in reads) and 1 <= L % 16 <= 8 and 203 <= len(target) <= 600, name
        npairs = (len(reads) + 1) // 2
        dead_chain += npairs % 2
        no_qb += len(reads) % 2
        null_cols += len(target) % 16 != 0
        # ssw_host.c's small-call rule: a call of a few pairs gets tiles down to max(halo / 8, 64) columns wherever the halo is shorter than the target
        P16 = (L + 15) // 16 * 16
        halo = P16 + (P16 * max(int(mat.max()), 0) + gE - 1) // gE + 1
        tiled += halo < len(target) and len(target) // max(halo // 8, 64) >= 2
        if R8 == 9:
            continue      # (no pair adds: RowFrame8<9>::PAIR)
        for k in range(0, len(reads), 2):
            qa, qb = reads[k], reads[k + 1] if k + 1 < len(reads) else None
            for b in set(int(x) for x in target):
                for p, ws in enumerate(_words(mat, gE, R8, qa, qb, b)):
                    for r in range(0, R8 - 1, 2):      # the lower words of the pairs
                        if ws[r] < 0:
                            borrow += 1
                            zero_upper += p * R8 + r + 1 >= L
    return borrow, zero_upper, dead_chain, no_qb, null_cols, tiled


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_no_case_is_vacuous(si):
    inst = calls_instances(si)
    assert sorted(_r8(len(r[0])) for _, r, _, _ in inst) == sorted(2 * list(range(1, 24, 2)))
    assert {len(r) for _, r, _, _ in inst} == {1, 2, 3, 4}
    for L in (len(r[0]) for _, r, _, _ in inst):
        R8 = _r8(L)
        if L % 8 and R8 >= 3 and R8 != 9:      # a zero-score row in the upper word of a pair
            assert any(p * R8 + r >= L for p in range(8) for r in range(1, R8 - 1, 2)), L
    for R8, rows in SEAM_ROWS.items():
        # pair boundaries (rows 2 and 4 of a position), class-0 rows (4 and 8; 0 and 4 of the next position), the seam between two positions
        assert all(x - 1 in rows and x in rows for x in (2, 4, 8, R8, R8 + 2, R8 + 4)), R8
    borrow, zero_upper, dead_chain, no_qb, null_cols, tiled = census(si)
    assert borrow > 0 and zero_upper > 0 and dead_chain > 0 and no_qb > 0 and null_cols > 0 and tiled > 0, (borrow, zero_upper, dead_chain, no_qb, null_cols, tiled)


def test_minus100_borrows_outside_class_0():
    """the strongly negative entry makes lower words of class 2 (profile entry: score + gapE) borrow too; under 2/-2/3/1 only class 0 does"""
    mat = _matrix(2)
    qa = np.array([0, 1] * 20, dtype=np.int8)
    ws = _words(mat, 1, 5, qa, None, 1) + _words(mat, 1, 5, qa, qa, 0)
    assert {r % 4 for w in ws for r in range(0, 4, 2) if w[r] < 0} == {0, 2}
    assert not any(w < 0 for x in _words(dna_matrix(2, 2), 1, 5, qa, qa, 1) for r, w in enumerate(x) if r % 4)


# ---- running the calls ----------------------------------------------------------------------------------------------------------------------

def run_calls(ctx, si, check=True, half=True):
    """every call of scoring si through ctx, every record against the reference; returns the records"""
    match, mism, gO, gE = SCORINGS[si]
    mat = _matrix(si)
    recs = []
    for name, reads, target, flag in build_calls(si):
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        assert tm["fill_kernel"].startswith("k_fill8<%d," % _r8(len(reads[0])) if half else "k_fill<"), (tm["fill_kernel"], name)
        recs.append(res.tobytes() + np.asarray(cig).tobytes())
        if check:
            bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, flag, 0, 0, -1, 2)
            assert not bad, "%s, %s: " % (IDS[si], name) + "\n".join(bad)
    return recs


def run_bound(ctx, bi, frame_k):
    """perfect copies at the largest match score of the frame form: every sum of the chain stays inside the range the carry rests on"""
    mism, gO, gE = BOUND_SCORINGS[bi]
    match = bound_match(bi, frame_k)
    mat = dna_matrix(match, mism)
    target = random_ref(400, 7900 + bi, 4)
    reads = [target[100:284].copy(), target[7:191].copy(), target[216:400].copy()]
    Q = ctx.upload(reads); T = ctx.upload([target])
    try:
        res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, 1, 0, 0, -1, 2)
    finally:
        Q.free(); T.free()
    assert ctx.timing()["fill_kernel"].startswith("k_fill8<23,"), ctx.timing()["fill_kernel"]
    assert [int(res[k, 0]["score1"]) for k in range(3)] == [184 * match] * 3
    bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, 1, 0, 0, -1, 2)
    assert not bad, "bound %s match %d: " % (BOUND_SCORINGS[bi], match) + "\n".join(bad)


_EMU_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill_pairadd as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
si = int(os.environ["PAIRADD_SI"])
n = len(m.run_calls(ctx, si))
if si < 2:
    m.run_bound(ctx, si, int(os.environ["SSW_GPU_FRAME_K"]))
ctx.close()
print("ok", n)
'''


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_pair_add_on_the_emulator(emu_lib_path, K, si):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K, PAIRADD_SI=str(si))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_pair_add_hooks_library_gpu(gpu_hctx, monkeypatch, si, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)      # (hooks of libssw_hooks.so, read at every call)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    recs = run_calls(gpu_hctx, si)
    if si < 2:
        run_bound(gpu_hctx, si, int(K))
    monkeypatch.setenv("SSW_GPU_FILL_HALF", "0")
    assert run_calls(gpu_hctx, si, check=False, half=False) == recs


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_pair_add_product_library_gpu(gpu_ctx, si):
    run_calls(gpu_ctx, si)
    if si < 2:
        run_bound(gpu_ctx, si, 0)
