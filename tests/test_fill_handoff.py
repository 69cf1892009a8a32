"""k_fill8's diagonal-gap form with its plain 32-bit adds in pairs (DESIGN.md "The plain adds in pairs"): (a1 : a2) - (g : 2g) in the class
reduction, and F's 4 x gapE subtracts each in one 64-bit add with an independent add -- the floor of the step after next, x of the odd last
row (its addend pair comes out of the profile: the word behind the last row's holds -4 gapE), a3 - 3g.  Results are bit for bit what they
were; what can break is a carry or a borrow between the two words of a pair, a pair formed from the wrong step's value (the floor is
formed a step ahead, x of the last row eleven rows ahead), and the profile word that no row owned before.  The hand-offs between lanes
keep their DPP form (the probe decided against LDS: docs/NOTEBOOK.md); the seam and column-maximum cases below run over every lane all the
same, because F, which every pair but one shares an instruction with, is what crosses the seams.

The calls, smallest shapes that can still go wrong:
  * every instance R8 = 1, 3 .. 23 at one read length each, calls of one to four reads (a dead chain B; a pair without query B), flags 0,
    1, 2, targets of 40, 200 and 1 100 columns -- the last crosses several renormalisation periods under SSW_GPU_FRAME_K 16 and 64;
  * one call per scoring on a 6 400-column target (tiles of 64 columns behind halos: a tile's first column sees the heads);
  * reads that copy a target segment with an insertion or a deletion over the position seam p -> p + 1, p = 0 .. 6, at R8 = 5 and 19;
  * reads whose best column has its maximum in a row of position p = 0 .. 7 and class 0 .. 3 (a prefix copy that ends there), with a
    second, weaker prefix copy elsewhere so that score2 / ref_end2 depend on the column maxima too -- the numpy DP asserts the row;
  * heads: alignments that begin in row 0 at column 0 and at a tile's first column; N residues before and inside the alignment;
  * pair arithmetic: 2/-2/3/1, 1/-3/5/2, the wide-gap scorings of tests/test_fill_rowframe.py (gapE 220 and 250) with the perfect 184-bp
    copy at the planner's last match score (tests/test_fill_diag_gaps.run_bound).
Every record is compared with the reference (tests/test_fill_diag_gaps._run), flag-0 records also with a plain numpy DP.  With
SSW_GPU_FILL_PAIRS=0 the hooks library and the emulator run the form without the pairs: records byte-identical; with SSW_GPU_FILL_DG=0 and
SSW_GPU_FILL_HALF=0 likewise.  On the emulator fr_add2 / fr_add_pair_sub assert at every pair that it equals the two 32-bit operations,
fr_add_pair its carry, pk_max3_fr the range of every operand: none may fire.  That SSW_GPU_FILL_PAIRS=0 selects another instantiation under
the same kernel name is seen in ssw_gpu_timing.fill_ops_per_row of the R8 = 7 call: 37/7 with the pairs, 38/7 without.

A case of the emulator test runs every lane of about a hundred small calls twice on the CPU: some 20 seconds; the device tests take
one to two seconds each."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import make_reads
from sswutil import dna_matrix, random_ref
from test_fill_diag_gaps import _r8, _run, run_bound
from test_fill_rowframe import BOUND_SCORINGS, TILE, TILES, T_LEN, _gapped, bound_match

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")

SCORINGS = ((2, 2, 3, 1), (1, 3, 5, 2))      # match, mismatch, gapO, gapE (the wide-gap scorings: run_bound)
IDS = ["2_2_3_1", "1_3_5_2"]
LENGTHS = {5: 40, 19: 150}
T_SIZES = (40, 200, 1100)


def np_dp(read, target, mat, n, gO, gE):
    """H of plain Smith-Waterman with affine gaps (gapO >= gapE), [len(read) + 1][len(target) + 1]: row by row, E as a running maximum"""
    L, m = len(read), len(target)
    S = np.asarray(mat, dtype=np.int64).reshape(n, n)[np.asarray(target, dtype=np.int64)]      # [m][n]
    H = np.zeros((L + 1, m + 1), dtype=np.int64)
    F = np.full(m + 1, -10 ** 6, dtype=np.int64)
    k = np.arange(m + 1, dtype=np.int64) * gE
    for i in range(1, L + 1):
        F = np.maximum(F - gE, H[i - 1] - gO)
        h = np.zeros(m + 1, dtype=np.int64)
        h[1:] = np.maximum(0, np.maximum(H[i - 1, :-1] + S[:, int(read[i - 1])], F[1:]))
        run = np.maximum.accumulate(h + k)      # a gap opened from an H that is itself E never beats extending: gapO >= gapE
        e = np.full(m + 1, -10 ** 6, dtype=np.int64)
        e[1:] = run[:-1] - k[:-1] - gO
        H[i] = np.maximum(h, e)
        H[i, 0] = 0
    return H


def _junk(n, avoid):
    """n times one residue that does not fit behind the copy: a run that scores next to nothing anywhere in a random target (random residues
    would: a hundred of them against a thousand columns reach a local score of 20 to 40 by chance)"""
    return np.full(n, (int(avoid[0]) + 1) % 4, dtype=np.int8)


# ---- the calls: (name, reads, target, flag) ----------------------------------------------------------------------------------------------

def calls_instances(si):
    rng = np.random.default_rng(7200 + si)
    calls = []
    for j, L in enumerate([8 * r - (5 * r) % 8 for r in range(1, 24, 2)]):
        m = T_SIZES[j % 3]
        target = random_ref(m, 7300 + 10 * j + si, 4)
        if j % 4 == 1:
            target[np.arange(11, m, 37)] = 4      # N residues
        reads = make_reads(rng, np.concatenate([target] * (1 + (L + 20) // m)), 1 + (j + si) % 4, [L], 4, frac_random=0.0)
        calls.append(("instance R8 %d, %d bp, %d columns" % (_r8(L), L, m), reads, target, (j + si) % 3))
    return calls


def _deleted(target, X, L, a, g):
    """rows 0 .. a - 1 are target[X : X + a], row a goes on g columns further on"""
    return np.concatenate([target[X:X + a], target[X + a + g:X + L + g]]).astype(np.int8)


def seam_cases(R8):
    """(first row behind the seam p -> p + 1, kind, length of the run), p = 0 .. 6"""
    return [((p + 1) * R8 - (1 if kind == "ins" else 0), kind, (2 if kind == "ins" else 1) + p % 3) for p in range(7) for kind in ("ins", "del")]


def calls_seams(si):
    calls = []
    for R8, L in LENGTHS.items():
        cases = seam_cases(R8)
        for k in range(0, len(cases), 4):
            target = random_ref(1100, 7500 + 100 * R8 + k + 1000 * si, 4)
            reads = []
            for j, (a, kind, g) in enumerate(cases[k:k + 4]):
                X = 30 + 230 * j
                reads.append(_gapped(target, X, L, a, g) if kind == "ins" else _deleted(target, X, L, a, g))
            calls.append(("seams R8 %d: %s" % (R8, cases[k:k + 4]), reads, target, (k // 4) % 3))
    return calls


def cm_reads(si, R8, L, p):
    """four reads, one per row class: rows 0 .. r are a copy of the target (best, ending in row r of position p) and the rest fits nothing;
    a second, shorter prefix copy stands elsewhere in the target.  Returns (reads, target, rows r)"""
    rng = np.random.default_rng(7700 + 1000 * si + 100 * R8 + p)
    target = random_ref(1100, 7800 + 100 * R8 + p + 1000 * si, 4)
    reads, rows = [], []
    for cls in range(4):
        k = [x for x in range(R8) if x % 4 == cls and p * R8 + x >= 12]
        if not k:
            continue
        r = p * R8 + k[len(k) // 2]
        X = 20 + 270 * cls
        weak = max(8, (r + 1) * 2 // 3)
        read = np.concatenate([target[X:X + r + 1], _junk(L - r - 1, target[X + r + 1:X + L + 1])]).astype(np.int8)
        for i in range(4):            # four columns behind the copy that the tail cannot match: the best cell is the copy's last, alone
            target[X + r + 1 + i] = ((int(read[r + 1]) if r + 1 < L else 0) + 1 + i % 3) % 4
        Y = X + 160                   # the weaker copy: the first `weak` rows again, behind the best one and before the next read's
        target[Y:Y + weak] = read[:weak]
        target[Y + weak] = (int(read[weak]) + 1) % 4
        reads.append(read); rows.append(r)
    return reads, target, rows


def calls_colmax(si):
    calls = []
    for R8, L in LENGTHS.items():
        for p in range(8):
            reads, target, rows = cm_reads(si, R8, L, p)
            if reads:
                calls.append(("column maximum R8 %d position %d rows %s" % (R8, p, rows), reads, target, 0 if p % 2 else 1))
    return calls


def calls_heads(si):
    calls = []
    for R8, L in LENGTHS.items():
        target = random_ref(T_LEN, 7900 + R8 + 1000 * si, 4)
        reads = [target[0:L].copy(), target[TILE * TILES[1]:TILE * TILES[1] + L].copy(), target[TILE * TILES[2]:TILE * TILES[2] + L].copy()]
        target[TILE * TILES[1] - 3:TILE * TILES[1]] = 4      # N residues directly before an alignment that begins at a tile's first column
        target[TILE * TILES[2] + L // 2] = 4                 # ... and inside one
        calls.append(("heads R8 %d, 6400 columns" % R8, reads, target, R8 % 3))
        small = random_ref(200, 7950 + R8 + 1000 * si, 4)
        rd = small[0:L].copy()
        small[L // 3] = 4; small[L + 3] = 4
        calls.append(("heads R8 %d, column 0 of 200" % R8, [rd], small, 0))
    return calls


def build_calls(si):
    return calls_instances(si) + calls_seams(si) + calls_colmax(si) + calls_heads(si)


# ---- the cases are what they claim to be (CPU) --------------------------------------------------------------------------------------------

def test_shapes_cover_every_instance_seam_and_class():
    for si in range(len(SCORINGS)):
        inst = calls_instances(si)
        assert [_r8(len(r[0])) for _, r, _, _ in inst] == list(range(1, 24, 2))
        assert all(1 <= len(r[0]) % 16 <= 8 for _, r, _, _ in inst)
        assert {len(r) for _, r, _, _ in inst} == {1, 2, 3, 4} and {f for _, _, _, f in inst} == {0, 1, 2}
        assert {len(t) for _, _, t, _ in inst} == set(T_SIZES) and any((t == 4).any() for _, _, t, _ in inst)
        for R8 in LENGTHS:
            assert all(g >= 2 for _, kind, g in seam_cases(R8) if kind == "ins")      # (the inserted run lies on both sides of the seam)
            assert {(a + (1 if kind == "ins" else 0)) // R8 for a, kind, _ in seam_cases(R8)} == set(range(1, 8))
        assert any(len(t) == T_LEN for _, _, t, _ in calls_heads(si))


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_the_column_maximum_lies_where_the_case_says(si):
    """the plain DP: the best cell of each column-maximum read lies in the row the case names -- every position 0 .. 7 and every class 0 .. 3
    at R8 = 19 -- the weaker copy scores less, and it ends in another row"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    seen = set()
    for R8, L in LENGTHS.items():
        for p in range(8):
            reads, target, rows = cm_reads(si, R8, L, p)
            for rd, r in zip(reads, rows):
                H = np_dp(rd, target, mat, 5, gO, gE)
                i, j = np.unravel_index(int(np.argmax(H)), H.shape)
                assert i - 1 == r and (H == H.max()).sum() == 1 and H.max() == match * (r + 1), (R8, p, r, i, H.max())      # (every case, R8 = 5 too)
                far = np.ones(H.shape[1], dtype=bool); far[max(0, j - L):j + L // 2] = False      # (behind the best cell H decays to 0 within a few columns)
                second = H[:, far].max()
                assert 8 * match <= second < H.max(), (R8, p, r, second)
                seen.add((R8, p, r % R8 % 4))
    assert {(p, c) for R8, p, c in seen if R8 == 19} == {(p, c) for p in range(8) for c in range(4)}
    # R8 = 5 (40 bp): positions 0 and 1 end before row 12, where a copy is too short to stand out; every class from position 2 on that has a row there
    assert {(p, c) for R8, p, c in seen if R8 == 5} == {(p, c) for p in range(2, 8) for c in range(4) if any(x % 4 == c and 5 * p + x >= 12 for x in range(5))}


# ---- running the calls ----------------------------------------------------------------------------------------------------------------------

def run_calls(ctx, si, dg=True, check=True, name=True):
    """every call of scoring si, every record against the reference and every flag-0 record against the numpy DP; returns the records"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    calls = build_calls(si)
    recs = _run(ctx, calls, mat, gO, gE, dg, check, IDS[si]) if name else _run_unnamed(ctx, calls, mat, gO, gE)
    if check:
        for (cname, reads, target, flag), rec in zip(calls, recs):
            if flag != 0:
                continue
            from ssw_amd import RESULT_DTYPE
            res = np.frombuffer(rec[:RESULT_DTYPE.itemsize * len(reads)], dtype=RESULT_DTYPE)
            for q, rd in enumerate(reads):
                H = np_dp(rd, target, mat, 5, gO, gE)
                assert int(res[q]["score1"]) == int(H.max()), (cname, q, int(res[q]["score1"]), int(H.max()))
                assert H[int(res[q]["read_end1"]) + 1, int(res[q]["ref_end1"]) + 1] == H.max(), (cname, q)
    return recs


def _run_unnamed(ctx, calls, mat, gO, gE):
    """the product library on its own choice of kernel (no hook holds the small calls on k_fill8): records against the reference"""
    from parity import compare_batch
    recs = []
    for name, reads, target, flag in calls:
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        recs.append(res.tobytes() + np.asarray(cig).tobytes())
        bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, flag, 0, 0, -1, 2)
        assert not bad, name + ": " + "\n".join(bad)
    return recs


def bound_records(ctx, bi, frame_k):
    """the perfect 184-bp copies of run_bound at the planner's last match score of the wide-gap scoring bi: the records"""
    mism, gO, gE = BOUND_SCORINGS[bi]
    mat = dna_matrix(bound_match(bi, frame_k), mism)
    target = random_ref(T_LEN, 6900 + bi, 4)
    reads = [target[3000:3184].copy(), target[70:254].copy(), target[5000:5184].copy()]
    return _run(ctx, [("bound %s" % (BOUND_SCORINGS[bi],), reads, target, 1)], mat, gO, gE, True, True, "bound")


def ops_of_r8_7(ctx, si):
    """ssw_gpu_timing.fill_ops_per_row of the R8 = 7 instance call: the exact count of the instantiation that ran"""
    match, mism, gO, gE = SCORINGS[si]
    call = [c for c in calls_instances(si) if _r8(len(c[1][0])) == 7]
    assert len(call) == 1
    _run(ctx, call, dna_matrix(match, mism), gO, gE, True, False, "R8 7")
    return ctx.timing()["fill_ops_per_row"]


def run_all_forms(ctx, si, frame_k, setenv, delenv):
    """the calls and the bound case with the pairs, every record checked; then without them (SSW_GPU_FILL_PAIRS=0): another instantiation by
    its instruction count, the same records byte for byte"""
    recs = run_calls(ctx, si) + bound_records(ctx, si, frame_k)
    run_bound(ctx, si, frame_k)
    ops = ops_of_r8_7(ctx, si)
    assert abs(ops - 37.0 / 7) < 1e-9, ops
    setenv("SSW_GPU_FILL_PAIRS", "0")
    ops0 = ops_of_r8_7(ctx, si)
    assert abs(ops0 - 38.0 / 7) < 1e-9, ("SSW_GPU_FILL_PAIRS=0 did not select the form without the pairs", ops0)
    assert run_calls(ctx, si, check=False) + bound_records(ctx, si, frame_k) == recs, "the form without the pairs gives other records"
    delenv("SSW_GPU_FILL_PAIRS")
    return recs


_EMU_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill_handoff as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
si = int(os.environ["HANDOFF_SI"])
recs = m.run_all_forms(ctx, si, int(os.environ["SSW_GPU_FRAME_K"]), os.environ.__setitem__, os.environ.pop)
ctx.close()
print("ok", len(recs))
'''


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_paired_adds_on_the_emulator(emu_lib_path, K, si):
    """no pair assertion, no carry assertion and no range assertion fires; records equal the reference's and those of the form without pairs"""
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K, HANDOFF_SI=str(si))
    e.pop("SSW_GPU_FILL_PAIRS", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_paired_adds_hooks_library_gpu(gpu_hctx, monkeypatch, si, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)      # (hooks of libssw_hooks.so, read at every call)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    recs = run_all_forms(gpu_hctx, si, int(K), monkeypatch.setenv, monkeypatch.delenv)[:len(build_calls(si))]
    monkeypatch.setenv("SSW_GPU_FILL_DG", "0")
    assert run_calls(gpu_hctx, si, dg=False, check=False) == recs
    monkeypatch.setenv("SSW_GPU_FILL_HALF", "0")
    assert run_calls(gpu_hctx, si, check=False, name=False) == recs


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_paired_adds_product_library_gpu(gpu_ctx, si):
    run_calls(gpu_ctx, si, name=False)
    run_bound(gpu_ctx, si, 0)
