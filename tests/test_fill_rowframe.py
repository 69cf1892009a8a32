"""Half-row fill chains (k_fill8) in the blocked row frame: row r of a position is held (r mod 4) x gapE above the column frame, so that F
pays its gap extension once per four rows (DESIGN.md "Blocked row frame").  What changes with it, and the shapes that reach each piece:

  * every instance (the class of a position's last row is 0 or 2, the hand-off constants differ): read lengths 1, 17, .. 177 and 8, 24, ..
    184 -- R8 = 1, 3, .. 23, each twice;
  * the floors of every class: reads with a soft-clipped prefix of r residues, r = 0 .. 2 R8, whose local alignment therefore begins in row
    r -- E and H of that row start from the floor of its class -- with the alignment's first column in the first 16 columns of the target
    (floors of the first trip), in mid-tile and at the first column of a tile; R8 = 5 (40 bp) and R8 = 19 (150 bp);
  * F across every seam: reads with an inserted run of 1 .. 6 residues (a vertical gap) over the class-3 / class-0 seam inside a position,
    over the seam between two positions, and over neither (runs of 1 .. 3 rows in classes 1 .. 3: a longer run always crosses a class seam);
  * the column maximum of every class: reads decided under the 8-bit rule with a weaker second copy outside the mask window, cut off after
    a row of class 0, 1, 2, 3 -- score2 / ref_end2 are that column's maximum -- and the whole weaker copy ending in row P8 - 1, where the
    closed form of the padded rows starts from the values position 7 parks in the class of its last row;
  * lane 0's boundary: an alignment that starts in column 0 of the target, and one that starts in the first traversal column of a tile;
  * the bound: a perfect 184-bp copy at the largest match score for which the planner still takes the frame form, and at the next one.

Scorings 2/-2/3/1, 1/-3/5/2 and 5/-4/10/4 (gapE = 4); targets of 6 400 columns, one to four reads per call: the small-call rule cuts the
target into tiles of 64 columns behind halos of several hundred.  Every record is compared with the reference (parity.compare_batch); the
hooks library and the emulator renormalise every 16 and every 64 steps (SSW_GPU_FRAME_K), and the hooks library's records are compared
byte for byte with the 16-lane kernel's (SSW_GPU_FILL_HALF=0).  Under the emulator pk_max3_fr asserts the range of every operand.

8-bit rule and scoring 5/-4/10/4: a 150-bp read cannot stay under 255 - bias there with its alignment in one piece, so the column-maximum
cases of that scoring are the 40-bp ones; the other two scorings have both lengths."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_batch, expected, make_reads
from sswutil import dna_matrix, random_ref
from test_fill_half import _plain_dp
from test_fill_half_flush import _copies, _halo

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")

SCORINGS = ((2, 2, 3, 1), (1, 3, 5, 2), (5, 4, 10, 4))      # match, mismatch, gapO, gapE
IDS = ["2_2_3_1", "1_3_5_2", "5_4_10_4"]
BOUND_SCORINGS = ((4, 255, 220), (2, 255, 250))               # mismatch, gapO, gapE: int8 match scores reach the frame's range only with wide gaps
T_LEN = 6400
TILE = 64
TILES = (20, 40, 60, 80)
LENGTHS = {5: 40, 19: 150}                                    # R8 -> read length of the shaped cases
TOP8 = 244


def _r8(L):
    return (L + 7) // 8


def _cls(row, L):
    """class of a read's row in the blocked row frame"""
    return row % _r8(L) % 4


# ---- the calls: (name, reads, target, flag) ----------------------------------------------------------------------------------------------

def calls_instances(si):
    rng = np.random.default_rng(5200 + si)
    calls = []
    for j, L in enumerate([1 + 16 * i for i in range(12)] + [8 + 16 * i for i in range(12)]):
        target = random_ref(T_LEN, 8000 + 10 * j + si, 4)
        reads = make_reads(rng, target, 1 + j % 4, [L], 4, frac_random=0.0)
        calls.append(("instance R8 %d, %d bp" % (_r8(L), L), reads, target, j % 3))
    return calls


def _clipped(rng, target, X, L, r):
    """a read whose rows r .. L - 1 are target[X : X + L - r] and whose first r residues differ from what stands before column X"""
    read = np.empty(L, dtype=np.int8)
    read[r:] = target[X:X + L - r]
    for i in range(r):
        c = X - r + i
        read[i] = (target[c] + 1 + i % 3) % 4 if c >= 0 else rng.integers(0, 4)
    return read


def floor_places(r, R8):
    """first columns of the three alignments of a call: in the first 16 columns, in mid-tile, at the first column of a tile"""
    return (5 * r + R8) % 16, TILE * TILES[1] + 13 + (7 * r) % 40, TILE * TILES[2 + r % 2]


def calls_floors(si):
    rng = np.random.default_rng(5300 + si)
    calls = []
    for R8, L in LENGTHS.items():
        for r in range(2 * R8 + 1):
            target = random_ref(T_LEN, 8300 + 100 * R8 + r + 1000 * si, 4)
            reads = [_clipped(rng, target, X, L, r) for X in floor_places(r, R8)]
            calls.append(("floors R8 %d, alignment from row %d" % (R8, r), reads, target, 1))
    return calls


def gap_cases(R8):
    """(first row of the inserted run, its length, what it spans) in position 3 of the chain"""
    p0 = 3 * R8
    out = []
    for g in range(1, 7):
        out.append((p0 + 4 - g // 2, g, "class"))          # rows p0 + 3 (class 3) and p0 + 4 (class 0) are both in a - 1 .. a + g - 1
        out.append((p0 + R8 - g // 2, g, "position"))      # rows p0 + R8 - 1 and the next position's row 0
        if g <= 3:
            out.append((p0 + 1, g, "neither"))             # F born in row p0 (class 0) runs through classes 1 .. 3 at most
    return out


def _gapped(target, X, L, a, g):
    seg = target[X:X + L - g]
    run = np.array([(int(seg[a]) + 1 + k % 3) % 4 for k in range(g)], dtype=np.int8)      # (no residue of the run fits behind it)
    return np.concatenate([seg[:a], run, seg[a:]]).astype(np.int8)


def gap_calls(si):
    """(cases of the call, reads, target)"""
    out = []
    for R8, L in LENGTHS.items():
        cases = gap_cases(R8)
        k = shape = 0
        while k < len(cases):
            n = min(1 + shape % 4, len(cases) - k); shape += 1
            target = random_ref(T_LEN, 8600 + 100 * R8 + k + 1000 * si, 4)
            reads = [_gapped(target, TILE * TILES[j] + 5 + 9 * j, L, cases[k + j][0], cases[k + j][1]) for j in range(n)]
            out.append((cases[k:k + n], reads, target))
            k += n
    return out


def calls_gaps(si):
    return [("gaps R8 %d: %s" % (_r8(len(reads[0])), cases), reads, target, 2) for cases, reads, target in gap_calls(si)]


def _weak_copy(read, scoring):
    """(best copy, weaker whole copy): tests/test_fill_half_flush.py's for 150 bp; a 40-bp read scores under TOP8 as it is and its weaker
    copy has two substitutions between runs that outweigh them"""
    if len(read) >= 100:
        best, weak, top = _copies(read, scoring)
    else:
        best, weak, top = read.copy(), read.copy(), scoring[0] * len(read)
        for p in (9, 19):
            weak[p] = (weak[p] + 1) % 4
    assert top <= TOP8
    return best, weak


def cm_cases(si):
    """(L, m): the second copy is the read's first m residues, m - 1 a row of position 4 in each of the four classes; m = 0: the whole weaker copy"""
    out = []
    for R8, L in LENGTHS.items():
        if SCORINGS[si][0] * L > 2 * TOP8 and L >= 100:
            continue      # (5/-4/10/4 and 150 bp: see the module text)
        rows = [4 * R8 + 4 + k for k in range(4)] if R8 > 5 else [4 * R8 + k for k in range(4)]
        assert sorted(_cls(x, L) for x in rows) == [0, 1, 2, 3]
        out += [(L, x + 1) for x in rows] + [(L, 0)]
    return out


def _cm_call(si, idx, L, m, nreads):
    """read k of the call has its second copy end in column X_k (returned) and its best copy 200 columns behind"""
    scoring = SCORINGS[si]
    rng = np.random.default_rng(5500 + 100 * si + idx)
    target = random_ref(T_LEN, 8900 + idx + 1000 * si, 4)
    reads, ends = [], []
    for j in range(nreads):
        read = rng.integers(0, 4, size=L, dtype=np.int8)
        best, weak = _weak_copy(read, scoring)
        X = TILE * TILES[j] + 11 + 17 * j + idx
        if m:
            target[X + 1 - m:X + 1] = read[:m]
            target[X + 1] = (read[m] + 1) % 4                  # the copy ends here
        else:
            target[X + 1 - L:X + 1] = weak
        b0 = X + 200
        target[b0:b0 + L] = best
        reads.append(read); ends.append(X)
    return reads, target, ends


def calls_colmax(si):
    calls = []
    for idx, (L, m) in enumerate(cm_cases(si)):
        reads, target, ends = _cm_call(si, idx, L, m, 1 + idx % 4)
        calls.append(("column maximum %d bp, second copy of %d rows" % (L, m or L), reads, target, 0))
    return calls


def calls_boundary(si):
    rng = np.random.default_rng(5600 + si)
    calls = []
    for R8, L in LENGTHS.items():
        target = random_ref(T_LEN, 9200 + R8 + 1000 * si, 4)
        c_first = TILE * TILES[1] - _halo(L, SCORINGS[si])       # first traversal column of tile TILES[1]
        assert c_first > L
        reads = [target[0:L].copy(), target[c_first:c_first + L].copy()]
        reads += make_reads(rng, target, R8 % 3, [L], 4, frac_random=0.0)
        calls.append(("boundary R8 %d: columns 0 and %d" % (R8, c_first), reads, target, 1))
    return calls


def build_calls(si):
    return calls_instances(si) + calls_floors(si) + calls_gaps(si) + calls_colmax(si) + calls_boundary(si)


# ---- the cases are what they claim to be (CPU) --------------------------------------------------------------------------------------------

def test_shapes_cover_every_instance_class_and_seam():
    for si in range(len(SCORINGS)):
        inst = calls_instances(si)
        assert sorted(_r8(len(r[0])) for _, r, _, _ in inst) == sorted(2 * list(range(1, 24, 2)))
        assert {len(r) for _, r, _, _ in inst} == {1, 2, 3, 4}
        assert {(_r8(len(r[0])) - 1) % 4 for _, r, _, _ in inst} == {0, 2}          # class of the last row of a position
        for R8, L in LENGTHS.items():
            assert _r8(L) == R8 and (L + 7) // 8 * 8 == (L + 15) // 16 * 16 - 8      # eligible for the half-row chains
            for r in range(2 * R8 + 1):
                first, mid, seam = floor_places(r, R8)
                assert first < 16 and 8 < mid % TILE < TILE - 8 and seam % TILE == 0
            spans = {}
            for a, g, what in gap_cases(R8):
                rows = range(a - 1, a + g)                                           # F is born in row a - 1 and runs to row a + g - 1
                crossed_cls = any(x % R8 % 4 == 3 and (x + 1) % R8 != 0 and x + 1 in rows for x in rows)
                crossed_pos = any((x + 1) % R8 == 0 and x + 1 in rows for x in rows)
                # (R8 = 5: the class seam is one row above the position seam, a run of three rows and more crosses both)
                assert (what == "class") <= crossed_cls and (what == "position") <= crossed_pos, (R8, a, g, what)
                assert (what == "neither") <= (not crossed_cls and not crossed_pos), (R8, a, g, what)
                spans.setdefault(what, set()).add(g)
            assert spans == {"class": set(range(1, 7)), "position": set(range(1, 7)), "neither": {1, 2, 3}}
        assert {len(r) for _, r, _, _ in calls_gaps(si)} == {1, 2, 3, 4}


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_gapped_reads_align_through_their_gap(si):
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    for cases, reads, target in gap_calls(si):
        for (a, g, what), read in zip(cases, reads):
            if match * min(a, len(read) - a - g) < gO + (g - 1) * gE + 4:
                continue      # 40 bp under 1/-3/5/2: a flank of 16 or 17 matches does not pay for a run of 5 or 6 (the cells are computed all the same)
            _, cig = expected(read, mat, 5, target, gO, gE, 2, 0, 0, len(read) // 2, 2)
            assert any(c & 15 == 1 and c >> 4 == g for c in cig), ("vacuous case: no insertion of %d in the reference's alignment" % g, a, what, SCORINGS[si])


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_no_column_maximum_case_is_vacuous(si):
    """the plain DP over the columns that can reach X: a copy cut off after row m - 1 puts the maximum of column X into that row alone -- a row
    of the intended class; the whole weaker copy raises a maximum of X .. X + 7 in the padded rows"""
    match, mism, gO, gE = SCORINGS[si]
    seen = set()
    for idx, (L, m) in enumerate(cm_cases(si)):
        reads, target, ends = _cm_call(si, idx, L, m, 1 + idx % 4)
        P16 = (L + 15) // 16 * 16
        for rd, X in zip(reads, ends):
            lo, hi = max(0, X + 1 - L - 8 - _halo(L, SCORINGS[si])), min(T_LEN, X + 8)
            t = target[lo:hi].tolist()
            cm8, cm16, _, _ = _plain_dp(rd.tolist(), t, match, mism, gO, gE, P16)
            if m:
                upto, _, _, _ = _plain_dp(rd.tolist(), t, match, mism, gO, gE, m + 8)           # rows < m
                below, _, _, _ = _plain_dp(rd.tolist(), t, match, mism, gO, gE, m + 7)          # rows < m - 1
                assert cm8[X - lo] == upto[X - lo] == match * m > below[X - lo], ("vacuous case: the maximum of column X is not row m - 1's", L, m, X)
                seen.add((L, _cls(m - 1, L)))
            else:
                assert any(cm16[j] > cm8[j] for j in range(X - lo, hi - lo)), ("vacuous case: the padded rows raise no maximum in X .. X + 7", L, X)
                seen.add((L, "pad"))
    lens = {L for L, _ in cm_cases(si)}
    assert seen == {(L, k) for L in lens for k in (0, 1, 2, 3, "pad")} and 40 in lens and (si == 2 or 150 in lens)


# ---- the bound ----------------------------------------------------------------------------------------------------------------------------

def _frame_fits(match, mism, gO, gE, L, lanes, frame_k):
    """ssw_frame_params (ssw_host.c) for a bucket of L-bp reads"""
    K = 1024
    if frame_k:
        K = 16
        while K * 2 <= frame_k and K < 1024:
            K <<= 1
    while K > 64 and K * gE > 4096:
        K >>= 1
    b = mism + gO + 2 * gE + 8
    up = lanes + 2 + (3 if lanes == 8 else 0)
    top = (L + 15) // 16 * 16 * match
    while K > 64 and top + b + (K + up) * gE >= 31744:
        K >>= 1
    return top + b + (K + up) * gE < 31744


def bound_match(bi, frame_k):
    """the largest match score at which a 184-bp bucket gets the frame form on 16-lane AND on half-row chains (the planner asks for both)"""
    mism, gO, gE = BOUND_SCORINGS[bi]
    fits = [m for m in range(1, 127) if _frame_fits(m, mism, gO, gE, 184, 16, frame_k) and _frame_fits(m, mism, gO, gE, 184, 8, frame_k)]
    assert fits and fits[-1] < 126 and fits == list(range(1, fits[-1] + 1))
    return fits[-1]


def run_bound(ctx, bi, frame_k):
    mism, gO, gE = BOUND_SCORINGS[bi]
    top = bound_match(bi, frame_k)
    target = random_ref(T_LEN, 9500 + bi, 4)
    reads = [target[3000:3184].copy(), target[70:254].copy()]
    for match, frame in ((top, True), (top + 1, False)):
        mat = dna_matrix(match, mism)
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, 1, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        assert tm["fill_kernel"].startswith("k_fill8<23,") == frame, (tm["fill_kernel"], match, BOUND_SCORINGS[bi])
        assert (tm["fill_ops_per_row"] < 6.5) == frame and (frame or tm["fill_ops_per_row"] == 9.0), (tm["fill_ops_per_row"], tm["fill_kernel"])
        assert int(res[0, 0]["score1"]) == 184 * match
        bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, 1, 0, 0, -1, 2)
        assert not bad, "bound %s match %d: " % (BOUND_SCORINGS[bi], match) + "\n".join(bad)


@pytest.mark.parametrize("bi", [0, 1])
def test_reference_is_unsaturated_at_the_bound(bi):
    mism, gO, gE = BOUND_SCORINGS[bi]
    target = random_ref(T_LEN, 9500 + bi, 4)
    for fk in (0, 16, 64):
        m = bound_match(bi, fk)
        for match in (m, m + 1):
            assert match <= 127 and 184 * match < 32767
            d, _ = expected(target[3000:3184].copy(), dna_matrix(match, mism), 5, target, gO, gE, 1, 0, 0, 92, 2)
            assert d["score1"] == 184 * match and d["ref_end1"] == 3183


# ---- running the calls ----------------------------------------------------------------------------------------------------------------------

def run_calls(ctx, si, check=True, half=True):
    """every call of scoring si through ctx, every record against the reference; returns the records"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    recs = []
    for name, reads, target, flag in build_calls(si):
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        assert tm["fill_kernel"].startswith("k_fill8<%d," % _r8(len(reads[0])) if half else "k_fill<"), (tm["fill_kernel"], name)
        if half:
            # (R8 = 9 is the one instance that keeps the column frame alone: it has no registers for four floors and accumulators)
            assert tm["fill_ops_per_row"] == 6.5 if _r8(len(reads[0])) == 9 else 5.0 <= tm["fill_ops_per_row"] < 6.5, (tm["fill_ops_per_row"], name)
        recs.append(res.tobytes() + np.asarray(cig).tobytes())
        if check:
            bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, flag, 0, 0, -1, 2)
            assert not bad, "%s, %s: " % (SCORINGS[si], name) + "\n".join(bad)
    return recs


_EMU_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill_rowframe as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
si = int(os.environ["ROWFRAME_SI"])
n = len(m.run_calls(ctx, si))
if si < 2:
    m.run_bound(ctx, si, int(os.environ["SSW_GPU_FRAME_K"]))
ctx.close()
print("ok", n)
'''


@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_row_frame_on_the_emulator(emu_lib_path, K, si):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K, ROWFRAME_SI=str(si))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
@pytest.mark.parametrize("K", ["16", "64"])
def test_row_frame_hooks_library_gpu(gpu_hctx, monkeypatch, si, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)      # (hooks of libssw_hooks.so, read at every call)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    recs = run_calls(gpu_hctx, si)
    monkeypatch.setenv("SSW_GPU_FILL_HALF", "0")
    assert run_calls(gpu_hctx, si, check=False, half=False) == recs


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SCORINGS)), ids=IDS)
def test_row_frame_product_library_gpu(gpu_ctx, si):
    run_calls(gpu_ctx, si)


@pytest.mark.gpu
@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("K", ["16", "64"])
def test_bound_hooks_library_gpu(gpu_hctx, monkeypatch, bi, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    run_bound(gpu_hctx, bi, int(K))


@pytest.mark.gpu
@pytest.mark.parametrize("bi", [0, 1])
def test_bound_product_library_gpu(gpu_ctx, bi):
    run_bound(gpu_ctx, bi, 0)
