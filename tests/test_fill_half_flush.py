"""Half-row fill chains (k_fill8): what the stage and the flush make of the values position 7 parks -- the closed form of the padded rows,
column by column.  Record-level tests hit a given column of a given trip only by luck; here the column is chosen.

Every read is decided under the 8-bit rule (101 bp, and 150 bp with enough substitutions in its best copy to stay under 253 - bias), so its
second-best score is scanned over the maxima of ALL P16 rows, the eight zero-score rows below the read included, which k_fill8 does not
compute.  Each read has its best copy somewhere in the target and a weaker second copy outside the mask window of the best one, which ends
P8 - len columns before column X (P8 = 8 * ceil(len / 8): 3 spare zero-score rows for 101 bp, 2 for 150 bp, which the chain computes): in
column X the copy's score stands in row P8 - 1, the last row of position 7, enters the padded rows, v(X + 1) carries it, the window holds
it for eight columns and T lets it decay behind them.  X is swept so that the step at which position 7 finishes it walks over everything
the parked values pass through:

  * a whole tile and nine columns on either side of it (tiles of 64 columns: what the small-call rule makes of a 6 400-column target for
    one to four reads on 256 compute units, with a halo of 176 to 496 columns -- _halo() -- so every tile from the eighth on starts its
    traversal `halo` columns early).  Relative to the tile's first traversal column the steps of 64 + 18 consecutive X cover every residue
    mod 64: -9 .. +9 around every multiple of 16 (group edge and carry; a renormalisation with SSW_GPU_FRAME_K=16), around the multiple of
    64 (wrap of the v ring and its mirror, two laps of the 32-slot ring of maxima; a renormalisation with SSW_GPU_FRAME_K=64) as far as
    the tile has stored columns there, and the seam itself;
  * columns 2 .. 9 of the target (nothing before the chain: the second copy is the read's last few residues).  DROPPED: columns 0 and 1 --
    no residue of a read reaches row P8 - 1 before column P8 - len, the padded rows are zero there whatever the input;
  * the last 16 columns of the target (the flushes after the loop).  DROPPED: the last column -- what it hands to the padded rows would
    show in columns that do not exist.

SSW_GPU_FRAME_K is a hook: the hooks library and the emulator run the sweep with 16 and 64.  The product library has the natural period,
1 024 steps at gapE = 1, which a call of at most four reads never reaches -- its tiles are 64 columns behind at most 496 of halo -- so there
the same sweep runs without a renormalisation inside it; tests/test_full_size.py has the natural period at full size.

Batch shapes: one read (chain B dead), two (one full pair; chain B a pair that does not exist), three and four (chain B live with a lone
read / a full pair); the reads of a call have DIFFERENT offsets into their tiles, so a value of one chain that leaks into the other's
rings or group maxima lands in a column where the reference has something else.  One call has a two-letter tandem repeat, where the padded
rows raise the maxima of several consecutive groups and T is carried from group to group.

No case is vacuous: for every X the plain DP of tests/test_fill_half.py, over the columns that can reach X, must show cm16 > cm8 somewhere
in X .. X + 7 (test_no_case_is_vacuous; it fails, it does not skip).  The three columns named above are the only cases dropped."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_batch
from sswutil import dna_matrix, random_ref
from test_fill_half import _plain_dp

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")

SCORINGS = ((2, 2, 3, 1), (1, 3, 5, 2))      # match, mismatch, gapO, gapE
T_LEN = 6400
TILE = 64
TILES = (20, 40, 60, 80)                      # where the reads of a call have their second copies: all behind the widest halo
OFFSETS = tuple(range(-9, TILE + 10))         # X = 64 * tile + offset: a whole tile and nine columns on either side
UNIT = np.array([0, 0, 0, 0, 0, 0, 0, 2], dtype=np.int8)
EMU_LENGTHS = ((150,), (101,))               # the bench's shape under the bench's scoring; the short class under the other
TOP8 = 244                                    # best copies score at most this: under 253 - bias with room to spare


def _halo(L, scoring):
    """the planner's halo for reads of L residues (ssw_host.c, halo_for): P16 + ceil(P16 * match / gapE) + 1, rounded up to 16 columns"""
    match, _, _, gE = scoring
    P16 = (L + 15) // 16 * 16
    return (P16 + (P16 * match + gE - 1) // gE + 1 + 15) // 16 * 16


def _rel_step(X, L, scoring):
    """the step, counted from the tile's first traversal column, at which position 7 finishes column X"""
    c_first = max(0, X // TILE * TILE - _halo(L, scoring))
    return X - c_first + 7


def _with_subs(read, n):
    """a copy of the read with n substitutions, evenly spread, none in the first 6 or the last 14 residues: every run between two of them
    outweighs a mismatch, so the local alignment spans the whole read and ends in its last row"""
    c = read.copy()
    if n:
        step = (len(read) - 20) // n
        assert step >= 5
        for k in range(n):
            c[6 + k * step] = (c[6 + k * step] + 1 + k % 2) % 3 if c.max() < 3 else (c[6 + k * step] + 1 + k % 3) % 4
    return c


def _copies(read, scoring):
    match, mism = scoring[:2]
    L = len(read)
    n1 = max(0, -(-(match * L - TOP8) // (match + mism)))
    return _with_subs(read, n1), _with_subs(read, n1 + 6), match * L - n1 * (match + mism)


def _length(i, si):
    return (150, 101)[(i + si) % 2]


def _call(rng, target, scoring, ends, lens):
    """plants, for read k, a weak copy that stands in row P8 - 1 in column ends[k] and the best copy 200 columns behind it; returns the reads"""
    reads = []
    for X, L in zip(ends, lens):
        X -= (L + 7) // 8 * 8 - L              # where the copy itself ends
        assert X >= 0
        # at the start of the target the second copy is a handful of residues and any chance match in the rows above would equal it: there
        # the read has three letters and the eight columns behind X the fourth, so that the rows of the read only lose from X on
        read = rng.integers(0, 3 if X < 16 else 4, size=L, dtype=np.int8)
        best, weak, top = _copies(read, scoring)
        assert top <= TOP8
        n = min(L, X + 1)                      # X < L - 1: only the read's last X + 1 residues fit in front of column X
        target[X + 1 - n:X + 1] = weak[L - n:]
        if X < 16:
            target[X + 1:X + 9] = 3
        b0 = X + 200 if X + 200 + L <= T_LEN - 200 else X - 1000
        assert b0 >= 0 and np.all(target[b0:b0 + L] < 4)
        target[b0:b0 + L] = best
        reads.append(read)
    return reads


def build_calls(si, lengths=(150, 101)):
    """the calls of scoring si: (reads, target, [X of every read]); the same on every machine.  One read length per call (one bucket: the
    half-row kernel).  The sweep over a tile is made once per length of `lengths` -- the halo, and with it the step of a column, depends on
    the length: the device and the checks below take both, the emulator one per scoring (EMU_LENGTHS) to stay within its time"""
    scoring = SCORINGS[si]
    rng = np.random.default_rng(4100 + si)
    calls = []
    for L in lengths:
        offs, shape = list(OFFSETS), 0
        while offs:      # 1, 2, 3, 4, 1, ... reads per call, read k in tile TILES[k] at the next offset
            k = min(1 + shape % 4, len(offs)); shape += 1
            target = random_ref(T_LEN, 7000 + 10 * len(calls) + si, 4)
            ends = [TILE * TILES[j] + offs.pop(0) for j in range(k)]
            calls.append((_call(rng, target, scoring, ends, [L] * k), target, ends))
    for j in range(15):      # the last columns of the target, and columns 2 .. 9 in the same call while they last (column 2: 150 bp only)
        target = random_ref(T_LEN, 7500 + 10 * j + si, 4)
        ends = [T_LEN - 16 + j] + ([j + 2] if j < 8 else [])
        lens = [150 if j == 0 else _length(j, si)] * len(ends)
        calls.append((_call(rng, target, scoring, ends, lens), target, ends))
    return calls


def build_repeat_call(si):
    """150-bp reads that end in 40 residues of a two-letter repeat of period 8, against a target with 300 columns of it: the read's tail fits
    at every eighth column of the stretch; the two spare rows of the chain carry its score for two columns, the padded rows for the five
    after them, where the rows of the read are out of phase and have less -- v is high in one column of eight, the window is full all
    the time, T is refreshed in every group -- and behind the stretch T decays over (score - gapO) / gapE columns"""
    scoring = SCORINGS[si]
    rng = np.random.default_rng(4200 + si)
    target = random_ref(T_LEN, 7900 + si, 4)
    target[2000:2304] = np.tile(UNIT, 38)
    reads = []
    for k in range(3):
        read = np.concatenate([rng.integers(0, 4, size=110, dtype=np.int8), np.tile(UNIT, 5)])
        best, _, top = _copies(read, scoring)
        assert top <= TOP8
        target[3000 + 400 * k:3150 + 400 * k] = best
        reads.append(read)
    return reads, target


def _window(X, L, scoring):
    """the columns that can reach X (the exact halo), up to X + 7"""
    return max(0, X + 1 - L - 8 - _halo(L, scoring)), min(T_LEN, X + 8)


def test_sweep_covers_what_it_claims():
    for si, scoring in enumerate(SCORINGS):
        calls = build_calls(si)
        shapes = {len(r) for r, _, _ in calls}
        assert shapes == {1, 2, 3, 4}
        steps = {}
        for reads, _, ends in calls:
            assert len({X % TILE for X in ends}) == len(ends)                       # different offsets in chains A and B
            for rd, X in zip(reads, ends):
                steps.setdefault(len(rd), set()).add((X, _rel_step(X, len(rd), scoring)))
        both = set().union(*steps.values())
        assert {X for X, _ in both} >= set(range(2, 10)) | set(range(T_LEN - 16, T_LEN - 1))
        assert {(len(r), len(r[0])) for r, _, _ in calls} == {(k, L) for k in (1, 2, 3, 4) for L in (101, 150)}      # every shape with both lengths
        for L in (101, 150):      # either length alone: every offset of the sweep, and with them every residue mod 64 of the step
            assert {X - TILE * t for X, _ in steps[L] for t in TILES if -9 <= X - TILE * t < TILE + 10} >= set(OFFSETS)
            assert {s % 64 for X, s in steps[L] if 1000 < X < T_LEN - 100} == set(range(64))
        for L in EMU_LENGTHS[si]:
            assert {(len(r), len(r[0])) for r, _, _ in build_calls(si, (L,))} >= {(k, L) for k in (1, 2, 3, 4)}


@pytest.mark.parametrize("si", [0, 1], ids=["2_2_3_1", "1_3_5_2"])
def test_no_case_is_vacuous(si):
    match, mism, gO, gE = SCORINGS[si]
    for reads, target, ends in build_calls(si):
        for rd, X in zip(reads, ends):
            L = len(rd)
            lo, hi = _window(X, L, SCORINGS[si])
            cm8, cm16, _, _ = _plain_dp(rd.tolist(), target[lo:hi].tolist(), match, mism, gO, gE, (L + 15) // 16 * 16)
            at = [j for j in range(X - lo, hi - lo) if cm16[j] > cm8[j]]
            assert at, ("vacuous case: the padded rows raise no column maximum in X .. X + 7", X, L, SCORINGS[si])
    reads, target = build_repeat_call(si)
    cm8, cm16, _, _ = _plain_dp(reads[0].tolist(), target[1400:2400].tolist(), match, mism, gO, gE, 160)
    run = best = 0
    for a, b in zip(cm16, cm8):
        run = run + 1 if a > b else 0
        best = max(best, run)
    inside = sum(a > b for a, b in zip(cm16[640:900], cm8[640:900]))      # columns 2040 .. 2299
    assert inside >= 100 and best >= (40 * match - gO) // gE - 8, ("the repeat does not raise the maxima of consecutive groups", inside, best)


def run_calls(ctx, si, lengths=(150, 101)):
    """every call of scoring si through ctx, every record against the reference; returns the number of calls"""
    match, mism, gO, gE = SCORINGS[si]
    mat = dna_matrix(match, mism)
    calls = [(r, t) for r, t, _ in build_calls(si, lengths)] + [build_repeat_call(si)]
    for reads, target in calls:
        Q = ctx.upload(reads); T = ctx.upload([target])
        try:
            res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, 0, 0, 0, -1, 2)
        finally:
            Q.free(); T.free()
        tm = ctx.timing()
        lens = [len(r) for r in reads]
        assert tm["fill_kernel"].startswith("k_fill8<"), (tm["fill_kernel"], lens)
        assert tm["n_byte"] == len(reads), (tm["n_byte"], tm["n_word"], lens)      # only those read the closed form
        bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, 0, 0, 0, -1, 2)
        assert not bad, "%s lens %s: " % (SCORINGS[si], lens) + "\n".join(bad)
    return len(calls)


# ---- the kernel source on the emulator -------------------------------------------------------------------------------------------------

_EMU_CODE = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill_half_flush as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
n = sum(m.run_calls(ctx, si, m.EMU_LENGTHS[si]) for si in (0, 1))
ctx.close()
print("ok", n)
'''


@pytest.mark.parametrize("K", ["16", "64"])
def test_flush_sweep_on_the_emulator(emu_lib_path, K):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


# ---- on the device ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("si", [0, 1], ids=["2_2_3_1", "1_3_5_2"])
@pytest.mark.parametrize("K", ["16", "64"])
def test_flush_sweep_with_renormalisations_gpu(gpu_hctx, monkeypatch, si, K):
    monkeypatch.setenv("SSW_GPU_FRAME_K", K)      # (a hook of libssw_hooks.so, read at every call)
    monkeypatch.setenv("SSW_GPU_NO_DB", "1")
    run_calls(gpu_hctx, si)


@pytest.mark.gpu
@pytest.mark.parametrize("si", [0, 1], ids=["2_2_3_1", "1_3_5_2"])
def test_flush_sweep_product_library_gpu(gpu_ctx, si):
    run_calls(gpu_ctx, si)
