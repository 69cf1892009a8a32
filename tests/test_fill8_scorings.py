"""k_fill8 over the scoring space.  Every trick of the half-row kernel's arithmetic -- the 8-lane chains, the blocked row frame, the 64-bit
pair add with a borrowed profile word, the diagonal-gap form, the class floors -- is exact inside a range that the scoring sets: min(mat),
max(mat), gapE, gapO - gapE and the renormalisation period that ssw_frame_params derives from gapE.  This file sweeps that space at random
and visits its edges one by one (DESIGN.md "Gaps from the diagonal" and "Blocked row frame" name what is guarded here).

THE SWEEP (tests/fill8_cases.py: sweep_case(seed, index), 12 chunks of 96 cases):
    gapE from {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64} -- both sides of every halving of the period (4|5, 8|9, 16|17, 32|33);
    gapO - gapE from {1, 2, 3, 7, 40};  alphabets of 4, 5, 8, 16, 24 and 32 letters;
    asymmetric matrices with a positive diagonal and entries uniform in +-(2 gapE + 2), in [-2 gapE, 11] or in +-20 (clipped to int8), by turns;
    per chunk two cases of R <= 3 with max(mat) of 40, 90 or 127 and one matrix without a positive entry (every score is 0);
    1 to 4 reads of one padded class, 16 (R - 1) + 1 .. 8 residues for R = 1 .. 12: R8 = 1, 3, .. 23, each instance 8 times per chunk;
    flags 0, 1, 2; score_size 0, 1, 2; one random target of 700 to 800 columns over the same alphabet (the smallest at which such a call has
    several tiles).
Why the reference covers all of it: its 8-bit kernel saturates and hands over to the 16-bit one, whose scores here stay below 32767 (at most
192 rows x 127), its gap penalties are uint8 (gapO <= 104) and its profile takes any n.  No case is excused or filtered: the planner keeps
every one of them on k_fill8 (n = 32 and max(mat) = 127 included: nothing had to be narrowed), which every call asserts BY NAME -- with
" dg" if and only if -min(mat) <= 2 gapE, R8 is neither 9 nor 17 and every target code lies in [0, n): the documented contract, written out
in fill8_cases.fill8_name, not read off the planner.  Every record and CIGAR equals the reference's; for flag 0 and score_size 2 score1,
ref_end1 and read_end1 also equal a plain numpy DP, a second witness where the reference itself has seldom been used (gap penalties above 30).
The emulator (one process per chunk and per edge, started together: emu_jobs) and the product library run all cases; the hooks library runs a third each with SSW_GPU_FRAME_K 16 and 64, and its records are
byte-identical under SSW_GPU_FILL_DG=0 (the old form, by name) and under SSW_GPU_FILL_HALF=0 (the 16-lane kernel, by name).

THE EDGES (emulator, and the device through the hooks library):
    period boundaries -- gapE 4, 5, 8, 9, 16, 17, 32, 33 under the default period, gapO = gapE + 1 and gapE + 40, a 150-bp and a 40-bp read
        with an insertion and a deletion of three residues each; the match score is chosen so that the halo covers the whole target, which
        is then ONE tile whose steps pass the period twice (asserted on the timing record's cell count).  The 40-bp read cannot get there
        with an int8 score where K gapE = 4096 (gapE 4, 8, 16, 32): it passes the period once;
    zero crossing of profile words -- matrices that hold every value of {-2gE-1, -2gE, -gE-1, -gE, gE-1, gE, 2gE-1, 2gE} for gE = 1, 2, 5 on
        residue pairs that meet in the rectangle, with two reads of different length in one chain and in both, three reads and a single one;
    the matrix gate -- min(mat) = -2 gE against -2 gE - 1 for gE = 1, 2, 3, the entry on a pair that the alignments use and on a letter that
        occurs nowhere: the gate goes by the matrix, not by the sequences;
    the null-column gate -- codes -1 and n, a resident target called under n = 5, n = 4 and n = 5 again, sets made by with_revcomp and
        ssw_gpu_seqs_revcomp, and an ASCII upload whose table maps an unused character out of range.  The reference cannot take these
        inputs: the oracle is the 16-lane kernel's records, byte for byte, and the plain DP with a null column as "no diagonal".  Such a
        target is asked for scores and ends only (flag 0): the begin and traceback passes index the matrix by the raw code as the reference
        does, outside the matrix for such a code (below it for a negative one), so flags 1 and 2 are outside every domain there;
    the top of the frame with real matrices -- the largest diagonal score at which R8 = 23 still names k_fill8 is FOUND from the names by
        bisection, for three (gapO, gapE, min(mat)), and three perfect 184-bp copies run at it and one above."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from fill8_cases import CHUNKS, GAP_E, PER_CHUNK, SEED, fill8_name, plain_sw, r8_of, sweep_case
from parity import compare_batch, expected, make_reads
from sswutil import random_ref
from test_fill_half import _plain_dp

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")


@contextlib.contextmanager
def _env(**kw):
    """the hooks are read at every call"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _call(ctx, reads, targets, mat, n, gO, gE, flag, score_size=2, T=None):
    """-> (records, CIGAR pool, timing, the records' bytes)"""
    Q = ctx.upload(reads)
    Tn = T if T is not None else ctx.upload(targets)
    try:
        res, cig = ctx.align_batch(Q, Tn, mat, n, gO, gE, flag, 0, 0, -1, score_size)
    finally:
        Q.free()
        if T is None:
            Tn.free()
    return res, cig, ctx.timing(), res.tobytes() + np.asarray(cig).tobytes()


def _check_plain(res, reads, targets, mat, n, gO, gE, what):
    for qi, rd in enumerate(reads):
        for ti, tg in enumerate(targets):
            score, col, row = plain_sw(rd, tg, mat, n, gO, gE)
            g = res[qi, ti]
            assert int(g["score1"]) == score, (what, qi, ti, int(g["score1"]), score)
            if score > 0:
                assert (int(g["ref_end1"]), int(g["read_end1"])) == (col, row), (what, qi, ti, g, col, row)


# ---- the plain DP is the plain DP (CPU) -------------------------------------------------------------------------------------------------------

def test_plain_sw_equals_the_cell_by_cell_dp_and_the_reference():
    """fill8_cases.plain_sw (row by row, any matrix) against tests/test_fill_half.py's cell-by-cell DP on match / mismatch scorings, and against
    the reference's ends on asymmetric matrices with wide gaps"""
    rng = np.random.default_rng(811)
    for match, mism, gO, gE in ((2, 2, 3, 1), (1, 3, 5, 2), (5, 4, 44, 4), (9, 20, 73, 33)):
        target = rng.integers(0, 4, size=240, dtype=np.int8)
        read = make_reads(rng, target, 1, [53], 4, frac_random=0.0)[0]
        mat = np.full((4, 4), -mism, dtype=np.int8); mat[np.diag_indices(4)] = match
        cm8, _, _, _ = _plain_dp(read.tolist(), target.tolist(), match, mism, gO, gE, len(read) + 8)
        score, col, _ = plain_sw(read, target, mat.reshape(-1), 4, gO, gE)
        assert score == max(cm8) and col == cm8.index(score)
    for k in range(12):
        c = sweep_case(SEED, 97 * k + 5)
        for rd in c["reads"]:
            exp, _ = expected(rd, c["mat"], c["n"], c["target"], c["gapO"], c["gapE"], 0, 0, 0, len(rd) // 2, 2)
            score, col, row = plain_sw(rd, c["target"], c["mat"], c["n"], c["gapO"], c["gapE"])
            assert exp["score1"] == score and (score == 0 or (exp["ref_end1"], exp["read_end1"]) == (col, row)), (k, exp, score, col, row)


def test_null_column_of_the_plain_dp():
    """a null column has no diagonal: an alignment crosses it with a gap only"""
    mat = np.full((5, 5), -2, dtype=np.int8); mat[np.diag_indices(5)] = 3
    target = np.array([0, 1, 2, 3, 0, 2, 1, 3, 1, 0, 2, 2, 3, 1, 0, 3], dtype=np.int8)
    read = target.copy()
    assert plain_sw(read, target, mat.reshape(-1), 5, 2, 1) == (48, 15, 15)
    for code in (-1, 5, 9):
        t2 = target.copy(); t2[8] = code
        # residues 0 .. 7 (24), then either stop or pay a deletion AND an insertion to cross: 24 - 2 - 2 + 21 = 41
        assert plain_sw(read, t2, mat.reshape(-1), 5, 2, 1) == (41, 15, 15)
        assert plain_sw(read, t2, mat.reshape(-1), 5, 40, 1)[0] == 24


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------

def chunk_cases(chunk, third=None):
    """the cases of a chunk; third 0 / 1: the third of them that the hooks library runs with SSW_GPU_FRAME_K 16 / 64"""
    idx = range(chunk * PER_CHUNK, (chunk + 1) * PER_CHUNK)
    return [sweep_case(SEED, i) for i in idx if third is None or (i % PER_CHUNK) // 12 % 3 == third]


def run_sweep(ctx, cases, check=True, form="dg"):
    """form "dg": the documented name; "old": k_fill8 without the diagonal-gap form; "16": the 16-lane kernel.  Returns the records' bytes."""
    recs = []
    for c in cases:
        reads, target, mat, n, gO, gE, flag, ss = (c[k] for k in ("reads", "target", "mat", "n", "gapO", "gapE", "flag", "score_size"))
        res, cig, tm, raw = _call(ctx, reads, [target], mat, n, gO, gE, flag, ss)
        what = "case %d (%s, n %d, gaps %d/%d, flag %d, score_size %d, lengths %s)" % (c["index"], c["kind"], n, gO, gE, flag, ss, [len(r) for r in reads])
        assert {r8_of(len(r)) for r in reads} == {c["R8"]}
        if form == "16":
            assert tm["fill_kernel"].startswith("k_fill<"), (tm["fill_kernel"], what)
        else:
            want = fill8_name(c["R8"], mat, gE, target, n) if form == "dg" else "k_fill8<%d,frame>" % c["R8"]
            assert tm["fill_kernel"] == want, (tm["fill_kernel"], want, what)
        recs.append(raw)
        if check:
            bad = compare_batch(res, cig, reads, [target], mat, n, gO, gE, flag, 0, 0, -1, ss)
            assert not bad, what + ": " + "\n".join(bad)
            if c["kind"] == "nonpos":
                assert not res["score1"].any(), what
            if flag == 0 and ss == 2:
                _check_plain(res, reads, [target], mat, n, gO, gE, what)
    return recs


def test_the_generator_covers_what_it_claims():
    gate = {True: 0, False: 0}
    plain = 0
    seen_ge = {}
    for chunk in range(CHUNKS):
        cases = chunk_cases(chunk)
        per = {}
        names = set()
        for c in cases:
            per[c["R8"]] = per.get(c["R8"], 0) + 1
            nm = fill8_name(c["R8"], c["mat"], c["gapE"], c["target"], c["n"])
            names.add(nm.endswith(" dg")); gate[nm.endswith(" dg")] += 1
            m = c["mat"].reshape(c["n"], c["n"])
            assert c["gapO"] > c["gapE"] and 1 <= len(c["reads"]) <= 4 and 700 <= len(c["target"]) <= 800
            assert all(1 <= len(r) - 16 * (c["R8"] // 2) <= 8 and r.min() >= 0 and r.max() < c["n"] for r in c["reads"])
            assert c["target"].min() >= 0 and c["target"].max() < c["n"]
            assert (np.diag(m) > 0).all() if c["kind"] != "nonpos" else m.max() <= 0
            assert 192 * max(int(m.max()), 0) < 32767 and c["gapO"] <= 255
            plain += c["flag"] == 0 and c["score_size"] == 2
            seen_ge.setdefault(c["R8"], set()).add(c["gapE"])
        assert per == {R8: PER_CHUNK // 12 for R8 in range(1, 24, 2)}, per
        assert names == {True, False}, chunk                                             # both outcomes of the gate in every chunk
        assert sum(c["kind"] == "nonpos" for c in cases) == 1 and sum(c["kind"] == "max127" for c in cases) == 6
        thirds = [chunk_cases(chunk, k) for k in (0, 1)]
        assert [len(t) for t in thirds] == [36, 36] and not {c["index"] for c in thirds[0]} & {c["index"] for c in thirds[1]}
        assert all({c["R8"] for c in t} == set(range(1, 24, 2)) for t in thirds)
    assert all(s == set(GAP_E) for s in seen_ge.values())                                # every instance under every gapE
    assert min(gate.values()) > CHUNKS * PER_CHUNK // 4 and plain > 100, (gate, plain)
    a, b = sweep_case(SEED, 500), sweep_case(SEED, 500)
    assert a["mat"].tobytes() == b["mat"].tobytes() and all((x == y).all() for x, y in zip(a["reads"], b["reads"]))
    nsym = sum(not np.array_equal(c["mat"].reshape(c["n"], c["n"]), c["mat"].reshape(c["n"], c["n"]).T) for c in chunk_cases(0))
    assert nsym > PER_CHUNK * 3 // 4                                                      # asymmetric matrices


# ---- the edges: each returns nothing and asserts on the way ---------------------------------------------------------------------------------

def _indel_read(target, at, L):
    """L residues of the target from `at`, with three foreign residues inserted a third of the way down and three residues deleted at two thirds"""
    a, b = L // 3, 2 * L // 3
    seg = target[at:at + L]                                    # a residues, 3 inserted, b - a - 3 more, 3 skipped, the rest
    ins = (seg[a:a + 3] + 2) % 4
    return np.concatenate([seg[:a], ins, seg[a:b - 3], target[at + b:at + L + 3]])[:L].astype(np.int8)


PERIODS = {4: 1024, 5: 512, 8: 512, 9: 256, 16: 256, 17: 128, 32: 128, 33: 64}      # gapE -> the default period (K gapE <= 4096, K >= 64)


def period_cases():
    """(gapE, gapO, read length, match score, target length): the halo P16 + P16 match / gapE covers the target, which is 2 K + P16 columns and more"""
    out = []
    for gE, K in PERIODS.items():
        for L in (150, 40):
            P16 = (L + 15) // 16 * 16
            cols = 2 * K + P16 + 24
            match = ((cols - P16) * gE + P16 - 1) // P16 + 1
            if match > 127:                                     # (40 bp where K gapE = 4096: no int8 score reaches two periods; one, then)
                match = 127; cols = P16 + P16 * match // gE
            for gO in (gE + 1, gE + 40):
                out.append((gE, gO, L, match, cols))
    return out


def test_period_cases_are_what_they_claim():
    cases = period_cases()
    assert len(cases) == 32 and sum(cols >= 2200 for _, _, _, _, cols in cases) == 2 and max(c[4] for c in cases) < 2300
    for gE, gO, L, match, cols in cases:
        K, P16 = PERIODS[gE], (L + 15) // 16 * 16
        assert K * gE <= 4096 and (K == 64 or 2 * K * gE > 4096) and K <= 1024
        assert P16 + P16 * match // gE + 1 >= cols and match <= 127              # the halo covers the target: one tile
        assert cols >= 2 * K + P16 or (L == 40 and K * gE == 4096 and match == 127 and cols > K + P16)


def run_periods(ctx, gE):
    for ge, gO, L, match, cols in period_cases():
        if ge != gE:
            continue
        mat = np.full((5, 5), -3, dtype=np.int8); mat[np.diag_indices(5)] = match; mat[4, :] = mat[:, 4] = 0
        target = random_ref(cols, 8100 + gE + L, 4)
        reads = [_indel_read(target, cols - L - 40, L), _indel_read(target, cols // 2, L - 2)]
        for flag in (1, 2):
            res, cig, tm, _ = _call(ctx, reads, [target], mat.reshape(-1), 5, gO, gE, flag)
            assert tm["fill_kernel"] == fill8_name(r8_of(L), mat, gE, target, 5), (tm["fill_kernel"], gE, gO, L)
            # (one chain of two reads: every column once, no halo computed twice)
            assert tm["fill_cells"] == cols * 8 * r8_of(L) * len(reads), ("the target is not one tile", tm["fill_cells"], cols, L)
            bad = compare_batch(res, cig, reads, [target], mat.reshape(-1), 5, gO, gE, flag, 0, 0, -1, 2)
            assert not bad, "period gapE %d gapO %d %d bp: " % (gE, gO, L) + "\n".join(bad)
            assert flag != 2 or all("I" in _cig(res, cig, q) or "D" in _cig(res, cig, q) for q in range(2))      # (gaps are on the path)


def _cig(res, cig, q):
    from sswutil import cigar_str
    off, ln = int(res[q, 0]["cigar_off"]), int(res[q, 0]["cigarLen"])
    return cigar_str([int(x) for x in cig[off:off + ln]])


def zero_values(gE):
    return [-2 * gE - 1, -2 * gE, -gE - 1, -gE, gE - 1, gE, 2 * gE - 1, 2 * gE]


def zero_matrix(gE, beyond):
    """5 x 5, asymmetric: the non-negative values on the diagonal (a positive one in every place), all eight -- seven without -2 gE - 1 when the
    matrix is to stay inside the gate -- on the other twenty entries, by turns"""
    vals = [v for v in zero_values(gE) if beyond or v != -2 * gE - 1]
    m = np.zeros((5, 5), dtype=np.int8)
    k = 0
    for i in range(5):
        for j in range(5):
            if i != j:
                m[i, j] = vals[k % len(vals)]; k += 1
    pos = [v for v in zero_values(gE) if v > 0]
    m[np.diag_indices(5)] = [pos[i % len(pos)] for i in range(5)]
    assert set(vals) <= {int(x) for x in m.reshape(-1)} and m.min() == (-2 * gE - 1 if beyond else -2 * gE)
    return m.reshape(-1).copy()


ZERO_LENGTHS = ((150, 146), (150, 145, 152), (147,), (152, 145, 149, 151), (40, 34), (38, 40, 33), (36,), (40, 33, 37, 39), (24, 17), (20,))


@pytest.mark.parametrize("gE", [1, 2, 5])
def test_zero_matrices_put_profile_entries_on_both_sides_of_zero(gE):
    """build_profile8 adds fr = (1 + class(r) - class(r - 1)) gapE to an entry: 2 gapE into classes 1 to 3, -2 gapE into class 0 and (1 - KL) gapE
    into a position's first row.  For every fr of the instances that run, the matrix holds the entries that make mat + fr 0 and -1"""
    for beyond in (False, True):
        have = {int(x) for x in zero_matrix(gE, beyond)}
        for lens in ZERO_LENGTHS:
            R8 = r8_of(lens[0])
            assert {r8_of(L) for L in lens} == {R8} and all(a != b for a, b in zip(lens[::2], lens[1::2]))      # the two reads of a chain differ
            for fr in {2 * gE, -2 * gE, (1 - (R8 - 1) % 4) * gE}:
                want = {-fr, -fr - 1} - ({-2 * gE - 1} if not beyond else set())
                assert want <= have, (gE, R8, fr, want - have)
    assert {len(lens) for lens in ZERO_LENGTHS} == {1, 2, 3, 4}


def run_zero_crossing(ctx, gE):
    rng = np.random.default_rng(8200 + gE)
    for beyond in (False, True):
        mat = zero_matrix(gE, beyond)
        for k, lens in enumerate(ZERO_LENGTHS):
            target = rng.integers(0, 5, size=760, dtype=np.int8)
            reads = make_reads(rng, target, len(lens), lens, 5, sub=0.15, frac_random=0.0)
            assert all(set(range(5)) <= set(r.tolist()) for r in reads if len(r) > 100) and set(range(5)) <= set(target.tolist())
            gO, flag = gE + (1, 3)[k % 2], (0, 1, 2)[k % 3]
            res, cig, tm, _ = _call(ctx, reads, [target], mat, 5, gO, gE, flag)
            assert tm["fill_kernel"] == "k_fill8<%d,frame>%s" % (r8_of(lens[0]), "" if beyond else " dg"), (tm["fill_kernel"], gE, lens)
            bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, flag, 0, 0, -1, 2)
            assert not bad, "zero crossing gapE %d %s %s: " % (gE, lens, "beyond" if beyond else "inside") + "\n".join(bad)
            if flag == 0:
                _check_plain(res, reads, [target], mat, 5, gO, gE, ("zero crossing", gE, lens))


def run_matrix_gate(ctx, gE):
    """six letters, the sixth in no sequence.  The minimal entry on (0, 1), which every alignment with a substitution meets, or on (5, 2)"""
    rng = np.random.default_rng(8300 + gE)
    target = rng.integers(0, 5, size=740, dtype=np.int8)
    reads = make_reads(rng, target, 3, [150, 148, 151], 5, sub=0.12, frac_random=0.0)
    for low, dg in ((-2 * gE, True), (-2 * gE - 1, False)):
        for place in ((0, 1), (5, 2)):
            mat = np.full((6, 6), -gE, dtype=np.int8); mat[np.diag_indices(6)] = 3; mat[place] = low
            assert mat.min() == low and not (target == 5).any() and not any((r == 5).any() for r in reads)
            for flag in (0, 2):
                res, cig, tm, _ = _call(ctx, reads, [target], mat.reshape(-1), 6, gE + 2, gE, flag)
                assert tm["fill_kernel"] == "k_fill8<19,frame>" + (" dg" if dg else ""), (tm["fill_kernel"], gE, low, place)
                bad = compare_batch(res, cig, reads, [target], mat.reshape(-1), 6, gE + 2, gE, flag, 0, 0, -1, 2)
                assert not bad, "matrix gate gapE %d min %d at %s: " % (gE, low, place) + "\n".join(bad)


def _dna5(match=3, mism=2):
    m = np.full((5, 5), -mism, dtype=np.int8); m[np.diag_indices(5)] = match; m[4, :] = m[:, 4] = 0
    return m


def _against_16_lanes(ctx, reads, targets, mat, n, gO, gE, name, what, T=None, plain_targets=None):
    """by the expected name; the records are those of the 16-lane kernel, and the ends those of the plain DP.  A target with a code outside
    the alphabet is asked for scores and ends only (flag 0): the passes behind the fill index the matrix by the raw code, as the reference
    does, which reads beside the matrix -- below it for a negative code, where the emulator stops the run"""
    legal = all(len(t) == 0 or (t.min() >= 0 and t.max() < n) for t in (plain_targets if plain_targets is not None else targets))
    for flag in (0, 2) if legal else (0,):
        res, cig, tm, raw = _call(ctx, reads, targets, mat, n, gO, gE, flag, T=T)
        assert tm["fill_kernel"] == name, (tm["fill_kernel"], name, what)
        with _env(SSW_GPU_FILL_HALF="0"):
            _, _, tm16, raw16 = _call(ctx, reads, targets, mat, n, gO, gE, flag, T=T)
        assert tm16["fill_kernel"].startswith("k_fill<"), (tm16["fill_kernel"], what)
        assert raw == raw16, what
        if flag == 0:
            _check_plain(res, reads, plain_targets if plain_targets is not None else targets, mat, n, gO, gE, what)
    return res


def _wrap(ctx, h, like):
    import ssw_amd
    s = object.__new__(ssw_amd.Seqs)
    s.ctx, s.count, s.lengths, s.h = ctx, like.count, like.lengths, h
    assert h, ctx.error()
    return s


def _revcomp(t):
    t = np.asarray(t)[::-1]
    return np.where((t >= 0) & (t < 4), 3 - t, t).astype(np.int8)


def run_null_columns(ctx):
    rng = np.random.default_rng(8400)
    clean = rng.integers(0, 5, size=750, dtype=np.int8)                     # codes 0 .. 4
    reads = [np.where(r == 4, 0, r).astype(np.int8) for r in make_reads(rng, clean, 3, [150, 147, 152], 4, frac_random=0.0)]
    assert max(int(r.max()) for r in reads) == 3 and (clean == 4).any()     # reads over 0 .. 3: legal under n = 4 too
    m5, m4 = _dna5().reshape(-1), np.ascontiguousarray(_dna5()[:4, :4]).reshape(-1)
    # codes -1 and n
    for code in (-1, 5):
        t = clean.copy(); t[[200, 377, 378]] = code
        res = _against_16_lanes(ctx, reads, [t], m5, 5, 3, 1, "k_fill8<19,frame>", "code %d" % code)
        assert res["score1"].max() > 100
    # one resident target, the gate changes with the call
    T = ctx.upload([clean])
    try:
        for n, mat in ((5, m5), (4, m4), (5, m5)):
            _against_16_lanes(ctx, reads, [clean], mat, n, 3, 1, "k_fill8<19,frame>" + (" dg" if n == 5 else ""), "resident target under n = %d" % n, T=T)
            if n == 5:
                res, cig, _, _ = _call(ctx, reads, [clean], mat, n, 3, 1, 2, T=T)
                assert not compare_batch(res, cig, reads, [clean], mat, 5, 3, 1, 2, 0, 0, -1, 2)
    finally:
        T.free()
    # sets made on the device from a resident set
    dirty = clean.copy(); dirty[300] = 9
    for t, dg in ((np.where(clean == 4, 0, clean).astype(np.int8), True), (clean, True), (dirty, False)):
        S = ctx.upload([t])
        both = S.with_revcomp()
        rc = _wrap(ctx, ctx.lib.ssw_gpu_seqs_revcomp(ctx.h, S.h), S)
        try:
            name = "k_fill8<19,frame>" + (" dg" if dg else "")
            _against_16_lanes(ctx, reads, [t, _revcomp(t)], m5, 5, 3, 1, name, "with_revcomp, dg %d" % dg, T=both)
            _against_16_lanes(ctx, reads, [_revcomp(t)], m5, 5, 3, 1, name, "seqs_revcomp, dg %d" % dg, T=rc)
            if dg:
                res, cig, _, _ = _call(ctx, reads, None, m5, 5, 3, 1, 2, T=both)
                assert not compare_batch(res, cig, reads, [t, _revcomp(t)], m5, 5, 3, 1, 2, 0, 0, -1, 2)
        finally:
            S.free(); both.free(); rc.free()
    # an ASCII upload takes the range of its table: a character that no sequence holds, mapped out of range, keeps the old form
    text = bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[clean])
    off = np.array([0, len(text)], dtype=np.int64)
    raws = []
    for stray, dg in ((4, True), (9, False), (-1, False)):
        table = np.full(128, 4, dtype=np.int8)
        for ch, v in zip("ACGT", range(4)):
            table[ord(ch)] = v
        table[ord("#")] = stray
        like = ctx.upload([clean])
        T = _wrap(ctx, ctx.lib.ssw_gpu_seqs_upload_ascii(ctx.h, text, off.ctypes.data_as(C.POINTER(C.c_int64)), 1, table.ctypes.data_as(C.POINTER(C.c_int8))), like)
        like.free()
        try:
            res, cig, tm, raw = _call(ctx, reads, None, m5, 5, 3, 1, 2, T=T)
        finally:
            T.free()
        assert tm["fill_kernel"] == "k_fill8<19,frame>" + (" dg" if dg else ""), (tm["fill_kernel"], stray)
        assert not compare_batch(res, cig, reads, [clean], m5, 5, 3, 1, 2, 0, 0, -1, 2)
        raws.append(raw)
    assert raws[0] == raws[1] == raws[2]


TOP_TRIPLES = ((130, 90, -128), (200, 150, -30), (241, 240, -100))      # gapO, gapE, min(mat)


def run_top_of_frame(ctx, ti):
    gO, gE, low = TOP_TRIPLES[ti]
    rng = np.random.default_rng(8500 + ti)
    target = random_ref(760, 8510 + ti, 4)
    reads = [target[500:684].copy(), target[3:187].copy(), target[290:474].copy()]
    base = rng.integers(low, 1, size=(5, 5)); base[1, 3] = low; base[4, :] = 0

    def call(match):
        mat = base.copy(); mat[np.diag_indices(4)] = match; mat[4, 4] = 1
        mat = np.ascontiguousarray(mat.astype(np.int8).reshape(-1))
        res, cig, tm, _ = _call(ctx, reads, [target], mat, 5, gO, gE, 1)
        return mat, res, cig, tm["fill_kernel"]

    assert -low <= 2 * gE
    lo, hi = 1, 127                                                       # the largest match score that still names k_fill8: found, not computed
    assert call(lo)[3] == "k_fill8<23,frame> dg" and not call(hi)[3].startswith("k_fill8")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if call(mid)[3].startswith("k_fill8"):
            lo = mid
        else:
            hi = mid
    for match, half in ((lo, True), (lo + 1, False)):
        mat, res, cig, name = call(match)
        assert (name == "k_fill8<23,frame> dg") == half and (half or name.startswith("k_fill<12,")), (name, match, TOP_TRIPLES[ti])
        assert [int(x) for x in res["score1"][:, 0]] == [184 * match] * 3
        bad = compare_batch(res, cig, reads, [target], mat, 5, gO, gE, 1, 0, 0, -1, 2)
        assert not bad, "top of the frame %s match %d: " % (TOP_TRIPLES[ti], match) + "\n".join(bad)
    return lo


EDGES = {"periods": (run_periods, (4, 5, 8, 9, 16, 17, 32, 33)), "zero": (run_zero_crossing, (1, 2, 5)), "gate": (run_matrix_gate, (1, 2, 3)),
         "null": (run_null_columns, None), "top": (run_top_of_frame, (0, 1, 2))}
EDGE_IDS = [(k, a) for k, (_, args) in EDGES.items() for a in (args or (None,))]


def run_edge(ctx, kind, arg):
    fn = EDGES[kind][0]
    return fn(ctx) if arg is None else fn(ctx, arg)


# ---- on the emulator ------------------------------------------------------------------------------------------------------------------------

_EMU_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
import test_fill8_scorings as m
ctx = ssw_amd.Context(0, ssw_amd.load(%r))
what = os.environ["FILL8_WHAT"].split(":")
if what[0] == "sweep":
    n = len(m.run_sweep(ctx, m.chunk_cases(int(what[1]))))
else:
    n = m.run_edge(ctx, what[0], None if what[1] == "" else int(what[1]))
ctx.close()
print("ok", n)
'''


def _emu(emu_lib_path, what):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", FILL8_WHAT=what)
    for k in ("SSW_GPU_FRAME_K", "SSW_GPU_FILL_DG", "SSW_GPU_FILL_HALF"):
        e.pop(k, None)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)


EMU_WORKERS = 4
EMU_TESTS = ("test_sweep_on_the_emulator", "test_edge_on_the_emulator")


@pytest.fixture(scope="module")
def emu_jobs(request, emu_lib_path):
    """what -> the finished emulator process.  The runs are independent processes of 3 to 20 s each, some five minutes in a row: those of the
    tests that this session selected start together, EMU_WORKERS at a time, and every test takes its own.  (An xdist worker cannot know its
    share of the tests: there each run starts when its test asks for it.)"""
    from concurrent.futures import ThreadPoolExecutor
    jobs = {}
    if not hasattr(request.config, "workerinput"):
        mine = [it.callspec.params["what"] for it in request.session.items
                if getattr(it, "originalname", None) in EMU_TESTS and it.module is request.module and hasattr(it, "callspec")]
        pool = ThreadPoolExecutor(max_workers=EMU_WORKERS)
        request.addfinalizer(lambda: pool.shutdown(wait=False, cancel_futures=True))
        jobs = {w: pool.submit(_emu, emu_lib_path, w) for w in mine}

    def get(what):
        return jobs[what].result() if what in jobs else _emu(emu_lib_path, what)
    return get


def _emu_ok(r):
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("what", ["sweep:%d" % c for c in range(CHUNKS)], ids=[str(c) for c in range(CHUNKS)])
def test_sweep_on_the_emulator(emu_jobs, what):
    _emu_ok(emu_jobs(what))


@pytest.mark.parametrize("what", ["%s:%s" % (k, "" if a is None else a) for k, a in EDGE_IDS],
                         ids=["%s_%s" % e if e[1] is not None else e[0] for e in EDGE_IDS])
def test_edge_on_the_emulator(emu_jobs, what):
    _emu_ok(emu_jobs(what))


# ---- on the device --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_product_library_gpu(gpu_ctx, chunk):
    run_sweep(gpu_ctx, chunk_cases(chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
@pytest.mark.parametrize("K", ["16", "64"])
def test_sweep_hooks_library_gpu(gpu_hctx, K, chunk):
    cases = chunk_cases(chunk, ("16", "64").index(K))
    with _env(SSW_GPU_NO_DB="1", SSW_GPU_FRAME_K=K):
        recs = run_sweep(gpu_hctx, cases)
        with _env(SSW_GPU_FILL_DG="0"):
            assert run_sweep(gpu_hctx, cases, check=False, form="old") == recs
        with _env(SSW_GPU_FILL_HALF="0"):
            assert run_sweep(gpu_hctx, cases, check=False, form="16") == recs


@pytest.mark.gpu
@pytest.mark.parametrize("kind,arg", EDGE_IDS, ids=["%s_%s" % e if e[1] is not None else e[0] for e in EDGE_IDS])
def test_edge_hooks_library_gpu(gpu_hctx, kind, arg):
    with _env(SSW_GPU_NO_DB="1"):
        run_edge(gpu_hctx, kind, arg)
