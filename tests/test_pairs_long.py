"""Long reads (769 residues and more) on the fused pair / window path: the pair mode of the strip kernel (k_chainq<R,pairs,form>), its
reduction (k_reduce_pairs) and the third class of the planner (pairs_core, csrc/ssw_host.c).

Every case goes through ONE helper (_ways): Context.align_pairs on the targets as sequences of their own, Context.align_windows with the same
targets laid inside resident sequences at odd and even offsets with foreign residues on both sides (test_pairs_regimes._lay_out) and, where
the case asks for it, Context.align_windows_best with one candidate per group.  align_pairs must equal parity.expected() -- the compiled
reference -- for EVERY pair: all RES_FIELDS, the CIGAR words, status 1 exactly where the reference returns NULL; the other two must equal
align_pairs in every field but cigar_off and in the pool words.  The helper splits the list by planner class -- "long" (gapO > gapE, n <= 32,
queries of 769 .. 65 535 residues, targets of 1 .. 65 000 columns, a job's scratch within half the budget), "short" (k_fillpairs' envelope),
"fallback" (the rest, 641 .. 768 residues among it) --, runs the classes as calls of their own and asserts the path of each: the long class
reports "k_chainq<R,pairs,frame|int16> x S strips[ + 1 of T]" with R, S, T as win_bucket_shape gives them (_shape mirrors it), win_copied 0
and the n_word / n_byte counts that follow from the reference's scores.  On the parent commit these pairs took the fallback (another kernel
name, win_copied > 0 for windows), so the path assertions fail there.

Families: 1 gate, 2 strip shapes, 3 register halves, 4 rules, 5 forms and ticket modes, 6 flags, 7 align_windows_best, 8 mixed list in one
call, 9 budget.  Emulator halves (`not gpu`): reads of 769 .. 1 700 residues, windows up to ~2 000 columns; GPU halves: every family in full."""
import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, mutate
from test_pairs_regimes import FIELDS, _cig, _lay_out, _mat, _rand, _same, _subst, in_envelope
from test_windows_best import _check as _best_check, _revcomp


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the planner, mirrored

def _shape(qlen, n):
    """win_geom_fill / win_bucket_key / win_bucket_shape of csrc/ssw_host.c -> (rows per lane, strips, rows per lane of a tail strip or 0)"""
    x = min(max(24 // (n + 1), 1), 3)
    xr = 4 * x
    while xr > 4 and n * ((xr + 3) // 4) * 1024 > 65535:
        xr -= 4
    P = -(-qlen // 16) * 16
    S = -(-P // (64 * xr))
    R, tail = -(-P // (64 * S)), 0
    if S > 1 and xr > 4:
        rem = P - (S - 1) * 64 * xr
        need = -(-rem // 64)
        tr = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 0
        if rem > 0 and tr > 0 and xr * (S - 1) + tr < R * S:
            R, tail = xr, tr
    return R, S, tail


def _kname(shape, form):
    R, S, tail = shape
    return "k_chainq<%d,pairs,%s> x %d strips" % (R, form, S - 1 if tail else S) + (" + 1 of %d" % tail if tail else "")


def _job_bytes(tl, strips):
    return 8 * ((tl + 15) // 16 * 16 + 16) + 16 * ((tl + 31) // 16 * 16) + 36 * strips + 32 + 2 * ssw_amd.RESULT_DTYPE.itemsize


def _klass(qlen, tlen, n, mat, gapO, gapE, budget):
    if gapO > gapE and n <= 32 and 769 <= qlen <= 65535 and 1 <= tlen <= 65000 and _job_bytes(tlen, _shape(qlen, n)[1]) <= budget // 2:
        return "long"
    return "short" if in_envelope(qlen, tlen, n, mat, gapO, gapE) else "fallback"


def _ref_all(reads, targets, qidx, tidx, mat, n, kw):
    gapO, gapE, flag = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("flag", 0)
    filters, filterd, ml, ss = kw.get("filters", 0), kw.get("filterd", 0), kw.get("maskLen", -1), kw.get("score_size", 2)
    return [expected(reads[q], mat, n, targets[t], gapO, gapE, flag, filters, filterd, ml if ml >= 0 else len(reads[q]) // 2, ss)
            for q, t in zip(qidx, tidx)]


def _against_ref(tag, res, cig, ix, ref, reads, targets, qidx, tidx, bad, mark=False):
    for k, i in enumerate(ix):
        exp, ecig = ref[i]
        g = res[k]
        if exp is None:
            ok = int(g["status"]) == 1
        elif mark:      # mark_mismatch rewrites the CIGAR (M -> = / X, soft clips): positions and scores stay the reference's
            ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS if f != "cigarLen"} == {f: v for f, v in exp.items() if f != "cigarLen"}
        else:
            ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp and _cig(g, cig) == ecig
        if not ok and len(bad) < 4:
            bad.append("%s pair %d (read %d x target %d columns): reference %s %s, got %s %s" % (
                tag, i, len(reads[qidx[i]]), len(targets[tidx[i]]), exp, cigar_str(ecig), g, cigar_str(_cig(g, cig))))


def _ways(ctx, reads, targets, qidx, tidx, mat, n, best=False, ncodes=None, budget=0, form=None, **kw):
    """-> (reference answers in pair order, {class: timing of align_pairs})"""
    qidx = np.asarray(qidx, dtype=np.int32); tidx = np.asarray(tidx, dtype=np.int32)
    ncodes = ncodes if ncodes is not None else (4 if n == 5 else n)
    gapO, gapE, ss = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("score_size", 2)
    ref = _ref_all(reads, targets, qidx, tidx, mat, n, kw)
    rng = np.random.default_rng(len(targets) * 7919 + len(reads))
    resident, wseq, wbeg = _lay_out(targets, rng, ncodes)
    tlen = np.array([len(targets[t]) for t in tidx], dtype=np.int32)
    minmat = int(np.min(mat))
    bias = -minmat if minmat < 0 else 0
    timings = {}
    Q = ctx.upload(reads); T = ctx.upload(targets); W = ctx.upload(resident)
    try:
        ctx.lib.ssw_gpu_set_budget(ctx.h, budget)
        bytes_ = int(ctx.lib.ssw_gpu_get_budget(ctx.h))
        klass = np.array([_klass(len(reads[q]), len(targets[t]), n, mat, gapO, gapE, bytes_) for q, t in zip(qidx, tidx)])
        for side in ("long", "short", "fallback"):
            ix = np.nonzero(klass == side)[0]
            if len(ix) == 0:
                continue
            q, t = qidx[ix], tidx[ix]
            bad = []
            ares, acig = ctx.align_pairs(Q, T, q, t, mat, n, **kw)
            tms = [("pairs", ctx.timing())]
            timings[side] = tms[0][1]
            _against_ref("pairs", ares, acig, ix, ref, reads, targets, qidx, tidx, bad, kw.get("mark_mismatch", False))
            bres, bcig = ctx.align_windows(Q, W, q, wseq[t], wbeg[t], tlen[ix], mat, n, **kw)
            tms.append(("windows", ctx.timing()))
            for k, i in enumerate(ix):
                _same("windows", ares[k], acig, bres[k], bcig, i, bad)
            if best:
                sel, cres, ccig = ctx.align_windows_best(Q, W, np.arange(len(ix) + 1), q, wseq[t], wbeg[t], tlen[ix], mat, n, **kw)
                tms.append(("windows_best", ctx.timing()))
                for k, i in enumerate(ix):
                    a = ares[k]
                    if int(a["status"]) == 0 and int(a["score1"]) > 0:
                        _same("windows_best", a, acig, cres[k], ccig, i, bad)
                        want = (0, -1, 1, 0)
                    else:
                        pad = {f: 0 for f in FIELDS}; pad["ref_begin1"] = pad["read_begin1"] = -1
                        if {f: int(cres[k][f]) for f in FIELDS} != pad or int(cres[k]["cigar_off"]) != -1:
                            bad.append("windows_best pair %d: padding record expected, got %s" % (i, cres[k]))
                        want = (-1, -1, 0, 0)
                    if tuple(int(sel[k][f]) for f in ("best", "second", "n_eligible", "second_score1")) != want:
                        bad.append("windows_best pair %d: selection %s, expected %s" % (i, sel[k], want))
            assert not bad, "\n".join(bad[:6])
            scored = [ref[i][0]["score1"] for i in ix if ref[i][0] is not None and ref[i][0]["score1"] > 0]
            n_word = sum(1 for s in scored if ss == 1 or (ss == 2 and s >= 255 - bias))
            shapes = set(_shape(len(reads[qq]), n) for qq in q)
            for who, tm in tms:
                name = tm["fill_kernel"]
                if side == "long":
                    assert name.startswith("k_chainq<") and ",pairs," in name and tm["win_copied"] == 0, (who, name, tm["win_copied"])
                    assert (tm["fill_rows_per_lane"], tm["fill_strips"]) in set((R, S) for R, S, _ in shapes), (who, name, tm["fill_strips"], shapes)
                    if len(shapes) == 1:
                        assert name in [_kname(min(shapes), f) for f in ((form,) if form else ("frame", "int16"))], (who, name, shapes)
                    assert (tm["n_word"], tm["n_byte"]) == (n_word, len(scored) - n_word), (who, tm["n_word"], tm["n_byte"], n_word, len(scored))
                elif side == "short":
                    assert name.startswith("k_fillpairs<") and tm["win_copied"] == 0, (who, name)
                else:
                    assert not name.startswith("k_fillpairs<") and ",pairs," not in name, (who, name)
                    if who != "pairs" and any(len(targets[x]) > 0 for x in t):
                        assert tm["win_copied"] > 0, (who, tm["win_copied"])
    finally:
        ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        Q.free(); T.free(); W.free()
    return ref, timings


MAT = dna_matrix(2, 2)


def _indel_read(rng, src, ncodes=4):
    """a read with substitutions, insertions and deletions (the CIGAR has I and D)"""
    return np.ascontiguousarray(mutate(src, rng, 0.03, 0.01, 0.01, ncodes), dtype=np.int8)


def _planted(rng, qlen, tcols, ncodes=4, indel=True):
    """-> (read of exactly qlen residues, target of tcols columns that holds its source)"""
    t = _rand(rng, tcols, ncodes)
    off = int(rng.integers(0, max(tcols - qlen - 40, 1)))
    src = t[off:off + qlen + 40]
    rd = _indel_read(rng, src, ncodes)[:qlen] if indel else src[:qlen].copy()
    if len(rd) < qlen:
        rd = np.concatenate([rd, _rand(rng, qlen - len(rd), ncodes)])
    return np.ascontiguousarray(rd, dtype=np.int8), t


# ------------------------------------------------------------------------------------------------------------------ 1 gate

def _gate(ctx, tcols):
    """768 / 769 residues against the same windows; n = 32 / 33; gapO = gapE"""
    rng = np.random.default_rng(9100)
    t0, t1 = _rand(rng, tcols), _rand(rng, tcols - 37)
    reads = [_indel_read(rng, t0[20:20 + 830])[:768], _indel_read(rng, t0[20:20 + 830])[:769], _indel_read(rng, t1[5:5 + 830])[:768], _indel_read(rng, t1[5:5 + 830])[:769]]
    assert [len(r) for r in reads] == [768, 769, 768, 769]
    for flag in (0, 2):
        ref, tms = _ways(ctx, reads, [t0, t1], [0, 1, 2, 3], [0, 0, 1, 1], MAT, 5, flag=flag)
        assert set(tms) == {"long", "fallback"} and all(e is not None and e["score1"] > 800 for e, _ in ref)
    ref, tms = _ways(ctx, reads, [t0, t1], [1, 3], [0, 1], MAT, 5, gapO=2, gapE=2, flag=2)
    assert set(tms) == {"fallback"}
    for n in (32, 33):
        m = np.full((n, n), -3, dtype=np.int8); np.fill_diagonal(m, 4)
        m = np.ascontiguousarray(m.reshape(-1))
        t = _rand(rng, 900, n)
        rd = _subst(t[11:11 + 800], rng, 0.05, ncodes=n)
        ref, tms = _ways(ctx, [rd], [t], [0], [0], m, n, gapO=6, gapE=2, flag=2)
        assert set(tms) == {"long" if n == 32 else "fallback"} and ref[0][0]["score1"] > 2000
        if n == 32:
            assert tms["long"]["fill_rows_per_lane"] == 4      # (a 32-letter profile: strips of 256 rows)


def test_emu_gate(ectx):
    _gate(ectx, 1100)


@pytest.mark.gpu
def test_gpu_gate(gpu_ctx):
    _gate(gpu_ctx, 3000)


@pytest.mark.gpu
def test_gpu_gate_window_limit(gpu_ctx):
    """65 000 columns: the new path; 65 001: the fallback; a 769-residue read whose exact copy ends on the LAST column"""
    rng = np.random.default_rng(9150)
    reads, targets = [], []
    for L in (65000, 65001):
        t = _rand(rng, L)
        reads.append(t[L - 769:].copy()); targets.append(t)
    for flag in (0, 2):
        ref, tms = _ways(gpu_ctx, reads, targets, [0, 1], [0, 1], MAT, 5, best=flag == 0, flag=flag)
        assert set(tms) == {"long", "fallback"}
        for k, L in enumerate((65000, 65001)):
            assert ref[k][0]["score1"] == 2 * 769 and ref[k][0]["ref_end1"] == L - 1 and ref[k][0]["read_end1"] == 768


# ------------------------------------------------------------------------------------------------------------------ 2 strip shapes

def test_shape_mirror():
    """the cases the issue names, as win_bucket_shape cuts them (DNA: strips of 768 rows; a short last strip where it computes fewer rows)"""
    assert _shape(769, 5) == (12, 2, 1) and _shape(1536, 5) == (12, 2, 0) and _shape(1537, 5) == (12, 3, 1) and _shape(1600, 5) == (12, 3, 1)
    assert _shape(1700, 5) == (9, 3, 0) and _shape(3100, 5)[1] == 5 and _shape(800, 24) == (4, 4, 0) and _shape(1030, 24)[0] == 4
    assert _kname((12, 3, 1), "frame") == "k_chainq<12,pairs,frame> x 2 strips + 1 of 1" and _kname((9, 3, 0), "int16") == "k_chainq<9,pairs,int16> x 3 strips"


def _strip_shapes_dna(ctx, lengths, tcols):
    rng = np.random.default_rng(9200)
    for L in lengths:
        rd, t = _planted(rng, L, tcols)
        rd2, t2 = _planted(rng, L, tcols - 101)
        for flag in (0, 2):
            ref, tms = _ways(ctx, [rd, rd2], [t, t2], [0, 1], [0, 1], MAT, 5, flag=flag)
            assert set(tms) == {"long"} and all(e["score1"] > L for e, _ in ref)
            assert tms["long"]["fill_kernel"] == _kname(_shape(L, 5), "frame")


def _strip_shapes_protein(ctx, lengths, tcols):
    rng = np.random.default_rng(9250)
    for L in lengths:
        t = _rand(rng, tcols, 20)
        rd = _subst(t[9:9 + L], rng, 0.1, ncodes=20)
        for flag in (0, 2):
            ref, tms = _ways(ctx, [rd], [t], [0], [0], blosum50(), 24, ncodes=20, gapO=10, gapE=2, flag=flag)
            assert set(tms) == {"long"} and ref[0][0]["score1"] > 3 * L
            assert tms["long"]["fill_rows_per_lane"] == 4 and tms["long"]["fill_strips"] == _shape(L, 24)[1]


@pytest.mark.parametrize("L", [769, 1536, 1537, 1600, 1700])
def test_emu_strip_shapes_dna(ectx, L):
    _strip_shapes_dna(ectx, [L], L + 260)


def test_emu_strip_shapes_protein(ectx):
    _strip_shapes_protein(ectx, [800, 1030], 1200)


@pytest.mark.gpu
def test_gpu_strip_shapes_dna(gpu_ctx):
    _strip_shapes_dna(gpu_ctx, [769, 1536, 1537, 1600, 1700, 3100], 4000)


@pytest.mark.gpu
def test_gpu_strip_shapes_protein(gpu_ctx):
    _strip_shapes_protein(gpu_ctx, [800, 1030], 2500)


@pytest.mark.gpu
def test_gpu_saturation(gpu_ctx):
    """a 16 500-residue exact copy under match 2 scores 33 000: the 16-bit kernels saturate at 32 767, as the reference does"""
    rng = np.random.default_rng(9280)
    t = _rand(rng, 17000)
    rd = t[250:250 + 16500].copy()
    ref, tms = _ways(gpu_ctx, [rd], [t], [0], [0], MAT, 5, flag=0)
    assert ref[0][0]["score1"] == 32767 and set(tms) == {"long"}


# ------------------------------------------------------------------------------------------------------------------ 3 halves

def _halves(ctx, T):
    """reads of ONE padded length (800 residues: one bucket, jobs pair neighbours): windows of 1 and T columns in one job; a lone query; two
    padded lengths (two jobs); identical and overlapping windows and the same pair twice; and the short half's second best: the long half's
    target holds a second, weaker copy BEYOND the short half's last column"""
    rng = np.random.default_rng(9300 + T)
    long_t = _rand(rng, T)
    rd_long = _indel_read(rng, long_t[T - 860:])[:800]
    one = _rand(rng, 1)
    rd_one = _rand(rng, 800)
    for flag in (0, 2):
        ref, tms = _ways(ctx, [rd_long, rd_one], [long_t, one], [0, 1], [0, 1], MAT, 5, flag=flag)      # unbalanced halves
        assert set(tms) == {"long"} and ref[0][0]["score1"] > 1200 and ref[1][0]["score1"] <= 2
        ref, tms = _ways(ctx, [rd_long], [long_t], [0], [0], MAT, 5, flag=flag)                           # idle half
        assert ref[0][0]["score1"] > 1200
    rd_b = _indel_read(rng, long_t[100:100 + 900])[:830]      # another padded length: a job of its own
    ref, tms = _ways(ctx, [rd_long, rd_b], [long_t], [0, 1], [0, 0], MAT, 5, flag=2)
    assert _shape(800, 5) == _shape(830, 5) == (12, 2, 1) and all(e["score1"] > 1200 for e, _ in ref)
    # two jobs were formed: each computes its 64 x (12 + 1) rows x 2 halves over the T columns; one shared job would count half of this
    assert tms["long"]["fill_cells"] == 2 * (64 * 13 * 2 * T), tms["long"]["fill_cells"]
    # identical and overlapping windows, the same pair twice
    sub_t = np.ascontiguousarray(long_t[T - 1000:])
    ref, tms = _ways(ctx, [rd_long, rd_long.copy()], [long_t, long_t.copy(), sub_t], [0, 1, 0, 0, 1], [0, 1, 2, 0, 2], MAT, 5, best=True, flag=2)
    assert set(tms) == {"long"} and ref[0] == ref[3]
    # second best of the SHORT half: both reads 800 residues; target A (short, 900 columns) holds its read once; target B (T columns) holds
    # its read at the start and a 4 %-substituted copy at column ~T - 850, beyond A's end: with maskLen -1 (400 columns) that copy is B's second best
    rdA, tA = _planted(rng, 800, 900, indel=False)
    tB = _rand(rng, T)
    rdB = tB[30:830].copy()
    tB[T - 850:T - 50] = _subst(rdB, rng, 0.04, at_least=8)
    for maskLen in (15, -1):
        ref, tms = _ways(ctx, [rdA, rdB], [tA, tB], [0, 1], [0, 1], MAT, 5, flag=0, maskLen=maskLen)
        assert ref[1][0]["score2"] > 1000, (ref[0][0], ref[1][0])
        if maskLen < 0:      # (maskLen 15: the shoulder of the best alignment, 15 columns behind its end, is the second best)
            # (A's own second best is half an alignment, ~800; the values that decay from its best cell into the columns behind its target,
            # where its half keeps running beside B's, are still ~1 200 at the end of the mask: a scan past A's last column would report them)
            assert ref[1][0]["ref_end2"] > 900 and ref[0][0]["score2"] < 1000, (ref[0][0], ref[1][0])


def test_emu_halves(ectx):
    _halves(ectx, 2000)


@pytest.mark.gpu
def test_gpu_halves(gpu_ctx):
    _halves(gpu_ctx, 3000)


# ------------------------------------------------------------------------------------------------------------------ 4 rules

def _rules(ctx, tcols, emu):
    rng = np.random.default_rng(9400)
    # len & 15 in {0, 1, 8, 9, 15}: the padded-length rule of the second best and the last strip's mask; an exact copy and a weaker second one
    reads, targets = [], []
    for d in (0, 1, 8, 9, 15):
        rd = _rand(rng, 784 + d)
        targets.append(np.concatenate([_rand(rng, 40 + d), rd, _rand(rng, 30), _subst(rd, rng, 0.05, at_least=5), _rand(rng, 20)]))
        reads.append(rd)
    ids = [3, 1, 4, 0, 2]
    for maskLen, flag in ((-1, 0), (15, 2), (0, 0)):
        ref, tms = _ways(ctx, reads, targets, ids, ids, MAT, 5, flag=flag, maskLen=maskLen)
        for k, i in enumerate(ids):
            e = ref[k][0]
            assert e["score1"] == 2 * len(reads[i]) and (e["score2"] > 0) == (maskLen != 0), (i, e)
        assert set(tms) == {"long"} and tms["long"]["n_word"] == 5
    # score_size 0 / 1 / 2: a long read against a FOREIGN window scores below 255 - bias (8-bit rules), its own window overflows 8 bits
    t = _rand(rng, tcols)
    own = _indel_read(rng, t[50:50 + 850])[:800]
    foreign = _rand(rng, 800)
    for ss in (0, 1, 2):
        ref, tms = _ways(ctx, [own, foreign], [t], [0, 1], [0, 0], MAT, 5, flag=0, score_size=ss)
        assert 0 < (ref[1][0]["score1"] if ref[1][0] else 0) < 253
        assert (ref[0][0] is None) == (ss == 0)      # the overflowing score under 8-bit rules alone: NULL, status 1
        assert (tms["long"]["n_word"], tms["long"]["n_byte"]) == {0: (0, 1), 1: (2, 0), 2: (1, 1)}[ss]


def test_emu_rules(ectx):
    _rules(ectx, 1100, True)


@pytest.mark.gpu
def test_gpu_rules(gpu_ctx):
    _rules(gpu_ctx, 3000, False)


# ------------------------------------------------------------------------------------------------------------------ 5 forms

def _forms(ctx, tcols):
    """the same 1 600-residue reads under a scoring ssw_frame_params accepts (match 2: top 3 200) and one it refuses (match 30: top 48 000)"""
    rng = np.random.default_rng(9500)
    rd, t = _planted(rng, 1600, tcols)
    rd2, t2 = _planted(rng, 1600, tcols - 64)
    for mat, gO, gE, form in ((MAT, 3, 1, "frame"), (_mat(30, 20), 40, 3, "int16")):
        for flag in (0, 2):
            ref, tms = _ways(ctx, [rd, rd2], [t, t2], [0, 1], [0, 1], mat, 5, form=form, gapO=gO, gapE=gE, flag=flag)
            assert tms["long"]["fill_kernel"] == _kname(_shape(1600, 5), form)
            assert all(e["score1"] > 1600 for e, _ in ref)


def test_emu_forms(ectx):
    _forms(ectx, 1900)


@pytest.mark.gpu
def test_gpu_forms(gpu_ctx):
    _forms(gpu_ctx, 2600)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"SSW_GPU_FRAME_K": "16"}, {"SSW_GPU_FRAME_K": "64"}, {"SSW_GPU_QUEUE": "strips"}, {"SSW_GPU_QUEUE": "jobs"}],
                         ids=lambda e: "_".join("%s%s" % (k[8:].lower(), v) for k, v in e.items()))
def test_gpu_forms_hooks(gpu_hctx, monkeypatch, env):
    """the frame renormalised every 16 / 64 steps; both ticket modes of the work queue (records equal: both equal the reference)"""
    rng = np.random.default_rng(9550)
    pairs = [_planted(rng, L, 2600) for L in (1600, 1600, 1600, 1700, 800)]
    reads, targets = [p[0] for p in pairs], [p[1] for p in pairs]
    ids = np.arange(len(pairs))
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        for flag in (0, 2):
            ref, tms = _ways(gpu_hctx, reads, targets, ids, ids, MAT, 5, flag=flag)
            assert set(tms) == {"long"} and "frame" in tms["long"]["fill_kernel"]


# ------------------------------------------------------------------------------------------------------------------ 6 flags

FLAG_KW = [dict(flag=0), dict(flag=2, filters=100), dict(flag=2, filters=30000), dict(flag=15, filterd=32767), dict(flag=15, filterd=820),
           dict(flag=2, mark_mismatch=True)]


def _flags(ctx, kw, tcols, npairs):
    rng = np.random.default_rng(9600)
    pairs = [_planted(rng, int(L), tcols) for L in ([780, 830, 1000, 800, 1100, 800] * 2)[:npairs]]
    reads, targets = [p[0] for p in pairs], [p[1] for p in pairs]
    ids = rng.permutation(len(pairs))
    ref, tms = _ways(ctx, reads, targets, ids, ids, MAT, 5, best=kw["flag"] in (0, 15), **kw)
    assert set(tms) == {"long"} and all(e["score1"] > 1000 for e, _ in ref)
    if kw["flag"] and kw.get("filters", 0) < 30000 and not kw.get("mark_mismatch"):
        cigs = [c for e, c in ref if e["cigarLen"] > 0]
        assert cigs and any((w & 0xf) == 1 for c in cigs for w in c) and any((w & 0xf) == 2 for c in cigs for w in c)      # I and D
        if kw.get("filterd", 32767) < 32767:
            assert any(e["cigarLen"] == 0 for e, _ in ref) and any(e["cigarLen"] > 0 for e, _ in ref)      # filterd drops some
    if kw.get("filters", 0) >= 30000:
        assert all(e["cigarLen"] == 0 and e["ref_begin1"] == -1 for e, _ in ref)


@pytest.mark.parametrize("kw", FLAG_KW, ids=lambda k: "_".join("%s%s" % (a[:5], b) for a, b in k.items()))
def test_emu_flags(ectx, kw):
    _flags(ectx, kw, 1400, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", FLAG_KW, ids=lambda k: "_".join("%s%s" % (a[:5], b) for a, b in k.items()))
def test_gpu_flags(gpu_ctx, kw):
    _flags(gpu_ctx, kw, 2500, 12)


# ------------------------------------------------------------------------------------------------------------------ 7 align_windows_best

def _best_groups(ctx, L, ngroups):
    """groups that mix long-read candidates on both strands, short-read candidates, a 700-residue fallback candidate and an empty window;
    test_windows_best._check: selections and winners' records equal align_windows plus a host top-2, winners equal the reference"""
    rng = np.random.default_rng(9700)
    genome = [_rand(rng, L), _rand(rng, L - 333)]
    fwd, cand_off, qidx, tidx, tbeg, tlen = [], [0], [], [], [], []
    plan = []
    for g in range(ngroups):
        kind = g % 4      # 0: long read, forward; 1: long read from the reverse strand; 2: short read; 3: 700 residues (fallback)
        qlen = (900, 1000, 150, 700)[kind]
        t = g % 2
        off = int(rng.integers(50, len(genome[t]) - qlen - 400))
        src = _indel_read(rng, genome[t][off:off + qlen + 30])[:qlen]
        fwd.append(_revcomp(src) if kind == 1 else src)
        plan.append((kind, t, off, qlen))
    nq = len(fwd)
    reads = fwd + [_revcomp(r) for r in fwd]
    for g, (kind, t, off, qlen) in enumerate(plan):
        for strand in (0, 1):
            for shift in (0, 173):      # the true window and a shifted one that cuts the read's source
                qidx.append(g + strand * nq); tidx.append(t); tbeg.append(max(off - 40 + shift, 0)); tlen.append(qlen + 120)
        if g % 3 == 0:
            qidx.append(g); tidx.append(t); tbeg.append(off); tlen.append(0)      # an empty window
        cand_off.append(len(qidx))
    Q0 = ctx.upload(fwd)
    Q = Q0.with_revcomp()
    T = ctx.upload(genome)
    try:
        for kw in (dict(flag=0), dict(flag=2), dict(flag=15, filterd=32767)):
            sel, res, cig, tm = _best_check(ctx, reads, genome, cand_off, qidx, tidx, tbeg, tlen, MAT, 5, Q=Q, T=T, **kw)
            assert (sel["best"] >= 0).all() and (res["score1"] > 200).all()
            for g, (kind, t, off, qlen) in enumerate(plan):      # the winner is a candidate of the strand the read came from
                assert int(qidx[cand_off[g] + int(sel["best"][g])]) // nq == (1 if kind == 1 else 0), (g, sel[g])
            assert ",pairs," in tm["fill_kernel"] and tm["win_copied"] > 0      # (the long class has the most cells; the 700-residue candidates were copied)
            if kw["flag"]:
                assert tm["best_flagged"] == int((sel["best"] >= 0).sum())
    finally:
        Q.free(); Q0.free(); T.free()


def test_emu_windows_best(ectx):
    _best_groups(ectx, 3000, 4)


@pytest.mark.gpu
def test_gpu_windows_best(gpu_ctx):
    _best_groups(gpu_ctx, 20000, 16)


# ------------------------------------------------------------------------------------------------------------------ 8 mixed list

def _mixed(ctx, tcols, nlong, nshort):
    """short pairs (k_fillpairs), long pairs (pair mode) and fallback pairs (700 residues, an empty query, an empty window) in ONE call in
    shuffled order: records and pool in pair order, equal to the three classes' calls made separately"""
    rng = np.random.default_rng(9800)
    genome = _rand(rng, tcols)
    reads, tb, tl = [], [], []
    for k in range(nlong + nshort + 1):
        qlen = int(rng.integers(769, 1300)) if k < nlong else int(rng.integers(30, 300)) if k < nlong + nshort else 700
        off = int(rng.integers(20, tcols - qlen - 200))
        reads.append(_indel_read(rng, genome[off:off + qlen + 30])[:qlen]); tb.append(off - 15); tl.append(qlen + 100)
    reads.append(np.zeros(0, dtype=np.int8)); tb.append(100); tl.append(300)        # an empty query
    qidx = list(range(len(reads))) + [0]; tb.append(500); tl.append(0)               # the first long read against an empty window
    perm = rng.permutation(len(qidx))
    qidx = np.array(qidx, dtype=np.int32)[perm]; tb = np.array(tb, dtype=np.int64)[perm]; tl = np.array(tl, dtype=np.int32)[perm]
    tix = np.zeros(len(qidx), dtype=np.int32)
    budget = 64 << 30
    klass = np.array([_klass(len(reads[q]), int(l), 5, MAT, 3, 1, budget) for q, l in zip(qidx, tl)])
    assert set(klass) == {"long", "short", "fallback"}
    Q = ctx.upload(reads); T = ctx.upload([genome])
    try:
        for kw in (dict(flag=0), dict(flag=2), dict(flag=15, filterd=32767, mark_mismatch=True)):
            res, cig = ctx.align_windows(Q, T, qidx, tix, tb, tl, MAT, 5, **kw)
            tm = ctx.timing()
            assert ",pairs," in tm["fill_kernel"] and tm["win_copied"] == 700 + 100 + 300      # the long class has the most cells; two windows copied
            offs = [int(r["cigar_off"]) for r in res if int(r["cigarLen"]) > 0]
            assert offs == sorted(offs) and (not offs or offs[0] == 0)                        # the pool is in pair order
            bad = []
            for side in ("long", "short", "fallback"):
                ix = np.nonzero(klass == side)[0]
                sres, scig = ctx.align_windows(Q, T, qidx[ix], tix[ix], tb[ix], tl[ix], MAT, 5, **kw)
                for k, i in enumerate(ix):
                    _same(side, sres[k], scig, res[i], cig, i, bad)
            assert not bad, "\n".join(bad)
            if not kw.get("mark_mismatch"):
                ref = [expected(reads[q], MAT, 5, np.ascontiguousarray(genome[int(b):int(b) + int(l)]), 3, 1, kw["flag"], 0, kw.get("filterd", 0), len(reads[q]) // 2, 2)
                       for q, b, l in zip(qidx, tb, tl)]
                for i, (exp, ecig) in enumerate(ref):
                    g = res[i]
                    assert exp is not None and {f: int(g[f]) for f in RES_FIELDS} == exp and _cig(g, cig) == ecig, (i, exp, g)
    finally:
        Q.free(); T.free()


def test_emu_mixed_list(ectx):
    _mixed(ectx, 4000, 3, 5)


@pytest.mark.gpu
def test_gpu_mixed_list(gpu_ctx):
    _mixed(gpu_ctx, 100000, 40, 200)


# ------------------------------------------------------------------------------------------------------------------ 9 budget

def _budget(lib_path, npairs, tcols, big):
    """a fresh context under the 1 MiB budget: the long jobs need several fill launches, records unchanged; a window whose job does not fit
    half the budget (`big` columns) takes the fallback without error"""
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        rng = np.random.default_rng(9900)
        genome = _rand(rng, max(tcols * 4, big + 2000))
        tb = rng.integers(0, len(genome) - tcols - 1, size=npairs).astype(np.int64)
        tl = np.full(npairs, tcols, dtype=np.int32); tl[::3] -= 33
        reads = [_indel_read(rng, genome[int(b) + 40:int(b) + 40 + 830])[:800] for b in tb]
        qidx = np.arange(npairs, dtype=np.int32); tix = np.zeros(npairs, dtype=np.int32)
        per_launch = (1 << 19) // _job_bytes(tcols, _shape(800, 5)[1])
        assert 1 <= per_launch < (npairs + 1) // 2
        Q = ctx.upload(reads); T = ctx.upload([genome])
        for flag in (0, 2):
            r0, c0 = ctx.align_windows(Q, T, qidx, tix, tb, tl, MAT, 5, flag=flag)
            t0 = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
            r1, c1 = ctx.align_windows(Q, T, qidx, tix, tb, tl, MAT, 5, flag=flag)
            t1 = ctx.timing()
            assert t1["fill_launches"] > 1 and t1["fill_launches"] > t0["fill_launches"] and t1["win_copied"] == 0 and ",pairs," in t1["fill_kernel"]
            assert (r0 == r1).all() and c0.tobytes() == c1.tobytes() and (r0["score1"] > 1200).all()
            if big:      # _job_bytes(big) > 512 KiB: the fallback, no error
                assert _job_bytes(big, 2) > (1 << 19)
                rb, cb = ctx.align_windows(Q, T, qidx[:1], tix[:1], np.array([0], dtype=np.int64), np.array([big], dtype=np.int32), MAT, 5, flag=flag)
                tmb = ctx.timing()
                assert ",pairs," not in tmb["fill_kernel"] and tmb["win_copied"] == big
                ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
                rc, cc = ctx.align_windows(Q, T, qidx[:1], tix[:1], np.array([0], dtype=np.int64), np.array([big], dtype=np.int32), MAT, 5, flag=flag)
                assert ",pairs," in ctx.timing()["fill_kernel"] and (rb == rc).all() and cb.tobytes() == cc.tobytes()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        Q.free(); T.free()
    finally:
        ctx.close()


def test_emu_budget(emu_lib_path):
    _budget(emu_lib_path, 24, 2000, 22000)      # (24 bytes x 22 016 columns: above half of 1 MiB)


@pytest.mark.gpu
def test_gpu_budget(product_lib_path):
    _budget(product_lib_path, 64, 3000, 30000)
