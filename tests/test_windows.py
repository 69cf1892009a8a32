"""ssw_gpu_align_windows: (query, window of a resident target) pairs (include/ssw_gpu.h).

Record i must equal, bit for bit, what ssw_gpu_align_pairs gives for query qidx[i] against residues [tbeg[i], tbeg[i] + tlen[i]) of target
tidx[i] uploaded as a sequence of its own -- and through it the reference's ssw_init + ssw_align(profile, ref + tbeg, tlen, ...) answer.
Two oracles, no pair left out: (a) Context.align_pairs over the windows cut out on the host (all fields, cigar_off and its order included,
and the CIGAR words); (b) the reference through parity.expected() on the cut-out window (every pair on the emulator, a fixed-seed sample
on the GPU; windows of length 0 under (a) only -- the reference is not called with an empty target).
Every case runs on the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source, small sizes) and, marked gpu, on
the MI355X at larger sizes."""
import os
import subprocess

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, mutate, random_ref

MAT = dna_matrix(2, 2)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def _cut(targets, tidx, tbeg, tlen):
    return [np.ascontiguousarray(targets[int(t)][int(b):int(b) + int(l)]) for t, b, l in zip(tidx, tbeg, tlen)]


def _check(ctx, reads, targets, qidx, tidx, tbeg, tlen, mat, n, sample=None, T=None, **kw):
    """align_windows against oracle (a) for every pair and oracle (b) for every pair (or `sample`); -> (records, pool, timing)"""
    qidx = np.asarray(qidx, dtype=np.int32); tidx = np.asarray(tidx, dtype=np.int32)
    tbeg = np.asarray(tbeg, dtype=np.int64); tlen = np.asarray(tlen, dtype=np.int32)
    wins = _cut(targets, tidx, tbeg, tlen)
    assert [len(w) for w in wins] == [int(l) for l in tlen]
    Q = ctx.upload(reads); Tn = T if T is not None else ctx.upload(targets); W = ctx.upload(wins)
    try:
        res, cig = ctx.align_windows(Q, Tn, qidx, tidx, tbeg, tlen, mat, n, **kw)
        tm = ctx.timing()
        pres, pcig = ctx.align_pairs(Q, W, qidx, np.arange(len(qidx), dtype=np.int32), mat, n, **kw)
    finally:
        Q.free(); W.free()
        if T is None:
            Tn.free()
    bad = []
    for i in np.nonzero(res != pres)[0][:4]:
        bad.append("pair %d (read %d len %d, target %d [%d, +%d)): pairs %s %s, windows %s %s" % (
            i, qidx[i], len(reads[qidx[i]]), tidx[i], tbeg[i], tlen[i], pres[i], cigar_str(_cig(pres[i], pcig)), res[i], cigar_str(_cig(res[i], cig))))
    assert not bad, "\n".join(bad)
    assert (res == pres).all()                          # every field, cigar_off and its order included (not the struct's padding bytes)
    assert cig.tobytes() == pcig.tobytes()
    gapO, gapE, flag = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("flag", 0)
    if not kw.get("mark_mismatch", False):
        for i in (range(len(qidx)) if sample is None else sample):
            rd, rf = reads[qidx[i]], wins[i]
            if len(rf) == 0:
                continue
            ml = kw.get("maskLen", -1)
            exp, ecig = expected(rd, mat, n, rf, gapO, gapE, flag, kw.get("filters", 0), kw.get("filterd", 0), ml if ml >= 0 else len(rd) // 2,
                                 kw.get("score_size", 2))
            g = res[i]
            if exp is None:
                ok = int(g["status"]) == 1
            else:
                ok = int(g["status"]) == 0 and {k: int(g[k]) for k in RES_FIELDS} == exp and _cig(g, cig) == ecig
            if not ok and len(bad) < 4:
                bad.append("pair %d (len %d x %d): expected %s %s got %s" % (i, len(rd), len(rf), exp, cigar_str(ecig), g))
        assert not bad, "\n".join(bad)
    return res, cig, tm


def _genome_case(rng, lengths, npairs, qmax, wmin, wmax, n_codes=4, zero=1):
    """targets of different lengths; windows at random (odd and even) offsets; reads mutated from inside their window, some unrelated"""
    targets = [np.asarray(random_ref(L, int(rng.integers(1 << 30)), n_codes), dtype=np.int8) for L in lengths]
    tidx = rng.integers(0, len(targets), size=npairs).astype(np.int32)
    tlen = np.array([int(rng.integers(wmin, min(wmax, len(targets[t])) + 1)) for t in tidx], dtype=np.int32)
    tbeg = np.array([int(rng.integers(0, len(targets[t]) - l + 1)) for t, l in zip(tidx, tlen)], dtype=np.int64)
    tbeg[0] |= 1
    if tbeg[0] + tlen[0] > len(targets[tidx[0]]):
        tbeg[0] -= 1
    for k in range(zero):
        tlen[3 + k] = 0
    reads = []
    for i in range(npairs):
        w = targets[tidx[i]][tbeg[i]:tbeg[i] + tlen[i]]
        ql = int(rng.integers(1, qmax + 1))
        if rng.random() < 0.75 and len(w) > 4:
            s = int(rng.integers(0, max(1, len(w) - ql)))
            rd = mutate(w[s:s + ql], rng, 0.02, 0.01, 0.01, n_codes)[:qmax]      # (insertions must not take a read past qmax: the fast path's 640)
            if len(rd) == 0:
                rd = w[:1].copy()
        else:
            rd = random_ref(ql, int(rng.integers(1 << 30)), n_codes)
        reads.append(np.asarray(rd, dtype=np.int8))
    assert (tbeg & 1).any() and not (tbeg & 1).all()
    return reads, targets, np.arange(npairs, dtype=np.int32), tidx, tbeg, tlen


def _flag_kw(flag):
    return dict(gapO=3, gapE=1, flag=flag, filters=30 if flag == 2 else 0, filterd=40 if flag == 15 else 0)


def _geometry_case(rng, L=900, qlen=50):
    """the window shapes of the contract over 3 targets; -> (reads, targets, qidx, tidx, tbeg, tlen)"""
    targets = [np.asarray(random_ref(n, 40 + k, 4), dtype=np.int8) for k, n in enumerate((L, L // 2 + 7, L // 3))]
    rd = lambda t, b: mutate(targets[t][b:b + qlen], rng, 0.03, 0.01, 0.01, 4)
    reads = [rd(0, 100), rd(1, 20), rd(2, 30), rd(0, 300), rd(0, 330)]
    rows = [(0, 0, 0, L),                                     # the whole target
            (1, 1, len(targets[1]) - 120, 120),               # ends on the target's last residue
            (2, 2, 0, 110),                                   # starts at 0
            (0, 0, 117, 1),                                   # length 1
            (1, 1, 33, 0),                                    # length 0
            (3, 0, 280, 150), (3, 0, 280, 150),               # two identical windows
            (3, 0, 281, 150), (4, 0, 301, 141),               # two overlapping windows with different reads
            (0, 0, 60, 200), (0, 0, 95, 70), (0, 1, 0, 100), (0, 2, 5, 90)]      # the same read against several windows
    rows = [rows[k] for k in rng.permutation(len(rows))]      # list order permuted
    q, t, b, l = (np.array(c) for c in zip(*rows))
    return reads, targets, q, t, b, l


def _straddle_case(qlen=60, L=600):
    """a read planted at [270, 270 + qlen) of a target; window A ends inside the read, window B starts inside it"""
    target = np.asarray(random_ref(L, 91, 4), dtype=np.int8)
    read = target[270:270 + qlen].copy()
    mid = 270 + qlen // 2
    return [read], [target], np.array([0, 0]), np.array([0, 0]), np.array([mid - 150, mid]), np.array([150, 150])


def _check_straddle(ctx, flag):
    reads, targets, q, t, b, l = _straddle_case()
    res, cig, _ = _check(ctx, reads, targets, q, t, b, l, MAT, 5, flag=flag)
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        whole, _ = ctx.align_pairs(Q, T, q, t, MAT, 5, flag=flag)
    finally:
        Q.free(); T.free()
    assert int(whole[0]["score1"]) == 2 * len(reads[0])      # in the whole target the read matches end to end ...
    for i in range(2):                                       # ... in either window only the half that lies inside it
        assert int(res[i]["score1"]) < int(whole[i]["score1"]) and int(res[i]["score1"]) >= len(reads[0]) - 4
    assert int(res[0]["ref_end1"]) == 149                    # the window's last column
    if flag:
        assert int(res[1]["ref_begin1"]) == 0                # the window's first column


def _grid_case(rng, npairs, qmax, wmax, qlen_over):
    reads, targets, q, t, b, l = _genome_case(rng, (wmax * 3, wmax * 2 + 1, wmax + 50), npairs, qmax, 20, wmax)
    # an 8-bit overflow: an exact match of qlen_over residues at match 2 scores over 255 - bias
    b[0] = 51; l[0] = qlen_over + 140; t[0] = 0
    reads[0] = targets[0][100:100 + qlen_over].copy()
    return reads, targets, q, t, b, l


def _protein_case(rng, npairs, qmax, lengths):
    targets = [rng.integers(0, 20, size=n, dtype=np.int8) for n in lengths]
    tidx = rng.integers(0, len(targets), size=npairs).astype(np.int32)
    tlen = np.array([int(rng.integers(40, min(3 * qmax, len(targets[t])))) for t in tidx], dtype=np.int32)
    tbeg = np.array([int(rng.integers(0, len(targets[t]) - l + 1)) for t, l in zip(tidx, tlen)], dtype=np.int64)
    reads = [mutate(targets[t][b + 3:b + 3 + int(rng.integers(20, qmax))][:l], rng, 0.2, 0.02, 0.02, 20) for t, b, l in zip(tidx, tbeg, tlen)]
    return reads, targets, np.arange(npairs, dtype=np.int32), tidx, tbeg, tlen


def _distinct_residues(tidx, tbeg, tlen, which):
    return sum(l for (_, _, l) in set((int(tidx[i]), int(tbeg[i]), int(tlen[i])) for i in which))


def _errors(ctx):
    reads = [random_ref(30, 1, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        ok = dict(qidx=[0, 0, 0], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30])
        cases = [("qidx", 1, "out of range"), ("qidx", -1, "out of range"), ("tidx", 2, "out of range"), ("tidx", -1, "out of range"),
                 ("tbeg", -1, "window out of range"), ("tlen", -1, "window out of range"), ("tlen", 31, "window out of range"),
                 ("tbeg", 41, "window out of range"), ("tbeg", 1 << 40, "window out of range")]
        for field, value, what in cases:
            for flag in (0, 2):
                args = {k: list(v) for k, v in ok.items()}
                args[field][2] = value
                out = np.zeros(3, dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
                before = out.tobytes()      # (a numpy array of the caller: every byte, padding included, must stay)
                with pytest.raises(RuntimeError, match=what + r".*pair 2\b"):
                    ctx.align_windows(Q, T, args["qidx"], args["tidx"], args["tbeg"], args["tlen"], MAT, 5, flag=flag, out=out)
                assert out.tobytes() == before
                # the context answers the next call
                _check(ctx, reads, targets, ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], MAT, 5, T=T, flag=flag)
        e = np.zeros(0, np.int32)
        res, cig = ctx.align_windows(Q, T, e, e, np.zeros(0, np.int64), e, MAT, 5, flag=2)
        assert res.shape == (0,) and cig.shape == (0,)
        with pytest.raises(ValueError):
            ctx.align_windows(Q, T, [0], [0, 0], [0], [1], MAT, 5)
    finally:
        Q.free(); T.free()


def _rebase(ctx, rng, npairs, qmax, wmax):
    reads, targets, q, t, b, l = _genome_case(rng, (3 * wmax, 2 * wmax + 1, wmax + 9), npairs, qmax, 30, wmax)
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        for kw in (dict(flag=0), dict(flag=15, filterd=32767), dict(flag=0, maskLen=5), dict(flag=2, filters=10000)):
            rel, c0 = ctx.align_windows(Q, T, q, t, b, l, MAT, 5, **kw)
            reb, c1 = ctx.align_windows(Q, T, q, t, b, l, MAT, 5, rebase=True, **kw)
            exp = rel.copy()
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                exp[f] = np.where(rel[f] >= 0, rel[f] + b, rel[f])
            assert (reb == exp).all() and c0.tobytes() == c1.tobytes()
            if kw.get("flag") == 0:
                assert (reb["ref_begin1"] == -1).all()
            if kw.get("maskLen") == 5:
                assert (reb["ref_end2"][rel["score1"] > 0] == -1).all()      # maskLen < 15: the reference's -1 stays -1
            if kw.get("flag") == 15:
                hit = rel["score1"] > 0
                assert hit.any() and (reb["ref_begin1"][hit] >= b[hit]).all()
    finally:
        Q.free(); T.free()


def _cpp_check(lib_dir, lib_name, tmp_path, args):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / ("windows_check_" + lib_name))
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "windows_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-l" + lib_name, "-lm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_emu_one_to_one_dna(ectx, flag):
    rng = np.random.default_rng(3100 + flag)
    case = _genome_case(rng, (700, 431, 1200, 256), 24, 110, 1, 240)
    _, _, tm = _check(ectx, *case, MAT, 5, **_flag_kw(flag))
    assert tm["fill_kernel"].startswith("k_fillpairs<")
    assert tm["win_copied"] == 0          # (the empty window leaves the fast path, and has nothing to copy)


@pytest.mark.parametrize("flag", [0, 15])
def test_emu_window_geometry(ectx, flag):
    rng = np.random.default_rng(3200 + flag)
    _, _, tm = _check(ectx, *_geometry_case(rng), MAT, 5, flag=flag)
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    _check_straddle(ectx, flag)


@pytest.mark.parametrize("maskLen,score_size", [(-1, 0), (10, 1), (30, 2), (-1, 1)])
def test_emu_masklen_score_size(ectx, maskLen, score_size):
    rng = np.random.default_rng(3300 + maskLen + 7 * score_size)
    res, _, tm = _check(ectx, *_grid_case(rng, 12, 100, 200, 160), MAT, 5, flag=0, maskLen=maskLen, score_size=score_size)
    assert tm["win_copied"] == 0
    if score_size == 0:
        assert int(res[0]["status"]) == 1


def test_emu_protein_blosum50_mark_mismatch(ectx):
    rng = np.random.default_rng(3400)
    case = _protein_case(rng, 12, 80, (400, 333, 250))
    _, _, tm = _check(ectx, *case, blosum50(), 24, gapO=10, gapE=2, flag=2, filters=40, mark_mismatch=True)
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    _check(ectx, *case, blosum50(), 24, gapO=10, gapE=2, flag=2, filters=40)


def test_emu_fallbacks(ectx):
    rng = np.random.default_rng(3500)
    reads, targets, q, t, b, l = _genome_case(rng, (1500, 901, 700), 14, 90, 30, 200, zero=0)
    big = 700                                                  # a query over 640 residues: beyond the fused kernel
    reads.append(targets[0][300:300 + big].copy()); reads.append(np.zeros(0, dtype=np.int8))
    nq = len(reads)
    # pairs 0, 1: the long query against two IDENTICAL windows; pair 2: an empty query; pair 3: an ordinary read against the long query's window
    q[0] = q[1] = nq - 2; t[0] = t[1] = 0; b[0] = b[1] = 251; l[0] = l[1] = 900
    q[2] = nq - 1
    t[3] = 0; b[3] = 251; l[3] = 900
    for flag in (0, 2):
        _, _, tm = _check(ectx, reads, targets, q, t, b, l, MAT, 5, flag=flag)
        assert tm["win_copied"] == _distinct_residues(t, b, l, (0, 1, 2)) == 900 + int(l[2])
    # gapO <= gapE: every pair leaves the fast path, identical windows are gathered once
    for flag in (0, 2):
        _, _, tm = _check(ectx, reads, targets, q, t, b, l, MAT, 5, gapO=1, gapE=1, flag=flag)
        assert tm["win_copied"] == _distinct_residues(t, b, l, range(len(q))) < int(l.sum())
    # a 40-letter alphabet
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    t40 = [np.asarray(random_ref(300 + 11 * i, 400 + i, 40), dtype=np.int8) for i in range(2)]
    q40 = [mutate(t40[i % 2][35:90], rng, 0.05, 0.0, 0.0, 40) for i in range(3)]
    ti, tb, tl = np.array([0, 1, 0, 1]), np.array([21, 30, 21, 0]), np.array([100, 90, 100, 311])
    _, _, tm = _check(ectx, q40, t40, np.array([0, 1, 2, 1]), ti, tb, tl, m40, 40, flag=2)
    assert tm["win_copied"] == 100 + 90 + 311


def test_emu_small_budget_chunks(emu_lib_path):
    """1 MiB budget (the floor): jobs per launch are cut down, results as under the default budget"""
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    try:
        rng = np.random.default_rng(3600)
        ref = np.asarray(random_ref(60000, 700, 4), dtype=np.int8)
        tbeg = rng.integers(0, 40000, size=48).astype(np.int64); tlen = np.full(48, 19000, dtype=np.int32); tlen[::3] = 15001
        reads = [ref[int(s) + 200:int(s) + 230].copy() for s in tbeg]
        qidx = np.arange(48, dtype=np.int32); tidx = np.zeros(48, dtype=np.int32)
        Q = ctx.upload(reads); T = ctx.upload([ref])
        for flag in (0, 2):
            r0, c0 = ctx.align_windows(Q, T, qidx, tidx, tbeg, tlen, MAT, 5, flag=flag)
            l0 = ctx.timing()["fill_launches"]
            ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
            r1, c1 = ctx.align_windows(Q, T, qidx, tidx, tbeg, tlen, MAT, 5, flag=flag)
            tm = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert tm["fill_launches"] > 1 and tm["fill_launches"] > l0 and tm["win_copied"] == 0
            assert (r0 == r1).all() and c0.tobytes() == c1.tobytes()
            assert (r0["score1"] == 60).all() and (r0["ref_end1"] == 229).all()
        Q.free(); T.free()
    finally:
        ctx.close()


def test_emu_errors(ectx):
    _errors(ectx)


def test_emu_rebase(ectx):
    _rebase(ectx, np.random.default_rng(3800), 16, 90, 220)


def test_cpp_align_windows_emulated(emu_lib_path, tmp_path):
    """include/ssw_gpu_cpp.h BatchAligner::AlignWindows against AlignPairs over cut-out windows (tests/cpp/windows_check.cpp)"""
    _cpp_check(os.path.dirname(emu_lib_path), "ssw_emu", tmp_path, ["24", "4"])


# ---------------------------------------------------------------------------------------------------------------- MI355X

def _sample(rng, n, k=240):
    return [int(x) for x in rng.choice(n, size=min(n, k), replace=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_gpu_one_to_one_dna(gpu_ctx, flag):
    rng = np.random.default_rng(4100 + flag)
    case = _genome_case(rng, (70001, 20000, 131072, 9999, 40003, 655), 1500, 640, 1, 2500, zero=2)
    for filters, filterd in ((0, 0), (60, 50)):
        kw = dict(flag=flag, filters=filters, filterd=filterd)
        _, _, tm = _check(gpu_ctx, *case, MAT, 5, sample=_sample(np.random.default_rng(1), 1500), **kw)
        assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 15])
def test_gpu_window_geometry(gpu_ctx, flag):
    rng = np.random.default_rng(4200 + flag)
    _, _, tm = _check(gpu_ctx, *_geometry_case(rng, L=60000, qlen=150), MAT, 5, flag=flag)
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    _check_straddle(gpu_ctx, flag)


@pytest.mark.gpu
@pytest.mark.parametrize("maskLen,score_size", [(-1, 0), (10, 1), (30, 2), (-1, 2)])
def test_gpu_masklen_score_size(gpu_ctx, maskLen, score_size):
    rng = np.random.default_rng(4300 + maskLen + 7 * score_size)
    res, _, tm = _check(gpu_ctx, *_grid_case(rng, 400, 640, 2000, 400), MAT, 5, sample=_sample(np.random.default_rng(2), 400),
                        flag=0, maskLen=maskLen, score_size=score_size)
    assert tm["win_copied"] == 0
    if score_size == 0:
        assert int(res[0]["status"]) == 1


@pytest.mark.gpu
def test_gpu_protein_blosum50(gpu_ctx):
    rng = np.random.default_rng(4400)
    case = _protein_case(rng, 800, 500, (5000, 3333, 2500, 900))
    _, _, tm = _check(gpu_ctx, *case, blosum50(), 24, gapO=10, gapE=2, flag=2, filters=60, mark_mismatch=True)
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    _check(gpu_ctx, *case, blosum50(), 24, sample=_sample(np.random.default_rng(3), 800), gapO=10, gapE=2, flag=2, filters=60)


@pytest.mark.gpu
def test_gpu_fallbacks(gpu_ctx):
    rng = np.random.default_rng(4500)
    reads, targets, q, t, b, l = _genome_case(rng, (200000, 90001, 70000), 60, 400, 30, 2000, zero=0)
    reads.append(targets[0][150000:150700].copy()); reads.append(np.zeros(0, dtype=np.int8))
    reads.append(targets[0][100000 + 69000:100000 + 69150].copy())
    nq = len(reads)
    # pairs 0, 1: a window over 65 000 columns, twice; pair 2: an empty query; pairs 3, 4: a query over 640 residues and an ordinary one, same window
    q[0] = q[1] = nq - 1; t[0] = t[1] = 0; b[0] = b[1] = 100000; l[0] = l[1] = 70000
    q[2] = nq - 2
    q[3] = nq - 3; t[3] = t[4] = 0; b[3] = b[4] = 149501; l[3] = l[4] = 1500
    for gO, gE, flag in ((3, 1, 0), (3, 1, 2)):
        res, _, tm = _check(gpu_ctx, reads, targets, q, t, b, l, MAT, 5, gapO=gO, gapE=gE, flag=flag)
        assert tm["win_copied"] == _distinct_residues(t, b, l, (0, 1, 2, 3)) == 70000 + int(l[2]) + 1500
        assert int(res[0]["score1"]) == 300 and int(res[0]["ref_end1"]) == 69149
    for flag in (0, 2):
        _, _, tm = _check(gpu_ctx, reads, targets, q, t, b, l, MAT, 5, gapO=1, gapE=1, flag=flag)
        assert tm["win_copied"] == _distinct_residues(t, b, l, range(len(q)))
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    t40 = [np.asarray(random_ref(3000 + 11 * i, 400 + i, 40), dtype=np.int8) for i in range(3)]
    ti = rng.integers(0, 3, size=12); tl = rng.integers(250, 900, size=12); tb = np.array([int(rng.integers(0, 3000 - n)) for n in tl])
    q40 = [mutate(t40[x][y + 5:y + 200], rng, 0.05, 0.0, 0.0, 40) for x, y in zip(ti, tb)]
    _, _, tm = _check(gpu_ctx, q40, t40, np.arange(12), ti, tb, tl, m40, 40, flag=2)
    assert tm["win_copied"] == int(tl.sum())


@pytest.mark.gpu
def test_gpu_budget_16mib(product_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(product_lib_path))
    try:
        rng = np.random.default_rng(4600)
        reads, targets, q, t, b, l = _genome_case(rng, (500000, 300001), 6000, 150, 300, 700, zero=0)
        Q = ctx.upload(reads); T = ctx.upload(targets)
        for flag in (0, 2):
            r0, c0 = ctx.align_windows(Q, T, q, t, b, l, MAT, 5, flag=flag)
            ctx.lib.ssw_gpu_set_budget(ctx.h, 16 << 20)
            r1, c1 = ctx.align_windows(Q, T, q, t, b, l, MAT, 5, flag=flag)
            tm = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert tm["fill_launches"] > 1 and tm["win_copied"] == 0
            assert (r0 == r1).all() and c0.tobytes() == c1.tobytes()
        Q.free(); T.free()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    _errors(gpu_ctx)


@pytest.mark.gpu
def test_gpu_rebase(gpu_ctx):
    _rebase(gpu_ctx, np.random.default_rng(4800), 500, 300, 1500)


@pytest.mark.gpu
def test_gpu_resident_set_above_2_31(gpu_ctx):
    """a resident set of 2^31 + 2^27 residues and more: flag-15 windows, half of them wholly above absolute offset 2^31, stay on the fused
    path -- the window kernels reach their target through a 64-bit base (the parent's pair path fell back to a batch per target here)"""
    rng = np.random.default_rng(4900)
    lengths = (1000000000, 700000000, 600000001)
    assert sum(lengths) >= (1 << 31) + (1 << 27) and max(lengths) < (1 << 31)
    targets = [rng.integers(0, 4, size=n, dtype=np.int8) for n in lengths]
    npairs = 3000
    tidx = rng.integers(0, 3, size=npairs).astype(np.int32); tidx[:npairs // 2] = 2
    tlen = rng.integers(300, 701, size=npairs).astype(np.int32)
    tbeg = np.array([int(rng.integers(0, lengths[t] - n + 1)) for t, n in zip(tidx, tlen)], dtype=np.int64)
    above = (1 << 31) - (lengths[0] + lengths[1])            # offset in target 2 of absolute offset 2^31
    tbeg[:npairs // 2] = rng.integers(above, lengths[2] - 701, size=npairs // 2)
    tbeg[0] = lengths[2] - int(tlen[0])                      # the last residue of the set
    start = np.array([0, lengths[0], lengths[0] + lengths[1]])[tidx] + tbeg
    assert (start >= (1 << 31)).sum() * 3 >= npairs
    reads = []
    for t, s, n in zip(tidx, tbeg, tlen):
        o = int(rng.integers(0, n - 150))
        reads.append(np.asarray(mutate(targets[t][s + o:s + o + 150], rng, 0.02, 0.005, 0.005, 4), dtype=np.int8))
    perm = rng.permutation(npairs)
    qidx = np.arange(npairs, dtype=np.int32)[perm]; tidx = tidx[perm]; tbeg = tbeg[perm]; tlen = tlen[perm]
    T = gpu_ctx.upload(targets)
    try:
        res, _, tm = _check(gpu_ctx, reads, targets, qidx, tidx, tbeg, tlen, MAT, 5, sample=_sample(np.random.default_rng(4), npairs), T=T,
                            flag=15, filterd=32767)
    finally:
        T.free()
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    assert (res["score1"] > 200).all() and (res["cigarLen"] > 0).all()


@pytest.mark.gpu
def test_gpu_at_scale(gpu_ctx):
    """200 000 reads of 150 bp against windows of 300..700 bp of one resident 100 Mb target, flag 0 and flag 2 with CIGARs"""
    rng = np.random.default_rng(5000)
    L, npairs = 100000000, 200000
    target = rng.integers(0, 4, size=L, dtype=np.int8)
    tlen = rng.integers(300, 701, size=npairs).astype(np.int32)
    tbeg = rng.integers(0, L - 700, size=npairs).astype(np.int64)
    reads = []
    for s, n in zip(tbeg, tlen):
        o = int(rng.integers(0, n - 150))
        reads.append(np.asarray(mutate(target[s + o:s + o + 150], rng, 0.02, 0.005, 0.005, 4), dtype=np.int8))
    qidx = rng.permutation(npairs).astype(np.int32)
    tidx = np.zeros(npairs, dtype=np.int32)
    T = gpu_ctx.upload([target])
    try:
        for flag in (0, 2):      # pair i: read qidx[i] against ITS window
            _, _, tm = _check(gpu_ctx, reads, [target], qidx, tidx, tbeg[qidx], tlen[qidx], MAT, 5, sample=_sample(np.random.default_rng(5), npairs, 400),
                              T=T, flag=flag, filters=0)
            assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    finally:
        T.free()


@pytest.mark.gpu
def test_cpp_align_windows_gpu(product_lib_path, tmp_path):
    _cpp_check(os.path.dirname(product_lib_path), "ssw", tmp_path, ["600", "6"])
