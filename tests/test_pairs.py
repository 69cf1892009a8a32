"""ssw_gpu_align_pairs: an explicit list of (query, target) pairs (include/ssw_gpu.h).

Record i must equal, bit for bit, what ssw_gpu_align_batch(queries, targets, tidx[i], 1, ...) gives at row qidx[i] -- and through it
the reference's ssw_init + ssw_align answer.  Every case runs on the CPU SIMT emulator (tests/emu: the real host driver and the real
kernel source, small sizes) and, marked gpu, on the MI355X at larger sizes."""
import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, mutate, random_ref

FIELDS = [f for f in ssw_amd.RESULT_DTYPE.names if f != "cigar_off"]


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def _pairs_vs_batch(ctx, reads, refs, qidx, tidx, mat, n, **kw):
    """align_pairs against one align_batch call per distinct target (the contract); returns the pair records and pool"""
    Q = ctx.upload(reads); T = ctx.upload(refs)
    try:
        res, cig = ctx.align_pairs(Q, T, qidx, tidx, mat, n, **kw)
        _pairs_vs_batch.timing = ctx.timing()
        bad = []
        for t in sorted(set(int(x) for x in tidx)):
            bres, bcig = ctx.align_batch(Q, T, mat, n, target_first=t, target_count=1, **kw)
            for i in np.nonzero(np.asarray(tidx) == t)[0]:
                g, e = res[i], bres[int(qidx[i]), 0]
                got = {f: int(g[f]) for f in FIELDS}
                exp = {f: int(e[f]) for f in FIELDS}
                if got != exp or _cig(g, cig) != _cig(e, bcig) or (int(e["cigarLen"]) == 0 and int(g["cigar_off"]) != int(e["cigar_off"])):
                    if len(bad) < 4:
                        bad.append("pair %d (q%d len %d, t%d len %d): batch %s %s, pairs %s %s" % (
                            i, qidx[i], len(reads[qidx[i]]), t, len(refs[t]), exp, cigar_str(_cig(e, bcig)), got, cigar_str(_cig(g, cig))))
        assert not bad, "\n".join(bad)
    finally:
        Q.free(); T.free()
    return res, cig


def _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1,
                        score_size=2, sample=None):
    idx = range(len(qidx)) if sample is None else sample
    bad = []
    for i in idx:
        rd, rf = reads[qidx[i]], refs[tidx[i]]
        if len(rf) == 0:
            continue      # (the reference is not called with an empty target; align_batch's record is checked above)
        ml = maskLen if maskLen >= 0 else len(rd) // 2
        exp, ecig = expected(rd, mat, n, rf, gapO, gapE, flag, filters, filterd, ml, score_size)
        g = res[i]
        if exp is None:
            ok = int(g["status"]) == 1
        else:
            ok = int(g["status"]) == 0 and {k: int(g[k]) for k in RES_FIELDS} == exp and _cig(g, cig) == ecig
        if not ok and len(bad) < 4:
            bad.append("pair %d (len %d x %d): expected %s %s got %s" % (i, len(rd), len(rf), exp, cigar_str(ecig), g))
    assert not bad, "\n".join(bad)


def _one_to_one(rng, npairs, qmax, tmax, n_codes=4, empties=True):
    """reads taken (mutated) from their own windows, lengths mixed; some empty reads / windows"""
    reads, refs = [], []
    for i in range(npairs):
        tl = int(rng.integers(1, tmax + 1))
        ref = random_ref(tl, int(rng.integers(1 << 30)), n_codes)
        ql = int(rng.integers(1, qmax + 1))
        if rng.random() < 0.7 and tl > 4:
            s = int(rng.integers(0, max(1, tl - ql)))
            rd = mutate(ref[s:s + ql], rng, 0.02, 0.01, 0.01, n_codes)
            if len(rd) == 0:
                rd = ref[:1].copy()
        else:
            rd = random_ref(ql, int(rng.integers(1 << 30)), n_codes)
        reads.append(np.asarray(rd, dtype=np.int8)); refs.append(np.asarray(ref, dtype=np.int8))
    if empties:
        reads[1] = np.zeros(0, dtype=np.int8)
        refs[2] = np.zeros(0, dtype=np.int8)
    qidx = np.arange(npairs, dtype=np.int32)
    tidx = np.arange(npairs, dtype=np.int32)
    return reads, refs, qidx, tidx


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_emu_one_to_one_dna(ectx, flag):
    rng = np.random.default_rng(100 + flag)
    reads, refs, qidx, tidx = _one_to_one(rng, 10, 120, 260)
    kw = dict(gapO=3, gapE=1, flag=flag, filters=30 if flag == 2 else 0, filterd=0 if flag != 15 else 40, maskLen=-1, score_size=2)
    res, cig = _pairs_vs_batch(ectx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
    _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
    assert _pairs_vs_batch.timing["fill_kernel"].startswith("k_fillpairs<")      # flagged pairs too: fill, then reverse pass + traceback


@pytest.mark.parametrize("maskLen,score_size", [(-1, 0), (10, 1), (30, 2), (-1, 1)])
def test_emu_masklen_score_size(ectx, maskLen, score_size):
    rng = np.random.default_rng(200 + maskLen + 7 * score_size)
    reads, refs, qidx, tidx = _one_to_one(rng, 8, 100, 200)
    # an 8-bit overflow: a 160-residue exact match at match 2 scores 320 > 255 - bias
    refs[0] = random_ref(300, 5, 4); reads[0] = refs[0][50:210].copy()
    kw = dict(flag=0, maskLen=maskLen, score_size=score_size)
    res, cig = _pairs_vs_batch(ectx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
    _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
    if score_size == 0:
        assert int(res[0]["status"]) == 1


def test_emu_one_to_many_unsorted_repeats(ectx):
    rng = np.random.default_rng(7)
    refs = [random_ref(int(rng.integers(40, 300)), 50 + i, 4) for i in range(6)]
    reads = [mutate(refs[i % 6][10:10 + int(rng.integers(20, 90))], rng, 0.03, 0.01, 0.01, 4) for i in range(7)]
    qidx = np.array([0, 0, 0, 0, 3, 1, 2, 3, 4, 5, 6, 6, 2, 0, 5, 5, 1], dtype=np.int32)          # one-to-many, many-to-one, repeats
    tidx = np.array([0, 1, 2, 3, 3, 3, 3, 0, 5, 4, 1, 1, 2, 0, 2, 2, 4], dtype=np.int32)
    perm = rng.permutation(len(qidx))
    for flag in (0, 2):
        _pairs_vs_batch(ectx, reads, refs, qidx[perm], tidx[perm], dna_matrix(2, 2), 5, flag=flag)


def test_emu_protein_blosum50_mark_mismatch(ectx):
    rng = np.random.default_rng(9)
    refs = [rng.integers(0, 20, size=int(rng.integers(60, 220)), dtype=np.int8) for _ in range(5)]
    reads = [mutate(refs[i % 5][5:5 + int(rng.integers(30, 90))], rng, 0.2, 0.02, 0.02, 20) for i in range(8)]
    qidx = np.arange(8, dtype=np.int32); tidx = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.int32)
    kw = dict(gapO=10, gapE=2, flag=2, filters=40, mark_mismatch=True)
    _pairs_vs_batch(ectx, reads, refs, qidx, tidx, blosum50(), 24, **kw)
    _pairs_vs_batch(ectx, reads, refs, qidx, tidx, blosum50(), 24, gapO=10, gapE=2, flag=0)


def _fallback_cases(rng, long_target=0):
    """gapO <= gapE, a 40-letter alphabet, queries over 640 residues -- mixed with ordinary pairs"""
    refs = [random_ref(int(rng.integers(50, 250)), 300 + i, 4) for i in range(4)]
    reads = [mutate(refs[i % 4][0:int(rng.integers(20, 100))], rng, 0.03, 0.01, 0.01, 4) for i in range(6)]
    big = random_ref(900, 77, 4)
    refs.append(big); reads.append(big[100:800].copy())            # a 700-residue query: beyond the fused kernel
    if long_target:
        lt = random_ref(long_target, 78, 4); refs.append(lt); reads.append(lt[long_target - 300:long_target - 150].copy())
    nq, nt = len(reads), len(refs)
    qidx = np.array([i % nq for i in range(2 * nq)], dtype=np.int32)
    tidx = np.array([(i * 3) % nt for i in range(2 * nq)], dtype=np.int32)
    qidx[nq - 1] = nq - 1; tidx[nq - 1] = 4
    if long_target:
        qidx[nq - 2] = nq - 1; tidx[nq - 2] = nt - 1
    return reads, refs, qidx, tidx


def test_emu_fallback_paths(ectx):
    rng = np.random.default_rng(11)
    reads, refs, qidx, tidx = _fallback_cases(rng)
    for gO, gE, flag in ((1, 1, 0), (3, 1, 0), (1, 1, 2), (3, 1, 2)):      # gapO <= gapE; > 640 residues beside ordinary pairs
        res, cig = _pairs_vs_batch(ectx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, gapO=gO, gapE=gE, flag=flag)
        _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, gapO=gO, gapE=gE, flag=flag)
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    r40 = [random_ref(80 + 10 * i, 400 + i, 40) for i in range(3)]
    q40 = [mutate(r40[i][5:60], rng, 0.05, 0.0, 0.0, 40) for i in range(3)]
    _pairs_vs_batch(ectx, q40, r40, np.array([0, 1, 2, 1], np.int32), np.array([1, 2, 0, 1], np.int32), m40, 40, flag=2)


@pytest.mark.parametrize("env", [{}, {"SSW_GPU_DB_FORM": "0"}, {"SSW_GPU_FRAME_K": "16"}])
def test_emu_scores_near_2048(ectx, monkeypatch, env):
    """scores around 2 048 in the frame form (with frequent renormalisation) and in the plain int16 form"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(13)
    refs = [random_ref(700, 600 + i, 4) for i in range(3)]
    reads = [refs[0][20:620].copy(), mutate(refs[1][0:600], rng, 0.01, 0.0, 0.0, 4), refs[2][100:700].copy()]
    mat = dna_matrix(4, 3)        # ~600 x 4 = 2 400
    qidx = np.array([0, 1, 2], np.int32); tidx = np.array([0, 1, 2], np.int32)
    res, cig = _pairs_vs_batch(ectx, reads, refs, qidx, tidx, mat, 5, gapO=5, gapE=2)
    _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, mat, 5, gapO=5, gapE=2)
    assert int(res["score1"].max()) > 2048
    assert _pairs_vs_batch.timing["fill_kernel"] == ("k_fillpairs<38,int16+max3>" if env.get("SSW_GPU_DB_FORM") == "0" else "k_fillpairs<38,frame>")


def test_emu_small_budget_chunks(emu_lib_path):
    """1 MiB budget (the floor): jobs per launch are cut down, results as under the default budget"""
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    try:
        rng = np.random.default_rng(15)
        ref = random_ref(20000, 700, 4)
        reads = [ref[int(s):int(s) + 30].copy() for s in rng.integers(0, 19000, size=48)]
        qidx = np.arange(48, dtype=np.int32); tidx = np.zeros(48, dtype=np.int32)
        Q = ctx.upload(reads); T = ctx.upload([ref])
        r0, _ = ctx.align_pairs(Q, T, qidx, tidx, dna_matrix(2, 2), 5)
        ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
        r1, _ = ctx.align_pairs(Q, T, qidx, tidx, dna_matrix(2, 2), 5)
        assert ctx.timing()["fill_launches"] > 1
        Q.free(); T.free()
        assert r0.tobytes() == r1.tobytes()
    finally:
        ctx.close()


def test_emu_errors(ectx):
    Q = ectx.upload([random_ref(30, 1, 4)]); T = ectx.upload([random_ref(40, 2, 4)])
    try:
        out = np.zeros(2, dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777
        with pytest.raises(RuntimeError, match="out of range"):
            ectx.align_pairs(Q, T, np.array([0, 1], np.int32), np.array([0, 0], np.int32), dna_matrix(2, 2), 5, out=out)
        assert (out["score1"] == 777).all()
        with pytest.raises(RuntimeError, match="out of range"):
            ectx.align_pairs(Q, T, np.array([0, 0], np.int32), np.array([0, -1], np.int32), dna_matrix(2, 2), 5, out=out)
        assert (out["score1"] == 777).all()
        res, cig = ectx.align_pairs(Q, T, np.zeros(0, np.int32), np.zeros(0, np.int32), dna_matrix(2, 2), 5, flag=2)
        assert res.shape == (0,) and cig.shape == (0,)
    finally:
        Q.free(); T.free()


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_gpu_one_to_one_dna(gpu_ctx, flag):
    rng = np.random.default_rng(1100 + flag)
    reads, refs, qidx, tidx = _one_to_one(rng, 300, 640, 2000)
    for filters, filterd in ((0, 0), (60, 50)):
        kw = dict(flag=flag, filters=filters, filterd=filterd)
        res, cig = _pairs_vs_batch(gpu_ctx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
        _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, sample=range(0, 300, 3), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("maskLen,score_size", [(-1, 0), (10, 1), (30, 2), (-1, 2)])
def test_gpu_masklen_score_size(gpu_ctx, maskLen, score_size):
    rng = np.random.default_rng(1200 + maskLen + 7 * score_size)
    reads, refs, qidx, tidx = _one_to_one(rng, 200, 640, 2000)
    refs[0] = random_ref(600, 5, 4); reads[0] = refs[0][50:450].copy()
    kw = dict(flag=0, maskLen=maskLen, score_size=score_size)
    res, cig = _pairs_vs_batch(gpu_ctx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, **kw)
    _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, sample=range(0, 200, 2), **kw)
    if score_size == 0:
        assert int(res[0]["status"]) == 1


@pytest.mark.gpu
def test_gpu_one_to_many_unsorted_repeats(gpu_ctx):
    rng = np.random.default_rng(17)
    refs = [random_ref(int(rng.integers(100, 1500)), 900 + i, 4) for i in range(40)]
    reads = [mutate(refs[i % 40][10:10 + int(rng.integers(20, 400))], rng, 0.03, 0.01, 0.01, 4) for i in range(120)]
    qidx = np.concatenate([np.repeat(np.arange(10), 30), rng.integers(0, 120, size=600)]).astype(np.int32)
    tidx = np.concatenate([np.tile(np.arange(30), 10), rng.integers(0, 40, size=600)]).astype(np.int32)
    perm = rng.permutation(len(qidx))
    for flag in (0, 2):
        _pairs_vs_batch(gpu_ctx, reads, refs, qidx[perm], tidx[perm], dna_matrix(2, 2), 5, flag=flag)


@pytest.mark.gpu
def test_gpu_protein_blosum50(gpu_ctx):
    rng = np.random.default_rng(19)
    refs = [rng.integers(0, 20, size=int(rng.integers(100, 900)), dtype=np.int8) for _ in range(50)]
    reads = [mutate(refs[i % 50][5:5 + int(rng.integers(30, 500))], rng, 0.2, 0.02, 0.02, 20) for i in range(200)]
    qidx = np.repeat(np.arange(200, dtype=np.int32), 4); tidx = rng.integers(0, 50, size=800).astype(np.int32)
    _pairs_vs_batch(gpu_ctx, reads, refs, qidx, tidx, blosum50(), 24, gapO=10, gapE=2, flag=2, filters=60, mark_mismatch=True)
    res, _ = _pairs_vs_batch(gpu_ctx, reads, refs, qidx, tidx, blosum50(), 24, gapO=10, gapE=2, flag=0)
    assert _pairs_vs_batch.timing["fill_kernel"].startswith("k_fillpairs<")


@pytest.mark.gpu
def test_gpu_fallback_paths(gpu_ctx):
    rng = np.random.default_rng(21)
    reads, refs, qidx, tidx = _fallback_cases(rng, long_target=70000)
    for gO, gE, flag in ((1, 1, 0), (3, 1, 0), (3, 1, 2), (1, 1, 2)):
        res, cig = _pairs_vs_batch(gpu_ctx, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, gapO=gO, gapE=gE, flag=flag)
        _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, dna_matrix(2, 2), 5, gapO=gO, gapE=gE, flag=flag)
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    r40 = [random_ref(300 + 10 * i, 400 + i, 40) for i in range(5)]
    q40 = [mutate(r40[i % 5][5:200], rng, 0.05, 0.0, 0.0, 40) for i in range(8)]
    _pairs_vs_batch(gpu_ctx, q40, r40, np.arange(8, dtype=np.int32), np.array([1, 2, 0, 1, 4, 3, 3, 0], np.int32), m40, 40, flag=2)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"SSW_GPU_DB_FORM": "0"}, {"SSW_GPU_FRAME_K": "16"}])
def test_gpu_scores_near_2048(gpu_hctx, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(23)
    refs = [random_ref(800, 650 + i, 4) for i in range(40)]
    reads = [mutate(refs[i][int(s):int(s) + 600], rng, 0.005, 0.0, 0.0, 4) for i, s in enumerate(rng.integers(0, 200, size=40))]
    mat = dna_matrix(4, 3)
    qidx = np.arange(40, dtype=np.int32); tidx = np.arange(40, dtype=np.int32)
    res, cig = _pairs_vs_batch(gpu_hctx, reads, refs, qidx, tidx, mat, 5, gapO=5, gapE=2)
    _pairs_vs_reference(res, cig, reads, refs, qidx, tidx, mat, 5, gapO=5, gapE=2)
    assert _pairs_vs_batch.timing["fill_kernel"] == ("k_fillpairs<38,int16+max3>" if env.get("SSW_GPU_DB_FORM") == "0" else "k_fillpairs<38,frame>")
    assert int(res["score1"].max()) > 2048 and int(res["score1"].min()) < 2048 + 400


@pytest.mark.gpu
def test_gpu_budget_16mib(product_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(product_lib_path))
    try:
        rng = np.random.default_rng(25)
        reads, refs, qidx, tidx = _one_to_one(rng, 6000, 150, 700, empties=False)
        Q = ctx.upload(reads); T = ctx.upload(refs)
        for flag in (0, 2):
            r0, c0 = ctx.align_pairs(Q, T, qidx, tidx, dna_matrix(2, 2), 5, flag=flag)
            ctx.lib.ssw_gpu_set_budget(ctx.h, 16 << 20)
            r1, c1 = ctx.align_pairs(Q, T, qidx, tidx, dna_matrix(2, 2), 5, flag=flag)
            if flag == 0:
                assert ctx.timing()["fill_launches"] > 1
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes()
        Q.free(); T.free()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    Q = gpu_ctx.upload([random_ref(30, 1, 4)]); T = gpu_ctx.upload([random_ref(40, 2, 4)])
    try:
        out = np.zeros(2, dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777
        with pytest.raises(RuntimeError, match="out of range"):
            gpu_ctx.align_pairs(Q, T, np.array([0, 0], np.int32), np.array([0, 1], np.int32), dna_matrix(2, 2), 5, out=out)
        assert (out["score1"] == 777).all()
        res, cig = gpu_ctx.align_pairs(Q, T, np.zeros(0, np.int32), np.zeros(0, np.int32), dna_matrix(2, 2), 5)
        assert res.shape == (0,) and cig.shape == (0,)
    finally:
        Q.free(); T.free()


@pytest.mark.gpu
def test_gpu_at_scale(gpu_ctx):
    """200 000 one-to-one pairs over 2 000 windows (100 reads per window), flag 2 with CIGARs: every record against 2 000 align_batch
    calls, a sample of 2 000 against the reference"""
    rng = np.random.default_rng(27)
    windows = [random_ref(int(rng.integers(300, 701)), 5000 + w, 4) for w in range(2000)]
    reads = []
    for w in range(2000):
        ref = windows[w]
        for s in rng.integers(0, len(ref) - 150, size=100):
            reads.append(mutate(ref[int(s):int(s) + 150], rng, 0.02, 0.005, 0.005, 4))
    qidx = np.arange(200000, dtype=np.int32); tidx = np.repeat(np.arange(2000, dtype=np.int32), 100)
    perm = rng.permutation(200000)
    qidx, tidx = qidx[perm], tidx[perm]
    kw = dict(flag=2, filters=0)
    mat = dna_matrix(2, 2)
    Q = gpu_ctx.upload(reads); T = gpu_ctx.upload(windows)
    try:
        res, cig = gpu_ctx.align_pairs(Q, T, qidx, tidx, mat, 5, **kw)
        assert gpu_ctx.timing()["fill_kernel"].startswith("k_fillpairs<")      # the fused fill, then one reverse pass + traceback
    finally:
        Q.free()
    where = np.empty(200000, dtype=np.int64); where[qidx] = np.arange(200000)      # pair of read r
    bad = []
    try:
        for w in range(2000):
            rs = list(range(100 * w, 100 * w + 100))
            Qw = gpu_ctx.upload([reads[r] for r in rs])
            try:
                bres, bcig = gpu_ctx.align_batch(Qw, T, mat, 5, target_first=w, target_count=1, **kw)
            finally:
                Qw.free()
            for k, r in enumerate(rs):
                g, e = res[where[r]], bres[k, 0]
                if any(int(g[f]) != int(e[f]) for f in FIELDS) or _cig(g, cig) != _cig(e, bcig):
                    bad.append("read %d window %d" % (r, w))
    finally:
        T.free()
    assert not bad, "%d mismatches: %s" % (len(bad), bad[:4])
    _pairs_vs_reference(res, cig, reads, windows, qidx, tidx, dna_matrix(2, 2), 5, sample=rng.choice(200000, 2000, replace=False), **kw)
