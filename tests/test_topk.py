"""ssw_gpu_search_topk: the best k targets of every query (include/ssw_gpu.h).

The expected lists always come from ssw_gpu_align_batch over the whole query x target matrix (and, through it or directly, from the
reference): for query q the eligible targets -- status 0, score1 > 0, score1 >= min_score -- ordered by score1 descending, then target
index ascending; the first k of them, -1 past the last.  Records must equal the align_batch records bit for bit (the CIGAR pool in
(q, r) order).  Every case runs on the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source, small sizes) and,
marked gpu, on the MI355X at larger sizes."""
import os

import numpy as np
import pytest

import ssw_amd
import workloads as W
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, mutate, random_ref

FIELDS = [f for f in ssw_amd.RESULT_DTYPE.names if f != "cigar_off"]
FULL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full")


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def expected_lists(score1, status, k, min_score=1):
    """[nq, nt] score1 / status of align_batch -> expected tidx [nq, k]"""
    nq, nt = score1.shape
    out = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        s = score1[q].astype(np.int64)
        elig = np.flatnonzero((status[q] == 0) & (s > 0) & (s >= min_score))
        order = elig[np.lexsort((elig, -s[elig]))][:k]
        out[q, :len(order)] = order
    return out


def check_topk(ti, res, cig, bres, bcig, k, min_score=1):
    """search_topk's output against the full align_batch matrix (bres [nq, nt], bcig)"""
    et = expected_lists(bres["score1"], bres["status"], k, min_score)
    bad_rows = np.flatnonzero((ti != et).any(axis=1))
    assert len(bad_rows) == 0, "%d rows differ; query %d: got %s expected %s (scores %s)" % (
        len(bad_rows), bad_rows[0], ti[bad_rows[0]].tolist(), et[bad_rows[0]].tolist(),
        [int(bres["score1"][bad_rows[0], t]) for t in et[bad_rows[0]] if t >= 0])
    empty = np.zeros(1, dtype=ssw_amd.RESULT_DTYPE)[0]
    empty["ref_begin1"] = -1; empty["read_begin1"] = -1; empty["cigar_off"] = -1
    bad, woff = [], 0
    for q in range(ti.shape[0]):
        for r in range(k):
            g = res[q, r]
            if ti[q, r] < 0:
                if any(int(g[f]) != int(empty[f]) for f in ssw_amd.RESULT_DTYPE.names):
                    bad.append("q%d r%d: padding slot holds %s" % (q, r, g))
                continue
            e = bres[q, ti[q, r]]
            got = {f: int(g[f]) for f in FIELDS}
            exp = {f: int(e[f]) for f in FIELDS}
            if got != exp or _cig(g, cig) != _cig(e, bcig):
                bad.append("q%d r%d (t%d): batch %s %s, topk %s %s" % (q, r, ti[q, r], exp, cigar_str(_cig(e, bcig)), got, cigar_str(_cig(g, cig))))
            if int(g["cigarLen"]) > 0:
                if int(g["cigar_off"]) != woff:
                    bad.append("q%d r%d: CIGAR at %d, expected %d (pool in (q, r) order)" % (q, r, int(g["cigar_off"]), woff))
                woff += int(g["cigarLen"])
            elif int(g["cigar_off"]) != -1:
                bad.append("q%d r%d: no CIGAR but cigar_off %d" % (q, r, int(g["cigar_off"])))
            if len(bad) >= 4:
                break
    assert not bad, "\n".join(bad)
    assert woff == len(cig), (woff, len(cig))


def same_records(a, b):
    """every field of two record arrays (the struct's padding bytes are not part of a record)"""
    return all((a[f] == b[f]).all() for f in ssw_amd.RESULT_DTYPE.names)


def run_case(ctx, reads, refs, mat, n, ks, chunks, min_score=1, **kw):
    """search_topk for every (k, chunk) against ONE full align_batch of the same parameters; -> the last (tidx, res, cig)"""
    Q = ctx.upload(reads); T = ctx.upload(refs)
    try:
        bres, bcig = ctx.align_batch(Q, T, mat, n, **kw)
        out = None
        for k in ks:
            for ch in chunks:
                ti, res, cig = ctx.search_topk(Q, T, k, mat, n, min_score=min_score, chunk=ch, **kw)
                run_case.timing = ctx.timing()
                check_topk(ti, res, cig, bres, bcig, k, min_score)
                out = (ti, res, cig)
    finally:
        Q.free(); T.free()
    return out, bres


def mixed_set(rng, nq, nt, n_codes, qmax, tmax, empties=True):
    """targets of mixed lengths; queries mutated pieces of some of them (so the lists have a clear head) or random; one empty
    query and one empty target"""
    refs = [np.asarray(random_ref(int(rng.integers(20, tmax + 1)), int(rng.integers(1 << 30)), n_codes), dtype=np.int8) for _ in range(nt)]
    reads = []
    for i in range(nq):
        src = refs[int(rng.integers(0, nt))]
        ql = int(rng.integers(10, qmax + 1))
        if rng.random() < 0.6 and len(src) > 12:
            s = int(rng.integers(0, max(1, len(src) - ql)))
            rd = mutate(src[s:s + ql], rng, 0.05, 0.01, 0.01, n_codes)
            if len(rd) == 0:
                rd = src[:5].copy()
        else:
            rd = random_ref(ql, int(rng.integers(1 << 30)), n_codes)
        reads.append(np.asarray(rd, dtype=np.int8))
    if empties:
        reads[1] = np.zeros(0, dtype=np.int8)
        refs[2] = np.zeros(0, dtype=np.int8)
    return reads, refs


def tie_set(rng, nt, chunk, n_codes=4):
    """many equal scores: duplicated database entries (some at t and t + chunk, so that the ties straddle a chunk boundary) and
    low-complexity entries; queries that hit them"""
    base = [np.asarray(random_ref(int(rng.integers(40, 120)), 900 + i, n_codes), dtype=np.int8) for i in range(4)]
    refs = [np.asarray(random_ref(int(rng.integers(30, 120)), 1000 + i, n_codes), dtype=np.int8) for i in range(nt)]
    for t in range(0, nt, 5):
        refs[t] = base[(t // 5) % 4].copy()
    for t in range(3, nt - chunk, 11):
        refs[t + chunk] = refs[t].copy()
    for t in range(1, nt, 13):
        refs[t] = np.zeros(60 + 7 * (t % 3), dtype=np.int8)           # poly-A of a few lengths: equal scores against an A-run
    reads = [base[i % 4][5:35].copy() for i in range(4)] + [np.zeros(25, dtype=np.int8), refs[3][:30].copy(), refs[4][:20].copy()]
    return reads, refs


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("alphabet", ["dna", "protein"])
def test_emu_mixed_sets(ectx, alphabet):
    rng = np.random.default_rng(11 if alphabet == "dna" else 12)
    if alphabet == "dna":
        reads, refs = mixed_set(rng, 9, 80, 4, 120, 200)
        mat, n, kw = dna_matrix(2, 2), 5, dict(gapO=3, gapE=1)
    else:
        reads, refs = mixed_set(rng, 7, 70, 20, 90, 160)
        mat, n, kw = blosum50(), 24, dict(gapO=10, gapE=2)
    run_case(ectx, reads, refs, mat, n, ks=(1, 5, len(refs) + 3), chunks=(16, 37, 0), **kw)
    assert run_case.timing["fill_kernel"].startswith("k_filldb<")      # the streamed path: selection on the device


def test_emu_ties_across_chunks(ectx):
    rng = np.random.default_rng(21)
    reads, refs = tie_set(rng, 90, 16)
    (ti, _, _), bres = run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(1, 3, 7, 40), chunks=(16, 37, 0))
    s = bres["score1"]
    assert max(int((s[q] == s[q].max()).sum()) for q in range(len(reads))) >= 6      # (the ties the test is about: more than k = 1, 3)


def test_emu_fewer_eligible_than_k(ectx):
    rng = np.random.default_rng(31)
    reads, refs = mixed_set(rng, 6, 50, 4, 60, 150)
    Q = ectx.upload(reads); T = ectx.upload(refs)
    try:
        bres, bcig = ectx.align_batch(Q, T, dna_matrix(2, 2), 5)
        ms = int(np.percentile(bres["score1"], 95))       # excludes most targets
        for min_score, k in ((ms, 20), (ms, 1), (0, 60), (10 ** 4, 4)):
            for ch in (16, 0):
                ti, res, cig = ectx.search_topk(Q, T, k, dna_matrix(2, 2), 5, min_score=min_score, chunk=ch)
                check_topk(ti, res, cig, bres, bcig, k, min_score)
        assert (ti == -1).all()            # min_score above every score: nothing but padding
        ti, res, cig = ectx.search_topk(Q, T, 20, dna_matrix(2, 2), 5, min_score=ms)
        assert (ti == -1).any() and (ti >= 0).any()
    finally:
        Q.free(); T.free()


def test_emu_score_size0_overflow_excluded(ectx):
    rng = np.random.default_rng(41)
    reads, refs = mixed_set(rng, 6, 40, 4, 100, 300)
    refs[5] = random_ref(320, 5, 4); reads[0] = refs[5][50:210].copy()         # 160 x 2 = 320 > 255: the reference returns NULL
    refs[9] = refs[5].copy()
    (ti, res, _), bres = run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(3,), chunks=(16, 0), score_size=0)
    assert int(bres[0, 5]["status"]) == 1 and 5 not in ti[0] and 9 not in ti[0]
    run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(3,), chunks=(0,), score_size=1)


@pytest.mark.parametrize("flag,mm", [(2, False), (15, True)])
def test_emu_flagged(ectx, flag, mm):
    rng = np.random.default_rng(51 + flag)
    reads, refs = mixed_set(rng, 7, 60, 4, 100, 220)
    kw = dict(flag=flag, filters=30 if flag == 2 else 0, filterd=40 if flag == 15 else 0, mark_mismatch=mm)
    (ti, res, cig), _ = run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(1, 4), chunks=(16, 0), **kw)
    assert len(cig) > 0
    rng = np.random.default_rng(52)
    preads, prefs = mixed_set(rng, 5, 40, 20, 80, 150)
    run_case(ectx, preads, prefs, blosum50(), 24, ks=(3,), chunks=(16,), gapO=10, gapE=2, **kw)


def test_emu_generic_path(ectx):
    """outside the fused kernel's envelope: gapO <= gapE, a query over 640 residues, max(mat) > 49, 40 letters"""
    rng = np.random.default_rng(61)
    reads, refs = mixed_set(rng, 5, 30, 4, 80, 200)
    for flag in (0, 2):
        run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(1, 4), chunks=(16, 0), gapO=1, gapE=1, flag=flag)
        assert not run_case.timing["fill_kernel"].startswith("k_filldb<")
    big = random_ref(900, 77, 4)
    lreads = reads + [big[100:800].copy()]
    lrefs = refs + [big]
    run_case(ectx, lreads, lrefs, dna_matrix(2, 2), 5, ks=(3,), chunks=(16,))
    run_case(ectx, reads, refs, dna_matrix(60, 2), 5, ks=(3,), chunks=(0,), flag=15, mark_mismatch=True)
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    r40 = [np.asarray(random_ref(60 + 10 * i, 400 + i, 40), dtype=np.int8) for i in range(12)]
    q40 = [mutate(r40[i][5:50], rng, 0.05, 0.0, 0.0, 40) for i in range(4)]
    run_case(ectx, q40, r40, m40, 40, ks=(2, 20), chunks=(5,), flag=2)


def test_emu_generic_matches_reference(ectx):
    """records of the generic path against the reference itself (flag 2): what align_batch is checked against elsewhere"""
    rng = np.random.default_rng(62)
    reads, refs = mixed_set(rng, 4, 20, 4, 60, 150, empties=False)
    (ti, res, cig), _ = run_case(ectx, reads, refs, dna_matrix(2, 2), 5, ks=(3,), chunks=(0,), gapO=1, gapE=1, flag=2)
    for q in range(len(reads)):
        for r in range(3):
            if ti[q, r] < 0:
                continue
            exp, ecig = expected(reads[q], dna_matrix(2, 2), 5, refs[ti[q, r]], 1, 1, 2, 0, 0, len(reads[q]) // 2, 2)
            assert {f: int(res[q, r][f]) for f in RES_FIELDS} == exp and _cig(res[q, r], cig) == ecig


def test_emu_errors_and_busy(ectx, emu_lib_path):
    Q = ectx.upload([random_ref(30, 1, 4), random_ref(40, 3, 4)]); T = ectx.upload([random_ref(40, 2, 4), random_ref(60, 4, 4)])
    other = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    Qo = other.upload([random_ref(30, 1, 4)])
    try:
        ti = np.full((2, 2), 777, dtype=np.int32); res = np.zeros((2, 2), dtype=ssw_amd.RESULT_DTYPE); res["score1"] = 777
        for k, q, msg in ((0, Q, "k must be"), (SSW_TOPK_MAX + 1, Q, "k must be"), (2, Qo, "another context")):
            with pytest.raises(RuntimeError, match=msg):
                ectx.search_topk(q, T, k, dna_matrix(2, 2), 5, out=(ti, res))
            assert (ti == 777).all() and (res["score1"] == 777).all()
        import ctypes as C
        p = ssw_amd.Params(dna_matrix(2, 2).ctypes.data_as(C.POINTER(C.c_int8)), 5, 3, 1, 0, 0, 0, -1, 2, 0)
        for a_ti, a_res in ((None, res.ctypes.data_as(C.c_void_p)), (ti.ctypes.data_as(C.c_void_p), None)):
            assert ectx.lib.ssw_gpu_search_topk(ectx.h, Q.h, T.h, C.byref(p), 2, 1, 0, a_ti, a_res, None, None) == -1
            assert "NULL" in ectx.error()
        assert ectx.lib.ssw_gpu_search_topk(ectx.h, Q.h, T.h, None, 2, 1, 0, ti.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), None, None) == -1
        assert (ti == 777).all() and (res["score1"] == 777).all()
        # a busy context: search_topk from inside a streamed search's chunk function on the same context
        seen = []

        def inside(t0, hits):
            try:
                ectx.search_topk(Q, T, 2, dna_matrix(2, 2), 5, out=(ti, res))
            except RuntimeError as e:
                seen.append(str(e))
            return 0
        ectx.search_db(Q, T, dna_matrix(2, 2), 5, chunk=1, on_chunk=inside)
        assert seen and all("inside another call" in s for s in seen), seen
        assert (ti == 777).all()
        # nq == 0 and nt == 0
        Q0 = ectx.upload([]); T0 = ectx.upload([])
        try:
            t0, r0, c0 = ectx.search_topk(Q0, T, 3, dna_matrix(2, 2), 5)
            assert t0.shape == (0, 3) and len(c0) == 0
            t1, r1, c1 = ectx.search_topk(Q, T0, 3, dna_matrix(2, 2), 5, flag=2)
            assert (t1 == -1).all() and (r1["ref_begin1"] == -1).all() and (r1["cigar_off"] == -1).all() and (r1["score1"] == 0).all()
        finally:
            Q0.free(); T0.free()
    finally:
        Q.free(); T.free(); Qo.free(); other.close()


SSW_TOPK_MAX = 1024


def test_emu_large_k_and_small_budget(emu_lib_path):
    """k = SSW_GPU_TOPK_MAX (the 2048-key buffer, a radix select on the first chunk) and a 1 MiB budget (several query blocks)"""
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    try:
        rng = np.random.default_rng(71)
        refs = [np.asarray(random_ref(int(rng.integers(8, 30)), 3000 + i, 4), dtype=np.int8) for i in range(1500)]
        reads = [np.asarray(random_ref(12, 77 + i, 4), dtype=np.int8) for i in range(3)]
        run_case(ctx, reads, refs, dna_matrix(2, 2), 5, ks=(SSW_TOPK_MAX, 300), chunks=(0, 700))
        ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
        run_case(ctx, reads, refs, dna_matrix(2, 2), 5, ks=(SSW_TOPK_MAX,), chunks=(0,))
    finally:
        ctx.close()


def test_emu_pool_matches_single_context(emu_lib_path, monkeypatch):
    monkeypatch.setenv("SSW_EMU_DEVICES", "2")
    lib = ssw_amd.load(emu_lib_path)
    rng = np.random.default_rng(81)
    reads, refs = mixed_set(rng, 11, 40, 4, 80, 160)
    ctx = ssw_amd.Context(0, lib)
    pool = ssw_amd.Pool([0, 1], lib)
    try:
        Q = ctx.upload(reads); T = ctx.upload(refs)
        for flag in (0, 15):
            t1, r1, c1 = ctx.search_topk(Q, T, 4, dna_matrix(2, 2), 5, flag=flag)
            pool.set_targets(refs)
            t2, r2, c2 = pool.search_topk(reads, 4, dna_matrix(2, 2), 5, flag=flag, block=3)
            assert (t1 == t2).all() and same_records(r1, r2) and c1.tobytes() == c2.tobytes()
            assert sum(s["blocks"] for s in pool.stats()) == 4
        Q.free(); T.free()
    finally:
        pool.close(); ctx.close()


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", ["dna", "protein"])
def test_gpu_mixed_sets(gpu_ctx, alphabet):
    rng = np.random.default_rng(111 if alphabet == "dna" else 112)
    if alphabet == "dna":
        reads, refs = mixed_set(rng, 300, 900, 4, 400, 1500)
        mat, n, kw = dna_matrix(2, 2), 5, dict(gapO=3, gapE=1)
    else:
        reads, refs = mixed_set(rng, 250, 800, 20, 600, 1000)
        mat, n, kw = blosum50(), 24, dict(gapO=10, gapE=2)
    run_case(gpu_ctx, reads, refs, mat, n, ks=(1, 5, len(refs) + 3), chunks=(16, 37, 0), **kw)
    assert run_case.timing["fill_kernel"].startswith("k_filldb<")


@pytest.mark.gpu
def test_gpu_ties_fewer_eligible_score_size0(gpu_ctx):
    rng = np.random.default_rng(121)
    reads, refs = tie_set(rng, 2000, 37)
    run_case(gpu_ctx, reads * 20, refs, dna_matrix(2, 2), 5, ks=(1, 7, 100, 1024), chunks=(16, 37, 0))
    reads, refs = mixed_set(rng, 200, 600, 4, 300, 800)
    refs[5] = random_ref(320, 5, 4); reads[0] = refs[5][50:210].copy()
    run_case(gpu_ctx, reads, refs, dna_matrix(2, 2), 5, ks=(5,), chunks=(37, 0), score_size=0)
    Q = gpu_ctx.upload(reads); T = gpu_ctx.upload(refs)
    try:
        bres, bcig = gpu_ctx.align_batch(Q, T, dna_matrix(2, 2), 5)
        ms = int(np.percentile(bres["score1"], 97))
        ti, res, cig = gpu_ctx.search_topk(Q, T, 30, dna_matrix(2, 2), 5, min_score=ms, chunk=37)
        check_topk(ti, res, cig, bres, bcig, 30, ms)
        assert (ti == -1).any()
    finally:
        Q.free(); T.free()


@pytest.mark.gpu
@pytest.mark.parametrize("flag,mm", [(2, False), (15, True)])
def test_gpu_flagged(gpu_ctx, flag, mm):
    rng = np.random.default_rng(131 + flag)
    reads, refs = mixed_set(rng, 200, 700, 20, 500, 900)
    kw = dict(gapO=10, gapE=2, flag=flag, filters=60 if flag == 2 else 0, filterd=80 if flag == 15 else 0, mark_mismatch=mm)
    run_case(gpu_ctx, reads, refs, blosum50(), 24, ks=(1, 10), chunks=(37, 0), **kw)


@pytest.mark.gpu
def test_gpu_generic_path(gpu_ctx):
    rng = np.random.default_rng(141)
    reads, refs = mixed_set(rng, 60, 200, 4, 300, 900)
    big = random_ref(1500, 77, 4)
    run_case(gpu_ctx, reads + [big[100:1000].copy()], refs + [big], dna_matrix(2, 2), 5, ks=(1, 6), chunks=(37, 0), flag=2)
    run_case(gpu_ctx, reads, refs, dna_matrix(2, 2), 5, ks=(6,), chunks=(37,), gapO=1, gapE=1, flag=15, mark_mismatch=True)
    run_case(gpu_ctx, reads, refs, dna_matrix(60, 2), 5, ks=(6,), chunks=(0,))
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    r40 = [np.asarray(random_ref(100 + 10 * i, 400 + i, 40), dtype=np.int8) for i in range(40)]
    q40 = [mutate(r40[i][5:90], rng, 0.05, 0.0, 0.0, 40) for i in range(12)]
    run_case(gpu_ctx, q40, r40, m40, 40, ks=(3,), chunks=(16,), flag=2)


@pytest.mark.gpu
def test_gpu_errors_and_busy(gpu_ctx):
    Q = gpu_ctx.upload([random_ref(30, 1, 4)]); T = gpu_ctx.upload([random_ref(40, 2, 4), random_ref(50, 3, 4)])
    try:
        ti = np.full((1, 2), 777, dtype=np.int32); res = np.zeros((1, 2), dtype=ssw_amd.RESULT_DTYPE); res["score1"] = 777
        with pytest.raises(RuntimeError, match="k must be"):
            gpu_ctx.search_topk(Q, T, 1025, dna_matrix(2, 2), 5, out=(ti, res))
        seen = []

        def inside(t0, hits):
            try:
                gpu_ctx.search_topk(Q, T, 2, dna_matrix(2, 2), 5, out=(ti, res))
            except RuntimeError as e:
                seen.append(str(e))
            return 0
        gpu_ctx.search_db(Q, T, dna_matrix(2, 2), 5, chunk=1, on_chunk=inside)
        assert seen and all("inside another call" in s for s in seen)
        assert (ti == 777).all() and (res["score1"] == 777).all()
    finally:
        Q.free(); T.free()


@pytest.mark.gpu
def test_gpu_pool_repeated_device(product_lib_path):
    lib = ssw_amd.load(product_lib_path)
    rng = np.random.default_rng(151)
    reads, refs = mixed_set(rng, 700, 500, 20, 400, 700)
    ctx = ssw_amd.Context(0, lib)
    pool = ssw_amd.Pool([0, 0], lib)
    try:
        Q = ctx.upload(reads); T = ctx.upload(refs)
        pool.set_targets(refs)
        for flag in (0, 2):
            t1, r1, c1 = ctx.search_topk(Q, T, 8, blosum50(), 24, gapO=10, gapE=2, flag=flag)
            t2, r2, c2 = pool.search_topk(reads, 8, blosum50(), 24, gapO=10, gapE=2, flag=flag, block=100)
            assert (t1 == t2).all() and same_records(r1, r2) and c1.tobytes() == c2.tobytes()
        Q.free(); T.free()
    finally:
        pool.close(); ctx.close()


@pytest.mark.gpu
def test_gpu_config5_full_database(gpu_ctx):
    """config 5 at full database size: the first 2 048 queries of protein_config(0) against all 10 000 entries.  The 16 queries of the
    stored reference output: k = 10 and k = 100 lists and records derived from it; all 2 048: lists derived from search_db."""
    z = np.load(os.path.join(FULL, "config5_block0.npz"))
    nq, nt = int(z["nq"]), int(z["nt"])
    db, qs, mat = W.protein_config(0)
    qs = qs[:nq]
    Q = gpu_ctx.upload(qs); T = gpu_ctx.upload(db)
    try:
        hits = gpu_ctx.search_db(Q, T, mat, 24, 3, 1, -1, 2, 0)
        got = {k: gpu_ctx.search_topk(Q, T, k, mat, 24, gapO=3, gapE=1) for k in (10, 100)}
    finally:
        Q.free(); T.free()
    f16 = z["first16"]      # [16, 10000, (score1, score2, ref_end1, read_end1, ref_end2)] from the reference
    for k, (ti, res, cig) in got.items():
        assert len(cig) == 0
        et = expected_lists(f16[..., 0], (f16[..., 4] == -2).astype(np.int32), k)
        assert (ti[:16] == et).all(), "k = %d: the first 16 lists differ from the reference's" % k
        for q in range(16):
            for r in range(k):
                t = ti[q, r]
                rec = res[q, r]
                assert [int(rec["score1"]), int(rec["score2"]), int(rec["ref_end1"]), int(rec["read_end1"]), int(rec["ref_end2"])] == f16[q, t].tolist()
                assert int(rec["ref_begin1"]) == -1 and int(rec["cigarLen"]) == 0 and int(rec["status"]) == 0
        st = (hits["ref_end2"] == -2).astype(np.int32)
        ea = expected_lists(hits["score1"], st, k)
        wrong = np.flatnonzero((ti != ea).any(axis=1))
        assert len(wrong) == 0, "k = %d: %d of %d lists differ from search_db's (first: query %d)" % (k, len(wrong), nq, int(wrong[0]))


@pytest.mark.gpu
def test_gpu_planted_homologs_flagged(gpu_ctx, reflib):
    """queries that are mutated copies of database entries: with flag 0x0f and k = 5, rank 0 is the source entry; a sample of records
    against the reference"""
    rng = np.random.default_rng(77)
    db, qs, _ = W.protein_config(3, queries=192, db_entries=3000)
    mat = blosum50()
    src = rng.integers(0, len(db), size=len(qs))
    qs = [np.ascontiguousarray(mutate(db[int(s)], rng, 0.1, 0.01, 0.01, 20)[:640]) for s in src]
    Q = gpu_ctx.upload(qs); T = gpu_ctx.upload(db)
    try:
        ti, res, cig = gpu_ctx.search_topk(Q, T, 5, mat, 24, gapO=10, gapE=2, flag=0x0f, filterd=32767)
        bres, bcig = gpu_ctx.align_batch(Q, T, mat, 24, gapO=10, gapE=2, flag=0x0f, filterd=32767)
    finally:
        Q.free(); T.free()
    assert (ti[:, 0] == src).mean() == 1.0, "rank 0 is not the source entry for %d queries" % int((ti[:, 0] != src).sum())
    check_topk(ti, res, cig, bres, bcig, 5)
    bad = []
    for q in range(0, len(qs), 8):
        for r in (0, 2, 4):
            t = int(ti[q, r])
            exp, ecig = expected(qs[q], mat, 24, db[t], 10, 2, 0x0f, 0, 32767, len(qs[q]) // 2, 2)
            if {f: int(res[q, r][f]) for f in RES_FIELDS} != exp or _cig(res[q, r], cig) != ecig:
                bad.append("q%d r%d t%d" % (q, r, t))
    assert not bad, bad[:4]
    assert len(cig) > 0


def test_cpp_search_topk_equals_align_pairs_emulated(emu_lib_path, tmp_path):
    """include/ssw_gpu_cpp.h BatchAligner::SearchTopK against AlignPairs over every pair (tests/cpp/topk_check.cpp), on the emulator"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "topk_check_emu")
    emu_dir = os.path.dirname(emu_lib_path)
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "topk_check.cpp"),
                    "-o", exe, "-L" + emu_dir, "-lssw_emu", "-lm", "-Wl,-rpath," + emu_dir], check=True)
    for args in (["8", "40", "5", "1"], ["5", "30", "40", "30"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
