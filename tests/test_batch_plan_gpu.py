"""The stream-ordered paths of ssw_gpu_align_batch's launch plan on the device, in small: the pipelined series and the double-buffered form of a
bucket whose column maxima do not fit the budget (the emulator covers in tests/test_emu_pipeline.py cannot see a misplaced event, wait or join:
the emulator's streams are no-ops), the buckets side by side against one after the other, and the loop over targets.  Every run against the
compiled reference, field for field and CIGAR for CIGAR.  (The allocation-retry ladder needs an allocator that refuses: the emulator test stays
its cover.)"""
import numpy as np
import pytest

from parity import compare_batch, make_reads
from sswutil import dna_matrix, random_ref

pytestmark = pytest.mark.gpu

MIXED_LENS = [int(x) for x in np.linspace(20, 700, 27)] + [int(x) for x in np.linspace(30, 380, 13)]      # 40 reads, 20..700


def _run(ctx, reads, refs, scoring, flag):
    """-> (records, the CIGAR of every record, timing); checked against the reference"""
    match, mism, gO, gE = scoring
    mat = dna_matrix(match, mism)
    Q = ctx.upload(reads); T = ctx.upload(refs)
    try:
        res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
    finally:
        Q.free(); T.free()
    tm = ctx.timing()
    bad = compare_batch(res, cig, reads, refs, mat, 5, gO, gE, flag, 0, 0, -1, 2)
    assert not bad, "%s flag %d: " % (scoring, flag) + "\n".join(bad)
    cigars = [tuple(cig[r["cigar_off"]:r["cigar_off"] + r["cigarLen"]]) if r["cigarLen"] > 0 else () for r in res.reshape(-1)]
    return res, cigars, tm


def _same(a, b):
    return all((a[0][f] == b[0][f]).all() for f in a[0].dtype.names if f != "cigar_off") and a[1] == b[1]


@pytest.fixture(scope="module", params=[(100, 150), (100, 160)], ids=["100_150", "100_160"])
def chunked_case(request):
    """64 reads of two lengths against 30 kb: under a budget of 1 MiB a launch holds two pairs (8 bytes x 30 032 columns per pair, one
    set of column maxima per stream), so each of the two buckets is a series of eight launches.  100 and 150 bp both pad to P16 - 8 under
    16-bit rules: with one target both buckets are half-row classes and every launch of the series is k_fill8.  100 and 160 bp: one half-row
    class and one of whole rows, whose series is k_fill's.  -> (reads, target, the kernel of the bucket with the most cells)"""
    ref = random_ref(30000, 41, 4)
    return make_reads(np.random.default_rng(41), ref, 64, list(request.param), 4), ref, "k_fill8<19," if request.param[1] == 150 else "k_fill<10,"


@pytest.fixture(scope="module")
def mixed_case():
    ref = random_ref(20000, 43, 4)
    return make_reads(np.random.default_rng(43), ref, len(MIXED_LENS), MIXED_LENS, 4), ref


@pytest.mark.parametrize("flag", [0, 2])
def test_pipelined_series(gpu_hctx, chunked_case, flag, monkeypatch):
    reads, ref, kernel = chunked_case
    runs = []
    try:
        gpu_hctx.lib.ssw_gpu_set_budget(gpu_hctx.h, 1 << 20)
        for env, pipelined in ((("SSW_GPU_PIPE", "1"), True), (("SSW_GPU_PIPE", "0"), False), (("SSW_GPU_PIPE_PARTS", "3"), True)):
            monkeypatch.setenv(*env)
            runs.append(_run(gpu_hctx, reads, [ref], (2, 2, 3, 1), flag))
            monkeypatch.delenv(env[0])
            t = runs[-1][2]
            assert t["fill_launches"] >= 4 and t["fill_kernel"].startswith(kernel), t
            assert t["fill_pipelined"] == (t["fill_launches"] if pipelined else 0), t
    finally:
        gpu_hctx.lib.ssw_gpu_set_budget(gpu_hctx.h, 0)
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])


@pytest.mark.parametrize("flag", [0, 2])
def test_double_buffered_form(gpu_hctx, chunked_case, flag, monkeypatch):
    reads, ref, kernel = chunked_case
    monkeypatch.setenv("SSW_GPU_OVERLAP", "1")
    try:
        gpu_hctx.lib.ssw_gpu_set_budget(gpu_hctx.h, 1 << 20)
        t = _run(gpu_hctx, reads, [ref], (2, 2, 3, 1), flag)[2]
    finally:
        gpu_hctx.lib.ssw_gpu_set_budget(gpu_hctx.h, 0)
    assert t["fill_launches"] >= 4 and t["fill_pipelined"] == 0 and t["fill_kernel"].startswith(kernel), t


@pytest.mark.parametrize("scoring", [(2, 2, 3, 1), (90, 80, 7, 2)], ids=["frame", "frame_and_int16"])
def test_buckets_side_by_side_and_one_after_the_other(gpu_hctx, mixed_case, scoring, monkeypatch):
    """many short-query buckets and the strip kernel's (reads above 384 bp) in one launch group; with match 90 the classes from 22 rows per
    lane on leave the column frame's range (16 x 22 x 90 = 31 680), so the group has grids of both forms"""
    reads, ref = mixed_case
    group = _run(gpu_hctx, reads, [ref], scoring, 2)
    assert group[2]["fill_launches"] == 1, group[2]
    monkeypatch.setenv("SSW_GPU_SERIAL_BUCKETS", "1")
    serial = _run(gpu_hctx, reads, [ref], scoring, 2)
    assert serial[2]["fill_launches"] > 1, serial[2]
    assert _same(group, serial)


def test_target_loop_with_an_empty_target(gpu_ctx, mixed_case):
    """three targets (below the four that switch to the database path), the second one empty: the per-target memset of the records, the
    query list uploaded again after a traceback that reordered it, the CIGAR pool's offsets across targets"""
    reads, ref = mixed_case
    res, cigars, _ = _run(gpu_ctx, reads, [ref, np.zeros(0, dtype=np.int8), random_ref(8000, 47, 4)], (2, 2, 3, 1), 2)
    assert res.shape == (len(reads), 3) and (res["score1"][:, 1] == 0).all() and (res["score1"][:, 0] > 0).any() and (res["cigarLen"][:, 2] > 0).any()
