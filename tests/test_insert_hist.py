"""ssw_gpu_insert_hist: the histogram of the spans between the best candidates of the two mates of every fragment (include/ssw_gpu.h).

Per fragment: a and b are what ssw_gpu_align_windows_best would return as `best` of groups 2 f and 2 f + 1; both exist (n_both), either
leads its group's second_score1 by min_margin (n_unique), both lie on one target (n_same); then, per orientation whose strand rule the two
strands satisfy, the span D of the orientation table goes to hist[o][D] (n_in[o]) when 0 <= D <= max_span, else to n_out[o].

Oracle, no fragment left out: Context.align_windows at flag 0 over ALL candidates (test_windows_mates._all) and the rule above in plain
Python integers -- not through k_groupbest.  hist and every field of counts must be equal.  Every case goes through one helper (_run) and
runs on the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source) and, marked gpu, on the MI355X.

Shapes: those of tests/test_windows_mates.py and tests/test_mates_orient.py, whose cases and helpers are reused -- the kernel sees scores,
end columns, lengths, targets and strands only; group sizes, fragment counts and the grid's stride are what can make it go wrong."""
import ctypes as C
import re

import numpy as np
import pytest

import ssw_amd
from sswutil import dna_matrix, random_ref
from test_mates_orient import GRID, _locus_case as orient_locus_case, lib_case, sizes_of
from test_windows_mates import MAT, Case, _all, _case, _locus_case as fr_locus_case, _revcomp, _sizes

ORIENTS = ("fr", "rf", "ff")
FR, RF, FF = 0, 1, 2
NFRAGS = [1, 3, 4, 5, 15, 16, 17, 33]   # row, wavefront and workgroup edges of one 16-lane row per fragment
SPAN_MAX = 65535                        # SSW_GPU_INSERT_SPAN_MAX (include/ssw_gpu.h)
GROUP_MAX = 4096                        # SSW_GPU_MATES_GROUP_MAX


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    lib = ssw_amd.load(emu_lib_path)
    assert lib.ssw_gpu_has_test_hooks() == 1      # SSW_GPU_ISTAT_GROUPS is read
    ctx = ssw_amd.Context(0, lib)
    yield ctx
    ctx.close()


def rule(a0, case, min_score, min_margin, max_span):
    """the header's rule over align_windows' flag-0 records of all candidates -> (hist [3, max_span + 1], counts)"""
    co = [int(x) for x in case.co]
    nf = (len(co) - 1) // 2
    s = [int(x) for x in a0["score1"]]
    ok = [int(st) == 0 and sc > 0 and sc >= min_score for st, sc in zip(a0["status"], s)]
    minus = [int(x) >= case.nfwd for x in case.q]
    ln = [len(case.reads[int(x)]) for x in case.q]
    E = [int(case.b[i]) + int(a0["ref_end1"][i]) for i in range(co[-1])]
    B = [E[i] - ln[i] + 1 for i in range(co[-1])]
    hist = np.zeros((3, max_span + 1), dtype=np.uint32)
    cnt = dict(n_both=0, n_unique=0, n_same=0, n_in=[0, 0, 0], n_out=[0, 0, 0])

    def best(lo, hi):
        order = sorted((i for i in range(lo, hi) if ok[i]), key=lambda i: (-s[i], i))
        return (order[0], s[order[1]] if len(order) > 1 else 0) if order else (None, 0)

    for f in range(nf):
        (a, sa2), (b, sb2) = best(co[2 * f], co[2 * f + 1]), best(co[2 * f + 1], co[2 * f + 2])
        if a is None or b is None:
            continue
        cnt["n_both"] += 1
        if s[a] - sa2 < min_margin or s[b] - sb2 < min_margin:
            continue
        cnt["n_unique"] += 1
        if int(case.t[a]) != int(case.t[b]):
            continue
        cnt["n_same"] += 1
        spans = {}
        if minus[a] != minus[b]:
            p, m = (b, a) if minus[a] else (a, b)
            spans[FR] = E[m] - B[p] + 1
            spans[RF] = E[p] - B[m] + 1
        else:
            spans[FF] = E[a] - B[b] + 1 if minus[a] else E[b] - B[a] + 1
        for o, d in spans.items():
            if 0 <= d <= max_span:
                hist[o, d] += 1
                cnt["n_in"][o] += 1
            else:
                cnt["n_out"][o] += 1
    return hist, cnt


def _call(ctx, case, Q, T, max_span, min_margin=0, min_score=0, mat=MAT, n=5, **kw):
    return ctx.insert_hist(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, mat, n, max_span, min_margin=min_margin,
                           min_score=min_score, **kw)


def _run(ctx, case, max_span, min_margin=0, min_score=0, mat=MAT, n=5, **kw):
    """insert_hist against the oracle, every bin and every counter -> (hist, counts, timing, align_windows' flag-0 records)"""
    Q, T = case.upload(ctx)
    try:
        hist, cnt = _call(ctx, case, Q, T, max_span, min_margin, min_score, mat, n, **kw)
        tm = ctx.timing()
        kw0 = {k: v for k, v in kw.items() if k not in ("flag", "filters", "filterd", "mark_mismatch")}
        a0, _ = _all(ctx, case, Q, T, mat, n, flag=0, **kw0)
    finally:
        Q.free(); T.free()
    ehist, ecnt = rule(a0, case, min_score, min_margin, max_span)
    assert hist.shape == (3, max_span + 1) and hist.dtype == np.uint32
    bad = ["hist[%s][%d]: expected %d, got %d" % (ORIENTS[o], d, ehist[o, d], hist[o, d]) for o, d in np.argwhere(hist != ehist)[:6]]
    assert not bad and cnt == ecnt, "\n".join(bad + ["counts: expected %s, got %s" % (ecnt, cnt)])
    assert [int(x) for x in hist.sum(axis=1)] == cnt["n_in"]
    assert tm["best_flagged"] == 0      # nothing goes on to the reverse pass or the traceback
    return hist, cnt, tm, a0


# ------------------------------------------------------------------------------------------------------------- the cases

def _libraries(ctx, made, nfrag, L, gpu=False):
    """1. fragments of one library: its own row holds them, the three rows differ (a kernel that ignores the orientation cannot pass)"""
    case = lib_case(9700 + ORIENTS.index(made), sizes_of(9710, nfrag, ((1, 1), (2, 3), (4, 4), (3, 1))), L, made)
    for margin in (0, 1):
        hist, cnt, tm, _ = _run(ctx, case, 1000, min_margin=margin)
        o = ORIENTS.index(made)
        assert cnt["n_in"][o] > 0
        assert not (hist[0] == hist[1]).all() and not (hist[0] == hist[2]).all() and not (hist[1] == hist[2]).all()
        assert cnt["n_both"] >= cnt["n_unique"] >= cnt["n_same"] > 0
        if gpu:
            assert tm["reduce_ms"] > 0                    # the device time of k_insertstat


def _grid(ctx, L):
    """2. every (n1, n2) of the grid in one call: empty groups, one-candidate groups, the 16-lane stride, groups over 48"""
    case = lib_case(9720, sizes_of(9721, len(GRID), GRID), L, "fr")
    assert [tuple(int(x) for x in np.diff(case.co)[2 * f:2 * f + 2]) for f in range(len(GRID))] == list(GRID)
    for margin in (0, 1):
        _, cnt, _, _ = _run(ctx, case, 1000, min_margin=margin)
        assert 0 < cnt["n_both"] < len(GRID)


def _counts(ctx, nfrag):
    """3a. fragment counts on the row, wavefront and workgroup edges"""
    case = _case(9150, _sizes(9151 + nfrag, nfrag, ((2, 3),)), 3000)
    _run(ctx, case, 1000)


def _stride(ctx, monkeypatch):
    """3b. 70 fragments on a grid capped at one and at two workgroups: the stride loop runs five and three passes, the last with dead rows"""
    case = _case(9160, _sizes(9161, 70, ((2, 3),)), 3000)
    monkeypatch.delenv("SSW_GPU_ISTAT_GROUPS", raising=False)
    free, fcnt, _, _ = _run(ctx, case, 1000, min_margin=1)
    assert fcnt["n_both"] > 32      # fragments of every pass count
    for groups in ("1", "2"):
        monkeypatch.setenv("SSW_GPU_ISTAT_GROUPS", groups)
        hist, cnt, _, _ = _run(ctx, case, 1000, min_margin=1)
        assert hist.tobytes() == free.tobytes() and cnt == fcnt
    monkeypatch.delenv("SSW_GPU_ISTAT_GROUPS")


def _known_spans(ctx):
    """4. D = 350, D = 260 from a read hanging over column 0, max_span on either side of 350, the wrong order counted in n_out"""
    for made in ORIENTS:
        case = fr_locus_case() if made == "fr" else orient_locus_case(made)
        o = ORIENTS.index(made)
        hist, cnt, _, _ = _run(ctx, case, 350)
        assert int(hist[o, 350]) == 2 and int(hist[o, 260]) == 1 and int(hist[o, 250]) == 0      # (250: what a clamped B would give)
        in350 = cnt["n_in"][o]
        hist, cnt, _, _ = _run(ctx, case, 349)
        assert int(hist[o, 260]) == 1 and cnt["n_in"][o] == in350 - 2
        if made == "fr":      # the FR pairs under RF: D = E(p) - B(m) + 1 = 1059 - 1300 + 1 < 0; fragment 1 lies on two targets
            assert cnt["n_out"][RF] == 3 and cnt["n_in"][RF] == 0 and cnt["n_same"] == cnt["n_unique"] - 1
            assert cnt["n_in"][FF] == 0 and cnt["n_out"][FF] == 1      # fragment 2: both plus, D = 350 > 349
        else:
            assert cnt["n_out"][o] >= 2 + (1 if made == "rf" else 2)   # the two of 350, and the fragments in the wrong order


def _one_bin(ctx):
    """5. 64 copies of one fragment: 64 rows add to one bin"""
    tg = np.asarray(random_ref(3000, 9200, 4), dtype=np.int8)
    U, V = tg[1000:1060].copy(), tg[1300:1350].copy()
    for o, (um, vm) in ((FR, (False, True)), (RF, (True, False)), (FF, (False, False))):
        reads = [_revcomp(U) if um else U, _revcomp(V) if vm else V]      # (a read on the minus strand is stored reverse-complemented)
        rows = [[((2 if um else 0) + 0, 0, 980, 100)], [((2 if vm else 0) + 1, 0, 1280, 100)]]
        case = Case.explicit(reads, [tg], rows * 64)
        hist, cnt, _, _ = _run(ctx, case, 400)
        assert int(hist[o, 350]) == 64 and cnt["n_in"][o] == 64 and cnt["n_same"] == 64


def _margin_case():
    """mate 1 P = tg[1000:1060] (score 120 at its locus); a copy of the locus with column 1030 deleted on the other target (P aligns with
    one inserted residue: 59 x 2 - 3 = 115); mate 2 M = revcomp(tg[1300:1360]): D = 1359 - 1000 + 1 = 360"""
    tg = np.asarray(random_ref(3000, 9200, 4), dtype=np.int8)
    t1 = np.asarray(random_ref(3000, 9201, 4), dtype=np.int8)
    t1[500:559] = np.concatenate([tg[1000:1030], tg[1031:1060]])
    t1[1300:1360] = tg[1300:1360]
    P, M = tg[1000:1060].copy(), _revcomp(tg[1300:1360])
    reads = [P, M] * 4
    nr = len(reads)
    rows = [[(0, 0, 980, 100), (0, 0, 980, 100)], [(nr + 1, 0, 1280, 100)],       # 0: a tie in mate 1's group
            [(2, 1, 480, 100), (2, 0, 980, 100)], [(nr + 3, 0, 1280, 100)],       # 1: the runner-up 5 below the best (listed first)
            [(4, 0, 980, 100)], [(nr + 5, 1, 1280, 100)],                         # 2: the bests on different targets
            [(6, 0, 980, 100)], [(nr + 7, 0, 1280, 100), (nr + 7, 1, 480, 100)]]  # 3: a runner-up that scores next to nothing
    return Case.explicit(reads, [tg, t1], rows)


def _margins(ctx):
    """6. ties, the margin on either side, an ineligible runner-up, bests on different targets"""
    case = _margin_case()
    hist, cnt, _, a0 = _run(ctx, case, 400, min_margin=0)
    assert [int(x) for x in a0["score1"][:5]] == [120, 120, 120, 115, 120]      # the construction: a tie; 5 below
    assert cnt["n_both"] == 4 and cnt["n_unique"] == 4 and cnt["n_same"] == 3 and int(hist[FR, 360]) == 3
    hist, cnt, _, _ = _run(ctx, case, 400, min_margin=1)          # the tie no longer contributes
    assert cnt["n_unique"] == 3 and cnt["n_same"] == 2 and int(hist[FR, 360]) == 2
    hist, cnt, _, _ = _run(ctx, case, 400, min_margin=5)          # 120 - 115 = 5 passes
    assert cnt["n_unique"] == 3 and int(hist[FR, 360]) == 2
    hist, cnt, _, _ = _run(ctx, case, 400, min_margin=6)          # ... and fails at 6
    assert cnt["n_unique"] == 2 and int(hist[FR, 360]) == 1
    hist, cnt, _, _ = _run(ctx, case, 400, min_margin=6, min_score=116)      # the runner-up is not eligible: it does not count against the margin
    assert cnt["n_both"] == 4 and cnt["n_unique"] == 3 and int(hist[FR, 360]) == 2
    hist, cnt, _, _ = _run(ctx, case, 400, min_margin=65535)
    assert cnt["n_both"] == 4 and cnt["n_unique"] == 0 and int(hist.sum()) == 0


def _flags(ctx, nfrag, L):
    """7. params.flag, filters, filterd and mark_mismatch are not looked at"""
    case = lib_case(9700, sizes_of(9710, nfrag, ((1, 1), (2, 3), (4, 4), (3, 1))), L, "fr")
    ref, rcnt, _, _ = _run(ctx, case, 1000, min_margin=1)
    for kw in (dict(flag=2), dict(flag=15, mark_mismatch=True), dict(flag=2, filters=120, filterd=50)):
        hist, cnt, _, _ = _run(ctx, case, 1000, min_margin=1, **kw)
        assert hist.tobytes() == ref.tobytes() and cnt == rcnt


def _envelope_case():
    """test_windows_mates._envelopes' mix: a 700-residue read (the fallback), an 800-residue read (the strip kernel's pair mode), empty
    windows, short reads"""
    tg = np.asarray(random_ref(6000, 9600, 4), dtype=np.int8)
    other = np.asarray(random_ref(2000, 9601, 4), dtype=np.int8)
    reads = [tg[1000:1800].copy(), _revcomp(tg[2500:3200]), tg[300:400].copy(), _revcomp(tg[500:580]), tg[4000:4100].copy(), _revcomp(tg[4300:4390])]
    nr = len(reads)
    rows = [[(0, 0, 900, 1000), (2, 1, 0, 200)], [(nr + 1, 0, 2400, 900), (nr + 3, 1, 100, 200)],
            [(0, 1, 0, 1000), (2, 0, 250, 200), (nr + 1, 1, 500, 900)], [(nr + 3, 0, 77, 0), (nr + 3, 0, 450, 200)],
            [(4, 0, 3950, 200)], [(nr + 5, 0, 77, 0)],
            [(4, 0, 3950, 200), (4, 0, 3900, 300)], [(nr + 5, 0, 4250, 200)]]
    return Case.explicit(reads, [tg, other], rows)


def _envelopes(ctx):
    """8. candidates outside the fused kernel's envelopes: their flag-0 records join the device array"""
    case = _envelope_case()
    hist, cnt, tm, _ = _run(ctx, case, 5000)
    assert tm["win_copied"] > 0 and cnt["n_both"] == 3 and cnt["n_in"][FR] == 3
    assert int(hist[FR, 3199 - 1000 + 1]) == 1 and int(hist[FR, 579 - 300 + 1]) == 1 and int(hist[FR, 4389 - 4000 + 1]) == 1
    _, cnt, tm, _ = _run(ctx, case, 5000, gapO=1, gapE=1)        # gapO <= gapE: every candidate takes the fallback
    assert not tm["fill_kernel"].startswith("k_fillpairs<") and cnt["n_both"] == 3
    _, cnt, tm, _ = _run(ctx, case, 5000, mat=dna_matrix(50, 3))      # max(mat) > 49: outside k_fillpairs' envelope
    assert not tm["fill_kernel"].startswith("k_fillpairs<") and cnt["n_both"] == 3


def _small_budget(lib_path, nfrag, L):
    """9. a budget of 1 MiB: several fill launches, one selection afterwards"""
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        case = _case(9800, _sizes(9801, nfrag, ((0, 20), (33, 17))), L, qlen=(64, 64), wlen=(230, 250))
        h0, c0, tm0, _ = _run(ctx, case, 1000, min_margin=1)
        ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
        h1, c1, tm1, _ = _run(ctx, case, 1000, min_margin=1)
        ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        assert tm1["fill_launches"] > 1 and tm1["fill_launches"] > tm0["fill_launches"] and tm1["win_copied"] == 0
        assert h0.tobytes() == h1.tobytes() and c0 == c1 and c0["n_same"] > 0
    finally:
        ctx.close()


def _errors(ctx, other_ctx):
    """10. refused calls leave hist and counts alone and the context usable"""
    reads = [random_ref(30, 1, 4), random_ref(30, 4, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    case = Case.explicit(reads, targets, [[(0, 0, 0, 40), (0, 1, 5, 50)], [(3, 0, 10, 30)]])
    Q, T = case.upload(ctx); Qo = other_ctx.upload(reads)
    ok = dict(cand_off=[0, 2, 3], qidx=[0, 0, 3], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30])
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    kinds = (("cand_off", np.int64), ("qidx", np.int32), ("tidx", np.int32), ("tbeg", np.int64), ("tlen", np.int32))

    def sentinel(span):
        hist = np.full((3, span + 1), 0x5a5a5a5a, dtype=np.uint32)
        cnt = ssw_amd.INSERT_COUNTS(); C.memset(C.byref(cnt), 0x5a, C.sizeof(cnt))
        return hist, cnt

    def call(arr, hist, cnt, Qx=Q, nfrag=1, nfwd=2, margin=0, span=100, flag=0, null=()):
        p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
        a = [ctx.h, Qx.h, T.h, arr[0].ctypes.data, nfrag, arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data, arr[4].ctypes.data, nfwd,
             C.byref(p), 0, margin, span, hist.ctypes.data, C.byref(cnt)]
        for at in null:
            a[at] = None
        return ctx.lib.ssw_gpu_insert_hist(*a)

    def untouched(hist, cnt):
        return (hist == 0x5a5a5a5a).all() and bytes(cnt) == b"\x5a" * C.sizeof(cnt)

    def refused(what, change=None, **kw):
        args = {f: list(v) for f, v in ok.items()}
        for f, (at, v) in (change or {}).items():
            args[f][at] = v
        hist, cnt = sentinel(100)
        arr = [np.ascontiguousarray(args[f], dtype=d) for f, d in kinds]
        rc = call(arr, hist, cnt, **kw)
        assert rc == -1 and re.search(what, ctx.error()), ctx.error()
        assert untouched(hist, cnt)
        _, c2, _, _ = _run(ctx, case, 100)      # the context answers the next call
        assert c2["n_both"] == 1
    try:
        refused(r"cand_off\[0\] must be 0.*fragment 0", dict(cand_off=(0, 1)))
        refused(r"cand_off decreases.*fragment 0, mate 2", dict(cand_off=(1, 4)))
        refused(r"insert_hist: window out of range.*pair 2\b", dict(tlen=(2, 31)))
        refused(r"insert_hist: index out of range.*pair 1\b", dict(tidx=(1, 2)))
        refused(r"nfwd outside.*nfwd = 5", nfwd=5)
        refused(r"nfwd outside.*nfwd = -1", nfwd=-1)
        refused(r"min_margin must be 0 \.\. 65535.*= -1", margin=-1)
        refused(r"min_margin must be 0 \.\. 65535.*= 65536", margin=65536)
        refused(r"max_span must be 0 \.\. 65535.*= -1", span=-1)
        refused(r"max_span must be 0 \.\. 65535.*= 65536", span=SPAN_MAX + 1)
        refused("another context", Qx=Qo)
        hist, cnt = sentinel(100)
        big = np.array([0, GROUP_MAX + 1, GROUP_MAX + 2], dtype=np.int64)      # refused from cand_off alone, before a candidate is read
        arr = [big] + [np.zeros(4, dtype=d) for d in (np.int32, np.int32, np.int64, np.int32)]
        assert call(arr, hist, cnt) == -1 and re.search(r"more than 4096 candidates in a group.*fragment 0, mate 1", ctx.error()), ctx.error()
        arr[0] = np.array([0, 1, 3], dtype=np.int64)
        assert call(arr, hist, cnt, nfrag=0x7fffff00 // 2 + 1) == -1 and "more than 2^31 output slots" in ctx.error()
        assert untouched(hist, cnt)
        # NULL arrays, hist and counts, straight through the C ABI
        arr = [np.ascontiguousarray(ok[f], dtype=d) for f, d in kinds]
        for at in (1, 2, 3, 5, 6, 7, 8, 10, 14, 15):
            assert call(arr, hist, cnt, null=(at,)) == -1 and "NULL argument" in ctx.error()
            assert untouched(hist, cnt)
        assert call(arr, hist, cnt, nfrag=0, null=(14,)) == -1 and call(arr, hist, cnt, nfrag=0, null=(15,)) == -1      # also without fragments
        # no fragments: both zeroed; fragments without candidates: likewise
        assert call(arr, hist, cnt, nfrag=0) == 0 and not hist.any() and bytes(cnt) == b"\x00" * C.sizeof(cnt)
        e = np.zeros(0, np.int32)
        h, c = ctx.insert_hist(Q, T, [0], e, e, np.zeros(0, np.int64), e, 2, MAT, 5, 100)
        assert h.shape == (3, 101) and not h.any() and c == dict(n_both=0, n_unique=0, n_same=0, n_in=[0, 0, 0], n_out=[0, 0, 0])
        h, c = ctx.insert_hist(Q, T, [0, 0, 0, 0, 0], e, e, np.zeros(0, np.int64), e, 2, MAT, 5, 100)
        assert not h.any() and c["n_both"] == 0
        # max_span == 0 is valid: one bin per row, everything else out of range
        hist, cnt, _, _ = _run(ctx, case, 0)
        assert hist.shape == (3, 1) and cnt["n_both"] == 1
        hist, cnt = sentinel(0)
        assert call(arr, hist, cnt, span=0) == 0 and (hist < 2).all()
        with pytest.raises(ValueError):
            ctx.insert_hist(Q, T, [0, 1], [0], [0], [0], [1], 2, MAT, 5, 100)
        with pytest.raises(ValueError):
            ctx.insert_hist(Q, T, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], 2, MAT, 5, SPAN_MAX + 1)
        with pytest.raises(RuntimeError, match="min_margin must be"):
            ctx.insert_hist(Q, T, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], 2, MAT, 5, 100, min_margin=70000)
    finally:
        Q.free(); T.free(); Qo.free()


# ---------------------------------------------------------------------------------------------------------------- emulator

E_L = 3000


@pytest.mark.parametrize("made", ORIENTS)
def test_emu_libraries(ectx, made):
    _libraries(ectx, made, 33, E_L)


def test_emu_group_size_grid(ectx):
    _grid(ectx, E_L)


@pytest.mark.parametrize("nfrag", NFRAGS)
def test_emu_fragment_counts(ectx, nfrag):
    _counts(ectx, nfrag)


def test_emu_grid_stride(ectx, monkeypatch):
    _stride(ectx, monkeypatch)


def test_emu_known_spans(ectx):
    _known_spans(ectx)


def test_emu_one_bin_many_rows(ectx):
    _one_bin(ectx)


def test_emu_margin_and_eligibility(ectx):
    _margins(ectx)


def test_emu_flag_independence(ectx):
    _flags(ectx, 20, E_L)


def test_emu_out_of_envelope_candidates(ectx):
    _envelopes(ectx)


def test_emu_small_budget(emu_lib_path):
    _small_budget(emu_lib_path, 120, 20000)


def test_emu_errors(ectx):
    other = ssw_amd.Context(0, ectx.lib)
    try:
        _errors(ectx, other)
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("made", ORIENTS)
def test_gpu_libraries(gpu_ctx, made):
    _libraries(gpu_ctx, made, 33, E_L, gpu=True)


@pytest.mark.gpu
def test_gpu_group_size_grid(gpu_ctx):
    _grid(gpu_ctx, E_L)


@pytest.mark.gpu
@pytest.mark.parametrize("nfrag", NFRAGS)
def test_gpu_fragment_counts(gpu_ctx, nfrag):
    _counts(gpu_ctx, nfrag)


@pytest.mark.gpu
def test_gpu_grid_stride(gpu_hctx, monkeypatch):
    _stride(gpu_hctx, monkeypatch)


@pytest.mark.gpu
def test_gpu_known_spans(gpu_ctx):
    _known_spans(gpu_ctx)


@pytest.mark.gpu
def test_gpu_one_bin_many_rows(gpu_ctx):
    _one_bin(gpu_ctx)


@pytest.mark.gpu
def test_gpu_margin_and_eligibility(gpu_ctx):
    _margins(gpu_ctx)


@pytest.mark.gpu
def test_gpu_flag_independence(gpu_ctx):
    _flags(gpu_ctx, 20, E_L)


@pytest.mark.gpu
def test_gpu_out_of_envelope_candidates(gpu_ctx):
    _envelopes(gpu_ctx)


@pytest.mark.gpu
def test_gpu_small_budget(product_lib_path):
    _small_budget(product_lib_path, 120, 20000)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    other = ssw_amd.Context(0, gpu_ctx.lib)
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()
