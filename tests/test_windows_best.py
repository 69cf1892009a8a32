"""ssw_gpu_align_windows_best: the best candidate window of every read (include/ssw_gpu.h).

Group g of a call is candidates [cand_off[g], cand_off[g + 1]); a candidate is what a pair of ssw_gpu_align_windows is.  Two oracles, no
group left out: (a) Context.align_windows over ALL candidates with the same parameters, then the selection rule in numpy -- eligible:
status 0, score1 > 0, score1 >= min_score; order: score1 descending, then position ascending -- compared with `sel` (all fields),
`results` (all fields, cigar_off included) and the pool bytes; (b) the reference through parity.expected() on the winner's cut-out window
(every winner on the emulator, a fixed-seed sample of 400 on the GPU).  The planted-read cases assert the chosen candidate without either.
Every case runs on the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source, small sizes) and, marked gpu, on the
MI355X at larger sizes."""
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


def _revcomp(r):
    r = np.asarray(r, dtype=np.int8)[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


def _select(ares, acig, cand_off, min_score):
    """the selection rule over align_windows' records of all candidates -> (sel, records, pool) as align_windows_best must return them"""
    ng = len(cand_off) - 1
    sel = np.zeros(ng, dtype=ssw_amd.BEST_DTYPE)
    res = np.zeros(ng, dtype=ssw_amd.RESULT_DTYPE)
    res["ref_begin1"] = -1; res["read_begin1"] = -1; res["cigar_off"] = -1
    sel["best"] = -1; sel["second"] = -1
    ok = (ares["status"] == 0) & (ares["score1"] > 0) & (ares["score1"].astype(np.int64) >= min_score)
    pool = []
    words = 0
    for g in range(ng):
        c0, c1 = int(cand_off[g]), int(cand_off[g + 1])
        e = np.nonzero(ok[c0:c1])[0]
        sel["n_eligible"][g] = len(e)
        if len(e) == 0:
            continue
        order = e[np.argsort(-ares["score1"][c0:c1][e].astype(np.int64), kind="stable")]      # ties: the lower position first
        sel["best"][g] = order[0]
        if len(order) > 1:
            sel["second"][g] = order[1]
            sel["second_score1"][g] = ares["score1"][c0 + order[1]]
        r = ares[c0 + order[0]].copy()
        if int(r["cigarLen"]) > 0 and int(r["cigar_off"]) >= 0:
            pool.append(acig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigarLen"])])
            r["cigar_off"] = words
            words += int(r["cigarLen"])
        res[g] = r
    return sel, res, (np.concatenate(pool) if pool else np.zeros(0, dtype=np.uint32))


def _check(ctx, reads, targets, cand_off, qidx, tidx, tbeg, tlen, mat, n, min_score=0, sample=None, T=None, Q=None, **kw):
    """align_windows_best against oracle (a) for every group and oracle (b) for every winner (or the winners of the groups in `sample`);
    `reads` are the host copies of the uploaded set Q (reverse complements included where the case has them) -> (sel, records, pool, timing)"""
    cand_off = np.asarray(cand_off, dtype=np.int64); qidx = np.asarray(qidx, dtype=np.int32); tidx = np.asarray(tidx, dtype=np.int32)
    tbeg = np.asarray(tbeg, dtype=np.int64); tlen = np.asarray(tlen, dtype=np.int32)
    ng = len(cand_off) - 1
    Qn = Q if Q is not None else ctx.upload(reads); Tn = T if T is not None else ctx.upload(targets)
    try:
        sel, res, cig = ctx.align_windows_best(Qn, Tn, cand_off, qidx, tidx, tbeg, tlen, mat, n, min_score=min_score, **kw)
        tm = ctx.timing()
        ares, acig = ctx.align_windows(Qn, Tn, qidx, tidx, tbeg, tlen, mat, n, **kw)
    finally:
        if Q is None:
            Qn.free()
        if T is None:
            Tn.free()
    esel, eres, ecig = _select(ares, acig, cand_off, min_score)
    bad = []
    for g in np.nonzero((sel != esel) | (res != eres))[0][:4]:
        bad.append("group %d (candidates [%d, %d)): expected %s %s %s, got %s %s %s" % (
            g, cand_off[g], cand_off[g + 1], esel[g], eres[g], cigar_str(_cig(eres[g], ecig)), sel[g], res[g], cigar_str(_cig(res[g], cig))))
    assert not bad, "\n".join(bad)
    assert (sel == esel).all() and (sel["pad"] == 0).all()
    assert (res == eres).all()                          # every field, cigar_off included
    assert cig.tobytes() == ecig.tobytes()
    assert tm["best_flagged"] <= ng
    if kw.get("flag", 0) == 0:
        assert tm["best_flagged"] == 0
    gapO, gapE, flag = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("flag", 0)
    if not kw.get("mark_mismatch", False):
        for g in (range(ng) if sample is None else sample):
            if int(sel["best"][g]) < 0:
                continue
            i = int(cand_off[g]) + int(sel["best"][g])
            rd = reads[qidx[i]]
            rf = np.ascontiguousarray(targets[int(tidx[i])][int(tbeg[i]):int(tbeg[i]) + int(tlen[i])])
            ml = kw.get("maskLen", -1)
            exp, xcig = expected(rd, mat, n, rf, gapO, gapE, flag, kw.get("filters", 0), kw.get("filterd", 0), ml if ml >= 0 else len(rd) // 2,
                                 kw.get("score_size", 2))
            r = res[g]
            ok = exp is not None and int(r["status"]) == 0 and {k: int(r[k]) for k in RES_FIELDS} == exp and _cig(r, cig) == xcig
            if not ok and len(bad) < 4:
                bad.append("group %d winner %d (len %d x %d): expected %s %s got %s" % (g, i, len(rd), len(rf), exp, cigar_str(xcig), r))
        assert not bad, "\n".join(bad)
    return sel, res, cig, tm


def _assert_fast(tm, gpu=False):
    assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
    if gpu:
        assert tm["reduce_ms"] > 0          # the device time of k_groupbest


def _groups_case(rng, sizes, L, qlen, wmin, wmax, ntargets=2, strands=False, dup_every=3, n_codes=4, sub=0.02):
    """one read per group, planted in ONE of the group's candidate windows, the others decoys elsewhere; every dup_every-th group of two or
    more candidates holds the planted window twice.  strands: odd groups carry the reverse complement of the planted sequence as their read,
    so that the planted candidate is a reverse-strand one (qidx = count + i) -- and every other candidate of every group alternates strands.
    -> (reads [+ reverse complements], targets, cand_off, qidx, tidx, tbeg, tlen, planted position per group (-1: empty group), base read count)"""
    targets = [np.asarray(random_ref(L + 37 * k, int(rng.integers(1 << 30)), n_codes), dtype=np.int8) for k in range(ntargets)]
    nr = len(sizes)
    reads, cand_off, qidx, tidx, tbeg, tlen, planted = [], [0], [], [], [], [], []
    for g, sz in enumerate(sizes):
        t = int(rng.integers(ntargets)); wl = int(rng.integers(wmin, wmax + 1)); wb = int(rng.integers(0, len(targets[t]) - wl + 1))
        o = int(rng.integers(0, wl - qlen + 1))
        seq = np.asarray(mutate(targets[t][wb + o:wb + o + qlen], rng, sub, 0.0, 0.0, n_codes), dtype=np.int8)
        rev = strands and g % 2 == 1
        reads.append(_revcomp(seq) if rev else seq)
        pl = int(rng.integers(sz)) if sz > 0 else -1
        dup = (pl + 1 + int(rng.integers(sz - 1))) % sz if sz >= 2 and g % dup_every == 0 else -1
        for k in range(sz):
            if k == pl or k == dup:
                tidx.append(t); tbeg.append(wb); tlen.append(wl)
                qidx.append(g + nr if rev else g)
            else:
                while True:      # a decoy that does not reach the planted read
                    dt = int(rng.integers(ntargets)); dl = int(rng.integers(wmin, wmax + 1)); db = int(rng.integers(0, len(targets[dt]) - dl + 1))
                    if dt != t or db + dl <= wb + o or db >= wb + o + qlen:
                        break
                tidx.append(dt); tbeg.append(db); tlen.append(dl)
                qidx.append(g + nr if strands and (k + g) % 2 == 1 else g)
        planted.append(min(pl, dup) if dup >= 0 else pl)
        cand_off.append(len(qidx))
    if strands:
        reads = reads + [_revcomp(r) for r in reads]
    return reads, targets, np.array(cand_off, dtype=np.int64), np.array(qidx, dtype=np.int32), np.array(tidx, dtype=np.int32), \
        np.array(tbeg, dtype=np.int64), np.array(tlen, dtype=np.int32), np.array(planted), nr


def _flag_kw(flag):
    return dict(gapO=3, gapE=1, flag=flag, filters=30 if flag == 2 else 0, filterd=40 if flag == 15 else 0)


def _check_planted(ctx, case, mat, n, strands=False, **kw):
    reads, targets, co, q, t, b, l, planted, nr = case
    if strands:
        base = ctx.upload(reads[:nr]); Q = base.with_revcomp(); base.free()
    else:
        Q = ctx.upload(reads)
    try:
        sel, res, cig, tm = _check(ctx, reads, targets, co, q, t, b, l, mat, n, Q=Q, **kw)
    finally:
        Q.free()
    assert (sel["best"] == planted).all(), np.nonzero(sel["best"] != planted)[0][:8]      # independent of either oracle
    sizes = np.diff(co)
    dup = np.array([g for g in range(len(sizes)) if sizes[g] >= 2 and sel["second"][g] >= 0 and
                    (t[co[g] + sel["second"][g]], b[co[g] + sel["second"][g]], l[co[g] + sel["second"][g]]) ==
                    (t[co[g] + sel["best"][g]], b[co[g] + sel["best"][g]], l[co[g] + sel["best"][g]]) and
                    q[co[g] + sel["second"][g]] == q[co[g] + sel["best"][g]]], dtype=np.int64)
    if len(dup):      # a tie through a duplicated window: the lower position wins, the runner-up has the winner's score
        assert (sel["second"][dup] > sel["best"][dup]).all() and (sel["second_score1"][dup] == res["score1"][dup]).all()
    return sel, res, cig, tm, dup


SIZES = [0, 1, 2, 17, 64, 65, 3, 0, 2, 5]


def _group_sizes(ctx, big, qlen, wmin, wmax, L, sizes=SIZES, gpu=False):
    rng = np.random.default_rng(6100)
    case = _groups_case(rng, list(sizes) + [big], L, qlen, wmin, wmax)
    for kw in (dict(flag=0), dict(flag=15, filterd=32767)):
        sel, res, cig, tm, dup = _check_planted(ctx, case, MAT, 5, **kw)
        _assert_fast(tm, gpu)
        assert len(dup) >= 2
        sizes_ = np.diff(case[2])
        assert (sel["best"][sizes_ == 0] == -1).all() and (sel["n_eligible"][sizes_ == 0] == 0).all() and (res["cigar_off"][sizes_ == 0] == -1).all()
        assert (sel["second"][sizes_ == 1] == -1).all() and (sel["second_score1"][sizes_ == 1] == 0).all()
        assert int(sel["n_eligible"][-1]) > big // 2
        if kw["flag"] == 15:
            assert tm["best_flagged"] == int((sel["best"] >= 0).sum())
            assert (res["cigarLen"][sel["best"] >= 0] > 0).all()


def _flags(ctx, flag, ngroups, qlen, wmin, wmax, L, gpu=False):
    rng = np.random.default_rng(6200 + flag)
    sizes = [int(x) for x in rng.integers(1, 9, size=ngroups)]
    case = _groups_case(rng, sizes, L, qlen, wmin, wmax, strands=True)
    for extra in (dict(), dict(mark_mismatch=True)) if flag in (2, 15) else (dict(),):
        sel, _, _, tm, _ = _check_planted(ctx, case, MAT, 5, strands=True, **_flag_kw(flag), **extra)
        _assert_fast(tm, gpu)
    rev = case[3][case[2][:-1] + sel["best"]] >= case[8]
    assert rev.any() and not rev.all()          # winners on both strands


def _min_score(ctx, ngroups, qlen, wmin, wmax, L):
    """min_score between the decoys' scores and the planted ones: one eligible candidate per group (two with a duplicate); above
    everything: nothing is eligible; score_size 0 with a read that overflows 8 bits: status 1, never chosen"""
    rng = np.random.default_rng(6300)
    sizes = [int(x) for x in rng.integers(1, 7, size=ngroups)]
    case = _groups_case(rng, sizes, L, qlen, wmin, wmax, sub=0.0)
    reads, targets, co, q, t, b, l, planted, _ = case
    sel, res, _, tm, dup = _check_planted(ctx, case, MAT, 5, min_score=2 * qlen - 10, flag=2)
    assert (res["score1"] == 2 * qlen).all() and set(np.unique(sel["n_eligible"])) <= {1, 2} and len(dup) > 0
    assert (sel["n_eligible"][dup] == 2).all()
    for ms in (2 * qlen + 1, 70000):
        sel, res, cig, tm = _check(ctx, reads, targets, co, q, t, b, l, MAT, 5, min_score=ms, flag=2)
        assert (sel["best"] == -1).all() and (sel["n_eligible"] == 0).all() and (res["cigar_off"] == -1).all() and len(cig) == 0
        assert tm["best_flagged"] == 0
    if 2 * qlen > 255 - 2:      # 8-bit overflow with score_size 0: the reference returns NULL for the planted candidates
        sel, res, _, _ = _check(ctx, reads, targets, co, q, t, b, l, MAT, 5, flag=0, score_size=0)
        assert (sel["best"] != planted).all()
        Q = ctx.upload(reads); T = ctx.upload(targets)
        try:
            ares, _ = ctx.align_windows(Q, T, q, t, b, l, MAT, 5, score_size=0)
        finally:
            Q.free(); T.free()
        assert (ares["status"][co[:-1] + planted] == 1).all()


def _protein(ctx, ngroups, qlen, L):
    rng = np.random.default_rng(6400)
    sizes = [int(x) for x in rng.integers(1, 6, size=ngroups)]
    case = _groups_case(rng, sizes, L, qlen, 2 * qlen, 4 * qlen, n_codes=20, sub=0.1)
    for extra in (dict(), dict(mark_mismatch=True)):
        _, _, _, tm, _ = _check_planted(ctx, case, blosum50(), 24, gapO=10, gapE=2, flag=2, filters=40, **extra)
        _assert_fast(tm)


def _envelope_mix(ctx, big_window):
    """candidates outside the fused kernel's envelope inside ordinary groups: a 700-residue read (winner in group 0, loser in group 1), an
    empty window (a loser in group 2, alone in group 3: its score is 0, so by the eligibility rule it cannot win), and -- big_window > 0 --
    a window of that many columns (winner in group 5, loser in group 6)"""
    rng = np.random.default_rng(6500)
    L = max(3000, 2 * big_window + 3000)
    target = np.asarray(random_ref(L, 651, 4), dtype=np.int8)
    other = np.asarray(random_ref(2000, 652, 4), dtype=np.int8)
    long_read = target[1000:1700].copy()
    short = [target[1200 + 90 * k:1260 + 90 * k].copy() for k in range(4)]
    reads = [long_read] + short + [target[300:900].copy()]      # (read 5: 600 residues, inside the envelope)
    rows = [[(0, 0, 900, 900), (1, 0, 1100, 300), (0, 1, 100, 900), (1, 1, 0, 500)],          # the long read's true window wins over a planted short read
            [(0, 1, 50, 800), (5, 0, 250, 700), (2, 1, 0, 300)],                                  # the long read against a foreign window loses
            [(3, 0, 1400, 0), (3, 0, 1350, 200), (3, 1, 10, 250)],                                # an empty window among ordinary candidates
            [(4, 0, 77, 0)],                                                                      # ... and alone
            [(1, 1, 5, 400), (1, 0, 1150, 260)]]                                                  # an ordinary group
    if big_window > 0:
        reads.append(target[2500 + big_window - 1000:2500 + big_window - 850].copy())
        bq = len(reads) - 1
        rows.append([(2, 1, 100, 400), (bq, 0, 2500, big_window), (bq, 1, 0, 700)])               # the big window holds its read: it wins
        rows.append([(5, 0, 250, 700), (5, 0, 2400, big_window)])                                 # a read's own window beats the big foreign one
    co = np.cumsum([0] + [len(r) for r in rows])
    q, t, b, l = (np.array(c) for c in zip(*[x for r in rows for x in r]))
    for kw in (dict(flag=0), dict(flag=2, filters=20), dict(flag=15, filterd=32767, mark_mismatch=True)):
        sel, res, _, tm = _check(ctx, reads, [target, other], co, q, t, b, l, MAT, 5, **kw)
        assert [int(x) for x in sel["best"][:5]] == [0, 1, 1, -1, 1] and int(res["score1"][0]) == 1400
        assert int(sel["n_eligible"][3]) == 0 and int(res["cigar_off"][3]) == -1
        if big_window > 0:
            assert [int(x) for x in sel["best"][5:]] == [1, 0] and int(res["score1"][5]) == 300
        assert tm["win_copied"] > 0
        if kw["flag"]:
            assert tm["best_flagged"] == int((sel["best"] >= 0).sum())


def _whole_call_fallbacks(ctx, ngroups, qlen):
    rng = np.random.default_rng(6600)
    sizes = [int(x) for x in rng.integers(0, 5, size=ngroups)]
    case = _groups_case(rng, sizes, 1500, qlen, 2 * qlen, 4 * qlen)
    for flag in (0, 2):      # gapO <= gapE: every candidate leaves the fast path
        _, _, _, tm, _ = _check_planted(ctx, case, MAT, 5, gapO=1, gapE=1, flag=flag)
        assert tm["win_copied"] > 0 and not tm["fill_kernel"].startswith("k_fillpairs<")
    m40 = np.full((40, 40), -1, dtype=np.int8); np.fill_diagonal(m40, 3)
    case = _groups_case(rng, sizes, 1500, qlen, 2 * qlen, 4 * qlen, n_codes=40)
    _, _, _, tm, _ = _check_planted(ctx, case, m40, 40, flag=2)
    assert tm["win_copied"] > 0


def _small_budget(lib_path, budget, ngroups, qlen, wlen, L):
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        rng = np.random.default_rng(6700)
        sizes = [int(x) for x in rng.integers(1, 5, size=ngroups)]
        reads, targets, co, q, t, b, l, planted, _ = _groups_case(rng, sizes, L, qlen, wlen, wlen + wlen // 4, ntargets=1)
        Q = ctx.upload(reads); T = ctx.upload(targets)
        for flag in (0, 2):
            s0, r0, c0 = ctx.align_windows_best(Q, T, co, q, t, b, l, MAT, 5, flag=flag)
            l0 = ctx.timing()["fill_launches"]
            ctx.lib.ssw_gpu_set_budget(ctx.h, budget)
            s1, r1, c1 = ctx.align_windows_best(Q, T, co, q, t, b, l, MAT, 5, flag=flag)
            tm = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert tm["fill_launches"] > 1 and tm["fill_launches"] > l0 and tm["win_copied"] == 0
            assert (s0 == s1).all() and (r0 == r1).all() and c0.tobytes() == c1.tobytes()
            assert (s0["best"] == planted).all()
        Q.free(); T.free()
    finally:
        ctx.close()


def _rebase(ctx, ngroups, qlen, wmin, wmax, L):
    rng = np.random.default_rng(6800)
    sizes = [int(x) for x in rng.integers(0, 6, size=ngroups)]
    reads, targets, co, q, t, b, l, planted, _ = _groups_case(rng, sizes, L, qlen, wmin, wmax)
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        for kw in (dict(flag=0), dict(flag=15, filterd=32767), dict(flag=0, min_score=10000)):
            s0, rel, c0 = ctx.align_windows_best(Q, T, co, q, t, b, l, MAT, 5, **kw)
            s1, reb, c1 = ctx.align_windows_best(Q, T, co, q, t, b, l, MAT, 5, rebase=True, **kw)
            won = s0["best"] >= 0
            wb = np.zeros(len(sizes), dtype=np.int64); wb[won] = b[co[:-1][won] + s0["best"][won]]
            exp = rel.copy()
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                exp[f] = np.where(rel[f] >= 0, rel[f] + wb, rel[f])
            assert (s0 == s1).all() and (reb == exp).all() and c0.tobytes() == c1.tobytes()
            assert (reb["ref_begin1"][~won] == -1).all()
            if kw.get("flag") == 15:
                assert won.any() and (reb["ref_begin1"][won] >= wb[won]).all()
            if kw.get("min_score"):
                assert not won.any()
    finally:
        Q.free(); T.free()


def _errors(ctx, other_ctx):
    reads = [random_ref(30, 1, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    Q = ctx.upload(reads); T = ctx.upload(targets); Qo = other_ctx.upload(reads)
    ok = dict(cand_off=[0, 2, 3], qidx=[0, 0, 0], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30])

    def refused(what, Qx=Q, **change):
        for flag in (0, 2):
            args = {k: list(v) for k, v in ok.items()}
            for k, (pos, v) in change.items():
                args[k][pos] = v
            sel = np.zeros(2, dtype=ssw_amd.BEST_DTYPE); sel["best"] = 777; sel["pad"] = 0x5a5a
            out = np.zeros(2, dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
            before = sel.tobytes() + out.tobytes()      # (arrays of the caller: every byte, padding included, must stay)
            with pytest.raises(RuntimeError, match=what):
                ctx.align_windows_best(Qx, T, args["cand_off"], args["qidx"], args["tidx"], args["tbeg"], args["tlen"], MAT, 5, flag=flag, out=(sel, out))
            assert sel.tobytes() + out.tobytes() == before
            # the context answers the next call
            s, r, _, _ = _check(ctx, reads, targets, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], MAT, 5, T=T, flag=flag)
            assert int(s["n_eligible"][0]) == 2
    try:
        for field, value, what in [("qidx", 1, "index out of range"), ("qidx", -1, "index out of range"), ("tidx", 2, "index out of range"),
                                   ("tidx", -1, "index out of range"), ("tbeg", -1, "window out of range"), ("tlen", -1, "window out of range"),
                                   ("tlen", 31, "window out of range"), ("tbeg", 41, "window out of range"), ("tbeg", 1 << 40, "window out of range")]:
            refused(what + r".*pair 2\b", **{field: (2, value)})
        refused(r"cand_off\[0\] must be 0.*group 0", cand_off=(0, 1))
        refused(r"cand_off decreases.*group 1\b", cand_off=(1, 4))      # [0, 4, 3]: group 1 runs backwards (and nothing beyond the arrays is read)
        refused("another context", Qx=Qo)
        # NULL arrays, straight through the C ABI
        co = np.array(ok["cand_off"], dtype=np.int64); qi = np.zeros(3, np.int32); tb = np.zeros(3, np.int64)
        sel = np.zeros(2, dtype=ssw_amd.BEST_DTYPE); out = np.zeros(2, dtype=ssw_amd.RESULT_DTYPE)
        m = np.ascontiguousarray(MAT, dtype=np.int8)
        p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, 0, 0, 0, -1, 2, 0)
        full = [co.ctypes.data, 2, qi.ctypes.data, qi.ctypes.data, tb.ctypes.data, qi.ctypes.data, None, 0, sel.ctypes.data, out.ctypes.data]
        import ctypes as C
        for k in (0, 2, 3, 4, 5, 8, 9):
            a = list(full); a[k] = None
            words = C.c_int64(5)
            rc = ctx.lib.ssw_gpu_align_windows_best(ctx.h, Q.h, T.h, a[0], a[1], a[2], a[3], a[4], a[5], C.byref(p), 0, a[8], a[9], None, C.byref(words))
            assert rc == -1 and "NULL argument" in ctx.error() and words.value == 0
        # more than 0x7fffff00 candidates: refused from cand_off alone, before any per-candidate array is read (they hold 3 entries here)
        big = np.array([0, 0x7fffff01], dtype=np.int64)
        sel[:] = 0; sel["best"] = 777; out[:] = 0; out["score1"] = 777
        before = sel.tobytes() + out.tobytes()
        words = C.c_int64(5)
        rc = ctx.lib.ssw_gpu_align_windows_best(ctx.h, Q.h, T.h, big.ctypes.data, 1, qi.ctypes.data, qi.ctypes.data, tb.ctypes.data, qi.ctypes.data, C.byref(p), 0,
                                                sel.ctypes.data, out.ctypes.data, None, C.byref(words))
        assert rc == -1 and "more than 2^31 candidates" in ctx.error() and words.value == 0
        assert sel.tobytes() + out.tobytes() == before
        s, _, _, _ = _check(ctx, reads, targets, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], MAT, 5, T=T, flag=2)
        assert int(s["n_eligible"][0]) == 2
        # no groups; groups without candidates
        e = np.zeros(0, np.int32)
        s, r, c = ctx.align_windows_best(Q, T, [0], e, e, np.zeros(0, np.int64), e, MAT, 5, flag=2)
        assert s.shape == (0,) and r.shape == (0,) and c.shape == (0,)
        s, r, c = ctx.align_windows_best(Q, T, [0, 0, 0], e, e, np.zeros(0, np.int64), e, MAT, 5, flag=2)
        assert (s["best"] == -1).all() and (s["second"] == -1).all() and (r["cigar_off"] == -1).all() and (r["ref_begin1"] == -1).all() and c.shape == (0,)
        with pytest.raises(ValueError):
            ctx.align_windows_best(Q, T, [0, 1], [0], [0, 0], [0], [1], MAT, 5)
        with pytest.raises(ValueError):
            ctx.align_windows_best(Q, T, [0, 2], [0], [0], [0], [1], MAT, 5)
    finally:
        Q.free(); T.free(); Qo.free()


def _cpp_check(lib_dir, lib_name, tmp_path, args):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / ("windows_best_check_" + lib_name))
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "windows_best_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-l" + lib_name, "-lm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- emulator

def test_emu_group_sizes(ectx):
    """groups of 0, 1, 2, 17, 64, 65 candidates and one of 5 000"""
    _group_sizes(ectx, 5000, 24, 30, 44, 4000)


@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_emu_flags_both_strands(ectx, flag):
    _flags(ectx, flag, 14, 40, 60, 140, 1500)


def test_emu_min_score_and_overflow(ectx):
    _min_score(ectx, 10, 130, 160, 260, 2500)


def test_emu_protein_blosum50(ectx):
    _protein(ectx, 8, 50, 1200)


def test_emu_envelope_mix(ectx):
    _envelope_mix(ectx, 0)


def test_emu_whole_call_fallbacks(ectx):
    _whole_call_fallbacks(ectx, 8, 40)


def test_emu_small_budget_chunks(emu_lib_path):
    """1 MiB budget (the floor): fill launches are cut down, the call-long record array is not -- output as under the default budget"""
    _small_budget(emu_lib_path, 1 << 20, 20, 30, 15000, 60000)


def test_emu_rebase(ectx):
    _rebase(ectx, 14, 40, 60, 150, 2000)


def test_emu_errors(ectx, emu_lib_path):
    other = ssw_amd.Context(0, ectx.lib)
    try:
        _errors(ectx, other)
    finally:
        other.close()


def test_cpp_align_windows_best_emulated(emu_lib_path, tmp_path):
    """include/ssw_gpu_cpp.h BatchAligner::AlignWindowsBest against AlignWindows over all candidates (tests/cpp/windows_best_check.cpp)"""
    _cpp_check(os.path.dirname(emu_lib_path), "ssw_emu", tmp_path, ["16", "3"])


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
def test_gpu_group_sizes(gpu_ctx):
    rng = np.random.default_rng(7100)
    _group_sizes(gpu_ctx, 5000, 150, 300, 700, 400000, sizes=SIZES + [int(x) for x in rng.integers(0, 9, size=400)], gpu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 1, 2, 8, 15])
def test_gpu_flags_both_strands(gpu_ctx, flag):
    _flags(gpu_ctx, flag, 600, 150, 300, 700, 300000, gpu=True)


@pytest.mark.gpu
def test_gpu_min_score_and_overflow(gpu_ctx):
    _min_score(gpu_ctx, 300, 150, 300, 700, 200000)


@pytest.mark.gpu
def test_gpu_protein_blosum50(gpu_ctx):
    _protein(gpu_ctx, 300, 200, 50000)


@pytest.mark.gpu
def test_gpu_envelope_mix(gpu_ctx):
    _envelope_mix(gpu_ctx, 70000)


@pytest.mark.gpu
def test_gpu_whole_call_fallbacks(gpu_ctx):
    _whole_call_fallbacks(gpu_ctx, 40, 100)


@pytest.mark.gpu
def test_gpu_budget_16mib(product_lib_path):
    _small_budget(product_lib_path, 16 << 20, 3000, 150, 500, 800000)


@pytest.mark.gpu
def test_gpu_rebase(gpu_ctx):
    _rebase(gpu_ctx, 400, 150, 300, 700, 300000)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx, product_lib_path):
    other = ssw_amd.Context(0, gpu_ctx.lib)
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_at_scale(gpu_ctx):
    """200 000 reads of 150 bp against one resident 100 Mb target, 1..8 candidates per read: the true window, decoys of 300..700 bp
    elsewhere, an occasional duplicate of the true window; flag 0, and flag 2 with CIGARs"""
    rng = np.random.default_rng(7900)
    L, nr = 100000000, 200000
    target = rng.integers(0, 4, size=L, dtype=np.int8)
    sizes = rng.integers(1, 9, size=nr)
    co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nc = int(co[-1])
    tlen = rng.integers(300, 701, size=nc).astype(np.int32)
    tbeg = rng.integers(0, L - 700, size=nc).astype(np.int64)
    planted = (rng.random(nr) * sizes).astype(np.int64)
    own = np.repeat(tbeg[co[:-1] + planted], sizes)          # a decoy that comes near its read's own window moves half a target away
    clash = (np.abs(tbeg - own) < 1400) & (np.arange(nc) != np.repeat(co[:-1] + planted, sizes))
    tbeg[clash] = (own[clash] + L // 2) % (L - 700)
    dup = np.nonzero((sizes >= 2) & (rng.random(nr) < 0.1))[0]
    other = (planted[dup] + 1 + (rng.random(len(dup)) * (sizes[dup] - 1)).astype(np.int64)) % sizes[dup]
    tbeg[co[dup] + other] = tbeg[co[dup] + planted[dup]]; tlen[co[dup] + other] = tlen[co[dup] + planted[dup]]
    first = planted.copy(); first[dup] = np.minimum(planted[dup], other)
    reads = []
    for g in range(nr):
        i = int(co[g] + planted[g]); s, n = int(tbeg[i]), int(tlen[i])
        o = int(rng.integers(0, n - 150))
        reads.append(np.asarray(mutate(target[s + o:s + o + 150], rng, 0.02, 0.005, 0.005, 4), dtype=np.int8))
    qidx = np.repeat(np.arange(nr, dtype=np.int32), sizes)
    tidx = np.zeros(nc, dtype=np.int32)
    Q = gpu_ctx.upload(reads); T = gpu_ctx.upload([target])
    sample = [int(x) for x in np.random.default_rng(5).choice(nr, size=400, replace=False)]
    try:
        for flag in (0, 2):
            sel, res, cig, tm = _check(gpu_ctx, reads, [target], co, qidx, tidx, tbeg, tlen, MAT, 5, sample=sample, T=T, Q=Q, flag=flag, filters=0)
            _assert_fast(tm, gpu=True)
            assert (sel["best"] == first).all()          # a decoy of random sequence never reaches a planted read's score
            assert (sel["second_score1"][dup] == res["score1"][dup]).all()
            if flag:
                assert tm["best_flagged"] == nr and (res["cigarLen"] > 0).all()
    finally:
        Q.free(); T.free()


@pytest.mark.gpu
def test_cpp_align_windows_best_gpu(product_lib_path, tmp_path):
    _cpp_check(os.path.dirname(product_lib_path), "ssw", tmp_path, ["400", "5"])
