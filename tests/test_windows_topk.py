"""ssw_gpu_align_windows_topk: the best k candidate windows of every read (include/ssw_gpu.h).

Groups and candidates are ssw_gpu_align_windows_best's; k ranks per group come back.  Two oracles, no group left out: (a) Context.align_windows
over ALL candidates with the same parameters, then the rule in numpy with a stable sort -- eligible: status 0, score1 > 0, score1 >= min_score;
order: score1 descending, then position ascending; rank r >= 1 only while score1 >= score1(rank 0) - max_drop -- compared with `pos`,
`n_eligible`, every record field (cigar_off included) and the pool bytes; (b) the reference through parity.expected() on the cut-out window of
every reported slot (all of them on the emulator, a fixed-seed sample of 400 on the GPU).  Every case goes through one helper (_check) and runs on
the CPU SIMT emulator (tests/emu: the real host driver and the real kernel source) at the small size and, marked gpu, on the MI355X with the
group counts raised.  The inputs of a case and oracle (a)'s records are computed once per parameter set and shared."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, random_ref

MAT = dna_matrix(2, 2)
KS = [1, 2, 3, 8, 16, 64]
EDGES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200]      # lane, row and wavefront edges of the 16-lane selection


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


def _mut(seq, rng, n_codes, sub):
    """substitutions everywhere, now and then one short insertion or deletion"""
    s = np.array(seq, dtype=np.int8)
    m = rng.random(len(s)) < sub
    s[m] = (s[m] + rng.integers(1, n_codes, size=int(m.sum()))) % n_codes
    u = rng.random()
    if u < 0.3 and len(s) > 20:
        p = int(rng.integers(5, len(s) - 8)); d = int(rng.integers(1, 4))
        s = np.concatenate([s[:p], s[p + d:]]) if u < 0.15 else np.concatenate([s[:p], rng.integers(0, n_codes, size=d, dtype=np.int8), s[p:]])
    return np.ascontiguousarray(s, dtype=np.int8)


class Case(object):
    """one read per group; about half of a group's candidates overlap the read's locus by a random amount (a spread of scores, the full
    window among them), the others lie anywhere (low scores that tie often).  strands: the reads of odd groups are stored reverse-complemented
    and every candidate picks its strand (qidx = count + i is the reverse complement), so that good candidates sit on both strands."""

    def __init__(self, seed, sizes, L, qlen=(60, 150), wlen=(100, 300), n_codes=4, strands=False, sub=0.03):
        rng = np.random.default_rng(seed)
        self.targets = [np.asarray(random_ref(L + 37 * j, int(rng.integers(1 << 30)), n_codes), dtype=np.int8) for j in range(2)]
        nr = len(sizes)
        reads, qidx, tidx, tbeg, tlen = [], [], [], [], []
        for g, sz in enumerate(sizes):
            t = int(rng.integers(2)); ql = int(rng.integers(qlen[0], qlen[1] + 1)); s = int(rng.integers(0, len(self.targets[t]) - ql + 1))
            seq = _mut(self.targets[t][s:s + ql], rng, n_codes, sub)
            rev = strands and g % 2 == 1
            reads.append(_revcomp(seq) if rev else seq)
            for _ in range(sz):
                wl = int(rng.integers(wlen[0], wlen[1] + 1))
                if rng.random() < 0.5:
                    ct = t; wb = int(rng.integers(s - wl + ql // 4, s + ql - ql // 4 + 1))
                else:
                    ct = int(rng.integers(2)); wb = int(rng.integers(0, len(self.targets[ct]) - wl + 1))
                wb = min(max(wb, 0), len(self.targets[ct]) - wl)
                good = not strands or rng.random() < 0.7
                qidx.append(g + nr if strands and (rev == good) else g)
                tidx.append(ct); tbeg.append(wb); tlen.append(wl)
        self.nr = nr
        self.strands = strands
        self.reads = reads + [_revcomp(r) for r in reads] if strands else reads
        self.co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.q = np.array(qidx, dtype=np.int32); self.t = np.array(tidx, dtype=np.int32)
        self.b = np.array(tbeg, dtype=np.int64); self.l = np.array(tlen, dtype=np.int32)
        self.all = {}       # oracle (a): align_windows over all candidates, per context and parameter set

    @classmethod
    def explicit(cls, reads, targets, rows):
        """rows: per group a list of (query, target, tbeg, tlen)"""
        self = cls.__new__(cls)
        self.reads = [np.ascontiguousarray(r, dtype=np.int8) for r in reads]; self.targets = targets; self.nr = len(reads); self.strands = False
        self.co = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
        flat = [x for r in rows for x in r]
        self.q = np.array([x[0] for x in flat], dtype=np.int32); self.t = np.array([x[1] for x in flat], dtype=np.int32)
        self.b = np.array([x[2] for x in flat], dtype=np.int64); self.l = np.array([x[3] for x in flat], dtype=np.int32)
        self.all = {}
        return self

    def upload(self, ctx):
        T = ctx.upload(self.targets)
        if self.strands:
            base = ctx.upload(self.reads[:self.nr]); Q = base.with_revcomp(); base.free()
        else:
            Q = ctx.upload(self.reads)
        return Q, T


@functools.lru_cache(maxsize=None)
def _case(seed, sizes, L, **kw):
    return Case(seed, list(sizes), L, **dict(kw))


def _rule(ares, acig, co, k, min_score, max_drop):
    """the selection rule over align_windows' records of all candidates -> (pos, n_eligible, records, pool) as align_windows_topk must give them"""
    ng = len(co) - 1
    sizes = np.diff(co)
    grp = np.repeat(np.arange(ng), sizes)
    posn = np.arange(int(co[-1])) - np.repeat(co[:-1], sizes)
    sc = ares["score1"].astype(np.int64)
    e = np.nonzero((ares["status"] == 0) & (sc > 0) & (sc >= min_score))[0]
    e = e[np.lexsort((posn[e], -sc[e], grp[e]))]          # stable: group, then score1 descending, then position ascending
    nel = np.bincount(grp[e], minlength=ng).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(nel)])[:-1]
    rank = np.arange(len(e)) - start[grp[e]]
    top = np.zeros(ng, dtype=np.int64); top[grp[e][rank == 0]] = sc[e][rank == 0]
    keep = rank < k
    if max_drop >= 0:
        keep &= sc[e] >= top[grp[e]] - max_drop
    pos = np.full((ng, k), -1, dtype=np.int32)
    res = np.zeros((ng, k), dtype=ssw_amd.RESULT_DTYPE)
    res["ref_begin1"] = -1; res["read_begin1"] = -1; res["cigar_off"] = -1
    pos[grp[e][keep], rank[keep]] = posn[e][keep]
    res[grp[e][keep], rank[keep]] = ares[e][keep]
    flat = res.reshape(-1)
    has = np.nonzero((flat["cigarLen"] > 0) & (flat["cigar_off"] >= 0))[0]
    lens = flat["cigarLen"][has].astype(np.int64); offs = flat["cigar_off"][has].astype(np.int64)
    new = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pool = acig[np.repeat(offs - new, lens) + np.arange(int(lens.sum()))] if len(has) else np.zeros(0, dtype=np.uint32)
    flat["cigar_off"][has] = new
    return pos, nel, res, np.ascontiguousarray(pool, dtype=np.uint32)


def _check(ctx, case, mat, n, k, min_score=0, max_drop=-1, sample=None, **kw):
    """align_windows_topk against oracle (a) for every slot and oracle (b) for every reported slot (sample: that many of them, fixed seed)
    -> (pos, n_eligible, records, pool, timing, align_windows' records of all candidates)"""
    co, q, t, b, l = case.co, case.q, case.t, case.b, case.l
    ng = len(co) - 1
    Q, T = case.upload(ctx)
    try:
        pos, nel, res, cig = ctx.align_windows_topk(Q, T, co, q, t, b, l, mat, n, k, min_score=min_score, max_drop=max_drop, **kw)
        tm = ctx.timing()
        key = (id(ctx), np.asarray(mat).tobytes(), n, tuple(sorted(kw.items())))
        if key not in case.all:
            case.all[key] = ctx.align_windows(Q, T, q, t, b, l, mat, n, **kw)
        ares, acig = case.all[key]
    finally:
        Q.free(); T.free()
    epos, enel, eres, ecig = _rule(ares, acig, co, k, min_score, max_drop)
    bad = []
    for g in np.nonzero((pos != epos).any(axis=1) | (res != eres).any(axis=1) | (nel != enel))[0][:4]:
        bad.append("group %d (candidates [%d, %d)): expected %s %d %s, got %s %d %s" % (g, co[g], co[g + 1], epos[g], enel[g], eres[g], pos[g], nel[g], res[g]))
    assert not bad, "\n".join(bad)
    assert pos.shape == (ng, k) and (pos == epos).all() and (nel == enel).all()
    assert (res == eres).all()                          # every field, cigar_off included
    assert cig.tobytes() == ecig.tobytes()
    hit = pos >= 0
    assert (np.diff(hit.astype(np.int8), axis=1) <= 0).all()      # every slot after the first -1 is -1
    flag = kw.get("flag", 0)
    gate = hit if flag != 2 else hit & (res["score1"] >= kw.get("filters", 0))
    assert tm["best_flagged"] == (int(gate.sum()) if flag else 0) and tm["best_flagged"] <= ng * k
    if not kw.get("mark_mismatch", False):
        slots = np.argwhere(hit)
        if sample is not None and len(slots) > sample:
            slots = slots[np.random.default_rng(5).choice(len(slots), size=sample, replace=False)]
        gapO, gapE, ml = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("maskLen", -1)
        for g, r in slots:
            i = int(co[g]) + int(pos[g, r])
            rd = case.reads[q[i]]
            rf = np.ascontiguousarray(case.targets[int(t[i])][int(b[i]):int(b[i]) + int(l[i])])
            exp, xcig = expected(rd, mat, n, rf, gapO, gapE, flag, kw.get("filters", 0), kw.get("filterd", 0), ml if ml >= 0 else len(rd) // 2,
                                 kw.get("score_size", 2))
            rec = res[g, r]
            ok = exp is not None and int(rec["status"]) == 0 and {f: int(rec[f]) for f in RES_FIELDS} == exp and _cig(rec, cig) == xcig
            if not ok and len(bad) < 4:
                bad.append("group %d rank %d candidate %d (len %d x %d): expected %s %s got %s" % (g, r, i, len(rd), len(rf), exp, cigar_str(xcig), rec))
        assert not bad, "\n".join(bad)
    return pos, nel, res, cig, tm, ares


def _sizes(seed, ngroups, extra=()):
    rng = np.random.default_rng(seed)
    return tuple(list(extra) + [int(x) for x in rng.integers(0, 9, size=ngroups - len(extra))])


# ------------------------------------------------------------------------------------------------------------- the cases

def _boundaries(ctx, k, ngroups, L, sample=None, gpu=False):
    """1. group sizes on the lane, row and wavefront edges, and k - 1, k, k + 1 for every k of the list, in one call"""
    extra = EDGES + [x + d for x in KS for d in (-1, 0, 1)]
    case = _case(8100, _sizes(8101, ngroups, extra), L)
    for kw in (dict(flag=0), dict(flag=2)):
        pos, nel, res, _, tm, _ = _check(ctx, case, MAT, 5, k, sample=sample, **kw)
        assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
        sizes = np.diff(case.co)
        assert (nel == sizes).all()                     # min_score 0, ordinary windows: every candidate is eligible
        assert ((pos >= 0).sum(axis=1) == np.minimum(sizes, k)).all()
        if gpu:
            assert tm["reduce_ms"] > 0                  # the device time of k_grouptopk


def _ties(ctx):
    """2. 40 identical windows, k = 8: positions 0..7; equal scores straddling rank k; an exact copy of the best window at the end of a group of 33"""
    rng = np.random.default_rng(8200)
    tg = np.asarray(random_ref(6000, 8201, 4), dtype=np.int8)
    reads = [tg[1000:1100].copy(), tg[2000:2090].copy(), tg[3000:3120].copy()]
    g0 = [(0, 0, 950, 200)] * 40
    g1 = [(1, 0, 1950, 200)] * 3 + [(1, 0, 2030, 150)] * 6          # 3 full hits, then 6 equal partial ones: k = 5 ends inside the tie
    g2 = [(2, 0, int(x), 250) for x in rng.integers(0, 2500, size=33)]
    g2[5] = (2, 0, 2950, 250); g2[32] = g2[5]
    case = Case.explicit(reads, [tg], [g0, g1, g2])
    for flag in (0, 2):
        pos, nel, res, _, _, _ = _check(ctx, case, MAT, 5, 8, flag=flag)
        assert [int(x) for x in pos[0]] == list(range(8)) and int(nel[0]) == 40 and (res["score1"][0] == 200).all()
        assert [int(x) for x in pos[2, :2]] == [5, 32] and int(res["score1"][2, 0]) == int(res["score1"][2, 1]) == 240
        pos, _, res, _, _, _ = _check(ctx, case, MAT, 5, 5, flag=flag)
        assert [int(x) for x in pos[1]] == [0, 1, 2, 3, 4] and int(res["score1"][1, 2]) == 180 and int(res["score1"][1, 3]) == int(res["score1"][1, 4]) < 180
        pos, _, _, _, _, _ = _check(ctx, case, MAT, 5, 5, max_drop=0, flag=flag)
        assert [int(x) for x in pos[1]] == [0, 1, 2, -1, -1]


def _thresholds(ctx, ngroups, L, sample=None):
    """3. min_score through the middle of the groups; max_drop 0, 1, 10 and none; 8-bit overflow with score_size 0; an empty window; a
    group without an eligible candidate and an empty group"""
    case = _case(8300, _sizes(8301, ngroups, (0, 12, 20)), L, sub=0.0)
    _, nel0, _, _, _, ares = _check(ctx, case, MAT, 5, 8, sample=sample, flag=0)
    ms = int(np.median(ares["score1"]))
    _, nel, _, _, _, _ = _check(ctx, case, MAT, 5, 8, min_score=ms, sample=sample, flag=2)
    assert 0 < int(nel.sum()) < int(nel0.sum()) and ((nel > 0) & (nel < nel0)).any()
    for md in (0, 1, 10, -1):
        pos, nel, res, _, _, _ = _check(ctx, case, MAT, 5, 8, max_drop=md, sample=sample, flag=2, filters=40)
        hit = pos >= 0
        if md == 0:
            assert (res["score1"][hit] == np.broadcast_to(res["score1"][:, :1], res.shape)[hit]).all()      # only ties with the best remain
        if md >= 0:
            assert ((hit.sum(axis=1) < np.minimum(nel, 8)) & (nel > 1)).any()      # the cut did something, n_eligible does not notice
    pos, nel, _, _, _, _ = _check(ctx, case, MAT, 5, 8, min_score=70000, flag=2)
    assert (pos == -1).all() and (nel == 0).all()
    # score_size 0: the full-length hits of reads above 127 residues overflow 8 bits (status 1: the reference returns NULL) and never rank
    tg = np.asarray(random_ref(3000, 8302, 4), dtype=np.int8)
    reads = [tg[500:650].copy(), tg[1500:1560].copy()]
    rows = [[(0, 0, 450, 300), (0, 0, 560, 200), (0, 0, 2000, 300)],      # the overflowing window first, a partial hit, a decoy
            [(1, 0, 1480, 0), (1, 0, 1450, 200), (1, 0, 100, 150)],       # an empty window among ordinary candidates
            [(1, 0, 77, 0)], []]                                          # ... alone (score 0: not eligible), and an empty group
    case = Case.explicit(reads, [tg], rows)
    pos, nel, res, _, _, ares = _check(ctx, case, MAT, 5, 3, flag=0, score_size=0)
    assert int(ares["status"][0]) == 1 and [int(x) for x in pos[0]] == [1, 2, -1] and int(nel[0]) == 2
    for flag in (0, 2):
        pos, nel, res, _, _, _ = _check(ctx, case, MAT, 5, 3, flag=flag)
        assert [int(x) for x in pos[0]] == [0, 1, 2] and [int(x) for x in pos[1]] == [1, 2, -1] and int(nel[1]) == 2
        assert (pos[2:] == -1).all() and (nel[2:] == 0).all() and (res["cigar_off"][2:] == -1).all() and (res["ref_begin1"][2:] == -1).all()
        assert (res["score1"][2:] == 0).all()


def _planner_classes(ctx):
    """4. a 150-residue read (k_fillpairs), an 800-residue read (the strip kernel's pair mode) and a 700-residue read (the fallback) in one
    group, each against a window that holds its source: all three place; then gapO = gapE, where every candidate takes the fallback"""
    tg = np.asarray(random_ref(6000, 8400, 4), dtype=np.int8)
    other = np.asarray(random_ref(2000, 8401, 4), dtype=np.int8)
    reads = [tg[300:450].copy(), tg[1000:1800].copy(), tg[2500:3200].copy(), tg[4000:4100].copy()]
    rows = [[(0, 0, 250, 300), (3, 1, 0, 300), (1, 0, 900, 1000), (2, 0, 2400, 900), (3, 0, 3950, 200)],
            [(2, 1, 0, 900), (0, 0, 280, 200), (1, 1, 100, 1000)],        # the long reads against foreign windows lose to a short read's hit
            [(3, 0, 3900, 300), (3, 0, 3950, 200)]]
    case = Case.explicit(reads, [tg, other], rows)
    for kw in (dict(flag=0), dict(flag=2)):
        pos, nel, res, _, tm, _ = _check(ctx, case, MAT, 5, 3, **kw)
        assert [int(x) for x in pos[0]] == [2, 3, 0] and [int(x) for x in res["score1"][0]] == [1600, 1400, 300]
        assert int(pos[1, 0]) == 1 and tm["win_copied"] > 0
        if kw["flag"]:
            assert (res["cigarLen"][0] > 0).all()
        pos, _, _, _, tm, _ = _check(ctx, case, MAT, 5, 3, gapO=1, gapE=1, **kw)
        assert [int(x) for x in pos[0]] == [2, 3, 0] and not tm["fill_kernel"].startswith("k_fillpairs<")


def _flags(ctx, what, ngroups, L, sample=None):
    """5. flags and post-processing"""
    case = _case(8500, _sizes(8501, ngroups, (0, 9, 17)), L)
    kw = dict(flag0=dict(flag=0), flag1=dict(flag=1), filters=dict(flag=2, filters=120), filterd=dict(flag=15, filterd=60),
              mark=dict(flag=2, mark_mismatch=True))[what]
    pos, _, res, _, _, _ = _check(ctx, case, MAT, 5, 4, sample=sample, **kw)
    hit = pos >= 0
    if what == "filters":      # reported, but below `filters`: no begin position and no CIGAR, exactly as align_windows leaves them
        low = hit & (res["score1"] < 120)
        assert low.any() and (hit & ~low).any() and (res["ref_begin1"][low] == -1).all() and (res["cigarLen"][low] == 0).all()
        assert (res["cigarLen"][hit & ~low] > 0).all()
    if what == "mark":
        assert (res["edit_distance"][hit] >= 0).all() and (res["edit_distance"][hit] > 0).any()


def _rebase(ctx, ngroups, L):
    case = _case(8500, _sizes(8501, ngroups, (0, 9, 17)), L)
    Q, T = case.upload(ctx)
    try:
        for kw in (dict(flag=0), dict(flag=2), dict(flag=0, min_score=70000)):
            p0, n0, rel, c0 = ctx.align_windows_topk(Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5, 3, **kw)
            p1, n1, reb, c1 = ctx.align_windows_topk(Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5, 3, rebase=True, **kw)
            hit = p0 >= 0
            wb = np.zeros(p0.shape, dtype=np.int64); wb[hit] = case.b[(case.co[:-1, None] + p0)[hit]]
            exp = rel.copy()
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                exp[f] = np.where(rel[f] >= 0, rel[f] + wb, rel[f])
            assert (p0 == p1).all() and (n0 == n1).all() and (reb == exp).all() and c0.tobytes() == c1.tobytes()
            assert (reb["ref_begin1"][~hit] == -1).all() and (reb["ref_end1"][~hit] == 0).all()
            if kw["flag"] == 2:
                assert hit.any() and (reb["ref_begin1"][hit] >= wb[hit]).all()
            if kw.get("min_score"):
                assert not hit.any()
    finally:
        Q.free(); T.free()


def _protein(ctx, ngroups, L, sample=None):
    case = _case(8600, _sizes(8601, ngroups, (0, 10)), L, n_codes=20, sub=0.1)
    for extra in (dict(), dict(mark_mismatch=True)):
        _, _, _, _, tm, _ = _check(ctx, case, blosum50(), 24, 3, sample=sample, gapO=10, gapE=2, flag=2, filters=60, **extra)
        assert tm["fill_kernel"].startswith("k_fillpairs<")


def _strands(ctx, ngroups, L, sample=None):
    """6. forward and reverse-complement candidates of a read in one group (ssw_gpu_seqs_with_revcomp)"""
    case = _case(8700, _sizes(8701, ngroups, (0, 12, 5)), L, strands=True)
    for flag in (0, 2):
        pos, _, res, _, _, _ = _check(ctx, case, MAT, 5, 3, sample=sample, flag=flag)
    hit = pos >= 0
    rev = case.q[(case.co[:-1, None] + pos)[hit]] >= case.nr
    good = res["score1"][hit] >= 100
    assert (rev & good).any() and (~rev & good).any()          # well-placed candidates on both strands


def _against_best(ctx, ngroups, L):
    """7. k = 1 and k = 2 against align_windows_best, field for field"""
    case = _case(8800, _sizes(8801, ngroups, (0, 1, 2, 17)), L)
    Q, T = case.upload(ctx)
    a = (Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5)
    try:
        for kw in (dict(flag=0), dict(flag=2), dict(flag=2, min_score=80)):
            sel, bres, bcig = ctx.align_windows_best(*a, **kw)
            pos, nel, res, cig = ctx.align_windows_topk(*a, 1, **kw)
            assert (pos[:, 0] == sel["best"]).all() and (nel == sel["n_eligible"]).all() and (res[:, 0] == bres).all() and cig.tobytes() == bcig.tobytes()
            pos, nel, res, cig = ctx.align_windows_topk(*a, 2, max_drop=-1, **kw)
            assert (pos[:, 0] == sel["best"]).all() and (pos[:, 1] == sel["second"]).all() and (res["score1"][:, 1] == sel["second_score1"]).all()
            assert (nel == sel["n_eligible"]).all() and (sel["second"] >= 0).any()
    finally:
        Q.free(); T.free()


def _errors(ctx, other_ctx):
    """8. refused calls leave the caller's arrays alone and the context usable"""
    reads = [random_ref(30, 1, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    case = Case.explicit(reads, targets, [[(0, 0, 0, 40), (0, 1, 5, 50)], [(0, 0, 10, 30)]])
    Q, T = case.upload(ctx); Qo = other_ctx.upload(reads)
    ok = dict(cand_off=[0, 2, 3], qidx=[0, 0, 0], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30])

    def sentinel(k):
        pos = np.full((2, k), 777, dtype=np.int32); nel = np.full(2, 777, dtype=np.int32)
        out = np.zeros((2, k), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
        return pos, nel, out

    def refused(what, Qx=Q, k=2, **change):
        for flag in (0, 2):
            args = {f: list(v) for f, v in ok.items()}
            for f, (at, v) in change.items():
                args[f][at] = v
            pos, nel, out = sentinel(max(k, 1))
            before = pos.tobytes() + nel.tobytes() + out.tobytes()      # (arrays of the caller: every byte, padding included, must stay)
            words = C.c_int64(5)
            arr = [np.ascontiguousarray(args[f], dtype=d) for f, d in (("cand_off", np.int64), ("qidx", np.int32), ("tidx", np.int32), ("tbeg", np.int64), ("tlen", np.int32))]
            m = np.ascontiguousarray(MAT, dtype=np.int8)
            p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
            rc = ctx.lib.ssw_gpu_align_windows_topk(ctx.h, Qx.h, T.h, arr[0].ctypes.data, 2, arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data,
                                                    arr[4].ctypes.data, C.byref(p), k, 0, -1, pos.ctypes.data, nel.ctypes.data, out.ctypes.data, None, C.byref(words))
            import re
            assert rc == -1 and re.search(what, ctx.error()), ctx.error()
            assert words.value == 0 and pos.tobytes() + nel.tobytes() + out.tobytes() == before
            _, n2, _, _, _, _ = _check(ctx, case, MAT, 5, 2, flag=flag)      # the context answers the next call
            assert int(n2[0]) == 2
    try:
        refused(r"k must be 1 \.\. 64.*k = 0", k=0)
        refused(r"k must be 1 \.\. 64.*k = 65", k=65)
        refused(r"cand_off\[0\] must be 0.*group 0", cand_off=(0, 1))
        refused(r"cand_off decreases.*group 1\b", cand_off=(1, 4))      # [0, 4, 3]: group 1 runs backwards (and nothing beyond the arrays is read)
        refused(r"align_windows_topk: window out of range.*pair 2\b", tlen=(2, 31))
        refused(r"align_windows_topk: index out of range.*pair 1\b", tidx=(1, 2))
        refused("another context", Qx=Qo)
        with pytest.raises(RuntimeError, match="k must be"):
            ctx.align_windows_topk(Q, T, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], MAT, 5, 0)
        # NULL arrays, straight through the C ABI: pos (13), and every other one
        co = np.array(ok["cand_off"], dtype=np.int64); qi = np.zeros(3, np.int32); tb = np.zeros(3, np.int64)
        m = np.ascontiguousarray(MAT, dtype=np.int8)
        p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, 0, 0, 0, -1, 2, 0)
        pos, nel, out = sentinel(2)
        before = pos.tobytes() + nel.tobytes() + out.tobytes()
        full = [ctx.h, Q.h, T.h, co.ctypes.data, 2, qi.ctypes.data, qi.ctypes.data, tb.ctypes.data, qi.ctypes.data, C.byref(p), 2, 0, -1,
                pos.ctypes.data, nel.ctypes.data, out.ctypes.data, None]
        for at in (13, 3, 5, 6, 7, 8, 14, 15):
            a = list(full); a[at] = None
            words = C.c_int64(5)
            rc = ctx.lib.ssw_gpu_align_windows_topk(*a, C.byref(words))
            assert rc == -1 and "NULL argument" in ctx.error() and words.value == 0
            assert pos.tobytes() + nel.tobytes() + out.tobytes() == before
        # too many candidates / output slots: refused from cand_off and k alone, before any per-candidate array is read
        big = np.array([0, 0x7fffff01], dtype=np.int64)
        a = list(full); a[3] = big.ctypes.data; a[4] = 1
        words = C.c_int64(5)
        assert ctx.lib.ssw_gpu_align_windows_topk(*a, C.byref(words)) == -1 and "more than 2^31 candidates" in ctx.error() and words.value == 0
        a = list(full); a[4] = 0x7fffff00 // 2 + 1
        assert ctx.lib.ssw_gpu_align_windows_topk(*a, C.byref(words)) == -1 and "more than 2^31 output slots" in ctx.error()
        assert pos.tobytes() + nel.tobytes() + out.tobytes() == before
        # no groups; groups without candidates
        e = np.zeros(0, np.int32)
        ps, ne, r, c = ctx.align_windows_topk(Q, T, [0], e, e, np.zeros(0, np.int64), e, MAT, 5, 3, flag=2)
        assert ps.shape == (0, 3) and ne.shape == (0,) and r.shape == (0, 3) and c.shape == (0,)
        ps, ne, r, c = ctx.align_windows_topk(Q, T, [0, 0, 0], e, e, np.zeros(0, np.int64), e, MAT, 5, 3, flag=2)
        assert (ps == -1).all() and (ne == 0).all() and (r["cigar_off"] == -1).all() and (r["ref_begin1"] == -1).all() and c.shape == (0,)
        with pytest.raises(ValueError):
            ctx.align_windows_topk(Q, T, [0, 2], [0], [0], [0], [1], MAT, 5, 2)
    finally:
        Q.free(); T.free(); Qo.free()


def _small_budget(lib_path, ngroups, L):
    """9. a budget of 1 MiB: the fill runs as several launches, the call-long record array and the output stay whole"""
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        case = _case(8900, _sizes(8901, ngroups, (0, 40, 33)), L, qlen=(64, 64), wlen=(280, 300))
        Q, T = case.upload(ctx)
        a = (Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5, 3)
        for flag in (0, 2):
            p0, n0, r0, c0 = ctx.align_windows_topk(*a, flag=flag)
            l0 = ctx.timing()["fill_launches"]
            ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
            p1, n1, r1, c1 = ctx.align_windows_topk(*a, flag=flag)
            tm = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert tm["fill_launches"] > 1 and tm["fill_launches"] > l0 and tm["win_copied"] == 0
            assert (p0 == p1).all() and (n0 == n1).all() and (r0 == r1).all() and c0.tobytes() == c1.tobytes()
            assert (p0[:, 0] >= 0).sum() == (np.diff(case.co) > 0).sum()
        Q.free(); T.free()
    finally:
        ctx.close()


def _cpp_check(lib_dir, lib_name, tmp_path, args):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / ("windows_topk_check_" + lib_name))
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "windows_topk_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-l" + lib_name, "-lm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- emulator

E_NG, E_L = 44, 3000          # (the boundary case brings its 31 edge groups; the others a few dozen small ones)


@pytest.mark.parametrize("k", KS)
def test_emu_group_size_boundaries(ectx, k):
    _boundaries(ectx, k, E_NG, E_L)


def test_emu_ties(ectx):
    _ties(ectx)


def test_emu_thresholds_and_ineligible(ectx):
    _thresholds(ectx, 24, E_L)


def test_emu_three_planner_classes(ectx):
    _planner_classes(ectx)


@pytest.mark.parametrize("what", ["flag0", "flag1", "filters", "filterd", "mark"])
def test_emu_flags(ectx, what):
    _flags(ectx, what, 24, E_L)


def test_emu_rebase(ectx):
    _rebase(ectx, 24, E_L)


def test_emu_protein_blosum50(ectx):
    _protein(ectx, 16, 2000)


def test_emu_both_strands(ectx):
    _strands(ectx, 24, E_L)


def test_emu_against_align_windows_best(ectx):
    _against_best(ectx, 30, E_L)


def test_emu_errors(ectx):
    other = ssw_amd.Context(0, ectx.lib)
    try:
        _errors(ectx, other)
    finally:
        other.close()


def test_emu_small_budget(emu_lib_path):
    _small_budget(emu_lib_path, 150, 20000)


def test_cpp_align_windows_topk_emulated(emu_lib_path, tmp_path):
    """include/ssw_gpu_cpp.h BatchAligner::AlignWindowsTopK against AlignWindows over all candidates (tests/cpp/windows_topk_check.cpp)"""
    _cpp_check(os.path.dirname(emu_lib_path), "ssw_emu", tmp_path, ["16", "3"])


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NG, G_L = 20000, 400000


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_gpu_group_size_boundaries(gpu_ctx, k):
    _boundaries(gpu_ctx, k, G_NG, G_L, sample=400, gpu=True)


@pytest.mark.gpu
def test_gpu_ties(gpu_ctx):
    _ties(gpu_ctx)


@pytest.mark.gpu
def test_gpu_thresholds_and_ineligible(gpu_ctx):
    _thresholds(gpu_ctx, G_NG, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_three_planner_classes(gpu_ctx):
    _planner_classes(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["flag0", "flag1", "filters", "filterd", "mark"])
def test_gpu_flags(gpu_ctx, what):
    _flags(gpu_ctx, what, G_NG, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_rebase(gpu_ctx):
    _rebase(gpu_ctx, G_NG, G_L)


@pytest.mark.gpu
def test_gpu_protein_blosum50(gpu_ctx):
    _protein(gpu_ctx, G_NG, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_both_strands(gpu_ctx):
    _strands(gpu_ctx, G_NG, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_against_align_windows_best(gpu_ctx):
    _against_best(gpu_ctx, G_NG, G_L)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    other = ssw_amd.Context(0, gpu_ctx.lib)
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_small_budget(product_lib_path):
    _small_budget(product_lib_path, G_NG, G_L)


@pytest.mark.gpu
def test_gpu_resident_target_at_size(gpu_ctx):
    """10. 20 000 groups x 6 candidates of 150-bp reads on windows of 300..400 columns of a resident 2 Mb target, k = 3, flags 0 and 2"""
    rng = np.random.default_rng(9000)
    L, ng, per = 2000000, 20000, 6
    target = rng.integers(0, 4, size=L, dtype=np.int8)
    nc = ng * per
    tlen = rng.integers(300, 401, size=nc).astype(np.int32)
    tbeg = rng.integers(0, L - 400, size=nc).astype(np.int64)
    home = tbeg[::per] + 100                                   # the read of group g lies in its candidate 0; 1 and 2 overlap it in part
    tbeg[1::per] = np.clip(home - 250, 0, L - 400); tbeg[2::per] = np.clip(home + 75, 0, L - 400)
    reads = []
    for g in range(ng):
        r = target[home[g]:home[g] + 150].copy()
        m = rng.random(150) < 0.02
        r[m] = (r[m] + 1) % 4
        reads.append(r)
    case = Case.explicit(reads, [target], [])
    case.co = (np.arange(ng + 1) * per).astype(np.int64)
    case.q = np.repeat(np.arange(ng, dtype=np.int32), per); case.t = np.zeros(nc, dtype=np.int32); case.b = tbeg; case.l = tlen
    for flag in (0, 2):
        pos, nel, res, _, tm, _ = _check(gpu_ctx, case, MAT, 5, 3, sample=400, flag=flag)
        assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0 and tm["reduce_ms"] > 0
        assert tm["best_flagged"] == (int((pos >= 0).sum()) if flag else 0)
        assert (pos[:, 0] == 0).all() and (nel == per).all() and (pos >= 0).all()
        if flag:
            assert (res["cigarLen"] > 0).all()


@pytest.mark.gpu
def test_cpp_align_windows_topk_gpu(product_lib_path, tmp_path):
    _cpp_check(os.path.dirname(product_lib_path), "ssw", tmp_path, ["400", "5"])
