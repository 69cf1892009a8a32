"""ssw_gpu_align_windows_mates: the best candidate pair of every read pair (include/ssw_gpu.h).

A fragment is two groups of candidates (group 2 f: mate 1, group 2 f + 1: mate 2); the call picks one candidate of each so that the pair
score S = score1(a) + score1(b) - (proper ? 0 : unpaired_penalty) is largest, ties to the lower (pos1, pos2).  Two oracles, no fragment
left out: (a) Context.align_windows over ALL candidates -- at flag 0 for the selection, at the caller's flag for the records -- and then the
rule of the header restated in plain Python (a double loop per fragment, Python integers) -- compared with every field of `sel`, every
record field (cigar_off included) and the pool bytes; (b) the reference through parity.expected() on the cut-out window of every chosen
candidate (all of them on the emulator, a fixed-seed sample of 400 on the GPU).  Every case goes through one helper (_check) and runs on the
CPU SIMT emulator (tests/emu: the real host driver and the real kernel source) at the small size and, marked gpu, on the MI355X with the
fragment counts raised.  A case's inputs and oracle (a)'s records are computed once per parameter set and shared.

Shapes: reads of 40..100 residues, windows of 80..250 columns, two targets of about 3 000 columns -- the selection sees only scores, end
columns, lengths, targets and strands, so nothing larger can make it go wrong; the group sizes and fragment counts are what matter."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, dna_matrix, random_ref

MAT = dna_matrix(2, 2)
N1S = [0, 1, 2, 3, 15, 16, 17, 33]      # n1 x n2 crosses 16, 32, 256 combinations and 48 candidates (the kernel's LDS digest size)
N2S = [0, 1, 2, 16, 17, 40]
GRID = tuple((a, b) for a in N1S for b in N2S)
NFRAGS = [1, 3, 4, 5, 15, 16, 17, 33]   # row, wavefront and workgroup edges of one 16-lane row per fragment
INS = (100, 500)
GROUP_MAX = 4096                        # SSW_GPU_MATES_GROUP_MAX (include/ssw_gpu.h)


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


def _mut(seq, rng, sub):
    s = np.array(seq, dtype=np.int8)
    m = rng.random(len(s)) < sub
    s[m] = (s[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
    return np.ascontiguousarray(s, dtype=np.int8)


class Case(object):
    """reads 2 f and 2 f + 1 are the mates of fragment f, stored as a sequencer gives them: an FR fragment of 150..400 columns somewhere on
    one of two targets, one mate the forward copy of its left end, the other the reverse complement of its right end (which of the two is
    mate 1 is random).  The reads are uploaded with their reverse complements (nfwd = number of reads): candidate query r is the read,
    nfwd + r its reverse complement.  About half of a group's candidates overlap the mate's locus by a random amount, the others lie
    anywhere; three in four are on the strand on which the read matches."""

    def __init__(self, seed, sizes, L, qlen=(40, 100), wlen=(80, 250), sub=0.03):
        rng = np.random.default_rng(seed)
        self.targets = [np.asarray(random_ref(L + 37 * j, int(rng.integers(1 << 30)), 4), dtype=np.int8) for j in range(2)]
        nr = 2 * len(sizes)
        reads, rows = [], []
        for f, (n1, n2) in enumerate(sizes):
            t = int(rng.integers(2)); ins = int(rng.integers(150, 401)); s = int(rng.integers(0, len(self.targets[t]) - ins + 1))
            l1, l2 = (int(x) for x in rng.integers(qlen[0], qlen[1] + 1, size=2))
            left = (_mut(self.targets[t][s:s + l1], rng, sub), s, False)                                   # (read, locus, matches as reverse complement)
            right = (_revcomp(_mut(self.targets[t][s + ins - l2:s + ins], rng, sub)), s + ins - l2, True)
            mates = (left, right) if rng.random() < 0.5 else (right, left)
            for h, sz in enumerate((n1, n2)):
                rd, home, rev = mates[h]
                reads.append(rd)
                row = []
                for _ in range(sz):
                    wl = int(rng.integers(wlen[0], wlen[1] + 1)); ql = len(rd)
                    if rng.random() < 0.5:
                        ct = t; wb = int(rng.integers(home - wl + ql // 4, home + ql - ql // 4 + 1))
                    else:
                        ct = int(rng.integers(2)); wb = int(rng.integers(0, len(self.targets[ct]) - wl + 1))
                    wb = min(max(wb, 0), len(self.targets[ct]) - wl)
                    use_rev = rev if rng.random() < 0.75 else not rev
                    row.append((2 * f + h + (nr if use_rev else 0), ct, wb, wl))
                rows.append(row)
        self._finish(reads, rows)

    def _finish(self, reads, rows):
        self.fwd = [np.ascontiguousarray(r, dtype=np.int8) for r in reads]
        self.nfwd = len(self.fwd)
        self.reads = self.fwd + [_revcomp(r) for r in self.fwd]
        self.co = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
        flat = [x for r in rows for x in r]
        self.q = np.array([x[0] for x in flat], dtype=np.int32); self.t = np.array([x[1] for x in flat], dtype=np.int32)
        self.b = np.array([x[2] for x in flat], dtype=np.int64); self.l = np.array([x[3] for x in flat], dtype=np.int32)
        self.all = {}       # oracle (a): align_windows over all candidates, per context and parameter set

    @classmethod
    def explicit(cls, reads, targets, rows):
        """rows: per group (two per fragment) a list of (query, target, tbeg, tlen); query r < len(reads): the read, len(reads) + r: its
        reverse complement"""
        self = cls.__new__(cls)
        self.targets = [np.ascontiguousarray(t, dtype=np.int8) for t in targets]
        assert len(rows) % 2 == 0
        self._finish(reads, rows)
        return self

    def upload(self, ctx):
        T = ctx.upload(self.targets)
        base = ctx.upload(self.fwd); Q = base.with_revcomp(); base.free()
        return Q, T


@functools.lru_cache(maxsize=None)
def _case(seed, sizes, L, **kw):
    return Case(seed, list(sizes), L, **dict(kw))


def _sizes(seed, nfrag, extra=()):
    rng = np.random.default_rng(seed)
    return tuple(list(extra) + [(int(a), int(b)) for a, b in rng.integers(0, 6, size=(nfrag - len(extra), 2))])


def _rule(a0, af, acig, case, min_score, mn, mx, pen):
    """the header's rule over align_windows' records of all candidates (a0: flag 0, af: the caller's flag) -> (sel, records, pool)"""
    co = [int(x) for x in case.co]
    nf = (len(co) - 1) // 2
    s = [int(x) for x in a0["score1"]]
    ok = [int(st) == 0 and sc > 0 and sc >= min_score for st, sc in zip(a0["status"], s)]
    minus = [int(x) >= case.nfwd for x in case.q]
    ln = [len(case.reads[int(x)]) for x in case.q]
    E = [int(case.b[i]) + int(a0["ref_end1"][i]) for i in range(co[-1])]
    B = [E[i] - ln[i] + 1 for i in range(co[-1])]

    def proper(a, b):
        if int(case.t[a]) != int(case.t[b]) or minus[a] == minus[b]:
            return False
        p, m = (b, a) if minus[a] else (a, b)
        return mn <= E[m] - B[p] + 1 <= mx

    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE)
    res = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE)
    res["ref_begin1"] = -1; res["read_begin1"] = -1; res["cigar_off"] = -1
    for f in range(nf):
        c0, c1, c2 = co[2 * f], co[2 * f + 1], co[2 * f + 2]
        e1 = [i for i in range(c0, c1) if ok[i]]; e2 = [i for i in range(c1, c2) if ok[i]]
        pos1 = pos2 = -1; score = second = npr = pr = 0
        if e1 and e2:
            comb = []
            for a in e1:
                for b in e2:
                    p = proper(a, b)
                    npr += p
                    comb.append((-(s[a] + s[b] - (0 if p else pen)), a - c0, b - c1, p))
            comb.sort()
            pos1, pos2, score, pr = comb[0][1], comb[0][2], -comb[0][0], int(comb[0][3])
            second = -comb[1][0] if len(comb) > 1 else 0
        elif e1 or e2:
            e, base = (e1, c0) if e1 else (e2, c1)
            order = sorted(e, key=lambda i: (-s[i], i))
            score = s[order[0]]; second = s[order[1]] if len(order) > 1 else 0
            if e1:
                pos1 = order[0] - base
            else:
                pos2 = order[0] - base
        sel[f] = (pos1, pos2, len(e1), len(e2), score, second, npr, pr, 0)
        if pos1 >= 0:
            res[f, 0] = af[c0 + pos1]
        if pos2 >= 0:
            res[f, 1] = af[c1 + pos2]
    flat = res.reshape(-1)
    has = np.nonzero((flat["cigarLen"] > 0) & (flat["cigar_off"] >= 0))[0]
    lens = flat["cigarLen"][has].astype(np.int64); offs = flat["cigar_off"][has].astype(np.int64)
    new = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pool = acig[np.repeat(offs - new, lens) + np.arange(int(lens.sum()))] if len(has) else np.zeros(0, dtype=np.uint32)
    flat["cigar_off"][has] = new
    return sel, res, np.ascontiguousarray(pool, dtype=np.uint32)


def _all(ctx, case, Q, T, mat, n, **kw):
    key = (id(ctx), np.asarray(mat).tobytes(), n, tuple(sorted(kw.items())))
    if key not in case.all:
        case.all[key] = ctx.align_windows(Q, T, case.q, case.t, case.b, case.l, mat, n, **kw)
    return case.all[key]


def _check(ctx, case, mn, mx, pen, min_score=0, sample=None, mat=MAT, n=5, **kw):
    """align_windows_mates against oracle (a) for every fragment and oracle (b) for every chosen candidate (sample: that many, fixed seed)
    -> (sel, records, pool, timing, align_windows' flag-0 records of all candidates)"""
    co = case.co
    nf = (len(co) - 1) // 2
    Q, T = case.upload(ctx)
    try:
        sel, res, cig = ctx.align_windows_mates(Q, T, co, case.q, case.t, case.b, case.l, case.nfwd, mat, n, mn, mx, pen, min_score=min_score, **kw)
        tm = ctx.timing()
        kw0 = {k: v for k, v in kw.items() if k not in ("flag", "filters", "filterd", "mark_mismatch")}
        a0, _ = _all(ctx, case, Q, T, mat, n, flag=0, **kw0)
        af, acig = _all(ctx, case, Q, T, mat, n, **kw) if kw.get("flag", 0) or kw.get("mark_mismatch") else (a0, np.zeros(0, dtype=np.uint32))
    finally:
        Q.free(); T.free()
    esel, eres, ecig = _rule(a0, af, acig, case, min_score, mn, mx, pen)
    bad = []
    for f in np.nonzero((sel != esel) | (res != eres).any(axis=1))[0][:4]:
        bad.append("fragment %d (candidates [%d, %d) + [%d, %d)): expected %s %s, got %s %s" % (f, co[2 * f], co[2 * f + 1], co[2 * f + 1], co[2 * f + 2],
                                                                                                 esel[f], eres[f], sel[f], res[f]))
    assert not bad, "\n".join(bad)
    assert sel.shape == (nf,) and res.shape == (nf, 2)
    assert sel.tobytes() == esel.tobytes()              # every field, the padding included
    assert (res == eres).all()                          # every field, cigar_off included
    assert cig.tobytes() == ecig.tobytes()
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    hit = pos >= 0
    flag = kw.get("flag", 0)
    assert tm["best_flagged"] == (int(hit.sum()) if flag else 0) and tm["best_flagged"] <= 2 * nf      # the winners handed on
    if not kw.get("mark_mismatch", False):
        slots = np.argwhere(hit)
        if sample is not None and len(slots) > sample:
            slots = slots[np.random.default_rng(5).choice(len(slots), size=sample, replace=False)]
        gapO, gapE, ml = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("maskLen", -1)
        for f, h in slots:
            i = int(co[2 * f + h]) + int(pos[f, h])
            rd = case.reads[case.q[i]]
            rf = np.ascontiguousarray(case.targets[int(case.t[i])][int(case.b[i]):int(case.b[i]) + int(case.l[i])])
            exp, xcig = expected(rd, mat, n, rf, gapO, gapE, flag, kw.get("filters", 0), kw.get("filterd", 0), ml if ml >= 0 else len(rd) // 2,
                                 kw.get("score_size", 2))
            rec = res[f, h]
            ok = exp is not None and int(rec["status"]) == 0 and {x: int(rec[x]) for x in RES_FIELDS} == exp and _cig(rec, cig) == xcig
            if not ok and len(bad) < 4:
                bad.append("fragment %d mate %d candidate %d (len %d x %d): expected %s %s got %s" % (f, h + 1, i, len(rd), len(rf), exp, cigar_str(xcig), rec))
        assert not bad, "\n".join(bad)
    return sel, res, cig, tm, a0


def _against_best(ctx, case, sel0, **kw):
    """unpaired_penalty 0: pos1 / pos2 are align_windows_best's `best` of groups 2 f and 2 f + 1"""
    Q, T = case.upload(ctx)
    try:
        b, _, _ = ctx.align_windows_best(Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5, **kw)
    finally:
        Q.free(); T.free()
    assert (sel0["pos1"] == b["best"][0::2]).all() and (sel0["pos2"] == b["best"][1::2]).all()
    assert (sel0["n_eligible1"] == b["n_eligible"][0::2]).all() and (sel0["n_eligible2"] == b["n_eligible"][1::2]).all()


# ------------------------------------------------------------------------------------------------------------- the cases

def _grid(ctx, nfrag, L, sample=None, gpu=False):
    """1a. every (n1, n2) of the grid in one call, then random small fragments up to nfrag"""
    case = _case(9100, _sizes(9101, max(nfrag, len(GRID)), GRID), L)
    for kw in (dict(flag=0), dict(flag=2)):
        sel, _, _, tm, _ = _check(ctx, case, INS[0], INS[1], 30, sample=sample, **kw)
        assert tm["fill_kernel"].startswith("k_fillpairs<") and tm["win_copied"] == 0
        sizes = np.diff(case.co)
        assert (sel["n_eligible1"] == sizes[0::2]).all() and (sel["n_eligible2"] == sizes[1::2]).all()      # min_score 0, ordinary windows
        assert (sel["proper"] == 1).any() and ((sel["proper"] == 0) & (sel["pos1"] >= 0) & (sel["pos2"] >= 0)).any()
        assert (sel["n_proper"] > 1).any() and ((sel["pos1"] < 0) != (sel["pos2"] < 0)).any()
        if gpu:
            assert tm["reduce_ms"] > 0                  # the device time of k_matebest
    sel0, _, _, _, _ = _check(ctx, case, INS[0], INS[1], 0, sample=sample, flag=0)
    _against_best(ctx, case, sel0)
    # min_score through the middle: fragments lose one mate or both
    sel, _, _, _, a0 = _check(ctx, case, INS[0], INS[1], 30, min_score=60, sample=sample, flag=2)
    assert 0 < int(sel["n_eligible1"].sum()) < int(sel0["n_eligible1"].sum())
    _against_best(ctx, case, _check(ctx, case, INS[0], INS[1], 0, min_score=60, sample=sample, flag=0)[0], min_score=60)


def _counts(ctx, nfrag):
    """1b. fragment counts on the row, wavefront and workgroup edges"""
    case = _case(9150, _sizes(9151 + nfrag, nfrag, ((2, 3),)), 3000)
    sel, _, _, _, _ = _check(ctx, case, INS[0], INS[1], 30, flag=2)
    assert sel.shape == (nfrag,)


def _locus_case():
    """exact-copy mates of known loci, so that E and B are known.  Plus mate P = tg[1000:1060] in window [980, 1080): E = 1059, B = 1000;
    minus mate M = revcomp(tg[1300:1350]) in window [1280, 1380): E = 1349 -- ins = 350."""
    tg = np.asarray(random_ref(3000, 9200, 4), dtype=np.int8)
    t1 = np.asarray(random_ref(3000, 9201, 4), dtype=np.int8)
    t1[1300:1350] = tg[1300:1350]                                         # M's locus once more, on the other target
    rng = np.random.default_rng(9202)
    over = np.concatenate([rng.integers(0, 4, size=10, dtype=np.int8), tg[0:50]])      # hangs 10 residues over column 0: E = 49, B = -10
    P, M, Mf = tg[1000:1060].copy(), _revcomp(tg[1300:1350]), tg[1300:1350].copy()
    M2 = _revcomp(tg[200:250])
    reads = [P, M, P, M, P, Mf, M, P, over, M2]
    nr = len(reads)
    rows = [[(0, 0, 980, 100)], [(nr + 1, 0, 1280, 100)],                 # 0: the FR pair, ins = 350
            [(2, 0, 980, 100)], [(nr + 3, 1, 1280, 100)],                 # 1: the mates on different targets
            [(4, 0, 980, 100)], [(5, 0, 1280, 100)],                      # 2: both on the plus strand
            [(nr + 6, 0, 1280, 100)], [(7, 0, 980, 100)],                 # 3: mate 1 minus, mate 2 plus: the same FR pair, ins = 350
            [(8, 0, 0, 100)], [(nr + 9, 0, 180, 100)]]                    # 4: B = -10, E(m) = 249: ins = 260 (a clamped B would give 250)
    return Case.explicit(reads, [tg, t1], rows)


def _insert_edges(ctx):
    """2. ins = min_insert - 1, min_insert, max_insert, max_insert + 1; other target; same strand; minus mate upstream; B < 0"""
    case = _locus_case()
    pen = 17
    for (mn, mx), want in (((351, 500), [0, 0, 0, 0, 0]), ((350, 500), [1, 0, 0, 1, 0]), ((100, 350), [1, 0, 0, 1, 1]), ((100, 349), [0, 0, 0, 0, 1]),
                           ((260, 260), [0, 0, 0, 0, 1]), ((250, 259), [0, 0, 0, 0, 0]), ((0, 1 << 30), [1, 0, 0, 1, 1])):
        sel, _, _, _, a0 = _check(ctx, case, mn, mx, pen, flag=2)
        assert [int(x) for x in a0["ref_end1"]] == [79, 69, 79, 69, 79, 69, 69, 79, 49, 69] and int(a0["score1"][8]) == 100
        assert [int(x) for x in sel["proper"]] == want and [int(x) for x in sel["n_proper"]] == want
        full = np.array([220, 220, 220, 220, 200])
        assert (sel["score"] == full - pen * (1 - np.array(want))).all() and (sel["second_score"] == 0).all()
    # the minus mate UPSTREAM of the plus mate: ins = E(m) - B(p) + 1 = 1059 - 1300 + 1 < 0, improper whatever the bounds
    tg = case.targets[0]
    up = Case.explicit([_revcomp(tg[1000:1060]), tg[1300:1350].copy()], [tg], [[(2 + 0, 0, 980, 100)], [(1, 0, 1280, 100)]])
    for mn, mx in ((0, 1 << 30), (0, 0)):
        sel, _, _, _, _ = _check(ctx, up, mn, mx, pen, flag=0)
        assert int(sel["proper"][0]) == 0 and int(sel["n_proper"][0]) == 0 and int(sel["score"][0]) == 220 - pen


def _penalty_case():
    """mate 1 is a repeat: its exact copy at 500 (far from mate 2: improper) and a copy with three substitutions at 2000 (proper with
    mate 2 at 2200).  Fragment 0 lists the exact copy first, fragment 1 the degraded one."""
    tg = np.asarray(random_ref(3000, 9300, 4), dtype=np.int8)
    R1 = tg[500:580].copy()
    deg = R1.copy()
    for p in (20, 40, 60):
        deg[p] = (deg[p] + 1) % 4
    tg[2000:2080] = deg
    M = _revcomp(tg[2200:2260])
    reads = [R1, M, R1, M]
    rows = [[(0, 0, 480, 120), (0, 0, 1980, 120)], [(4 + 1, 0, 2180, 100)],
            [(2, 0, 1980, 120), (2, 0, 480, 120)], [(4 + 3, 0, 2180, 100)]]
    return Case.explicit(reads, [tg], rows)


def _penalty_switch(ctx):
    """3. unpaired_penalty 0, d - 1, d, d + 1: the winner flips exactly where the order says, the tie at d goes to the lower (pos1, pos2)"""
    case = _penalty_case()
    sel, _, _, _, a0 = _check(ctx, case, INS[0], INS[1], 0, flag=2)
    d = int(a0["score1"][0]) - int(a0["score1"][1])
    assert d == 12 and [int(x) for x in a0["score1"]] == [160, 148, 120, 148, 160, 120]      # three interior substitutions: 3 x (2 + 2)
    _against_best(ctx, case, sel)
    assert [int(x) for x in sel["pos1"]] == [0, 1] and [int(x) for x in sel["proper"]] == [0, 0] and (sel["n_proper"] == 1).all()
    for pen, p1, pr in ((d - 1, [0, 1], [0, 0]), (d, [0, 0], [0, 1]), (d + 1, [1, 0], [1, 1])):
        sel, _, _, _, _ = _check(ctx, case, INS[0], INS[1], pen, flag=2)
        assert [int(x) for x in sel["pos1"]] == p1 and [int(x) for x in sel["proper"]] == pr and (sel["pos2"] == 0).all()
        best = max(280 - pen, 280 - d)
        assert (sel["score"] == best).all() and (sel["second_score"] == min(280 - pen, 280 - d)).all()


def _ties(ctx):
    """4. identical windows repeated in both groups: n_proper and second_score hold equal-S combinations"""
    case0 = _locus_case()
    tg = case0.targets[0]
    P, M = tg[1000:1060].copy(), _revcomp(tg[1300:1350])
    rows = [[(0, 0, 980, 100)] * 5, [(6 + 1, 0, 1280, 100)] * 4,                                         # 20 equal proper combinations
            [(2, 0, 980, 100), (2, 0, 980, 100)], [(3, 0, 1280, 100), (6 + 3, 0, 1280, 100), (6 + 3, 0, 1280, 100)],
            [(4, 0, 980, 100)], [(6 + 5, 1, 1280, 100), (6 + 5, 0, 1280, 100)]]                          # the same hit on the other target first
    case = Case.explicit([P, M, P, M, P, M], case0.targets, rows)
    for flag in (0, 2):
        sel, _, _, _, _ = _check(ctx, case, 100, 500, 25, flag=flag)
        assert (int(sel["pos1"][0]), int(sel["pos2"][0]), int(sel["n_proper"][0]), int(sel["score"][0]), int(sel["second_score"][0])) == (0, 0, 20, 220, 220)
        assert (int(sel["pos1"][1]), int(sel["pos2"][1]), int(sel["n_proper"][1]), int(sel["proper"][1])) == (0, 1, 4, 1)
        assert int(sel["score"][1]) == int(sel["second_score"][1]) == 220
        assert (int(sel["pos2"][2]), int(sel["proper"][2]), int(sel["score"][2]), int(sel["second_score"][2])) == (1, 1, 220, 195)
        # penalty 0: a proper and an improper combination of equal S tie-break by position only
        sel, _, _, _, _ = _check(ctx, case, 100, 500, 0, flag=flag)
        assert (int(sel["pos1"][2]), int(sel["pos2"][2]), int(sel["proper"][2]), int(sel["n_proper"][2])) == (0, 0, 0, 1)
        assert int(sel["score"][2]) == int(sel["second_score"][2]) == 220


def _flags(ctx, what, nfrag, L, sample=None):
    """5. flags and post-processing; best_flagged equals the winners handed on (asserted in _check)"""
    case = _case(9500, _sizes(9501, nfrag, ((0, 3), (4, 0), (17, 9))), L)
    kw = dict(flag0=dict(flag=0), flag1=dict(flag=1), flag2=dict(flag=2), filters=dict(flag=2, filters=120), mark=dict(flag=2, mark_mismatch=True))[what]
    sel, res, _, _, _ = _check(ctx, case, INS[0], INS[1], 30, sample=sample, **kw)
    hit = np.stack([sel["pos1"], sel["pos2"]], axis=1) >= 0
    if what == "filters":      # chosen, but below `filters`: no begin position and no CIGAR, exactly as align_windows leaves them
        low = hit & (res["score1"] < 120)
        assert low.any() and (hit & ~low).any() and (res["ref_begin1"][low] == -1).all() and (res["cigarLen"][low] == 0).all()
        assert (res["cigarLen"][hit & ~low] > 0).all()
    if what == "flag2":
        assert (res["cigarLen"][hit] > 0).all() and (res["cigar_off"][~hit] == -1).all()
    if what == "mark":
        assert (res["edit_distance"][hit] >= 0).all() and (res["edit_distance"][hit] > 0).any()


def _rebase(ctx, nfrag, L):
    case = _case(9500, _sizes(9501, nfrag, ((0, 3), (4, 0), (17, 9))), L)
    Q, T = case.upload(ctx)
    a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, INS[0], INS[1], 30)
    try:
        for kw in (dict(flag=0), dict(flag=2), dict(flag=0, min_score=70000)):
            s0, rel, c0 = ctx.align_windows_mates(*a, **kw)
            s1, reb, c1 = ctx.align_windows_mates(*a, rebase=True, **kw)
            pos = np.stack([s0["pos1"], s0["pos2"]], axis=1)
            hit = pos >= 0
            nf = len(s0)
            wb = np.zeros((nf, 2), dtype=np.int64); wb[hit] = case.b[(case.co[:-1].reshape(nf, 2) + pos)[hit]]
            exp = rel.copy()
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                exp[f] = np.where(rel[f] >= 0, rel[f] + wb, rel[f])
            assert s0.tobytes() == s1.tobytes() and (reb == exp).all() and c0.tobytes() == c1.tobytes()
            assert (reb["ref_begin1"][~hit] == -1).all() and (reb["ref_end1"][~hit] == 0).all()
            if kw["flag"] == 2:
                assert hit.any() and (reb["ref_begin1"][hit] >= wb[hit]).all()
            if kw.get("min_score"):
                assert not hit.any() and (s0["score"] == 0).all()
    finally:
        Q.free(); T.free()


def _envelopes(ctx):
    """6. a 700-residue read (the fallback), an 800-residue read (the strip kernel's pair mode), an empty window and gapO == gapE inside
    fragments, as winners and as losers"""
    tg = np.asarray(random_ref(6000, 9600, 4), dtype=np.int8)
    other = np.asarray(random_ref(2000, 9601, 4), dtype=np.int8)
    reads = [tg[1000:1800].copy(), _revcomp(tg[2500:3200]), tg[300:400].copy(), _revcomp(tg[500:580]), tg[4000:4100].copy(), _revcomp(tg[4300:4390])]
    nr = len(reads)
    rows = [[(0, 0, 900, 1000), (2, 1, 0, 200)], [(nr + 1, 0, 2400, 900), (nr + 3, 1, 100, 200)],          # 0: the long reads win, both classes in one fragment
            [(0, 1, 0, 1000), (2, 0, 250, 200), (nr + 1, 1, 500, 900)], [(nr + 3, 0, 77, 0), (nr + 3, 0, 450, 200)],      # 1: they lose to short reads' hits; an empty window
            [(4, 0, 3950, 200)], [(nr + 5, 0, 77, 0)],                                                      # 2: mate 2 has an empty window only
            [(4, 0, 3950, 200), (4, 0, 3900, 300)], [(nr + 5, 0, 4250, 200)]]
    case = Case.explicit(reads, [tg, other], rows)
    for kw in (dict(flag=0), dict(flag=2)):
        sel, res, _, tm, _ = _check(ctx, case, 0, 5000, 40, **kw)
        assert [int(x) for x in sel["pos1"]] == [0, 1, 0, 0] and [int(x) for x in sel["pos2"]] == [0, 1, -1, 0]
        assert [int(x) for x in sel["score"]] == [3000, 360, 200, 380] and [int(x) for x in sel["proper"]] == [1, 1, 0, 1]
        assert int(sel["n_eligible2"][2]) == 0 and int(sel["second_score"][2]) == 0 and int(sel["second_score"][3]) == 380
        assert tm["win_copied"] > 0
        if kw["flag"]:
            assert (res["cigarLen"][sel["pos1"] >= 0, 0] > 0).all()
        sel, _, _, tm, _ = _check(ctx, case, 0, 5000, 40, gapO=1, gapE=1, **kw)      # gapO == gapE: every candidate takes the fallback
        # (with gaps that cheap the long reads score high against any window: fragment 1's winner is the oracle's business alone)
        assert [int(x) for x in sel["pos1"][[0, 2, 3]]] == [0, 0, 0] and not tm["fill_kernel"].startswith("k_fillpairs<")


def _errors(ctx, other_ctx):
    """7. refused calls leave the caller's arrays alone and the context usable"""
    reads = [random_ref(30, 1, 4), random_ref(30, 4, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    case = Case.explicit(reads, targets, [[(0, 0, 0, 40), (0, 1, 5, 50)], [(3, 0, 10, 30)]])
    Q, T = case.upload(ctx); Qo = other_ctx.upload(reads)
    ok = dict(cand_off=[0, 2, 3], qidx=[0, 0, 3], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30])
    m = np.ascontiguousarray(MAT, dtype=np.int8)

    def sentinel():
        sel = np.zeros(1, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
        out = np.zeros((1, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
        return sel, out

    def call(arr, sel, out, words, Qx=Q, nfrag=1, nfwd=2, mn=0, mx=500, pen=10, flag=0, null=()):
        p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
        a = [ctx.h, Qx.h, T.h, arr[0].ctypes.data, nfrag, arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data, arr[4].ctypes.data, nfwd,
             C.byref(p), 0, mn, mx, pen, sel.ctypes.data, out.ctypes.data, None]
        for at in null:
            a[at] = None
        return ctx.lib.ssw_gpu_align_windows_mates(*a, C.byref(words))

    def refused(what, change=None, **kw):
        for flag in (0, 2):
            args = {f: list(v) for f, v in ok.items()}
            for f, (at, v) in (change or {}).items():
                args[f][at] = v
            sel, out = sentinel()
            before = sel.tobytes() + out.tobytes()      # (arrays of the caller: every byte, padding included, must stay)
            words = C.c_int64(5)
            arr = [np.ascontiguousarray(args[f], dtype=d) for f, d in (("cand_off", np.int64), ("qidx", np.int32), ("tidx", np.int32), ("tbeg", np.int64), ("tlen", np.int32))]
            rc = call(arr, sel, out, words, flag=flag, **kw)
            assert rc == -1 and re.search(what, ctx.error()), ctx.error()
            assert words.value == 0 and sel.tobytes() + out.tobytes() == before
            s2, _, _, _, _ = _check(ctx, case, 0, 500, 10, flag=flag)      # the context answers the next call
            assert int(s2["n_eligible1"][0]) == 2
    try:
        refused(r"cand_off\[0\] must be 0.*fragment 0", dict(cand_off=(0, 1)))
        refused(r"cand_off decreases.*fragment 0, mate 2", dict(cand_off=(1, 4)))      # [0, 4, 3]: mate 2 runs backwards
        refused(r"align_windows_mates: window out of range.*pair 2\b", dict(tlen=(2, 31)))
        refused(r"align_windows_mates: index out of range.*pair 1\b", dict(tidx=(1, 2)))
        refused(r"nfwd outside.*nfwd = 5", nfwd=5)
        refused(r"nfwd outside.*nfwd = -1", nfwd=-1)
        refused(r"min_insert <= max_insert.*min_insert = -1", mn=-1)
        refused(r"min_insert <= max_insert.*min_insert = 501", mn=501)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= -1", pen=-1)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= 65536", pen=65536)
        refused("another context", Qx=Qo)
        big = np.array([0, GROUP_MAX + 1, GROUP_MAX + 2], dtype=np.int64)      # refused from cand_off alone, before a candidate is read
        arr = [big] + [np.zeros(4, dtype=d) for d in (np.int32, np.int32, np.int64, np.int32)]
        sel, out = sentinel(); before = sel.tobytes() + out.tobytes(); words = C.c_int64(5)
        assert call(arr, sel, out, words) == -1 and re.search(r"more than 4096 candidates in a group.*fragment 0, mate 1", ctx.error()), ctx.error()
        assert words.value == 0 and sel.tobytes() + out.tobytes() == before
        # too many fragments / candidates: refused from nfrag and cand_off alone
        arr[0] = np.array([0, 1, 3], dtype=np.int64)
        assert call(arr, sel, out, words, nfrag=0x7fffff00 // 2 + 1) == -1 and "more than 2^31 output slots" in ctx.error()
        assert sel.tobytes() + out.tobytes() == before
        # NULL arrays, straight through the C ABI
        arr = [np.ascontiguousarray(ok[f], dtype=d) for f, d in (("cand_off", np.int64), ("qidx", np.int32), ("tidx", np.int32), ("tbeg", np.int64), ("tlen", np.int32))]
        for at in (3, 5, 6, 7, 8, 15, 16):
            words = C.c_int64(5)
            assert call(arr, sel, out, words, null=(at,)) == -1 and "NULL argument" in ctx.error() and words.value == 0
            assert sel.tobytes() + out.tobytes() == before
        # no fragments; fragments without candidates
        e = np.zeros(0, np.int32)
        s, r, c = ctx.align_windows_mates(Q, T, [0], e, e, np.zeros(0, np.int64), e, 2, MAT, 5, 0, 500, 10, flag=2)
        assert s.shape == (0,) and r.shape == (0, 2) and c.shape == (0,)
        words = C.c_int64(5)
        assert call(arr, sel, out, words, nfrag=0) == 0 and words.value == 0 and sel.tobytes() + out.tobytes() == before
        s, r, c = ctx.align_windows_mates(Q, T, [0, 0, 0, 0, 0], e, e, np.zeros(0, np.int64), e, 2, MAT, 5, 0, 500, 10, flag=2)
        assert (s["pos1"] == -1).all() and (s["pos2"] == -1).all() and (s["score"] == 0).all() and (s["n_eligible1"] == 0).all()
        assert (r["cigar_off"] == -1).all() and (r["ref_begin1"] == -1).all() and c.shape == (0,)
        with pytest.raises(ValueError):
            ctx.align_windows_mates(Q, T, [0, 1], [0], [0], [0], [1], 2, MAT, 5, 0, 500, 10)
        with pytest.raises(RuntimeError, match="unpaired_penalty must be"):
            ctx.align_windows_mates(Q, T, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], 2, MAT, 5, 0, 500, 70000)
    finally:
        Q.free(); T.free(); Qo.free()


def _small_budget(lib_path, nfrag, L):
    """8. a budget of 1 MiB: the fill runs as several launches, the call-long record array and the output stay whole"""
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        case = _case(9800, _sizes(9801, nfrag, ((0, 20), (33, 17))), L, qlen=(64, 64), wlen=(230, 250))
        Q, T = case.upload(ctx)
        a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, INS[0], INS[1], 30)
        for flag in (0, 2):
            s0, r0, c0 = ctx.align_windows_mates(*a, flag=flag)
            l0 = ctx.timing()["fill_launches"]
            ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
            s1, r1, c1 = ctx.align_windows_mates(*a, flag=flag)
            tm = ctx.timing()
            ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
            assert tm["fill_launches"] > 1 and tm["fill_launches"] > l0 and tm["win_copied"] == 0
            assert s0.tobytes() == s1.tobytes() and (r0 == r1).all() and c0.tobytes() == c1.tobytes()
            assert (s0["pos1"] >= 0).sum() == (np.diff(case.co)[0::2] > 0).sum()
        Q.free(); T.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- emulator

E_L = 3000


def test_emu_group_size_grid(ectx):
    _grid(ectx, len(GRID), E_L)


@pytest.mark.parametrize("nfrag", NFRAGS)
def test_emu_fragment_counts(ectx, nfrag):
    _counts(ectx, nfrag)


def test_emu_insert_edges(ectx):
    _insert_edges(ectx)


def test_emu_penalty_switch(ectx):
    _penalty_switch(ectx)


def test_emu_ties(ectx):
    _ties(ectx)


@pytest.mark.parametrize("what", ["flag0", "flag1", "flag2", "filters", "mark"])
def test_emu_flags(ectx, what):
    _flags(ectx, what, 20, E_L)


def test_emu_rebase(ectx):
    _rebase(ectx, 20, E_L)


def test_emu_out_of_envelope_candidates(ectx):
    _envelopes(ectx)


def test_emu_errors(ectx):
    other = ssw_amd.Context(0, ectx.lib)
    try:
        _errors(ectx, other)
    finally:
        other.close()


def test_emu_small_budget(emu_lib_path):
    _small_budget(emu_lib_path, 120, 20000)


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NF, G_L = 10000, 400000


@pytest.mark.gpu
def test_gpu_group_size_grid(gpu_ctx):
    _grid(gpu_ctx, G_NF, G_L, sample=400, gpu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("nfrag", NFRAGS)
def test_gpu_fragment_counts(gpu_ctx, nfrag):
    _counts(gpu_ctx, nfrag)


@pytest.mark.gpu
def test_gpu_largest_group(gpu_ctx):
    """one fragment with a group of SSW_GPU_MATES_GROUP_MAX cheap candidates: 20-residue reads, 30-column windows, 4096 x 3 combinations"""
    rng = np.random.default_rng(9900)
    tg = np.asarray(random_ref(3000, 9901, 4), dtype=np.int8)
    reads = [tg[1000:1020].copy(), _revcomp(tg[1200:1220])]
    g1 = [(0, 0, int(x), 30) for x in rng.integers(1100, 2970, size=GROUP_MAX)]      # (none of them holds the read's locus)
    g1[4000] = (0, 0, 995, 30)
    g2 = [(2 + 1, 0, 100, 30), (2 + 1, 0, 1195, 30), (1, 0, 1195, 30)]
    case = Case.explicit(reads, [tg], [g1, g2, [(0, 0, 995, 30)], [(2 + 1, 0, 1195, 30)]])
    for flag in (0, 2):
        sel, _, _, _, _ = _check(gpu_ctx, case, 100, 500, 30, sample=400, flag=flag)
        assert (int(sel["pos1"][0]), int(sel["pos2"][0]), int(sel["proper"][0]), int(sel["score"][0])) == (4000, 1, 1, 80)
        assert int(sel["n_eligible1"][0]) == GROUP_MAX


@pytest.mark.gpu
def test_gpu_insert_edges(gpu_ctx):
    _insert_edges(gpu_ctx)


@pytest.mark.gpu
def test_gpu_penalty_switch(gpu_ctx):
    _penalty_switch(gpu_ctx)


@pytest.mark.gpu
def test_gpu_ties(gpu_ctx):
    _ties(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["flag0", "flag1", "flag2", "filters", "mark"])
def test_gpu_flags(gpu_ctx, what):
    _flags(gpu_ctx, what, G_NF, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_rebase(gpu_ctx):
    _rebase(gpu_ctx, G_NF, G_L)


@pytest.mark.gpu
def test_gpu_out_of_envelope_candidates(gpu_ctx):
    _envelopes(gpu_ctx)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    other = ssw_amd.Context(0, gpu_ctx.lib)
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_small_budget(product_lib_path):
    _small_budget(product_lib_path, G_NF, G_L)
