"""ssw_gpu_align_windows_mates_rescue: mate rescue on the device (include/ssw_gpu.h).

Every group of a fragment gets A = max_anchors rescue slots behind the caller's candidates: for the r-th best eligible candidate of the
OTHER mate (score1 >= anchor_min_score; score1 descending, position ascending) that has no proper partner among the caller's eligible
candidates of this mate, the window a proper partner can occupy -- [B + mn - L - P, B + mx - 1 + P] downstream of the anchor,
[E + 1 - mx - P, E - mn + L + P] upstream, clipped to the target; every other slot is empty.  The call's answer is, bit for bit, what
ssw_gpu_align_windows_mates_lib gives for that augmented list.

Two oracles, no fragment left out.  (a) the definition: Context.align_windows at flag 0 over the caller's candidates, the rule above in
plain Python (Python integers), the augmented list, and the EXISTING Context.align_windows_mates over it -- every field of `sel`, every
record field (cigar_off included), the pool bytes, `origin` against the augmented arrays and rescue_windows against the Python count of
non-empty slots.  (b) the reference through parity.expected() on the cut-out window of every chosen rescue candidate (all of them on the
emulator, a fixed-seed sample of 400 on the GPU).  Every case goes through one helper (_check) and runs on the CPU SIMT emulator
(tests/emu: the real host driver and the real kernel source) and, marked gpu, on the MI355X with more fragments.

Shapes: reads of 40..100 residues, two targets of about 3 000 columns, inserts of 150..400 with (mn, mx) = (100, 500), P = 16: rescue
windows of at most about 530 columns.  The selection and the window arithmetic see only scores, end columns, lengths, targets and
strands, so nothing larger can make them go wrong."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, random_ref
from test_windows_mates import MAT, Case, _all, _cig, _mut, _revcomp

INS = (100, 500)
PAD = 16
NFRAGS = [1, 3, 4, 5, 15, 16, 17, 33]   # row, wavefront and workgroup edges of one 16-lane row per fragment
GROUP_MAX = 4096                        # SSW_GPU_MATES_GROUP_MAX (include/ssw_gpu.h)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


class RescueCase(Case):
    """fragments of a library `made` (fr / rf / ff as in tests/test_mates_orient.py: ff has both mates on the plus strand with mate 1
    left in even fragments, both on the minus strand with mate 2 left in odd ones), 150..400 columns on one of two targets; reads 2 f and
    2 f + 1 are the mates of fragment f.  sizes[f] = (n1, n2) candidates.  The FIRST candidate of a group is the mate's true locus with
    20 columns of margin, on its strand; the others lie anywhere, on either target and strand.  plant[f]: 0 nothing; 1 mate 2 loses its
    true candidate and keeps wrong ones only (the other target, or its own target on the wrong strand); 2 the same for mate 1.  edge[f]: 1 the fragment starts within 5 columns of column 0,
    2 it ends within 5 columns of the target's end (the rescue windows leave the target there)."""

    def __init__(self, seed, sizes, made, plant=None, edge=None, L=3000, qlen=(40, 100), sub=0.03, long_mate=None):
        rng = np.random.default_rng(seed)
        self.targets = [np.asarray(random_ref(L + 37 * j, int(rng.integers(1 << 30)), 4), dtype=np.int8) for j in range(2)]
        nr = 2 * len(sizes)
        reads, rows, self.home = [], [], []
        for f, (n1, n2) in enumerate(sizes):
            t = int(rng.integers(2)); tl = len(self.targets[t])
            l1, l2 = (int(x) for x in rng.integers(qlen[0], qlen[1] + 1, size=2))
            ins = int(rng.integers(150, 401))
            if long_mate is not None and f == long_mate[0]:
                ins = 1200; l2 = long_mate[1]      # the right mate is a long read
            e = edge[f] if edge else 0
            s = int(rng.integers(0, 6)) if e == 1 else tl - ins - int(rng.integers(0, 6)) if e == 2 else int(rng.integers(0, tl - ins + 1))
            lrev, rrev = dict(fr=(False, True), rf=(True, False), ff=((True, True) if f % 2 else (False, False)))[made]
            lseq = _mut(self.targets[t][s:s + l1], rng, sub); rseq = _mut(self.targets[t][s + ins - l2:s + ins], rng, sub)
            left = (_revcomp(lseq) if lrev else lseq, s, lrev)                    # (read as stored, locus, matches as reverse complement)
            right = (_revcomp(rseq) if rrev else rseq, s + ins - l2, rrev)
            if made == "ff":
                mates = (right, left) if f % 2 else (left, right)
            else:
                mates = (left, right) if rng.random() < 0.5 else (right, left)
            for h, sz in enumerate((n1, n2)):
                rd, home, rev = mates[h]
                reads.append(rd)
                self.home.append((t, home, len(rd)))
                row = []
                for k in range(sz):
                    if k == 0:
                        wb = max(home - 20, 0); wl = min(home + len(rd) + 20, tl) - wb
                        row.append((2 * f + h + (nr if rev else 0), t, wb, wl))
                    else:
                        ct = int(rng.integers(2)); wl = int(rng.integers(80, 251)); wb = int(rng.integers(0, len(self.targets[ct]) - wl + 1))
                        crev = rng.random() < 0.5
                        if plant and plant[f] == 2 - h and ct == t:      # the mate that loses its candidate keeps WRONG ones only: the other
                            crev = not rev                               # target, or the strand on which the read does not match
                        row.append((2 * f + h + (nr if crev else 0), ct, wb, wl))
                if plant and plant[f] == 2 - h and sz > 0:
                    row = row[1:]
                rows.append(row)
        self._finish(reads, rows)
        self.mate_q = np.arange(nr, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _case(seed, sizes, made, plant=None, edge=None, **kw):
    return RescueCase(seed, list(sizes), made, plant, edge, **dict(kw))


def _sizes(seed, nfrag, extra=(), hi=5):
    rng = np.random.default_rng(seed)
    return tuple(list(extra) + [(int(a), int(b)) for a, b in rng.integers(0, hi + 1, size=(nfrag - len(extra), 2))])


def _augment(a0, case, orient, A, ams, pad, mn, mx, min_score):
    """the header's rule over align_windows' flag-0 records of the caller's candidates, in Python integers
    -> (cand_off, qidx, tidx, tbeg, tlen of the augmented list, anchor per slot [2 nfrag][A] (-1: empty), non-empty slots)"""
    co = [int(x) for x in case.co]
    ng = len(co) - 1
    s = [int(x) for x in a0["score1"]]
    ok = [int(st) == 0 and sc > 0 and sc >= min_score for st, sc in zip(a0["status"], s)]
    minus = [int(x) >= case.nfwd for x in case.q]
    ln = [len(case.reads[int(x)]) for x in case.q]
    E = [int(case.b[i]) + int(a0["ref_end1"][i]) for i in range(co[-1])]
    B = [E[i] - ln[i] + 1 for i in range(co[-1])]

    def proper(a, b):      # a of mate 1, b of mate 2
        if int(case.t[a]) != int(case.t[b]):
            return False
        if orient == "ff":
            if minus[a] != minus[b]:
                return False
            d = E[a] - B[b] + 1 if minus[a] else E[b] - B[a] + 1
        else:
            if minus[a] == minus[b]:
                return False
            p, m = (b, a) if minus[a] else (a, b)
            d = E[m] - B[p] + 1 if orient == "fr" else E[p] - B[m] + 1
        return mn <= d <= mx

    aco, aq, at, ab, al, anchors, filled = [0], [], [], [], [], [], 0
    for g in range(ng):
        h, og = g & 1, g ^ 1
        mq = int(case.mate_q[g]); L = len(case.reads[mq])
        rank = sorted([i for i in range(co[og], co[og + 1]) if ok[i] and s[i] >= ams], key=lambda i: (-s[i], i))[:A]
        mine = [i for i in range(co[g], co[g + 1]) if ok[i]]
        for i in range(co[g], co[g + 1]):
            aq.append(int(case.q[i])); at.append(int(case.t[i])); ab.append(int(case.b[i])); al.append(int(case.l[i]))
        row = []
        for r in range(A):
            slot = (mq, 0, 0, 0, -1)
            if r < len(rank) and not any((proper(x, rank[r]) if h == 0 else proper(rank[r], x)) for x in mine):
                a = rank[r]
                sa = minus[a]; sr = sa if orient == "ff" else not sa
                # which of the two lies downstream: the minus-strand one (FR), the plus-strand one (RF), mate 2 if both are plus and mate 1
                # if both are minus (FF)
                down = sr if orient == "fr" else (not sr) if orient == "rf" else ((h == 0) if sr else (h == 1))
                w0, w1 = (B[a] + mn - L - pad, B[a] + mx - 1 + pad) if down else (E[a] + 1 - mx - pad, E[a] - mn + L + pad)
                t = int(case.t[a])
                w0 = max(w0, 0); w1 = min(w1, len(case.targets[t]) - 1)
                if w1 - w0 + 1 >= 1:
                    slot = (mq + (case.nfwd if sr else 0), t, w0, w1 - w0 + 1, a - co[og])
                    filled += 1
            aq.append(slot[0]); at.append(slot[1]); ab.append(slot[2]); al.append(slot[3]); row.append(slot[4])
        anchors.append(row)
        aco.append(len(aq))
    return (np.array(aco, dtype=np.int64), np.array(aq, dtype=np.int32), np.array(at, dtype=np.int32), np.array(ab, dtype=np.int64),
            np.array(al, dtype=np.int32), anchors, filled)


def _check(ctx, case, orient="fr", A=2, ams=0, pad=PAD, mn=INS[0], mx=INS[1], pen=17, min_score=0, sample=None, mat=MAT, n=5, **kw):
    """align_windows_mates_rescue against oracle (a) for every fragment and oracle (b) for every chosen rescue candidate
    -> (sel, records, origin, timing, (sel, records, pool) of the EXISTING call on the caller's list, augmented arrays, pool)"""
    co = case.co
    nf = (len(co) - 1) // 2
    Q, T = case.upload(ctx)
    try:
        a = (Q, T, co, case.q, case.t, case.b, case.l, case.nfwd)
        sel, res, org, cig = ctx.align_windows_mates_rescue(*a, case.mate_q, mat, n, mn, mx, pen, max_anchors=A, anchor_min_score=ams, rescue_pad=pad,
                                                            min_score=min_score, orientation=orient, **kw)
        tm = ctx.timing()
        kw0 = {k: v for k, v in kw.items() if k not in ("flag", "filters", "filterd", "mark_mismatch")}
        a0, _ = _all(ctx, case, Q, T, mat, n, flag=0, **kw0)
        aco, aq, at, ab, al, anchors, filled = _augment(a0, case, orient, A, ams, pad, mn, mx, min_score)
        esel, eres, ecig = ctx.align_windows_mates(Q, T, aco, aq, at, ab, al, case.nfwd, mat, n, mn, mx, pen, min_score=min_score, orientation=orient, **kw)
        assert ctx.timing()["rescue_windows"] == 0          # the existing entry points report none
        old = ctx.align_windows_mates(*a, mat, n, mn, mx, pen, min_score=min_score, orientation=orient, **kw)
        assert ctx.timing()["rescue_windows"] == 0
    finally:
        Q.free(); T.free()
    bad = []
    for f in np.nonzero((sel != esel) | (res != eres).any(axis=1))[0][:4]:
        bad.append("fragment %d (candidates [%d, %d) + [%d, %d)): expected %s %s, got %s %s" % (f, co[2 * f], co[2 * f + 1], co[2 * f + 1], co[2 * f + 2],
                                                                                                 esel[f], eres[f], sel[f], res[f]))
    assert not bad, "\n".join(bad)
    assert sel.shape == (nf,) and res.shape == (nf, 2) and org.shape == (nf, 2)
    assert sel.tobytes() == esel.tobytes()              # every field, the padding included
    assert (res == eres).all()                          # every field, cigar_off included
    assert cig.tobytes() == ecig.tobytes()
    assert tm["rescue_windows"] == filled
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    size = np.diff(co).reshape(nf, 2)
    eorg = np.zeros((nf, 2), dtype=ssw_amd.RESCUED_DTYPE)
    eorg["tidx"] = -1; eorg["qidx"] = -1; eorg["anchor"] = -1
    for f, h in np.argwhere(pos >= 0):
        i = int(aco[2 * f + h]) + int(pos[f, h])
        eorg[f, h] = (ab[i], al[i], at[i], aq[i], anchors[2 * f + h][pos[f, h] - size[f, h]] if pos[f, h] >= size[f, h] else -1)
    assert org.tobytes() == eorg.tobytes()
    assert ((pos < size) | (org["anchor"] >= 0)).all()      # an empty slot is never chosen
    if not kw.get("mark_mismatch", False):
        slots = np.argwhere(pos >= size)
        if sample is not None and len(slots) > sample:
            slots = slots[np.random.default_rng(5).choice(len(slots), size=sample, replace=False)]
        gapO, gapE, ml, flag = kw.get("gapO", 3), kw.get("gapE", 1), kw.get("maskLen", -1), kw.get("flag", 0)
        for f, h in slots:
            o = org[f, h]
            rd = case.reads[int(o["qidx"])]
            rf = np.ascontiguousarray(case.targets[int(o["tidx"])][int(o["tbeg"]):int(o["tbeg"]) + int(o["tlen"])])
            exp, xcig = expected(rd, mat, n, rf, gapO, gapE, flag, kw.get("filters", 0), kw.get("filterd", 0), ml if ml >= 0 else len(rd) // 2,
                                 kw.get("score_size", 2))
            rec = res[f, h]
            ok = exp is not None and int(rec["status"]) == 0 and {x: int(rec[x]) for x in RES_FIELDS} == exp and _cig(rec, cig) == xcig
            if not ok and len(bad) < 4:
                bad.append("fragment %d mate %d rescue window (len %d x %d): expected %s %s got %s" % (f, h + 1, len(rd), len(rf), exp, cigar_str(xcig), rec))
        assert not bad, "\n".join(bad)
    return sel, res, org, tm, old, (aco, aq, at, ab, al), cig


# ------------------------------------------------------------------------------------------------------------- the cases

def _planted(ctx, nfrag, orient, sample=None):
    """1. in a third of the fragments one mate has lost its true candidate: the existing call finds no proper pair there, the new one
    finds it in a rescue slot, at the planted locus"""
    plant = tuple((1 + (f // 3) % 2) if f % 3 == 0 else 0 for f in range(nfrag))
    sizes = tuple((3, 3) if f % 6 else (3, 1) for f in range(nfrag))      # (f % 6 == 0: mate 2 ends up without any candidate)
    case = _case(9700, sizes, orient, plant)
    for kw in (dict(flag=0), dict(flag=2)):
        # (min_score 50: above what a read scores against a window it does not come from, so that the mate that lost its candidate has none)
        sel, res, org, tm, (old, _, _), _, _ = _check(ctx, case, orient, min_score=50, sample=sample, **kw)
        lost = np.array(plant) > 0
        assert (old["proper"][lost] == 0).all() and (sel["proper"][lost] == 1).all() and tm["rescue_windows"] >= int(lost.sum())
        size = np.diff(case.co).reshape(nfrag, 2)
        for f in np.nonzero(lost)[0]:
            h = 2 - plant[f]
            p = (sel["pos1"], sel["pos2"])[h][f]
            assert p >= size[f, h] and org["anchor"][f, h] >= 0
            t, home, ln = case.home[2 * f + h]
            end = int(org["tbeg"][f, h]) + int(res["ref_end1"][f, h])      # (rebase: origin's tbeg)
            # the alignment ends at the locus' last column, give or take what 3 % substitutions can move it: a mismatch run at the
            # read's end is clipped (to the left), a gap near the end bought by the matches behind it shifts it (either way); a shift
            # of k columns costs 3 + (k - 1) against 2 per match regained, so 12 columns is far outside what a 40..100-residue read
            # with a handful of substitutions can pay for
            assert int(org["tidx"][f, h]) == t and home + ln - 1 - 12 <= end <= home + ln - 1 + 12
    Q, T = case.upload(ctx)
    try:
        a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, case.mate_q, MAT, 5, INS[0], INS[1], 17)
        s0, r0, o0, c0 = ctx.align_windows_mates_rescue(*a, flag=2, min_score=50, orientation=orient)
        s1, r1, o1, c1 = ctx.align_windows_mates_rescue(*a, flag=2, min_score=50, orientation=orient, rebase=True)
        assert s0.tobytes() == s1.tobytes() and o0.tobytes() == o1.tobytes() and c0.tobytes() == c1.tobytes()
        for f in ("ref_begin1", "ref_end1", "ref_end2"):
            assert (r1[f] == np.where(r0[f] >= 0, r0[f] + o0["tbeg"], r0[f])).all()
    finally:
        Q.free(); T.free()


def _suppressed(ctx, nfrag):
    """2. every fragment's anchors already have a proper partner: only empty slots, no second fill, the existing call's answer"""
    case = _case(9710, tuple((1, 1) for _ in range(nfrag)), "fr")
    for flag in (0, 2):
        sel, res, org, tm, (osel, ores, ocig), _, cig = _check(ctx, case, "fr", flag=flag)
        assert tm["rescue_windows"] == 0 and (sel["proper"] == 1).all() and (org["anchor"] == -1).all()
        # the whole answer of the existing call on the caller's list (positions below the group sizes are the same in either list)
        assert sel.tobytes() == osel.tobytes() and (res == ores).all() and cig.tobytes() == ocig.tobytes()


def _clipping(ctx, orient):
    """3. fragments at column 0 and at the target's last column, the anchor on either strand and as either mate"""
    nfrag = 16
    plant = tuple(1 + f % 2 for f in range(nfrag))
    edge = tuple(1 + (f // 2) % 2 for f in range(nfrag))
    case = _case(9720, tuple((2, 2) for _ in range(nfrag)), orient, plant, edge)
    sel, res, org, tm, old, aug, _ = _check(ctx, case, orient, min_score=50, flag=2)
    aco, aq, at, ab, al = aug
    tl = np.array([len(t) for t in case.targets])
    live = al > 0
    assert (ab[live] == 0).any() and (ab[live] + al[live] == tl[at[live]]).any()      # windows cut at both ends of a target
    assert (sel["proper"] == 1).sum() >= nfrag // 2


def _clipped_away(ctx):
    """3b. the window lies beyond the target's end: an empty slot.  Plus-strand anchor at [2930, 2990) of a 3 000-column target, FR,
    (mn, mx) = (200, 500), L = 60, P = 16: columns [2930 + 200 - 60 - 16, ...] = [3054, ...] -- none left after clipping"""
    tg = np.asarray(random_ref(3000, 9730, 4), dtype=np.int8)
    reads = [tg[2930:2990].copy(), _revcomp(tg[100:160])]
    case = Case.explicit(reads, [tg], [[(0, 0, 2900, 100)], []])
    case.mate_q = np.arange(2, dtype=np.int32)
    sel, res, org, tm, old, aug, _ = _check(ctx, case, "fr", mn=200, mx=500, flag=2)
    assert tm["rescue_windows"] == 0 and int(sel["pos1"][0]) == 0 and int(sel["pos2"][0]) == -1
    sel, res, org, tm, old, aug, _ = _check(ctx, case, "fr", mn=100, mx=500, flag=2)      # (mn = 100: columns [2954, 2999] remain)
    assert tm["rescue_windows"] == 1 and int(aug[3][3]) == 2954 and int(aug[4][3]) == 46


def _anchors(ctx, A):
    """4. A anchors per mate; fewer eligible anchors than A; anchor_min_score through the middle; ties in the anchors' score (the same
    window twice in a group)"""
    nfrag = 12
    sizes = ((4, 0), (0, 4), (9, 1), (1, 9)) + tuple((5, 5) for _ in range(nfrag - 4))
    plant = (0, 0, 1, 2) + tuple(1 + f % 2 for f in range(nfrag - 4))
    case = _case(9740 + A, sizes, "fr", plant)
    # a tie: fragment 4's mate 1 (which keeps its true locus) lists it twice
    c0 = int(case.co[8])
    case.q[c0 + 1], case.t[c0 + 1], case.b[c0 + 1], case.l[c0 + 1] = case.q[c0], case.t[c0], case.b[c0], case.l[c0]
    case.all.clear()
    sel, res, org, tm, old, _, _ = _check(ctx, case, "fr", A=A, flag=2)
    assert tm["rescue_windows"] > 0
    if A >= 2:
        assert tm["rescue_windows"] > int((np.array(plant) > 0).sum())      # more than the best anchor produced a window
    _, _, _, tm2, _, _, _ = _check(ctx, case, "fr", A=A, ams=140, flag=0)      # reads of 40 .. 100 residues score 80 .. 200
    assert 0 < tm2["rescue_windows"] < tm["rescue_windows"]
    _, _, _, tm3, _, _, _ = _check(ctx, case, "fr", A=A, ams=60000, flag=0)
    assert tm3["rescue_windows"] == 0


def _geometry(ctx, nfrag):
    """5. fragment counts on the row, wavefront and workgroup edges; n1 + n2 + 2 A on both sides of 16 and of 48 (the LDS digests);
    empty groups for one mate and for both"""
    extra = ((0, 0), (0, 3), (6, 6), (6, 7), (22, 22), (21, 22), (23, 22), (40, 30))[:max(1, min(8, nfrag))]
    sizes = _sizes(9750 + nfrag, nfrag, extra[:nfrag])
    plant = tuple(f % 3 for f in range(nfrag))
    case = _case(9760, sizes, "fr", plant)
    sel, _, _, _, _, _, _ = _check(ctx, case, "fr", flag=2)
    assert sel.shape == (nfrag,)


def _grown_record_array(lib_path):
    """5b. the FIRST call of a fresh context: the record array is sized for the caller's candidates (48 bytes each, one more for the empty
    slots, 64 per group, an eighth and 256 bytes of headroom), and the rescue windows' records do not fit behind them -- the array moves
    (k_copy16) before the second fill.  20 fragments of (3, 0) candidates, min_score 0, A = 8: 60 candidates -> 48 x 61 + 64 x 40 = 5 488
    bytes (a few records more where a length class holds an odd number of pairs), capacity about 6 430; every candidate of mate 1 is an anchor without a partner, 60 windows -> 48 x 121 + 2 560 = 8 368 bytes."""
    ctx = ssw_amd.Context(0, ssw_amd.load(lib_path))
    try:
        case = _case(9790, tuple((3, 0) for _ in range(20)), "fr")
        sel, _, _, tm, _, _, _ = _check(ctx, case, "fr", A=8, flag=2)
        assert tm["rescue_windows"] == 60 and (sel["pos2"] >= 0).all()
    finally:
        ctx.close()


def _flags(ctx, what, nfrag, sample=None):
    """6. flags and post-processing, unpaired_penalty 0 and 17"""
    plant = tuple(f % 3 for f in range(nfrag))
    case = _case(9770, _sizes(9771, nfrag, ((0, 3), (4, 0))), "fr", plant)
    kw = dict(flag0=dict(flag=0), flag1=dict(flag=1), flag2=dict(flag=2), mark=dict(flag=2, mark_mismatch=True))[what]
    for pen in (0, 17):
        sel, res, org, tm, _, _, _ = _check(ctx, case, "fr", pen=pen, sample=sample, **kw)
        hit = np.stack([sel["pos1"], sel["pos2"]], axis=1) >= 0
        assert tm["rescue_windows"] > 0 and tm["best_flagged"] == (int(hit.sum()) if kw["flag"] else 0)
        if what == "flag2":
            assert (res["cigarLen"][hit] > 0).all()
        if what == "mark":
            assert (res["edit_distance"][hit] >= 0).all()


def _fallback(ctx):
    """7. outside the fast-path envelopes: a whole call with gapO <= gapE; one fragment whose rescued mate has 650 residues inside an
    otherwise fast-path list"""
    nfrag = 4
    plant = tuple(1 if f % 2 == 0 else 0 for f in range(nfrag))
    case = _case(9780, tuple((2, 2) for _ in range(nfrag)), "fr", plant)
    _, _, _, tm, _, _, _ = _check(ctx, case, "fr", gapO=1, gapE=1, flag=2)
    assert tm["rescue_windows"] > 0 and not tm["fill_kernel"].startswith("k_fillpairs<")
    # an FF library: in the even fragment 2 mate 2 is the right-hand read -- the 650-residue one -- and it is the mate that lost its
    # candidate, so the second fill holds a fallback slot (that read's) beside the fast-path slots of fragment 0 (mixed second fill)
    big = _case(9781, tuple((2, 2) for _ in range(nfrag)), "ff", plant, None, long_mate=(2, 650))
    sel, res, org, tm, _, _, _ = _check(ctx, big, "ff", mx=1500, min_score=50, flag=2)
    assert len(big.reads[5]) == 650 and len(big.reads[1]) <= 100 and tm["win_copied"] > 0 and tm["rescue_windows"] >= 2
    for f in (0, 2):
        assert int(org["anchor"][f, 1]) >= 0 and int(sel["proper"][f]) == 1
    assert len(big.reads[int(org["qidx"][2, 1])]) == 650


def _errors(ctx, other_ctx):
    """8. refused calls leave the caller's arrays alone and the context usable"""
    reads = [random_ref(30, 1, 4), random_ref(30, 4, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    case = Case.explicit(reads, targets, [[(0, 0, 0, 40), (0, 1, 5, 50)], [(3, 0, 10, 30)]])
    case.mate_q = np.arange(2, dtype=np.int32)
    Q, T = case.upload(ctx); Qo = other_ctx.upload(reads + reads); Qf = ctx.upload(reads)
    ok = dict(cand_off=[0, 2, 3], qidx=[0, 0, 3], tidx=[0, 1, 0], tbeg=[0, 5, 10], tlen=[40, 50, 30], mate_q=[0, 1])
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    types = (("cand_off", np.int64), ("qidx", np.int32), ("tidx", np.int32), ("tbeg", np.int64), ("tlen", np.int32), ("mate_q", np.int32))

    def sentinel():
        sel = np.zeros(1, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
        out = np.zeros((1, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
        org = np.zeros((1, 2), dtype=ssw_amd.RESCUED_DTYPE); org["tbeg"] = 777; org["anchor"] = 777
        return sel, out, org

    def call(arr, sel, out, org, words, Qx=Q, nfrag=1, nfwd=2, mn=0, mx=500, pen=10, orient=0, A=2, ams=0, pad=16, flag=0, null=()):
        p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
        a = [ctx.h, Qx.h, T.h, arr[0].ctypes.data, nfrag, arr[1].ctypes.data, arr[2].ctypes.data, arr[3].ctypes.data, arr[4].ctypes.data, nfwd,
             arr[5].ctypes.data, C.byref(p), 0, mn, mx, pen, orient, A, ams, pad, sel.ctypes.data, out.ctypes.data, org.ctypes.data, None]
        for at in null:
            a[at] = None
        return ctx.lib.ssw_gpu_align_windows_mates_rescue(*a, C.byref(words))

    def refused(what, change=None, **kw):
        for flag in (0, 2):
            args = {f: list(v) for f, v in ok.items()}
            for f, (at, v) in (change or {}).items():
                args[f][at] = v
            sel, out, org = sentinel()
            before = sel.tobytes() + out.tobytes() + org.tobytes()      # (arrays of the caller: every byte, padding included, must stay)
            words = C.c_int64(5)
            arr = [np.ascontiguousarray(args[f], dtype=d) for f, d in types]
            rc = call(arr, sel, out, org, words, flag=flag, **kw)
            assert rc == -1 and re.search(what, ctx.error()), ctx.error()
            assert words.value == 0 and sel.tobytes() + out.tobytes() + org.tobytes() == before
        s2, _, _, _ = ctx.align_windows_mates_rescue(Q, T, case.co, case.q, case.t, case.b, case.l, 2, case.mate_q, MAT, 5, 0, 500, 10, flag=2)
        assert int(s2["n_eligible1"][0]) >= 2      # the context answers the next call
    try:
        # every check of ssw_gpu_align_windows_mates_lib, under this entry point's name
        refused(r"align_windows_mates_rescue: cand_off\[0\] must be 0.*fragment 0", dict(cand_off=(0, 1)))
        refused(r"align_windows_mates_rescue: cand_off decreases.*fragment 0, mate 2", dict(cand_off=(1, 4)))
        refused(r"align_windows_mates_rescue: window out of range.*pair 2\b", dict(tlen=(2, 31)))
        refused(r"align_windows_mates_rescue: index out of range.*pair 1\b", dict(tidx=(1, 2)))
        refused(r"nfwd outside.*nfwd = 5", nfwd=5)
        refused(r"nfwd outside.*nfwd = -1", nfwd=-1)
        refused(r"min_insert <= max_insert.*min_insert = -1", mn=-1)
        refused(r"min_insert <= max_insert.*min_insert = 501", mn=501)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= -1", pen=-1)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= 65536", pen=65536)
        refused(r"orientation must be.*orientation = 3", orient=3)
        refused("another context", Qx=Qo)
        # its own
        refused(r"queries->count must be 2 \* nfwd.*nfwd = 1, 4 queries", nfwd=1, change=dict(qidx=(2, 1)))
        refused(r"queries->count must be 2 \* nfwd.*nfwd = 2, 2 queries", Qx=Qf, change=dict(qidx=(2, 1)))
        refused(r"mate_q outside the forward reads.*fragment 0, mate 2: mate_q = 2", dict(mate_q=(1, 2)))
        refused(r"mate_q outside the forward reads.*fragment 0, mate 1: mate_q = -1", dict(mate_q=(0, -1)))
        refused(r"neither strand of its mate's read.*pair 1 of fragment 0, mate 1: query 1", dict(qidx=(1, 1)))
        refused(r"neither strand of its mate's read.*pair 2 of fragment 0, mate 2: query 2", dict(qidx=(2, 2)))
        refused(r"max_anchors must be 1 \.\. 8.*= 0", A=0)
        refused(r"max_anchors must be 1 \.\. 8.*= 9", A=9)
        refused(r"rescue_pad must be 0 \.\. 65535.*= -1", pad=-1)
        refused(r"rescue_pad must be 0 \.\. 65535.*= 65536", pad=65536)
        refused(r"anchor_min_score must be >= 0.*= -1", ams=-1)
        # a group whose size plus A exceeds the limit: refused before a candidate's window is used
        nbig = GROUP_MAX - 1
        arr = [np.array([0, nbig, nbig + 1], dtype=np.int64), np.zeros(nbig + 1, np.int32), np.zeros(nbig + 1, np.int32), np.zeros(nbig + 1, np.int64),
               np.ones(nbig + 1, np.int32), np.array([0, 1], np.int32)]
        arr[1][nbig] = 1
        sel, out, org = sentinel(); before = sel.tobytes() + out.tobytes() + org.tobytes(); words = C.c_int64(5)
        assert call(arr, sel, out, org, words) == -1 and re.search(r"more than 4096 candidates and rescue slots.*fragment 0, mate 1: 4095 candidates \+ 2", ctx.error()), ctx.error()
        assert words.value == 0 and sel.tobytes() + out.tobytes() + org.tobytes() == before
        arr = [np.ascontiguousarray(ok[f], dtype=d) for f, d in types]
        for at in (3, 5, 6, 7, 8, 10, 20, 21, 22):      # NULL arrays, straight through the C ABI
            words = C.c_int64(5)
            assert call(arr, sel, out, org, words, null=(at,)) == -1 and "NULL argument" in ctx.error() and words.value == 0
            assert sel.tobytes() + out.tobytes() + org.tobytes() == before
        # no fragments; fragments without candidates
        words = C.c_int64(5)
        assert call(arr, sel, out, org, words, nfrag=0) == 0 and words.value == 0 and sel.tobytes() + out.tobytes() + org.tobytes() == before
        e = np.zeros(0, np.int32)
        s, r, o, c = ctx.align_windows_mates_rescue(Q, T, [0, 0, 0], e, e, np.zeros(0, np.int64), e, 2, [0, 1], MAT, 5, 0, 500, 10, flag=2)
        assert (s["pos1"] == -1).all() and (s["pos2"] == -1).all() and (r["cigar_off"] == -1).all() and (o["tidx"] == -1).all() and c.shape == (0,)
        _check(ctx, case, "fr", mn=0, mx=500, pen=10, flag=2)
        with pytest.raises(RuntimeError, match="max_anchors must be"):
            ctx.align_windows_mates_rescue(Q, T, ok["cand_off"], ok["qidx"], ok["tidx"], ok["tbeg"], ok["tlen"], 2, [0, 1], MAT, 5, 0, 500, 10, max_anchors=9)
    finally:
        Q.free(); T.free(); Qo.free(); Qf.free()


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_emu_planted_rescue(ectx, orient):
    _planted(ectx, 12, orient)


def test_emu_suppression(ectx):
    _suppressed(ectx, 9)


@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_emu_clipping(ectx, orient):
    _clipping(ectx, orient)


def test_emu_clipped_away(ectx):
    _clipped_away(ectx)


@pytest.mark.parametrize("A", [1, 2, 3, 8])
def test_emu_anchors(ectx, A):
    _anchors(ectx, A)


@pytest.mark.parametrize("nfrag", NFRAGS)
def test_emu_geometry(ectx, nfrag):
    _geometry(ectx, nfrag)


@pytest.mark.parametrize("what", ["flag0", "flag1", "flag2", "mark"])
def test_emu_flags(ectx, what):
    _flags(ectx, what, 10)


def test_emu_grown_record_array(emu_lib_path):
    _grown_record_array(emu_lib_path)


def test_emu_fallback(ectx):
    _fallback(ectx)


def test_emu_errors(ectx):
    other = ssw_amd.Context(0, ectx.lib)
    try:
        _errors(ectx, other)
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NF = 3000


@pytest.mark.gpu
@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_gpu_planted_rescue(gpu_ctx, orient):
    _planted(gpu_ctx, G_NF, orient, sample=400)


@pytest.mark.gpu
def test_gpu_suppression(gpu_ctx):
    _suppressed(gpu_ctx, G_NF)


@pytest.mark.gpu
@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_gpu_clipping(gpu_ctx, orient):
    _clipping(gpu_ctx, orient)


@pytest.mark.gpu
def test_gpu_clipped_away(gpu_ctx):
    _clipped_away(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 3, 8])
def test_gpu_anchors(gpu_ctx, A):
    _anchors(gpu_ctx, A)


@pytest.mark.gpu
@pytest.mark.parametrize("nfrag", NFRAGS + [G_NF])
def test_gpu_geometry(gpu_ctx, nfrag):
    _geometry(gpu_ctx, nfrag)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["flag0", "flag1", "flag2", "mark"])
def test_gpu_flags(gpu_ctx, what):
    _flags(gpu_ctx, what, G_NF, sample=400)


@pytest.mark.gpu
def test_gpu_grown_record_array(product_lib_path):
    _grown_record_array(product_lib_path)


@pytest.mark.gpu
def test_gpu_fallback(gpu_ctx):
    _fallback(gpu_ctx)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx):
    other = ssw_amd.Context(0, gpu_ctx.lib)
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()
