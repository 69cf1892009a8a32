"""ssw_gpu_align_windows_mates_lib: the library orientation of the proper-pair rule (include/ssw_gpu.h, SSW_GPU_MATES_FR / _RF / _FF).

For candidate a of mate 1 and b of mate 2 on one target, E = tbeg + ref_end1 and B = E - len + 1:
  FR  strands differ, p the plus- and m the minus-strand one:  D = E(m) - B(p) + 1
  RF  strands differ:                                           D = E(p) - B(m) + 1
  FF  strands equal; both plus: D = E(b) - B(a) + 1; both minus: D = E(a) - B(b) + 1
and the combination is proper iff min_insert <= D <= max_insert.  Nothing else depends on the orientation.

Two oracles, no fragment left out, as in tests/test_windows_mates.py (whose cases, sizes and helpers are reused): (a) Context.align_windows over
ALL candidates and then the rule above in plain Python -- every field of `sel`, every record field and the pool words; (b) the reference through
parity.expected() on the cut-out window of every chosen candidate (all of them on the emulator, a fixed-seed sample of 400 on the GPU).  Every
case runs on the CPU SIMT emulator at the small size and, marked gpu, on the MI355X with the fragment counts raised."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, random_ref
from test_windows_mates import MAT, Case, _all, _cig, _mut, _revcomp

ORIENTS = ("fr", "rf", "ff")
N1S = [0, 1, 2, 16, 17, 33]         # the 16-lane stride; 33 + 16 = 49 candidates: one past the 48 digests a fragment keeps in LDS
N2S = [0, 1, 16, 40]
GRID = tuple((a, b) for a in N1S for b in N2S)
NFRAGS = [1, 16, 17, 33]
INS = (100, 500)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


class LibCase(Case):
    """test_windows_mates.Case with the fragments of a library `made`: a fragment of 150..400 columns on one of two targets, one mate from
    its left end and one from its right end.
      fr  left on the plus strand (stored as the forward copy), right on the minus strand (stored reverse-complemented); either is mate 1
      rf  left on the minus strand, right on the plus strand; either is mate 1
      ff  both on the plus strand with mate 1 left, or both on the minus strand with mate 2 left (every other fragment)
    Candidates as there: about half overlap the mate's locus, three in four on the strand on which the read matches."""

    def __init__(self, seed, sizes, L, made, qlen=(40, 100), wlen=(80, 250), sub=0.03):
        rng = np.random.default_rng(seed)
        self.targets = [np.asarray(random_ref(L + 37 * j, int(rng.integers(1 << 30)), 4), dtype=np.int8) for j in range(2)]
        nr = 2 * len(sizes)
        reads, rows = [], []
        for f, (n1, n2) in enumerate(sizes):
            t = int(rng.integers(2)); ins = int(rng.integers(150, 401)); s = int(rng.integers(0, len(self.targets[t]) - ins + 1))
            l1, l2 = (int(x) for x in rng.integers(qlen[0], qlen[1] + 1, size=2))
            coin = rng.random() < 0.5
            lrev, rrev = dict(fr=(False, True), rf=(True, False), ff=((True, True) if f % 2 else (False, False)))[made]
            lseq = _mut(self.targets[t][s:s + l1], rng, sub); rseq = _mut(self.targets[t][s + ins - l2:s + ins], rng, sub)
            left = (_revcomp(lseq) if lrev else lseq, s, lrev)                    # (read as stored, locus, matches as reverse complement)
            right = (_revcomp(rseq) if rrev else rseq, s + ins - l2, rrev)
            if made == "ff":
                mates = (right, left) if f % 2 else (left, right)
            else:
                mates = (left, right) if coin else (right, left)
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


@functools.lru_cache(maxsize=None)
def lib_case(seed, sizes, L, made):
    return LibCase(seed, list(sizes), L, made)


def sizes_of(seed, nfrag, extra=()):
    rng = np.random.default_rng(seed)
    return tuple(list(extra) + [(int(a), int(b)) for a, b in rng.integers(0, 6, size=(nfrag - len(extra), 2))])


def rule(a0, af, acig, case, min_score, mn, mx, pen, orient):
    """the header's rule with the orientation, over align_windows' records of all candidates (a0: flag 0, af: the caller's flag)
    -> (sel, records, pool)"""
    co = [int(x) for x in case.co]
    nf = (len(co) - 1) // 2
    s = [int(x) for x in a0["score1"]]
    ok = [int(st) == 0 and sc > 0 and sc >= min_score for st, sc in zip(a0["status"], s)]
    minus = [int(x) >= case.nfwd for x in case.q]
    ln = [len(case.reads[int(x)]) for x in case.q]
    E = [int(case.b[i]) + int(a0["ref_end1"][i]) for i in range(co[-1])]
    B = [E[i] - ln[i] + 1 for i in range(co[-1])]

    def proper(a, b):
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


def check(ctx, case, orient, mn, mx, pen, min_score=0, sample=None, mat=MAT, n=5, **kw):
    """align_windows_mates(orientation=orient) against oracle (a) for every fragment and oracle (b) for every chosen candidate (sample: that
    many, fixed seed) -> (sel, records, pool, align_windows' flag-0 records of all candidates)"""
    co = case.co
    nf = (len(co) - 1) // 2
    Q, T = case.upload(ctx)
    try:
        sel, res, cig = ctx.align_windows_mates(Q, T, co, case.q, case.t, case.b, case.l, case.nfwd, mat, n, mn, mx, pen, min_score=min_score,
                                                orientation=orient, **kw)
        kw0 = {k: v for k, v in kw.items() if k not in ("flag", "filters", "filterd", "mark_mismatch")}
        a0, _ = _all(ctx, case, Q, T, mat, n, flag=0, **kw0)
        af, acig = _all(ctx, case, Q, T, mat, n, **kw) if kw.get("flag", 0) or kw.get("mark_mismatch") else (a0, np.zeros(0, dtype=np.uint32))
    finally:
        Q.free(); T.free()
    esel, eres, ecig = rule(a0, af, acig, case, min_score, mn, mx, pen, orient)
    bad = []
    for f in np.nonzero((sel != esel) | (res != eres).any(axis=1))[0][:4]:
        bad.append("%s fragment %d (candidates [%d, %d) + [%d, %d)): expected %s %s, got %s %s" % (orient, f, co[2 * f], co[2 * f + 1], co[2 * f + 1],
                                                                                                    co[2 * f + 2], esel[f], eres[f], sel[f], res[f]))
    assert not bad, "\n".join(bad)
    assert sel.shape == (nf,) and res.shape == (nf, 2)
    assert sel.tobytes() == esel.tobytes()              # every field, the padding included
    assert (res == eres).all()                          # every field, cigar_off included
    assert cig.tobytes() == ecig.tobytes()
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    hit = pos >= 0
    flag = kw.get("flag", 0)
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
    return sel, res, cig, a0


def old_symbol(ctx, case, Q, T, mn, mx, pen, flag, min_score=0):
    """ssw_gpu_align_windows_mates, the symbol without an orientation, straight through the C ABI -> (sel, records, pool)"""
    nf = (len(case.co) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE); res = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE)
    pool = ssw_amd._u32p(); words = C.c_int64(0)
    rc = ctx.lib.ssw_gpu_align_windows_mates(ctx.h, Q.h, T.h, case.co.ctypes.data, nf, case.q.ctypes.data, case.t.ctypes.data, case.b.ctypes.data,
                                             case.l.ctypes.data, case.nfwd, C.byref(p), min_score, mn, mx, pen, sel.ctypes.data, res.ctypes.data,
                                             C.byref(pool), C.byref(words))
    assert rc == 0, ctx.error()
    cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if words.value > 0 else np.zeros(0, dtype=np.uint32)
    if pool:
        C.CDLL(None).free(pool)
    return sel, res, cig


# ------------------------------------------------------------------------------------------------------------- the cases

def _libraries(ctx, made, nfrag, L, sample=None):
    """1. fragments of one library under all three orientations: the orientation they were made as finds them proper, and the selection
    changes with the argument (a kernel that ignores it cannot pass); FR is the old symbol byte for byte"""
    case = lib_case(9700 + ORIENTS.index(made), sizes_of(9710, nfrag, ((1, 1), (2, 3), (4, 4), (3, 1))), L, made)
    got = {}
    for o in ORIENTS:
        for flag in (0, 2):
            sel, res, cig, _ = check(ctx, case, o, INS[0], INS[1], 30, sample=sample, flag=flag)
            got[o, flag] = (sel, res, cig)
        sel = got[o, 0][0]
        assert got[o, 2][0].tobytes() == sel.tobytes()      # sel does not depend on the flag
        both = (sel["pos1"] >= 0) & (sel["pos2"] >= 0)
        if o == made:
            assert (sel["proper"][both] == 1).any() and (sel["n_proper"] > 0).any()
    for o in ORIENTS:
        if o == made:
            continue
        a, b = got[made, 0][0], got[o, 0][0]
        assert ((a["pos1"] != b["pos1"]) | (a["pos2"] != b["pos2"])).any() and (a["proper"] != b["proper"]).any()
        assert int(a["n_proper"].sum()) > int(b["n_proper"].sum())
        for f in ("n_eligible1", "n_eligible2"):
            assert (a[f] == b[f]).all()
    for o in (0, 1, 2):      # the integer spelling of the argument
        Q, T = case.upload(ctx)
        try:
            s, r, c = ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, INS[0], INS[1], 30, flag=2, orientation=o)
            if o == 0:
                for flag in (0, 2):
                    so, ro, cg = old_symbol(ctx, case, Q, T, INS[0], INS[1], 30, flag)
                    sel, res, cig = got["fr", flag]
                    assert so.tobytes() == sel.tobytes() and (ro == res).all() and cg.tobytes() == cig.tobytes()
                s2, r2, c2 = ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, INS[0], INS[1], 30, flag=2)
                assert s2.tobytes() == s.tobytes() and (r2 == r).all() and c2.tobytes() == c.tobytes()      # the default is FR
        finally:
            Q.free(); T.free()
        sel, res, cig = got[ORIENTS[o], 2]
        assert s.tobytes() == sel.tobytes() and (r == res).all() and c.tobytes() == cig.tobytes()


def _grid(ctx, o, nfrag, L, sample=None):
    """2. every (n1, n2) of the grid in one call, then random small fragments up to nfrag"""
    case = lib_case(9720 + ORIENTS.index(o), sizes_of(9721, max(nfrag, len(GRID)), GRID), L, o)
    for flag in (0, 2):
        sel, _, _, _ = check(ctx, case, o, INS[0], INS[1], 30, sample=sample, flag=flag)
        sizes = np.diff(case.co)
        assert (sel["n_eligible1"] == sizes[0::2]).all() and (sel["n_eligible2"] == sizes[1::2]).all()      # min_score 0, ordinary windows
        assert (sel["proper"] == 1).any() and ((sel["proper"] == 0) & (sel["pos1"] >= 0) & (sel["pos2"] >= 0)).any()
        assert (sel["n_proper"] > 1).any() and ((sel["pos1"] < 0) != (sel["pos2"] < 0)).any()


def _counts(ctx, o, nfrag):
    """3. fragment counts on the row and workgroup edges"""
    case = lib_case(9730 + ORIENTS.index(o), sizes_of(9731 + nfrag, nfrag, ((2, 3),)), 3000, o)
    sel, _, _, _ = check(ctx, case, o, INS[0], INS[1], 30, flag=2)
    assert sel.shape == (nfrag,)


def _locus_case(o):
    """exact copies of known loci, so that E and B are known.  U = tg[1000:1060] in window [980, 1080): E = 1059, B = 1000; V =
    tg[1300:1350] in window [1280, 1380): E = 1349, B = 1300; U upstream of V: D = 1349 - 1000 + 1 = 350.  `over` hangs 10 residues over
    column 0 in window [0, 100): E = 49, B = -10; W = tg[200:250] in [180, 280): E = 249; D = 249 + 10 + 1 = 260 (a clamped B: 250).
    Fragments, with the strands the orientation asks for (a read on the minus strand is stored reverse-complemented and named nr + r):
      rf  0: mate 1 = U minus, mate 2 = V plus;  1: mate 1 = V plus, mate 2 = U minus (the same pair);  2: the plus mate upstream (U plus,
          V minus: an FR pair, D = E(p) - B(m) + 1 = 1059 - 1300 + 1 < 0);  3: over minus, W plus
      ff  0: U, V both plus, mate 1 = U;  1: both minus, mate 2 = U (upstream);  2: both plus, mate 1 = V (downstream: D < 0);  3: both minus,
          mate 1 = U (upstream: D < 0);  4: over, W both plus"""
    tg = np.asarray(random_ref(3000, 9200, 4), dtype=np.int8)
    rng = np.random.default_rng(9202)
    over = np.concatenate([rng.integers(0, 4, size=10, dtype=np.int8), tg[0:50]])
    U, V, W = tg[1000:1060].copy(), tg[1300:1350].copy(), tg[200:250].copy()
    wU, wV, wO, wW = (0, 980, 100), (0, 1280, 100), (0, 0, 100), (0, 180, 100)
    if o == "rf":
        frags = [((U, True, wU), (V, False, wV)), ((V, False, wV), (U, True, wU)), ((U, False, wU), (V, True, wV)), ((over, True, wO), (W, False, wW))]
    else:
        frags = [((U, False, wU), (V, False, wV)), ((V, True, wV), (U, True, wU)), ((V, False, wV), (U, False, wU)), ((U, True, wU), (V, True, wV)),
                 ((over, False, wO), (W, False, wW))]
    nr = 2 * len(frags)
    reads, rows = [], []
    for f, pair in enumerate(frags):
        for h, (seq, minus, w) in enumerate(pair):
            reads.append(_revcomp(seq) if minus else seq.copy())
            rows.append([(2 * f + h + (nr if minus else 0),) + w])
    return Case.explicit(reads, [tg], rows)


def _insert_edges(ctx):
    """4. D = min_insert - 1, min_insert, max_insert, max_insert + 1; the wrong order; B < 0 -- per orientation"""
    pen = 17
    for o, ends, full in (("rf", [[79, 69], [69, 79], [79, 69], [49, 69]], [220, 220, 220, 200]),
                          ("ff", [[79, 69], [69, 79], [69, 79], [79, 69], [49, 69]], [220, 220, 220, 220, 200])):
        case = _locus_case(o)
        nf = len(full)
        good = [1, 1] + [0] * (nf - 3)      # the fragments with D = 350; the last one has D = 260
        for (mn, mx), w350, w260 in (((351, 500), 0, 0), ((350, 500), 1, 0), ((100, 350), 1, 1), ((100, 349), 0, 1), ((260, 260), 0, 1),
                                     ((261, 349), 0, 0), ((250, 259), 0, 0), ((0, 1 << 30), 1, 1)):
            sel, _, _, a0 = check(ctx, case, o, mn, mx, pen, flag=2)
            assert [int(x) for x in a0["ref_end1"]] == [x for e in ends for x in e]      # E is what the docstring says
            want = [w350 * g for g in good] + [w260]
            assert [int(x) for x in sel["proper"]] == want and [int(x) for x in sel["n_proper"]] == want
            assert (sel["score"] == np.array(full) - pen * (1 - np.array(want))).all() and (sel["second_score"] == 0).all()
        for other in ORIENTS:      # under another orientation: the oracle's business; fragments 0 and 1 are no longer proper under FR
            sel, _, _, _ = check(ctx, case, other, 0, 1 << 30, pen, flag=0)
            if other == "fr":
                assert [int(x) for x in sel["proper"][:2]] == [0, 0]


def _penalties(ctx, nfrag, L, sample=None):
    """5. unpaired_penalty 0 and 65535"""
    for o in ("rf", "ff"):
        case = lib_case(9740 + ORIENTS.index(o), sizes_of(9741, nfrag, ((3, 4), (5, 5))), L, o)
        s0, _, _, _ = check(ctx, case, o, INS[0], INS[1], 0, sample=sample, flag=2)
        s1, _, _, _ = check(ctx, case, o, INS[0], INS[1], 65535, sample=sample, flag=2)
        both = (s1["pos1"] >= 0) & (s1["pos2"] >= 0)
        assert (s1["proper"][both & (s1["n_proper"] > 0)] == 1).all()      # no improper combination outranks a proper one at that price
        assert (s1["score"][both & (s1["n_proper"] == 0)] < 0).all() and (s0["score"] >= 0).all()


def _envelopes(ctx):
    """6. an empty window and gapO == gapE (every candidate on the fallback) inside fragments of an RF and an FF library"""
    tg = np.asarray(random_ref(3000, 9600, 4), dtype=np.int8)
    U, V = tg[300:400].copy(), tg[500:580].copy()
    for o in ("rf", "ff"):
        um, vm = (True, False) if o == "rf" else (False, False)
        reads = [_revcomp(U) if um else U, _revcomp(V) if vm else V] * 2
        nr = len(reads)
        q = [r + (nr if m else 0) for r, m in zip(range(nr), [um, vm] * 2)]
        rows = [[(q[0], 0, 77, 0), (q[0], 0, 250, 200)], [(q[1], 0, 450, 200), (q[1], 0, 77, 0)],       # empty windows beside the hits
                [(q[2], 0, 250, 200)], [(q[3], 0, 77, 0)]]                                             # mate 2 has an empty window only
        case = Case.explicit(reads, [tg], rows)
        for kw in (dict(flag=0), dict(flag=2), dict(flag=2, gapO=1, gapE=1)):
            sel, res, _, _ = check(ctx, case, o, 0, 5000, 40, **kw)
            assert [int(x) for x in sel["pos1"]] == [1, 0] and [int(x) for x in sel["pos2"]] == [0, -1]
            assert [int(x) for x in sel["proper"]] == [1, 0] and [int(x) for x in sel["score"]] == [360, 200]
            assert int(sel["n_eligible2"][1]) == 0


def _refused(ctx):
    """7. orientation 3 and -1: -1 with a message, nothing written, the context answers the next call"""
    case = _locus_case("rf")
    nf = (len(case.co) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    Q, T = case.upload(ctx)
    try:
        for o in (3, -1):
            for flag in (0, 2):
                p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
                sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
                out = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
                before = sel.tobytes() + out.tobytes()
                words = C.c_int64(5); pool = ssw_amd._u32p()
                rc = ctx.lib.ssw_gpu_align_windows_mates_lib(ctx.h, Q.h, T.h, case.co.ctypes.data, nf, case.q.ctypes.data, case.t.ctypes.data,
                                                             case.b.ctypes.data, case.l.ctypes.data, case.nfwd, C.byref(p), 0, 0, 500, 10, o,
                                                             sel.ctypes.data, out.ctypes.data, C.byref(pool), C.byref(words))
                assert rc == -1 and re.search(r"^align_windows_mates: orientation must be .*orientation = %d\)" % o, ctx.error()), ctx.error()
                assert words.value == 0 and not pool and sel.tobytes() + out.tobytes() == before
            with pytest.raises(RuntimeError, match="orientation must be"):
                ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, 0, 500, 10, orientation=o)
        with pytest.raises(ValueError):
            ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, 0, 500, 10, orientation="rr")
        s, _, _ = ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, 0, 500, 10, orientation="RF")
        assert [int(x) for x in s["proper"]] == [1, 1, 0, 1]
    finally:
        Q.free(); T.free()


# ---------------------------------------------------------------------------------------------------------------- emulator

E_L = 3000


@pytest.mark.parametrize("made", ORIENTS)
def test_emu_libraries_under_every_orientation(ectx, made):
    _libraries(ectx, made, 24, E_L)


@pytest.mark.parametrize("o", ORIENTS)
def test_emu_group_size_grid(ectx, o):
    _grid(ectx, o, len(GRID), E_L)


@pytest.mark.parametrize("nfrag", NFRAGS)
@pytest.mark.parametrize("o", ["rf", "ff"])
def test_emu_fragment_counts(ectx, o, nfrag):
    _counts(ectx, o, nfrag)


def test_emu_insert_edges(ectx):
    _insert_edges(ectx)


def test_emu_penalty_extremes(ectx):
    _penalties(ectx, 20, E_L)


def test_emu_out_of_envelope_candidates(ectx):
    _envelopes(ectx)


def test_emu_orientation_refused(ectx):
    _refused(ectx)


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NF, G_L = 2000, 100000


@pytest.mark.gpu
@pytest.mark.parametrize("made", ORIENTS)
def test_gpu_libraries_under_every_orientation(gpu_ctx, made):
    _libraries(gpu_ctx, made, G_NF, G_L, sample=400)


@pytest.mark.gpu
@pytest.mark.parametrize("o", ORIENTS)
def test_gpu_group_size_grid(gpu_ctx, o):
    _grid(gpu_ctx, o, 600, G_L, sample=400)


@pytest.mark.gpu
@pytest.mark.parametrize("nfrag", NFRAGS)
@pytest.mark.parametrize("o", ["rf", "ff"])
def test_gpu_fragment_counts(gpu_ctx, o, nfrag):
    _counts(gpu_ctx, o, nfrag)


@pytest.mark.gpu
def test_gpu_insert_edges(gpu_ctx):
    _insert_edges(gpu_ctx)


@pytest.mark.gpu
def test_gpu_penalty_extremes(gpu_ctx):
    _penalties(gpu_ctx, 600, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_out_of_envelope_candidates(gpu_ctx):
    _envelopes(gpu_ctx)


@pytest.mark.gpu
def test_gpu_orientation_refused(gpu_ctx):
    _refused(gpu_ctx)
