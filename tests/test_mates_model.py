"""ssw_gpu_align_windows_mates_model: the pair model's insert-size penalty table (include/ssw_gpu.h, ssw_gpu_pair_model).

Everything is ssw_gpu_align_windows_mates_lib's but the score of a combination (a of mate 1, b of mate 2):
  S(a, b) = score1(a) + score1(b) - (proper ? insert_penalty[D - min_insert] : unpaired_penalty)
with D the span the orientation table defines (tests/test_mates_orient.py).  The table is used as given: no clamping against
unpaired_penalty.  With a NULL or an all-zero table the answer is ssw_gpu_align_windows_mates_lib's, bit for bit.

Two oracles, no fragment left out, as in tests/test_windows_mates.py and tests/test_mates_orient.py (whose cases, sizes and helpers are
reused): (a) Context.align_windows over ALL candidates and then the rule above in plain Python integers -- every field of `sel`, every record
field and the pool words; (b) the reference through parity.expected() on the cut-out window of every chosen candidate (all of them on the
emulator, a fixed-seed sample of 400 on the GPU).  Every case runs on the CPU SIMT emulator at the small size and, marked gpu, on the MI355X
through the same helper."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, random_ref
from test_mates_orient import GRID, NFRAGS, ORIENTS, lib_case, sizes_of
from test_windows_mates import MAT, Case, _all, _case, _cig, _revcomp, _sizes

INS = (100, 500)
TABLE_MAX = 65536      # SSW_GPU_INSERT_TABLE_MAX (include/ssw_gpu.h)
KWS = (dict(flag=0), dict(flag=2), dict(flag=2, mark_mismatch=True))


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def stepped(n):
    """a table whose neighbouring entries all differ"""
    return (1 + (7 * np.arange(n, dtype=np.int64)) % 13).astype(np.uint16)


def rule(a0, af, acig, case, min_score, mn, mx, pen, orient, table):
    """the header's rule under the pair model, over align_windows' records of all candidates (a0: flag 0, af: the caller's flag), in Python
    integers -> (sel, records, pool, span of the chosen combination per fragment or None)"""
    co = [int(x) for x in case.co]
    nf = (len(co) - 1) // 2
    tab = None if table is None else [int(x) for x in table]
    s = [int(x) for x in a0["score1"]]
    ok = [int(st) == 0 and sc > 0 and sc >= min_score for st, sc in zip(a0["status"], s)]
    minus = [int(x) >= case.nfwd for x in case.q]
    ln = [len(case.reads[int(x)]) for x in case.q]
    E = [int(case.b[i]) + int(a0["ref_end1"][i]) for i in range(co[-1])]
    B = [E[i] - ln[i] + 1 for i in range(co[-1])]

    def span(a, b):      # D, or None where target or strands rule the combination out
        if int(case.t[a]) != int(case.t[b]):
            return None
        if orient == "ff":
            if minus[a] != minus[b]:
                return None
            return E[a] - B[b] + 1 if minus[a] else E[b] - B[a] + 1
        if minus[a] == minus[b]:
            return None
        p, m = (b, a) if minus[a] else (a, b)
        return E[m] - B[p] + 1 if orient == "fr" else E[p] - B[m] + 1

    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE)
    res = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE)
    res["ref_begin1"] = -1; res["read_begin1"] = -1; res["cigar_off"] = -1
    spans = [None] * nf
    for f in range(nf):
        c0, c1, c2 = co[2 * f], co[2 * f + 1], co[2 * f + 2]
        e1 = [i for i in range(c0, c1) if ok[i]]; e2 = [i for i in range(c1, c2) if ok[i]]
        pos1 = pos2 = -1; score = second = npr = pr = 0
        if e1 and e2:
            comb = []
            for a in e1:
                for b in e2:
                    d = span(a, b)
                    p = d is not None and mn <= d <= mx
                    npr += p
                    cost = (tab[d - mn] if tab is not None else 0) if p else pen
                    comb.append((-(s[a] + s[b] - cost), a - c0, b - c1, p, d))
            comb.sort(key=lambda x: x[:3])
            pos1, pos2, score, pr = comb[0][1], comb[0][2], -comb[0][0], int(comb[0][3])
            spans[f] = comb[0][4]
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
    return sel, res, np.ascontiguousarray(pool, dtype=np.uint32), spans


def check(ctx, case, orient, mn, mx, pen, table, min_score=0, sample=None, mat=MAT, n=5, **kw):
    """align_windows_mates(insert_penalty=table) against oracle (a) for every fragment and oracle (b) for every chosen candidate (sample: that
    many, fixed seed) -> (sel, records, pool, align_windows' flag-0 records of all candidates, spans of the chosen combinations)"""
    co = case.co
    nf = (len(co) - 1) // 2
    Q, T = case.upload(ctx)
    try:
        sel, res, cig = ctx.align_windows_mates(Q, T, co, case.q, case.t, case.b, case.l, case.nfwd, mat, n, mn, mx, pen, min_score=min_score,
                                                orientation=orient, insert_penalty=table, **kw)
        kw0 = {k: v for k, v in kw.items() if k not in ("flag", "filters", "filterd", "mark_mismatch")}
        a0, _ = _all(ctx, case, Q, T, mat, n, flag=0, **kw0)
        af, acig = _all(ctx, case, Q, T, mat, n, **kw) if kw.get("flag", 0) or kw.get("mark_mismatch") else (a0, np.zeros(0, dtype=np.uint32))
    finally:
        Q.free(); T.free()
    esel, eres, ecig, spans = rule(a0, af, acig, case, min_score, mn, mx, pen, orient, table)
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
    flag = kw.get("flag", 0)
    if not kw.get("mark_mismatch", False):
        slots = np.argwhere(pos >= 0)
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
    return sel, res, cig, a0, spans


def model_symbol(ctx, case, Q, T, mn, mx, pen, o, table, flag=0, mark=False, min_score=0, null_model=False, sel=None, res=None, words=None,
                 **change):
    """ssw_gpu_align_windows_mates_model straight through the C ABI (table None: a NULL insert_penalty) -> (rc, sel, records, pool)"""
    nf = (len(case.co) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    p = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 1 if mark else 0)
    sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE) if sel is None else sel
    res = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE) if res is None else res
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint16)
    pm = ssw_amd.PairModel(mn, mx, pen, o, tab.ctypes.data_as(C.POINTER(C.c_uint16)) if tab is not None else None)
    pool = ssw_amd._u32p(); words = C.c_int64(0) if words is None else words
    a = dict(co=case.co, q=case.q, t=case.t, b=case.b, l=case.l, nfrag=nf, nfwd=case.nfwd, queries=Q)
    a.update(change)
    rc = ctx.lib.ssw_gpu_align_windows_mates_model(ctx.h, a["queries"].h, T.h, a["co"].ctypes.data, a["nfrag"], a["q"].ctypes.data, a["t"].ctypes.data,
                                                   a["b"].ctypes.data, a["l"].ctypes.data, a["nfwd"], C.byref(p), min_score,
                                                   None if null_model else C.byref(pm), sel.ctypes.data, res.ctypes.data, C.byref(pool), C.byref(words))
    cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if rc == 0 and words.value > 0 else np.zeros(0, dtype=np.uint32)
    if pool:
        assert rc == 0
        C.CDLL(None).free(pool)
    return rc, sel, res, cig


# ------------------------------------------------------------------------------------------------------------- the cases

def _flat(ctx, case, o, kws=KWS):
    """a NULL table (the C ABI), an all-zero table (the keyword) and the _lib call: sel, records and pool bytes equal"""
    mn, mx = INS
    oi = ORIENTS.index(o)
    Q, T = case.upload(ctx)
    try:
        for kw in kws:
            a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, mn, mx, 30)
            sel, res, cig = ctx.align_windows_mates(*a, orientation=o, **kw)
            z = ctx.align_windows_mates(*a, orientation=o, insert_penalty=np.zeros(mx - mn + 1, dtype=np.int64), **kw)
            rc, nsel, nres, ncig = model_symbol(ctx, case, Q, T, mn, mx, 30, oi, None, flag=kw["flag"], mark=kw.get("mark_mismatch", False))
            assert rc == 0, ctx.error()
            for s, r, c in (z, (nsel, nres, ncig)):
                assert s.tobytes() == sel.tobytes() and (r == res).all() and r.tobytes() == res.tobytes() and c.tobytes() == cig.tobytes()
    finally:
        Q.free(); T.free()
    return sel


def _flat_grid(ctx, o, nfrag, L):
    """1. flat equivalence over the grid of group sizes"""
    sel = _flat(ctx, lib_case(9720 + ORIENTS.index(o), sizes_of(9721, max(nfrag, len(GRID)), GRID), L, o), o)
    assert (sel["proper"] == 1).any() and (sel["n_proper"] > 1).any()


def _flat_counts(ctx, o, nfrag):
    """1. flat equivalence on the row and workgroup edges of the fragment count"""
    _flat(ctx, lib_case(9730 + ORIENTS.index(o), sizes_of(9731 + nfrag, nfrag, ((2, 3),)), 3000, o), o, kws=KWS[:2])


def span_case(o, spans, L=3000, step=400):
    """exact copies of known loci, one fragment per span D: the upstream read U = tg[s : s + 50] and the downstream read V =
    tg[s + D - 50 : s + D], each in a window with 20 columns of margin, so that B(U) = s, E(V) = s + D - 1 and the span is D.  Strands and
    mate order as the orientation asks: fr U plus, V minus; rf U minus, V plus; ff both plus with mate 1 = U (even fragments), both minus
    with mate 2 = U (odd ones).  FR and RF: U is mate 1 in even, mate 2 in odd fragments."""
    tg = np.asarray(random_ref(L, 9900, 4), dtype=np.int8)
    nr = 2 * len(spans)
    reads, rows = [], []
    for f, D in enumerate(spans):
        s = 100 + step * f
        assert D >= 50 and s + D + 20 <= L
        U = (tg[s:s + 50].copy(), s - 20, 90); V = (tg[s + D - 50:s + D].copy(), s + D - 70, 90)
        um, vm = dict(fr=(False, True), rf=(True, False), ff=((True, True) if f % 2 else (False, False)))[o]
        pair = ((U, um), (V, vm))
        if f % 2:
            pair = pair[::-1]
        for h, ((seq, wb, wl), minus) in enumerate(pair):
            reads.append(_revcomp(seq) if minus else seq)
            rows.append([(2 * f + h + (nr if minus else 0), 0, wb, wl)])
    return Case.explicit(reads, [tg], rows)


def _index_edges(ctx):
    """2. D = mn - 1, mn, mn + 1, mx - 1, mx, mx + 1 per orientation against a table whose neighbours differ; mn == mx; 65536 entries"""
    pen = 17
    for o in ORIENTS:
        mn, mx = 200, 300
        spans = [mn - 1, mn, mn + 1, mx - 1, mx, mx + 1]
        case = span_case(o, spans)
        table = stepped(mx - mn + 1)
        for flag in (0, 2):
            sel, _, _, a0, got = check(ctx, case, o, mn, mx, pen, table, flag=flag)
            assert got == spans and (a0["score1"] == 100).all()      # E and B are what span_case says
            want = [200 - (int(table[D - mn]) if mn <= D <= mx else pen) for D in spans]
            assert [int(x) for x in sel["score"]] == want and [int(x) for x in sel["proper"]] == [0, 1, 1, 1, 1, 0]
            assert [int(x) for x in sel["n_proper"]] == [0, 1, 1, 1, 1, 0] and (sel["second_score"] == 0).all()
        assert len(set(want[1:5])) == 4      # (the four proper spans pay four different entries: an index off by one cannot pass)
        # mn == mx: a table of one entry
        sel, _, _, _, _ = check(ctx, case, o, mx, mx, pen, np.array([9], dtype=np.uint16), flag=2)
        assert [int(x) for x in sel["score"]] == [183, 183, 183, 183, 191, 183] and [int(x) for x in sel["proper"]] == [0, 0, 0, 0, 1, 0]
    # a table of exactly SSW_GPU_INSERT_TABLE_MAX entries, D at its first and its last index and one past it
    mn, mx = 100, 100 + TABLE_MAX - 1
    table = stepped(TABLE_MAX)
    table[-1] = 40000; table[-2] = 3; table[0] = 11; table[1] = 5
    spans = [mx, mx + 1, mn, mx - 1]
    for o in ORIENTS:
        case = span_case(o, spans, L=4 * 100 + TABLE_MAX + 300, step=100)
        sel, _, _, _, got = check(ctx, case, o, mn, mx, pen, table, flag=0)
        assert got == spans
        assert [int(x) for x in sel["score"]] == [200 - 40000, 200 - pen, 200 - 11, 200 - 3] and [int(x) for x in sel["proper"]] == [1, 0, 1, 1]


def decide_case():
    """FR fragments in which the model and the flat rule disagree; mate 1 is U = tg[s : s + 50] on the plus strand, mate 2 has two candidates
    on the minus strand, min_insert 100, max_insert 500:
      0  tandem copies: V's 50 columns stand at span 490 (candidate 0) and at span 300 (candidate 1) -- equal scores
      1  V exact at span 490 (candidate 0); a copy with two substitutions at span 300 (candidate 1): a lower sum at the mode
      2  V at span 300 (candidate 0, proper) and a copy at span 650 (candidate 1, improper): equal scores"""
    tg = np.asarray(random_ref(4000, 9910, 4), dtype=np.int8).copy()
    rows, reads = [], []
    nr = 6

    def put(f, s, dv, copy_at, subs=()):
        V = tg[s + dv - 50:s + dv].copy()
        c = V.copy()
        for k in subs:
            c[k] = (c[k] + 1) % 4
        tg[s + copy_at - 50:s + copy_at] = c
        return V

    def win(s, D):
        return (0, s + D - 60, 70)

    V0 = put(0, 100, 300, 490)
    V1 = put(1, 1100, 490, 300, subs=(20, 30))
    V2 = put(2, 2100, 300, 650)
    for f, (s, V, spans) in enumerate(((100, V0, (490, 300)), (1100, V1, (490, 300)), (2100, V2, (300, 650)))):
        reads += [tg[s:s + 50].copy(), _revcomp(V)]
        rows += [[(2 * f, 0, s - 10, 70)], [(nr + 2 * f + 1,) + win(s, D) for D in spans]]
    return Case.explicit(reads, [tg], rows)


def _decides(ctx):
    """3. the model decides where the flat rule has a position tie-break or a raw sum"""
    case = decide_case()
    mn, mx, pen = INS[0], INS[1], 17
    normal = ssw_amd.insert_penalty_normal(300, 50, mn, mx, 2, 17)
    assert normal[300 - mn] == 0 and normal[490 - mn] >= 9
    steep = np.zeros(mx - mn + 1, dtype=np.uint16); steep[300 - mn] = 30      # above unpaired_penalty
    for flag in (0, 2):
        flat, _, _, a0, _ = check(ctx, case, "fr", mn, mx, pen, None, flag=flag)
        s = [int(x) for x in a0["score1"]]
        assert s[1] == s[2] == 100 and s[4] == 100 and s[5] == 92 and s[7] == s[8] == 100
        mod, _, _, _, spans = check(ctx, case, "fr", mn, mx, pen, normal, flag=flag)
        # (i) tandem copies: the flat rule takes the lower position, the model the likelier span
        assert (int(flat["pos2"][0]), int(flat["score"][0]), int(flat["second_score"][0])) == (0, 200, 200)
        assert (int(mod["pos2"][0]), int(mod["score"][0]), int(mod["second_score"][0])) == (1, 200, 200 - int(normal[490 - mn])) and spans[0] == 300
        # (ii) the higher raw sum at a heavily penalised span loses to the lower sum at the mode
        assert (int(flat["pos2"][1]), int(flat["score"][1])) == (0, 200)
        assert (int(mod["pos2"][1]), int(mod["score"][1]), int(mod["second_score"][1])) == (1, 192, 200 - int(normal[490 - mn]))
        assert (mod["proper"] == 1).all() and (flat["proper"] == 1).all() and [int(x) for x in mod["n_proper"]] == [2, 2, 1]
        # (iii) an entry above unpaired_penalty: the proper combination ranks below the improper one of equal sum; properness as defined
        assert (int(flat["pos2"][2]), int(flat["score"][2]), int(flat["proper"][2])) == (0, 200, 1)
        st, _, _, _, _ = check(ctx, case, "fr", mn, mx, pen, steep, flag=flag)
        assert (int(st["pos2"][2]), int(st["score"][2]), int(st["second_score"][2]), int(st["proper"][2]), int(st["n_proper"][2])) == (1, 183, 170, 0, 1)


def _signed(ctx):
    """4. entries and unpaired_penalty at 65535, small alignment scores: negative and exact; second_score == 0 only without a second combination"""
    case = decide_case()
    mn, mx = INS
    table = np.full(mx - mn + 1, 65535, dtype=np.uint16)
    sel, _, _, _, _ = check(ctx, case, "fr", mn, mx, 65535, table, flag=2)
    assert [int(x) for x in sel["score"]] == [200 - 65535, 200 - 65535, 200 - 65535]
    assert [int(x) for x in sel["second_score"]] == [200 - 65535, 192 - 65535, 200 - 65535] and [int(x) for x in sel["pos2"]] == [0, 0, 0]
    one = span_case("fr", [300, 700])      # one combination per fragment: a proper and an improper one
    sel, _, _, _, _ = check(ctx, one, "fr", mn, mx, 65535, table, flag=0)
    assert [int(x) for x in sel["score"]] == [200 - 65535] * 2 and (sel["second_score"] == 0).all() and [int(x) for x in sel["proper"]] == [1, 0]


def _random_tables(ctx, nfrag, L, sample=None):
    """5. random lists, random tables: entries 0 .. 40, then {0, 65535}; min_score 0 and 30; group sizes from 0"""
    mn, mx = INS
    rng = np.random.default_rng(9920)
    tables = (rng.integers(0, 41, size=mx - mn + 1).astype(np.uint16), (rng.integers(0, 2, size=mx - mn + 1) * 65535).astype(np.uint16))
    extra = ((0, 3), (1, 1), (1, 0), (0, 0), (4, 4), (0, 1), (5, 1))
    cases = [("fr", _case(9921, _sizes(9922, nfrag, extra), L))] + [(o, lib_case(9923 + i, sizes_of(9926, nfrag, extra), L, o)) for i, o in enumerate(ORIENTS)]
    differs = 0
    for o, case in cases:
        for min_score, flag in ((0, 2), (30, 0)):
            flat, _, _, _, _ = check(ctx, case, o, mn, mx, 30, None, min_score=min_score, sample=sample, flag=flag)
            for table in tables:
                sel, _, _, _, _ = check(ctx, case, o, mn, mx, 30, table, min_score=min_score, sample=sample, flag=flag)
                differs += int(((sel["pos1"] != flat["pos1"]) | (sel["pos2"] != flat["pos2"]) | (sel["score"] != flat["score"])).sum())
                one = (sel["pos1"] < 0) != (sel["pos2"] < 0)      # the one-mate and no-mate paths do not see the table
                assert one.any() and sel[one].tobytes() == flat[one].tobytes() and (sel["n_proper"] == flat["n_proper"]).all()
    assert differs > 0


def _fallback_mix(ctx):
    """6. an empty window and gapO == gapE (every candidate on the fallback) beside ordinary candidates, under the model"""
    tg = np.asarray(random_ref(3000, 9600, 4), dtype=np.int8)
    U, V = tg[300:400].copy(), tg[500:580].copy()
    table = stepped(5001)
    for o in ORIENTS:
        um, vm = dict(fr=(False, True), rf=(True, False), ff=(False, False))[o]
        reads = [_revcomp(U) if um else U, _revcomp(V) if vm else V] * 2
        nr = len(reads)
        q = [r + (nr if m else 0) for r, m in zip(range(nr), [um, vm] * 2)]
        rows = [[(q[0], 0, 77, 0), (q[0], 0, 250, 200)], [(q[1], 0, 450, 200), (q[1], 0, 77, 0)],       # empty windows beside the hits
                [(q[2], 0, 250, 200)], [(q[3], 0, 77, 0)]]                                             # mate 2 has an empty window only
        case = Case.explicit(reads, [tg], rows)
        for kw in (dict(flag=0), dict(flag=2), dict(flag=2, gapO=1, gapE=1)):
            sel, _, _, _, spans = check(ctx, case, o, 0, 5000, 40, table, **kw)
            assert [int(x) for x in sel["pos1"]] == [1, 0] and [int(x) for x in sel["pos2"]] == [0, -1] and spans[0] == 280
            assert [int(x) for x in sel["proper"]] == [1, 0] and [int(x) for x in sel["score"]] == [360 - int(table[280]), 200]


def _errors(ctx, other_ctx):
    """7. refused calls: -1, a message that names the problem, the caller's arrays untouched, the context usable afterwards"""
    reads = [random_ref(30, 1, 4), random_ref(30, 4, 4)]; targets = [random_ref(40, 2, 4), random_ref(55, 3, 4)]
    case = Case.explicit(reads, targets, [[(0, 0, 0, 40), (0, 1, 5, 50)], [(3, 0, 10, 30)]])
    Q, T = case.upload(ctx); Qo = other_ctx.upload(reads)
    table = stepped(501)

    def refused(what, mn=0, mx=500, pen=10, o=0, tab=table, **change):
        for flag in (0, 2):
            sel = np.zeros(1, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
            out = np.zeros((1, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
            before = sel.tobytes() + out.tobytes()      # (arrays of the caller: every byte, padding included, must stay)
            words = C.c_int64(5)
            ch = {k: (np.ascontiguousarray(v[0], dtype=v[1]) if isinstance(v, tuple) else v) for k, v in change.items()}
            rc, _, _, _ = model_symbol(ctx, case, Q, T, mn, mx, pen, o, tab, flag=flag, sel=sel, res=out, words=words, **ch)
            assert rc == -1 and re.search(what, ctx.error()), ctx.error()
            assert words.value == 0 and sel.tobytes() + out.tobytes() == before
            s2, _, _, _, _ = check(ctx, case, "fr", 0, 500, 10, table, flag=flag)      # the context answers the next call
            assert int(s2["n_eligible1"][0]) == 2
    try:
        refused(r"^align_windows_mates_model: NULL argument \(model\)", null_model=True)
        refused(r"^align_windows_mates_model: insert_penalty covers more than 65536 spans \(min_insert = 0, max_insert = 65536: 65537 entries\)",
                mx=TABLE_MAX, tab=stepped(TABLE_MAX + 1))
        refused(r"^align_windows_mates_model: cand_off\[0\] must be 0.*fragment 0", co=([1, 2, 3], np.int64))
        refused(r"^align_windows_mates_model: cand_off decreases.*fragment 0, mate 2", co=([0, 4, 3], np.int64))
        refused(r"^align_windows_mates_model: window out of range.*pair 2\b", l=([40, 50, 31], np.int32))
        refused(r"^align_windows_mates_model: index out of range.*pair 1\b", t=([0, 2, 0], np.int32))
        refused(r"nfwd outside.*nfwd = 5", nfwd=5)
        refused(r"nfwd outside.*nfwd = -1", nfwd=-1)
        refused(r"min_insert <= max_insert.*min_insert = -1", mn=-1, tab=stepped(502))
        refused(r"min_insert <= max_insert.*min_insert = 501", mn=501)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= -1", pen=-1)
        refused(r"unpaired_penalty must be 0 \.\. 65535.*= 65536", pen=65536)
        refused(r"orientation must be .*orientation = 3\)", o=3)
        refused("another context", queries=Qo)
        refused(r"more than 4096 candidates in a group.*fragment 0, mate 1", co=([0, 4097, 4098], np.int64))
        refused(r"more than 2\^31 output slots", nfrag=0x7fffff00 // 2 + 1)
        # a NULL table keeps the range unlimited, as ssw_gpu_align_windows_mates_lib
        rc, sel, _, _ = model_symbol(ctx, case, Q, T, 0, 1 << 30, 10, 0, None)
        assert rc == 0 and int(sel["n_eligible1"][0]) == 2
        # no fragments
        words = C.c_int64(5)
        rc, _, _, _ = model_symbol(ctx, case, Q, T, 0, 500, 10, 0, table, words=words, nfrag=0)
        assert rc == 0 and words.value == 0
        # the keyword's own checks: before the call
        a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, 0, 500, 10)
        for bad, what in ((stepped(500), "501 entries, not 500"), (stepped(502), "501 entries"), (np.full(501, 65536), r"0 \.\. 65535"),
                          (np.full(501, -1), r"0 \.\. 65535"), (np.zeros(501, dtype=np.float64), "1-D integer"), (np.zeros((501, 1), dtype=np.int32), "1-D integer")):
            with pytest.raises(ValueError, match=what):
                ctx.align_windows_mates(*a, insert_penalty=bad)
            with pytest.raises(ValueError, match=what):
                ctx.align_windows_mates_rescue(*a[:8], np.arange(2, dtype=np.int32), *a[8:], insert_penalty=bad)
        with pytest.raises(RuntimeError, match="insert_penalty covers more than 65536 spans"):
            ctx.align_windows_mates(*a[:10], 0, TABLE_MAX, 10, insert_penalty=stepped(TABLE_MAX + 1))
        s, _, _ = ctx.align_windows_mates(*a, insert_penalty=[int(x) for x in table])      # a list of Python integers is an integer array
        assert int(s["n_eligible1"][0]) == 2
    finally:
        Q.free(); T.free(); Qo.free()


# ---------------------------------------------------------------------------------------------------------------- the helper

def test_insert_penalty_normal():
    mean, sd, mn, mx, match, cap = 450, 75, 100, 1000, 2, 17
    t = ssw_amd.insert_penalty_normal(mean, sd, mn, mx, match, cap)
    assert t.dtype == np.uint16 and t.shape == (mx - mn + 1,) and t.flags["C_CONTIGUOUS"]
    assert t[mean - mn] == 0
    k = min(mean - mn, mx - mean)
    assert (t[mean - mn - k:mean - mn] == t[mean - mn + k:mean - mn:-1]).all()      # symmetric about the mean
    assert (np.diff(t[mean - mn:].astype(np.int64)) >= 0).all() and (np.diff(t[:mean - mn + 1].astype(np.int64)) <= 0).all()
    assert int(t.max()) == cap and t[0] == cap and t[-1] == cap
    # one entry by hand: D = 600, |D - mean| / (sd sqrt 2) = 150 / 106.066... = 1.41421...; erfc(sqrt 2) = 0.0455002638...;
    # -ln = 3.09004...; x 0.721 x 2 = 4.4558...; + 0.5, floor: 4
    assert t[600 - mn] == 4 and int(math.floor(0.721 * 2 * -math.log(math.erfc(math.sqrt(2.0))) + 0.5)) == 4
    # where erfc underflows the entry is the cap; a cap above every entry changes nothing below it
    far = ssw_amd.insert_penalty_normal(100, 1, 100, 200, 2, 60000)
    assert far[0] == 0 and far[-1] == 60000 and math.erfc(100 / math.sqrt(2.0)) == 0.0 and (np.diff(far.astype(np.int64)) >= 0).all()
    assert far[3] == int(math.floor(0.721 * 2 * -math.log(math.erfc(3 / math.sqrt(2.0))) + 0.5)) == 9
    one = ssw_amd.insert_penalty_normal(300, 50, 300, 300, 2, 17)
    assert one.shape == (1,) and one[0] == 0


# ---------------------------------------------------------------------------------------------------------------- emulator

E_L = 3000


@pytest.mark.parametrize("o", ORIENTS)
def test_emu_flat_equivalence_grid(ectx, o):
    _flat_grid(ectx, o, len(GRID), E_L)


@pytest.mark.parametrize("nfrag", NFRAGS)
@pytest.mark.parametrize("o", ORIENTS)
def test_emu_flat_equivalence_counts(ectx, o, nfrag):
    _flat_counts(ectx, o, nfrag)


def test_emu_index_edges(ectx):
    _index_edges(ectx)


def test_emu_model_decides(ectx):
    _decides(ectx)


def test_emu_signed_scores(ectx):
    _signed(ectx)


def test_emu_random_tables(ectx):
    _random_tables(ectx, 14, E_L)


def test_emu_fallback_mix(ectx):
    _fallback_mix(ectx)


def test_emu_errors(ectx, emu_lib_path):
    other = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    try:
        _errors(ectx, other)
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NF, G_L = 2000, 100000


@pytest.mark.gpu
@pytest.mark.parametrize("o", ORIENTS)
def test_gpu_flat_equivalence_grid(gpu_ctx, o):
    _flat_grid(gpu_ctx, o, 600, G_L)


@pytest.mark.gpu
@pytest.mark.parametrize("nfrag", NFRAGS)
@pytest.mark.parametrize("o", ORIENTS)
def test_gpu_flat_equivalence_counts(gpu_ctx, o, nfrag):
    _flat_counts(gpu_ctx, o, nfrag)


@pytest.mark.gpu
def test_gpu_index_edges(gpu_ctx):
    _index_edges(gpu_ctx)


@pytest.mark.gpu
def test_gpu_model_decides(gpu_ctx):
    _decides(gpu_ctx)


@pytest.mark.gpu
def test_gpu_signed_scores(gpu_ctx):
    _signed(gpu_ctx)


@pytest.mark.gpu
def test_gpu_random_tables(gpu_ctx):
    _random_tables(gpu_ctx, G_NF, G_L, sample=400)


@pytest.mark.gpu
def test_gpu_fallback_mix(gpu_ctx):
    _fallback_mix(gpu_ctx)


@pytest.mark.gpu
def test_gpu_errors(gpu_ctx, product_lib_path):
    other = ssw_amd.Context(0, ssw_amd.load(product_lib_path))
    try:
        _errors(gpu_ctx, other)
    finally:
        other.close()
