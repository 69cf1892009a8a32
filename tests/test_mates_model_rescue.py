"""ssw_gpu_align_windows_mates_rescue_model: mate rescue under the pair model (include/ssw_gpu.h, ssw_gpu_pair_model).

The rescue rule -- anchors, the "already has a proper partner" test, the window formulas, clipping -- does not look at the penalty table:
the slot table is the flat rescue call's.  Only the final selection over the AUGMENTED list does, and its answer is bit for bit
ssw_gpu_align_windows_mates_model's over the list that tests/test_mates_rescue.py's _augment builds in Python integers: sel, records,
origin and pool.  Oracle (b), the reference on the cut-out window of every chosen RESCUE candidate, as there.  Every case runs on the CPU
SIMT emulator at the small size and, marked gpu, on the MI355X through the same helper."""
import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, random_ref
from test_mates_rescue import INS, PAD, _augment, _case
from test_windows_mates import MAT, Case, _all, _cig, _revcomp


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


def check(ctx, case, table, orient="fr", A=2, ams=0, pad=PAD, mn=INS[0], mx=INS[1], pen=17, min_score=0, sample=None, **kw):
    """align_windows_mates_rescue(insert_penalty=table) against align_windows_mates(insert_penalty=table) over the augmented list of
    _augment, the flat rescue call's slot table, and the reference for every chosen rescue candidate
    -> (sel, records, origin, timing, (sel, records, origin, pool) of the FLAT rescue call)"""
    co = case.co
    nf = (len(co) - 1) // 2
    Q, T = case.upload(ctx)
    try:
        a = (Q, T, co, case.q, case.t, case.b, case.l, case.nfwd)
        r = dict(max_anchors=A, anchor_min_score=ams, rescue_pad=pad, min_score=min_score, orientation=orient)
        sel, res, org, cig = ctx.align_windows_mates_rescue(*a, case.mate_q, MAT, 5, mn, mx, pen, insert_penalty=table, **r, **kw)
        tm = ctx.timing()
        flat = ctx.align_windows_mates_rescue(*a, case.mate_q, MAT, 5, mn, mx, pen, **r, **kw)
        tmf = ctx.timing()
        a0, _ = _all(ctx, case, Q, T, MAT, 5, flag=0)
        aco, aq, at, ab, al, anchors, filled = _augment(a0, case, orient, A, ams, pad, mn, mx, min_score)
        esel, eres, ecig = ctx.align_windows_mates(Q, T, aco, aq, at, ab, al, case.nfwd, MAT, 5, mn, mx, pen, min_score=min_score, orientation=orient,
                                                   insert_penalty=table, **kw)
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
    # the slot table: the rule's (which has no table), and the flat call's
    assert tm["rescue_windows"] == filled == tmf["rescue_windows"] and tm["fill_cells"] == tmf["fill_cells"]
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    size = np.diff(co).reshape(nf, 2)
    eorg = np.zeros((nf, 2), dtype=ssw_amd.RESCUED_DTYPE)
    eorg["tidx"] = -1; eorg["qidx"] = -1; eorg["anchor"] = -1
    for f, h in np.argwhere(pos >= 0):
        i = int(aco[2 * f + h]) + int(pos[f, h])
        eorg[f, h] = (ab[i], al[i], at[i], aq[i], anchors[2 * f + h][pos[f, h] - size[f, h]] if pos[f, h] >= size[f, h] else -1)
    assert org.tobytes() == eorg.tobytes()
    fsel, fres, forg, _ = flat
    fpos = np.stack([fsel["pos1"], fsel["pos2"]], axis=1)
    eq = pos == fpos      # the same position of the same augmented list: the same window, query and anchor
    assert org[eq].tobytes() == forg[eq].tobytes()
    assert (fsel["n_eligible1"] == sel["n_eligible1"]).all() and (fsel["n_eligible2"] == sel["n_eligible2"]).all() and (fsel["n_proper"] == sel["n_proper"]).all()
    if not kw.get("mark_mismatch", False):
        slots = np.argwhere(pos >= size)
        if sample is not None and len(slots) > sample:
            slots = slots[np.random.default_rng(5).choice(len(slots), size=sample, replace=False)]
        for f, h in slots:
            o = org[f, h]
            rd = case.reads[int(o["qidx"])]
            rf = np.ascontiguousarray(case.targets[int(o["tidx"])][int(o["tbeg"]):int(o["tbeg"]) + int(o["tlen"])])
            exp, xcig = expected(rd, MAT, 5, rf, 3, 1, kw.get("flag", 0), 0, 0, len(rd) // 2, 2)
            rec = res[f, h]
            ok = exp is not None and int(rec["status"]) == 0 and {x: int(rec[x]) for x in RES_FIELDS} == exp and _cig(rec, cig) == xcig
            if not ok and len(bad) < 4:
                bad.append("fragment %d mate %d rescue window (len %d x %d): expected %s %s got %s" % (f, h + 1, len(rd), len(rf), exp, cigar_str(xcig), rec))
        assert not bad, "\n".join(bad)
    return sel, res, org, tm, flat


# ------------------------------------------------------------------------------------------------------------- the cases

def _planted(ctx, nfrag, orient, A, sample=None):
    """1. in a third of the fragments one mate has lost its true candidate (tests/test_mates_rescue.py): the rescue slot holds it under
    either rule; the selection over the augmented list follows the table"""
    plant = tuple((1 + (f // 3) % 2) if f % 3 == 0 else 0 for f in range(nfrag))
    sizes = tuple((3, 3) if f % 6 else (3, 1) for f in range(nfrag))
    case = _case(9700, sizes, orient, plant)
    mn, mx = INS
    rng = np.random.default_rng(9930)
    tables = (rng.integers(0, 41, size=mx - mn + 1).astype(np.uint16), ssw_amd.insert_penalty_normal(275, 60, mn, mx, 2, 17))
    lost = np.array(plant) > 0
    for table, kw in zip(tables, (dict(flag=2), dict(flag=0))):
        sel, res, org, tm, (fsel, _, forg, _) = check(ctx, case, table, orient, A=A, min_score=50, sample=sample, **kw)
        assert tm["rescue_windows"] >= int(lost.sum()) and (fsel["proper"][lost] == 1).all()
        assert ((sel["score"] != fsel["score"]) & (sel["proper"] == 1)).any()      # the table reached the selection
        assert (sel["score"] <= fsel["score"]).all()
    zero = check(ctx, case, np.zeros(mx - mn + 1, dtype=np.uint16), orient, A=A, min_score=50, sample=sample, flag=2)
    fsel, fres, forg, fcig = zero[4]
    assert zero[0].tobytes() == fsel.tobytes() and (zero[1] == fres).all() and zero[2].tobytes() == forg.tobytes()      # an all-zero table: the flat call


def lose_case():
    """one FR fragment: mate 1 is U = tg[2100 : 2150] on the plus strand, with its true window; mate 2 is V = tg[2350 : 2400] (span 300) on
    the minus strand, whose only candidate is a tandem copy at span 650 -- improper at max_insert 500, equal score.  The anchor U has no
    proper partner, so V's true locus comes back in a rescue window."""
    tg = np.asarray(random_ref(4000, 9940, 4), dtype=np.int8).copy()
    s = 2100
    V = tg[s + 250:s + 300].copy()
    tg[s + 600:s + 650] = V
    case = Case.explicit([tg[s:s + 50].copy(), _revcomp(V)], [tg], [[(0, 0, s - 10, 70)], [(2 + 1, 0, s + 590, 70)]])
    case.mate_q = np.arange(2, dtype=np.int32)
    return case


def _rescued_loses(ctx):
    """2. the model makes a rescued candidate lose to a caller's candidate that the flat rule passes over"""
    case = lose_case()
    mn, mx, pen = INS[0], INS[1], 17
    steep = np.zeros(mx - mn + 1, dtype=np.uint16); steep[300 - mn] = 30      # above unpaired_penalty
    for flag in (0, 2):
        sel, res, org, tm, (fsel, fres, forg, _) = check(ctx, case, steep, "fr", A=1, min_score=50, flag=flag)
        # flat: the rescued candidate (position 1 = the slot) makes the proper pair, 100 + 100
        assert (int(fsel["pos1"][0]), int(fsel["pos2"][0]), int(fsel["score"][0]), int(fsel["second_score"][0]), int(fsel["proper"][0])) == (0, 1, 200, 183, 1)
        assert int(forg["anchor"][0, 1]) == 0 and int(forg["tbeg"][0, 1]) + int(fres["ref_end1"][0, 1]) == 2399
        # model: the proper pair pays 30, the improper one 17 -- the caller's candidate wins; properness as defined
        assert (int(sel["pos1"][0]), int(sel["pos2"][0]), int(sel["score"][0]), int(sel["second_score"][0]), int(sel["proper"][0])) == (0, 0, 183, 170, 0)
        assert int(sel["n_proper"][0]) == 1 and int(org["anchor"][0, 1]) == -1 and int(org["tbeg"][0, 1]) == 2690
        assert tm["rescue_windows"] >= 1


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_emu_planted_rescue_under_model(ectx, orient, A):
    _planted(ectx, 12, orient, A)


def test_emu_rescued_candidate_loses(ectx):
    _rescued_loses(ectx)


# ---------------------------------------------------------------------------------------------------------------- MI355X

G_NF = 3000


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("orient", ["fr", "rf", "ff"])
def test_gpu_planted_rescue_under_model(gpu_ctx, orient, A):
    _planted(gpu_ctx, G_NF, orient, A, sample=400)


@pytest.mark.gpu
def test_gpu_rescued_candidate_loses(gpu_ctx):
    _rescued_loses(gpu_ctx)
