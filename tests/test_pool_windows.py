"""ssw_gpu_pool_align_windows / ssw_gpu_pool_align_windows_topk: the window entry points over a pool of workers (include/ssw_gpu.h).

The contract is equality: whatever the number of workers and whatever `block` is, the pool gives bit for bit -- pos, n_eligible, every field of
every record (cigar_off included) and the bytes of the CIGAR pool -- what ONE context gives for Context.align_windows / align_windows_topk over
all the reads (with_revcomp: over Seqs.with_revcomp() of them).  So the oracle of every case but one is the single context on the same library;
one case goes to the reference directly (parity.expected).  Every family is written once as a helper over an `Env` and runs on the CPU SIMT
emulator (two pretend-devices, Pool([0, 1])) at the small size and, marked gpu, on the MI355X (Pool([0]) and Pool([0, 0, 0])).  The single
context's answers are computed once per parameter set and shared."""
import re

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix, mutate, random_ref

MAT = dna_matrix(2, 2)
AUTO_FLOOR = 16384          # candidates per block when block <= 0 (include/ssw_gpu.h)


def _revcomp(r):
    r = np.asarray(r, dtype=np.int8)[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


class Env(object):
    """a library, one context on it, a one-worker pool and a several-worker pool"""

    def __init__(self, lib, multi, **sizes):
        self.lib = lib
        self.ctx = ssw_amd.Context(0, lib)
        self.one = ssw_amd.Pool([0], lib)
        self.multi = ssw_amd.Pool(multi, lib)
        self.pools = (self.one, self.multi)
        self.cache = {}
        self.__dict__.update(sizes)

    def close(self):
        self.one.close(); self.multi.close(); self.ctx.close()


@pytest.fixture(scope="module")
def eenv(emu_lib_path):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SSW_EMU_DEVICES", "2")
        env = Env(ssw_amd.load(emu_lib_path), [0, 1], ng=30, tl=(900, 1300), ql=(30, 120), nref=40)
        yield env
        env.close()


@pytest.fixture(scope="module")
def genv(product_lib_path):
    lib = ssw_amd.load(product_lib_path)
    assert lib.ssw_gpu_device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    env = Env(lib, [0, 0, 0], ng=1000, tl=(2000, 5000), ql=(30, 300), nref=200)
    yield env
    env.close()


class Case(object):
    """Three resident targets; reads sampled from them (odd ones stored reverse-complemented when `strands`), a few unrelated short ones.
    Groups of 0..6 candidates: a group mostly follows one read picked at random -- so reads repeat, come out of order and some are never
    named --, a candidate is a window over the read's locus on the matching strand or any window on any strand.  Forced among the groups:
    empty ones, groups of an unrelated 30-residue read on random windows (no candidate reaches min_score), groups whose candidates are all
    reverse strand."""

    def __init__(self, seed, ng, tl, ql, n_codes=4, strands=True, extra=()):
        rng = np.random.default_rng(seed)
        self.targets = [np.asarray(random_ref(int(rng.integers(tl[0], tl[1] + 1)), int(rng.integers(1 << 30)), n_codes), dtype=np.int8) for _ in range(3)]
        nr = max(ng, 8)
        reads, locus = [], []
        for r in range(nr):
            if r % 9 == 4:      # unrelated and short: every score stays low
                reads.append(rng.integers(0, n_codes, size=30, dtype=np.int8)); locus.append(None)
                continue
            t = int(rng.integers(3)); n = int(rng.integers(ql[0], ql[1] + 1)); s = int(rng.integers(0, len(self.targets[t]) - n))
            seq = mutate(self.targets[t][s:s + n], rng, 0.04, 0.01, 0.01, n_codes)
            rev = strands and r % 2 == 1
            reads.append(np.ascontiguousarray(_revcomp(seq) if rev else seq, dtype=np.int8)); locus.append((t, s, n, rev))
        reads = reads + [np.ascontiguousarray(x, dtype=np.int8) for x in extra]
        self.reads, self.nr, self.strands = reads, len(reads), strands
        rows = []
        for g in range(ng):
            kind = g % 10
            size = 0 if kind == 3 else int(rng.integers(0, 7))
            r = int(rng.integers(nr))
            if kind == 6:
                r = 4 + 9 * int(rng.integers((nr - 5) // 9 + 1)); size = max(size, 2)
            row = []
            for _ in range(size):
                q = r if rng.random() < 0.85 else int(rng.integers(nr))
                wl = int(rng.integers(60, 2 * ql[1]))
                if locus[q] is not None and kind != 6 and rng.random() < 0.6:
                    t, s, n, rev = locus[q]
                    wb = int(rng.integers(s - wl + n // 4, s + n - n // 4 + 1)); on_rev = rev
                else:
                    t = int(rng.integers(3)); wb = int(rng.integers(0, len(self.targets[t]))); on_rev = bool(strands and rng.random() < 0.5)
                wl = min(wl, len(self.targets[t])); wb = min(max(wb, 0), len(self.targets[t]) - wl)
                if strands and kind == 8:
                    on_rev = True
                row.append((q + self.nr if on_rev else q, t, wb, wl))
            rows.append(row)
        self.set_rows(rows)

    def set_rows(self, rows):
        self.rows = rows
        self.co = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
        flat = [x for r in rows for x in r]
        self.q = np.array([x[0] for x in flat], dtype=np.int32); self.t = np.array([x[1] for x in flat], dtype=np.int32)
        self.b = np.array([x[2] for x in flat], dtype=np.int64); self.l = np.array([x[3] for x in flat], dtype=np.int32)

    def upload(self, ctx):
        T = ctx.upload(self.targets)
        Q = ctx.upload(self.reads)
        if self.strands:
            both = Q.with_revcomp(); Q.free(); Q = both
        return Q, T

    def read(self, q):
        return self.reads[q] if q < self.nr else _revcomp(self.reads[q - self.nr])


def blocks_of_groups(co, block, workers):
    """the documented rule: whole groups, in order, until a block holds at least `block` candidates; at least one group"""
    ng = len(co) - 1
    if block <= 0:
        block = max(-(-int(co[-1]) // (4 * workers)), AUTO_FLOOR)
    nb = g = 0
    while g < ng:
        c0 = co[g]; g += 1
        while g < ng and co[g] - c0 < block:
            g += 1
        nb += 1
    return nb


def blocks_of_pairs(npairs, block, workers):
    if block <= 0:
        block = max(-(-npairs // (4 * workers)), AUTO_FLOOR)
    return -(-npairs // min(block, npairs))


def _same_topk(a, b):
    """every array of two outputs equal: the records field by field (the four bytes after `status` are padding of the C struct and belong to
    no field), everything else -- pos, n_eligible, the CIGAR words -- byte by byte"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and (bool((x == y).all()) if x.dtype.names else x.tobytes() == y.tobytes())
                                    for x, y in zip(a, b))


def _single(env, case, name, what, mat, n, **kw):
    """the single context's answer, once per case and parameter set"""
    key = (name, what, np.asarray(mat).tobytes(), n, tuple(sorted(kw.items())))
    if key not in env.cache:
        Q, T = case.upload(env.ctx)
        try:
            if what == "topk":
                env.cache[key] = env.ctx.align_windows_topk(Q, T, case.co, case.q, case.t, case.b, case.l, mat, n, **kw)
            else:
                env.cache[key] = env.ctx.align_windows(Q, T, case.q, case.t, case.b, case.l, mat, n, **kw)
        finally:
            Q.free(); T.free()
    return env.cache[key]


def _pool_topk(pool, case, mat, n, **kw):
    return pool.align_windows_topk(case.reads, case.co, case.q, case.t, case.b, case.l, mat, n, with_revcomp=case.strands, **kw)


def _pool_flat(pool, case, mat, n, **kw):
    return pool.align_windows(case.reads, case.q, case.t, case.b, case.l, mat, n, with_revcomp=case.strands, **kw)


def _agree(env, case, name, mat, n, blocks_topk, blocks_flat, pools=None, **kw):
    """pool == single context for the grouped list (kw holds k, min_score, max_drop and the parameters) and for the same list flat"""
    pkw = {f: v for f, v in kw.items() if f not in ("k", "min_score", "max_drop")}
    want = _single(env, case, name, "topk", mat, n, **kw)
    wantf = _single(env, case, name, "flat", mat, n, **pkw)
    npairs = len(case.q)
    for pool in pools or env.pools:
        pool.set_targets(case.targets)
        for block in blocks_topk:
            got = _pool_topk(pool, case, mat, n, block=block, **kw)
            assert _same_topk(got, want), "topk, %d workers, block %d, %s" % (pool.size(), block, kw)
            st = pool.stats()
            assert sum(s["blocks"] for s in st) == blocks_of_groups(case.co, block, pool.size())
            assert sum(s["queries"] for s in st) >= len(set(int(x) % case.nr for x in case.q)) and (npairs == 0 or sum(s["cells"] for s in st) > 0)
        for block in blocks_flat:
            got = _pool_flat(pool, case, mat, n, block=block, **pkw)
            assert _same_topk(got, wantf), "flat, %d workers, block %d, %s" % (pool.size(), block, pkw)
            assert sum(s["blocks"] for s in pool.stats()) == blocks_of_pairs(npairs, block, pool.size())
    return want, wantf


# ------------------------------------------------------------------------------------------------------------- the families

FLAGS = {"flag0": dict(flag=0), "flag2_filters": dict(flag=2, filters=80), "flag15_filterd_mark": dict(flag=15, filters=60, filterd=150, mark_mismatch=True)}
RANKS = [(1, -1), (2, 0), (5, 10)]          # (k, max_drop)


def _equality(env, what):
    """1. both strands, every flag, k and max_drop, block = 1 / about 7 blocks / 0 / more than everything"""
    case = env.cache.setdefault("case1", Case(9100, env.ng, env.tl, env.ql))
    npairs = int(case.co[-1])
    seven = -(-npairs // 7)
    # block = 1: every non-empty group closes a block (the empty groups before it belong to that block: the documented rule)
    assert blocks_of_groups(case.co, seven, 1) in range(4, 9) and blocks_of_groups(case.co, 1, 1) >= int((np.diff(case.co) > 0).sum())
    at = sorted(FLAGS).index(what)
    for i, (k, max_drop) in enumerate(RANKS):
        kw = dict(k=k, min_score=40, max_drop=max_drop, **FLAGS[what])
        # block = 1 means a call of a context per group or pair: once per flag for the groups, once in all for the pairs, on the several-worker
        # pool.  The flat list does not depend on k and max_drop: it runs beside the first pair of them only.
        if i == at:
            _agree(env, case, "case1", MAT, 5, [1], [1] if what == "flag15_filterd_mark" else [], pools=[env.multi], **kw)
        # all the cuts beside the first (k, max_drop); the others on one cut per pool
        one, multi = ([seven, 0], [seven, 0, npairs + 5]) if i == 0 else ([0], [seven])
        _agree(env, case, "case1", MAT, 5, one, one[:1] if i == 0 else [], pools=[env.one], **kw)
        (pos, nel, res, _), _ = _agree(env, case, "case1", MAT, 5, multi, multi if i == 0 else [], pools=[env.multi], **kw)
    sizes = np.diff(case.co)
    assert (sizes == 0).any() and ((sizes > 0) & (nel == 0)).any() and (nel > 1).any()          # empty groups, groups without an eligible candidate
    rev = case.q >= case.nr
    all_rev = np.array([sizes[g] > 0 and rev[case.co[g]:case.co[g + 1]].all() for g in range(env.ng)])
    assert all_rev.any() and (rev[(case.co[:-1, None] + pos)[pos >= 0]]).any() and (~rev[(case.co[:-1, None] + pos)[pos >= 0]]).any()
    named = set(int(x) % case.nr for x in case.q)
    assert len(named) < case.nr and len(named) < npairs and (np.diff(case.q % case.nr) < 0).any()      # never named, repeated, out of order


def _envelopes(env):
    """2. the fallback (reads of 700), the strip kernel's pair mode (800), an empty read and an empty window on either side of block borders"""
    rng = np.random.default_rng(9200)
    case = Case(9201, 6, env.tl, env.ql, extra=[rng.integers(0, 4, size=700, dtype=np.int8), rng.integers(0, 4, size=700, dtype=np.int8),
                                                 rng.integers(0, 4, size=800, dtype=np.int8), np.zeros(0, dtype=np.int8)])
    t0 = case.targets[0]
    r700a, r700b, r800, rempty = case.nr - 4, case.nr - 3, case.nr - 2, case.nr - 1
    case.reads[r700a] = np.ascontiguousarray(mutate(t0[40:760], rng, 0.03, 0.005, 0.005)[:700])
    case.reads[r800] = np.ascontiguousarray(mutate(t0[10:840], rng, 0.03, 0.005, 0.005)[:800])
    assert len(case.reads[r700a]) == 700 and len(case.reads[r800]) == 800
    special = [[(r700a, 0, 20, 780), (0, 1, 5, 200)], [(r800, 0, 0, 880), (r800 + case.nr, 0, 0, 880)], [(rempty, 1, 3, 150), (1, 1, 0, 0)],
               [(r700b + case.nr, 2, 100, 400), (r700a, 0, 0, 850)], [(2, 2, 50, 0), (rempty + case.nr, 0, 0, 0)]]
    rows = []
    for i, sp in enumerate(special):      # a special group between ordinary ones: with 2 candidates per block every border separates two classes
        rows += [sp, [x for x in case.rows[i]][:2] or [(0, 0, 0, 100), (1, 1, 0, 120)]]
    rows = [r if len(r) == 2 else r + [(3, 2, 10, 90)] for r in rows]
    case.set_rows(rows)
    kw = dict(k=2, min_score=0, max_drop=-1, flag=2, filters=30)
    _agree(env, case, "case2", MAT, 5, [5], [3], pools=[env.one], **kw)
    want, wantf = _agree(env, case, "case2", MAT, 5, [2, 0], [1], pools=[env.multi], **kw)
    assert (wantf[0]["score1"][[0, 4]] > 1000).all() and (wantf[0]["score1"][[8, 9, 16, 17]] == 0).all()      # the long reads found their loci; the empty ones score 0
    Q, T = case.upload(env.ctx)
    try:
        wr = env.ctx.align_windows_topk(Q, T, case.co, case.q, case.t, case.b, case.l, MAT, 5, 2, flag=2, rebase=True)
        wrf = env.ctx.align_windows(Q, T, case.q, case.t, case.b, case.l, MAT, 5, flag=2, rebase=True)
    finally:
        Q.free(); T.free()
    assert (wrf[0]["ref_end1"] != wantf[0]["ref_end1"]).any()
    assert _same_topk(_pool_topk(env.multi, case, MAT, 5, k=2, flag=2, rebase=True, block=2), wr)
    assert _same_topk(_pool_flat(env.multi, case, MAT, 5, flag=2, rebase=True, block=3), wrf)


def _protein(env):
    """3. BLOSUM50, no reverse strand"""
    case = env.cache.setdefault("case3", Case(9300, max(env.ng // 2, 20), env.tl, env.ql, n_codes=20, strands=False))
    npairs = int(case.co[-1])
    (pos, _, res, _), _ = _agree(env, case, "case3", blosum50(), 24, [-(-npairs // 5), 0], [-(-npairs // 5)], k=3, min_score=0, max_drop=-1, gapO=10,
                                 gapE=2, flag=2, filters=60)
    assert (res["cigarLen"][pos >= 0] > 0).any()


def _reference(env):
    """4. one flat list through the pool against the reference itself"""
    case = env.cache.setdefault("case1", Case(9100, env.ng, env.tl, env.ql))
    sub = Case.__new__(Case)
    sub.targets, sub.reads, sub.nr, sub.strands = case.targets, case.reads, case.nr, True
    sub.set_rows([[(int(case.q[i]), int(case.t[i]), int(case.b[i]), int(case.l[i]))] for i in range(min(env.nref, len(case.q)))])
    env.multi.set_targets(sub.targets)
    res, cig = _pool_flat(env.multi, sub, MAT, 5, flag=1, block=max(len(sub.q) // 5, 1))
    bad = []
    for i in range(len(sub.q)):
        rd = sub.read(int(sub.q[i]))
        rf = np.ascontiguousarray(sub.targets[int(sub.t[i])][int(sub.b[i]):int(sub.b[i]) + int(sub.l[i])])
        exp, xcig = expected(rd, MAT, 5, rf, 3, 1, 1, 0, 0, len(rd) // 2, 2)
        rec = res[i]
        off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
        got = [int(x) for x in cig[off:off + ln]] if ln > 0 else []
        if not (exp is not None and int(rec["status"]) == 0 and {f: int(rec[f]) for f in RES_FIELDS} == exp and got == xcig) and len(bad) < 4:
            bad.append("pair %d (len %d x %d): expected %s %s got %s %s" % (i, len(rd), len(rf), exp, cigar_str(xcig), rec, cigar_str(got)))
    assert not bad, "\n".join(bad)
    assert (res["cigarLen"] > 0).sum() > len(sub.q) // 2 and (sub.q >= sub.nr).any()


def _errors(env):
    """5. refused calls name the caller's index, write nothing and leave the pool usable"""
    case = env.cache.setdefault("case1", Case(9100, env.ng, env.tl, env.ql))
    ng, npairs, nq = env.ng, int(case.co[-1]), case.nr

    def sentinel(k):
        pos = np.full((ng, k), 777, dtype=np.int32); nel = np.full(ng, 777, dtype=np.int32)
        res = np.zeros((ng, k), dtype=ssw_amd.RESULT_DTYPE); flat = np.zeros(npairs, dtype=ssw_amd.RESULT_DTYPE)
        for f in ssw_amd.RESULT_DTYPE.names:
            res[f] = 777; flat[f] = 777
        return pos, nel, res, flat

    def refused(pool, what, k=2, with_revcomp=True, flat=True, **change):
        arr = dict(co=case.co.copy(), q=case.q.copy(), t=case.t.copy(), b=case.b.copy(), l=case.l.copy())
        for f, (at, v) in change.items():
            arr[f][at] = v
        pos, nel, res, fl = sentinel(max(k, 0))
        before = pos.tobytes() + nel.tobytes() + res.tobytes() + fl.tobytes()
        with pytest.raises(RuntimeError) as e:
            pool.align_windows_topk(case.reads, arr["co"], arr["q"], arr["t"], arr["b"], arr["l"], MAT, 5, k, with_revcomp=with_revcomp, flag=2,
                                    block=7, out=(pos, nel, res))
        assert re.search(what, str(e.value)), str(e.value)
        if flat:
            with pytest.raises(RuntimeError) as e:
                pool.align_windows(case.reads, arr["q"], arr["t"], arr["b"], arr["l"], MAT, 5, with_revcomp=with_revcomp, flag=2, block=7, out=fl)
            assert re.search(what, str(e.value)), str(e.value)
        assert pos.tobytes() + nel.tobytes() + res.tobytes() + fl.tobytes() == before

    fresh = ssw_amd.Pool([0], env.lib)
    try:
        refused(fresh, "no target set")
    finally:
        fresh.close()
    want = _single(env, case, "case1", "topk", MAT, 5, k=2, min_score=40, max_drop=0, **FLAGS["flag2_filters"])
    last = npairs - 1
    fwd = int(np.nonzero(case.q < nq)[0][-1])
    tl_last = len(case.targets[int(case.t[last])])
    g_dec = int(np.nonzero(np.diff(case.co) > 1)[0][-1])
    for pool in env.pools:
        pool.set_targets(case.targets)
        # a read index that only exists with the reverse strand; one past both strands
        q_fwd = np.where(case.q < nq, case.q, case.q - nq).astype(np.int32)
        arr_q = q_fwd.copy(); arr_q[fwd] = nq
        refused(pool, r"index out of range.*pair %d\b.*query %d of %d\b" % (fwd, nq, nq), with_revcomp=False, q=(slice(None), arr_q))
        refused(pool, r"index out of range.*pair %d\b.*query %d of %d\b" % (last, 2 * nq, 2 * nq), q=(last, 2 * nq))
        # one residue past the end of its target, in the last pair of the list
        refused(pool, r"window out of range.*pair %d\b" % last, b=(last, tl_last - int(case.l[last]) + 1))
        refused(pool, r"cand_off decreases.*group %d\b" % g_dec, flat=False, co=(g_dec + 1, int(case.co[g_dec]) - 1))
        refused(pool, r"k must be 1 \.\. 64.*k = 0", k=0, flat=False)
        refused(pool, r"k must be 1 \.\. 64.*k = 65", k=65, flat=False)
        got = _pool_topk(pool, case, MAT, 5, k=2, min_score=40, max_drop=0, block=9, **FLAGS["flag2_filters"])      # the pool answers the next call
        assert _same_topk(got, want)
        e = np.zeros(0, np.int32)
        ps, ne, r, c = pool.align_windows_topk(case.reads, [0], e, e, np.zeros(0, np.int64), e, MAT, 5, 3, flag=2)
        assert ps.shape == (0, 3) and ne.shape == (0,) and r.shape == (0, 3) and c.shape == (0,)
        r, c = pool.align_windows(case.reads, e, e, np.zeros(0, np.int64), e, MAT, 5, flag=2)
        assert r.shape == (0,) and c.shape == (0,)
        ps, ne, r, c = pool.align_windows_topk(case.reads, [0, 0, 0], e, e, np.zeros(0, np.int64), e, MAT, 5, 3, flag=2, block=1)      # groups without candidates
        assert (ps == -1).all() and (ne == 0).all() and (r["cigar_off"] == -1).all() and (r["ref_begin1"] == -1).all() and c.shape == (0,)
        assert sum(s["blocks"] for s in pool.stats()) == blocks_of_groups(np.zeros(3, np.int64), 1, pool.size()) == 1


def _order(env):
    """6. one worker or several, one cut or another: the same bytes"""
    case = env.cache.setdefault("case1", Case(9100, env.ng, env.tl, env.ql))
    npairs = int(case.co[-1])
    outs, flats = [], []
    for pool in env.pools:
        pool.set_targets(case.targets)
        for block in (-(-npairs // 5), -(-npairs // 2)):
            outs.append(_pool_topk(pool, case, MAT, 5, k=3, min_score=30, max_drop=20, block=block, flag=1))
            flats.append(_pool_flat(pool, case, MAT, 5, block=block, flag=1))
    assert len(outs) == 4 and all(_same_topk(o, outs[0]) for o in outs[1:]) and all(_same_topk(o, flats[0]) for o in flats[1:])
    assert len(outs[0][3]) > 0 and len(flats[0][1]) > 0


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("what", sorted(FLAGS))
def test_emu_equality_both_strands(eenv, what):
    _equality(eenv, what)


def test_emu_envelopes_across_block_borders(eenv):
    _envelopes(eenv)


def test_emu_protein_blosum50(eenv):
    _protein(eenv)


def test_emu_against_reference(eenv):
    _reference(eenv)


def test_emu_errors_write_nothing(eenv):
    _errors(eenv)


def test_emu_order_independence(eenv):
    _order(eenv)


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(FLAGS))
def test_gpu_equality_both_strands(genv, what):
    _equality(genv, what)


@pytest.mark.gpu
def test_gpu_envelopes_across_block_borders(genv):
    _envelopes(genv)


@pytest.mark.gpu
def test_gpu_protein_blosum50(genv):
    _protein(genv)


@pytest.mark.gpu
def test_gpu_against_reference(genv):
    _reference(genv)


@pytest.mark.gpu
def test_gpu_errors_write_nothing(genv):
    _errors(genv)


@pytest.mark.gpu
def test_gpu_order_independence(genv):
    _order(genv)
