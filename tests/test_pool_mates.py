"""ssw_gpu_pool_align_windows_mates: the best candidate pair per read pair over a pool of workers (include/ssw_gpu.h).

The contract is equality: whatever the number of workers and whatever `block` is, the pool gives bit for bit -- every field of `sel`, every
field of both records per fragment (cigar_off included) and the words of the CIGAR pool -- what ONE context gives for
Context.align_windows_mates over all the reads with nfwd = the number of reads (with_revcomp: over Seqs.with_revcomp() of them; without it
everything is on the plus strand).  So the oracle is the single context on the same library, which tests/test_mates_orient.py holds against
Context.align_windows plus the rule in plain Python and against the reference.  Every family is written once over an `Env` and runs on the CPU
SIMT emulator (three pretend-devices: pools of 1, 2 and 3 workers) and, marked gpu, on the MI355X (Pool([0]) and Pool([0, 0])).  Sizes as in
tests/test_windows_mates.py: reads of 40..100 residues, windows of 80..250 columns, two targets of about 3 000 columns."""
import ctypes as C
import re

import numpy as np
import pytest

import ssw_amd
from test_mates_orient import INS, MAT, ORIENTS, LibCase, sizes_of
from test_windows_mates import Case

AUTO_FLOOR = 16384          # candidates per block when block <= 0 (include/ssw_gpu.h)
GROUP_MAX = 4096            # SSW_GPU_MATES_GROUP_MAX


class Env(object):
    """a library, one context on it and pools of several sizes"""

    def __init__(self, lib, pools, nfrag, L):
        self.lib = lib
        self.ctx = ssw_amd.Context(0, lib)
        self.pools = [ssw_amd.Pool(devs, lib) for devs in pools]
        self.nfrag, self.L = nfrag, L
        self.cases = {}

    def close(self):
        for p in self.pools:
            p.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def eenv(emu_lib_path):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SSW_EMU_DEVICES", "3")
        env = Env(ssw_amd.load(emu_lib_path), ([0], [0, 1], [0, 1, 2]), 12, 3000)
        yield env
        env.close()


@pytest.fixture(scope="module")
def genv(product_lib_path):
    lib = ssw_amd.load(product_lib_path)
    assert lib.ssw_gpu_device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    env = Env(lib, ([0], [0, 0]), 1200, 100000)
    yield env
    env.close()


def pool_case(env, made):
    """fragments of a library `made` (test_mates_orient.LibCase), then re-listed: in DESCENDING fragment order -- so that the reads a block
    names come out of order --, three of them once more at the end (reads named by several fragments), empty fragments at the start, in
    the middle and at the end, one fragment with (0, n) candidates, one fragment with candidates on the plus strand only beside fragments that
    name a reverse strand."""
    if made not in env.cases:
        nf = env.nfrag
        base = LibCase(9800 + ORIENTS.index(made), list(sizes_of(9801, nf, ((3, 2), (2, 4), (5, 5), (1, 1)))), env.L, made)
        nr = base.nfwd
        rows = [[tuple(int(x) for x in (base.q[i], base.t[i], base.b[i], base.l[i])) for i in range(int(base.co[g]), int(base.co[g + 1]))]
                for g in range(2 * nf)]
        order = list(range(nf - 1, -1, -1)) + [2, 2, 0]
        new = []
        for f in order:
            new += [rows[2 * f], rows[2 * f + 1]]
        n = len(order)
        for f in (0, n // 2, n - 1):                       # empty fragments at the start, in the middle and at the end
            new[2 * f] = []; new[2 * f + 1] = []
        new[2 * 1] = []                                    # (0, n)
        new[2 * 1 + 1] = rows[2 * 2 + 1] + rows[2 * 2]     # ... with the candidates of both mates of fragment 2: n >= 1
        plus = n - 3                                       # fragment 2's second copy: everything on the plus strand
        new[2 * plus] = [(q % nr, t, b, l) for q, t, b, l in new[2 * plus]]; new[2 * plus + 1] = [(q % nr, t, b, l) for q, t, b, l in new[2 * plus + 1]]
        case = Case.explicit(base.fwd, base.targets, new)
        case.plus_only = plus
        env.cases[made] = case
        for p in env.pools:
            p.set_targets(case.targets)                    # (every library's case has its own targets: every family sets them again)
    return env.cases[made]


def blocks_of_fragments(co, block, workers):
    """the documented rule: whole fragments, in order, until a block holds at least `block` candidates; at least one fragment; an empty
    fragment stays in the block it falls into -> the first fragment of every block, and nfrag"""
    nf = (len(co) - 1) // 2
    if block <= 0:
        block = max(-(-int(co[-1]) // (4 * workers)), AUTO_FLOOR)
    starts = []
    f = 0
    while f < nf:
        starts.append(f)
        c0 = co[2 * f]; f += 1
        while f < nf and co[2 * f] - c0 < block:
            f += 1
    return starts + [nf]


def single(env, case, key, with_revcomp, o, mn, mx, pen, **kw):
    """the single context's answer, once per parameter set"""
    k = (id(case), key, with_revcomp, o, mn, mx, pen, tuple(sorted(kw.items())))
    if k not in env.cases:
        T = env.ctx.upload(case.targets)
        F = env.ctx.upload(case.fwd)
        Q = F.with_revcomp() if with_revcomp else F
        try:
            env.cases[k] = env.ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, mn, mx, pen, orientation=o, **kw)
        finally:
            if with_revcomp:
                Q.free()
            F.free(); T.free()
    return env.cases[k]


def same(pool, case, want, with_revcomp, o, mn, mx, pen, block, **kw):
    sel, res, cig = pool.align_windows_mates(case.fwd, case.co, case.q, case.t, case.b, case.l, MAT, 5, mn, mx, pen, orientation=o,
                                             with_revcomp=with_revcomp, block=block, **kw)
    esel, eres, ecig = want
    bad = ["fragment %d: expected %s %s, got %s %s" % (f, esel[f], eres[f], sel[f], res[f]) for f in np.nonzero((sel != esel) | (res != eres).any(axis=1))[0][:4]]
    assert not bad, "%d workers, block %d:\n" % (pool.size(), block) + "\n".join(bad)
    assert sel.tobytes() == esel.tobytes() and (res == eres).all() and cig.tobytes() == ecig.tobytes()      # (a record has padding bytes that no one writes)
    st = pool.stats()
    assert sum(s["blocks"] for s in st) == len(blocks_of_fragments(case.co, block, pool.size())) - 1
    return sel, res, cig, st


# ------------------------------------------------------------------------------------------------------------- the cases

def _equal(env, o, kw):
    """1. every pool size x block 1 (a fragment per block), 7, 10^9 (one block) and the default against the single context: every block
    size on the largest pool, block 7 (and, at flag 0, the default) on the others"""
    case = pool_case(env, o)
    for p in env.pools:
        p.set_targets(case.targets)
    nr = case.nfwd
    n = (len(case.co) - 1) // 2
    sizes = np.diff(case.co)
    assert sizes[0] == sizes[1] == 0 and sizes[2 * n - 1] == sizes[2 * n - 2] == 0 and sizes[2 * (n // 2)] == sizes[2 * (n // 2) + 1] == 0
    assert sizes[2] == 0 and sizes[3] >= 1                                                       # the (0, n) fragment
    f = case.plus_only
    assert sizes[2 * f] + sizes[2 * f + 1] > 0 and (case.q[case.co[2 * f]:case.co[2 * f + 2]] < nr).all() and (case.q >= nr).any()
    assert (np.diff(case.q.astype(np.int64) % nr) < 0).any()                                     # reads out of order
    want = single(env, case, "list", True, o, INS[0], INS[1], 30, **kw)
    assert (want[0]["proper"] == 1).any() and (want[0]["pos1"] >= 0).any()
    if kw.get("flag"):
        assert len(want[2]) > 0
    for p in env.pools:
        for block in ((1, 7, 10 ** 9, 0) if p is env.pools[-1] else (7, 0) if not kw.get("flag") else (7,)):
            _, _, _, st = same(p, case, want, True, o, INS[0], INS[1], 30, block, **kw)
            if block == 1:      # a block closes with its first candidate: one fragment with candidates per block at most; `queries`: distinct reads, summed over the blocks
                cut = blocks_of_fragments(case.co, 1, p.size())
                assert all(int(((sizes[0::2] + sizes[1::2])[a:b] > 0).sum()) <= 1 for a, b in zip(cut, cut[1:]))
                assert sum(s["queries"] for s in st) == sum(len(set(int(x) % nr for x in case.q[case.co[2 * a]:case.co[2 * b]])) for a, b in zip(cut, cut[1:]))
            if block == 10 ** 9:
                assert sum(s["blocks"] for s in st) == 1


def _plus_only(env):
    """2. with_revcomp = 0: nfwd = nq over the reads alone, everything on the plus strand -- only FF can call a pair proper"""
    base = pool_case(env, "ff")
    for p in env.pools:
        p.set_targets(base.targets)
    nr = base.nfwd
    rows = [[(int(base.q[i]) % nr, int(base.t[i]), int(base.b[i]), int(base.l[i])) for i in range(int(base.co[g]), int(base.co[g + 1]))]
            for g in range(len(base.co) - 1)]
    case = Case.explicit(base.fwd, base.targets, rows)
    for o in ORIENTS:
        want = single(env, case, "plus", False, o, INS[0], INS[1], 30, flag=2)
        assert (want[0]["proper"] == 1).any() == (o == "ff")
        for p in (env.pools if o == "ff" else env.pools[-1:]):
            for block in ((1, 0) if p is env.pools[-1] else (7,)):
                same(p, case, want, False, o, INS[0], INS[1], 30, block, flag=2)
    # the same list with with_revcomp = 1 and no candidate above nq: the same answer
    want = single(env, case, "plus", False, "ff", INS[0], INS[1], 30, flag=2)
    same(env.pools[-1], case, want, True, "ff", INS[0], INS[1], 30, 7, flag=2)


def _rebase_and_out(env):
    """3. rebase as in the context method; `out` arrays are filled in place"""
    case = pool_case(env, "fr")
    p = env.pools[-1]
    p.set_targets(case.targets)
    want = single(env, case, "list", True, "fr", INS[0], INS[1], 30, flag=2, rebase=True)
    rel = single(env, case, "list", True, "fr", INS[0], INS[1], 30, flag=2)
    assert (want[1]["ref_begin1"] != rel[1]["ref_begin1"]).any()
    same(p, case, want, True, "fr", INS[0], INS[1], 30, 7, flag=2, rebase=True)
    nf = (len(case.co) - 1) // 2
    out = (np.zeros(nf, dtype=ssw_amd.MATES_DTYPE), np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE))
    sel, res, _ = p.align_windows_mates(case.fwd, case.co, case.q, case.t, case.b, case.l, MAT, 5, INS[0], INS[1], 30, with_revcomp=True, block=7, flag=2, out=out)
    assert sel is out[0] and res is out[1] and sel.tobytes() == rel[0].tobytes() and (res == rel[1]).all()


def _errors(env):
    """4. every refusal: -1, the caller's fragment / mate / pair in the message, no output written, no worker started"""
    case = pool_case(env, "fr")
    p = env.pools[-1]
    p.set_targets(case.targets)
    codes, off = ssw_amd._pack(case.fwd)
    nq = len(off) - 1
    nf = (len(case.co) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    ok = dict(cand_off=case.co, qidx=case.q, tidx=case.t, tbeg=case.b, tlen=case.l)
    want = single(env, case, "list", True, "fr", INS[0], INS[1], 30, flag=2)
    late = nf - 4                                       # a fragment well behind the first block
    assert case.co[2 * late + 1] > case.co[2 * late] and case.co[2 * late + 2] > case.co[2 * late + 1]
    first = int(case.co[2 * late])                      # its first candidate, as the caller counts

    def call(pool, arr, sel, out, words, nfrag=nf, mn=0, mx=500, pen=10, o=0, flag=0, rev=1, null=()):
        prm = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
        cp = ssw_amd._u32p()
        a = [pool.h, codes.ctypes.data_as(ssw_amd._i8p), off.ctypes.data_as(ssw_amd._i64p), nq, rev, arr["cand_off"].ctypes.data, nfrag,
             arr["qidx"].ctypes.data, arr["tidx"].ctypes.data, arr["tbeg"].ctypes.data, arr["tlen"].ctypes.data, 1, C.byref(prm), 0, mn, mx, pen, o,
             sel.ctypes.data, out.ctypes.data, C.byref(cp), C.byref(words)]
        for at in null:
            a[at] = None
        rc = pool.lib.ssw_gpu_pool_align_windows_mates(*a)
        if rc != 0:
            assert not cp
        elif cp:
            C.CDLL(None).free(cp)
        return rc

    def sentinel():
        sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
        out = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
        return sel, out

    def refused(what, change=None, pool=p, **kw):
        for flag in (0, 2):
            arr = {f: np.array(v, copy=True) for f, v in ok.items()}
            for f, (at, v) in (change or {}).items():
                arr[f][at] = v
            sel, out = sentinel()
            before = sel.tobytes() + out.tobytes()
            words = C.c_int64(5)
            rc = call(pool, arr, sel, out, words, flag=flag, **kw)
            assert rc == -1 and re.search(what, pool.error()), pool.error()
            assert words.value == 0 and sel.tobytes() + out.tobytes() == before

    refused(r"^pool_align_windows_mates: cand_off\[0\] must be 0.*fragment 0 starts at candidate 1", dict(cand_off=(0, 1)))
    refused(r"^pool_align_windows_mates: cand_off decreases \(fragment %d, mate 2" % late, dict(cand_off=(2 * late + 1, int(case.co[2 * late + 2]) + 1)))
    refused(r"^pool_align_windows_mates: cand_off decreases \(fragment %d, mate 1" % late, dict(cand_off=(2 * late + 1, int(case.co[2 * late]) - 1)))
    refused(r"^pool_align_windows_mates: window out of range \(pair %d:" % first, dict(tlen=(first, 1 << 20)))
    refused(r"^pool_align_windows_mates: window out of range \(pair %d:" % first, dict(tbeg=(first, -1)))
    refused(r"^pool_align_windows_mates: index out of range \(pair %d: query %d of %d" % (first + 1, 2 * nq, 2 * nq), dict(qidx=(first + 1, 2 * nq)))
    firstrev = int(np.nonzero(case.q >= nq)[0][0])      # without with_revcomp the list's first reverse-strand candidate is out of range
    refused(r"^pool_align_windows_mates: index out of range \(pair %d: query %d of %d" % (firstrev, int(case.q[firstrev]), nq), rev=0)
    refused(r"^pool_align_windows_mates: index out of range \(pair %d: query .* target 2 of 2" % first, dict(tidx=(first, 2)))
    refused(r"0 <= min_insert <= max_insert required \(min_insert = -1", mn=-1)
    refused(r"0 <= min_insert <= max_insert required \(min_insert = 501, max_insert = 500", mn=501)
    refused(r"unpaired_penalty must be 0 \.\. 65535 \(unpaired_penalty = -1\)", pen=-1)
    refused(r"unpaired_penalty must be 0 \.\. 65535 \(unpaired_penalty = 65536\)", pen=65536)
    refused(r"orientation must be .*\(orientation = 3\)", o=3)
    refused(r"orientation must be .*\(orientation = -1\)", o=-1)
    for at in (5, 7, 8, 9, 10, 18, 19):      # cand_off, qidx, tidx, tbeg, tlen, sel, results
        refused(r"^pool_align_windows_mates: NULL argument", null=(at,))
    same(p, case, want, True, "fr", INS[0], INS[1], 30, 7, flag=2)      # the pool answers the next call
    # a group over the limit: refused from cand_off alone, before a candidate is read
    big = np.array(case.co, copy=True); big[2 * late + 1:] += GROUP_MAX + 1
    sel, out = sentinel(); before = sel.tobytes() + out.tobytes(); words = C.c_int64(5)
    arr = dict(ok); arr["cand_off"] = big
    assert call(p, arr, sel, out, words) == -1 and re.search(r"more than 4096 candidates in a group \(fragment %d, mate 1" % late, p.error()), p.error()
    assert words.value == 0 and sel.tobytes() + out.tobytes() == before
    # no target set
    fresh = ssw_amd.Pool([0], env.lib)
    try:
        refused(r"^pool_align_windows_mates: no target set", pool=fresh)
    finally:
        fresh.close()
    same(p, case, want, True, "fr", INS[0], INS[1], 30, 1, flag=2)
    # nfrag == 0: 0, no words, nothing written
    sel, out = sentinel(); before = sel.tobytes() + out.tobytes(); words = C.c_int64(5)
    assert call(p, ok, sel, out, words, nfrag=0) == 0 and words.value == 0 and sel.tobytes() + out.tobytes() == before
    e = np.zeros(0, np.int32)
    s, r, c = p.align_windows_mates(case.fwd, [0], e, e, np.zeros(0, np.int64), e, MAT, 5, 0, 500, 10, with_revcomp=True, flag=2)
    assert s.shape == (0,) and r.shape == (0, 2) and c.shape == (0,)
    # fragments without a candidate
    s, r, c = p.align_windows_mates(case.fwd, [0, 0, 0, 0, 0], e, e, np.zeros(0, np.int64), e, MAT, 5, 0, 500, 10, with_revcomp=True, flag=2)
    assert (s["pos1"] == -1).all() and (s["pos2"] == -1).all() and (s["score"] == 0).all() and (r["cigar_off"] == -1).all() and c.shape == (0,)
    with pytest.raises(ValueError):
        p.align_windows_mates(case.fwd, [0, 1], [0], [0], [0], [1], MAT, 5, 0, 500, 10)
    with pytest.raises(ValueError):
        p.align_windows_mates(case.fwd, case.co, case.q, case.t, case.b, case.l, MAT, 5, 0, 500, 10, orientation="xx")


# ---------------------------------------------------------------------------------------------------------------- emulator

KWS = dict(flag0=dict(flag=0), flag2=dict(flag=2), mark=dict(flag=2, mark_mismatch=True))


@pytest.mark.parametrize("what", sorted(KWS))
@pytest.mark.parametrize("o", ORIENTS)
def test_emu_pool_equals_single_context(eenv, o, what):
    _equal(eenv, o, KWS[what])


def test_emu_plus_strand_only(eenv):
    _plus_only(eenv)


def test_emu_rebase_and_out(eenv):
    _rebase_and_out(eenv)


def test_emu_errors(eenv):
    _errors(eenv)


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(KWS))
@pytest.mark.parametrize("o", ORIENTS)
def test_gpu_pool_equals_single_context(genv, o, what):
    _equal(genv, o, KWS[what])


@pytest.mark.gpu
def test_gpu_plus_strand_only(genv):
    _plus_only(genv)


@pytest.mark.gpu
def test_gpu_rebase_and_out(genv):
    _rebase_and_out(genv)


@pytest.mark.gpu
def test_gpu_errors(genv):
    _errors(genv)
