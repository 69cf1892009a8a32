"""ssw_gpu_pool_align_windows_mates_model: the pair model over the pool (include/ssw_gpu.h).  Bit for bit the single context's
ssw_gpu_align_windows_mates_model over the whole list -- sel, records, cigar_off, pool words -- for one and for two workers, for a block of
one fragment, a mid value and the default, with and without with_revcomp, at flags 0 and 2; the whole-list refusals name the caller's
fragment.  Cases and helpers of tests/test_pool_mates.py.  On the CPU SIMT emulator and, marked gpu, on the MI355X."""
import ctypes as C
import re

import numpy as np
import pytest

import ssw_amd
from test_mates_orient import INS, MAT, ORIENTS
from test_pool_mates import Env, blocks_of_fragments, pool_case
from test_windows_mates import Case

TABLE_MAX = 65536      # SSW_GPU_INSERT_TABLE_MAX


@pytest.fixture(scope="module")
def eenv(emu_lib_path):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SSW_EMU_DEVICES", "2")
        env = Env(ssw_amd.load(emu_lib_path), ([0], [0, 0]), 9, 3000)
        yield env
        env.close()


@pytest.fixture(scope="module")
def genv(product_lib_path):
    lib = ssw_amd.load(product_lib_path)
    assert lib.ssw_gpu_device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    env = Env(lib, ([0], [0, 0]), 1200, 100000)
    yield env
    env.close()


def table_of(seed):
    return np.random.default_rng(seed).integers(0, 41, size=INS[1] - INS[0] + 1).astype(np.uint16)


def single(env, case, with_revcomp, o, table, **kw):
    """the single context's answer under the model"""
    T = env.ctx.upload(case.targets)
    F = env.ctx.upload(case.fwd)
    Q = F.with_revcomp() if with_revcomp else F
    try:
        return env.ctx.align_windows_mates(Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5, INS[0], INS[1], 30, orientation=o,
                                           insert_penalty=table, **kw)
    finally:
        if with_revcomp:
            Q.free()
        F.free(); T.free()


def same(pool, case, want, with_revcomp, o, table, block, **kw):
    sel, res, cig = pool.align_windows_mates(case.fwd, case.co, case.q, case.t, case.b, case.l, MAT, 5, INS[0], INS[1], 30, orientation=o,
                                             with_revcomp=with_revcomp, block=block, insert_penalty=table, **kw)
    esel, eres, ecig = want
    bad = ["fragment %d: expected %s %s, got %s %s" % (f, esel[f], eres[f], sel[f], res[f]) for f in np.nonzero((sel != esel) | (res != eres).any(axis=1))[0][:4]]
    assert not bad, "%d workers, block %d:\n" % (pool.size(), block) + "\n".join(bad)
    assert sel.tobytes() == esel.tobytes() and (res == eres).all() and cig.tobytes() == ecig.tobytes()
    assert sum(s["blocks"] for s in pool.stats()) == len(blocks_of_fragments(case.co, block, pool.size())) - 1


# ------------------------------------------------------------------------------------------------------------- the cases

def _equal(env, o):
    """1. Pool([0]) and Pool([0, 0]) x block 1 (a fragment per block), 7 and the default, flags 0 and 2, against the single context"""
    case = pool_case(env, o)
    for p in env.pools:
        p.set_targets(case.targets)
    table = table_of(9950 + ORIENTS.index(o))
    for kw in (dict(flag=0), dict(flag=2)):
        want = single(env, case, True, o, table, **kw)
        flat = single(env, case, True, o, None, **kw)
        assert (want[0]["proper"] == 1).any() and (want[0]["score"] != flat[0]["score"]).any()      # the table reached every worker's selection
        for p in env.pools:
            for block in (1, 7, 0):
                same(p, case, want, True, o, table, block, **kw)


def _plus_only(env):
    """2. with_revcomp = 0: everything on the plus strand -- only FF can call a pair proper, and pays the table for it"""
    base = pool_case(env, "ff")
    for p in env.pools:
        p.set_targets(base.targets)
    nr = base.nfwd
    rows = [[(int(base.q[i]) % nr, int(base.t[i]), int(base.b[i]), int(base.l[i])) for i in range(int(base.co[g]), int(base.co[g + 1]))]
            for g in range(len(base.co) - 1)]
    case = Case.explicit(base.fwd, base.targets, rows)
    table = table_of(9960)
    for kw in (dict(flag=0), dict(flag=2)):
        want = single(env, case, False, "ff", table, **kw)
        assert (want[0]["proper"] == 1).any()
        for p in env.pools:
            for block in (1, 7, 0):
                same(p, case, want, False, "ff", table, block, **kw)


def _errors(env):
    """3. the whole-list refusals: -1, the caller's fragment / pair in the message, no output written, no worker started"""
    case = pool_case(env, "fr")
    p = env.pools[-1]
    p.set_targets(case.targets)
    codes, off = ssw_amd._pack(case.fwd)
    nq = len(off) - 1
    nf = (len(case.co) - 1) // 2
    m = np.ascontiguousarray(MAT, dtype=np.int8)
    ok = dict(cand_off=case.co, qidx=case.q, tidx=case.t, tbeg=case.b, tlen=case.l)
    table = table_of(9970)
    late = nf - 4                                       # a fragment well behind the first block
    first = int(case.co[2 * late])                      # its first candidate, as the caller counts

    def refused(what, change=None, mn=INS[0], mx=INS[1], pen=10, o=0, tab=table, null_model=False):
        for flag in (0, 2):
            arr = {f: np.array(v, copy=True) for f, v in ok.items()}
            for f, (at, v) in (change or {}).items():
                arr[f][at] = v
            sel = np.zeros(nf, dtype=ssw_amd.MATES_DTYPE); sel["pos1"] = 777; sel["score"] = 777
            out = np.zeros((nf, 2), dtype=ssw_amd.RESULT_DTYPE); out["score1"] = 777; out["cigar_off"] = 0x5a5a5a5a
            before = sel.tobytes() + out.tobytes()
            words = C.c_int64(5); cp = ssw_amd._u32p()
            prm = ssw_amd.Params(m.ctypes.data_as(ssw_amd._i8p), 5, 3, 1, flag, 0, 0, -1, 2, 0)
            t16 = None if tab is None else np.ascontiguousarray(tab, dtype=np.uint16)
            pm = ssw_amd.PairModel(mn, mx, pen, o, t16.ctypes.data_as(C.POINTER(C.c_uint16)) if t16 is not None else None)
            rc = p.lib.ssw_gpu_pool_align_windows_mates_model(p.h, codes.ctypes.data_as(ssw_amd._i8p), off.ctypes.data_as(ssw_amd._i64p), nq, 1,
                                                              arr["cand_off"].ctypes.data, nf, arr["qidx"].ctypes.data, arr["tidx"].ctypes.data,
                                                              arr["tbeg"].ctypes.data, arr["tlen"].ctypes.data, 1, C.byref(prm), 0,
                                                              None if null_model else C.byref(pm), sel.ctypes.data, out.ctypes.data, C.byref(cp),
                                                              C.byref(words))
            assert rc == -1 and not cp and re.search(what, p.error()), p.error()
            assert words.value == 0 and sel.tobytes() + out.tobytes() == before

    refused(r"^pool_align_windows_mates_model: NULL argument \(model\)", null_model=True)
    refused(r"^pool_align_windows_mates_model: insert_penalty covers more than 65536 spans \(min_insert = 0, max_insert = 65536: 65537 entries\)",
            mn=0, mx=TABLE_MAX, tab=np.zeros(TABLE_MAX + 1, dtype=np.uint16))
    refused(r"^pool_align_windows_mates_model: cand_off decreases \(fragment %d, mate 2" % late, dict(cand_off=(2 * late + 1, int(case.co[2 * late + 2]) + 1)))
    refused(r"^pool_align_windows_mates_model: window out of range \(pair %d:" % first, dict(tlen=(first, 1 << 20)))
    refused(r"^pool_align_windows_mates_model: index out of range \(pair %d: query .* target 2 of 2" % first, dict(tidx=(first, 2)))
    refused(r"0 <= min_insert <= max_insert required \(min_insert = 501, max_insert = 500", mn=501)
    refused(r"unpaired_penalty must be 0 \.\. 65535 \(unpaired_penalty = 65536\)", pen=65536)
    refused(r"orientation must be .*\(orientation = 3\)", o=3)
    want = single(env, case, True, "fr", table, flag=2)
    same(p, case, want, True, "fr", table, 7, flag=2)      # the pool answers the next call
    a = (case.fwd, case.co, case.q, case.t, case.b, case.l, MAT, 5, INS[0], INS[1], 10)
    with pytest.raises(ValueError, match="401 entries, not 400"):
        p.align_windows_mates(*a, with_revcomp=True, insert_penalty=table[:-1])
    with pytest.raises(ValueError, match=r"0 \.\. 65535"):
        p.align_windows_mates(*a, with_revcomp=True, insert_penalty=np.full(len(table), 70000))


# ---------------------------------------------------------------------------------------------------------------- emulator

@pytest.mark.parametrize("o", ORIENTS)
def test_emu_pool_equals_single_context(eenv, o):
    _equal(eenv, o)


def test_emu_plus_strand_only(eenv):
    _plus_only(eenv)


def test_emu_errors(eenv):
    _errors(eenv)


# ---------------------------------------------------------------------------------------------------------------- MI355X

@pytest.mark.gpu
@pytest.mark.parametrize("o", ORIENTS)
def test_gpu_pool_equals_single_context(genv, o):
    _equal(genv, o)


@pytest.mark.gpu
def test_gpu_plus_strand_only(genv):
    _plus_only(genv)


@pytest.mark.gpu
def test_gpu_errors(genv):
    _errors(genv)
