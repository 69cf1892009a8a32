"""ssw_gpu_insert_fit: one histogram row -> quartiles, outlier bounds, mean, sd and the insert range of a mates call (include/ssw_gpu.h).

Host arithmetic only; no device.  The function is defined by the transcription below (mem_pestat's rule, the rounding pinned in integers);
the C must give the same integers and the same BITS in mean and sd: every floating-point step is one correctly rounded IEEE double
operation in both languages (Python's int -> float conversion and its true division of floats, sqrt and floor are), so equality is the
test.  Rows: hand-made edge cases and 200 random ones with a fixed seed (normal, bimodal, heavy-tailed; N = 10 .. 10^6), built as counts."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import ssw_amd
from test_mates_orient import lib_case, sizes_of
from test_windows_mates import MAT

INT_FIELDS = ("n_total", "n_used", "p25", "p50", "p75", "out_lo", "out_hi", "sum", "sum2", "min_insert", "max_insert")


@pytest.fixture(scope="module")
def lib(emu_lib_path):
    return ssw_amd.load(emu_lib_path)


def fit(h):
    """the transcription: None (with N) for "too few observations", else the dict of the struct's fields"""
    h = [int(x) for x in h]
    N = sum(h)
    if N < 10:
        return None, N

    def kth(k):      # k-th smallest span, 0-based: the smallest d with sum(h[:d + 1]) > k
        run = 0
        for d, c in enumerate(h):
            run += c
            if run > k:
                return d
        raise AssertionError("k >= N")
    p25, p50, p75 = kth((250 * N + 499) // 1000), kth((500 * N + 499) // 1000), kth((750 * N + 499) // 1000)
    iqr = p75 - p25
    lo, hi = max(p25 - 2 * iqr, 1), min(p75 + 2 * iqr, len(h) - 1)
    n = sum(h[d] for d in range(lo, hi + 1))
    S1 = sum(d * h[d] for d in range(lo, hi + 1))
    S2 = sum(d * d * h[d] for d in range(lo, hi + 1))
    if n == 0:
        return None, N
    mean = float(S1) / float(n)
    sd = math.sqrt(float(n * S2 - S1 * S1) / (float(n) * float(n)))
    low = min(p25 - 3 * iqr, math.floor(mean - 4.0 * sd + 0.499))
    high = max(p75 + 3 * iqr, math.floor(mean + 4.0 * sd + 0.499))
    return dict(n_total=N, n_used=n, p25=p25, p50=p50, p75=p75, out_lo=lo, out_hi=hi, sum=S1, sum2=S2, mean=mean, sd=sd,
                min_insert=max(low, 1), max_insert=min(high, len(h) - 1)), N


def bits(x):
    return struct.pack("<d", x)


def check(lib, h):
    h = np.ascontiguousarray(h, dtype=np.uint32)
    want, N = fit(h)
    st = ssw_amd.INSERT_STATS(); C.memset(C.byref(st), 0x5a, C.sizeof(st))
    rc = lib.ssw_gpu_insert_fit(h.ctypes.data, len(h), C.byref(st))
    if want is None:
        assert rc == 1 and st.n_total == N
        assert all(getattr(st, f) == 0 for f in INT_FIELDS if f != "n_total") and bits(st.mean) == bits(0.0) and bits(st.sd) == bits(0.0)
        assert ssw_amd.insert_fit(h, lib) is None
        return None
    assert rc == 0
    got = {f: getattr(st, f) for f in INT_FIELDS}
    assert got == {f: want[f] for f in INT_FIELDS}, "expected %s, got %s" % (want, got)
    assert bits(st.mean) == bits(want["mean"]) and bits(st.sd) == bits(want["sd"]), "mean %r / %r, sd %r / %r" % (want["mean"], st.mean, want["sd"], st.sd)
    d = ssw_amd.insert_fit(h, lib)
    assert {f: d[f] for f in INT_FIELDS} == got and bits(d["mean"]) == bits(st.mean) and bits(d["sd"]) == bits(st.sd)
    return d


def row(n_entries, spikes):
    h = np.zeros(n_entries, dtype=np.uint32)
    for d, c in spikes:
        h[d] = c
    return h


def test_hand_made_rows(lib):
    assert check(lib, row(500, [(300, 9)])) is None                        # N = 9
    d = check(lib, row(500, [(300, 10)]))                                  # N = 10; a single spike: iqr == 0, sd == 0
    assert (d["p25"], d["p50"], d["p75"], d["out_lo"], d["out_hi"], d["sd"], d["mean"]) == (300, 300, 300, 300, 300, 0.0, 300.0)
    assert (d["min_insert"], d["max_insert"]) == (300, 300)
    d = check(lib, row(1000, [(200, 600), (400, 500)]))                    # two spikes
    assert (d["p25"], d["p50"], d["p75"]) == (200, 200, 400) and d["n_used"] == 1100 and d["sd"] > 0
    assert check(lib, row(500, [(0, 1000)])) is None                       # all mass at span 0: nothing inside [1, ..]
    assert check(lib, row(1, [(0, 1000)])) is None                         # n_entries == 1
    d = check(lib, row(401, [(380, 100), (390, 100), (400, 100)]))         # the high bound cut at n_entries - 1
    assert d["max_insert"] == 400 and d["out_hi"] == 400
    d = check(lib, row(1000, [(1, 5), (2, 5), (3, 5), (900, 1)]))          # the low bound cut at 1, an outlier left out
    assert d["min_insert"] == 1 and d["n_used"] == 15 and d["n_total"] == 16
    check(lib, row(65536, [(65535, 2 ** 31 - 1)]))                         # the largest sums: S2 just below 2^63
    check(lib, row(65536, [(1, 1 << 30), (65535, (1 << 30) - 1)]))         # the largest variance


def test_random_rows(lib):
    rng = np.random.default_rng(20240611)
    for i in range(200):
        ne = int(rng.integers(50, 3000))
        N = int(10 ** rng.uniform(1, 6))
        x = np.arange(ne, dtype=np.float64)
        kind = i % 3
        if kind == 0:        # normal
            mu, sg = rng.uniform(0.1, 0.9) * ne, rng.uniform(0.5, 0.2 * ne)
            p = np.exp(-0.5 * ((x - mu) / sg) ** 2)
        elif kind == 1:      # bimodal
            m1, m2, sg = rng.uniform(0.1, 0.5) * ne, rng.uniform(0.5, 0.9) * ne, rng.uniform(0.5, 0.1 * ne)
            p = np.exp(-0.5 * ((x - m1) / sg) ** 2) + rng.uniform(0.1, 1.0) * np.exp(-0.5 * ((x - m2) / sg) ** 2)
        else:                # heavy-tailed
            mu, g = rng.uniform(0.1, 0.9) * ne, rng.uniform(0.5, 0.05 * ne)
            p = 1.0 / (1.0 + ((x - mu) / g) ** 2)
        h = rng.multinomial(N, p / p.sum()).astype(np.uint32)              # the row as counts
        assert int(h.sum()) == N >= 10
        check(lib, h)


def test_refusals(lib):
    h = row(10, [(5, 20)])
    st = ssw_amd.INSERT_STATS()
    assert lib.ssw_gpu_insert_fit(None, 10, C.byref(st)) == -1
    assert lib.ssw_gpu_insert_fit(h.ctypes.data, 10, None) == -1
    assert lib.ssw_gpu_insert_fit(h.ctypes.data, 0, C.byref(st)) == -1
    assert lib.ssw_gpu_insert_fit(h.ctypes.data, -1, C.byref(st)) == -1
    big = np.array([1 << 30, 1 << 30], dtype=np.uint32)                    # N = 2^31
    assert lib.ssw_gpu_insert_fit(big.ctypes.data, 2, C.byref(st)) == -1
    with pytest.raises(ValueError):
        ssw_amd.insert_fit(big, lib)
    with pytest.raises(ValueError):
        ssw_amd.insert_fit(np.zeros((2, 5), dtype=np.uint32), lib)
    assert lib.ssw_gpu_insert_fit(np.array([(1 << 31) - 1, 0], dtype=np.uint32).ctypes.data, 2, C.byref(st)) == 1      # N = 2^31 - 1, all at span 0


def test_model_round_trip(lib):
    """histogram -> fit -> insert_model_normal -> align_windows_mates(insert_penalty=...) on the emulator, without a refusal"""
    case = lib_case(9700, sizes_of(9710, 33, ((1, 1), (2, 3), (4, 4), (3, 1))), 3000, "fr")
    ctx = ssw_amd.Context(0, lib)
    try:
        Q, T = case.upload(ctx)
        a = (Q, T, case.co, case.q, case.t, case.b, case.l, case.nfwd, MAT, 5)
        hist, cnt = ctx.insert_hist(*a, 1000)
        assert cnt["n_in"][0] >= 10                                        # (the case: enough FR fragments for a fit)
        st = ssw_amd.insert_fit(hist[0], lib)
        assert st is not None and st["sd"] > 0 and 1 <= st["min_insert"] <= st["p50"] <= st["max_insert"] <= 1000
        model = ssw_amd.insert_model_normal(st, 2, 30)
        assert sorted(model) == ["insert_penalty", "max_insert", "min_insert"]
        assert model["insert_penalty"].dtype == np.uint16 and len(model["insert_penalty"]) == st["max_insert"] - st["min_insert"] + 1
        sel, res, _ = ctx.align_windows_mates(*a, unpaired_penalty=30, flag=0, **model)
        assert (sel["proper"] == 1).any()
        with pytest.raises(ValueError):      # sd == 0: insert_penalty_normal's refusal stands
            ssw_amd.insert_model_normal(ssw_amd.insert_fit(row(500, [(300, 10)]), lib), 2, 30)
        Q.free(); T.free()
    finally:
        ctx.close()
