"""Half-row fill chains (k_fill8): eight positions x R8 = ceil(len / 8) rows are exactly the rows the reference's 16-bit kernel pads a read
to; the eight further zero-score rows that only its 8-bit kernel has are not computed but taken from a closed form (DESIGN.md "Half-row
chains").

(a) the closed form against a plain DP over all P16 rows, on the CPU, and never vacuously: in every case the padded rows raise at
    least one column maximum;
(b) the real kernel source on the emulator against the reference: every eligible R8 class at both ends of the instance list and around the
    bench's read length, ineligible neighbours in the same batch, 1 / 2 / 3 reads (a lone read, a full pair, a dead second chain), flags
    0 / 1 / 2, both scorings of the bench, a target that the small-call rule cuts into many tiles, renormalisation inside a scan
    (SSW_GPU_FRAME_K), and records identical to the 16-lane kernel's (SSW_GPU_FILL_HALF=0)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "complete-striped-smith-waterman-library_amd")

SCORINGS = ((2, 2, 3, 1), (1, 3, 5, 2), (3, 1, 2, 1), (2, 2, 4, 3))     # match, mismatch, gapO, gapE
NEG = -10 ** 9


def _plain_dp(read, target, match, mism, gO, gE, rows):
    """Smith-Waterman with affine gaps, cell by cell, over `rows` rows: the read, then zero-score rows.  Per column: the maximum over the
    first rows - 8 rows, over all rows, H of row rows - 9 and the F that enters row rows - 8."""
    P8 = rows - 8
    m = len(target)
    Hp = [0] * (rows + 1)                     # previous column, index 0: the boundary row
    E = [NEG] * (rows + 1)
    cm8, cm16, htop, ftop = [0] * m, [0] * m, [0] * m, [0] * m
    L = len(read)
    for j in range(m):
        tj = target[j]
        Hn = [0] * (rows + 1)
        F = NEG
        m8 = m16 = 0
        for i in range(1, rows + 1):
            s = 0 if i > L else (match if read[i - 1] == tj else -mism)
            e = max(E[i] - gE, Hp[i] - gO)    # horizontal gap: from column j - 1
            E[i] = e
            h = max(0, Hp[i - 1] + s, e, F)
            Hn[i] = h
            if h > m16:
                m16 = h
            if i <= P8 and h > m8:
                m8 = h
            F = max(F - gE, h - gO)           # the F that enters row i + 1
            if i == P8:
                htop[j] = h
                ftop[j] = F
        Hp = Hn
        cm8[j], cm16[j] = m8, m16
    return cm8, cm16, htop, ftop


def _closed_form(cm8, htop, ftop, gO, gE):
    """v(c) = max(0, Htop(c-1), Ftop(c)); T(j) = max(T(j-1) - gapE, v(j-8) - gapO); M(j) = max(v(j..j-7), T(j)); all rows: max(cm8, M)"""
    m = len(cm8)
    v = [max(0, htop[c - 1] if c > 0 else 0, ftop[c]) for c in range(m)]
    out, T = [0] * m, NEG
    for j in range(m):
        T = max(T - gE, (v[j - 8] if j >= 8 else 0) - gO)
        M = max(max(v[max(0, j - 7):j + 1]), T)
        out[j] = max(cm8[j], M)
    return out


def _target(kind, m, rng):
    if kind == 0:
        return rng.integers(0, 4, size=m).tolist()
    if kind == 1:                              # two letters only
        return rng.choice([1, 3], size=m).tolist()
    unit = rng.integers(0, 4, size=int(rng.integers(2, 6))).tolist()     # tandem repeat with a few substitutions
    t = (unit * (m // len(unit) + 1))[:m]
    for k in rng.integers(0, m, size=m // 40):
        t[k] = int(rng.integers(0, 4))
    return t


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "%d_%d_%d_%d" % s)
def test_closed_form_of_the_padded_rows_equals_the_plain_dp(scoring):
    match, mism, gO, gE = scoring
    rng = np.random.default_rng(1000 + 7 * match + gO)
    for ci, L in enumerate((1, 6, 8, 17, 22, 38, 101, 150, 152)):
        P16 = (L + 15) // 16 * 16
        assert (L + 7) // 8 * 8 == P16 - 8     # these are the lengths the half-row chains take
        for kind in range(3):
            m = int(rng.integers(300, 701))
            tgt = _target(kind if L > 8 else 0, m, rng)
            off = int(rng.integers(0, m - L))
            read = tgt[off:off + L]            # an exact copy of a target segment: the best cell lies in the last real row
            if (ci + kind) % 2 and L > 8:      # ... or a copy with substitutions and one deletion
                read = [int(rng.integers(0, 4)) if rng.random() < 0.08 else x for x in read]
                read = read[:L // 2] + tgt[off + L:off + L + 1] + read[L // 2:L - 1]
            assert len(read) == L
            cm8, cm16, htop, ftop = _plain_dp(read, tgt, match, mism, gO, gE, P16)
            got = _closed_form(cm8, htop, ftop, gO, gE)
            raised = sum(a > b for a, b in zip(cm16, cm8))
            assert raised > 0, ("vacuous case: the padded rows change no column maximum", L, kind, scoring)
            diff = [j for j in range(m) if got[j] != cm16[j]]
            assert not diff, (L, kind, scoring, diff[:5], [(cm16[j], got[j]) for j in diff[:5]])


# ---- (b) the kernel on the emulator --------------------------------------------------------------------------------------------------

_EMU_CODE = r'''
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ssw_amd
from parity import compare_batch, make_reads
from sswutil import dna_matrix, random_ref
lib = ssw_amd.load(%r)
ctx = ssw_amd.Context(0, lib)
half_on = os.environ.get("SSW_GPU_FILL_HALF") != "0"
check = os.environ.get("FILL_HALF_CHECK", "1") == "1"
rng = np.random.default_rng(5)
ref = random_ref(int(os.environ["FILL_HALF_REFLEN"]), 77, 4)
ref[2000:2300] = np.tile(np.array([0, 2], dtype=np.int8), 150)            # a low-complexity stretch
CLASSES = {1: (1, 6, 8), 3: (17, 22, 24), 13: (97, 101, 104), 19: (145, 150, 152), 23: (177, 181, 184)}
NEIGHBOURS = (140, 144, 160)
recs = []
def run(reads, scoring, flag, want):
    match, mism, gO, gE = scoring
    mat = dna_matrix(match, mism)
    Q = ctx.upload(reads); T = ctx.upload([ref])
    res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
    name = ctx.timing()["fill_kernel"]
    Q.free(); T.free()
    assert name.startswith(want if half_on or not want.startswith("k_fill8<") else "k_fill<"), (name, want, [len(r) for r in reads])
    recs.append((res.tobytes(), np.asarray(cig).tobytes()))
    if check:
        bad = compare_batch(res, cig, reads, [ref], mat, 5, gO, gE, flag, 0, 0, -1, 2)
        assert not bad, "%%s flag %%d lens %%s: " %% (scoring, flag, [len(r) for r in reads]) + "\n".join(bad)
for scoring in ((2, 2, 3, 1), (1, 3, 5, 2)):
    for flag in (0, 1, 2):
        for R8, lens in CLASSES.items():
            for nr in (1, 2, 3):
                reads = make_reads(rng, ref, nr, lens[nr %% 3:] + lens[:nr %% 3], 4, frac_random=0.0)
                run(reads, scoring, flag, "k_fill8<%%d,frame>" %% R8)                 # the class alone: one bucket, the half-row kernel
        # every class and the ineligible neighbours in one batch (155: ineligible, in the padded-length class of 150): the buckets side by
        # side in one grid of 16-lane chains, then one after the other -- each eligible bucket on the half-row kernel
        mixed = make_reads(rng, ref, 14, [150, 6, 140, 22, 144, 101, 160, 181, 155, 152, 17, 8, 184, 145], 4, frac_random=0.0)
        run(mixed, scoring, flag, "k_fill<")
        os.environ["SSW_GPU_SERIAL_BUCKETS"] = "1"                                 # (the hooks are read at every call)
        run(mixed, scoring, flag, "k_fill8<")
        del os.environ["SSW_GPU_SERIAL_BUCKETS"]
        run(make_reads(rng, ref, 3, NEIGHBOURS, 4, frac_random=0.0), scoring, flag, "k_fill<")
ctx.close()
import hashlib
print("ok", len(recs), hashlib.sha256(b"".join(a + b for a, b in recs)).hexdigest())
'''


def _emu_run(emu_lib_path, reflen, check=True, **env):
    code = _EMU_CODE % (PKG, HERE, emu_lib_path)
    e = dict(os.environ, SSW_GPU_NO_DB="1", FILL_HALF_REFLEN=str(reflen), FILL_HALF_CHECK="1" if check else "0", **env)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=3000)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.split()[2]


@pytest.fixture(scope="module")
def half_digest(emu_lib_path):
    """run 1: a target of several kilobases that the small-call rule cuts into many tiles (seams and halos), every record against the
    reference; the digest of all records is what the other runs must reproduce"""
    return _emu_run(emu_lib_path, 6400)


def test_half_row_kernel_on_the_emulator_against_the_reference(half_digest):
    assert len(half_digest) == 64


@pytest.mark.parametrize("K", ["16", "64"])
def test_half_row_kernel_renormalises_inside_a_scan(emu_lib_path, half_digest, K):
    """run 2: the frame drops every 16 / 64 steps -- inside the flush's window and T scan; every record against the reference again"""
    assert _emu_run(emu_lib_path, 6400, SSW_GPU_FRAME_K=K) == half_digest


def test_records_identical_to_the_16_lane_kernel(emu_lib_path, half_digest):
    """run 3: SSW_GPU_FILL_HALF=0 forces k_fill everywhere; byte-identical records and CIGARs"""
    assert _emu_run(emu_lib_path, 6400, check=False, SSW_GPU_FILL_HALF="0") == half_digest
