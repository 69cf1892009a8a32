"""Cases of tests/test_fill8_scorings.py: the deterministic generator of the random sweep over k_fill8's scoring space, the documented
contract of the kernel's name, and a plain Smith-Waterman in numpy that takes any matrix and models a null column."""
import numpy as np

from parity import make_reads

SEED = 20811
CHUNKS = 12
PER_CHUNK = 96                                                  # 8 cases per chunk for every R = 1 .. 12, that is R8 = 1, 3, .. 23
GAP_E = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
GAP_D = (1, 2, 3, 7, 40)                                        # gapO - gapE
ALPHABETS = (4, 5, 8, 16, 24, 32)
KINDS = ("pm2e", "gate", "pm20", "nonpos", "max127")
NEG = -10 ** 9


def r8_of(L):
    return (L + 7) // 8


def _matrix(rng, n, lo, hi, dlo, dhi):
    """entries uniform in [lo, hi], the diagonal uniform in [dlo, dhi]; clipped to int8"""
    m = rng.integers(max(lo, -128), min(hi, 127) + 1, size=(n, n))
    m[np.diag_indices(n)] = rng.integers(dlo, min(dhi, 127) + 1, size=n)
    return np.ascontiguousarray(m.astype(np.int8).reshape(-1))


def sweep_case(seed, index):
    """(seed, index) -> case, a dict: reads, target, mat, n, gapO, gapE, flag, score_size, R8, kind.  Case i of a chunk has R = 1 + i % 12 and
    a = i // 12; over the twelve chunks every (R, a) meets every gapE once.  Per chunk: the three ways of drawing the matrix by turns, two
    cases of R <= 3 with max(mat) of 40 to 127 and one all-non-positive matrix, on another R in every chunk."""
    chunk, i = divmod(index, PER_CHUNK)
    R, a = 1 + i % 12, i // 12
    rng = np.random.default_rng([seed, index])
    gE = GAP_E[(a + 5 * (R - 1) + chunk) % 12]
    gO = gE + int(rng.choice(GAP_D))
    n = int(rng.choice(ALPHABETS))
    kind = KINDS[(a + chunk + R) % 3]
    if a == 7 and R - 1 == chunk % 12:
        kind = "nonpos"
    elif a in (5, 6) and R <= 3:
        kind = "max127"
    if kind == "pm2e":
        mat = _matrix(rng, n, -(2 * gE + 2), 2 * gE + 2, 1, 2 * gE + 2)
    elif kind == "gate":
        mat = _matrix(rng, n, -2 * gE, 11, 1, 11)
    elif kind == "pm20":
        mat = _matrix(rng, n, -20, 20, 1, 20)
    elif kind == "nonpos":
        mat = _matrix(rng, n, -(2 * gE + 2), 0, -3, 0)
    else:
        top = int(rng.choice((40, 90, 127)))
        lo = -2 * gE - (2 if a == 5 else 0)                     # (a = 5: mostly beyond the gate, a = 6: inside it)
        mat = _matrix(rng, n, lo, 11, 1, top)
        mat[int(rng.integers(0, n)) * (n + 1)] = top
    target = rng.integers(0, n, size=int(rng.integers(700, 801)), dtype=np.int8)
    nr = int(rng.integers(1, 5))
    lens = [16 * (R - 1) + int(x) for x in rng.integers(1, 9, size=nr)]
    reads = make_reads(rng, target, nr, lens, n, frac_random=0.1)
    return dict(reads=reads, target=target, mat=mat, n=n, gapO=gO, gapE=gE, flag=int(rng.integers(0, 3)), score_size=int(rng.choice((2, 2, 0, 1))),
                R8=2 * R - 1, kind=kind, index=index)


def fill8_name(R8, mat, gapE, codes, n):
    """the documented contract of the fill kernel's name (DESIGN.md "Gaps from the diagonal"): the half-row kernel of the frame form, in the
    diagonal-gap form exactly where no matrix entry is below -2 gapE, the instance has the form and no target code lies outside [0, n)"""
    codes = np.asarray(codes)
    dg = -int(np.min(mat)) <= 2 * gapE and R8 not in (9, 17) and (codes.size == 0 or (int(codes.min()) >= 0 and int(codes.max()) < n))
    return "k_fill8<%d,frame>%s" % (R8, " dg" if dg else "")


def plain_sw(read, target, mat, n, gO, gE):
    """Smith-Waterman with affine gaps in int64, row by row, gapO > gapE >= 1: (best score, its first column, its first row in that column;
    -1, -1 when the score is 0).  A target code outside [0, n) makes a null column: its cells have no diagonal candidate -- H there is
    max(0, E, F), and gaps pass through it."""
    mat = np.asarray(mat, dtype=np.int64).reshape(n, n)
    t = np.asarray(target, dtype=np.int64)
    m = len(t)
    inside = (t >= 0) & (t < n)
    tc = np.where(inside, t, 0)
    j = np.arange(m, dtype=np.int64)
    Hp = np.zeros(m, dtype=np.int64)
    F = np.full(m, NEG, dtype=np.int64)
    best, bcol, brow = 0, -1, -1
    for i, b in enumerate(read):
        s = np.where(inside, mat[tc, int(b)], NEG)
        F = np.maximum(F - gE, Hp - gO)
        diag = np.concatenate(([0], Hp[:-1])) + s
        h0 = np.maximum(np.maximum(diag, F), 0)                 # H without the horizontal gap: a gap never opens from a gap (gapO > gapE)
        run = np.maximum.accumulate(h0 + j * gE)                # E(j) = max over k < j of h0(k) - gapO - (j - 1 - k) gapE
        E = np.concatenate(([NEG], run[:-1] - gO - (j[1:] - 1) * gE))
        Hp = np.maximum(h0, E)
        top = int(Hp.max())
        col = int(np.argmax(Hp))
        if top > best or (top == best and top > 0 and col < bcol):
            best, bcol, brow = top, col, i
    return best, bcol, brow
