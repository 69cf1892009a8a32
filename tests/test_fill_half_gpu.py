"""Half-row fill chains (k_fill8) on the device: the shapes of tests/test_fill_half.py (b) through the product library, and a batch of
150-bp reads against a 200-kb target that is decided under both the 16-bit and the 8-bit rules (the latter read the closed form of the
padded rows).  tests/test_full_size.py runs the same kernel over all 100 000 reads of config 2."""
import numpy as np
import pytest

from parity import compare_batch, make_reads
from sswutil import dna_matrix, random_ref, sample_reads

pytestmark = pytest.mark.gpu

CLASSES = {1: (1, 6, 8), 3: (17, 22, 24), 13: (97, 101, 104), 19: (145, 150, 152), 23: (177, 181, 184)}
NEIGHBOURS = (140, 144, 160)
MIXED = [150, 6, 140, 22, 144, 101, 160, 181, 155, 152, 17, 8, 184, 145]


@pytest.fixture(scope="module")
def target():
    ref = random_ref(6400, 77, 4)
    ref[2000:2300] = np.tile(np.array([0, 2], dtype=np.int8), 150)
    return ref


def _run(ctx, reads, ref, scoring, flag, want):
    match, mism, gO, gE = scoring
    mat = dna_matrix(match, mism)
    Q = ctx.upload(reads); T = ctx.upload([ref])
    try:
        res, cig = ctx.align_batch(Q, T, mat, 5, gO, gE, flag, 0, 0, -1, 2)
    finally:
        Q.free(); T.free()
    tm = ctx.timing()
    assert tm["fill_kernel"].startswith(want), (tm["fill_kernel"], want, [len(r) for r in reads])
    bad = compare_batch(res, cig, reads, [ref], mat, 5, gO, gE, flag, 0, 0, -1, 2)
    assert not bad, "%s flag %d lens %s: " % (scoring, flag, [len(r) for r in reads]) + "\n".join(bad)
    return tm


@pytest.mark.parametrize("scoring", [(2, 2, 3, 1), (1, 3, 5, 2)], ids=["2_2_3_1", "1_3_5_2"])
@pytest.mark.parametrize("flag", [0, 1, 2])
def test_eligible_classes_alone_and_among_ineligible_neighbours(gpu_ctx, gpu_hctx, monkeypatch, target, scoring, flag):
    rng = np.random.default_rng(5 + flag)
    for R8, lens in CLASSES.items():
        for nr in (1, 2, 3):      # a lone read, a full pair, a second chain with a lone read
            reads = make_reads(rng, target, nr, lens[nr % 3:] + lens[:nr % 3], 4, frac_random=0.0)
            _run(gpu_ctx, reads, target, scoring, flag, "k_fill8<%d,frame>" % R8)
    mixed = make_reads(rng, target, len(MIXED), MIXED, 4, frac_random=0.0)
    _run(gpu_ctx, mixed, target, scoring, flag, "k_fill<")                # buckets side by side: one grid of 16-lane chains
    _run(gpu_ctx, make_reads(rng, target, 3, NEIGHBOURS, 4, frac_random=0.0), target, scoring, flag, "k_fill<")
    monkeypatch.setenv("SSW_GPU_SERIAL_BUCKETS", "1")                     # (a hook of libssw_hooks.so, read at every call)
    _run(gpu_hctx, mixed, target, scoring, flag, "k_fill8<")              # one after the other: the eligible buckets on the half-row kernel


@pytest.mark.parametrize("flag", [0, 2])
def test_150bp_reads_against_200kb_under_both_rules(gpu_ctx, flag):
    ref = random_ref(200000, 9, 4)
    reads = sample_reads(ref, 256, 150, seed=21)
    tm = _run(gpu_ctx, reads, ref, (2, 2, 3, 1), flag, "k_fill8<19,frame>")
    assert tm["n_word"] > 0 and tm["n_byte"] > 0, (tm["n_word"], tm["n_byte"])
