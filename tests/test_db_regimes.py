"""Regime and boundary parity of the fused database-search kernel (k_filldb) and of its host planner (align_db, csrc/ssw_host.c).

Every case goes four ways through ONE helper (_db_ways): (a) Context.align_batch at flag 0 over the targets (or a sub-range of them), (b)
Context.search_db in chunks chosen per case (one that splits the targets unevenly and 1 are always among them) where the call is
streamable, (c) Context.search_topk with k = the number of targets and min_score 1, (d) -- where the case asks for it -- align_batch at
flag 2 with a `filters` value that separates the case's pairs.  (a) must equal parity.expected() -- the compiled reference -- for EVERY
(query, target): all RES_FIELDS, status 1 exactly where the reference returns NULL; n_word / n_byte of the timing record must equal the
counts that follow from the reference's scores (status 0, score1 > 0; score1 >= 255 - bias decides, src/ssw.c:881-899) and `cells` the sum
of readLen x refLen.  (b) must equal (a) in the five hit fields (ref_end2 -2 where (a) has status 1), (c) must list (a)'s eligible targets
by score descending, then index ascending, with records equal field for field, (d) must equal the reference in all fields and in every CIGAR
word with status 0 or 1 only (the kernel's SSW_OUT_WORD mark never reaches the caller).  The helper also asserts WHICH path answered: it
evaluates the envelope of align_batch_locked -- gapO > gapE, n <= 32, max(mat) <= 49, at least four targets, the longest at most 65 000
columns, queries of 1..384 residues or of 385..640 with n x 10 x 256 <= 65535 -- and wants fill_kernel "k_filldb<..." inside and anything
else outside; a call whose queries lie on both sides is also run as two calls, one per side, which must give the same rows and the path of
their side (the mixed call itself reports whichever kernel filled most cells).  A call without a single cell (all targets or all queries
empty) launches nothing and names no kernel.  Where a case is built to reach a value (a last-column ref_end1, a score of exactly 255 - bias,
a NULL, a far ref_end2) the assertion is made on the REFERENCE's answer first.

Families: 1 workgroup tail and target order; 2 unequal chains; 3 the column limit 64 999 / 65 000 / 65 001; 4 launch cuts and the result
layouts (direct, sub-batched, hits, top-k); 5 the 8-bit / 16-bit decision, NULL, the padded rule and the mask edges of the second best;
6 ties and the chain-best filter; 7 the alphabet, matrix and gap gates.  Every family runs on the CPU SIMT emulator (tests/emu: the real
host driver and the real kernel source; `not gpu`) and on the MI355X (`gpu`).  A k_filldb workgroup always steps sixteen chains through its
longest target and an emulated call costs 0.15 s before its first cell, so the emulator half runs a cover of each family -- what it leaves
out is named at each family -- and the gpu half runs every case.

Running time, one session, same machine, emulator library already built, the two modules in turn: `pytest -m "not gpu"
tests/test_pairs_regimes.py` 34.9 s and 31.3 s; `pytest -m "not gpu" tests/test_db_regimes.py` 52.0 s and 52.0 s -- below twice the former.
That bound sets the emulator cover: every call of the library costs the emulator 0.15 .. 0.25 s before its first cell and every chunk of
way (b) 0.2 s more (chunks of one target over seventeen targets: 3.3 s), so the emulator half keeps chunks of one target for the cases
of three to five targets.  `pytest -m gpu tests/test_db_regimes.py` on an MI355X: 12 tests in 4 s
(profiles/db_regimes_gpu_tests_mi355x.log).  Sensitivity (seven one-token mutants of filldb_pass) is recorded in docs/NOTEBOOK.md, "k_filldb at its limits"."""
import os

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, cigar_str, dna_matrix

FIELDS = list(ssw_amd.RESULT_DTYPE.names)
HIT_FIELDS = ("score1", "score2", "ref_end1", "read_end1", "ref_end2")
FAST = "k_filldb<"
NCH = 16      # chains (targets) of a k_filldb workgroup (SSW_DB_NCH)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the one helper

_REF = {}      # the reference's answers, computed once per (read, target, scoring) and shared by every test and both halves


def _ref(rd, tg, mat, n, gapO, gapE, flag, filters, ml, ss):
    key = (rd.tobytes(), tg.tobytes(), mat.tobytes(), n, gapO, gapE, flag, filters, ml, ss)
    if key not in _REF:
        _REF[key] = expected(rd, mat, n, tg, gapO, gapE, flag, filters, 0, ml, ss)
    return _REF[key]


def query_inside(qlen, n):
    return 1 <= qlen <= 384 or (385 <= qlen <= 640 and n * 10 * 256 <= 65535)


def call_inside(tlens, n, mat, gapO, gapE, min_targets=4):
    """the gates of align_batch_locked that hold for the call as a whole (ssw_gpu_search_db streams below four targets too: min_targets 0)"""
    return bool(gapO > gapE and n <= 32 and int(np.max(mat)) <= 49 and len(tlens) >= min_targets and max(tlens) <= 65000)


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def _check_ref(tag, res, cig, reads, targets, tf, ref, bad, with_cigar):
    for q in range(len(reads)):
        for k in range(res.shape[1]):
            exp, ecig = ref[q][k]
            g = res[q, k]
            if exp is None:
                ok = int(g["status"]) == 1
            else:
                ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp and (not with_cigar or _cig(g, cig) == ecig)
            if not ok and len(bad) < 6:
                bad.append("%s: read %d (%d residues) x target %d (%d columns): reference %s %s, got %s %s" % (
                    tag, q, len(reads[q]), tf + k, len(targets[tf + k]), exp, cigar_str(ecig), g, cigar_str(_cig(g, cig))))


def _counts(ref_rows, reads, tlens, mat, ss):
    """(n_word, n_byte, cells) as they follow from the reference's answers"""
    minmat = int(np.min(mat))
    bias = -minmat if minmat < 0 else 0
    scored = [e["score1"] for row in ref_rows for e, _ in row if e is not None and e["score1"] > 0]
    n_word = sum(1 for s in scored if ss == 1 or (ss == 2 and s >= 255 - bias))
    return n_word, len(scored) - n_word, sum(len(r) for r in reads) * sum(tlens)


def _same_records(tag, a, b, bad, fields=FIELDS):
    a, b = np.asarray(a), np.asarray(b)
    for idx in np.ndindex(a.shape):
        if any(int(a[idx][f]) != int(b[idx][f]) for f in fields) and len(bad) < 6:
            bad.append("%s %s: %s against %s" % (tag, idx, a[idx], b[idx]))


def _db_ways(ctx, reads, targets, mat, n, gapO=3, gapE=1, maskLen=-1, score_size=2, target_first=0, target_count=None, chunks=None,
             topk=True, flagged=None, sides=True, chunk1=True):
    """reads x targets[target_first : target_first + target_count] the four ways of the module docstring.
    chunks: targets per chunk of way (b) -- 1 is added; None: no way (b); flagged: the `filters` of way (d), None: no way (d);
    topk / sides / chunk1:
    False leaves way (c) / the per-side calls of a mixed call / the chunk size 1 of way (b) out (emulator covers: a chunk is a launch group
    of its own, 0.2 s on the emulator)
    -> (ref [q][k] of (dict | None, cigar) in range order, records of (a), timing of (a), {layout name: (n_word, n_byte, cells)})"""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    reads = [np.ascontiguousarray(r, dtype=np.int8) for r in reads]
    targets = [np.ascontiguousarray(t, dtype=np.int8) for t in targets]
    tf = target_first
    tc = len(targets) - tf if target_count is None else target_count
    sub = tf != 0 or tc != len(targets)
    kw = dict(gapO=gapO, gapE=gapE, maskLen=maskLen, score_size=score_size)
    ml = [maskLen if maskLen >= 0 else len(r) // 2 for r in reads]

    def ref_of(t0, t1, flag=0, filters=0):
        return [[_ref(rd, targets[t], mat, n, gapO, gapE, flag, filters, ml[q], score_size) for t in range(t0, t1)] for q, rd in enumerate(reads)]

    def path_of(qs, tlens, min_targets=4):
        """True: k_filldb must have answered, False: must not, None: the call's queries lie on both sides, "": no cell, no kernel"""
        if sum(len(reads[q]) for q in qs) * sum(tlens) == 0:
            return ""
        if not call_inside(tlens, n, mat, gapO, gapE, min_targets):
            return False
        inside = set(query_inside(len(reads[q]), n) for q in qs if len(reads[q]) > 0)
        return inside.pop() if len(inside) == 1 else None

    def assert_path(who, want, tm):
        if want == "":
            assert tm["fill_kernel"] == "", (who, tm["fill_kernel"])
        elif want is not None:
            assert tm["fill_kernel"].startswith(FAST) == want, (who, want, tm["fill_kernel"])

    ref = ref_of(tf, tf + tc)
    tlens = [len(t) for t in targets[tf:tf + tc]]
    all_q = list(range(len(reads)))
    counts = {}
    bad = []
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        # (a) full records at flag 0, against the reference
        ares, acig = ctx.align_batch(Q, T, mat, n, flag=0, target_first=tf, target_count=tc, **kw)
        atm = ctx.timing()
        _check_ref("align_batch", ares, acig, reads, targets, tf, ref, bad, True)
        assert not bad, "\n".join(bad)
        counts["batch"] = (atm["n_word"], atm["n_byte"], atm["cells"])
        assert counts["batch"] == _counts(ref, reads, tlens, mat, score_size), (counts["batch"], _counts(ref, reads, tlens, mat, score_size))
        want = path_of(all_q, tlens)
        assert_path("align_batch", want, atm)
        if want is None and sides:      # queries on both sides of the gate: each side as a call of its own
            for side in (True, False):
                qs = [q for q in all_q if len(reads[q]) == 0 or query_inside(len(reads[q]), n) == side]
                S = ctx.upload([reads[q] for q in qs])
                try:
                    sres, _ = ctx.align_batch(S, T, mat, n, flag=0, target_first=tf, target_count=tc, **kw)
                    assert_path("align_batch, one side", path_of(qs, tlens), ctx.timing())
                finally:
                    S.free()
                _same_records("one side against the mixed call", sres, ares[qs], bad)
        # whole-set records for (b) and (c), which take no sub-range
        if sub:
            fres, fcig = ctx.align_batch(Q, T, mat, n, flag=0, **kw)
            _check_ref("align_batch, all targets", fres, fcig, reads, targets, 0, ref_of(0, len(targets)), bad, True)
            _same_records("sub-range against all targets", ares, fres[:, tf:tf + tc], bad)
        else:
            fres = ares
        assert not bad, "\n".join(bad)
        all_tlens = [len(t) for t in targets]
        # (b) the streamed search, where the fused kernel streams
        if chunks is not None and path_of(all_q, all_tlens, 0) is True:
            nt = len(targets)
            for chunk in sorted(set(list(chunks) + ([1] if chunk1 else []))):
                hits = ctx.search_db(Q, T, mat, n, gapO, gapE, maskLen, score_size, chunk)
                htm = ctx.timing()
                assert htm["fill_kernel"].startswith(FAST), htm["fill_kernel"]
                for f in HIT_FIELDS:
                    w = np.where(fres["status"] == 1, -2, fres[f]) if f == "ref_end2" else fres[f]
                    assert (hits[f] == w).all(), ("search_db", chunk, f, np.argwhere(hits[f] != w)[:4].tolist())
                counts["hits/%d" % chunk] = (htm["n_word"], htm["n_byte"], htm["cells"])
            assert any(c < nt and nt % c for c in chunks), "no chunk size splits the targets unevenly"
        # (c) the best k = all targets per query
        if topk:
            nt = len(targets)
            ti, tres, _ = ctx.search_topk(Q, T, nt, mat, n, flag=0, min_score=1, **kw)
            ttm = ctx.timing()
            pad = np.zeros((), dtype=ssw_amd.RESULT_DTYPE); pad["ref_begin1"] = pad["read_begin1"] = -1; pad["cigar_off"] = -1
            for q in all_q:
                elig = [t for t in range(nt) if int(fres[q, t]["status"]) == 0 and int(fres[q, t]["score1"]) >= 1]
                elig.sort(key=lambda t: (-int(fres[q, t]["score1"]), t))
                assert [int(x) for x in ti[q]] == elig + [-1] * (nt - len(elig)), ("search_topk", q, ti[q].tolist(), elig)
                for r, t in enumerate(elig):
                    _same_records("search_topk query %d slot %d" % (q, r), tres[q, r], fres[q, t], bad)
                for r in range(len(elig), nt):
                    _same_records("search_topk query %d padding slot %d" % (q, r), tres[q, r], pad, bad)
            if path_of(all_q, all_tlens, 0) is True:
                counts["topk"] = (ttm["n_word"], ttm["n_byte"], ttm["cells"])
        # (d) flag 2 behind a score filter
        if flagged is not None:
            dref = ref_of(tf, tf + tc, 2, flagged)
            dres, dcig = ctx.align_batch(Q, T, mat, n, flag=2, filters=flagged, target_first=tf, target_count=tc, **kw)
            dtm = ctx.timing()
            assert set(np.unique(dres["status"]).tolist()) <= {0, 1}, np.unique(dres["status"])
            _check_ref("align_batch flag 2 filters %d" % flagged, dres, dcig, reads, targets, tf, dref, bad, True)
            assert_path("align_batch flag 2", path_of(all_q, tlens), dtm)
            with_cigar = sum(1 for row in dref for e, _ in row if e is not None and e["cigarLen"] > 0)
            scored = sum(1 for row in dref for e, _ in row if e is not None and e["score1"] > 0)
            assert 0 < with_cigar < scored, ("the filter does not separate the pairs", with_cigar, scored)
        assert not bad, "\n".join(bad)
    finally:
        Q.free(); T.free()
    return ref, ares, atm, counts


def _rand(rng, L, ncodes=4):
    return rng.integers(0, ncodes, size=int(L), dtype=np.int8)


def _subst(seq, rng, count, ncodes=4, lo=0):
    """`count` substitutions at distinct places from `lo` on (lengths stay)"""
    r = np.array(seq, dtype=np.int8)
    hit = lo + rng.choice(len(r) - lo, size=count, replace=False)
    r[hit] = (r[hit] + 1 + rng.integers(0, ncodes - 1, size=count)) % ncodes
    return r


class _env(object):
    """test hooks of the emulator and hooks libraries (read at every call), set for one block"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k in self.kv:
            del os.environ[k]


# ------------------------------------------------------------------------------------------------------------------ 1 workgroup tail, target order

def _tail_case(nt, seed):
    """nt targets of 20..90 columns in shuffled order, lengths repeated (the sort falls back to the index); five reads: pieces of the first,
    the middle and the last target of 30, 40 and 21 residues, a random one of 17 and one of 33 -- classes R = 2 (three queries: an odd
    number, qb = -1) and R = 3 (two)"""
    rng = np.random.default_rng(9100 + seed)
    lens = rng.choice([20, 33, 47, 48, 64, 90], size=nt)
    lens[0], lens[nt // 2], lens[-1] = 64, 48, 90
    targets = [_rand(rng, L) for L in lens]
    reads = [targets[0][10:40].copy(), targets[nt // 2][5:45].copy(), targets[-1][69:].copy(), _rand(rng, 17), _rand(rng, 33)]
    return reads, targets


def _wg_tail(ctx, emu):
    """target counts 3 and 4 (the routing switch, at flag 2 as well), 15, 16, 17, 32, 33 (a full workgroup, one chain more, one fewer);
    one empty target in the middle, all targets empty, one empty query, a sub-range target_first = 3.
    Emulator: counts 15, 16, 17 (the empty and sub-range cases have seventeen targets) and 32 left out; way (d) at 3 and 4 targets and
    with the sub-range only, chunks of one target at 3 and 4 targets only"""
    for nt in (3, 4, 33) if emu else (3, 4, 15, 16, 17, 32, 33):
        reads, targets = _tail_case(nt, nt)
        ref, res, tm, _ = _db_ways(ctx, reads, targets, dna_matrix(2, 2), 5, chunks=(nt - 1, 16) if nt > 16 else (nt - 1,),
                                   flagged=30 if nt in (3, 4) or not emu else None, chunk1=nt in (3, 4) or not emu)
        assert ref[0][0][0]["score1"] == 60 and ref[2][nt - 1][0]["score1"] == 42 and ref[2][nt - 1][0]["ref_end1"] == 89
        assert tm["fill_kernel"].startswith(FAST) == (nt >= 4)
    reads, targets = _tail_case(17, 1)
    e = np.zeros(0, dtype=np.int8)
    # an empty target in the middle and an empty query; the same through a sub-range that starts at target 3
    t2 = targets[:5] + [e] + targets[6:]
    ref, res, tm, _ = _db_ways(ctx, reads[:2] + [e] + reads[2:], t2, dna_matrix(2, 2), 5, chunks=(5,), flagged=None if emu else 30, chunk1=not emu)
    assert all(row[5][0]["score1"] == 0 for row in ref) and all(x[0]["score1"] == 0 and x[0]["ref_begin1"] == -1 for x in ref[2])
    _db_ways(ctx, reads, t2, dna_matrix(2, 2), 5, target_first=3, target_count=9, chunks=(5,), flagged=30, chunk1=not emu)
    _db_ways(ctx, reads, t2, dna_matrix(2, 2), 5, target_first=3, target_count=3, topk=False)      # three targets of seventeen: not fused
    # all targets empty / all queries empty: no launch
    ref, res, tm, _ = _db_ways(ctx, reads, [e] * 5, dna_matrix(2, 2), 5, chunks=(3,), topk=not emu)
    assert tm["fill_kernel"] == "" and (res["score1"] == 0).all() and (res["ref_begin1"] == -1).all()
    _db_ways(ctx, [e, e], targets[:5], dna_matrix(2, 2), 5, chunks=(3,), topk=not emu)


def test_emu_workgroup_tail_and_target_order(ectx):
    _wg_tail(ectx, True)


@pytest.mark.gpu
def test_gpu_workgroup_tail_and_target_order(gpu_ctx):
    _wg_tail(gpu_ctx, False)


# ------------------------------------------------------------------------------------------------------------------ 2 unequal chains

SHORT_COLS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49]
QL_ALL = [1, 15, 16, 17, 384, 385, 640]      # classes R = 1 (three queries), 2, 24, and the `mid` buckets 25 and 40


def _unequal_chains(ctx, tlong, qlens, emu):
    """ONE workgroup: targets of 1 .. 49 columns next to one of `tlong`; every read is a suffix of one 640-residue sequence, every short
    target a suffix of it too, so that their common suffix ends in the target's LAST column; the long target starts with the last 41
    residues: its best cell lies in column 40 and is kept over the tlong - 41 steps that follow.
    Emulator: the queries of up to 17 residues against a long target of 1 000 columns instead of 5 000, those of 384, 385 and 640 against
    one of 120 (R = 24, 25 and 40 cost the emulator as many times a row class of one); way (d) and chunks of one target left out"""
    rng = np.random.default_rng(9200)
    base = _rand(rng, 640)
    long_t = np.concatenate([base[-41:], _rand(rng, tlong - 41)])
    targets = [base[640 - c:].copy() for c in SHORT_COLS[:5]] + [long_t] + [base[640 - c:].copy() for c in SHORT_COLS[5:]]
    order = rng.permutation(len(targets))
    targets = [targets[i] for i in order]
    reads = [base[640 - L:].copy() for L in qlens]
    # (match 2, mismatch 4, gaps 10 / 2: unrelated stretches of a 640-residue read and 5 000 random columns stay far below the planted 82)
    ref, res, tm, _ = _db_ways(ctx, reads, targets, dna_matrix(2, 4), 5, 10, 2, chunks=(5,), flagged=None if emu else 60, chunk1=not emu)
    for q, L in enumerate(qlens):
        for k, t in enumerate(targets):
            e = ref[q][k][0]
            if len(t) == tlong:
                assert e["score1"] == 2 * min(L, 41) and (L < 15 or (e["ref_end1"] == 40 and e["read_end1"] == L - 1)), (L, e)
            elif L >= 15:      # (a target of one or two columns matches the read in many rows: the column is certain, the row is not)
                assert e["score1"] == 2 * min(L, len(t)) and e["ref_end1"] == len(t) - 1 and (len(t) < 15 or e["read_end1"] == L - 1), (L, len(t), e)
    assert tm["fill_kernel"].startswith(FAST)


def test_emu_unequal_chains(ectx):
    _unequal_chains(ectx, 1000, QL_ALL[:4], True)
    _unequal_chains(ectx, 120, QL_ALL[4:], True)


@pytest.mark.gpu
def test_gpu_unequal_chains(gpu_ctx):
    _unequal_chains(gpu_ctx, 5000, QL_ALL, False)


# ------------------------------------------------------------------------------------------------------------------ 3 column limit

def _limit_case(L):
    """four targets, the longest of L columns: the 640-residue read's exact copy ends in its LAST column, a copy with three substitutions
    (one of them in its last 17 residues) ends in column 40 639; the 17-residue read is the long one's tail.  Match 2, mismatch 4, gaps
    10 / 2, maskLen 15: the second best is decided 24 000 columns away from the best end, above the shoulder of the best alignment
    (16 columns before its end: 32 less) and above what 65 000 random columns give a 17-residue read"""
    rng = np.random.default_rng(9300)
    rd = _rand(rng, 640)
    t = _rand(rng, L)
    t[L - 640:] = rd
    second = _subst(rd[:623], rng, 2)
    t[40000:40623] = second
    t[40623:40640] = rd[623:]
    t[40626] = (t[40626] + 1) % 4
    targets = [_rand(rng, 300), t, rd[600:].copy(), _rand(rng, 30)]
    return [rd, rd[623:].copy()], targets


def _check_limit(ref, L, qlens=(640, 17)):
    for q, ql in enumerate(qlens):
        e = ref[q][1][0]
        assert e["score1"] == 2 * ql and e["ref_end1"] == L - 1 and e["read_end1"] == ql - 1, (ql, e)
        assert e["score2"] > 0 and 32768 < e["ref_end2"] < 40640, (ql, e)


def _column_limit(ctx, lengths):
    for L in lengths:
        reads, targets = _limit_case(L)
        ref, res, tm, _ = _db_ways(ctx, reads, targets, dna_matrix(2, 4), 5, 10, 2, maskLen=15, chunks=(3,), flagged=1000)
        _check_limit(ref, L)
        assert tm["fill_kernel"].startswith(FAST) == (L <= 65000)


def _column_limit_stand_in(ctx):
    """the emulator's stand-in: the same plants in a 5 000-column target (last column; second best beyond column 3 000), the 17-residue
    read and a 48-residue one (R = 3) -- a 640-residue class steps forty rows per lane through every column; way (c) and chunks of one target left out"""
    rng = np.random.default_rng(9350)
    L = 5000
    rd = _rand(rng, 48)
    t = _rand(rng, L)
    t[L - 48:] = rd
    t[3000:3048] = rd
    t[3020] = (t[3020] + 1) % 4
    t[3034] = (t[3034] + 1) % 4
    targets = [_rand(rng, 300), t, rd[20:].copy(), _rand(rng, 30)]
    ref, res, tm, _ = _db_ways(ctx, [rd, rd[31:].copy()], targets, dna_matrix(2, 4), 5, 10, 2, maskLen=15, chunks=(3,), flagged=60, topk=False, chunk1=False)
    for q, ql in enumerate((48, 17)):
        e = ref[q][1][0]
        assert e["score1"] == 2 * ql and e["ref_end1"] == L - 1 and e["score2"] > 0 and 3000 < e["ref_end2"] < 3048, (ql, e)


def test_emu_column_limit(ectx):
    """Emulator: the 5 000-column stand-in; 64 999 / 65 000 / 65 001 columns are left to the gpu half (sixteen chains x 65 000 steps x 40
    rows per lane do not fit the module's time on the emulator)"""
    _column_limit_stand_in(ectx)


@pytest.mark.gpu
def test_gpu_column_limit(gpu_ctx):
    _column_limit(gpu_ctx, (64999, 65000, 65001))


@pytest.mark.gpu
def test_gpu_column_limit_forced_forms(gpu_hctx):
    """65 000 columns in the frame form renormalised every 16 and every 64 steps and in the plain int16 form: equal records"""
    reads, targets = _limit_case(65000)
    got = []
    for env in ({"SSW_GPU_FRAME_K": 16}, {"SSW_GPU_FRAME_K": 64}, {"SSW_GPU_DB_FORM": 0}):
        with _env(**env):
            ref, res, tm, _ = _db_ways(gpu_hctx, reads, targets, dna_matrix(2, 4), 5, 10, 2, maskLen=15, chunks=(3,))
        assert tm["fill_kernel"].startswith(FAST) and tm["fill_kernel"].endswith("int16+max3>" if "SSW_GPU_DB_FORM" in env else "frame>"), tm["fill_kernel"]
        got.append(res)
    _check_limit(ref, 65000)
    bad = []
    _same_records("K = 64 against K = 16", got[1], got[0], bad)
    _same_records("int16 against K = 16", got[2], got[0], bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ 4 launch cuts, layouts

DB_STREAMS = 4      # csrc/ssw_host.c


def _plan(budget, maxt, npairs, nz):
    """align_db's cut of one size class into launches -> (pairs per launch, targets per launch)"""
    stride = (maxt + 15) // 16 * 16 + 16
    sl = budget // 2 // (2 * DB_STREAMS) // 16 * 16
    need = max(min(4 * stride * nz * npairs, sl), 4 * stride * NCH)
    ppl = max(1, min(npairs, need // (4 * stride * NCH)))
    per = max(NCH, need // (4 * stride * ppl) // NCH * NCH)
    return ppl, per


def _cuts_case(extra, tmax):
    """33 targets of 40..tmax columns and one of 1 200, seven reads of three classes (R = 1: three, R = 2: two, R = 3: two), each a piece of a target"""
    rng = np.random.default_rng(9400)
    lens = [int(x) for x in rng.integers(40, tmax, size=33)]
    lens[7], lens[20] = 1200, 40
    targets = [_rand(rng, L) for L in lens]
    reads = [targets[k][5:5 + L].copy() for k, L in ((0, 16), (7, 12), (13, 9), (20, 30), (32, 21), (7, 48), (3, 35))]
    reads[5] = targets[7][1152:].copy()      # ends in the last column of the longest target
    return reads + extra(rng, targets), targets


def _launch_cuts(ctx_factory, emu, extra=lambda rng, targets: [], mat=None, n=5, gapO=3, gapE=1, ncodes=4, filters=40):
    """a 1 MiB scratch budget on the case's own context: one pair and sixteen targets per launch -- the p0 loop runs once per pair, the k0
    loop three times, its last launch with ONE target; SSW_GPU_DB_TSUB 16 and 5: chunks of 16 + 16 + 1 and 6 x 5 + 3 targets through the
    sub-batched d_res layout and its host conversion.  All layouts: equal records, equal n_word / n_byte / cells.
    Emulator: all targets but the longest below 150 columns instead of 1 100, chunks of 16 targets only in way (b), way (d) left out
    (tests/test_search_db_flags.py runs it in chunks of three targets there); a mixed call (never in the direct layout: its long query's
    rows come later) under SSW_GPU_DB_TSUB = 16 only, way (a) alone -- the per-side calls of a mixed call run in the gate family there"""
    reads, targets = _cuts_case(extra, 150 if emu else 1100)
    mixed = not all(query_inside(len(r), n) for r in reads)
    if ncodes != 4:
        rng = np.random.default_rng(9450)
        targets = [_rand(rng, len(t), ncodes) for t in targets]
        src = [(5 * k) % 33 if len(targets[(5 * k) % 33]) >= 3 + len(r) else 7 for k, r in enumerate(reads)]
        reads = [targets[t][3:3 + len(r)].copy() for t, r in zip(src, reads)]
    mat = dna_matrix(2, 2) if mat is None else mat
    assert _plan(1 << 20, 1200, 2, 33) == (1, 16) and 33 % 16 == 1
    ctx = ctx_factory()
    try:
        ctx.lib.ssw_gpu_set_budget(ctx.h, 1 << 20)
        runs = {}
        for tsub in (16,) if emu and mixed else (0, 16, 5):
            with _env(**({"SSW_GPU_DB_TSUB": tsub} if tsub else {})):
                runs[tsub] = _db_ways(ctx, reads, targets, mat, n, gapO, gapE, chunks=None if tsub else (16,) if emu else (16, 5), topk=tsub == 0,
                                      chunk1=not emu, flagged=None if emu else filters,
                                      sides=not emu)
        first = min(runs)
        ref, direct, tm, counts = runs[first]
        assert ncodes != 4 or (ref[5][7][0]["ref_end1"] == 1199 and ref[5][7][0]["score1"] == 96)
        bad = []
        for tsub in sorted(set(runs) - {first}):
            _same_records("SSW_GPU_DB_TSUB %d against the direct layout" % tsub, runs[tsub][1], direct, bad)
            counts["tsub%d" % tsub] = runs[tsub][3]["batch"]
            assert runs[tsub][2]["fill_launches"] == tm["fill_launches"] - 1 + -(-33 // tsub), (tsub, runs[tsub][2]["fill_launches"], tm["fill_launches"])
        assert not bad, "\n".join(bad)
        assert len(set(counts.values())) == 1, counts
        return counts
    finally:
        ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        ctx.close()


def _gate26_mat():
    rng = np.random.default_rng(9460)
    mat = rng.integers(-6, 7, size=(26, 26)).astype(np.int8)
    np.fill_diagonal(mat, rng.integers(3, 9, size=26))
    return np.ascontiguousarray(mat.reshape(-1))


def test_emu_launch_cuts_and_layouts(ectx):
    counts = _launch_cuts(lambda: ssw_amd.Context(0, ectx.lib), True)
    assert set(counts) == {"batch", "hits/16", "topk", "tsub16", "tsub5"}


@pytest.mark.gpu
def test_gpu_launch_cuts_and_layouts(gpu_hctx):
    counts = _launch_cuts(lambda: ssw_amd.Context(0, gpu_hctx.lib), False)
    assert set(counts) == {"batch", "hits/1", "hits/5", "hits/16", "topk", "tsub16", "tsub5"}


def _long_query(rng, targets):
    return [np.concatenate([targets[7][:650], _rand(rng, 50)])]      # 700 residues: any_long -- rows of mixed origin, not streamable


def test_emu_launch_cuts_mixed_origin(ectx):
    """Emulator: the 700-residue repeat only; n = 26 with a 400-residue query runs in the alphabet-gate family there"""
    _launch_cuts(lambda: ssw_amd.Context(0, ectx.lib), True, extra=_long_query)


@pytest.mark.gpu
def test_gpu_launch_cuts_mixed_origin(gpu_hctx):
    _launch_cuts(lambda: ssw_amd.Context(0, gpu_hctx.lib), False, extra=_long_query)
    # n = 26: 26 x 10 x 256 > 65535 -- the 400-residue query takes the per-target path, the short ones stay fused
    _launch_cuts(lambda: ssw_amd.Context(0, gpu_hctx.lib), False, extra=lambda rng, targets: [np.zeros(400, dtype=np.int8)], mat=_gate26_mat(), n=26,
                 gapO=10, gapE=2, ncodes=26, filters=150)      # (the reads are redrawn from the 26-letter targets, the eighth with 400 residues)


# ------------------------------------------------------------------------------------------------------------------ 5 byte / word, NULL, second best

def _byte_word_decision(ctx, tcols, emu):
    """match 1, mismatch x: bias = x; exact copies of 255 - x - 1, 255 - x and 255 - x + 1 residues score their length: 254, 255 and
    256 - bias.  score_size 0: NULL (status 1; ref_end2 -2 in the hits) from 255 - x on.  Five targets: one per read and two unrelated.
    Emulator: x = 1 only, chunks of one target at score_size 2 only, way (c) at score_size 0 and 2"""
    rng = np.random.default_rng(9500)
    for x in (1,) if emu else (1, 3):
        lens = [255 - x - 1, 255 - x, 255 - x + 1]
        targets = [_rand(rng, tcols - 7 * k) for k in range(5)]
        reads = [targets[k + 1][11 + k:11 + k + L].copy() for k, L in enumerate(lens)]
        for ss in (0, 1, 2):
            ref, res, tm, _ = _db_ways(ctx, reads, targets, dna_matrix(1, x), 5, score_size=ss, chunks=(3,), flagged=200 if ss == 2 else None,
                                       chunk1=ss == 2 or not emu, topk=ss != 1 or not emu)
            for k, L in enumerate(lens):
                if ss == 0 and L >= 255 - x:
                    assert ref[k][k + 1][0] is None and int(res[k, k + 1]["status"]) == 1
                else:
                    assert ref[k][k + 1][0]["score1"] == L
            assert (tm["n_word"], tm["n_byte"]) == {0: (0, 13), 1: (15, 0), 2: (2, 13)}[ss], (ss, tm["n_word"], tm["n_byte"])


def test_emu_byte_word_decision(ectx):
    _byte_word_decision(ectx, 300, True)


@pytest.mark.gpu
def test_gpu_byte_word_decision(gpu_ctx):
    _byte_word_decision(gpu_ctx, 1500, False)


def _pads(L):
    """rows below the read under byte rules and under word rules (segments of 16 and of 8 rows, src/ssw.c:148 / 197)"""
    return -L % 16, -L % 8


def _padded_second_best(ctx, emu):
    """word rules (match 2: an exact copy of 256 residues overflows 8 bits), reads of 256 + {0, 1, 8, 9} residues: len & 15 = 0, 1, 8, 9.
    The reference's column maximum runs over the rows of the PADDED read, and a score reached in the read's last row travels on through
    the pad rows, one column per row: 16 R - len of them under byte rules, 8 fewer under word rules where len & 15 is 1..8 (the kernel's
    other tap, o8).  maskLen = len + 40; a second copy with substitutions ends pw + 4 columns before the first column behind the mask:
    its last-row score reaches that column under byte padding and stops short of it under word padding -- only its last eight rows
    separate the two maxima.  Way (d): filters 520 lies above the word-decided 512 and 514 of the two shorter reads -- non-survivors
    decided under word rules come back with status 0.
    Emulator: the read of 256 residues (no pad rows under either rule) in the call of way (d) only, which has all four; the other calls
    with their one read; way (c) and chunks of one target left out"""
    rng = np.random.default_rng(9550)
    reads, targets, plant = [], [], []
    for d in (0, 1, 8, 9):
        L = 256 + d
        pb, pw = _pads(L)
        assert pb - pw == (8 if 1 <= (L & 15) <= 8 else 0)
        rd = _rand(rng, L)
        gap = 36 - pw      # the second copy's last column is bc + maskLen - (pw + 4)
        second = _subst(rd, rng, 6, lo=0)
        second[-20:] = rd[-20:]           # its last rows match: the score in its last row is its best
        targets.append(np.concatenate([_rand(rng, 30 + d), rd, _rand(rng, gap), second, _rand(rng, 60)]))
        reads.append(rd)
        plant.append((30 + d + L - 1, _ref(rd, second, dna_matrix(2, 2), 5, 3, 1, 0, 0, L + 40, 2)[0]["score1"]))
    targets.append(_rand(rng, 200))
    for q, rd in enumerate(reads):
        if emu and q == 0:
            continue
        others = reads[:q] + reads[q + 1:]      # (maskLen is the call's: one call per read, the read first)
        ref, res, tm, _ = _db_ways(ctx, [rd] + (others[:0] if emu and q != 3 else others), targets, dna_matrix(2, 2), 5, maskLen=len(rd) + 40,
                                   chunks=(3,), flagged=520 if q == 3 else None, topk=not emu, chunk1=not emu)
        e = ref[0][q][0]
        bc, s = plant[q]
        assert e["score1"] == 2 * len(rd) and e["ref_end1"] == bc, e
        assert 0 < e["score2"] < s and e["ref_end2"] >= bc + len(rd) + 40, (e, s)      # the second copy's end, and what the pad rows carry on, is masked
        assert tm["n_word"] >= 1


def test_emu_padded_second_best(ectx):
    _padded_second_best(ectx, True)


@pytest.mark.gpu
def test_gpu_padded_second_best(gpu_ctx):
    _padded_second_best(gpu_ctx, False)


def _mask_edges(ctx, emu):
    """a 12-residue read over {A, C, G}; targets: T-runs around its exact copy and a copy of its first eight residues (score 16, falling
    by 2 per column on either side) that ends d = maskLen - 1, maskLen, maskLen + 1 columns before / after the best end.  Byte rules mask
    [bc - maskLen, bc + maskLen], word rules (score_size 1) one column fewer on the upper side (src/ssw.c:376 against 578): the expected
    score2 / ref_end2 are worked out here and asserted on the reference first.  One target whose best ends 5 columns before its end
    (bc + maskLen beyond the target).  maskLen 15 and 14 (no second best: score2 0, ref_end2 -1).
    Emulator: nothing left out"""
    rng = np.random.default_rng(9570)
    rd = np.array([0, 1, 2, 2, 0, 1, 1, 2, 0, 2, 1, 0], dtype=np.int8)
    part = rd[:8]
    run = lambda k: np.full(k, 3, dtype=np.int8)
    targets, want = [], {}
    M = 15
    for d in (M - 1, M, M + 1):
        # after: [run 20][read][run d - 8][part][run 30] -- bc = 31, the part ends in column bc + d
        targets.append(np.concatenate([run(20), rd, run(d - 8), part, run(30)]))
        # before: [run 20][part][run d - 12][read][run 30] -- the part ends in column 27, bc = 27 + d
        targets.append(np.concatenate([run(20), part, run(d - 12), rd, run(30)]))
    targets.append(np.concatenate([part, run(32), rd, run(5)]))      # (and the eight residues at its start: the second best)
    for ss in (2, 1):
        ref, res, tm, _ = _db_ways(ctx, [rd, part.copy()], targets, dna_matrix(2, 2), 5, maskLen=M, score_size=ss, chunks=(4,))
        for k, d in enumerate((M - 1, M, M + 1)):
            after, before = ref[0][2 * k][0], ref[0][2 * k + 1][0]
            assert after["score1"] == 24 and after["ref_end1"] == 31 and before["score1"] >= 24 and before["ref_end1"] == 27 + d, (after, before)
            first = 31 + M + (0 if ss == 1 else 1)      # first column behind the mask
            assert (after["score2"], after["ref_end2"]) == (16 - 2 * max(0, first - (31 + d)), max(first, 31 + d)), (ss, d, after)
            assert (before["score2"], before["ref_end2"]) == (16 - 2 * max(0, M + 1 - d), 27 + d - M - 1 if d <= M else 27), (ss, d, before)
        e = ref[0][6][0]
        assert e["ref_end1"] == 51 and e["score1"] == 24 and (e["score2"], e["ref_end2"]) == (16, 7)
        assert (tm["n_word"] > 0) == (ss == 1)
    ref, res, tm, _ = _db_ways(ctx, [rd, part.copy()], targets, dna_matrix(2, 2), 5, maskLen=14, chunks=(4,), topk=not emu)
    assert all(e["score2"] == 0 and e["ref_end2"] == -1 for row in ref for e, _ in row if e["score1"] > 0)


def test_emu_mask_edges(ectx):
    _mask_edges(ectx, True)


@pytest.mark.gpu
def test_gpu_mask_edges(gpu_ctx):
    _mask_edges(gpu_ctx, False)


# ------------------------------------------------------------------------------------------------------------------ 6 ties, chain-best filter

def _ties_case(Rs, tlens):
    """homopolymer, period-2 and period-3 reads of 16 R and 16 R - 7 residues against like targets of `tlens` columns (the
    period-3 ones with a foreign residue in the middle); and a 32-residue read (R = 2) of an A-run in rows 0..9 (lanes 0..4) and a C-run in
    rows 10..19 (lanes 5..9) against targets that hold the two runs 60 columns apart, in both orders: the same maximum in two columns more
    than 48 apart, the earlier one in the higher lane and in the lower lane.  And the order of STEPS against the order of columns: lane l
    stands in column s - l at step s, so a lane far down reaches an earlier column later than a lane high up reached a later one.  A read with
    an A-run in rows 0..5 (it ends in lane 2) and a C-run in rows 20..25 (lane 12) against C C C C C C T A A A A A A from column 17 on: 12 is
    reached in column 29 at step 31 and in column 22 at step 34, and between them, at step 32, every lane learns the chain's best.  Only
    because the lanes are told one LESS than the chain's best does lane 12 still record the tie that wins (the earlier column)"""
    reads, targets = [], []
    for period in (1, 2, 3):
        unit = np.arange(period, dtype=np.int8)
        for R in Rs:
            reads += [np.resize(unit, 16 * R).astype(np.int8), np.resize(unit, 16 * R - 7).astype(np.int8)]
        for tl in tlens:
            t = np.resize(unit, tl).astype(np.int8)
            if period == 3:
                t[tl // 2] = 3
            targets.append(t)
    a, c, g, t3 = (np.full(60, k, dtype=np.int8) for k in range(4))
    reads.append(np.concatenate([a[:10], c[:10], g[:12]]))
    targets += [np.concatenate([t3[:7], c[:10], t3[:50], a[:10], t3[:5]]), np.concatenate([t3[:7], a[:10], t3[:50], c[:10], t3[:5]])]
    reads.append(np.concatenate([a[:6], g[:14], c[:6], g[:6]]))
    targets.append(np.concatenate([t3[:17], c[:6], t3[:1], a[:6], t3[:40]]))
    return reads, targets


def _ties(ctx, Rs, emu, hooks):
    """hooks: also with SSW_GPU_DB_CHAIN_BEST=0 -- the same records.  Emulator: R = 1 and 3 (the gpu half adds R = 24), targets of 65, 80,
    100 and 130 columns instead of 65, 100, 130 and 333, way (d) and chunks of one target left out"""
    reads, targets = _ties_case(Rs, (65, 80, 100, 130) if emu else (65, 100, 130, 333))
    got = []
    for env in ({}, {"SSW_GPU_DB_CHAIN_BEST": 0}) if hooks else ({},):
        with _env(**env):
            ref, res, tm, _ = _db_ways(ctx, reads, targets, dna_matrix(2, 2), 5, chunks=(4,), topk=not env, flagged=None if emu or env else 50, chunk1=not emu)
        got.append(res)
    # the first column that holds the maximum wins: a homopolymer read inside a longer homopolymer target ends at column len - 1
    for q in range(2 * len(Rs)):
        for k in range(4):
            if len(reads[q]) <= len(targets[k]):
                assert ref[q][k][0]["score1"] == 2 * len(reads[q]) and ref[q][k][0]["ref_end1"] == len(reads[q]) - 1
    for k, row in ((12, 19), (13, 9)):
        e = ref[-2][k][0]
        assert e["score1"] == 20 and e["ref_end1"] == 16 and e["read_end1"] == row, e
    e = ref[-1][14][0]
    assert (e["score1"], e["ref_end1"], e["read_end1"]) == (12, 22, 25), e
    assert any(e["score2"] > 0 for row in ref for e, _ in row) and tm["fill_kernel"].startswith(FAST)
    if hooks:
        bad = []
        _same_records("chain-best filter off against on", got[1], got[0], bad)
        assert not bad, "\n".join(bad)


def test_emu_ties_and_chain_best(ectx):
    _ties(ectx, (1, 3), True, True)


@pytest.mark.gpu
def test_gpu_ties(gpu_ctx):
    _ties(gpu_ctx, (1, 3, 24), False, False)


@pytest.mark.gpu
def test_gpu_ties_chain_best_off(gpu_hctx):
    _ties(gpu_hctx, (1, 3, 24), False, True)


# ------------------------------------------------------------------------------------------------------------------ 7 gates

def _gate_case(ctx, n, mm, gapO, gapE, tcols, emu):
    """queries of 384 and 385 residues (and one of 20) against five targets; the path assertion of _db_ways decides what must have run"""
    rng = np.random.default_rng(9700 + n)
    nc = min(n, 20) if n != 5 else 4
    mat = rng.integers(-8, 9, size=(n, n)).astype(np.int8)
    np.fill_diagonal(mat, rng.integers(2, 9, size=n))
    mat[0, 0] = mm
    mat = np.ascontiguousarray(mat.reshape(-1))
    targets = [_rand(rng, tcols - 11 * k, nc) for k in range(5)]
    reads = [_subst(targets[0][3:387], rng, 20, nc), _subst(targets[1][2:387], rng, 20, nc), targets[2][7:27].copy()]
    ref, res, tm, _ = _db_ways(ctx, reads, targets, mat, n, gapO, gapE, chunks=(3,), topk=not emu, flagged=None if emu else 600, chunk1=not emu)
    inside = [gapO > gapE and n <= 32 and mm <= 49 and (L <= 384 or n <= 25) for L in (384, 385, 20)]
    if all(inside) or not any(inside):
        assert tm["fill_kernel"].startswith(FAST) == all(inside), (n, mm, gapO, gapE, tm["fill_kernel"])
    return tuple(inside)


def _gates(ctx, tcols, emu):
    """n = 24, 25, 26, 32, 33; max(mat) 49 and 50; gapO = gapE + 1 and gapO = gapE.
    Emulator: n = 26 (the 385-residue query leaves, the 384-residue one stays; family 2 runs 385 and 640 residues inside) and 33,
    max(mat) and gapO = gapE at n = 5 (gapO = gapE + 1 left out); 400-column targets, ways (c) and (d) and chunks of one target left out"""
    seen = set()
    for n in (26, 33) if emu else (24, 25, 26, 32, 33):
        seen.add(_gate_case(ctx, n, 9, 10, 2, tcols, emu))
    for mm in (49, 50):
        seen.add(_gate_case(ctx, 5, mm, 10, 2, tcols, emu))
    for gapO in (2,) if emu else (3, 2):
        seen.add(_gate_case(ctx, 5, 9, gapO, 2, tcols, emu))
    assert seen == {(True, True, True), (True, False, True), (False, False, False)}, seen


def test_emu_gates(ectx):
    _gates(ectx, 400, True)


@pytest.mark.gpu
def test_gpu_gates(gpu_ctx):
    _gates(gpu_ctx, 900, False)
