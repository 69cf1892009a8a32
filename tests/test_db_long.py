"""The long class of the database path (dbl_class / dbl_chunk, csrc/ssw_host.c): queries above k_filldb's classes -- 641 residues and
more, 385 and more where n x 10 x 256 > 65535 -- against four or more targets on the strip kernel's pair mode.  A job is (q, ta, q, tb):
both register halves hold the same query against two neighbours of the chunk's length-sorted targets; k_dbjobs builds the jobs on the
device and k_reduce_pairs (database mode) stores the records in the chunk's matrix beside k_filldb's, in the layout the call needs.

Every case goes through ONE helper (_ways): align_batch at flag 0 must equal parity.expected() -- the compiled reference -- in all
RES_FIELDS, status 1 exactly where the reference returns NULL; search_db hits (every chunk size asked for) and search_topk lists (every k
asked for) must equal what follows from those records; flagged align_batch calls must equal the reference in all fields and every CIGAR
word, CIGARs in (query, target) order.  The helper also asserts the PATH: db_long_pairs = (queries of the class) x (non-empty targets),
where the class is evaluated by a mirror of the host's gate (_in_class), and fill_launches = the number of target chunks -- one launch
group per chunk however many targets it holds (the per-target loop the class replaces launches at least once per target).  Cases that
run one strip shape assert fill_kernel against a mirror of win_bucket_shape (_shape) and of ssw_frame_params (_frame).

Families: 1 gate and strip shapes (DNA), 2 proteins and the alphabet gate, 3 rules, 4 mixed call, 5 streamed search, 6 flags, 7 budget.
Each has an emulator half (`not gpu`: the real host driver and kernel source on the SIMT emulator, 5..13 targets of 0..~400 columns) and
a GPU half (the same cases plus a few dozen targets).  Every target set holds an empty target, a 1-column target, two targets of equal
length and an odd number of non-empty targets."""
import os

import numpy as np
import pytest

import ssw_amd
from parity import expected
from sswutil import RES_FIELDS, blosum50, cigar_str, dna_matrix

HIT_FIELDS = ("score1", "score2", "ref_end1", "read_end1", "ref_end2")
FIELDS = list(ssw_amd.RESULT_DTYPE.names)


@pytest.fixture(scope="module")
def ectx(emu_lib_path):
    ctx = ssw_amd.Context(0, ssw_amd.load(emu_lib_path))
    yield ctx
    ctx.close()


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


# ------------------------------------------------------------------------------------------------------------------ the planner, mirrored

def _shape(qlen, n):
    """win_geom_fill / win_bucket_key / win_bucket_shape of csrc/ssw_host.c -> (rows per lane, strips, rows per lane of a tail strip or 0)"""
    x = min(max(24 // (n + 1), 1), 3)
    xr = 4 * x
    while xr > 4 and n * ((xr + 3) // 4) * 1024 > 65535:
        xr -= 4
    P = -(-qlen // 16) * 16
    S = -(-P // (64 * xr))
    R, tail = -(-P // (64 * S)), 0
    if S > 1 and xr > 4:
        rem = P - (S - 1) * 64 * xr
        need = -(-rem // 64)
        tr = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 0
        if rem > 0 and tr > 0 and xr * (S - 1) + tr < R * S:
            R, tail = xr, tr
    return R, S, tail


def _frame(qlen, mat, gapO, gapE):
    """ssw_frame_params for a 64-lane chain of ceil16(qlen) rows: the column-frame form fits"""
    top = -(-qlen // 16) * 16 * max(int(np.max(mat)), 0)
    K = 1024
    while K > 64 and K * gapE > 4096:
        K >>= 1
    b = max(-int(np.min(mat)), 0) + gapO + 2 * gapE + 8
    while K > 64 and top + b + (K + 66) * gapE >= 31744:
        K >>= 1
    return top + b + (K + 66) * gapE < 31744


def _kname(qlen, n, form):
    R, S, tail = _shape(qlen, n)
    return "k_chainq<%d,pairs,%s> x %d strips" % (R, form, S - 1 if tail else S) + (" + 1 of %d" % tail if tail else "")


def _job_bytes(tl, strips):
    return 8 * ((tl + 15) // 16 * 16 + 16) + 16 * ((tl + 31) // 16 * 16) + 36 * strips + 32 + 2 * ssw_amd.RESULT_DTYPE.itemsize


def _in_filldb(qlen, n):
    return 1 <= qlen <= 384 or (385 <= qlen <= 640 and n * 10 * 256 <= 65535)


def _in_class(qlen, n, maxt, budget):
    """the membership rule of the long class, for a call that is on the database path"""
    return 385 <= qlen <= 65535 and not _in_filldb(qlen, n) and _job_bytes(maxt, _shape(qlen, n)[1]) <= budget // 2


# ------------------------------------------------------------------------------------------------------------------ the one helper

_REF = {}      # the reference's answers, computed once per (read, target, scoring) and shared by every test and both halves


def _ref(rd, tg, mat, n, gapO, gapE, flag, filters, ml, ss):
    key = (rd.tobytes(), tg.tobytes(), mat.tobytes(), n, gapO, gapE, flag, filters, ml, ss)
    if key not in _REF:
        _REF[key] = expected(rd, mat, n, tg, gapO, gapE, flag, filters, 0, ml, ss)
    return _REF[key]


def _cig(rec, pool):
    off, ln = int(rec["cigar_off"]), int(rec["cigarLen"])
    return [int(x) for x in pool[off:off + ln]] if ln > 0 else []


def _check_ref(tag, res, cig, reads, targets, ref, bad, mark=False):
    for q in range(len(reads)):
        for k in range(len(targets)):
            exp, ecig = ref[q][k]
            g = res[q, k]
            if exp is None:
                ok = int(g["status"]) == 1
            elif mark:      # mark_mismatch rewrites the CIGAR (M -> = / X, soft clips): positions and scores stay the reference's
                ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS if f != "cigarLen"} == {f: v for f, v in exp.items() if f != "cigarLen"}
            else:
                ok = int(g["status"]) == 0 and {f: int(g[f]) for f in RES_FIELDS} == exp and _cig(g, cig) == ecig
            if not ok and len(bad) < 6:
                bad.append("%s: read %d (%d residues) x target %d (%d columns): reference %s %s, got %s %s" % (
                    tag, q, len(reads[q]), k, len(targets[k]), exp, cigar_str(ecig), g, cigar_str(_cig(g, cig))))


def _same_records(tag, a, b, bad, fields=FIELDS):
    a, b = np.asarray(a), np.asarray(b)
    for idx in np.ndindex(a.shape):
        if any(int(a[idx][f]) != int(b[idx][f]) for f in fields) and len(bad) < 6:
            bad.append("%s %s: %s against %s" % (tag, idx, a[idx], b[idx]))


def _cigar_order(res):
    """cigar_off of the records that have a CIGAR: the CIGARs tile the pool without gap or overlap, those of one query in target order
    (the pool of a database call is written survivor by survivor: geometry bucket, query, target); -1 where there is none -> words"""
    spans = []
    for q in range(res.shape[0]):
        last = -1
        for g in res[q]:
            if int(g["cigarLen"]) > 0:
                assert int(g["cigar_off"]) > last, (q, int(g["cigar_off"]), last)
                last = int(g["cigar_off"])
                spans.append((last, int(g["cigarLen"])))
            else:
                assert int(g["cigar_off"]) == -1
    at = 0
    for off, ln in sorted(spans):
        assert off == at, (off, at)
        at += ln
    return at


def _ways(ctx, reads, targets, mat, n, gapO=3, gapE=1, maskLen=-1, score_size=2, chunks=(), ks=(), flags=(), form=None, kname_of=None,
          budget=0):
    """flags: (flag, filters, mark_mismatch) triples of flagged align_batch calls; chunks: targets per chunk of search_db; ks: the k of
    search_topk at flag 0; kname_of: the query length whose strip shape must name the call; form: "frame" / "int16" where the case forces one;
    budget: the scratch budget of the calls (0: the default).  -> (reference [q][t], records at flag 0, timing at flag 0)"""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    reads = [np.ascontiguousarray(r, dtype=np.int8) for r in reads]
    targets = [np.ascontiguousarray(t, dtype=np.int8) for t in targets]
    nt = len(targets)
    tlens = [len(t) for t in targets]
    nz = sum(1 for L in tlens if L > 0)
    assert nt >= 4 and gapO > gapE and n <= 32 and int(np.max(mat)) <= 49 and max(tlens) <= 65000      # the call is on the database path
    assert 0 in tlens and 1 in tlens and nz % 2 == 1 and len(set(L for L in tlens if L > 1)) < sum(1 for L in tlens if L > 1), tlens
    ml = [maskLen if maskLen >= 0 else len(r) // 2 for r in reads]

    def ref_of(flag=0, filters=0):
        return [[_ref(rd, tg, mat, n, gapO, gapE, flag, filters, ml[q], score_size) for tg in targets] for q, rd in enumerate(reads)]

    kw = dict(gapO=gapO, gapE=gapE, maskLen=maskLen, score_size=score_size)
    bad = []
    Q = ctx.upload(reads); T = ctx.upload(targets)
    try:
        ctx.lib.ssw_gpu_set_budget(ctx.h, budget)
        bytes_ = int(ctx.lib.ssw_gpu_get_budget(ctx.h))
        member = [_in_class(len(r), n, max(tlens), bytes_) for r in reads]
        want_pairs = sum(member) * nz
        ref = ref_of()
        res, cig = ctx.align_batch(Q, T, mat, n, flag=0, **kw)
        tm = ctx.timing()
        _check_ref("align_batch", res, cig, reads, targets, ref, bad)
        assert not bad, "\n".join(bad)
        assert len(cig) == 0 and (res["cigar_off"] == -1).all()
        print("align_batch: db_long_pairs %s (want %d), fill_launches %d, fill_kernel %s" % (tm.get("db_long_pairs"), want_pairs, tm["fill_launches"], tm["fill_kernel"]))
        assert tm["db_long_pairs"] == want_pairs, (tm["db_long_pairs"], want_pairs)
        if all(m or _in_filldb(len(r), n) or len(r) == 0 for m, r in zip(member, reads)):
            assert tm["fill_launches"] == 1, tm["fill_launches"]      # one launch group for the one chunk: no per-target loop
        if kname_of is not None:
            forms = (form,) if form else ("frame",) if _frame(kname_of, mat, gapO, gapE) else ("int16",)
            assert tm["fill_kernel"] in [_kname(kname_of, n, f) for f in forms], (tm["fill_kernel"], _kname(kname_of, n, forms[0]))
        scored = [(q, t) for q in range(len(reads)) for t in range(nt) if ref[q][t][0] is not None and ref[q][t][0]["score1"] > 0]
        assert tm["n_word"] + tm["n_byte"] == len(scored) and tm["cells"] == sum(len(r) for r in reads) * sum(tlens)
        # the streamed search: hits of every chunk size equal the batch records
        for chunk in chunks:
            hits = ctx.search_db(Q, T, mat, n, gapO, gapE, maskLen, score_size, chunk)
            htm = ctx.timing()
            for f in HIT_FIELDS:
                w = np.where(res["status"] == 1, -2, res[f]) if f == "ref_end2" else res[f]
                assert (hits[f] == w).all(), ("search_db", chunk, f, np.argwhere(hits[f] != w)[:4].tolist())
            nchunks = -(-nt // chunk) if chunk > 0 else 1
            print("search_db chunk %d: db_long_pairs %s, fill_launches %d" % (chunk, htm.get("db_long_pairs"), htm["fill_launches"]))
            assert htm["db_long_pairs"] == want_pairs and htm["fill_launches"] == nchunks, (chunk, htm["db_long_pairs"], htm["fill_launches"])
        # the best k per query: by score descending, then target index
        for k in ks:
            ti, tres, _ = ctx.search_topk(Q, T, k, mat, n, flag=0, min_score=1, **kw)
            ttm = ctx.timing()
            pad = np.zeros((), dtype=ssw_amd.RESULT_DTYPE); pad["ref_begin1"] = pad["read_begin1"] = -1; pad["cigar_off"] = -1
            for q in range(len(reads)):
                elig = [t for t in range(nt) if int(res[q, t]["status"]) == 0 and int(res[q, t]["score1"]) >= 1]
                elig.sort(key=lambda t: (-int(res[q, t]["score1"]), t))
                elig = elig[:k]
                assert [int(x) for x in ti[q]] == elig + [-1] * (k - len(elig)), ("search_topk", k, q, ti[q].tolist(), elig)
                for r, t in enumerate(elig):
                    _same_records("search_topk k %d query %d slot %d" % (k, q, r), tres[q, r], res[q, t], bad)
                for r in range(len(elig), k):
                    _same_records("search_topk k %d query %d padding slot %d" % (k, q, r), tres[q, r], pad, bad)
            print("search_topk k %d: db_long_pairs %s, reduce_ms %g" % (k, ttm.get("db_long_pairs"), ttm["reduce_ms"]))
            assert ttm["db_long_pairs"] == want_pairs and ttm["reduce_ms"] > 0, (k, ttm["db_long_pairs"], ttm["reduce_ms"])      # the device selected
        # flagged calls: the pairs that pass src/ssw.c:916 through one batched reverse pass and traceback
        for flag, filters, mark in flags:
            fref = ref_of(flag, filters)
            fres, fcig = ctx.align_batch(Q, T, mat, n, flag=flag, filters=filters, mark_mismatch=mark, **kw)
            ftm = ctx.timing()
            assert set(np.unique(fres["status"]).tolist()) <= {0, 1}, np.unique(fres["status"])
            _check_ref("align_batch flag %d filters %d mark %d" % (flag, filters, mark), fres, fcig, reads, targets, fref, bad, mark)
            assert _cigar_order(fres) == len(fcig)
            print("align_batch flag %d: db_long_pairs %s, fill_launches %d" % (flag, ftm.get("db_long_pairs"), ftm["fill_launches"]))
            assert ftm["db_long_pairs"] == want_pairs, (flag, ftm["db_long_pairs"], want_pairs)
            if flag == 2 and filters > 0:
                with_cigar = sum(1 for row in fref for e, _ in row if e is not None and e["cigarLen"] > 0)
                assert 0 < with_cigar < len(scored), ("the filter does not separate the pairs", with_cigar, len(scored))
        assert not bad, "\n".join(bad)
    finally:
        ctx.lib.ssw_gpu_set_budget(ctx.h, 0)
        Q.free(); T.free()
    return ref, res, tm


# ------------------------------------------------------------------------------------------------------------------ the cases

def _rand(rng, L, ncodes=4):
    return rng.integers(0, ncodes, size=int(L), dtype=np.int8)


def _mutate(rng, seq, rate, ncodes):
    out = seq.copy()
    hit = rng.random(len(out)) < rate
    out[hit] = (out[hit] + rng.integers(1, ncodes, size=int(hit.sum()))) % ncodes
    return out


def _targets(rng, count, maxcols, ncodes=4):
    """count targets: an empty one (two when count is odd: the number of non-empty targets is odd), one column, two of equal length, the
    rest of 2..maxcols columns with maxcols among them, in shuffled order"""
    nempty = 2 if count % 2 else 1
    lens = [1, maxcols, maxcols // 2, maxcols // 2] if count - nempty >= 4 else [1, maxcols, maxcols]      # (five targets: three non-empty ones)
    lens = lens + [int(x) for x in rng.integers(2, maxcols, size=count - nempty - len(lens))] + [0] * nempty
    assert len(lens) == count
    order = rng.permutation(len(lens))
    return [_rand(rng, lens[i], ncodes) for i in order]


def _read(rng, L, targets, ncodes=4, rate=0.08):
    """L residues: a mutated copy of the longest target, an exact copy of the next one, pieces of others and random filler"""
    by_len = sorted(targets, key=lambda t: -len(t))
    parts = [_rand(rng, 7 + L % 5, ncodes), _mutate(rng, by_len[0], rate, ncodes), _rand(rng, 11, ncodes), by_len[1].copy(), _rand(rng, 5, ncodes)]
    parts += [by_len[k][:max(len(by_len[k]) // 2, 1)].copy() for k in range(2, min(len(by_len), 5))]
    rd = np.concatenate(parts)
    if len(rd) < L:
        rd = np.concatenate([rd, _rand(rng, L - len(rd), ncodes)])
    return np.ascontiguousarray(rd[:L])


# ---- 1 gate and strip shapes, DNA

DNA_LENS = (640, 641, 704, 705, 768, 769, 1600, 2000)


def _gate_and_shapes(ctx, emu):
    """640 stays in k_filldb<40>; 641..704 one strip of 11 rows per lane, 705..768 of 12; 769 twelve rows + a tail strip of 1; 1 600 two
    strips of 12 + a tail strip of 1 (25 rows per lane against 27 of three balanced strips of 9); 2 000 three balanced strips of 11.  Every
    length as a call of its own (the shape names the call), then all of them against 5 and 13 targets (GPU: and 37): the same fill_launches"""
    rng = np.random.default_rng(4101)
    mat = dna_matrix(2, 2)
    t5 = _targets(rng, 5, 300 if emu else 400)
    assert [_shape(L, 5) for L in DNA_LENS[1:]] == [(11, 1, 0), (11, 1, 0), (12, 1, 0), (12, 1, 0), (12, 2, 1), (12, 3, 1), (11, 3, 0)]
    for L in DNA_LENS:
        rd = _read(rng, L, t5)
        ref, res, tm = _ways(ctx, [rd], t5, mat, 5, kname_of=L if L > 640 else None, form="frame" if L > 640 else None)
        if L == 640:
            assert tm["fill_kernel"].startswith("k_filldb<40,") and tm["db_long_pairs"] == 0
        else:
            assert tm["fill_strips"] == _shape(L, 5)[1] and tm["fill_rows_per_lane"] == _shape(L, 5)[0]
    launches = []
    for count in (5, 13) if emu else (5, 13, 37):
        tg = t5 if count == 5 else _targets(rng, count, 200 if emu else 400)
        reads = [_read(rng, L, tg) for L in ((641, 769) if emu else DNA_LENS)]
        launches.append(_ways(ctx, reads, tg, mat, 5)[2]["fill_launches"])
    assert len(set(launches)) == 1, launches


def test_emu_gate_and_shapes(ectx):
    _gate_and_shapes(ectx, True)


@pytest.mark.gpu
def test_gpu_gate_and_shapes(gpu_ctx):
    _gate_and_shapes(gpu_ctx, False)


# ---- 2 proteins, the alphabet gate

def _gate26_mat():
    rng = np.random.default_rng(9460)
    mat = rng.integers(-6, 7, size=(26, 26)).astype(np.int8)
    np.fill_diagonal(mat, rng.integers(3, 9, size=26))
    return np.ascontiguousarray(mat.reshape(-1))


def _proteins(ctx, emu):
    """BLOSUM50, n = 24 (four rows per lane: 641 residues are three strips, 1 000 four) under gaps 10/2 and 3/1; n = 26: a 400-residue query
    is in the class (two strips), a 384-residue one in k_filldb<24>"""
    rng = np.random.default_rng(4201)
    tg = _targets(rng, 7, 160 if emu else 350, 20)
    assert _shape(641, 24) == (4, 3, 0) and _shape(1000, 24) == (4, 4, 0) and _shape(400, 26) == (4, 2, 0)
    for gapO, gapE in ((10, 2), (3, 1)):
        for L in (641, 1000):
            _ways(ctx, [_read(rng, L, tg, 20, 0.2)], tg, blosum50(), 24, gapO, gapE, kname_of=L, chunks=(3,) if L == 641 else ())
    tg26 = _targets(rng, 7, 160 if emu else 350, 26)
    ref, res, tm = _ways(ctx, [_read(rng, 400, tg26, 26, 0.1)], tg26, _gate26_mat(), 26, 10, 2, kname_of=400)
    assert tm["db_long_pairs"] == 5
    ref, res, tm = _ways(ctx, [_read(rng, 384, tg26, 26, 0.1)], tg26, _gate26_mat(), 26, 10, 2)
    assert tm["db_long_pairs"] == 0 and tm["fill_kernel"].startswith("k_filldb<24,")
    # both sides of the alphabet gate in one call
    ref, res, tm = _ways(ctx, [_read(rng, 400, tg26, 26, 0.1), _read(rng, 384, tg26, 26, 0.1), _read(rng, 30, tg26, 26, 0.1)], tg26, _gate26_mat(), 26, 10, 2, chunks=(2,))
    assert tm["db_long_pairs"] == 5


def test_emu_proteins_and_alphabet_gate(ectx):
    _proteins(ectx, True)


@pytest.mark.gpu
def test_gpu_proteins_and_alphabet_gate(gpu_ctx):
    _proteins(gpu_ctx, False)


# ---- 3 rules

def _mat(match, mismatch):
    m = np.full((5, 5), -mismatch, dtype=np.int8)
    np.fill_diagonal(m, match)
    m[4, :] = 0; m[:, 4] = 0
    return np.ascontiguousarray(m.reshape(-1))


def _rules_case(rng, L, maxcols):
    """a read of L residues (L & 15 in 1..8: the rows below ceil8 are padding under 16-bit rules) that holds an exact copy of the longest
    target (score 2 x its columns: beyond 8 bits) and a 40-residue piece that one target holds TWICE, 60 columns apart (a second best)"""
    tg = _targets(rng, 7, maxcols)
    piece = _rand(rng, 40)
    same = [i for i, t in enumerate(tg) if len(t) == maxcols // 2]
    k = same[0]
    tg[k] = np.concatenate([piece, _rand(rng, 60), piece, _rand(rng, maxcols)])[:150]
    tg[same[1]] = _rand(rng, 150)      # (still two targets of equal length)
    big = max(tg, key=len)
    rd = np.concatenate([_rand(rng, 9), big, _rand(rng, 13), piece, _rand(rng, L)])[:L]
    return np.ascontiguousarray(rd), tg, k


def _rules(ctx, emu):
    rng = np.random.default_rng(4301)
    mat = dna_matrix(2, 2)
    for L in (705, 769) if emu else (641, 648, 705, 769, 1601):
        assert 1 <= (L & 15) <= 8
        rd, tg, k = _rules_case(rng, L, 200 if emu else 400)
        for ss in (0, 1, 2):
            for maskLen in ((16,) if ss == 1 or emu and ss == 0 else (-1, 16)):
                ref, res, tm = _ways(ctx, [rd], tg, mat, 5, maskLen=maskLen, score_size=ss, chunks=(3,) if ss == 0 and maskLen == 16 else ())
                big = max(range(len(tg)), key=lambda t: len(tg[t]))
                if ss == 0:      # the exact copy overflows 8 bits: the reference returns NULL (ref_end2 -2 in the hits, checked by _ways)
                    assert ref[0][big][0] is None and int(res[0, big]["status"]) == 1
                else:
                    assert ref[0][big][0]["score1"] == 2 * len(tg[big]) and tm["n_word"] >= 1
                if maskLen == 16:      # the repeated piece: a second best outside the mask
                    assert ref[0][k][0]["score2"] > 0 and ref[0][k][0]["ref_end2"] > 0, ref[0][k][0]
    # the plain int16 form: scores that leave the frame's range (match 30 over 1 600 rows)
    rd, tg, k = _rules_case(rng, 1601, 200 if emu else 400)
    assert not _frame(1601, _mat(30, 20), 40, 3)
    _ways(ctx, [rd], tg, _mat(30, 20), 5, 40, 3, kname_of=1601, form="int16")


def test_emu_rules(ectx):
    _rules(ectx, True)


@pytest.mark.gpu
def test_gpu_rules(gpu_ctx):
    _rules(gpu_ctx, False)


def _forms_and_tickets(ctx, emu):
    """hooks: the plain form forced where the frame fits (SSW_GPU_DB_FORM=0), and both ticket modes of the work queue -- whole jobs, and
    strip tickets as a launch with more jobs than wavefront slots draws them (GPU: also unforced, 6 000 jobs against 39 targets)"""
    rng = np.random.default_rng(4351)
    mat = dna_matrix(2, 2)
    rd, tg, k = _rules_case(rng, 769, 200 if emu else 400)
    with _env(SSW_GPU_DB_FORM=0):
        _ways(ctx, [rd], tg, mat, 5, kname_of=769, form="int16", chunks=(3,))
    for mode in ("jobs", "strips"):
        with _env(SSW_GPU_QUEUE=mode):
            _ways(ctx, [rd, _read(rng, 1600, tg)], tg, mat, 5, chunks=(3,))
    if not emu:
        tg = _targets(rng, 40, 120)
        reads = [_read(rng, 769, tg) for _ in range(4)] * 75      # 300 queries x 20 jobs: more jobs than the device holds wavefronts
        Q = ctx.upload(reads); T = ctx.upload(tg); Q4 = ctx.upload(reads[:4])
        try:
            res, _ = ctx.align_batch(Q, T, mat, 5)
            tm = ctx.timing()
            assert tm["db_long_pairs"] == 300 * 39 and tm["fill_launches"] == 1
            one, _ = ctx.align_batch(Q4, T, mat, 5)
            bad = []
            _check_ref("strip tickets", one, np.zeros(0, dtype=np.uint32), reads[:4], tg,
                       [[_ref(rd, t, mat, 5, 3, 1, 0, 0, len(rd) // 2, 2) for t in tg] for rd in reads[:4]], bad)
            for r in range(75):
                _same_records("repeat %d" % r, res[4 * r:4 * r + 4], one, bad)
            assert not bad, "\n".join(bad)
        finally:
            Q.free(); T.free(); Q4.free()


def test_emu_forms_and_tickets(ectx):
    _forms_and_tickets(ectx, True)


@pytest.mark.gpu
def test_gpu_forms_and_tickets(gpu_hctx):
    _forms_and_tickets(gpu_hctx, False)


# ---- 4 mixed call

def _mixed(ctx, emu):
    """short, mid (385..640: k_filldb's classes 25..40), empty and long queries in one call: the rows equal the same queries as calls of
    their own, db_long_pairs counts the long rows only"""
    rng = np.random.default_rng(4401)
    mat = dna_matrix(2, 2)
    tg = _targets(rng, 9 if emu else 31, 200 if emu else 400)
    lens = (50, 700, 0, 500, 1000, 33) if emu else (50, 700, 0, 500, 1000, 33, 641, 384, 385, 768, 2500, 150)
    if not emu:      # queries of several strips: a bucket per padded length -- more buckets than any fixed table would hold
        lens = lens + tuple(800 + 16 * i for i in range(70))
    reads = [_read(rng, L, tg) if L else np.zeros(0, dtype=np.int8) for L in lens]
    nz = sum(1 for t in tg if len(t))
    ref, res, tm = _ways(ctx, reads, tg, mat, 5)
    assert tm["db_long_pairs"] == sum(1 for L in lens if L > 640) * nz
    bad = []
    for side in (True, False):
        qs = [q for q, L in enumerate(lens) if (L > 640) == side]
        ref2, res2, tm2 = _ways(ctx, [reads[q] for q in qs], tg, mat, 5)
        assert (tm2["db_long_pairs"] > 0) == side and tm2["fill_kernel"].startswith("k_filldb<") != side
        _same_records("one side against the mixed call", res2, res[qs], bad)
    assert not bad, "\n".join(bad)


def test_emu_mixed_call(ectx):
    _mixed(ectx, True)


@pytest.mark.gpu
def test_gpu_mixed_call(gpu_ctx):
    _mixed(gpu_ctx, False)


# ---- 5 streamed search

def _streamed(ctx, emu):
    """search_db in chunks that split the targets unevenly and in chunks of one target (short and long rows of a chunk in one matrix),
    the stop code of the chunk function, search_topk with k = 1, 3 and all targets at flag 0 and 2"""
    rng = np.random.default_rng(4501)
    mat = dna_matrix(2, 2)
    nt = 7 if emu else 27
    tg = _targets(rng, nt, 150 if emu else 400)
    reads = [_read(rng, L, tg) if L else np.zeros(0, dtype=np.int8) for L in ((40, 700, 0, 1000) if emu else (40, 700, 0, 1000, 500, 769, 100))]
    assert nt % 4 and nt % 5
    ref, res, tm = _ways(ctx, reads, tg, mat, 5, chunks=(4, 1) if emu else (4, 5, 1, 0), ks=(1, 3, nt))
    nz = sum(1 for t in tg if len(t))
    Q = ctx.upload(reads); T = ctx.upload(tg)
    try:
        calls = []
        rc = ctx.search_db(Q, T, mat, 5, 3, 1, -1, 2, 2, lambda t0, h: (calls.append(t0), 7)[1] if t0 >= 2 else calls.append(t0))
        assert rc == 7 and calls == [0, 2]
        # flag 2: the lists are the flag-0 lists, the selected pairs complete (begins, CIGARs) -- against the reference
        for k in (1, 3):
            ti, tres, tcig = ctx.search_topk(Q, T, k, mat, 5, flag=2, min_score=1)
            ttm = ctx.timing()
            assert ttm["db_long_pairs"] == sum(1 for r in reads if len(r) > 640) * nz and ttm["reduce_ms"] > 0
            for q, rd in enumerate(reads):
                elig = [t for t in range(nt) if int(res[q, t]["status"]) == 0 and int(res[q, t]["score1"]) >= 1]
                elig.sort(key=lambda t: (-int(res[q, t]["score1"]), t))
                assert [int(x) for x in ti[q]] == elig[:k] + [-1] * (k - len(elig[:k]))
                for r, t in enumerate(elig[:k]):
                    exp, ecig = _ref(rd, tg[t], mat, 5, 3, 1, 2, 0, len(rd) // 2, 2)
                    g = tres[q, r]
                    assert {f: int(g[f]) for f in RES_FIELDS} == exp and _cig(g, tcig) == ecig, (k, q, r, exp, g)
    finally:
        Q.free(); T.free()
    return reads, tg, res


def test_emu_streamed_search(ectx):
    _streamed(ectx, True)


@pytest.mark.gpu
def test_gpu_streamed_search(gpu_ctx):
    _streamed(gpu_ctx, False)


def _pool_equals_context(lib, devices, emu):
    rng = np.random.default_rng(4551)
    mat = dna_matrix(2, 2)
    tg = _targets(rng, 7 if emu else 21, 150 if emu else 400)
    reads = [_read(rng, L, tg) for L in (40, 700, 1000, 90)]
    ctx = ssw_amd.Context(0, lib)
    pool = ssw_amd.Pool(devices, lib)
    try:
        Q = ctx.upload(reads); T = ctx.upload(tg)
        pool.set_targets(tg)
        for flag in (0, 2):
            t1, r1, c1 = ctx.search_topk(Q, T, 3, mat, 5, flag=flag)
            assert ctx.timing()["db_long_pairs"] > 0
            t2, r2, c2 = pool.search_topk(reads, 3, mat, 5, flag=flag, block=3)
            assert (t1 == t2).all() and (c1 == c2).all()
            bad = []
            _same_records("pool against the single context, flag %d" % flag, r2, r1, bad)
            assert not bad, "\n".join(bad)
        Q.free(); T.free()
    finally:
        pool.close(); ctx.close()


def test_emu_pool_equals_context(emu_lib_path, monkeypatch):
    monkeypatch.setenv("SSW_EMU_DEVICES", "2")
    _pool_equals_context(ssw_amd.load(emu_lib_path), [0, 1], True)


@pytest.mark.gpu
def test_gpu_pool_equals_context(product_lib_path):
    _pool_equals_context(ssw_amd.load(product_lib_path), [0, 0], False)


# ---- 6 flags

def _flags(ctx, emu):
    """flag 1 (begins), 2 behind a filter that separates the pairs, 8, 15 and mark_mismatch: (query, target) pairs of the class go through
    ONE batched reverse pass and traceback with the short rows' survivors"""
    rng = np.random.default_rng(4601)
    mat = dna_matrix(2, 2)
    tg = _targets(rng, 7 if emu else 23, 150 if emu else 400)
    reads = [_read(rng, L, tg) for L in ((700, 60, 1000) if emu else (700, 60, 1000, 641, 769, 500, 1600))]
    flags = ((2, 150, False), (15, 0, False)) if emu else ((1, 0, False), (2, 150, False), (8, 0, False), (15, 0, False), (2, 0, True))
    _ways(ctx, reads, tg, mat, 5, flags=flags)


def test_emu_flags(ectx):
    _flags(ectx, True)


@pytest.mark.gpu
def test_gpu_flags(gpu_ctx):
    _flags(gpu_ctx, False)


# ---- 7 budget

def _budget(lib, emu):
    """a budget that holds five jobs of the class where a chunk has six: two launches per chunk, the same records; a budget below one
    job's scratch: the query is back on the per-target loop (db_long_pairs 0), the same records"""
    rng = np.random.default_rng(4701)
    mat = dna_matrix(2, 2)
    ctx = ssw_amd.Context(0, lib)
    try:
        bad = []
        # 1 MiB (the smallest budget a context takes): a job against 4 000 columns needs ~94 KiB, five fit half the budget; two queries of
        # one bucket x three jobs are two launches in the one chunk
        tg = [_rand(rng, L) for L in (0, 1, 4000, 40, 40, 60, 0)]
        reads = [_read(rng, 1000, tg, rate=0.3), _read(rng, 1000, tg, rate=0.3), _read(rng, 90, tg)]
        assert (1 << 19) // _job_bytes(4000, _shape(1000, 5)[1]) == 5 < 2 * 3
        ref, res, tm = _ways(ctx, reads, tg, mat, 5)
        ref1, res1, tm1 = _ways(ctx, reads, tg, mat, 5, budget=1 << 20, chunks=() if emu else (4,))
        assert tm1["db_long_pairs"] == 2 * 5
        _same_records("five jobs per launch against the default budget", res1, res, bad)
        # a job against 22 000 columns does not fit half of 1 MiB: the per-target loop, as before
        tg = [_rand(rng, L) for L in (0, 1, 22000, 40, 40, 60, 0)]
        reads = [_read(rng, 641, tg, rate=0.3)]
        assert _job_bytes(22000, 1) > (1 << 19)
        ref, res, tm = _ways(ctx, reads, tg, mat, 5)
        assert tm["db_long_pairs"] == 5
        ref2, res2, tm2 = _ways(ctx, reads, tg, mat, 5, budget=1 << 20)
        assert tm2["db_long_pairs"] == 0 and tm2["fill_launches"] >= 5 and ",pairs," not in tm2["fill_kernel"]
        _same_records("below one job's scratch against the default budget", res2, res, bad)
        assert not bad, "\n".join(bad)
    finally:
        ctx.close()


def test_emu_budget(ectx):
    _budget(ectx.lib, True)


@pytest.mark.gpu
def test_gpu_budget(gpu_ctx):
    _budget(gpu_ctx.lib, False)
