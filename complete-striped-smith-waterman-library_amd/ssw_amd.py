"""ctypes binding of libssw.so (the MI355X-native Smith-Waterman library).

Two layers, both thin:

* ``CSsw`` mirrors the reference's own ctypes wrapper (reference src/ssw_lib.py:94-197: class
  ``CSsw`` with ``ssw_init`` / ``ssw_align`` / ``init_destroy`` / ``align_destroy`` and the
  ``CAlignRes`` field layout of src/ssw_lib.py:61-69) so that code written against it runs unchanged.
* ``Context`` / ``Seqs`` / ``align_batch`` bind the batch ABI of include/ssw_gpu.h.

This module never computes alignments itself: if the shared library (and through it the HIP device)
is missing, loading or calling fails loudly.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libssw.so")

_i8p = C.POINTER(C.c_int8)
_u32p = C.POINTER(C.c_uint32)
_i64p = C.POINTER(C.c_int64)


class CAlignRes(C.Structure):
    """s_align (include/ssw.h; reference src/ssw.h:55-66)."""
    _fields_ = [("nScore", C.c_uint16), ("nScore2", C.c_uint16), ("nRefBeg", C.c_int32), ("nRefEnd", C.c_int32),
                ("nQryBeg", C.c_int32), ("nQryEnd", C.c_int32), ("nRefEnd2", C.c_int32), ("sCigar", _u32p),
                ("nCigarLen", C.c_int32), ("nFlag", C.c_uint16)]


class Params(C.Structure):
    """ssw_gpu_params (include/ssw_gpu.h)."""
    _fields_ = [("mat", _i8p), ("n", C.c_int32), ("gapO", C.c_uint8), ("gapE", C.c_uint8), ("flag", C.c_uint8),
                ("filters", C.c_uint16), ("filterd", C.c_int32), ("maskLen", C.c_int32), ("score_size", C.c_int8),
                ("mark_mismatch", C.c_int8)]


class PairModel(C.Structure):
    """ssw_gpu_pair_model (include/ssw_gpu.h)."""
    _fields_ = [("min_insert", C.c_int32), ("max_insert", C.c_int32), ("unpaired_penalty", C.c_int32), ("orientation", C.c_int32),
                ("insert_penalty", C.POINTER(C.c_uint16))]


class Result(C.Structure):
    """ssw_gpu_result (include/ssw_gpu.h)."""
    _fields_ = [("score1", C.c_uint16), ("score2", C.c_uint16), ("ref_begin1", C.c_int32), ("ref_end1", C.c_int32),
                ("read_begin1", C.c_int32), ("read_end1", C.c_int32), ("ref_end2", C.c_int32), ("cigarLen", C.c_int32),
                ("edit_distance", C.c_int32), ("cigar_off", C.c_int64), ("flag", C.c_uint16), ("status", C.c_uint16)]


class Timing(C.Structure):
    """ssw_gpu_timing (include/ssw_gpu.h)."""
    _fields_ = [("total_ms", C.c_double), ("fill_ms", C.c_double), ("fill_launches", C.c_int64),
                ("fill_cells", C.c_int64), ("cells", C.c_int64), ("reduce_ms", C.c_double), ("locate_ms", C.c_double),
                ("trace_ms", C.c_double), ("n_word", C.c_int64), ("n_byte", C.c_int64), ("fill_kernel", C.c_char * 48),
                ("fill_ops_per_row", C.c_double), ("fill_rows_per_lane", C.c_int32), ("fill_strips", C.c_int32),
                ("db_repeats", C.c_int64), ("fill_pipelined", C.c_int64), ("win_copied", C.c_int64), ("best_flagged", C.c_int64),
                ("db_long_pairs", C.c_int64), ("rescue_windows", C.c_int64)]


class INSERT_COUNTS(C.Structure):
    """ssw_gpu_insert_counts (include/ssw_gpu.h)."""
    _fields_ = [("n_both", C.c_int64), ("n_unique", C.c_int64), ("n_same", C.c_int64), ("n_in", C.c_int64 * 3), ("n_out", C.c_int64 * 3)]


class INSERT_STATS(C.Structure):
    """ssw_gpu_insert_stats (include/ssw_gpu.h)."""
    _fields_ = [("n_total", C.c_int64), ("n_used", C.c_int64), ("p25", C.c_int32), ("p50", C.c_int32), ("p75", C.c_int32),
                ("out_lo", C.c_int32), ("out_hi", C.c_int32), ("sum", C.c_uint64), ("sum2", C.c_uint64), ("mean", C.c_double),
                ("sd", C.c_double), ("min_insert", C.c_int32), ("max_insert", C.c_int32)]


HIT_DTYPE = np.dtype([("score1", "<u2"), ("score2", "<u2"), ("ref_end1", "<i4"), ("read_end1", "<i4"), ("ref_end2", "<i4")], align=True)
HITS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p)     # ssw_gpu_hits_fn (include/ssw_gpu.h)


class PoolStat(C.Structure):
    """ssw_gpu_pool_stat (include/ssw_gpu.h)."""
    _fields_ = [("device", C.c_int32), ("blocks", C.c_int64), ("queries", C.c_int64), ("cells", C.c_int64), ("busy_ms", C.c_double)]


RESULT_DTYPE = np.dtype([("score1", "<u2"), ("score2", "<u2"), ("ref_begin1", "<i4"), ("ref_end1", "<i4"),
                         ("read_begin1", "<i4"), ("read_end1", "<i4"), ("ref_end2", "<i4"), ("cigarLen", "<i4"),
                         ("edit_distance", "<i4"), ("cigar_off", "<i8"), ("flag", "<u2"), ("status", "<u2")], align=True)
assert RESULT_DTYPE.itemsize == C.sizeof(Result)
# ssw_gpu_best (include/ssw_gpu.h): the selection record of ssw_gpu_align_windows_best
BEST_DTYPE = np.dtype([("best", "<i4"), ("second", "<i4"), ("n_eligible", "<i4"), ("second_score1", "<u2"), ("pad", "<u2")], align=True)
assert BEST_DTYPE.itemsize == 16
# ssw_gpu_mates (include/ssw_gpu.h): the selection record of ssw_gpu_align_windows_mates, one per fragment
MATES_DTYPE = np.dtype([("pos1", "<i4"), ("pos2", "<i4"), ("n_eligible1", "<i4"), ("n_eligible2", "<i4"), ("score", "<i4"),
                        ("second_score", "<i4"), ("n_proper", "<i4"), ("proper", "<u2"), ("pad", "<u2")], align=True)
assert MATES_DTYPE.itemsize == 32
# ssw_gpu_rescued (include/ssw_gpu.h): where the chosen candidate of a mate came from (ssw_gpu_align_windows_mates_rescue)
RESCUED_DTYPE = np.dtype([("tbeg", "<i8"), ("tlen", "<i4"), ("tidx", "<i4"), ("qidx", "<i4"), ("anchor", "<i4")], align=True)
assert RESCUED_DTYPE.itemsize == 24
# SSW_GPU_MATES_FR / _RF / _FF (include/ssw_gpu.h): the library orientation of the proper-pair rule
MATES_ORIENTATION = {"fr": 0, "rf": 1, "ff": 2}


def _orientation(o):
    """"fr" | "rf" | "ff" (any case) -> 0 .. 2; an integer goes to the library as it is (which refuses what it does not know)"""
    if isinstance(o, str):
        if o.lower() not in MATES_ORIENTATION:
            raise ValueError("orientation must be 'fr', 'rf', 'ff' or 0 .. 2")
        return MATES_ORIENTATION[o.lower()]
    return int(o)


def _insert_table(insert_penalty, min_insert, max_insert):
    """the insert_penalty keyword of the mates calls -> a C-contiguous uint16 array of max_insert - min_insert + 1 entries"""
    t = np.asarray(insert_penalty)
    if t.ndim != 1 or t.dtype.kind not in "iu":
        raise ValueError("insert_penalty must be a 1-D integer array")
    if t.shape[0] != int(max_insert) - int(min_insert) + 1:
        raise ValueError("insert_penalty must have max_insert - min_insert + 1 = %d entries, not %d"
                         % (int(max_insert) - int(min_insert) + 1, t.shape[0]))
    if t.shape[0] > 0 and (int(t.min()) < 0 or int(t.max()) > 65535):
        raise ValueError("insert_penalty entries must be 0 .. 65535")
    return np.ascontiguousarray(t, dtype=np.uint16)


def _pair_model(min_insert, max_insert, unpaired_penalty, orient, table):
    return PairModel(int(min_insert), int(max_insert), int(unpaired_penalty), orient, table.ctypes.data_as(C.POINTER(C.c_uint16)))


def insert_penalty_normal(mean, sd, min_insert, max_insert, match, cap):
    """a penalty table for the insert_penalty keyword, for a library whose insert sizes are normal(mean, sd): entry i, for the span
    D = min_insert + i, is min(cap, floor(0.721 * match * (-ln erfc(|D - mean| / (sd * sqrt 2))) + 0.5)), and cap where erfc
    underflows to 0.  It is BWA-MEM's log-scaled insert term (0.721 = 1 / ln 4: log base 4 of the two-sided tail probability, in units
    of the match score) with the sign turned into a penalty, 0 at the mean -> uint16 [max_insert - min_insert + 1].  Host arithmetic only."""
    min_insert, max_insert, cap = int(min_insert), int(max_insert), int(cap)
    if not sd > 0:
        raise ValueError("sd must be > 0")
    if min_insert > max_insert:
        raise ValueError("min_insert <= max_insert required")
    if cap < 0 or cap > 65535:
        raise ValueError("cap must be 0 .. 65535")
    out = np.zeros(max_insert - min_insert + 1, dtype=np.uint16)
    for i in range(out.shape[0]):
        e = math.erfc(abs(min_insert + i - mean) / (sd * math.sqrt(2.0)))
        out[i] = cap if e <= 0.0 else min(cap, int(math.floor(0.721 * match * (-math.log(e)) + 0.5)))
    return out


def insert_fit(hist_row, lib=None):
    """one row of Context.insert_hist's histogram -> the dict of ssw_gpu_insert_stats' fields (quartiles, outlier bounds, mean, sd and
    the min_insert / max_insert a mates call takes), or None when the row holds too few observations (ssw_gpu_insert_fit returns 1).
    Host arithmetic inside the library; no device."""
    h = np.ascontiguousarray(hist_row, dtype=np.uint32)
    if h.ndim != 1:
        raise ValueError("hist_row must be a 1-D array")
    st = INSERT_STATS()
    rc = (lib or load()).ssw_gpu_insert_fit(h.ctypes.data_as(C.c_void_p), int(h.shape[0]), C.byref(st))
    if rc == 1:
        return None
    if rc != 0:
        raise ValueError("ssw_gpu_insert_fit: an empty row, or 2^31 observations or more")
    return {name: getattr(st, name) for name, _ in INSERT_STATS._fields_}


def insert_model_normal(stats, match, cap):
    """a fit (insert_fit's dict) -> dict(min_insert, max_insert, insert_penalty) to splat into Context.align_windows_mates: the fitted
    range and insert_penalty_normal's table for normal(mean, sd) over it.  A fit with sd == 0 is refused by insert_penalty_normal."""
    mn, mx = int(stats["min_insert"]), int(stats["max_insert"])
    return dict(min_insert=mn, max_insert=mx, insert_penalty=insert_penalty_normal(stats["mean"], stats["sd"], mn, mx, match, cap))


def _mates_rebase(sel, res, co, tb):
    """adds the chosen candidate's tbeg to ref_begin1, ref_end1 and ref_end2 where they are >= 0"""
    nf = sel.shape[0]
    pos = np.stack([sel["pos1"], sel["pos2"]], axis=1)
    hit = pos >= 0
    wb = np.zeros((nf, 2), dtype=np.int64)
    wb[hit] = tb[(co[:-1].reshape(nf, 2) + pos)[hit]]
    for f in ("ref_begin1", "ref_end1", "ref_end2"):
        v = res[f]
        res[f] = np.where(v >= 0, v + wb, v).astype(np.int32)


def load(path=None):
    path = path or os.environ.get("SSW_LIB", DEFAULT_LIB)
    if not os.path.exists(path):
        raise OSError("libssw.so not built: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
    L = C.CDLL(path)
    L.ssw_init.argtypes = [_i8p, C.c_int32, _i8p, C.c_int32, C.c_int8]
    L.ssw_init.restype = C.c_void_p
    L.init_destroy.argtypes = [C.c_void_p]
    L.init_destroy.restype = None
    L.ssw_align.argtypes = [C.c_void_p, _i8p, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32,
                            C.c_int32]
    L.ssw_align.restype = C.POINTER(CAlignRes)
    L.align_destroy.argtypes = [C.POINTER(CAlignRes)]
    L.align_destroy.restype = None
    L.mark_mismatch.argtypes = [C.c_int32, C.c_int32, C.c_int32, _i8p, _i8p, C.c_int32, C.POINTER(_u32p),
                                C.POINTER(C.c_int32)]
    L.mark_mismatch.restype = C.c_int32
    L.ssw_gpu_device_count.restype = C.c_int
    L.ssw_gpu_open.argtypes = [C.c_int]
    L.ssw_gpu_open.restype = C.c_void_p
    L.ssw_gpu_close.argtypes = [C.c_void_p]
    L.ssw_gpu_close.restype = None
    L.ssw_gpu_last_error.argtypes = [C.c_void_p]
    L.ssw_gpu_last_error.restype = C.c_char_p
    L.ssw_gpu_seqs_upload.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32]
    L.ssw_gpu_seqs_upload.restype = C.c_void_p
    L.ssw_gpu_seqs_upload_ascii.argtypes = [C.c_void_p, C.c_char_p, _i64p, C.c_int32, _i8p]
    L.ssw_gpu_seqs_upload_ascii.restype = C.c_void_p
    L.ssw_gpu_seqs_revcomp.argtypes = [C.c_void_p, C.c_void_p]
    L.ssw_gpu_seqs_revcomp.restype = C.c_void_p
    L.ssw_gpu_seqs_with_revcomp.argtypes = [C.c_void_p, C.c_void_p]
    L.ssw_gpu_seqs_with_revcomp.restype = C.c_void_p
    L.ssw_gpu_seqs_download.argtypes = [C.c_void_p, C.c_void_p, _i8p]
    L.ssw_gpu_seqs_download.restype = C.c_int
    L.ssw_gpu_seqs_free.argtypes = [C.c_void_p]
    L.ssw_gpu_seqs_free.restype = None
    L.ssw_gpu_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Params),
                                      C.c_void_p, C.POINTER(_u32p), _i64p]
    L.ssw_gpu_align_batch.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_pairs"):
        L.ssw_gpu_align_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params),
                                          C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_pairs.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows"):
        L.ssw_gpu_align_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.POINTER(Params), C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_best"):
        L.ssw_gpu_align_windows_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_best.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_topk"):
        L.ssw_gpu_align_windows_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_topk.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_mates"):
        L.ssw_gpu_align_windows_mates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_int32, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_mates.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_mates_lib"):
        L.ssw_gpu_align_windows_mates_lib.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int32, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                      C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_mates_lib.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_mates_rescue"):
        L.ssw_gpu_align_windows_mates_rescue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_mates_rescue.restype = C.c_int
    if hasattr(L, "ssw_gpu_pool_align_windows_mates"):
        L.ssw_gpu_pool_align_windows_mates.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
                                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_pool_align_windows_mates.restype = C.c_int
    if hasattr(L, "ssw_gpu_align_windows_mates_model"):
        L.ssw_gpu_align_windows_mates_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_int32, C.POINTER(Params), C.c_int32, C.POINTER(PairModel),
                                                        C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_mates_model.restype = C.c_int
        L.ssw_gpu_align_windows_mates_rescue_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Params), C.c_int32,
                                                               C.POINTER(PairModel), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_align_windows_mates_rescue_model.restype = C.c_int
        L.ssw_gpu_pool_align_windows_mates_model.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_int32,
                                                             C.POINTER(PairModel), C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_pool_align_windows_mates_model.restype = C.c_int
    if hasattr(L, "ssw_gpu_insert_hist"):
        L.ssw_gpu_insert_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.POINTER(INSERT_COUNTS)]
        L.ssw_gpu_insert_hist.restype = C.c_int
        L.ssw_gpu_insert_fit.argtypes = [C.c_void_p, C.c_int32, C.POINTER(INSERT_STATS)]
        L.ssw_gpu_insert_fit.restype = C.c_int
    if hasattr(L, "ssw_gpu_search_topk"):
        L.ssw_gpu_search_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_search_topk.restype = C.c_int
    if hasattr(L, "ssw_gpu_pool_search_topk"):
        L.ssw_gpu_pool_search_topk.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_pool_search_topk.restype = C.c_int
    if hasattr(L, "ssw_gpu_pool_align_windows"):
        L.ssw_gpu_pool_align_windows.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int64, C.c_int64, C.POINTER(Params), C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_pool_align_windows.restype = C.c_int
        L.ssw_gpu_pool_align_windows_topk.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_u32p), _i64p]
        L.ssw_gpu_pool_align_windows_topk.restype = C.c_int
    L.ssw_gpu_last_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.ssw_gpu_last_timing.restype = C.c_int
    L.ssw_gpu_last_timing_sized.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ssw_gpu_last_timing_sized.restype = C.c_int
    L.ssw_gpu_strerror.argtypes = [C.c_int]
    L.ssw_gpu_strerror.restype = C.c_char_p
    L.ssw_gpu_set_budget.argtypes = [C.c_void_p, C.c_size_t]
    L.ssw_gpu_set_budget.restype = C.c_int
    L.ssw_gpu_get_budget.argtypes = [C.c_void_p]
    L.ssw_gpu_get_budget.restype = C.c_size_t
    L.ssw_gpu_set_budget_exclusive.argtypes = [C.c_void_p]
    L.ssw_gpu_set_budget_exclusive.restype = C.c_int
    L.ssw_gpu_pool_budget.argtypes = [C.c_void_p, C.c_int]
    L.ssw_gpu_pool_budget.restype = C.c_size_t
    L.ssw_gpu_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.ssw_gpu_host_alloc.restype = C.c_void_p
    L.ssw_gpu_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.ssw_gpu_host_free.restype = None
    if hasattr(L, "ssw_gpu_valu_probe"):      # diagnostics (include/ssw_gpu_diag.h): libssw_hooks.so and the test emulator only
        L.ssw_gpu_selftest_lanes.argtypes = [C.c_void_p, _u32p]
        L.ssw_gpu_selftest_lanes.restype = C.c_int
        L.ssw_gpu_valu_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.ssw_gpu_valu_probe.restype = C.c_double
    L.ssw_gpu_release_parked.restype = C.c_int
    L.ssw_gpu_search_db.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_int32, HITS_FN, C.c_void_p]
    L.ssw_gpu_search_db.restype = C.c_int
    L.ssw_gpu_pool_open.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.ssw_gpu_pool_open.restype = C.c_void_p
    L.ssw_gpu_pool_close.argtypes = [C.c_void_p]
    L.ssw_gpu_pool_close.restype = None
    L.ssw_gpu_pool_size.argtypes = [C.c_void_p]
    L.ssw_gpu_pool_last_error.argtypes = [C.c_void_p]
    L.ssw_gpu_pool_last_error.restype = C.c_char_p
    L.ssw_gpu_pool_set_targets.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32]
    L.ssw_gpu_pool_align.argtypes = [C.c_void_p, _i8p, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params),
                                     C.c_void_p, C.POINTER(_u32p), _i64p]
    L.ssw_gpu_pool_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(PoolStat)]
    return L


class CSsw(object):
    """Same surface as the reference's src/ssw_lib.py CSsw (sLibPath = directory holding libssw.so)."""

    def __init__(self, sLibPath=None):
        path = os.path.join(sLibPath, "libssw.so") if sLibPath else None
        self.ssw = load(path)
        self.ssw_init = self.ssw.ssw_init
        self.init_destroy = self.ssw.init_destroy
        self.ssw_align = self.ssw.ssw_align
        self.align_destroy = self.ssw.align_destroy
        self._ctx = None

    def align_many(self, lQueries, lTargets, mat, nOpen, nExt, nFlag, nMaskLen, nFilterScore=0, nFilterDist=0, device=0):
        """The loop of the reference's pyssw.py (src/pyssw.py:236-275: for every query ssw_init, for every target align_one) as ONE
        batch call.  lQueries / lTargets: number arrays as pyssw.to_int builds them (ctypes c_int8 arrays, numpy int8 arrays or lists);
        mat: the flat score matrix (lScore); nMaskLen < 0: len(query) / 2 per query (pyssw.py:243).  Returns [query][target] of the
        tuples align_one returns: (nScore, nScore2, nRefBeg, nRefEnd, nQryBeg, nQryEnd, nRefEnd2, nCigarLen, lCigar)."""
        if self._ctx is None:
            self._ctx = Context(device, self.ssw)
        ctx = self._ctx
        qs = [np.frombuffer(bytes(bytearray(x)), dtype=np.int8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, dtype=np.int8) for x in
              ([(int(v) & 0xff) for v in q] if not isinstance(q, np.ndarray) else q for q in lQueries)]
        ts = [np.frombuffer(bytes(bytearray(x)), dtype=np.int8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, dtype=np.int8) for x in
              ([(int(v) & 0xff) for v in t] if not isinstance(t, np.ndarray) else t for t in lTargets)]
        m = np.ascontiguousarray(np.array(list(mat), dtype=np.int8))
        n = int(round(len(m) ** 0.5))
        Q = ctx.upload(qs); T = ctx.upload(ts)
        try:
            res, cig = ctx.align_batch(Q, T, m, n, nOpen, nExt, nFlag, nFilterScore, nFilterDist, nMaskLen, 2)
        finally:
            Q.free(); T.free()
        out = []
        for qi in range(len(qs)):
            row = []
            for ti in range(len(ts)):
                g = res[qi, ti]
                k, o = int(g["cigarLen"]), int(g["cigar_off"])
                row.append((int(g["score1"]), int(g["score2"]), int(g["ref_begin1"]), int(g["ref_end1"]), int(g["read_begin1"]), int(g["read_end1"]),
                            int(g["ref_end2"]), k, [int(x) for x in cig[o:o + k]] if k > 0 else []))
            out.append(row)
        return out

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class Seqs(object):
    def __init__(self, ctx, seqs):
        self.ctx = ctx
        self.count = len(seqs)
        off = np.zeros(self.count + 1, dtype=np.int64)
        for i, s in enumerate(seqs):
            off[i + 1] = off[i] + len(s)
        codes = (np.concatenate([np.asarray(s, dtype=np.int8) for s in seqs]) if self.count else
                 np.zeros(0, dtype=np.int8))
        codes = np.ascontiguousarray(codes, dtype=np.int8)
        self.lengths = np.diff(off)
        self.h = ctx.lib.ssw_gpu_seqs_upload(ctx.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), self.count)
        if not self.h:
            raise RuntimeError("ssw_gpu_seqs_upload: " + ctx.error())

    def with_revcomp(self):
        """a new set: these sequences followed by their reverse complements (ssw_gpu_seqs_with_revcomp; DNA codes 0..3) -- sequence
        count + i is the reverse complement of sequence i, which is how a candidate list names the reverse strand of a read"""
        lib = self.ctx.lib
        both = object.__new__(Seqs)
        both.ctx = self.ctx
        both.count = 2 * self.count
        both.lengths = np.concatenate([self.lengths, self.lengths])
        both.h = lib.ssw_gpu_seqs_with_revcomp(self.ctx.h, self.h)
        if not both.h:
            raise RuntimeError("ssw_gpu_seqs_with_revcomp: " + self.ctx.error())
        return both

    def free(self):
        if self.h:
            self.ctx.lib.ssw_gpu_seqs_free(self.h)
            self.h = None


class Context(object):
    """One GPU (include/ssw_gpu.h ssw_gpu_ctx)."""

    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None and not isinstance(lib, str) else load(lib)
        self._pinned = []
        self.device = device
        self.h = self.lib.ssw_gpu_open(device)
        if not self.h:
            raise RuntimeError("ssw_gpu_open: " + self.lib.ssw_gpu_last_error(None).decode())

    def error(self):
        return self.lib.ssw_gpu_last_error(self.h).decode()

    def set_exclusive(self):
        """this context has its device to itself: scratch budget sized for the whole HBM (ssw_gpu_set_budget_exclusive) -> bytes"""
        self.lib.ssw_gpu_set_budget_exclusive(self.h)
        return int(self.lib.ssw_gpu_get_budget(self.h))

    def upload(self, seqs):
        return Seqs(self, seqs)

    def align_batch(self, queries, targets, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1,
                    score_size=2, target_first=0, target_count=None, want_cigar=True, mark_mismatch=False, out=None):
        """-> (numpy record array [nq, nt] of RESULT_DTYPE, numpy uint32 CIGAR pool).  `out`: a result array to fill
        (e.g. page-locked, from result_array(): large database searches download at PCIe rate only into pinned pages)."""
        if target_count is None:
            target_count = targets.count - target_first
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            res = np.zeros((queries.count, target_count), dtype=RESULT_DTYPE)
        else:
            res = out
            if res.dtype != RESULT_DTYPE or res.shape != (queries.count, target_count) or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous [nq, nt] array of RESULT_DTYPE")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_align_batch(self.h, queries.h, targets.h, target_first, target_count, C.byref(p),
                                          res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None,
                                          C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_batch: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        if want_cigar and words.value > 0:
            cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy()
        else:
            cig = np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        return res, cig

    def align_pairs(self, queries, targets, qidx, tidx, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1,
                    score_size=2, want_cigar=True, mark_mismatch=False, out=None):
        """explicit pair list (ssw_gpu_align_pairs): record i is the alignment of query qidx[i] against target tidx[i]
        -> (numpy record array [npairs] of RESULT_DTYPE, numpy uint32 CIGAR pool in pair order)"""
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        if qi.ndim != 1 or qi.shape != ti.shape:
            raise ValueError("qidx and tidx must be 1-D arrays of the same length")
        npairs = int(qi.shape[0])
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            res = np.zeros(npairs, dtype=RESULT_DTYPE)
        else:
            res = out
            if res.dtype != RESULT_DTYPE or res.shape != (npairs,) or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous [npairs] array of RESULT_DTYPE")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_align_pairs(self.h, queries.h, targets.h, qi.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                                          npairs, C.byref(p), res.ctypes.data_as(C.c_void_p),
                                          C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_pairs: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        if want_cigar and words.value > 0:
            cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy()
        else:
            cig = np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        return res, cig

    def align_windows(self, queries, targets, qidx, tidx, tbeg, tlen, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1,
                      score_size=2, want_cigar=True, mark_mismatch=False, out=None, rebase=False):
        """windows of resident targets (ssw_gpu_align_windows): record i is the alignment of query qidx[i] against residues
        [tbeg[i], tbeg[i] + tlen[i]) of target tidx[i], positions relative to the window
        -> (numpy record array [npairs] of RESULT_DTYPE, numpy uint32 CIGAR pool in pair order).
        rebase=True adds tbeg[i] to ref_begin1, ref_end1 and ref_end2 where they are >= 0 (target coordinates, what a mapper writes into
        SAM; -1 sentinels stay).  The fields are int32: a target is below 2^31 residues (ref_end1 is an int32 for align_batch too), and a
        position inside a window of it is below the target's length, so the sums fit."""
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        npairs = int(qi.shape[0])
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            res = np.zeros(npairs, dtype=RESULT_DTYPE)
        else:
            res = out
            if res.dtype != RESULT_DTYPE or res.shape != (npairs,) or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous [npairs] array of RESULT_DTYPE")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_align_windows(self.h, queries.h, targets.h, qi.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                                            tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), npairs, C.byref(p),
                                            res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_windows: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        if want_cigar and words.value > 0:
            cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy()
        else:
            cig = np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase:
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                v = res[f]
                res[f] = np.where(v >= 0, v + tb, v).astype(np.int32)
        return res, cig

    def align_windows_best(self, queries, targets, cand_off, qidx, tidx, tbeg, tlen, mat, n, min_score=0, rebase=False, gapO=3, gapE=1, flag=0,
                           filters=0, filterd=0, maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False, out=None):
        """best candidate window per read (ssw_gpu_align_windows_best): group g is candidates [cand_off[g], cand_off[g + 1]) of the four
        per-candidate arrays, a candidate being what a pair of align_windows is
        -> (sel [ngroups] of BEST_DTYPE, records [ngroups] of RESULT_DTYPE -- the winner's, or the empty record where sel["best"] is -1 --,
        uint32 CIGAR pool in group order).  rebase=True adds the winner's tbeg to ref_begin1, ref_end1 and ref_end2 where they are >= 0.
        `out`: (sel, records) to fill."""
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1:
            raise ValueError("cand_off must be a 1-D array of ngroups + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        ng = int(co.shape[0]) - 1
        if ng > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[ngroups] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            sel = np.zeros(ng, dtype=BEST_DTYPE)
            res = np.zeros(ng, dtype=RESULT_DTYPE)
        else:
            sel, res = out
            if sel.dtype != BEST_DTYPE or res.dtype != RESULT_DTYPE or sel.shape != (ng,) or res.shape != (ng,) or not sel.flags["C_CONTIGUOUS"] or \
                    not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous [ngroups] arrays of BEST_DTYPE and RESULT_DTYPE")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_align_windows_best(self.h, queries.h, targets.h, co.ctypes.data_as(C.c_void_p), ng, qi.ctypes.data_as(C.c_void_p),
                                                 ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                 C.byref(p), int(min_score), sel.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                                 C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_windows_best: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and ng > 0:
            won = sel["best"] >= 0
            wb = np.zeros(ng, dtype=np.int64)
            wb[won] = tb[co[:-1][won] + sel["best"][won]]
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                v = res[f]
                res[f] = np.where(v >= 0, v + wb, v).astype(np.int32)
        return sel, res, cig

    def align_windows_topk(self, queries, targets, cand_off, qidx, tidx, tbeg, tlen, mat, n, k, min_score=0, max_drop=-1, rebase=False, gapO=3,
                           gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False, out=None):
        """best k candidate windows per read (ssw_gpu_align_windows_topk): align_windows_best's groups and ranking, k ranks per group; rank
        r >= 1 only while its score1 >= score1(rank 0) - max_drop (max_drop < 0: no cut)
        -> (pos int32 [ngroups, k] -- positions in the group, -1 past the last --, n_eligible int32 [ngroups], records [ngroups, k] of
        RESULT_DTYPE -- the empty record where pos is -1 --, uint32 CIGAR pool in (group, rank) order).  rebase=True adds the chosen
        candidate's tbeg to ref_begin1, ref_end1 and ref_end2 where they are >= 0.  `out`: (pos, n_eligible, records) to fill."""
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1:
            raise ValueError("cand_off must be a 1-D array of ngroups + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        ng = int(co.shape[0]) - 1
        if ng > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[ngroups] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        k = int(k)
        kk = max(k, 0)                                # (the library refuses k < 1; the arrays only have to exist)
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            pos = np.zeros((ng, kk), dtype=np.int32)
            nel = np.zeros(ng, dtype=np.int32)
            res = np.zeros((ng, kk), dtype=RESULT_DTYPE)
        else:
            pos, nel, res = out
            if pos.dtype != np.int32 or nel.dtype != np.int32 or res.dtype != RESULT_DTYPE or pos.shape != (ng, kk) or nel.shape != (ng,) or \
                    res.shape != (ng, kk) or not pos.flags["C_CONTIGUOUS"] or not nel.flags["C_CONTIGUOUS"] or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous arrays: int32 [ngroups, k], int32 [ngroups], RESULT_DTYPE [ngroups, k]")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_align_windows_topk(self.h, queries.h, targets.h, co.ctypes.data_as(C.c_void_p), ng, qi.ctypes.data_as(C.c_void_p),
                                                 ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                 C.byref(p), k, int(min_score), int(max_drop), pos.ctypes.data_as(C.c_void_p),
                                                 nel.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                                 C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_windows_topk: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and ng > 0:
            hit = pos >= 0
            wb = np.zeros((ng, kk), dtype=np.int64)
            wb[hit] = tb[(co[:-1, None] + pos)[hit]]
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                v = res[f]
                res[f] = np.where(v >= 0, v + wb, v).astype(np.int32)
        return pos, nel, res, cig

    def align_windows_mates(self, queries, targets, cand_off, qidx, tidx, tbeg, tlen, nfwd, mat, n, min_insert, max_insert, unpaired_penalty,
                            min_score=0, rebase=False, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2, want_cigar=True,
                            mark_mismatch=False, out=None, orientation="fr", insert_penalty=None):
        """best candidate pair per read pair (ssw_gpu_align_windows_mates_lib): cand_off has 2 nfrag + 1 offsets, group 2 f the candidates of
        mate 1 of fragment f and group 2 f + 1 those of mate 2; candidate i is on the minus strand iff qidx[i] >= nfwd
        -> (sel [nfrag] of MATES_DTYPE, records [nfrag, 2] of RESULT_DTYPE -- the chosen candidates', or the empty record where pos1 / pos2
        is -1 --, uint32 CIGAR pool in (fragment, mate) order).  rebase=True adds the chosen candidate's tbeg to ref_begin1, ref_end1 and
        ref_end2 where they are >= 0.  `out`: (sel, records) to fill.  orientation: "fr" (default), "rf", "ff" or 0 .. 2 -- the
        library orientation of the proper-pair rule (SSW_GPU_MATES_*).  insert_penalty: None, or a 1-D integer array of
        max_insert - min_insert + 1 entries 0 .. 65535 -- what a proper combination of span min_insert + i pays
        (ssw_gpu_align_windows_mates_model; insert_penalty_normal builds one)."""
        orient = _orientation(orientation)
        table = None if insert_penalty is None else _insert_table(insert_penalty, min_insert, max_insert)
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1 or co.shape[0] % 2 != 1:
            raise ValueError("cand_off must be a 1-D array of 2 nfrag + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        nf = (int(co.shape[0]) - 1) // 2
        if nf > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[2 nfrag] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            sel = np.zeros(nf, dtype=MATES_DTYPE)
            res = np.zeros((nf, 2), dtype=RESULT_DTYPE)
        else:
            sel, res = out
            if sel.dtype != MATES_DTYPE or res.dtype != RESULT_DTYPE or sel.shape != (nf,) or res.shape != (nf, 2) or \
                    not sel.flags["C_CONTIGUOUS"] or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous arrays: MATES_DTYPE [nfrag], RESULT_DTYPE [nfrag, 2]")
        pool = _u32p()
        words = C.c_int64(0)
        if table is not None:
            pm = _pair_model(min_insert, max_insert, unpaired_penalty, orient, table)
            rc = self.lib.ssw_gpu_align_windows_mates_model(self.h, queries.h, targets.h, co.ctypes.data_as(C.c_void_p), nf,
                                                            qi.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                                                            tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), int(nfwd), C.byref(p),
                                                            int(min_score), C.byref(pm), sel.ctypes.data_as(C.c_void_p),
                                                            res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        else:
            rc = self.lib.ssw_gpu_align_windows_mates_lib(self.h, queries.h, targets.h, co.ctypes.data_as(C.c_void_p), nf, qi.ctypes.data_as(C.c_void_p),
                                                          ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                          int(nfwd), C.byref(p), int(min_score), int(min_insert), int(max_insert),
                                                          int(unpaired_penalty), orient, sel.ctypes.data_as(C.c_void_p),
                                                          res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_windows_mates: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and nf > 0:
            _mates_rebase(sel, res, co, tb)
        return sel, res, cig

    def insert_hist(self, queries, targets, cand_off, qidx, tidx, tbeg, tlen, nfwd, mat, n, max_span, min_margin=0, min_score=0, gapO=3, gapE=1,
                    maskLen=-1, score_size=2, flag=0, filters=0, filterd=0, mark_mismatch=False):
        """insert-size histogram of a library (ssw_gpu_insert_hist): groups, candidates and nfwd as align_windows_mates; per fragment the
        span between the best candidates of the two mates, where both exist, lead their runners-up by min_margin and lie on one target,
        under every orientation their strands allow -> (hist uint32 [3, max_span + 1], rows "fr" / "rf" / "ff" (MATES_ORIENTATION),
        counts: dict of ssw_gpu_insert_counts' fields, n_in / n_out as lists of three).  flag, filters, filterd and mark_mismatch are
        passed on and ignored by the library: the fill is flag 0's.  insert_fit turns a row into the numbers a mates call takes."""
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1 or co.shape[0] % 2 != 1:
            raise ValueError("cand_off must be a 1-D array of 2 nfrag + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        nf = (int(co.shape[0]) - 1) // 2
        if nf > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[2 nfrag] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        max_span = int(max_span)
        if max_span < 0 or max_span > 65535:          # (the histogram is allocated here: the library's own bound, before the allocation)
            raise ValueError("max_span must be 0 .. 65535")
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        hist = np.zeros((3, max_span + 1), dtype=np.uint32)
        cnt = INSERT_COUNTS()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.lib.ssw_gpu_insert_hist(self.h, queries.h, targets.h, vp(co), nf, vp(qi), vp(ti), vp(tb), vp(tl), int(nfwd), C.byref(p),
                                          int(min_score), int(min_margin), max_span, vp(hist), C.byref(cnt))
        if rc != 0:
            raise RuntimeError("ssw_gpu_insert_hist: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        counts = dict(n_both=cnt.n_both, n_unique=cnt.n_unique, n_same=cnt.n_same, n_in=list(cnt.n_in), n_out=list(cnt.n_out))
        return hist, counts

    def align_windows_mates_rescue(self, queries, targets, cand_off, qidx, tidx, tbeg, tlen, nfwd, mate_q, mat, n, min_insert, max_insert,
                                   unpaired_penalty, max_anchors=2, anchor_min_score=0, rescue_pad=16, min_score=0, rebase=False, gapO=3, gapE=1,
                                   flag=0, filters=0, filterd=0, maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False, orientation="fr",
                                   insert_penalty=None):
        """align_windows_mates with mate rescue on the device (ssw_gpu_align_windows_mates_rescue): every group is followed by max_anchors
        rescue slots, windows in which a proper partner of the OTHER mate's best candidates would lie; mate_q[2 f + h] is the forward read
        of mate h of fragment f, `queries` holds the reads and their reverse complements (with_revcomp: count == 2 nfwd)
        -> (sel [nfrag] of MATES_DTYPE with pos1 / pos2 in the AUGMENTED groups, records [nfrag, 2] of RESULT_DTYPE, origin [nfrag, 2] of
        RESCUED_DTYPE -- window, query and anchor of every chosen candidate --, uint32 CIGAR pool in (fragment, mate) order).  rebase=True
        adds origin["tbeg"] to ref_begin1, ref_end1 and ref_end2 where they are >= 0 (the winner's window may not be the caller's).
        insert_penalty as Context.align_windows_mates (ssw_gpu_align_windows_mates_rescue_model): the rescue windows do not depend on it,
        the selection over the augmented list does."""
        orient = _orientation(orientation)
        table = None if insert_penalty is None else _insert_table(insert_penalty, min_insert, max_insert)
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        mq = np.ascontiguousarray(mate_q, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1 or co.shape[0] % 2 != 1:
            raise ValueError("cand_off must be a 1-D array of 2 nfrag + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        nf = (int(co.shape[0]) - 1) // 2
        if mq.shape != (2 * nf,):
            raise ValueError("mate_q must be a 1-D array of 2 nfrag read indices")
        if nf > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[2 nfrag] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        sel = np.zeros(nf, dtype=MATES_DTYPE)
        res = np.zeros((nf, 2), dtype=RESULT_DTYPE)
        org = np.zeros((nf, 2), dtype=RESCUED_DTYPE)
        pool = _u32p()
        words = C.c_int64(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if table is not None:
            pm = _pair_model(min_insert, max_insert, unpaired_penalty, orient, table)
            rc = self.lib.ssw_gpu_align_windows_mates_rescue_model(self.h, queries.h, targets.h, vp(co), nf, vp(qi), vp(ti), vp(tb), vp(tl), int(nfwd),
                                                                   vp(mq), C.byref(p), int(min_score), C.byref(pm), int(max_anchors),
                                                                   int(anchor_min_score), int(rescue_pad), vp(sel), vp(res), vp(org),
                                                                   C.byref(pool) if want_cigar else None, C.byref(words))
        else:
            rc = self.lib.ssw_gpu_align_windows_mates_rescue(self.h, queries.h, targets.h, vp(co), nf, vp(qi), vp(ti), vp(tb), vp(tl), int(nfwd), vp(mq),
                                                             C.byref(p), int(min_score), int(min_insert), int(max_insert), int(unpaired_penalty), orient,
                                                             int(max_anchors), int(anchor_min_score), int(rescue_pad), vp(sel), vp(res), vp(org),
                                                             C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_align_windows_mates_rescue: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and nf > 0:
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                res[f] = np.where(res[f] >= 0, res[f] + org["tbeg"], res[f]).astype(res[f].dtype)
        return sel, res, org, cig

    def search_db(self, queries, targets, mat, n, gapO=3, gapE=1, maskLen=-1, score_size=2, chunk=0, on_chunk=None):
        """streamed database search (ssw_gpu_search_db): on_chunk(target_first, hits[nq, target_count] of HIT_DTYPE) is called for
        every chunk of targets while the device works on the next one (the array is only valid during the call; return a
        non-zero int to stop).  Without on_chunk the chunks are assembled: -> hits [nq, nt]."""
        assert HIT_DTYPE.itemsize == 16
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, 0, 0, 0, maskLen, score_size, 0)
        nq = queries.count
        whole = None if on_chunk is not None else np.zeros((nq, targets.count), dtype=HIT_DTYPE)
        err = []
        stopped = []        # what the caller's function returned to stop the search (any non-zero int, negative ones included)

        def cb(_user, tfirst, tcount, ptr):
            try:
                buf = (C.c_char * (nq * tcount * 16)).from_address(ptr)
                hits = np.frombuffer(buf, dtype=HIT_DTYPE).reshape(nq, tcount)
                if on_chunk is not None:
                    r = int(on_chunk(tfirst, hits) or 0)
                    if r:
                        stopped.append(r)
                    return r
                whole[:, tfirst:tfirst + tcount] = hits
                return 0
            except Exception as e:     # noqa: BLE001 -- an exception must not unwind through the C caller
                err.append(e)
                return -99

        rc = self.lib.ssw_gpu_search_db(self.h, queries.h, targets.h, C.byref(p), chunk, HITS_FN(cb), None)
        if err:
            raise err[0]
        if stopped and rc == stopped[0]:
            return rc               # "non-zero to stop, that value is returned" (include/ssw_gpu.h): not a library failure
        if rc == -2:
            raise RuntimeError("ssw_gpu_search_db: " + self.lib.ssw_gpu_strerror(rc).decode())
        if rc < 0:
            raise RuntimeError("ssw_gpu_search_db: " + self.error())
        return whole if on_chunk is None else rc

    def search_topk(self, queries, targets, k, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2,
                    mark_mismatch=False, min_score=1, chunk=0, want_cigar=True, out=None):
        """best k targets per query (ssw_gpu_search_topk): -> (tidx int32 [nq, k], records [nq, k] of RESULT_DTYPE, uint32 CIGAR pool
        in (q, r) order).  Slots past a query's last eligible target hold -1 / the empty record.  `out`: (tidx, records) to fill."""
        nq = queries.count
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            ti = np.zeros((nq, max(int(k), 0)), dtype=np.int32)
            res = np.zeros((nq, max(int(k), 0)), dtype=RESULT_DTYPE)
        else:
            ti, res = out
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_search_topk(self.h, queries.h, targets.h, C.byref(p), int(k), int(min_score), int(chunk),
                                          ti.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                          C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_search_topk: " + (self.lib.ssw_gpu_strerror(rc).decode() if rc == -2 else self.error()))
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        return ti, res, cig

    def result_array(self, nq, nt):
        """[nq, nt] result records in page-locked host memory (freed with the context)"""
        nbytes = int(nq) * int(nt) * RESULT_DTYPE.itemsize
        p = self.lib.ssw_gpu_host_alloc(self.h, nbytes)
        if not p:
            raise RuntimeError("ssw_gpu_host_alloc: " + self.error())
        self._pinned.append(p)
        buf = (C.c_char * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=RESULT_DTYPE).reshape(int(nq), int(nt))

    def timing(self):
        t = Timing()
        self.lib.ssw_gpu_last_timing_sized(self.h, C.byref(t), C.sizeof(t))     # sized: this mirror may be older than the library
        d = {k: getattr(t, k) for k, _ in Timing._fields_}
        d["fill_kernel"] = d["fill_kernel"].decode()
        return d

    def selftest_lanes(self):
        """diagnostic of libssw_hooks.so (include/ssw_gpu_diag.h); the product library does not export it"""
        out = np.zeros((16, 64), dtype=np.uint32)
        if self.lib.ssw_gpu_selftest_lanes(self.h, out.ctypes.data_as(_u32p)) != 0:
            raise RuntimeError("ssw_gpu_selftest_lanes: " + self.error())
        return out

    def valu_probe(self, blocks=4096, iters=2000):
        return float(self.lib.ssw_gpu_valu_probe(self.h, blocks, iters))

    def close(self):
        if self.h:
            for p in self._pinned:
                self.lib.ssw_gpu_host_free(self.h, p)
            self._pinned = []
            self.lib.ssw_gpu_close(self.h)
            self.h = None


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    for i, x in enumerate(seqs):
        off[i + 1] = off[i] + len(x)
    codes = np.concatenate([np.asarray(x, dtype=np.int8) for x in seqs]) if len(seqs) else np.zeros(0, dtype=np.int8)
    return np.ascontiguousarray(codes, dtype=np.int8), off


class Pool(object):
    """Several devices, one batch (include/ssw_gpu.h ssw_gpu_pool): per-GPU work queues over host-resident reads."""

    def __init__(self, devices=None, lib=None):
        self.lib = lib if lib is not None and not isinstance(lib, str) else load(lib)
        if devices is None:
            self.h = self.lib.ssw_gpu_pool_open(None, 0)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self.h = self.lib.ssw_gpu_pool_open(arr, len(devices))
        if not self.h:
            raise RuntimeError("ssw_gpu_pool_open: " + self.lib.ssw_gpu_last_error(None).decode())
        self.ntargets = 0

    def size(self):
        return int(self.lib.ssw_gpu_pool_size(self.h))

    def error(self):
        return self.lib.ssw_gpu_pool_last_error(self.h).decode()

    def set_targets(self, seqs):
        codes, off = _pack(seqs)
        if self.lib.ssw_gpu_pool_set_targets(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), len(seqs)) != 0:
            raise RuntimeError("ssw_gpu_pool_set_targets: " + self.error())
        self.ntargets = len(seqs)

    def align(self, reads, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2, block=0,
              want_cigar=True, mark_mismatch=False, packed=None):
        """reads: list of code arrays, or packed=(codes int8, offsets int64).  -> (records [nq, nt], CIGAR pool)"""
        codes, off = packed if packed is not None else _pack(reads)
        nq = len(off) - 1
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        res = np.zeros((nq, self.ntargets), dtype=RESULT_DTYPE)
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_pool_align(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), nq, block, 0, self.ntargets,
                                         C.byref(p), res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_pool_align: " + self.error())
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        return res, cig

    def search_topk(self, reads, k, mat, n, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2,
                    mark_mismatch=False, min_score=1, block=0, want_cigar=True, packed=None):
        """best k of the pool's targets per read (ssw_gpu_pool_search_topk) -> (tidx [nq, k], records [nq, k], CIGAR pool)"""
        codes, off = packed if packed is not None else _pack(reads)
        nq = len(off) - 1
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        ti = np.zeros((nq, max(int(k), 0)), dtype=np.int32)
        res = np.zeros((nq, max(int(k), 0)), dtype=RESULT_DTYPE)
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_pool_search_topk(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), nq, block, C.byref(p),
                                               int(k), int(min_score), ti.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                               C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_pool_search_topk: " + self.error())
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        return ti, res, cig

    def align_windows(self, reads, qidx, tidx, tbeg, tlen, mat, n, with_revcomp=False, rebase=False, block=0, gapO=3, gapE=1, flag=0, filters=0,
                      filterd=0, maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False, out=None, packed=None):
        """Context.align_windows over the pool (ssw_gpu_pool_align_windows): windows of the pool's targets, reads from the host (a list of
        code arrays, or packed=(codes int8, offsets int64)).  with_revcomp: qidx = nq + i names the reverse complement of read i.  block:
        pairs per block (0: a few blocks per worker) -- the output does not depend on it
        -> (numpy record array [npairs] of RESULT_DTYPE, numpy uint32 CIGAR pool in pair order); rebase and out as Context.align_windows."""
        codes, off = packed if packed is not None else _pack(reads)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        npairs = int(qi.shape[0])
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            res = np.zeros(npairs, dtype=RESULT_DTYPE)
        else:
            res = out
            if res.dtype != RESULT_DTYPE or res.shape != (npairs,) or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous [npairs] array of RESULT_DTYPE")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_pool_align_windows(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), len(off) - 1, 1 if with_revcomp else 0,
                                                 qi.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p),
                                                 tl.ctypes.data_as(C.c_void_p), npairs, int(block), C.byref(p), res.ctypes.data_as(C.c_void_p),
                                                 C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_pool_align_windows: " + self.error())
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase:
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                v = res[f]
                res[f] = np.where(v >= 0, v + tb, v).astype(np.int32)
        return res, cig

    def align_windows_topk(self, reads, cand_off, qidx, tidx, tbeg, tlen, mat, n, k, min_score=0, max_drop=-1, with_revcomp=False, rebase=False,
                           block=0, gapO=3, gapE=1, flag=0, filters=0, filterd=0, maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False,
                           out=None, packed=None):
        """Context.align_windows_topk over the pool (ssw_gpu_pool_align_windows_topk): reads from the host, windows of the pool's targets;
        with_revcomp: qidx = nq + i names the reverse complement of read i.  block: candidates per block of whole groups (0: a few blocks
        per worker) -- the output does not depend on it
        -> (pos int32 [ngroups, k], n_eligible int32 [ngroups], records [ngroups, k], uint32 CIGAR pool in (group, rank) order); rebase
        and out as Context.align_windows_topk.  k = 1 answers align_windows_best; k = 2 with max_drop < 0 adds its runner-up."""
        codes, off = packed if packed is not None else _pack(reads)
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1:
            raise ValueError("cand_off must be a 1-D array of ngroups + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        ng = int(co.shape[0]) - 1
        if ng > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[ngroups] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        k = int(k)
        kk = max(k, 0)                                # (the library refuses k < 1; the arrays only have to exist)
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            pos = np.zeros((ng, kk), dtype=np.int32)
            nel = np.zeros(ng, dtype=np.int32)
            res = np.zeros((ng, kk), dtype=RESULT_DTYPE)
        else:
            pos, nel, res = out
            if pos.dtype != np.int32 or nel.dtype != np.int32 or res.dtype != RESULT_DTYPE or pos.shape != (ng, kk) or nel.shape != (ng,) or \
                    res.shape != (ng, kk) or not pos.flags["C_CONTIGUOUS"] or not nel.flags["C_CONTIGUOUS"] or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous arrays: int32 [ngroups, k], int32 [ngroups], RESULT_DTYPE [ngroups, k]")
        pool = _u32p()
        words = C.c_int64(0)
        rc = self.lib.ssw_gpu_pool_align_windows_topk(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), len(off) - 1,
                                                      1 if with_revcomp else 0, co.ctypes.data_as(C.c_void_p), ng, qi.ctypes.data_as(C.c_void_p),
                                                      ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                      int(block), C.byref(p), k, int(min_score), int(max_drop), pos.ctypes.data_as(C.c_void_p),
                                                      nel.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                                      C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_pool_align_windows_topk: " + self.error())
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and ng > 0:
            hit = pos >= 0
            wb = np.zeros((ng, kk), dtype=np.int64)
            wb[hit] = tb[(co[:-1, None] + pos)[hit]]
            for f in ("ref_begin1", "ref_end1", "ref_end2"):
                v = res[f]
                res[f] = np.where(v >= 0, v + wb, v).astype(np.int32)
        return pos, nel, res, cig

    def align_windows_mates(self, reads, cand_off, qidx, tidx, tbeg, tlen, mat, n, min_insert, max_insert, unpaired_penalty, min_score=0,
                            orientation="fr", with_revcomp=False, rebase=False, block=0, gapO=3, gapE=1, flag=0, filters=0, filterd=0,
                            maskLen=-1, score_size=2, want_cigar=True, mark_mismatch=False, out=None, packed=None, insert_penalty=None):
        """Context.align_windows_mates over the pool (ssw_gpu_pool_align_windows_mates): reads from the host, windows of the pool's targets;
        cand_off has 2 nfrag + 1 offsets.  with_revcomp: qidx = nq + i names the reverse complement of read i -- the minus strand;
        without it everything is on the plus strand.  block: candidates per block of whole fragments (0: a few blocks per worker) -- the
        output does not depend on it
        -> (sel [nfrag] of MATES_DTYPE, records [nfrag, 2], uint32 CIGAR pool in (fragment, mate) order); orientation, rebase and out as
        Context.align_windows_mates; insert_penalty too (ssw_gpu_pool_align_windows_mates_model)."""
        orient = _orientation(orientation)
        table = None if insert_penalty is None else _insert_table(insert_penalty, min_insert, max_insert)
        codes, off = packed if packed is not None else _pack(reads)
        co = np.ascontiguousarray(cand_off, dtype=np.int64)
        qi = np.ascontiguousarray(qidx, dtype=np.int32)
        ti = np.ascontiguousarray(tidx, dtype=np.int32)
        tb = np.ascontiguousarray(tbeg, dtype=np.int64)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        if co.ndim != 1 or co.shape[0] < 1 or co.shape[0] % 2 != 1:
            raise ValueError("cand_off must be a 1-D array of 2 nfrag + 1 offsets")
        if qi.ndim != 1 or qi.shape != ti.shape or qi.shape != tb.shape or qi.shape != tl.shape:
            raise ValueError("qidx, tidx, tbeg and tlen must be 1-D arrays of the same length")
        nf = (int(co.shape[0]) - 1) // 2
        if nf > 0 and int(co[-1]) > qi.shape[0]:      # (the library reads cand_off[2 nfrag] candidates; everything else is its own check)
            raise ValueError("cand_off names more candidates than the arrays hold")
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        p = Params(mat.ctypes.data_as(_i8p), n, gapO, gapE, flag, filters, filterd, maskLen, score_size, 1 if mark_mismatch else 0)
        if out is None:
            sel = np.zeros(nf, dtype=MATES_DTYPE)
            res = np.zeros((nf, 2), dtype=RESULT_DTYPE)
        else:
            sel, res = out
            if sel.dtype != MATES_DTYPE or res.dtype != RESULT_DTYPE or sel.shape != (nf,) or res.shape != (nf, 2) or \
                    not sel.flags["C_CONTIGUOUS"] or not res.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be C-contiguous arrays: MATES_DTYPE [nfrag], RESULT_DTYPE [nfrag, 2]")
        pool = _u32p()
        words = C.c_int64(0)
        if table is not None:
            pm = _pair_model(min_insert, max_insert, unpaired_penalty, orient, table)
            rc = self.lib.ssw_gpu_pool_align_windows_mates_model(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), len(off) - 1,
                                                                 1 if with_revcomp else 0, co.ctypes.data_as(C.c_void_p), nf,
                                                                 qi.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                                                                 tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), int(block), C.byref(p),
                                                                 int(min_score), C.byref(pm), sel.ctypes.data_as(C.c_void_p),
                                                                 res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        else:
            rc = self.lib.ssw_gpu_pool_align_windows_mates(self.h, codes.ctypes.data_as(_i8p), off.ctypes.data_as(_i64p), len(off) - 1,
                                                           1 if with_revcomp else 0, co.ctypes.data_as(C.c_void_p), nf, qi.ctypes.data_as(C.c_void_p),
                                                           ti.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                           int(block), C.byref(p), int(min_score), int(min_insert), int(max_insert),
                                                           int(unpaired_penalty), orient, sel.ctypes.data_as(C.c_void_p),
                                                           res.ctypes.data_as(C.c_void_p), C.byref(pool) if want_cigar else None, C.byref(words))
        if rc != 0:
            raise RuntimeError("ssw_gpu_pool_align_windows_mates: " + self.error())
        cig = np.ctypeslib.as_array(pool, shape=(words.value,)).copy() if want_cigar and words.value > 0 else np.zeros(0, dtype=np.uint32)
        if want_cigar and pool:
            C.CDLL(None).free(pool)
        if rebase and nf > 0:
            _mates_rebase(sel, res, co, tb)
        return sel, res, cig

    def stats(self):
        out = []
        for w in range(self.size()):
            st = PoolStat()
            self.lib.ssw_gpu_pool_stats(self.h, w, C.byref(st))
            out.append({k: getattr(st, k) for k, _ in PoolStat._fields_})
        return out

    def close(self):
        if self.h:
            self.lib.ssw_gpu_pool_close(self.h)
            self.h = None
