"""bench.py's plain line and --dump-outputs, on the emulated library (tests/emu): a run without --full times its steps and prints the
contract fields only; the dumped arrays are what the last timed step returned, the same from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

from sswutil import dna_matrix, oracle_align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("parity", "cpu_baseline", "roofline", "roofline_hbm", "value_with_h2d", "value_default_budget", "also")


def _bench(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _arrays(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(str(d), "*.npy")))}


def test_plain_run_times_only_its_steps(emu_lib_path):
    out = _bench(["--steps", "3", "--warmup", "1", "--reads", "4", "--ref-len", "2000", "--read-len", "60", "--lib", emu_lib_path])
    assert out["metric"] == "GCUPS" and out["unit"] == "GCUPS" and out["higher_is_better"] is True and out["dtype"]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] >= 0
    assert not [k for k in EXTRAS if k in out], out.keys()


def test_dump_outputs_are_the_timed_results(emu_lib_path, tmp_path):
    args = ["--steps", "2", "--warmup", "0", "--reads", "5", "--ref-len", "2000", "--read-len", "60", "--flag", "2", "--lib", emu_lib_path]
    _bench(args + ["--dump-outputs", str(tmp_path / "a")], env={"SSW_BENCH_DUMP": str(tmp_path)})
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    a, b = _arrays(tmp_path / "a"), _arrays(tmp_path / "b")
    assert set(a) == set(b) >= {"score1", "score2", "ref_begin1", "ref_end1", "read_begin1", "read_end1", "ref_end2", "cigarLen", "cigar"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert "row_index" not in a and len(a["score1"]) == 5 and a["cigarLen"].sum() == len(a["cigar"])
    z = np.load(str(tmp_path / "rank0.npz"))
    mat = dna_matrix(2, 2)
    at = 0
    for i, rd in enumerate(z["reads"]):
        d, cig = oracle_align(rd, mat, 5, z["ref"], 3, 1, 2, 0, 0, len(rd) // 2, 2, 0)
        for k in ("score1", "score2", "ref_begin1", "ref_end1", "read_begin1", "read_end1", "ref_end2"):
            assert a[k][i] == d[k] == z["res"][i, 0][k], (i, k)
        n = int(a["cigarLen"][i])
        assert [int(x) for x in a["cigar"][at:at + n]] == cig, i
        at += n


def test_dump_outputs_of_the_database_search(emu_lib_path, tmp_path):
    args = ["--config", "5", "--steps", "1", "--warmup", "0", "--reads", "12", "--db-targets", "5", "--db-chunk", "2", "--lib", emu_lib_path]
    for d in ("a", "b"):
        _bench(args + ["--dump-outputs", str(tmp_path / d)])
    a, b = _arrays(tmp_path / "a"), _arrays(tmp_path / "b")
    assert set(a) == {"score1", "score2", "ref_end1", "read_end1", "ref_end2", "query_index"}
    assert list(a["query_index"]) == list(range(12)) and a["score1"].shape == (12, 5)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_of_the_stated_size_job(emu_lib_path, tmp_path):
    """config 3 --stated-size: the records of every read block of the job, block after block"""
    out = _bench(["--config", "3", "--stated-size", "--blocks", "3", "--steps", "1", "--warmup", "1", "--reads", "3", "--ref-len", "2500",
                  "--read-len", "70", "--dump-outputs", str(tmp_path), "--lib", emu_lib_path])
    assert out["scaling"] == "strong" and out["steps"] == 1 and not [k for k in EXTRAS if k in out]
    a = _arrays(tmp_path)
    assert len(a["score1"]) == 9 and "cigar" not in a and (a["ref_begin1"] == -1).all()
