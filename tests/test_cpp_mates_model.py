"""include/ssw_gpu_cpp.h BatchAligner::AlignWindowsMates with an insert_penalty table (the pair model of include/ssw_gpu.h) against
BatchAligner::AlignWindows over all candidates plus the model's rule on the host (tests/cpp/mates_model_check.cpp): the three library
orientations, two tables, nullptr equal to the call without the argument, a table of the wrong length refused.  On the CPU SIMT emulator
and, marked gpu, on the MI355X."""
import os
import subprocess

import pytest


def _cpp_check(lib_dir, lib_name, tmp_path, args):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / ("mates_model_check_" + lib_name))
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "mates_model_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-l" + lib_name, "-lm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_cpp_align_windows_mates_model_emulated(emu_lib_path, tmp_path):
    _cpp_check(os.path.dirname(emu_lib_path), "ssw_emu", tmp_path, ["18", "2"])


@pytest.mark.gpu
def test_cpp_align_windows_mates_model_gpu(product_lib_path, tmp_path):
    _cpp_check(os.path.dirname(product_lib_path), "ssw", tmp_path, ["600", "3"])
