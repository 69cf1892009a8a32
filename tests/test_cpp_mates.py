"""include/ssw_gpu_cpp.h BatchAligner::AlignWindowsMates against BatchAligner::AlignWindows over all candidates plus the proper-pair rule on
the host (tests/cpp/windows_mates_check.cpp): the three library orientations, winners on the reverse strand checked through
reverse-complemented query strings -- the '=' / 'X' CIGAR strings included --, rebase true and false.  On the CPU SIMT emulator and, marked
gpu, on the MI355X."""
import os
import subprocess

import pytest


def _cpp_check(lib_dir, lib_name, tmp_path, args):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / ("windows_mates_check_" + lib_name))
    subprocess.run(["g++", "-O2", "-std=c++11", "-I" + os.path.join(os.path.dirname(here), "include"), os.path.join(here, "cpp", "windows_mates_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-l" + lib_name, "-lm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_cpp_align_windows_mates_emulated(emu_lib_path, tmp_path):
    _cpp_check(os.path.dirname(emu_lib_path), "ssw_emu", tmp_path, ["18", "2"])


@pytest.mark.gpu
def test_cpp_align_windows_mates_gpu(product_lib_path, tmp_path):
    _cpp_check(os.path.dirname(product_lib_path), "ssw", tmp_path, ["600", "3"])
