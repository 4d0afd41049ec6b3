"""The per-(kernel, device) record of raised dynamic-LDS limits (cqa-crct_amd/csrc/lds_limit.h) on its own: the header includes nothing
from HIP, so tests/lds_limit_check.cpp is built with the host compiler and run here -- no GPU, no Python extension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["first_use_needs_raise",                      # (k, device 0, 96 KB)
         "recorded_key_is_settled",                    # ... recorded: the same key (and anything below it) no longer
         "other_device_needs_raise",                   # (k, device 1, 96 KB) still does: the attribute is per device
         "more_bytes_need_raise_again",                # (k, device 0, 150 KB)
         "limit_only_rises",
         "second_kernel_is_independent",
         "second_kernel_settled",
         "up_to_64k_never_needs_raise",
         "device_out_of_range_always_needs_raise",
         "two_threads_same_state_as_one",              # disjoint and equal keys recorded by two threads at once
         "two_threads_expected_limits",
         "lookup_during_record_goes_settled_once",     # one thread asks while another records: true -> false, never back
         "full_table_degrades_to_always_raise"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lds_limit") / "lds_limit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "cqa-crct_amd", "csrc"),
                            os.path.join(ROOT, "tests", "lds_limit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return run.returncode, dict(line.split() for line in run.stdout.splitlines())


def test_header_includes_nothing_from_hip():
    with open(os.path.join(ROOT, "cqa-crct_amd", "csrc", "lds_limit.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(inc in ("<atomic>", "<cstddef>", "<cstdint>") for inc in includes), includes


@pytest.mark.parametrize("case", CASES)
def test_lds_limit_bookkeeping(report, case):
    status, lines = report
    assert lines.get(case) == "ok", (case, lines)


def test_every_case_ran_and_passed(report):
    status, lines = report
    assert status == 0 and sorted(lines) == sorted(CASES), (status, lines)
