"""CPU checks of the dense launch sites' first-use path (rusty_compression_amd/csrc/rc_launch.hpp).

tests/cpp/first_use_test.cpp exercises the guard itself, rc::FirstUse, without HIP and without the library: eight threads over four
device numbers, device numbers outside 0..63, an action that throws.  tests/cpp/dense_first_use_example.cpp is the two-thread first
use on a device; here it is only compiled and linked (tests/test_gpu_dense_first_use.py runs it)."""
import os
import re
import subprocess

from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rusty_compression_amd", "csrc")


def test_first_use_guard_runs_once_per_device_and_waits(tmp_path):
    exe = os.path.join(str(tmp_path), "first_use_test")
    cmd = ["g++", "-std=c++17", "-pthread", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
           os.path.join(ROOT, "tests", "cpp", "first_use_test.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ALL OK" in res.stdout and "FAILED" not in res.stdout, res.stdout + res.stderr


def test_dense_first_use_example_compiles_and_links(tmp_path):
    assert os.path.exists(build_cpp_mirror_examples(tmp_path, "dense_first_use_example.cpp"))


def test_launch_sites_share_one_first_use_path_and_one_lds_budget():
    """No hand-written per-device table is left outside kernels_wqcoop.hip's mutex-guarded ones, the CU's LDS size is written once,
    and the attribute call stands in rc_launch.hip alone."""
    budget, attribute = [], []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        assert "attr_set" not in text, name
        if name != "kernels_wqcoop.hip":
            assert "& 63]" not in text, name
        if re.search(r"160 \* 1024", text):
            budget.append(name)
        if "hipFuncSetAttribute" in text:
            attribute.append(name)
    assert budget == ["rc_launch.hpp"], budget
    assert attribute == ["rc_launch.hip"], attribute
