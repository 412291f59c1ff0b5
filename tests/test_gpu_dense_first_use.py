"""The dense kernels' first use from two host threads at once (tests/cpp/dense_first_use_example.cpp), in a fresh process so that
every first use is one: two threads with a context each run the pivoted QR and the SVD of a 1024 x 96 f64 matrix, whose CholeskyQR2
route launches four kernels above the default 64 KiB of dynamic LDS; the main thread repeats the calls afterwards.  Every status is
RC_OK, every health word 0, and the three result sets are equal byte for byte."""
import os
import subprocess

import pytest

from tests.test_abi_cpu import build_cpp_mirror_examples

pytestmark = pytest.mark.gpu


def test_two_threads_reach_the_dense_kernels_first_use_together(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "dense_first_use_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
