"""RC_GEMM_SPREAD changes scheduling only: all nine outputs of rc_rsvd_id_f64 with the switch off (every product of the chain through
gemm) and at its default (the Gram and shallow products on more and smaller workgroups), bit for bit.

The switch is read once per process, so each value runs in a fresh child process (tests/spread_products_worker.py), at hint 4 and
4 kernel slots, eager and replayed from a captured graph, every output poisoned before each run.  The stage timers of the two
processes must carry the same names (same products, same slab counts)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("range_q", "u", "s", "vt", "qr_q", "qr_r", "qr_ind", "id_c", "id_z")


def _worker(tmp_path, tag, shapes, **env_changes):
    env = {k: v for k, v in os.environ.items() if k != "RC_GEMM_SPREAD"}
    env.update(env_changes)
    out = str(tmp_path / (tag + ".npz"))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spread_products_worker.py"), out] + ["%d,%d,%d,%d" % s for s in shapes],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1 and json.loads(lines[0][7:]) == [], res.stdout[-2000:]
    return np.load(out)


def _compare(off, on, shapes):
    for (m, n, k, p) in shapes:
        tag = "%dx%d" % (m, n)
        assert list(off[tag + ".names"]) == list(on[tag + ".names"]), tag
        ref = {name: off["%s.eager.%s" % (tag, name)] for name in OUTPUTS}
        for name in OUTPUTS:
            assert not np.isnan(ref[name]).any() and not (name == "qr_ind" and (ref[name] < 0).any()), (tag, name)
            for run, mode in ((off, "replayed"), (on, "eager"), (on, "replayed")):
                got = run["%s.%s.%s" % (tag, mode, name)]
                assert np.array_equal(ref[name], got), (tag, mode, name, float(np.abs(ref[name].astype(np.float64) - got.astype(np.float64)).max()))
        print(tag, "last product: off", off[tag + ".last"], "| on", on[tag + ".last"])


def test_switch_off_against_default(tmp_path):
    """1024 x 1024, k = 128, p = 5: the smallest shape the fused consumers take; its tall side is under 2048, so only the Gram arm is
    active.  2048 x 2048: both arms, and the shallow products in two K slabs.  The last product of a compression is U = range ub."""
    shapes = [(1024, 1024, 128, 5), (2048, 2048, 128, 5)]
    off = _worker(tmp_path, "off", shapes, RC_GEMM_SPREAD="0")
    on = _worker(tmp_path, "on", shapes)
    _compare(off, on, shapes)
    assert str(off["1024x1024.last"]) == str(on["1024x1024.last"])
    assert ",128,128,16,1,8," in str(off["2048x2048.last"]), off["2048x2048.last"]
    assert ",128,32,16,4,2," in str(on["2048x2048.last"]), on["2048x2048.last"]


def test_switch_off_against_default_second_cholesky_pass_forced(tmp_path):
    """The same at 2048 x 2048 under RC_CHOLQR_SKIP=0: the second pass of every CholeskyQR2 factors its Gram matrix, so the second
    Gram product's value reaches the outputs and is not only compared with the identity."""
    shapes = [(2048, 2048, 128, 5)]
    off = _worker(tmp_path, "off_noskip", shapes, RC_GEMM_SPREAD="0", RC_CHOLQR_SKIP="0")
    on = _worker(tmp_path, "on_noskip", shapes, RC_CHOLQR_SKIP="0")
    _compare(off, on, shapes)
