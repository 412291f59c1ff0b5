"""Worker of test_non_skip_arithmetic_forced: a fresh process under RC_CHOLQR_SKIP=0 (read once per process), in which the second
pass of every CholeskyQR2 runs its factorization, so r = R2 R1, w = R2^-1 Q2, top = Q1[:k, :] w and small = R2^-1 Vc are real
products on Gaussian inputs too.  Compares, bit for bit, fused consumers on against off (all nine outputs of rc_rsvd_id_f64, eager
and replayed) and hint 1 against hint 8 (rc_pivoted_qr_f64), then holds the QR results to LAPACK.  Prints "RESULT <json>"."""
import ctypes, json, os, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
assert os.environ.get("RC_CHOLQR_SKIP") == "0"
import numpy as np
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests.helpers import npy
from tests.small_product_cases import pivoted_qr_at, qr_identities, small_products_left

failures = []
lib = _lib.lib()

# ---- fused consumers on against off: 1024 x 1024, k = 128, p = 5 (hint 4, 4 slots)
m = n = 1024
k, p = 128, 5
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
    a = rc.random_gaussian((m, n), rc.Rng(41), torch.float64)
    mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
             qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
    o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                             _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
    st.synchronize()

    def run():
        ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(7), ctypes.byref(o_))

    ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, 4)
    ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 4)
    runs = {}
    for fused in (0, 1):
        ctx.set_option(_lib.RC_OPT_FUSED_CONSUMERS, fused)
        for t in b.values():
            t.zero_()
        run()
        ctx.synchronize()
        if ctx.get_health() != 0:
            failures.append(("health", fused, "eager", ctx.get_health()))
        runs[(fused, "eager")] = {k_: npy(v).copy() for k_, v in b.items()}
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        run()
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        for t in b.values():
            t.zero_()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        if ctx.get_health() != 0:
            failures.append(("health", fused, "replayed", ctx.get_health()))
        runs[(fused, "replayed")] = {k_: npy(v).copy() for k_, v in b.items()}
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
    ctx.close()
ref = runs[(0, "eager")]
for key, got in runs.items():
    for name in ref:
        if not np.array_equal(ref[name], got[name]):
            failures.append(("fused on/off", key, name, float(np.abs(ref[name].astype(np.float64) - got[name].astype(np.float64)).max())))
g = runs[(1, "eager")]
if not np.abs(g["qr_q"].T @ g["qr_q"] - np.eye(k)).max() <= 1e-12:
    failures.append(("qr_q not orthonormal",))
if not np.linalg.norm((g["u"] * g["s"]) @ g["vt"] - g["range_q"] @ (g["range_q"].T @ npy(a))) / np.linalg.norm(npy(a)) <= 1e-12:
    failures.append(("u s vt is not the projection of a on its range",))

# ---- hint 1 (Q2 and the products on several workgroups) against hint 8 (inside k_qrcp_small, the products in their own launch)
for (mm, nn, kk, seed) in ((1024, 65, 65, 65), (1024, 133, 128, 133)):
    x = np.random.default_rng(seed).standard_normal((mm, nn))
    got = pivoted_qr_at(x, kk, [(1, 8), (8, 8)])
    (q1, r1, i1, n1), (q8, r8, i8, n8) = got[(1, 8)], got[(8, 8)]
    if not (np.array_equal(q1, q8) and np.array_equal(r1, r8) and np.array_equal(i1, i8)):
        failures.append(("hint 1 / hint 8", nn, float(np.abs(q1 - q8).max()), float(np.abs(r1 - r8).max())))
    if not any("qrcp_small_q2" in nm for nm in n1) or any("qrcp_small_q2" in nm for nm in n8):
        failures.append(("Q2 launch at the wrong hint", nn))
    for names in (n1, n8):
        if small_products_left(names):
            failures.append(("small products left", nn, small_products_left(names)))
    try:
        qr_identities(x, kk, q1, r1, i1, o.pivoted_qr(x))
    except AssertionError as e:  # reported, not raised: the parent test shows every failure at once
        failures.append(("identities", nn, str(e)))

print("RESULT " + json.dumps(failures))
