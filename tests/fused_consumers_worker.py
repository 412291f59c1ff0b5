"""Worker of test_fused_launch_on_fresh_workspace_memory: a fresh process whose first call is an rc_rsvd_id_f64 that qualifies for
the fused launch of the pivoted QR of B and the Jacobi SVD of its core (4096 x 2048, k = 128, p = 5; RC_OPT_FUSED_CONSUMERS at
its default).  Prints a digest of every output, the health word, and whether the fused launch ran (a second, timed call)."""
import ctypes, hashlib, json, os, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib

m, n, k, p = 4096, 2048, 128, 5
lib = _lib.lib()
ctx = _lib.default_context()
a = rc.random_gaussian((m, n), rc.Rng(21), torch.float64)
mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
         qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                         _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))


def run():
    ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(3), ctypes.byref(o_))


run()
ctx.synchronize()
out = {"health": ctx.get_health()}
for name, t in b.items():
    out[name] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
lib.rc_profile_enable(ctx._h, 1)
lib.rc_profile_reset(ctx._h)
run()
cnt = ctypes.c_int32(0)
ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
ran = False
for i in range(cnt.value):
    nm = ctypes.create_string_buffer(192)
    ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
    ctx.check(lib.rc_profile_get(ctx._h, i, nm, 192, ctypes.byref(ms), ctypes.byref(calls)))
    ran = ran or "+ jacobi_svd" in nm.value.decode()
lib.rc_profile_enable(ctx._h, 0)
ctx.synchronize()
out["fused_launch_ran"] = ran
print("DIGESTS " + json.dumps(out))
