"""Worker of tests/test_gpu_spread_switch.py: one fresh process per value of RC_GEMM_SPREAD (read once per process).  Runs
rc_rsvd_id_f64 at hint 4, 4 kernel slots, on the shapes given as "m,n,k,p" arguments, eager and replayed from a captured graph,
outputs poisoned before each run, and writes all nine outputs of every run into the .npz named by the first argument, with the
stage timers' names and the instantiation of the last product.  Prints "RESULT <json>" with the health failures (none expected)."""
import ctypes, json, os, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import npy
from tests.small_product_cases import op_names

out_path, shapes = sys.argv[1], [tuple(int(x) for x in s.split(",")) for s in sys.argv[2:]]
lib = _lib.lib()
last = lib.rc_last_gemm_kernel_name
last.restype = ctypes.c_char_p
last.argtypes = [ctypes.c_void_p]
failures, saved = [], {}

for (m, n, k, p) in shapes:
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = rc.random_gaussian((m, n), rc.Rng(41), torch.float64)
        mk = lambda r, c: torch.empty((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
        b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.empty(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
                 qr_ind=torch.empty(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
        o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                                 _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
        st.synchronize()

        def run():
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(7), ctypes.byref(o_))

        def poison():
            for t in b.values():
                t.fill_(float("nan") if t.is_floating_point() else -1)

        def keep(mode):
            ctx.synchronize()
            if ctx.get_health() != 0:
                failures.append(("health", m, n, mode, ctx.get_health()))
            for name, t in b.items():
                saved["%dx%d.%s.%s" % (m, n, mode, name)] = npy(t).copy()

        ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, 4)
        ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 4)
        poison()
        lib.rc_profile_enable(ctx._h, 1)
        lib.rc_profile_reset(ctx._h)
        run()
        names = sorted(op_names(ctx, lib))
        lib.rc_profile_enable(ctx._h, 0)
        keep("eager")
        saved["%dx%d.names" % (m, n)] = np.array(names)
        saved["%dx%d.last" % (m, n)] = np.array(last(ctx._h).decode())
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        run()
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        poison()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        keep("replayed")
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()

np.savez(out_path, **saved)
print("RESULT " + json.dumps(failures))
