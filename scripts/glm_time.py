"""Times the ABC-GLM posterior of the batched ranking (abc_glm_rank_targets_dev) beside the loclinear density product
(abc_rank_targets_density_dev, method 1) on the same fitted model at the same shape: by default N = 1e5 rows, M = 32 metrics,
P = 16 parameters, A = 8 components, B = 1000 targets, K = 1e4, G = 512.  Both calls write dens and the modes.  Wall ms per call
between device synchronisations, median (min .. max) of --reps after one warm-up, the two calls alternating.  Writes a text table
(default profiles/glm.txt).  One timing, no bar attached."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--G", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm.txt"))
    a = ap.parse_args()
    N, M, P, A, B, K, G = a.N, 32, 16, 8, a.B, a.K, a.G
    dev = "cuda:0"
    wl = synthetic.Workload(M, P, 2024)
    X, Y = wl.rows(0, N)
    Xd, Yd = device.colmajor(X, dev), device.colmajor(Y, dev)
    L = _lib.lib()
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=dev)
    model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=dev)
    zero = torch.zeros(M, dtype=torch.float64, device=dev)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, N // 2, stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), zero.data_ptr(), M, P, A, _lib.RULE_MIN_PRESS, model.data_ptr()))
    torch.cuda.synchronize()
    nc = int(model[0].item())
    T, _ = wl.rows_by_index((1 << 40) + np.arange(B))
    Td = device.colmajor(T, dev)
    status = {}

    def glm():
        r = device.rank_targets_glm(Xd, model, A, Td, K, Yd, G=G, outputs=("dens", "lo_x", "step", "mode", "mode_dens", "mean", "var",
                                                                           "ess", "log_md", "status"), ctx=ctx)
        status["glm"] = r["status"]

    def loclinear():
        device.rank_targets_density(Xd, model, A, Td, K, Yd, G=G, method=_lib.POSTERIOR_LOCLINEAR, ctx=ctx)

    calls = (("glm", glm), ("loclinear density", loclinear))
    ts = {k: [] for k, _ in calls}
    for _, fn in calls:
        fn()
        torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in calls:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    fitted = int((status["glm"] == 0).sum().item())
    lines = ["# scripts/glm_time.py on %s: N = %d, M = %d, P = %d, A = %d (nc = %d), B = %d, K = %d, G = %d" %
             (torch.cuda.get_device_name(0), N, M, P, A, nc, B, K, G),
             "# wall ms per call: median (min .. max) of %d after one warm-up, the two calls alternating; both write dens and the modes"
             % a.reps,
             "# glm: abc_glm_rank_targets_dev (%d of %d targets with status 0); loclinear density: abc_rank_targets_density_dev, method 1"
             % (fitted, B)]
    for k, _ in calls:
        v = np.array(ts[k])
        lines.append("%-20s %10.3f (%.3f .. %.3f)" % (k, np.median(v), v.min(), v.max()))
    lines.append("glm / loclinear density: %.3f" % (np.median(ts["glm"]) / np.median(ts["loclinear density"])))
    lines.append("# kernel evaluations of the glm density: B P K G = %.3g" % (float(B) * P * K * G))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
