"""Times the exact quantiles and CDF of the ABC-GLM posterior (abc_glm_rank_targets_summary_dev) beside the calls they are to be
compared with, on one fitted model at scripts/glm_time.py's shape: by default N = 1e5 rows, M = 32 metrics, P = 16 parameters, A = 8
components, B = 1000 targets, K = 1e4, G = 512.
  (a) the ABC-GLM call with mean, var and log_md only
  (b) the same plus quant at {0.025, 0.25, 0.5, 0.75, 0.975} and cdf at a truth
  (c) the same as (a) plus dens and the modes
  (d) abc_rank_targets_summary_dev, method 1 (loclinear), at the same levels with the same truth
Wall ms per call between device synchronisations, median (min .. max) of --reps after one warm-up, the calls alternating.  Writes a
text table (default profiles/glm_summary.txt).  --only-old times (a) and (c) alone, which is what a tree without the *_summary
entries can run.  One timing, no bar attached."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402

LEVELS = (0.025, 0.25, 0.5, 0.75, 0.975)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--G", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-old", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_summary.txt"))
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
    T, Tth = wl.rows_by_index((1 << 40) + np.arange(B))
    Td = device.colmajor(T, dev)
    truth = torch.tensor(np.ascontiguousarray(Tth), device=dev)
    few = ("mean", "var", "log_md", "status")
    keep = {}

    def moments():
        keep["a"] = device.rank_targets_glm(Xd, model, A, Td, K, Yd, G=G, outputs=few, ctx=ctx)

    def quantiles():
        keep["b"] = device.rank_targets_glm(Xd, model, A, Td, K, Yd, G=G, outputs=few, ctx=ctx, probs=LEVELS, truth=truth)

    def density():
        keep["c"] = device.rank_targets_glm(Xd, model, A, Td, K, Yd, G=G, outputs=few + ("dens", "lo_x", "step", "mode", "mode_dens"), ctx=ctx)

    def loclinear():
        device.rank_targets_summary(Xd, model, A, Td, K, Yd, probs=LEVELS, truth=truth, method=_lib.POSTERIOR_LOCLINEAR, ctx=ctx)

    calls = [("(a) glm moments", moments), ("(b) glm quantiles", quantiles), ("(c) glm density", density), ("(d) loclinear summary", loclinear)]
    if a.only_old:
        calls = [calls[0], calls[2]]
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
    fitted = int((keep["a"]["status"] == 0).sum().item())
    lines = ["# scripts/glm_summary_time.py on %s: N = %d, M = %d, P = %d, A = %d (nc = %d), B = %d, K = %d, G = %d" %
             (torch.cuda.get_device_name(0), N, M, P, A, nc, B, K, G),
             "# wall ms per call: median (min .. max) of %d after one warm-up, the calls alternating; %d of %d targets with status 0"
             % (a.reps, fitted, B),
             "# (a) mean, var, log_md; (b) the same plus quant at %s and cdf; (c) as (a) plus dens and the modes;" % (LEVELS,),
             "# (d) abc_rank_targets_summary_dev, method 1, at the same levels"]
    med = {}
    for k, _ in calls:
        v = np.array(ts[k])
        med[k[:3]] = np.median(v)
        lines.append("%-24s %10.3f (%.3f .. %.3f)" % (k, np.median(v), v.min(), v.max()))
    if not a.only_old:
        lines.append("(b) - (a): %.3f   (c) - (a): %.3f   ratio %.3f" % (med["(b)"] - med["(a)"], med["(c)"] - med["(a)"],
                                                                         (med["(b)"] - med["(a)"]) / (med["(c)"] - med["(a)"])))
        q = keep["b"]["quant"]
        lines.append("# the median of parameter 0 of target 0: %.6f; truth_cdf in [0.025, 0.975] for %.3f of the (target, parameter) pairs"
                     % (q[0, 2, 0].item(), ((keep["b"]["cdf"] >= 0.025) & (keep["b"]["cdf"] <= 0.975)).double().mean().item()))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
