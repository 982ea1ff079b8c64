"""Times the local-linear adjustment of the batched ranking (abc_rank_targets_adjust_dev) against the plain batched ranking
(abc_rank_targets_dev) on the same fitted model, at N = 1e6 rows, M = 32 metrics, P = 16 parameters, A = 8 components,
K = 1e4, B in {1, 16, 256, 1024}.  Columns: the plain call, the adjusted call writing coef only, the adjusted call writing theta
and the weights too, and the coef-only call with the row gather forced through the row-major table or straight from the scores
(diagnostic switch ABC_ADJ_GATHER under ABC_DIAG=1).  Writes a text table (default profiles/adjust_time.txt).
--only B: one adjusted call (theta written) at that B, nothing written (for a rocprofv3 kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

os.environ["ABC_DIAG"] = "1"          # (read once, at the library's first getenv; ABC_ADJ_GATHER is read per call)
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--B", type=str, default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjust_time.txt"))
    a = ap.parse_args()
    N, M, P, A, K = a.N, 32, 16, 8, a.K
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
    Bs = [a.only] if a.only else [int(b) for b in a.B.split(",")]
    T, _ = wl.rows_by_index((1 << 40) + np.arange(max(Bs)))
    Td_all = device.colmajor(T, dev)

    def plain(B):
        device.rank_targets(Xd, model, A, Td_all[:, :B], K, ctx=ctx)

    def adjusted(B, theta, gather=None):
        if gather:
            os.environ["ABC_ADJ_GATHER"] = gather
        else:
            os.environ.pop("ABC_ADJ_GATHER", None)
        device.rank_targets_adjust(Xd, model, A, Td_all[:, :B], K, Yd, theta=theta, weight=theta, ctx=ctx)

    if a.only:
        adjusted(a.only, True)
        torch.cuda.synchronize()
        return

    def timeit(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    lines = ["# scripts/adjust_time.py on %s: N = %d, M = %d, P = %d, A = %d (nc = %d), K = %d; wall ms per call (median of %d, "
             "after one warm-up)" % (torch.cuda.get_device_name(0), N, M, P, A, nc, K, a.reps),
             "# plain: abc_rank_targets_dev (idx, dist); coef: abc_rank_targets_adjust_dev writing coef only; theta: also theta and "
             "weight (B K P + B K doubles)",
             "# coef_table / coef_direct: the coef-only call with the gather forced through the row-major table / straight from the "
             "scores (default rule: table when 4 B K >= N)",
             "%6s %10s %10s %10s %10s %10s %12s %12s" % ("B", "plain_ms", "coef_ms", "theta_ms", "+coef_ms", "+theta_ms",
                                                         "coef_table", "coef_direct")]
    for B in Bs:
        tp = timeit(lambda: plain(B), a.reps)
        tc = timeit(lambda: adjusted(B, False), a.reps)
        tt = timeit(lambda: adjusted(B, True), a.reps)
        ta = timeit(lambda: adjusted(B, False, "table"), a.reps)
        td = timeit(lambda: adjusted(B, False, "direct"), a.reps)
        lines.append("%6d %10.3f %10.3f %10.3f %10.3f %10.3f %12.3f %12.3f" % (B, tp, tc, tt, tc - tp, tt - tp, ta, td))
        print(lines[-1], flush=True)
    os.environ.pop("ABC_ADJ_GATHER", None)
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
