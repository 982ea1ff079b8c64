"""Times the batched ranking of B observed targets (abc_rank_targets_dev) against today's per-target device loop on the same
fitted model (abc_project_distance_dev + abc_select_smallest_dev with the record's observed scores replaced), at N = 1e6 rows,
M = 32 metrics, P = 16 parameters, A = 8 components, K = 1e4, B in {1, 16, 256, 1024}.  Writes a text table (default
profiles/targets_time.txt).  --only B: one batched call at that B, nothing written (for a rocprofv3 kernel-trace run)."""
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
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--B", type=str, default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_time.txt"))
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
    ml = L.abc_model_len(M, P, A)
    model = torch.empty(ml, dtype=torch.float64, device=dev)
    zero = torch.zeros(M, dtype=torch.float64, device=dev)
    ntr = N // 2
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, ntr, stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), zero.data_ptr(), M, P, A, _lib.RULE_MIN_PRESS, model.data_ptr()))
    torch.cuda.synchronize()
    Bs = [a.only] if a.only else [int(b) for b in a.B.split(",")]
    Bmax = max(Bs)
    T, _ = wl.rows_by_index((1 << 40) + np.arange(Bmax))
    Td_all = device.colmajor(T, dev)

    def batched(B):
        idx, d, _ = device.rank_targets(Xd, model, A, Td_all[:, :B], K, ctx=ctx)
        return idx, d

    if a.only:
        batched(a.only)
        torch.cuda.synchronize()
        return
    # model records with the observed scores of each target (the loop's inputs), built once: host arithmetic, timing only
    mh = model.cpu().numpy()
    off_mean, off_sd = 4, 4 + M + P
    off_zobs = off_sd + M + P
    off_os, off_R = off_zobs + M, off_zobs + M + A
    R = mh[off_R:off_R + M * A].reshape(A, M).T
    mean, sd = mh[off_mean:off_mean + M], mh[off_sd:off_sd + M]
    models = np.repeat(mh[None, :], Bmax, axis=0)
    z = np.where(sd == 0, 0.0, (T - mean) / np.where(sd == 0, 1.0, sd))
    models[:, off_os:off_os + A] = z @ R
    models_d = torch.from_numpy(models).to(dev)
    dist = torch.empty(N, dtype=torch.float64, device=dev)
    idx1 = torch.empty(K, dtype=torch.int64, device=dev)
    d1 = torch.empty(K, dtype=torch.float64, device=dev)

    def loop(B):
        for b in range(B):
            ctx.check(L.abc_project_distance_dev(ctx.handle, Xd.data_ptr(), N, N, M, P, A, models_d[b].data_ptr(), 0, dist.data_ptr()))
            ctx.check(L.abc_select_smallest_dev(ctx.handle, dist.data_ptr(), N, K, 0, idx1.data_ptr(), d1.data_ptr()))

    def timeit(fn, B, reps):
        fn(B)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn(B)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    lines = ["# scripts/targets_time.py on %s: N = %d, M = %d, P = %d, A = %d, K = %d; wall ms per call (median of %d, after one warm-up)"
             % (torch.cuda.get_device_name(0), N, M, P, A, K, a.reps),
             "# batched: abc_rank_targets_dev (scores of all rows, thresholds, candidate pass, segmented select, exact fallbacks)",
             "# loop: per target abc_project_distance_dev + abc_select_smallest_dev on the same model, observed scores replaced",
             "%6s %12s %12s %10s %12s %10s" % ("B", "batched_ms", "loop_ms", "ratio", "ms/target", "fallbacks")]
    for B in Bs:
        ctx.targets_fallbacks(reset=True)
        tb = timeit(batched, B, a.reps)
        fb = ctx.targets_fallbacks()
        tl = timeit(loop, B, max(1, min(a.reps, 3)))
        lines.append("%6d %12.3f %12.3f %10.2f %12.4f %10d" % (B, tb, tl, tl / tb, tb / B, fb))
        print(lines[-1], flush=True)
    lines.append("# at B = %d the batched call is %.1fx faster than the per-target loop" % (Bs[-1], tl / tb))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
