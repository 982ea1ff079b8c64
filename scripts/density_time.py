"""Times the weighted posterior densities of the batched ranking (abc_rank_targets_density_dev) against the summary call
(abc_rank_targets_summary_dev, three quantiles) on the same fitted model, at N = 1e6 rows, M = 32 metrics, P = 16 parameters,
A = 8 components, K = 1000, G = 512 grid points, B in {1, 16, 256, 1024}, method loclinear.  Columns: the summary call, the
density call writing the mode only, the density call writing dens too, the density kernel's own time (k_dn_dens, from a
rocprofv3 --kernel-trace --stats run of this script with --only B, one process per B; "-" when rocprofv3 is not to be had) and
the kernel evaluations per second that time amounts to (B P K G pairs).  Writes a text table (default profiles/density_time.txt).
--only B: one density call (dens written) at that B, nothing written (for the rocprofv3 run)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402


def kernel_ms(B, a):
    """k_dn_dens's total time in one call at B targets, from a kernel trace of a fresh process; None if it cannot be had"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--only", str(B), "--N", str(a.N), "--K", str(a.K), "--G", str(a.G)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return None
        total = 0.0
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                if "k_dn_dens" in row.get("Name", ""):
                    total += float(row["TotalDurationNs"]) / float(row["Calls"])       # (the warm-up call and the timed one)
        return total * 1e-6 if total else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--G", type=int, default=512)
    ap.add_argument("--B", type=str, default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_time.txt"))
    a = ap.parse_args()
    N, M, P, A, K, G = a.N, 32, 16, 8, a.K, a.G
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

    def summary(B):
        device.rank_targets_summary(Xd, model, A, Td_all[:, :B], K, Yd, method=_lib.POSTERIOR_LOCLINEAR, ctx=ctx)

    def density(B, dens):
        device.rank_targets_density(Xd, model, A, Td_all[:, :B], K, Yd, G=G, method=_lib.POSTERIOR_LOCLINEAR, dens=dens, ctx=ctx)

    if a.only:
        density(a.only, True)
        torch.cuda.synchronize()
        density(a.only, True)
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

    lines = ["# scripts/density_time.py on %s: N = %d, M = %d, P = %d, A = %d (nc = %d), K = %d, G = %d, loclinear; wall ms per call "
             "(median of %d, after one warm-up)" % (torch.cuda.get_device_name(0), N, M, P, A, nc, K, G, a.reps),
             "# summary: abc_rank_targets_summary_dev (3 quantiles); mode: abc_rank_targets_density_dev writing grid, bw, mode and "
             "mode_dens; dens: also dens (B P G doubles)",
             "# kernel_ms: k_dn_dens alone in the dens call (rocprofv3 --kernel-trace --stats, a run of its own); Geval/s: "
             "B P K G / kernel time",
             "%6s %11s %10s %10s %10s %10s %10s" % ("B", "summary_ms", "mode_ms", "dens_ms", "+dens_ms", "kernel_ms", "Geval/s")]
    for B in Bs:
        ts = timeit(lambda: summary(B), a.reps)
        tm = timeit(lambda: density(B, False), a.reps)
        td = timeit(lambda: density(B, True), a.reps)
        lines.append([B, ts, tm, td])
        print(B, ts, tm, td, flush=True)
    del Xd, Yd, Td_all
    torch.cuda.empty_cache()
    for i, (B, ts, tm, td) in enumerate(lines[4:]):
        km = kernel_ms(B, a)
        ks = ("%10.3f %10.1f" % (km, B * P * K * G / (km * 1e-3) * 1e-9)) if km else ("%10s %10s" % ("-", "-"))
        lines[4 + i] = "%6d %11.3f %10.3f %10.3f %10.3f %s" % (B, ts, tm, td, td - ts, ks)
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
