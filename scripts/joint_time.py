"""Times the joint posterior of the batched ranking (abc_rank_targets_joint_dev) at N = 1e6 rows, M = 32 metrics, P = 16
parameters (all 120 pairs), A = 8 components, K = 1000, G = 64, B = 1000 targets, for rejection and loclinear, with dens off (the
moments and the joint modes) and with dens on (B x 120 x 64 x 64 doubles, 3.9 GB), beside the marginal density call at the same G.
One timed call each after one warm-up; the first call that raises ends the script (an error of the library is an exception, so
nothing more is started on the card after it).  The pair kernel's own time (k_jt_pair) comes from a rocprofv3 --kernel-trace --stats run of
this script with --only METHOD, one process per method ("-" when rocprofv3 is not to be had); the fraction of the fp64 matrix peak
counts the algorithmic flops 2 G^2 K per (target, pair) against 78.6 TFLOP/s (256 CUs x 4 SIMDs x 32 flop per cycle at 2.4 GHz).
Writes a text table (default profiles/joint_kernel_stats.txt)."""
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

PEAK = 78.6e12


def kernel_ms(method, a):
    """every kernel of one dens-on call, name -> ms, from a kernel trace of a fresh process under a time limit of its own.
    Returns (times or None, exit status): None with status 0 when rocprofv3 is not to be had or left no statistics."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None, 0
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "600", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--only", str(method), "--N", str(a.N), "--K", str(a.K), "--G", str(a.G), "--B", str(a.B)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            return None, p.returncode
        out = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                for k in ("k_jt_pair", "k_jt_cov", "k_jt_mean", "k_jt_mode", "k_dn_moments"):
                    if k in row.get("Name", ""):
                        out[k] = out.get(k, 0.0) + float(row["TotalDurationNs"]) / float(row["Calls"]) * 1e-6
        return out or None, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_kernel_stats.txt"))
    a = ap.parse_args()
    N, M, P, A, K, G, B = a.N, 32, 16, 8, a.K, a.G, a.B
    npairs = P * (P - 1) // 2
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
    T, _ = wl.rows_by_index((1 << 40) + np.arange(B))
    Td = device.colmajor(T, dev)

    def joint(method, dens):
        device.rank_targets_joint(Xd, model, A, Td, K, Yd, G=G, method=method, dens=dens, ctx=ctx)

    def marginal(method):
        device.rank_targets_density(Xd, model, A, Td, K, Yd, G=G, method=method, dens=False, ctx=ctx)

    if a.only >= 0:
        joint(a.only, True)
        torch.cuda.synchronize()
        joint(a.only, True)
        torch.cuda.synchronize()
        return

    def once(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    flops = 2.0 * G * G * K * npairs * B
    lines = ["# scripts/joint_time.py on %s: N = %d, M = %d, P = %d (%d pairs), A = %d, K = %d, G = %d, B = %d; wall ms of one call after "
             "one warm-up" % (torch.cuda.get_device_name(0), N, M, P, npairs, A, K, G, B),
             "# marginal: abc_rank_targets_density_dev without dens at the same G; modes: abc_rank_targets_joint_dev writing mean, cov, "
             "corr, grid, bw, mode and mode_dens; dens: also dens (%.2f GB)" % (B * npairs * G * G * 8e-9),
             "# k_jt_pair etc.: the kernels' own time in the dens call (rocprofv3 --kernel-trace --stats, a run of its own); peak: "
             "2 G^2 K flop per (target, pair) = %.3g flop against 78.6 TFLOP/s of the fp64 matrix pipe" % flops,
             "%10s %12s %10s %10s %10s %8s %9s %9s %9s" % ("method", "marginal_ms", "modes_ms", "dens_ms", "k_jt_pair", "of_peak",
                                                         "k_jt_cov", "k_jt_mean", "k_jt_mode")]
    rows = []
    for method, name in ((0, "rejection"), (1, "loclinear")):
        rows.append((method, name, once(lambda: marginal(method)), once(lambda: joint(method, False)), once(lambda: joint(method, True))))
        print(rows[-1], flush=True)
    del Xd, Yd, Td
    torch.cuda.empty_cache()
    failed = 0                                                  # after a profile run that failed nothing more is started on the card
    for method, name, tm, t0, t1 in rows:
        km = None
        if not failed:
            km, failed = kernel_ms(method, a)
            if failed:
                lines.append("# the rocprofv3 run of %s ended with status %d: no further profile run was started" % (name, failed))
        if km and "k_jt_pair" in km:
            ks = "%10.3f %8.3f %9.3f %9.3f %9.3f" % (km["k_jt_pair"], flops / (km["k_jt_pair"] * 1e-3) / PEAK, km.get("k_jt_cov", 0.0),
                                                   km.get("k_jt_mean", 0.0), km.get("k_jt_mode", 0.0))
        else:
            ks = "%10s %8s %9s %9s %9s" % ("-", "-", "-", "-", "-")
        lines.append("%10s %12.3f %10.3f %10.3f %s" % (name, tm, t0, t1, ks))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
