"""Times the posterior draws of the batched ranking (abc_rank_targets_draws_dev) at N = 1e6 rows, M = 32 metrics, P = 16 parameters,
A = 8 components, K = 1000, B = 1000 targets, S = 1000 draws per target, loclinear, with smooth 0 and 1, beside the density call at
the same B, K and P without dens (the ranking, the adjustment, the quantiles and the bandwidths, which a smoothed draws call
shares) and the adjustment call on its own (what a plain draws call shares).  Calls: a warm-up of 3, then the median of --reps
calls, each between two device events.  Kernels: a rocprofv3 --kernel-trace --stats run of this script with --only, in a process
of its own under its own time limit ("-" when rocprofv3 is not to be had): k_dr_draw<false> / <true>, k_dr_cdf, and k_perturb<16>
of abc_perturb_dev at the generation's shape (1e6 multivariate proposals from 1e5 rows of 16 parameters: 264 MB read and written),
the project's kernel of the same kind, from the same build on the same card.  The fraction of HBM counts the bytes an algorithm
must move (draws: the B S P 8 = 128 MB it writes) against 8 TB/s.  Writes a text table (default profiles/draws_kernel_stats.txt)."""
import argparse
import csv
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402

HBM = 8e12
KERNELS = ("k_dr_draw<false>", "k_dr_draw<true>", "k_dr_cdf", "k_perturb<16")


def kernel_us(a):
    """name -> us per launch from a kernel trace of a fresh process.  Returns (times or None, exit status): None with status 0
    when rocprofv3 is not to be had or left no statistics."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None, 0
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "600", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--only", "--N", str(a.N), "--K", str(a.K), "--B", str(a.B), "--S", str(a.S)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            return None, p.returncode
        out = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                for k in KERNELS:
                    if k in row.get("Name", ""):
                        out[k] = float(row["TotalDurationNs"]) / float(row["Calls"]) * 1e-3
        return out or None, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--S", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="store_true", help="the calls alone, for the kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draws_kernel_stats.txt"))
    a = ap.parse_args()
    N, M, P, A, K, B, S = a.N, 32, 16, 8, a.K, a.B, a.S
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

    def draws(smooth):
        device.rank_targets_draws(Xd, model, A, Td, K, Yd, S, smooth=smooth, seed=11, method=1, ctx=ctx)

    def density():
        device.rank_targets_density(Xd, model, A, Td, K, Yd, G=64, method=1, dens=False, ctx=ctx)

    def adjust():
        device.rank_targets_adjust(Xd, model, A, Td, K, Yd, theta=False, weight=False, dist=False, ctx=ctx)

    if a.only:
        # the generation's proposals: 1e6 rows from 1e5 parents, wide priors (nothing is rejected), a diagonal factor
        rng = np.random.default_rng(3)
        Kp, n = 100000, 1000000
        th = device.colmajor(rng.normal(size=(Kp, P)), dev)
        pr = device.priors_to_device(_lib.make_priors([(_lib.PRIOR_UNIF_REAL, -1e300, 1e300)] * P), dev)
        par = torch.from_numpy(rng.integers(0, Kp, size=n)).to(dev)
        lv = device.colmajor(np.eye(P) * 0.1, dev)
        out = torch.empty((P, n), dtype=torch.float64, device=dev)
        r = _lib.Rng(1, 2, 3)
        for _ in range(5):
            draws(False)
            draws(True)
            ctx.check(L.abc_perturb_dev(ctx.handle, C.byref(r), th.data_ptr(), Kp, P, pr.data_ptr(), par.data_ptr(), 0, n, 1,
                                        lv.data_ptr(), out.data_ptr(), None, 0))
        torch.cuda.synchronize()
        return

    def median_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    calls = [("adjust", adjust), ("density (no dens)", density), ("draws smooth=0", lambda: draws(False)),
             ("draws smooth=1", lambda: draws(True))]
    rows = []
    for name, fn in calls:
        rows.append((name,) + median_ms(fn))
        print(rows[-1], flush=True)
    del Xd, Yd, Td
    torch.cuda.empty_cache()
    km, failed = kernel_us(a)
    nbytes = B * S * P * 8
    lines = ["# scripts/draws_time.py on %s: N = %d, M = %d, P = %d, A = %d, K = %d, B = %d, S = %d, loclinear; ms per call between two "
             "device events: median (min .. max) of %d after a warm-up of 3" % (torch.cuda.get_device_name(0), N, M, P, A, K, B, S, a.reps)]
    lines += ["%-20s %9.3f  (%.3f .. %.3f)" % r for r in rows]
    lines.append("# kernels, us per launch (rocprofv3 --kernel-trace --stats, a run of its own) and the fraction of 8 TB/s by algorithmic "
                 "bytes: k_dr_draw writes B S P 8 = %.0f MB; k_perturb<16> moves 264 MB (1e6 proposals from 1e5 rows)" % (nbytes * 1e-6))
    if failed:
        lines.append("# the rocprofv3 run ended with status %d" % failed)
    for k in KERNELS:
        if km and k in km:
            b = 264e6 if k.startswith("k_perturb") else nbytes if k.startswith("k_dr_draw") else None
            lines.append("%-20s %9.2f  %s" % (k + (">" if k.endswith("16") else ""), km[k],
                                             "%.3f of HBM" % (b / (km[k] * 1e-6) / HBM) if b else ""))
        else:
            lines.append("%-20s %9s" % (k, "-"))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
