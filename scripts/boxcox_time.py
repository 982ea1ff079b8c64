"""Times the Box-Cox pre-pass of the metrics (abc_optimize_box_cox_dev, abc_box_cox_dev) at configs[2]'s table: M = 32 metrics,
N = 1e6 and 1e5 rows, the reference's default grid (L = 100).  Per N: the search call and the transform call (in place), each
between two device events, a warm-up of 3, then the median of --reps; the search as exponentials per second and as a share of the
fp64 vector peak; and the same search evaluated in double-precision NumPy on this machine's host (one thread of it; at N = 1e6
on --host-cols columns, scaled to M).
The share of peak counts what the kernel issues per (row, column, grid value): 32 fp64 vector instructions, 14 of them fused
multiply-adds (the expm1, the three moments and this element's part of the cross-lane sums; counted in the disassembly of
k_bc_search's loop over the grid: 256 per 8 rows), so 46 floating-point operations against a peak of 78.6e12 per second.
Writes a text table (default profiles/boxcox.txt)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12      # floating-point operations / s (MI355X)
FLOP_PER_ELEMENT = 46           # (above)


def host_search(X, grid):
    """the header's definition in float64 NumPy, column by column (what a CPU implementation of the pre-pass would run)"""
    lam_out = np.empty(X.shape[1])
    for j in range(X.shape[1]):
        l = np.log(X[:, j])
        u = l - l.mean()
        best, pk = np.inf, 0
        for k, lam in enumerate(grid):
            d = np.expm1(lam * u) if lam != 0 else u
            c = d - d.mean()
            c2 = c * c
            m2 = c2.sum() / (c.size - 1)
            s = ((c2 * c).sum() / c.size) / (m2 * np.sqrt(m2))
            if np.isfinite(s) and abs(s) < abs(best):
                best, pk = s, k
        lam_out[j] = grid[pk]
    return lam_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1000000, 100000])
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-cols", type=int, default=2, help="columns of the host evaluation at N >= 1e6 (scaled to M)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxcox.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boxcox_time.py: no GPU (nothing is measured without one)")
    dev = "cuda:0"
    ctx = _lib.default_context(0)
    grid = _lib.box_cox_grid()
    L, M = grid.size, a.M
    fmt = lambda v: "%9.3f  (%.3f .. %.3f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = ["# scripts/boxcox_time.py on %s: M = %d, L = %d; ms per call between two device events: median (min .. max) of %d after a "
             "warm-up of 3" % (torch.cuda.get_device_name(0), M, L, a.reps)]
    for N in a.N:
        g = np.random.default_rng(N)
        X = np.exp(0.6 * g.standard_normal((N, M)) + g.uniform(0, 3, M))        # right-skewed positive metrics
        Xd = device.colmajor(X, dev)
        r = None
        for _ in range(3):
            r = device.optimize_box_cox(Xd, ctx=ctx)
        ts = [timed(lambda: device.optimize_box_cox(Xd, ctx=ctx)) for _ in range(a.reps)]
        lam = r["lam"].cpu().numpy()
        Yd = Xd.clone()
        for _ in range(3):
            device.box_cox(Yd, lam, out=Yd, ctx=ctx)
        Yd.copy_(Xd)
        ta = []
        for _ in range(a.reps):
            ta.append(timed(lambda: device.box_cox(Yd, lam, out=Yd, ctx=ctx)))
            Yd.copy_(Xd)
        ms = float(np.median(ts))
        exps = float(N) * M * L
        lines.append("N = %-8d search  %s   %.3g exponentials/s, %.1f %% of the fp64 vector peak (%d flop each)" %
                     (N, fmt(ts), exps / (ms * 1e-3), 100.0 * exps * FLOP_PER_ELEMENT / (ms * 1e-3) / FP64_VECTOR_PEAK, FLOP_PER_ELEMENT))
        lines.append("N = %-8d apply   %s   in place, %.1f %% of the HBM peak (8 TB/s) by its 2 N M 8 bytes" %
                     (N, fmt(ta), 100.0 * 2 * N * M * 8 / (float(np.median(ta)) * 1e-3) / 8.0e12))
        cols = M if N < 1000000 else min(M, a.host_cols)
        t0 = time.perf_counter()
        hl = host_search(X[:, :cols], grid)
        th = (time.perf_counter() - t0) * M / cols
        lines.append("N = %-8d host    %9.1f ms   float64 NumPy, one thread, %d of %d columns%s; picks equal the device's: %s" %
                     (N, th * 1e3, cols, M, " (scaled to M)" if cols < M else "", bool(np.array_equal(hl, lam[:cols]))))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
