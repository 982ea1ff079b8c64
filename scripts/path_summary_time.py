"""Times the summaries along a tolerance path (abc_rank_targets_path_summary_dev) beside the calls they replace, at DESIGN 7c's shape:
N = 1e6 rows, M = 32 metrics, P = 16 parameters, A = 8 components, Ks = (1000, 2500, 5000, 10000), B = 16 / 256 / 1024 targets,
levels (0.025, 0.5, 0.975) and the CDF at a truth.  Per B and method (rejection, loclinear): the one path call writing quant and cdf
only, and the T rank_targets_summary calls (one per tolerance) in a row, the two alternating call by call in the same process; a
warm-up of 3 of each, then the median of --reps, each between two device events.  The spread of each is its (max - min) over the
repetitions.  Kernels (--trace): a rocprofv3 --kernel-trace --stats run of this script with --only, in a process of its own under
its own time limit ("-" when rocprofv3 is not to be had): the rejection path call and the K = K_max summary call at the largest B,
so that the one-sort evaluation stands beside k_sm_chunk.  Writes two text tables (default profiles/path_summary_time.txt and
profiles/path_summary_kernel_stats.txt)."""
import argparse
import csv
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

KERNELS = ("k_smp_eval_global", "k_smp_lds", "k_sm_chunk", "k_sm_merge", "k_sm_eval_global", "k_sm_lds")


def kernel_us(a):
    """name -> (us per launch, launches) from a kernel trace of a fresh process.  Returns (times or None, exit status): None with
    status 0 when rocprofv3 is not to be had or left no statistics."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None, 0
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "600", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--only", "--N", str(a.N), "--B", str(max(a.B)), "--Ks"] + [str(k) for k in a.Ks]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            return None, p.returncode
        out = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                name = row.get("Name", "")
                for k in KERNELS:
                    if k in name:
                        calls = float(row["Calls"])
                        us, n = out.get(k, (0.0, 0.0))
                        out[k] = (us + float(row["TotalDurationNs"]) * 1e-3, n + calls)
                        break
        return ({k: (us / n, int(n)) for k, (us, n) in out.items()} or None), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--B", type=int, nargs="+", default=[16, 256, 1024])
    ap.add_argument("--Ks", type=int, nargs="+", default=[1000, 2500, 5000, 10000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="store_true", help="the calls alone, for the kernel trace")
    ap.add_argument("--trace", action="store_true", help="the kernel trace instead of the timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_summary_time.txt"))
    ap.add_argument("--kernel-out", default=os.path.join(ROOT, "profiles", "path_summary_kernel_stats.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("path_summary_time.py: no GPU (nothing is measured without one)")
    N, M, P, A, Ks = a.N, 32, 16, 8, tuple(a.Ks)
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
    Tall, truth_all = wl.rows_by_index((1 << 40) + np.arange(max(a.B)))
    probs = (0.025, 0.5, 0.975)

    def calls(B, method):
        Td = device.colmajor(np.ascontiguousarray(Tall[:B]), dev)
        tr = torch.from_numpy(np.ascontiguousarray(truth_all[:B])).to(dev)

        def path():
            device.rank_targets_path_summary(Xd, model, A, Td, Ks, Yd, probs=probs, truth=tr, method=method, post_mean=False,
                                             coef=False, fit=False, idx=False, dist=False, ctx=ctx)

        def summary(K):
            device.rank_targets_summary(Xd, model, A, Td, K, Yd, probs=probs, truth=tr, method=method, ctx=ctx)

        def each():
            for K in Ks:
                summary(K)

        return path, each, summary

    if a.only:
        path, _, summary = calls(max(a.B), 0)
        for _ in range(5):
            path()
            summary(Ks[-1])
        torch.cuda.synchronize()
        return

    if a.trace:
        del Xd, Yd
        torch.cuda.empty_cache()
        km, failed = kernel_us(a)
        lines = ["# scripts/path_summary_time.py --only under rocprofv3 --kernel-trace --stats (a run of its own) on %s: the rejection "
                 "path call at Ks = %s and rank_targets_summary at K = %d, B = %d; us per launch (launches)" %
                 (torch.cuda.get_device_name(0), Ks, Ks[-1], max(a.B))]
        if failed:
            lines.append("# the rocprofv3 run ended with status %d" % failed)
        for k in KERNELS:
            lines.append("%-20s %10.2f  (%d)" % ((k,) + km[k]) if km and k in km else "%-20s %10s" % (k, "-"))
        ktxt = "\n".join(lines) + "\n"
        print(ktxt)
        with open(a.kernel_out, "w") as f:
            f.write(ktxt)
        sys.exit(1 if failed else 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fmt = lambda v: "%9.3f  (%.3f .. %.3f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    lines = ["# scripts/path_summary_time.py on %s: N = %d, M = %d, P = %d, A = %d, Ks = %s, levels %s and the CDF; ms per call between "
             "two device events: median (min .. max) of %d after a warm-up of 3, the two alternating" %
             (torch.cuda.get_device_name(0), N, M, P, A, Ks, probs, a.reps)]
    slower = []
    for method, name in ((0, "rejection"), (1, "loclinear")):
        for B in a.B:
            path, each, _ = calls(B, method)
            for _ in range(3):
                path()
                each()
            torch.cuda.synchronize()
            tp, tf = [], []
            for _ in range(a.reps):
                tp.append(timed(path))
                tf.append(timed(each))
            spread = max(np.max(tp) - np.min(tp), np.max(tf) - np.min(tf))
            lines.append("%s B = %-5d path summary (quant, cdf)  %s" % (name, B, fmt(tp)))
            lines.append("%s B = %-5d %d x summary (quant, cdf)     %s   ratio of medians %.2f, spread %.3f ms" %
                         (name, B, len(Ks), fmt(tf), np.median(tf) / np.median(tp), spread))
            print("\n".join(lines[-2:]), flush=True)
            if np.median(tp) > np.median(tf) + spread:
                slower.append((name, B))
    lines.append("# path summary slower than the calls it replaces beyond the spread at %s" % (slower if slower else "none"))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
