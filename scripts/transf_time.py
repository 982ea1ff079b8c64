"""Times the log / logit parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf) at DESIGN 7c's shape:
N = 1e6 rows, M = 32 metrics, P = 16 parameters (brought into [0.1, 0.9], so that every one has a logarithm), A = 8 components,
K = 10000, B = 16 / 256 / 1024 targets.  Per B: the adjustment (coef only), the summaries and the densities under method 1, each
with every column LOG and with nothing set, the two alternating call by call in the same process (the setting changes between the
timed brackets, never inside one); a warm-up of 3 of each, then the median of --reps, each between two device events.  Beside them
the forward kernel alone (abc_param_transf_dev over the N x P matrix): its time and the fraction of the HBM peak (8 TB/s) that its
2 N P 8 bytes make.
--parent: the nothing-set legs alone, for a library built from the parent commit (ABCSMC_HIP_SO=<that library>): the entries this
feature adds are not bound then.  Its rows are appended to the table under "parent", and the ratio new / parent of every
nothing-set leg is printed beside the pool's box-to-box +-3 % (README).
Writes a text table (default profiles/transf_time.txt)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402

NEW_ENTRIES = ("abc_ctx_set_param_transf", "abc_param_transf_dev", "abc_param_transf", "abc_param_transf_outside")
HBM_PEAK = 8.0e12     # bytes / s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--B", type=int, nargs="+", default=[16, 256, 1024])
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", action="store_true", help="the nothing-set legs alone (a library without the transforms)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transf_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("transf_time.py: no GPU (nothing is measured without one)")
    if a.parent:
        for n in NEW_ENTRIES:
            _lib.SIGNATURES.pop(n, None)
    N, M, P, A, K = a.N, 32, 16, 8, a.K
    dev = "cuda:0"
    wl = synthetic.Workload(M, P, 2024)
    X, Y = wl.rows(0, N)
    Y = np.asarray(Y, dtype=np.float64)
    Y = 0.1 + 0.8 * (Y - Y.min(axis=0)) / (Y.max(axis=0) - Y.min(axis=0))
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
    Tall, _ = wl.rows_by_index((1 << 40) + np.arange(max(a.B)))
    log_all = ["log"] * P

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def setting(on):
        if not a.parent:
            ctx.set_param_transf(log_all if on else None)

    fmt = lambda v: "%9.3f  (%.3f .. %.3f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    tag = "parent" if a.parent else "new"
    lines = ["# scripts/transf_time.py%s on %s: N = %d, M = %d, P = %d, A = %d, K = %d; ms per call between two device events: median "
             "(min .. max) of %d after a warm-up of 3, the legs alternating" %
             (" --parent" if a.parent else "", torch.cuda.get_device_name(0), N, M, P, A, K, a.reps)]
    for B in a.B:
        Td = device.colmajor(np.ascontiguousarray(Tall[:B]), dev)
        calls = (("adjust (coef)", lambda: device.rank_targets_adjust(Xd, model, A, Td, K, Yd, theta=False, weight=False, dist=False,
                                                                       ctx=ctx)),
                 ("summary m1", lambda: device.rank_targets_summary(Xd, model, A, Td, K, Yd, method=1, ctx=ctx)),
                 ("density m1", lambda: device.rank_targets_density(Xd, model, A, Td, K, Yd, method=1, ctx=ctx)))
        for name, fn in calls:
            legs = (False,) if a.parent else (False, True)
            for on in legs:
                setting(on)
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {on: [] for on in legs}
            for _ in range(a.reps):
                for on in legs:
                    setting(on)
                    t[on].append(timed(fn))
            setting(False)
            lines.append("%-6s B = %-5d %-14s nothing set  %s" % (tag, B, name, fmt(t[False])))
            if not a.parent:
                lines.append("%-6s B = %-5d %-14s every LOG    %s   +%.3f ms" %
                             (tag, B, name, fmt(t[True]), np.median(t[True]) - np.median(t[False])))
            print("\n".join(lines[-2:] if not a.parent else lines[-1:]), flush=True)
    if not a.parent:
        setting(True)
        for _ in range(3):
            device.param_transf(Yd, ctx=ctx)
        tf = [timed(lambda: device.param_transf(Yd, ctx=ctx)) for _ in range(a.reps)]
        setting(False)
        ms = float(np.median(tf))
        lines.append("forward kernel alone (N x P, every LOG, with its output's allocation) %s   %.1f %% of the HBM peak" %
                     (fmt(tf), 100.0 * 2 * N * P * 8 / (ms * 1e-3) / HBM_PEAK))
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    mode = "a" if a.parent and os.path.exists(a.out) else "w"
    with open(a.out, mode) as f:
        f.write(txt)
    if a.parent and mode == "a":      # the ratio new / parent of every nothing-set leg
        rows = {}
        for ln in open(a.out):
            p = ln.split()
            if len(p) > 6 and p[0] in ("new", "parent") and "nothing" in ln:
                key = ln[7:ln.index("nothing")].strip()
                rows.setdefault(key, {})[p[0]] = float(ln[ln.index("nothing set") + 11:].split()[0])
        out = ["# nothing set, new / parent (the pool's box-to-box spread is +-3 %):"]
        for key, v in rows.items():
            if "new" in v and "parent" in v:
                out.append("#   %-28s %.3f" % (key, v["new"] / v["parent"]))
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n")
        print("\n".join(out))


if __name__ == "__main__":
    main()
