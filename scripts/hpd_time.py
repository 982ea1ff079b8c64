"""Times the highest-density intervals of the batched ranking (abc_rank_targets_hpd_dev) beside the summary call they share their
sort with, and checks that the existing products did not move.
  shapes    M = 32 metrics, A = 8 components, P = 16 parameters: B = 1000 / K = 1000 at N = 1e5 under methods 0 and 1 (LDS path),
            and B = 100 / K = 1e5 at N = 2e5 under method 0 (global path).  Per shape the hpd call with nm = 2 masses (0.5, 0.95) on
            this library, and the summary call with nq = 4 levels on this library and on one built from the parent commit.  The
            ratio printed is hpd on this library over the summary on the parent's.
  existing  the summary call (B = 1000, default levels) and the draws call (B = 100, S = 1000, smoothed) at K = 1000, the legs of
            scripts/entropy_time.py, on both libraries.
A process of the parent's library is started with --parent and ABCSMC_HIP_SO=<that library> (the new entries are not bound there).
Every process appends its samples (ms per call between two device events, after a warm-up of 2) to --samples; --report reads them
all and writes the table (default profiles/hpd_time.txt): per leg the median (min .. max) over every sample; for legs run on both
libraries new / parent beside the process-to-process spread of the parent (the medians of its processes, (max - min) / median).

The sequence behind profiles/hpd_time.txt, on one card, from the repository's root (PARENT_SO: libabcsmc_hip.so built by
`make -C abcsmc_amd/csrc` in a checkout of the parent commit; S: a samples file that does not exist yet, it is scratch and is
not kept):
    for r in 1 2 3; do
        ABCSMC_HIP_SO=$PARENT_SO python scripts/hpd_time.py --parent --run p$r --samples $S
        python scripts/hpd_time.py --run n$r --samples $S
    done
    python scripts/hpd_time.py --report --samples $S --out profiles/hpd_time.txt
Three processes of five repetitions per library: 15 samples a leg."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ("abc_rank_targets_hpd_dev", "abc_particle_ranking_pls_targets_hpd", "abc_weighted_hpd_dev", "abc_weighted_hpd")
M, A, P = 32, 8, 16
SHAPES = ((100000, 1000, 1000, 0), (100000, 1000, 1000, 1), (200000, 100, 100000, 0))      # N, B, K, method
MASS = (0.5, 0.95)
PROBS4 = (0.025, 0.25, 0.75, 0.975)
SUMMARY4, HPD = "summary call, nq = 4", "hpd call, nm = 2"


def report(samples, out):
    rows, order = {}, []
    head = ""
    for ln in open(samples):
        if ln.startswith("#"):
            head = head or ln.rstrip("\n")
            continue
        tag, run, shape, leg, *t = ln.rstrip("\n").split("\t")
        if shape not in order:
            order.append(shape)
        rows.setdefault(shape, {}).setdefault(leg, {}).setdefault(tag, {}).setdefault(run, []).extend(float(x) for x in t)
    lines = [head, "# ms per call: median (min .. max) over every sample of every process; (a) parent, (b) this library,",
             "# spread(a): the medians of the parent's processes, (max - min) / median"]

    def stat(runs):
        allv = np.concatenate([np.asarray(v) for v in runs.values()])
        return float(np.median(allv)), float(allv.min()), float(allv.max()), [float(np.median(v)) for v in runs.values()], allv.size

    for shape in order:
        lines.append(shape)
        for leg, tags in rows[shape].items():
            a = stat(tags["parent"]) if "parent" in tags else None
            b = stat(tags["new"]) if "new" in tags else None
            if a:
                lines.append("    %-22s (a) %9.3f (%.3f .. %.3f, n = %d)" % (leg, a[0], a[1], a[2], a[4]))
            if b:
                extra = "  b/a %.3f  spread(a) %.3f" % (b[0] / a[0], (max(a[3]) - min(a[3])) / a[0]) if a else ""
                lines.append("    %-22s (b) %9.3f (%.3f .. %.3f, n = %d)%s" % (leg, b[0], b[1], b[2], b[4], extra))
        legs = rows[shape]
        if HPD in legs and "parent" in legs.get(SUMMARY4, {}):
            h, s = stat(legs[HPD]["new"]), stat(legs[SUMMARY4]["parent"])
            lines.append("    hpd (b) / summary (a): %.3f" % (h[0] / s[0]))
    txt = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(txt)
    print(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="0", help="a label for this process's samples")
    ap.add_argument("--parent", action="store_true", help="the existing calls alone (a library without the new entries)")
    ap.add_argument("--samples", default=os.path.join(ROOT, "profiles", "hpd_time.samples.tsv"))
    ap.add_argument("--report", action="store_true", help="no measurement: the table from --samples")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpd_time.txt"))
    a = ap.parse_args()
    if a.report:
        return report(a.samples, a.out)
    import torch
    from abcsmc_amd import _lib, device, synthetic
    if not torch.cuda.is_available():
        sys.exit("hpd_time.py: no GPU (nothing is measured without one)")
    if a.parent:
        for n in NEW_ENTRIES:
            _lib.SIGNATURES.pop(n, None)
    dev = "cuda:0"
    L = _lib.lib()
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    tag = "parent" if a.parent else "new"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def fit(N):
        wl = synthetic.Workload(M, P, 2024)
        X, Y = wl.rows(0, N)
        Xd, Yd = device.colmajor(X, dev), device.colmajor(Y, dev)
        stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=dev)
        model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=dev)
        zero = torch.zeros(M, dtype=torch.float64, device=dev)
        ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
        ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, N // 2, stats.data_ptr()))
        ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), zero.data_ptr(), M, P, A, 0, model.data_ptr()))
        model[0] = float(A)
        torch.cuda.synchronize()
        Tall, _ = wl.rows_by_index((1 << 40) + np.arange(1000))
        return Xd, Yd, model, device.colmajor(np.ascontiguousarray(Tall), dev)

    def measure(f, shape, leg, fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t = [timed(fn) for _ in range(a.reps)]
        f.write("\t".join([tag, a.run, shape, leg] + ["%.4f" % v for v in t]) + "\n")
        f.flush()
        print(tag, a.run, shape, leg, "%.3f" % float(np.median(t)), flush=True)

    new_file = not os.path.exists(a.samples)
    with open(a.samples, "a") as f:
        if new_file:
            f.write("# scripts/hpd_time.py on %s\n" % torch.cuda.get_device_name(0))
        fitted = {}
        for N, B, K, method in SHAPES:
            if N not in fitted:
                fitted.clear()                                   # (one set on the card at a time)
                fitted[N] = fit(N)
            Xd, Yd, model, Td = fitted[N]
            Tb = Td[:, :B]
            if (B, K, method) == (1000, 1000, 0):
                shape = "existing, N = %d, M = %d, P = %d, A = nc = %d, K = 1000" % (N, M, P, A)
                measure(f, "summary (B = 1000): " + shape, "existing", lambda: device.rank_targets_summary(Xd, model, A, Tb, 1000, Yd, ctx=ctx))
                measure(f, "draws (B = 100): " + shape, "existing",
                        lambda: device.rank_targets_draws(Xd, model, A, Td[:, :100], 1000, Yd, 1000, smooth=True, seed=1, ctx=ctx))
            shape = "N = %d, M = %d, P = %d, A = nc = %d, B = %d, K = %d, method %d (%s path)" % (N, M, P, A, B, K, method,
                                                                                                "LDS" if K <= 8192 else "global")
            measure(f, shape, SUMMARY4, lambda: device.rank_targets_summary(Xd, model, A, Tb, K, Yd, probs=PROBS4, method=method, ctx=ctx))
            if not a.parent:
                measure(f, shape, HPD, lambda: device.rank_targets_hpd(Xd, model, A, Tb, K, Yd, mass=MASS, method=method, ctx=ctx))


if __name__ == "__main__":
    main()
