"""Times the row importance weights of the batched ranking (abc_ctx_set_row_weights) on the adjust call
(abc_rank_targets_adjust_dev, coef / rank / status only: the fit, without the adjusted rows): N = 1e5 rows, M = 32 metrics,
P = 16 parameters, A = 8 components, B = 1000 targets at K = 100 and K = 1000, and one wide shape (M = 56, A = 52, P = 80,
B = 100, K = 300); and on one call of every product under method 0 at the second shape with B = 100 targets (summary: three
quantiles; density: G = 512; joint: G = 64, two pairs; draws: S = 1000, smoothed), whose kernels read the weights through
sm_weight.
Per shape and call
  (a) on a library built from the parent commit (--parent with ABCSMC_HIP_SO=<that library>: the new entries are not bound),
  (b) on this library with the setting off,
  (c) with the setting on (weights uniform on (0.1, 2)),
(b) and (c) alternating call by call in one process (the setting changes between the timed brackets, never inside one), (a) in
processes of its own that the caller alternates with the others.  Every process appends its samples (ms per call between two
device events, after a warm-up of 2) to --samples; --report reads them all and writes the table (default
profiles/rowweights_time.txt): per leg the median (min .. max) over every sample, b / a beside the run-to-run spread of (a) (the
medians of its processes), and what (c) adds to (b).

The sequence behind profiles/rowweights_time.txt, on one card, from the repository's root (PARENT_SO: libabcsmc_hip.so built by
`make -C abcsmc_amd/csrc` in a checkout of the parent commit; S: a samples file that does not exist yet, it is scratch and is
not kept):
    for r in 1 2 3; do
        ABCSMC_HIP_SO=$PARENT_SO python scripts/rowweights_time.py --parent --run p$r --samples $S
        python scripts/rowweights_time.py --run n$r --samples $S
    done
    python scripts/rowweights_time.py --report --samples $S --out profiles/rowweights_time.txt
Three processes of five repetitions per library: 15 samples a leg."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ("abc_ctx_set_row_weights", "abc_ctx_set_row_weights_dev", "abc_row_weights_info")
SHAPES = ((100000, 32, 16, 8, 1000, 100), (100000, 32, 16, 8, 1000, 1000), (100000, 56, 80, 52, 100, 300))     # N, M, P, A, B, K
LEGS = ("off", "on")
SUMMARY_SHAPE = 1                                               # the shape that also times the summary call


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
        rows.setdefault(shape, {}).setdefault((tag, leg), {}).setdefault(run, []).extend(float(x) for x in t)
    lines = [head, "# ms per call (adjust: coef, rank, status; the products: method 0): median (min .. max) over every",
             "# sample of every process; (a) parent, (b) setting off, (c) setting on; spread(a): the medians of the parent's",
             "# processes, (max - min) / median"]
    for shape in order:
        med = {}
        for k, runs in rows[shape].items():
            allv = np.concatenate([np.asarray(v) for v in runs.values()])
            med[k] = (float(np.median(allv)), float(allv.min()), float(allv.max()), [float(np.median(v)) for v in runs.values()], allv.size)
        a, b = med.get(("parent", "off")), med.get(("new", "off"))
        lines.append(shape)
        for name, m in (("a", a), ("b", b), ("c", med.get(("new", "on")))):
            if not m:
                continue
            txt = "    (%s) %9.3f (%.3f .. %.3f, n = %d)" % (name, m[0], m[1], m[2], m[4])
            if name == "b" and a:
                txt += "  b/a %.3f  spread(a) %.3f" % (b[0] / a[0], (max(a[3]) - min(a[3])) / a[0])
            if name == "c" and b:
                txt += "  %+.3f ms over (b) (x%.2f)" % (m[0] - b[0], m[0] / b[0])
            lines.append(txt)
    txt = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(txt)
    print(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="0", help="a label for this process's samples")
    ap.add_argument("--parent", action="store_true", help="the setting-off leg alone (a library without the setting)")
    ap.add_argument("--samples", default=os.path.join(ROOT, "profiles", "rowweights_time.samples.tsv"))
    ap.add_argument("--report", action="store_true", help="no measurement: the table from --samples")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowweights_time.txt"))
    a = ap.parse_args()
    if a.report:
        return report(a.samples, a.out)
    import torch
    from abcsmc_amd import _lib, device, synthetic
    if not torch.cuda.is_available():
        sys.exit("rowweights_time.py: no GPU (nothing is measured without one)")
    if a.parent:
        for n in NEW_ENTRIES:
            _lib.SIGNATURES.pop(n, None)
    dev = "cuda:0"
    L = _lib.lib()
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def setting(w):
        if not a.parent:
            ctx.set_row_weights(w)

    tag = "parent" if a.parent else "new"
    legs = LEGS[:1] if a.parent else LEGS
    new_file = not os.path.exists(a.samples)
    with open(a.samples, "a") as f:
        if new_file:
            f.write("# scripts/rowweights_time.py on %s\n" % torch.cuda.get_device_name(0))
        for si, (N, M, P, A, B, K) in enumerate(SHAPES):
            wl = synthetic.Workload(M, P, 2024)
            X, Y = wl.rows(0, N)
            Xd, Yd = device.colmajor(X, dev), device.colmajor(Y, dev)
            stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=dev)
            model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=dev)
            zero = torch.zeros(M, dtype=torch.float64, device=dev)
            ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
            ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, N // 2, stats.data_ptr()))
            ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), zero.data_ptr(), M, P, A, 0, model.data_ptr()))
            model[0] = float(A)                                  # every component: the shape's nc is A
            torch.cuda.synchronize()
            Tall, _ = wl.rows_by_index((1 << 40) + np.arange(B))
            Td = device.colmajor(np.ascontiguousarray(Tall), dev)
            shape = "N = %d, M = %d, P = %d, A = nc = %d, B = %d, K = %d" % (N, M, P, A, B, K)

            om = torch.tensor(np.random.default_rng(7).uniform(0.1, 2.0, N), device=dev)
            calls = [("adjust", lambda: device.rank_targets_adjust(Xd, model, A, Td, K, Yd, theta=False, weight=False, ctx=ctx))]
            if si == SUMMARY_SHAPE:
                Tp = Td[:, :100]                                 # the products at B = 100 (ldt stays B)
                calls.append(("summary", lambda: device.rank_targets_summary(Xd, model, A, Td, K, Yd, ctx=ctx)))
                calls.append(("density (B = 100)", lambda: device.rank_targets_density(Xd, model, A, Tp, K, Yd, ctx=ctx)))
                calls.append(("joint (B = 100)", lambda: device.rank_targets_joint(Xd, model, A, Tp, K, Yd, pairs=[(0, 1), (2, 3)], ctx=ctx)))
                calls.append(("draws (B = 100)", lambda: device.rank_targets_draws(Xd, model, A, Tp, K, Yd, 1000, smooth=True,
                                                                                 seed=1, ctx=ctx)))
            for call, fn in calls:
                for name in legs:
                    setting(om if name == "on" else None)
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                t = {name: [] for name in legs}
                for _ in range(a.reps):
                    for name in legs:
                        setting(om if name == "on" else None)
                        t[name].append(timed(fn))
                setting(None)
                for name in legs:
                    f.write("\t".join([tag, a.run, call + ": " + shape, name] + ["%.4f" % v for v in t[name]]) + "\n")
                    f.flush()
                    print(tag, a.run, call, shape, name, "%.3f" % float(np.median(t[name])), flush=True)


if __name__ == "__main__":
    main()
