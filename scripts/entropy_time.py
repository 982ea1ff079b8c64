"""Times the posterior entropy of the batched ranking (abc_rank_targets_entropy_dev, abc_weighted_entropy_dev) and checks that the
existing products did not move.
  entropy   the new call at N = 1e5 rows, M = 32 metrics, A = 8 components: B = 1000 / K = 1000 / P = 16 and B = 100 / K = 1000 /
            P = 4 with A = 4 (method 0; the plain ranking of the same shape beside it, so that the product's share can be read), and the generic
            call at K = 1e5 / P = 16.  k = 4.  Per shape the K^2 P multiply-adds of the neighbour kernel over the time, as a fraction
            of the fp64 vector peak (78.6 TFLOP/s = 39.3e12 multiply-adds per second, the public figure for the MI355X), and the
            same estimate by scipy.spatial.cKDTree on that host (query of k + 1 neighbours, 16 workers; targets one after another,
            timed on CKD_TARGETS of them and scaled; the generic shape: 2000 of the queries timed and scaled).
  existing  the draws and summary calls at the product shape of scripts/rowweights_time.py (N = 1e5, M = 32, P = 16, A = 8,
            K = 1000; summary B = 1000, draws B = 100, S = 1000, smoothed), on this library and on one built from the parent commit
            (--parent with ABCSMC_HIP_SO=<that library>: the new entries are not bound), in processes that the caller alternates.
Every process appends its samples (ms per call between two device events, after a warm-up of 2) to --samples; --report reads them
all and writes the table (default profiles/entropy_time.txt): per leg the median (min .. max) over every sample; for the existing
calls new / parent beside the process-to-process spread of the parent (the medians of its processes, (max - min) / median), the
gate of profiles/rowweights_time.txt.

The sequence behind profiles/entropy_time.txt, on one card, from the repository's root (PARENT_SO: libabcsmc_hip.so built by
`make -C abcsmc_amd/csrc` in a checkout of the parent commit; S: a samples file that does not exist yet, it is scratch and is
not kept):
    for r in 1 2 3; do
        ABCSMC_HIP_SO=$PARENT_SO python scripts/entropy_time.py --parent --run p$r --samples $S
        python scripts/entropy_time.py --run n$r --samples $S
    done
    python scripts/entropy_time.py --report --samples $S --out profiles/entropy_time.txt
Three processes of five repetitions per library: 15 samples a leg."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ("abc_rank_targets_entropy_dev", "abc_particle_ranking_pls_targets_entropy", "abc_weighted_entropy_dev",
               "abc_weighted_entropy")
N, M, A0, KNN = 100000, 32, 8, 4
TARGET_SHAPES = ((1000, 1000, 16), (100, 1000, 4))             # B, K, P
GENERIC = (100000, 16)                                          # K, P
PEAK_FMA = 39.3e12                                              # fp64 vector multiply-adds per second
CKD_TARGETS = 20


def report(samples, out):
    rows, order, notes = {}, [], {}
    head = ""
    for ln in open(samples):
        if ln.startswith("#"):
            head = head or ln.rstrip("\n")
            continue
        tag, run, shape, leg, *t = ln.rstrip("\n").split("\t")
        if tag == "note":
            notes.setdefault((shape, leg), t)                   # (the same in every process: the first one's)
            continue
        if shape not in order:
            order.append(shape)
        rows.setdefault(shape, {}).setdefault((tag, leg), {}).setdefault(run, []).extend(float(x) for x in t)
    lines = [head, "# ms per call: median (min .. max) over every sample of every process; existing calls: (a) parent, (b) this",
             "# library, spread(a): the medians of the parent's processes, (max - min) / median"]
    for shape in order:
        lines.append(shape)
        med = {}
        for k, runs in rows[shape].items():
            allv = np.concatenate([np.asarray(v) for v in runs.values()])
            med[k] = (float(np.median(allv)), float(allv.min()), float(allv.max()), [float(np.median(v)) for v in runs.values()], allv.size)
        a, b = med.get(("parent", "existing")), med.get(("new", "existing"))
        if a and b:
            lines.append("    (a) %9.3f (%.3f .. %.3f, n = %d)" % (a[0], a[1], a[2], a[4]))
            lines.append("    (b) %9.3f (%.3f .. %.3f, n = %d)  b/a %.3f  spread(a) %.3f" % (b[0], b[1], b[2], b[4], b[0] / a[0],
                                                                                           (max(a[3]) - min(a[3])) / a[0]))
        for (tag, leg), m in med.items():
            if leg != "existing":
                lines.append("    %-22s %9.3f (%.3f .. %.3f, n = %d)" % (leg, m[0], m[1], m[2], m[4]))
        e, r = med.get(("new", "entropy call")), med.get(("new", "plain ranking"))
        for (s, leg), t in notes.items():
            if s != shape:
                continue
            if leg == "fma":
                ms = e[0] - (r[0] if r else 0.0)
                lines.append("    %s: %.3e multiply-adds in %.3f ms = %.2f%% of the fp64 vector peak"
                             % ("entropy call - plain ranking" if r else "entropy call", float(t[0]), ms,
                                100.0 * float(t[0]) / (ms * 1e-3) / PEAK_FMA))
            else:
                lines.append("    cKDTree on the host: %.1f ms (%s)" % (float(t[0]), t[1]))
    txt = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(txt)
    print(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="0", help="a label for this process's samples")
    ap.add_argument("--parent", action="store_true", help="the existing calls alone (a library without the new entries)")
    ap.add_argument("--samples", default=os.path.join(ROOT, "profiles", "entropy_time.samples.tsv"))
    ap.add_argument("--report", action="store_true", help="no measurement: the table from --samples")
    ap.add_argument("--no-ckdtree", action="store_true", help="skip the host comparison (it is the same in every process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entropy_time.txt"))
    a = ap.parse_args()
    if a.report:
        return report(a.samples, a.out)
    import torch
    from abcsmc_amd import _lib, device, synthetic
    if not torch.cuda.is_available():
        sys.exit("entropy_time.py: no GPU (nothing is measured without one)")
    if a.parent:
        for n in NEW_ENTRIES:
            _lib.SIGNATURES.pop(n, None)
    dev = "cuda:0"
    L = _lib.lib()
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    tag = "parent" if a.parent else "new"
    A = A0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def fit(P, A):
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
        return Y, Xd, Yd, model, device.colmajor(np.ascontiguousarray(Tall), dev)

    def measure(f, shape, leg, fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t = [timed(fn) for _ in range(a.reps)]
        f.write("\t".join([tag, a.run, shape, leg] + ["%.4f" % v for v in t]) + "\n")
        f.flush()
        print(tag, a.run, shape, leg, "%.3f" % float(np.median(t)), flush=True)

    def ckdtree(f, shape, sets, scale_to, what, queries=None):
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        for V in sets:
            tree = cKDTree(V)
            t1 = time.perf_counter()
            tree.query(V[:queries], k=KNN + 1, workers=16)
            if queries:                                          # (the build once, the queries scaled to all rows)
                t0 -= (time.perf_counter() - t1) * (len(V) / queries - 1.0)
        ms = (time.perf_counter() - t0) * 1e3 * scale_to / len(sets)
        f.write("\t".join(["note", a.run, shape, "ckdtree", "%.3f" % ms, what]) + "\n")
        f.flush()

    new_file = not os.path.exists(a.samples)
    with open(a.samples, "a") as f:
        if new_file:
            f.write("# scripts/entropy_time.py on %s\n" % torch.cuda.get_device_name(0))
        # the existing calls, both libraries
        Y, Xd, Yd, model, Td = fit(16, A)
        shape = "existing, N = %d, M = %d, P = 16, A = nc = %d, K = 1000" % (N, M, A)
        Tp = Td[:, :100]
        measure(f, "summary (B = 1000): " + shape, "existing", lambda: device.rank_targets_summary(Xd, model, A, Td, 1000, Yd, ctx=ctx))
        measure(f, "draws (B = 100): " + shape, "existing",
                lambda: device.rank_targets_draws(Xd, model, A, Tp, 1000, Yd, 1000, smooth=True, seed=1, ctx=ctx))
        if a.parent:
            return
        # the new call
        for B, K, P in TARGET_SHAPES:
            A = min(A0, P)                                       # (no more components than parameters)
            if P != 16:
                Y, Xd, Yd, model, Td = fit(P, A)
            Tb = Td[:, :B]
            shape = "entropy: N = %d, M = %d, P = %d, A = nc = %d, B = %d, K = %d, k = %d" % (N, M, P, A, B, K, KNN)
            measure(f, shape, "plain ranking", lambda: device.rank_targets(Xd, model, A, Tb, K, Y=Yd, ctx=ctx))
            measure(f, shape, "entropy call", lambda: device.rank_targets_entropy(Xd, model, A, Tb, K, Yd, k=KNN, ctx=ctx))
            f.write("\t".join(["note", a.run, shape, "fma", "%d" % (B * K * K * P)]) + "\n")
            if not a.no_ckdtree:
                idx = device.rank_targets(Xd, model, A, Tb[:, :CKD_TARGETS], K, Y=Yd, ctx=ctx)[0].cpu().numpy()
                ckdtree(f, shape, [np.ascontiguousarray(Y[i]) for i in idx], B, "%d targets timed, scaled to %d" % (CKD_TARGETS, B))
        K, P = GENERIC
        V = np.random.default_rng(5).standard_normal((K, P))
        Vd = device.colmajor(V, dev)
        shape = "entropy, generic: K = %d, P = %d, k = %d" % (K, P, KNN)
        measure(f, shape, "entropy call", lambda: device.weighted_entropy(Vd, k=KNN, ctx=ctx))
        f.write("\t".join(["note", a.run, shape, "fma", "%d" % (K * K * P)]) + "\n")
        if not a.no_ckdtree:
            ckdtree(f, shape, [V], 1, "2000 of the %d queries timed, scaled" % K, queries=2000)


if __name__ == "__main__":
    main()
