"""Times the heteroscedastic variance correction of the local-linear adjustment (abc_ctx_set_adjust_hcorr): N = 1e6 rows, M = 32
metrics, P = 16 parameters, A = 8 components, K = 10000, B = 16 / 256 targets.  Per B the adjustment (theta and weights), the
summaries, densities, joint posteriors (moments and every pair at G = 64) and draws under method 1, and the tolerance path of four
tolerances, each
  (a) on a library built from the parent commit (--parent with ABCSMC_HIP_SO=<that library>: the new entries are not bound),
  (b) on this library with the setting off,
  (c) with it on,
(b) and (c) alternating call by call in one process (the setting changes between the timed brackets, never inside one), (a) in
processes of its own that the caller alternates with the others.  Every process appends its samples (ms per call between two
device events, after a warm-up of 2) to --samples; --report reads them all and writes the table (default
profiles/hcorr_time.txt): per leg the median (min .. max) over every sample, b / a beside the run-to-run spread of (a) (the
medians of its processes), and c - b.

The sequence behind profiles/hcorr_time.txt, on one card, from the repository's root (PARENT_SO: libabcsmc_hip.so built by
`make -C abcsmc_amd/csrc` in a checkout of the parent commit; S: a samples file that does not exist yet, it is scratch and is
not kept):
    for r in 1 2 3; do
        ABCSMC_HIP_SO=$PARENT_SO python scripts/hcorr_time.py --parent --run p$r --samples $S
        python scripts/hcorr_time.py --run n$r --samples $S
    done
    python scripts/hcorr_time.py --report --samples $S --out profiles/hcorr_time.txt
Three processes of five repetitions per library: 15 samples a leg."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ("abc_ctx_set_adjust_hcorr", "abc_adjust_last_hcorr", "abc_adjust_hcorr_skipped")


def report(samples, out):
    rows, order = {}, []
    head = ""
    for ln in open(samples):
        if ln.startswith("#"):
            head = head or ln.rstrip("\n")
            continue
        tag, run, B, call, leg, *t = ln.rstrip("\n").split("\t")
        key = (int(B), call)
        if key not in order:
            order.append(key)
        rows.setdefault(key, {}).setdefault((tag, leg), {}).setdefault(run, []).extend(float(x) for x in t)
    lines = [head, "# ms per call: median (min .. max) over every sample of every process; (a) parent, (b) setting off, (c) setting on;",
             "# spread(a): the medians of the parent's processes, (max - min) / median"]
    for key in order:
        r = rows[key]
        med = {}
        for k, runs in r.items():
            allv = np.concatenate([np.asarray(v) for v in runs.values()])
            med[k] = (float(np.median(allv)), float(allv.min()), float(allv.max()), [float(np.median(v)) for v in runs.values()], allv.size)
        a, b, c = med.get(("parent", "off")), med.get(("new", "off")), med.get(("new", "on"))
        txt = "B = %-4d %-18s" % key
        for name, m in (("a", a), ("b", b), ("c", c)):
            if m:
                txt += "  (%s) %9.3f (%.3f .. %.3f, n = %d)" % (name, m[0], m[1], m[2], m[4])
        if a and b:
            txt += "  b/a %.3f  spread(a) %.3f" % (b[0] / a[0], (max(a[3]) - min(a[3])) / a[0])
        if b and c:
            txt += "  c-b %+.3f ms (x%.2f)" % (c[0] - b[0], c[0] / b[0])
        lines.append(txt)
    txt = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(txt)
    print(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--B", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="0", help="a label for this process's samples")
    ap.add_argument("--parent", action="store_true", help="the setting-off legs alone (a library without the correction)")
    ap.add_argument("--samples", default=os.path.join(ROOT, "profiles", "hcorr_time.samples.tsv"))
    ap.add_argument("--report", action="store_true", help="no measurement: the table from --samples")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hcorr_time.txt"))
    a = ap.parse_args()
    if a.report:
        return report(a.samples, a.out)
    import torch
    from abcsmc_amd import _lib, device, synthetic
    if not torch.cuda.is_available():
        sys.exit("hcorr_time.py: no GPU (nothing is measured without one)")
    if a.parent:
        for n in NEW_ENTRIES:
            _lib.SIGNATURES.pop(n, None)
    N, M, P, A, K = a.N, 32, 16, 8, a.K
    Ks = (K // 8, K // 4, K // 2, K)
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
    Tall, _ = wl.rows_by_index((1 << 40) + np.arange(max(a.B)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def setting(on):
        if not a.parent:
            ctx.set_adjust_hcorr(on)

    tag = "parent" if a.parent else "new"
    legs = (False,) if a.parent else (False, True)
    new_file = not os.path.exists(a.samples)
    with open(a.samples, "a") as f:
        if new_file:
            f.write("# scripts/hcorr_time.py on %s: N = %d, M = %d, P = %d, A = %d, K = %d, path Ks = %s\n" %
                    (torch.cuda.get_device_name(0), N, M, P, A, K, list(Ks)))
        for B in a.B:
            Td = device.colmajor(np.ascontiguousarray(Tall[:B]), dev)
            args = (Xd, model, A, Td)
            calls = (("adjust", lambda: device.rank_targets_adjust(*args, K, Yd, ctx=ctx)),
                     ("summary m1", lambda: device.rank_targets_summary(*args, K, Yd, method=1, ctx=ctx)),
                     ("density m1", lambda: device.rank_targets_density(*args, K, Yd, method=1, ctx=ctx)),
                     ("joint m1", lambda: device.rank_targets_joint(*args, K, Yd, method=1, ctx=ctx)),
                     ("draws m1", lambda: device.rank_targets_draws(*args, K, Yd, 1000, smooth=True, method=1, ctx=ctx)),
                     ("path summary m1 x4", lambda: device.rank_targets_path_summary(*args, Ks, Yd, method=1, ctx=ctx)))
            for name, fn in calls:
                for on in legs:
                    setting(on)
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                t = {on: [] for on in legs}
                for _ in range(a.reps):
                    for on in legs:
                        setting(on)
                        t[on].append(timed(fn))
                setting(False)
                for on in legs:
                    f.write("\t".join([tag, a.run, str(B), name, "on" if on else "off"] + ["%.4f" % v for v in t[on]]) + "\n")
                    f.flush()
                    print(tag, a.run, B, name, "on" if on else "off", "%.3f" % float(np.median(t[on])), flush=True)


if __name__ == "__main__":
    main()
