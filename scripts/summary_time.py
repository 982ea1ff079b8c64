"""Times the weighted posterior summaries of the batched ranking (abc_rank_targets_summary_dev) against the plain batched
ranking (abc_rank_targets_dev), the coef-only adjustment (abc_rank_targets_adjust_dev) and the alternative they replace: the
retained rows (method 0) or theta and the weights (method 1) copied to the host and sorted there with NumPy.  N = 1e6 rows,
M = 32 metrics, P = 16 parameters, A = 8 components, K = 1e4, probs (0.025, 0.5, 0.975) plus the CDF at a truth, B in
{1, 16, 256, 1024}.  A second table compares the LDS and global paths (ABC_SUMMARY_PATH under ABC_DIAG=1) at B = 256 around
the LDS path's limit.  Writes a text table (default profiles/summary_time.txt).
--only B: one method-1 summary call at that B, nothing written (for a rocprofv3 kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

os.environ["ABC_DIAG"] = "1"          # (read once, at the library's first getenv; ABC_SUMMARY_PATH is read per call)
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abcsmc_amd import _lib, device, synthetic  # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def host_summary(v, w, truth):
    """v (B, K, P), w (B, K) or None, truth (B, P): the header's quantiles / CDF with NumPy (float64 sums)"""
    v = np.moveaxis(v, 1, 2)                                     # (B, P, K)
    o = np.argsort(v, axis=-1, kind="stable")
    u = np.take_along_axis(v, o, -1)
    om = np.ones_like(u) if w is None else np.take_along_axis(np.broadcast_to(w[:, None, :], v.shape), o, -1)
    W = np.cumsum(om, axis=-1)
    p = (W - 0.5 * om) / W[..., -1:]
    n = u.shape[-1]
    qs = []
    for q in PROBS:
        r = np.clip((p <= q).sum(-1) - 1, 0, n - 2)[..., None]
        plo, phi = np.take_along_axis(p, r, -1), np.take_along_axis(p, r + 1, -1)
        ulo, uhi = np.take_along_axis(u, r, -1), np.take_along_axis(u, r + 1, -1)
        t = np.clip((q - plo) / (phi - plo), 0.0, 1.0)
        qs.append((ulo + t * (uhi - ulo))[..., 0])
    cdf = (np.where(u < truth[..., None], om, 0).sum(-1) + 0.5 * np.where(u == truth[..., None], om, 0).sum(-1)) / W[..., -1]
    return np.stack(qs, 1), cdf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--K", type=int, default=10000)
    ap.add_argument("--B", type=str, default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_time.txt"))
    a = ap.parse_args()
    N, M, P, A, K = a.N, 32, 16, 8, a.K
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
    T, TY = wl.rows_by_index((1 << 40) + np.arange(max(max(Bs), 256)))
    Td_all = device.colmajor(T, dev)
    truth_all = torch.tensor(np.ascontiguousarray(TY), dtype=torch.float64, device=dev)

    def summ(B, method, k=K, path=None):
        if path:
            os.environ["ABC_SUMMARY_PATH"] = path
        else:
            os.environ.pop("ABC_SUMMARY_PATH", None)
        device.rank_targets_summary(Xd, model, A, Td_all[:, :B], k, Yd, probs=PROBS, truth=truth_all[:B], method=method, ctx=ctx)

    if a.only:
        summ(a.only, _lib.POSTERIOR_LOCLINEAR)
        torch.cuda.synchronize()
        return

    def plain(B):
        device.rank_targets(Xd, model, A, Td_all[:, :B], K, ctx=ctx)

    def coef(B):
        device.rank_targets_adjust(Xd, model, A, Td_all[:, :B], K, Yd, theta=False, weight=False, ctx=ctx)

    def host0(B):
        idx, _, _ = device.rank_targets(Xd, model, A, Td_all[:, :B], K, ctx=ctx)
        v = Yd.T[idx].cpu().numpy()                               # (B, K, P) gathered on the device, sorted on the host
        host_summary(v, None, truth_all[:B].cpu().numpy())

    def host1(B):
        r = device.rank_targets_adjust(Xd, model, A, Td_all[:, :B], K, Yd, theta=True, weight=True, ctx=ctx)
        host_summary(r["theta"].cpu().numpy(), r["weight"].cpu().numpy(), truth_all[:B].cpu().numpy())

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

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = ["# scripts/summary_time.py on %s: N = %d, M = %d, P = %d, A = %d (nc = %d), K = %d, probs %s plus the CDF; wall ms "
             "per call (median of %d after one warm-up; host columns: one run)" % (torch.cuda.get_device_name(0), N, M, P, A, nc,
                                                                                     K, PROBS, a.reps),
             "# plain: abc_rank_targets_dev; coef: abc_rank_targets_adjust_dev writing coef only; rej / ll: "
             "abc_rank_targets_summary_dev method 0 / 1 (quant and cdf only)",
             "# +rej = rej - plain, +ll = ll - coef; host_rej / host_ll: plain + Y[idx] / the adjust call with theta and weight, copied "
             "to the host and summarised with NumPy",
             "%6s %9s %9s %9s %9s %9s %9s %11s %11s" % ("B", "plain_ms", "coef_ms", "rej_ms", "ll_ms", "+rej_ms", "+ll_ms",
                                                       "host_rej_ms", "host_ll_ms")]
    for B in Bs:
        tp = timeit(lambda: plain(B), a.reps)
        tc = timeit(lambda: coef(B), a.reps)
        t0 = timeit(lambda: summ(B, 0), a.reps)
        t1 = timeit(lambda: summ(B, 1), a.reps)
        h0 = once(lambda: host0(B))
        h1 = once(lambda: host1(B))
        lines.append("%6d %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %11.1f %11.1f" % (B, tp, tc, t0, t1, t0 - tp, t1 - tc, h0, h1))
        print(lines[-1], flush=True)
    lines.append("# paths at B = 256, method 0: the summary call with ABC_SUMMARY_PATH=lds / global (the LDS path ends at K = 8192)")
    lines.append("%6s %9s %9s %9s" % ("K", "plain_ms", "lds_ms", "global_ms"))
    for k in (1024, 2048, 4096, 8192):
        tp = timeit(lambda: device.rank_targets(Xd, model, A, Td_all[:, :256], k, ctx=ctx), a.reps)
        tl = timeit(lambda: summ(256, 0, k, "lds"), a.reps)
        tg = timeit(lambda: summ(256, 0, k, "global"), a.reps)
        lines.append("%6d %9.3f %9.3f %9.3f" % (k, tp, tl, tg))
        print(lines[-1], flush=True)
    os.environ.pop("ABC_SUMMARY_PATH", None)
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
