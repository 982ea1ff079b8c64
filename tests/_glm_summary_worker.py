"""Worker of test_gpu_glm_summary.py's arena test: the four *_summary entries of ABC-GLM on a fresh context each and on one warm
context whose arena a larger earlier call has grown, then the four older entries (tests/_glm_worker.py's calls, unchanged) on a
fresh context each, in this process; the parent runs it once as the environment is and once under ABC_WS_POISON=ff (the library
reads the switch once per process), where every call starts from an arena full of NaN bytes.

Writes one .npz: "<mode>|<entry>|info" (abc_ws_info's reserved, asked, peak right after the call) and "<mode>|<entry>|<output>";
mode is warm, fresh or old.  A HIP error ends the run at once (nothing more is started on a device that has faulted).

usage: _glm_summary_worker.py OUT.npz"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import _glm_worker as GW

PROBS = (0.975, 0.025, 0.5, 0.5, 1e-6)


def entries(ctx, F):
    """name -> call() -> dict of outputs, each on ctx; F: the fit, made on another context"""
    import torch
    from abcsmc_amd import device, glm
    import test_gpu_glm as TG
    import test_gpu_glm_summary as TS
    X, Y, T, th, st, ob, w = GW.inputs()
    truth = Y[[5, 50, 500]]

    def dev():
        r = device.rank_targets_glm(F["Xd"], F["model"], 3, device.colmajor(T, TG.DEV), 100, F["Yd"], G=600, dist=True, outputs=GW.OUT, ctx=ctx,
                                    probs=PROBS, truth=torch.tensor(truth, device=TG.DEV))
        return TG.to_np(r)

    def host():
        return glm.particle_ranking_PLS_targets_glm(X, Y, T, 0.5, 100, G=600, max_comp=3, rule=0, ctx=ctx, outputs=GW.OUT, probs=PROBS,
                                                    truth=truth)

    def gen_host():
        return glm.weighted_glm(th, st, ob, w, G=33, ctx=ctx, outputs=GW.OUT, probs=PROBS, truth=th[3])

    def gen_dev():
        return TS.generic(ctx, th, st, ob, w, None, probs=PROBS, truth=th[3], outputs=GW.OUT, dev=True, G=33)

    def large():
        return glm.weighted_glm(np.tile(th, (20, 1)), np.tile(st, (20, 1)), ob, None, G=4096, ctx=ctx, outputs=GW.OUT, probs=PROBS,
                                truth=th[3])

    return dict(dev=dev, host=host, gen_host=gen_host, gen_dev=gen_dev), large


def main(out_path):
    from abcsmc_amd import _lib
    res = {}

    def one(mode, name, ctx, call):
        print(mode, name, flush=True)
        try:
            r = call()
        except _lib.AbcError as e:
            print(e, flush=True)
            np.savez_compressed(out_path, **res)
            sys.exit(3 if e.code == -2 else 4)
        res["%s|%s|info" % (mode, name)] = np.asarray(ctx.ws_info(), dtype=np.uint64)
        for k, v in r.items():
            if v is not None and k != "ncomp":
                res["%s|%s|%s" % (mode, name, k)] = np.ascontiguousarray(v)

    import test_gpu_glm as TG
    prep = _lib.Context(0)
    X, Y = GW.inputs()[:2]
    F = TG.fit(prep, X, Y, 3)
    warm = _lib.Context(0)
    calls, large = entries(warm, F)
    large()
    for name, call in calls.items():
        one("warm", name, warm, call)
    warm.close()
    for name in calls:
        ctx = _lib.Context(0)
        one("fresh", name, ctx, entries(ctx, F)[0][name])
        ctx.close()
    for name in calls:
        ctx = _lib.Context(0)
        one("old", name, ctx, GW.entries(ctx, F)[0][name])
        ctx.close()
    np.savez_compressed(out_path, **res)
    prep.close()


if __name__ == "__main__":
    main(sys.argv[1])
