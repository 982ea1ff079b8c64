"""Worker of test_gpu_arena.py: runs the catalogue of tests/_arena_cases.py twice in this process and writes one .npz.

  warm   one context; first the case with the largest stated block, so that the arena is at its largest and full of another call's
         data, then every case on that context
  fresh  every case on a new context of its own, closed afterwards

For every (mode, case) the .npz holds, under "<mode>|<case>|<field>": rc (0, or the library's status), err (its text), info (the
abc_ws_info triple reserved, asked, peak read right after the call), secs, and out:<name> for every output and path counter.  An
output above 8 KiB is stored as its SHA-256 (out:<name>#sha256) -- the parent compares bytes, and a digest compares the same.

The parent runs this program once as the environment is and once under ABC_WS_POISON=ff (the library reads it once per process).
Every case's name is printed, flushed, before it runs, so that a fault names its case.  A HIP error ends the run at once with
exit status 3, the results so far written: nothing more is started on a device that has faulted.

usage: _arena_worker.py OUT.npz [case ...]      (no case: the whole catalogue)"""
import hashlib
import os
import sys
import time
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

BIG = 8 << 10


def store(res, mode, name, rc, err, info, secs, out):
    p = "%s|%s|" % (mode, name)
    res[p + "rc"] = np.asarray(rc, dtype=np.int64)
    res[p + "err"] = np.asarray(err)
    res[p + "info"] = np.asarray(info, dtype=np.uint64)
    res[p + "secs"] = np.asarray(secs)
    for k, v in out.items():
        a = np.ascontiguousarray(v)
        if a.nbytes > BIG:
            h = hashlib.sha256(a.view(np.uint8).reshape(-1).data)
            h.update(repr((a.dtype.str, a.shape)).encode())
            res[p + "out:" + k + "#sha256"] = np.frombuffer(h.digest(), dtype=np.uint8)
        else:
            res[p + "out:" + k] = a


def run_case(case, ctx, prep):
    """-> (rc, err, info, secs, outputs); rc -2 (ABC_ERR_HIP) ends the worker"""
    from abcsmc_amd import _lib
    t0 = time.perf_counter()
    rc, err, out = 0, "", {}
    try:
        out = case.run(ctx, prep)
    except _lib.AbcError as e:
        rc, err = e.code, str(e)
    except Exception:       # noqa: BLE001 -- a mistake of the row itself: recorded, so that the parent names the case
        rc, err = 999, traceback.format_exc()
    return rc, err, ctx.ws_info(), time.perf_counter() - t0, out


def main(argv):
    out_path, only = argv[1], argv[2:]
    import _arena_cases as AC
    from abcsmc_amd import _lib
    names = [n for n in AC.CASES if not only or n in only]
    assert names and (not only or len(names) == len(set(only))), "unknown case among %r" % (only,)
    res = {}
    prep = _lib.Context(0)

    def one(mode, name, ctx):
        print("%s %s" % (mode, name), flush=True)
        r = run_case(AC.CASES[name], ctx, prep)
        store(res, mode, name, *r)
        print("   rc %d  reserved %d asked %d peak %d  %.2f s" % ((r[0],) + tuple(r[2]) + (r[3],)), flush=True)
        if r[0] == -2 or (r[0] == 999 and "hip" in r[1].lower() and "error" in r[1].lower()):
            print(r[1], flush=True)
            np.savez_compressed(out_path, **res)
            sys.exit(3)

    warm = _lib.Context(0)
    first = max(names, key=lambda n: AC.CASES[n].dominant)
    print("warm-up: %s" % first, flush=True)
    r = run_case(AC.CASES[first], warm, prep)
    if r[0]:
        print(r[1], flush=True)
        if r[0] == -2:
            sys.exit(3)
    for name in names:
        one("warm", name, warm)
    warm.close()
    for name in names:
        ctx = _lib.Context(0)
        one("fresh", name, ctx)
        ctx.close()
    np.savez_compressed(out_path, **res)
    prep.close()


if __name__ == "__main__":
    main(sys.argv)
