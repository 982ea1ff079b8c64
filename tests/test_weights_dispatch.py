"""CPU checks of tests/_weights_dispatch.py, the tests' copy of the weight stage's kernel choice (weights_plan.h:
abc_weights_plan; weights.hip: the kernel tables behind launch_weights_prev and launch_weights_raw): it gives what the plan
function itself gives on every case of tests/cxx/weights_plan_probe.cpp, the instances it can reach are exactly the entries of
the tables the two launchers launch through, so the copy and the source cannot drift apart unseen, and the decisions on both
sides of every threshold are pinned."""
import itertools
import os
import re
import subprocess

import numpy as np

import _weights_dispatch as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("WROWS", "KDE_SPLIT", "KDE_FP64", "KDE_EPAN", "KDE_FIXUPS")


def _source(name="weights.hip"):
    return open(os.path.join(ROOT, "abcsmc_amd", "csrc", name)).read()


def _launchers():
    src = _source()
    body = src[src.index("int launch_weights_prev("):]
    body = body[:body.index("int abc_kde_words(abc_ctx* ctx) {")]
    return body[:body.index("int launch_weights_raw(")], body[body.index("int launch_weights_raw("):]


def _helper(name):
    """the text of a static helper of the two launchers"""
    src = _source()
    body = src[src.index("static void %s(" % name):]
    return body[:body.index("\n}\n")]


def _table(name):
    """the initialiser of one of the static const kernel tables, as text"""
    return re.search(r"static const \w+ %s(?:\[\d+\])+ = \{(.*?)\};" % name, _source(), re.S).group(1)


def _int(expr, names):
    return int(eval(expr, {"__builtins__": {}}, names))


def _tables():
    """-> the kernel tables of weights.hip in the order of their entries: split[plain | fold | top-order][NCH - 1] as the tuples of
    _weights_dispatch, wrows[NCH - 1] as (instance, rows-per-group divisor), and kde / epan / fixups[log2 PP] as widths (None: no entry)"""
    plan_h = _source("weights_plan.h")
    names = {k: int(re.search(r"constexpr int %s = (\d+);" % k, plan_h).group(1)) for k in ("KS_FOLD", "KS_TOPN")}
    names["KDE_LDS_W3"] = int(re.search(r"#define KDE_LDS_W3 (\d+)", _source()).group(1))
    assert names == {"KS_FOLD": D.KS_FOLD, "KS_TOPN": D.KS_TOPN, "KDE_LDS_W3": D.KDE_LDS_W3}
    flat = []
    for lds, args in re.findall(r"\bk_kde_split(_lds)?<([^>]*)>", _table("KDE_SPLIT")):
        a = [s.strip() for s in args.split(",")]
        flat.append(("split_lds" if lds else "split", _int(a[0], names), _int(a[1], names)))
    assert len(flat) == 12
    split = [flat[0:4], flat[4:8], flat[8:12]]
    wrows = [(tuple(int(x) for x in a.split(",")), int(d)) for a, d in re.findall(r"\{k_wrows<([\d, ]+)>, (\d+)\}", _table("WROWS"))]
    width = lambda tab, kernel: [int(pp) if pp else None for pp in re.findall(r"nullptr|%s<(\d+)>" % kernel, _table(tab))]
    return split, wrows, width("KDE_FP64", "k_kde"), width("KDE_EPAN", "k_epan"), width("KDE_FIXUPS", "k_kde_fixups")


def _named(text):
    """the kernels a piece of host code launches: by name, through a kernel table, or through a helper that does"""
    direct = re.findall(r"hipLaunchKernelGGL\(\(?(k_[a-z0-9_]+)", text)
    tabs = [t for t in TABLES if re.search(r"\b%s\[" % t, text)]
    via = re.findall(r"hipLaunchKernelGGL\((?:%s)\[|hipLaunchKernelGGL\(e\.fn," % "|".join(TABLES), text)
    assert len(direct) + len(via) == text.count("hipLaunchKernelGGL("), "a launch this reader does not understand"
    assert len(via) == len(tabs), "one launch per table"
    names = set(direct)
    for t in tabs:
        names |= set(re.findall(r"\b(k_[a-z0-9_]+)<", _table(t)))
    if "launch_wrows(" in text and not text.startswith("static void launch_wrows("):
        names |= _named(_helper("launch_wrows"))
    return names


def _launch_table():
    """-> (pair kernels, k_wrows instances of the previous set, ... of the new set, fix-up widths) the two launchers launch"""
    prev, raw = _launchers()
    split, wrows, kde, epan, fixups = _tables()
    # the width tables are indexed by log2 PP; k_wrows' by chunks with the rows a wave takes
    assert kde == epan == [None, 2, 4, 8, 16, 32, 64] and fixups == [None, None, None, 8, 16, 32, 64]
    assert [d for _, d in wrows] == [32, 16, 8, 8]
    for tab in ("KDE_SPLIT", "KDE_FP64", "KDE_EPAN", "KDE_FIXUPS"):
        assert len(re.findall(r"hipLaunchKernelGGL\(%s\[" % tab, raw)) == 1 and tab not in prev, tab
    assert "KDE_EPAN[ks_lg(PP)]" in raw and "KDE_FIXUPS[ks_lg(PP)]" in raw and "KDE_FP64[ks_lg(PP)]" in raw
    assert "KDE_SPLIT[pl.fold ? 1 : pl.topn ? 2 : 0][pl.NCH - 1]" in raw and "WROWS[pl.NCH - 1]" in _helper("launch_wrows")
    pairs = {k for row in split for k in row} | {("kde", w) for w in kde if w} | {("epan", w) for w in epan if w}
    gen = re.findall(r"hipLaunchKernelGGL\(k_kde_gen,.*?part, PP, (\d), \(int\)P, w_prev\);", raw, re.S)
    assert sorted(gen) == ["0", "1"], gen
    pairs |= {("gen", False), ("gen", True)}
    # both launchers reach k_wrows through the one helper and its table
    rows = lambda text: {inst for inst, _ in wrows} if len(re.findall(r"\blaunch_wrows\(pl, ", text)) == 1 else set()
    assert "k_wrows<" not in prev and "k_wrows<" not in raw
    # nothing else is launched from the two, the helper they call included
    assert _named(prev) == {"k_wprep", "k_wcentre", "k_wcentre_finish", "k_whb", "k_wq_hist", "k_wq_scan", "k_wq_rank", "k_wrows",
                            "k_wscale", "k_tile_tmin"}, _named(prev)
    assert _named(raw) == {"k_wrows", "k_wscale", "k_kde", "k_epan", "k_kde_gen", "k_kde_split", "k_kde_split_lds", "k_kde_fixups",
                           "k_wfinish"}, _named(raw)
    return pairs, rows(prev), rows(raw), {w for w in fixups if w}


def test_mirror_agrees_with_the_plan_function(tmp_path):
    """abc_weights_plan itself (tests/cxx/weights_plan_probe.cpp prints it) and the kernel tables of weights.hip, indexed as
    launch_weights_raw indexes them, against _weights_dispatch.plan on every case of the probe"""
    exe = str(tmp_path / "weights_plan_probe")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cxx", "weights_plan_probe.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    split_tab, wrows_tab, kde_tab, epan_tab, fix_tab = _tables()
    shapes = [(300, 700), (150, 700), (300, 1300), (300, 2049), (1, 700), (255, 700), (256, 700), (257, 700), (40000, 100000),
              (39999, 100000), (100000, 100000), (600000, 100000), (256, 10 ** 6), (3084, 10 ** 6), (100000, 10 ** 7)]
    shapes += [(300, Kp) for Kp in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
    want = set(itertools.product(list(range(1, 201)) + [1024], (0, 1), (0, 1), (4.0e9, 0.0), shapes))
    seen = set()
    for line in out.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split())
        minp = float(f.pop("minp"))
        f = {k: int(v) for k, v in f.items()}
        P, kn, Kp, PP, NCH = f["P"], f["kn"], f["Kp"], f["PP"], f["NCH"]
        seen.add((P, f["fp64"], f["epan_in"], minp, (kn, Kp)))
        lg = PP.bit_length() - 1
        if f["epan"]:
            pair = ("gen", True) if PP > 64 else ("epan", epan_tab[lg])
        elif f["split"]:
            pair = split_tab[1 if f["fold"] else 2 if f["topn"] else 0][NCH - 1]
            assert pair[1] == f["V"], line
        else:
            pair = ("gen", False) if PP > 64 else ("kde", kde_tab[lg])
        got = {"width": PP, "chunks": NCH, "split": bool(f["split"]), "fold": bool(f["fold"]), "topn": bool(f["topn"]), "pair": pair,
               "wrows": wrows_tab[NCH - 1][0] if f["split"] else None, "fixup": fix_tab[lg] if f["split"] else None,
               "slices": f["slices"], "tiles": f["nbt"], "lim_i": f["lim_i"]}
        assert got == D.plan(P, kn, Kp, "fp64" if f["fp64"] else "auto", "epan" if f["epan_in"] else "gauss", minp), line
        assert f["epan"] == f["epan_in"] and f["V"] == NCH + (D.KS_FOLD if f["fold"] else D.KS_TOPN if f["topn"] else 0), line
        assert f["rb"] == (kn + 255) // 256 and f["nat"] == 8 * f["rb"] and f["opa"] == 4 * NCH, line
        assert f["opb"] == f["opa"] + (0 if f["fold"] else 1), line
    assert seen == want and len(out.stdout.splitlines()) == len(want) == 201 * 2 * 2 * 2 * 25


def test_mirror_reaches_exactly_the_launch_sites():
    pairs, rows_prev, rows_raw, fix = _launch_table()
    r_pairs, r_rows, r_fix = D.reachable()
    assert r_pairs == pairs, "in the mirror only: %s; in weights.hip only: %s" % (sorted(r_pairs - pairs), sorted(pairs - r_pairs))
    split = {k for k in pairs if k[0].startswith("split")}
    assert split == {("split", 1, 3), ("split", 2, 2), ("split_lds", 3, 3), ("split_lds", 4, 2),
                     ("split", 101, 3), ("split", 102, 2), ("split_lds", 103, 3), ("split_lds", 104, 2),
                     ("split", 201, 3), ("split", 202, 2), ("split_lds", 203, 3), ("split_lds", 204, 2)}
    widths = (2, 4, 8, 16, 32, 64)
    assert {k for k in pairs if k[0] == "kde"} == {("kde", w) for w in widths}
    assert {k for k in pairs if k[0] == "epan"} == {("epan", w) for w in widths}
    assert len(pairs) == 12 + 6 + 6 + 2
    assert r_fix == fix == {8, 16, 32, 64}
    assert r_rows == rows_prev == rows_raw == {(1,), (2,), (4, 3), (4,)}


def test_the_far_bounds_are_the_kernels():
    src = _source()
    val = lambda name: float(re.search(r"\b%s = (-?[\d.]+)" % name, src).group(1))
    assert (val("KS_BOUND"), val("KS_NORM2"), val("KS_LW_CAP"), val("KS_LW_MIN")) == (D.KS_BOUND, D.KS_NORM2, D.KS_LW_CAP, D.KS_LW_MIN)
    assert val("KS_MAX_FAR_J") == D.KS_MAX_FAR_J and val("W_COORD_BOUND") == D.W_COORD_BOUND
    assert "const double minp = e ? atof(e) : 4.0e9;" in src and D.TOPN_MIN_PAIRS == 4.0e9
    # the far-row budget of the plan; launch_weights_prev plans for kn_max rows and hands it to k_wprep
    assert "pl.lim_i = (int)(kn / 16 + 32);" in _source("weights_plan.h")
    assert "abc_weights_plan(P, kn_max, Kp, " in src and "(int)P, wc, pl.lim_i);" in src


def _p(P, kn=300, Kp=700, **kw):
    return D.plan(P, kn, Kp, **kw)


def test_parameter_thresholds():
    want = {   # P: (width, chunks, fold, pair, wrows, fixup)
        4: (4, 1, False, ("kde", 4), None, None), 5: (8, 1, True, ("split", 101, 3), (1,), 8),
        8: (8, 1, True, ("split", 101, 3), (1,), 8), 9: (16, 1, True, ("split", 101, 3), (1,), 16),
        13: (16, 1, True, ("split", 101, 3), (1,), 16), 14: (16, 1, False, ("split", 1, 3), (1,), 16),
        16: (16, 1, False, ("split", 1, 3), (1,), 16), 17: (32, 2, True, ("split", 102, 2), (2,), 32),
        29: (32, 2, True, ("split", 102, 2), (2,), 32), 30: (32, 2, False, ("split", 2, 2), (2,), 32),
        32: (32, 2, False, ("split", 2, 2), (2,), 32), 33: (64, 3, True, ("split_lds", 103, 3), (4, 3), 64),
        45: (64, 3, True, ("split_lds", 103, 3), (4, 3), 64), 46: (64, 3, False, ("split_lds", 3, 3), (4, 3), 64),
        48: (64, 3, False, ("split_lds", 3, 3), (4, 3), 64), 49: (64, 4, True, ("split_lds", 104, 2), (4,), 64),
        61: (64, 4, True, ("split_lds", 104, 2), (4,), 64), 62: (64, 4, False, ("split_lds", 4, 2), (4,), 64),
        64: (64, 4, False, ("split_lds", 4, 2), (4,), 64), 65: (128, 4, False, ("gen", False), None, None),
    }
    for P, w in want.items():
        pl = _p(P)
        assert (pl["width"], pl["chunks"], pl["fold"], pl["pair"], pl["wrows"], pl["fixup"]) == w, P
        assert pl["split"] == (5 <= P <= 64) and not pl["topn"]
    assert [D.padded_width(P) for P in (1, 2, 3, 64, 65, 128, 129, 1024)] == [2, 2, 4, 64, 128, 128, 192, 1024]
    # fp64 on request and the Epanechnikov extension: never the split kernel, its limb tiles or its fix-ups
    for P, pp in ((1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)):
        for kw, kern in ((dict(kde_mode="fp64"), "kde"), (dict(weight_kernel="epan"), "epan")):
            pl = _p(P, **kw)
            assert pl["pair"] == (kern, pp) and not pl["split"] and pl["wrows"] is None and pl["fixup"] is None, (P, kw)
    assert _p(65, weight_kernel="epan")["pair"] == ("gen", True) and _p(65, kde_mode="fp64")["pair"] == ("gen", False)


def test_top_order_threshold():
    # tiles in the order of the norm tops: full chunks only, from ABC_KDE_TOPN_MIN_PAIRS pairs (kn x K') on
    assert 40000 * 100000 == 4.0e9
    for P, v in ((14, ("split", 201, 3)), (16, ("split", 201, 3)), (30, ("split", 202, 2)), (32, ("split", 202, 2)),
                 (46, ("split_lds", 203, 3)), (48, ("split_lds", 203, 3)), (62, ("split_lds", 204, 2)), (64, ("split_lds", 204, 2))):
        assert D.plan(P, 40000, 100000)["pair"] == v and D.plan(P, 40000, 100000)["topn"]
        under = D.plan(P, 39999, 100000)
        assert not under["topn"] and under["pair"] == (v[0], v[1] - D.KS_TOPN, v[2])
        assert _p(P, Kp=2049, topn_min_pairs=0.0)["pair"] == v
    for P in (5, 13, 17, 29, 33, 45, 49, 61):
        pl = D.plan(P, 40000, 100000)
        assert pl["fold"] and not pl["topn"] and pl["pair"] == _p(P)["pair"]
    assert not D.plan(16, 40000, 100000, kde_mode="fp64")["topn"] and not D.plan(16, 40000, 100000, weight_kernel="epan")["topn"]


def test_slices_tiles_and_the_far_row_budget():
    # K = 300 against K' = 700: ten slices (K' / 64), 22 previous tiles, the last one partial
    assert _p(16)["slices"] == 10 and _p(16)["tiles"] == 22 and _p(16)["lim_i"] == 50
    # the K' / 64 clamp and its floor of one slice
    assert [_p(16, Kp=k)["slices"] for k in (1, 63, 64, 127, 128, 129)] == [1, 1, 1, 1, 2, 2]
    assert [_p(3, Kp=k)["slices"] for k in (63, 64, 127, 128)] == [1, 1, 1, 2]
    assert [_p(16, Kp=k)["tiles"] for k in (1, 31, 32, 33, 63, 64, 65)] == [1, 1, 1, 2, 2, 2, 3]
    # abc_kde_slices: small sets get 4096 work-groups' worth of slices, capped at 1024 ...
    assert D.kde_slices(300, 700, 16) == 10 and D.kde_slices(300, 10 ** 6, 16) == 1024 == _p(16, Kp=10 ** 6, kde_mode="fp64")["slices"]
    assert D.kde_slices(100000, 100000, 16) == 66 and D.kde_slices(0, 5, 16) == 1 and D.kde_slices(5, 0, 16) == 1
    assert D.kde_slices(100000, 10 ** 7, 64) == 83                       # the 64 MB of partial sums: (64 << 20) / (8 kn)
    # ... and the split kernel at most 12288 / rb of them, but eight
    assert D.plan(16, 100000, 100000)["slices"] == 12288 // 391 == 31 and D.plan(16, 100000, 100000, kde_mode="fp64")["slices"] == 66
    assert D.plan(16, 600000, 100000)["slices"] == 8 and D.plan(16, 600000, 100000, kde_mode="fp64")["slices"] == 13
    assert D.plan(16, 256, 10 ** 6)["slices"] == 1024 and D.plan(16, 257 * 12, 10 ** 6)["slices"] == 652
    assert [_p(16, kn=k)["lim_i"] for k in (1, 15, 16, 150, 255, 256, 257)] == [32, 32, 33, 41, 47, 48, 48]


def test_far_rows_and_the_kernel_word():
    rng = np.random.default_rng(5)
    P, K, Kp = 6, 40, 90
    dv = rng.uniform(0.5, 3.0, P)
    unit = np.sqrt(dv) / D.SQRT_LOG2E
    tp = rng.normal(size=(Kp, P)) * unit * 0.8 + 10.0
    th = rng.normal(size=(K, P)) * unit * 0.6 + 10.0
    wp = rng.random(Kp) + 0.1
    c = D.centre(tp, dv)
    assert np.allclose(c, tp.mean(axis=0), rtol=0, atol=1e-12)           # without outliers: the column mean
    pl = D.plan(P, K, Kp)
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert not fi.any() and not fj.any() and not beyond and D.ran(pl, th, tp, wp, dv) == D.RAN_SPLIT
    th2, tp2, wp2 = th.copy(), tp.copy(), wp.copy()
    th2[3, 1] = c[1] + 8.01 * unit[1]
    th2[4, 1] = c[1] + 7.99 * unit[1]
    th2[5] = c + np.array([7.9, 7.9, 7.9, 7.9, 7.9, 7.9]) * unit         # squared norm 374.5: inside
    th2[6] = c + np.array([7.9, -7.9, 7.9, -7.9, 7.9, 7.9]) * unit * np.sqrt(401.0 / 374.46)      # 401, coordinates 8.17: both
    # by the norm alone, every coordinate below 8 (seven parameters of unit scale, the centre at 0)
    norm_only = np.array([[np.sqrt(401.0 / 7)] * 7, [np.sqrt(399.0 / 7)] * 7])
    assert norm_only.max() < 7.6
    assert list(D.far(norm_only, np.zeros((2, 7)), np.ones(2), np.full(7, np.log2(np.e)))[0]) == [True, False]
    wp2[[7, 8, 9, 10, 11]] = [2.0 ** -301, 2.0 ** -299, 2.0 ** 101, 2.0 ** 99, 0.0]
    tp2[11, 0] += 500 * unit[0]                                          # weight 0: never far, wherever it lies
    fi, fj, beyond = D.far(th2, tp2, wp2, dv)
    # (the outlier of weight 0 moves the centre by 16 / K' units: rows 3 and 4 stay on their sides of the bound)
    assert list(np.flatnonzero(fi)) == [3, 6] and list(np.flatnonzero(fj)) == [7, 9] and not beyond
    assert D.ran(pl, th2, tp2, wp2, dv) == D.RAN_SPLIT
    tp3 = tp.copy()
    tp3[2, 4] += 3000 * unit[4]
    assert D.far(th, tp3, wp, dv)[2] and D.ran(pl, th, tp3, wp, dv) == D.RAN_FP64
    # a previous row 3000 units away moves the centre by its clipped offset, 16 / K' units (+ what it had), not by 3000 / K'
    assert 10.0 / Kp < np.max(np.abs(D.centre(tp3, dv) - c) / unit) < 20.0 / Kp
    dv0 = dv.copy()
    dv0[2] = 0.0
    assert D.scale(dv0)[2] == 0.0 and D.centre(tp, dv0)[2] == tp[0, 2] and D.ran(pl, th, tp, wp, dv0) == D.RAN_FP64
    # the far-row budgets: lim_i = 34 new rows, 1024 previous ones
    thm = th.copy()
    thm[:34, 0] = c[0] + 9 * unit[0]
    assert D.far(thm, tp, wp, dv)[0].sum() == 34 and D.ran(pl, thm, tp, wp, dv) == D.RAN_SPLIT
    thm[34, 0] = c[0] + 9 * unit[0]
    assert D.ran(pl, thm, tp, wp, dv) == D.RAN_FP64
    assert D.ran(D.plan(P, K, Kp, kde_mode="fp64"), th, tp, wp, dv) == D.RAN_FP64
