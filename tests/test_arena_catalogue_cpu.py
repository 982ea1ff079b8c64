"""CPU: the catalogue of tests/_arena_cases.py covers the header, its rows say what they build, and the worker compiles.  No GPU call."""
import os
import py_compile
import re

import numpy as np
import pytest

import _arena_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


def _context_functions():
    """every function of include/abcsmc_hip.h whose first parameter is abc_ctx* (const or not; abc_ctx* const* too)"""
    txt = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(abc_[a-z0-9_]+)\s*\(\s*(?:const\s+)?abc_ctx\s*\*\s*(?:const\s*\*\s*)?[a-z_]+\s*[,)]", txt)))


def test_every_context_function_is_catalogued_or_exempt():
    declared = set(_context_functions())
    assert len(declared) >= 100 and "abc_weighted_hpd_dev" in declared and "abc_generation_multi" in declared
    named = {c.entry for c in AC.CASES.values()}
    assert not named - declared, "rows name functions the header does not declare: %s" % sorted(named - declared)
    assert not set(AC.EXEMPT) - declared, "stale exemptions: %s" % sorted(set(AC.EXEMPT) - declared)
    assert not named & set(AC.EXEMPT), sorted(named & set(AC.EXEMPT))
    assert not declared - named - set(AC.EXEMPT), "neither catalogued nor exempt: %s" % sorted(declared - named - set(AC.EXEMPT))
    for fn, why in AC.EXEMPT.items():
        assert why.strip() and "\n" not in why, fn
        # an exemption is a setter, a getter, a communicator call, a sharded driver, or says why it takes nothing from the arena
        assert re.search(r"setter|getter|abc_comm_|sharded|no arena|frees the context", why), (fn, why)


def test_the_settings_and_entry_forms_the_catalogue_promises():
    by_entry = {}
    for c in AC.CASES.values():
        by_entry.setdefault(c.entry, []).append(c)
    for product in ("summary", "hpd", "density", "joint", "draws", "entropy"):
        for form in ("abc_rank_targets_%s_dev", "abc_particle_ranking_pls_targets_%s", "abc_weighted_%s_dev", "abc_weighted_%s"):
            assert form % product in by_entry, form % product
    for entry in ("abc_rank_targets_adjust_dev", "abc_rank_targets_path_dev"):          # the regressing entries under every setting
        seen = {k for c in by_entry[entry] for k in c.settings}
        assert seen == {"hcorr", "ridge", "transf", "row_weights"}, (entry, seen)
        assert any(not c.settings for c in by_entry[entry])
    assert {k for c in AC.CASES.values() for k in c.settings} == {"hcorr", "ridge", "transf", "row_weights"}
    assert len(AC.RIDGE) == 8 and len(AC.HPD_MASS) == 16 and AC.PATH_T == 16 and len(AC.PATH_KS) == 16       # the header's limits


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_row_states_what_it_builds(name):
    c = AC.CASES[name]
    h = c.host()
    for k, shape in c.shapes.items():
        assert np.asarray(h[k]).shape == tuple(shape), (k, np.asarray(h[k]).shape, shape)
        assert np.asarray(h[k]).dtype in (np.float64, np.int64), k
    for k, v in h.items():
        if isinstance(v, np.ndarray):
            assert k in c.shapes, "the row builds %s without stating its shape" % k
    assert c.klass in ("block", "sharp", "stage")
    if c.klass == "sharp":
        assert c.entry in AC.SHARP_ENTRIES, c.entry
    if c.klass == "stage":
        assert c.entry in AC.STAGE_ENTRIES and not c.blocks, c.entry
    if c.klass == "block":
        assert c.entry not in AC.SHARP_ENTRIES | AC.STAGE_ENTRIES
        assert c.dominant >= 4 * MIB, "largest stated block %d B" % c.dominant
        N, P = h["Y"].shape
        B = h["targets"].shape[0]
        for what, nbytes, recipe in c.blocks:
            assert recipe is not None, what
            assert nbytes == AC.block_from_recipe(recipe, N, P, c.A, B), (what, nbytes)
    for what, nbytes, _ in c.blocks:
        assert what and nbytes > 0, what


def test_plans_behind_the_block_arithmetic():
    """the figures the catalogue's shapes were chosen for"""
    assert AC.moment_bytes(1, 4000, 8, 16) == 16 * 9 * 25 * 8                    # 16 chunks x (1 + A) x (1 + A + P) doubles a target
    assert AC.sort_bytes(40, 9000, 16) == 40 * 16 * 9000 * 24                    # one batch
    assert AC.sort_bytes(1, 8192, 3) == 0 and AC.sort_bytes(1, 8193, 3) > 0      # the last LDS size
    # sm_batch floors: two targets a batch at the smaller tolerance, one at K_max, and the smaller one's buffers are the larger
    assert AC.sort_bytes(3, 80000, 64) == 2 * 64 * 80000 * 24 > AC.sort_bytes(3, 100000, 64) == 64 * 100000 * 24
    assert AC.sort_bytes(3, 300000, 16) == 2 * 16 * 300000 * 24 > AC.sort_bytes(3, 500000, 16) == 16 * 500000 * 24
    assert 4 * 512 * 4000 >= AC.FIT["N"]                                         # the adjust rows take the row-major table


def test_worker_compiles():
    py_compile.compile(os.path.join(ROOT, "tests", "_arena_worker.py"), doraise=True)
    py_compile.compile(os.path.join(ROOT, "tests", "_arena_cases.py"), doraise=True)
