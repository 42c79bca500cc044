"""The table of tests/test_env_variants_gpu.py names every switch that eld_amd/csrc reads from the environment (no GPU needed).

A switch is a getenv("ELD_...") in a .hip or .h file of eld_amd/csrc.  Each one is either run by a case of the GPU module (a key of some case's
environment), or listed in EXCLUDED with the reason: a new switch cannot be added without a test or a stated reason, and a case cannot outlive its switch."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'eld_amd', 'csrc')



def _switches():
    """the switches of the settings table (tests/variant_child.py ENV, which tests/test_env_variants_gpu.py runs case by case), read from the source:
    the module's rows need torch, its ENV literal does not, and this test must run where torch is missing"""
    with open(os.path.join(ROOT, 'tests', 'variant_child.py')) as fh:
        tree = ast.parse(fh.read())
    env = [ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', '') == 'ENV']
    assert len(env) == 1
    return sorted({k for e in env[0].values() for k in e})


SWITCHES = _switches()

EXCLUDED = {
    'ELD_XCD': 'tested: tests/test_placement_gpu.py (same bits with and without the XCD-aware ids)',
    'ELD_TILE_BAND': 'tested: tests/test_placement_gpu.py (same convolutions, weight gradients to summation order)',
    'ELD_NOISE_DBG': 'dump switch of a developer build (ELD_DEV_TOOLS): selects no kernel',
    'ELD_CONV_DBG': 'dump switch of a developer build (ELD_DEV_TOOLS): selects no kernel',
    'ELD_DEBUG_KERNEL_MASK': 'has a run-time setter, eld_debug_kernel_mask, which the tests of tests/test_unet_gpu.py already use',
}


def switches_read(csrc=CSRC):
    found = {}
    for f in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        with open(f) as fh:
            for name in re.findall(r'getenv\(\s*"(ELD_[A-Z0-9_]+)"\s*\)', fh.read()):
                found.setdefault(name, []).append(os.path.basename(f))
    return found


def uncovered(found, tested, excluded):
    return sorted(n for n in found if n not in tested and n not in excluded)


def test_every_switch_is_run_or_excluded_with_a_reason():
    found = switches_read()
    assert 'ELD_X3W' in found and 'ELD_CONV_TILES' in found      # (the scan itself still finds them)
    missing = uncovered(found, SWITCHES, EXCLUDED)
    assert not missing, 'switches without a case in tests/variant_child.py CASES or a reason in EXCLUDED: %s' % missing
    assert not set(SWITCHES) & set(EXCLUDED)
    stale = sorted(n for n in list(SWITCHES) + list(EXCLUDED) if n not in found)
    assert not stale, 'no getenv() of %s is left in eld_amd/csrc' % stale
    assert all(len(r) > 10 for r in EXCLUDED.values())


def test_a_new_switch_is_noticed(tmp_path):
    """the scan on a copy of one source with one more getenv: the new name is reported"""
    with open(os.path.join(CSRC, 'conv_x3w.hip')) as fh:
        src = fh.read()
    (tmp_path / 'conv_x3w.hip').write_text(src + '\nstatic const char* e_new = getenv("ELD_SOMETHING_NEW");\n')
    found = switches_read(str(tmp_path))
    assert 'ELD_X3W' in found
    assert uncovered(found, SWITCHES, EXCLUDED) == ['ELD_SOMETHING_NEW']
