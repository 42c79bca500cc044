"""Every kernel variant that an environment switch selects, against the float64 reference of its default (the switch table).

eld_amd/csrc reads its ELD_* switches once per process, so each setting runs in a fresh interpreter: tests/variant_child.py <case>, started with the
case's environment the way tests/test_placement_gpu.py starts its children.  The child calls the per-layer checks of tests/test_f32_layers_gpu.py and
tests/test_bf16_layers_gpu.py with the rows of their tables that the switch affects: the same operands, the same float64 layer, the same derived bound
(oracle/f32_ref.py x3_bound, oracle/bf16_ref.py margin / f32_bound) as the default family has to meet.  Nothing is compared with a tolerance of this
file's own.  A variant also has to prove that it ran: the launchers record "family/suffix" for every non-default instantiation or tile setting
(csrc/common.h eld_note_conv_variant) and the checks assert that name.  The table of cases is variant_child.CASES; tests/test_env_variants_cpu.py keeps it complete.

ELD_CONV_TILES: a tile's result does not depend on the tile's shape, so every convolution output under f / p / m16 / m36 / q8 / t must also equal the
default's bit for bit (SHA-256 of the output tensors, exchanged through the children's RESULT lines).

Trouble ends the module: children run one at a time under a 600 s limit; once one ends by a signal, an abort or the limit, every remaining case
fails at once without starting another process.

VARIANT_MEASURED: worst error as a fraction of its bound per (case, recorded name), one MI355X (this file); bf16 outputs ('flip'): the largest
near-tie flip rate as a fraction of test_bf16_layers_gpu.FLIP_MAX.  The bounds are the criterion, not these figures.  In that run every case passed and all
six ELD_CONV_TILES settings gave the default's bits; the products are exact and the order of accumulation per output is the family's, so most figures equal
the default's (tests/test_f32_layers_gpu.py F32_MEASURED)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from variant_child import CASES, SWITCHES, TILE_SETTINGS      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, 'tests', 'variant_child.py')

VARIANT_MEASURED = {
    ('first-mma0', 'unet'): 0.557,
    ('first-mma0', 'unet<bf16>'): 0.286,
    ('first-mma0', 'unet<bf16>', 'flip'): 0.445,
    ('nosplitk', 'unet'): 0.907,
    ('tiles-default', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-default', 'conv_bfd<64>', 'flip'): 0.128,
    ('tiles-default', 'conv_x3d<128,8>'): 0.767,
    ('tiles-default', 'conv_x3d<64,4>'): 0.539,
    ('tiles-default', 'conv_x3d<64,8>'): 0.824,
    ('tiles-f', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-f', 'conv_bfd<128>/tiles-f', 'flip'): 0.121,
    ('tiles-f', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-f', 'conv_bfd<64>/tiles-f', 'flip'): 0.128,
    ('tiles-f', 'conv_x3d<128,8>/tiles-f'): 0.767,
    ('tiles-f', 'conv_x3d<64,4>/tiles-f'): 0.539,
    ('tiles-f', 'conv_x3d<64,8>/tiles-f'): 0.824,
    ('tiles-m16', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-m16', 'conv_bfd<128>/tiles-m', 'flip'): 0.121,
    ('tiles-m16', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-m16', 'conv_bfd<64>/tiles-m', 'flip'): 0.128,
    ('tiles-m16', 'conv_x3d<128,8>/tiles-m'): 0.767,
    ('tiles-m16', 'conv_x3d<64,4>/tiles-m'): 0.539,
    ('tiles-m16', 'conv_x3d<64,8>/tiles-m'): 0.824,
    ('tiles-m36', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-m36', 'conv_bfd<128>/tiles-m', 'flip'): 0.121,
    ('tiles-m36', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-m36', 'conv_bfd<64>/tiles-m', 'flip'): 0.128,
    ('tiles-m36', 'conv_x3d<128,8>/tiles-m'): 0.767,
    ('tiles-m36', 'conv_x3d<64,4>/tiles-m'): 0.539,
    ('tiles-m36', 'conv_x3d<64,8>/tiles-m'): 0.824,
    ('tiles-p', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-p', 'conv_bfd<128>/tiles-p', 'flip'): 0.121,
    ('tiles-p', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-p', 'conv_bfd<64>/tiles-p', 'flip'): 0.128,
    ('tiles-p', 'conv_x3d<128,8>/tiles-p'): 0.767,
    ('tiles-p', 'conv_x3d<64,4>/tiles-p'): 0.539,
    ('tiles-p', 'conv_x3d<64,8>/tiles-p'): 0.824,
    ('tiles-q8', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-q8', 'conv_bfd<128>/tiles-q', 'flip'): 0.121,
    ('tiles-q8', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-q8', 'conv_bfd<64>/tiles-q', 'flip'): 0.128,
    ('tiles-q8', 'conv_x3d<128,8>/tiles-q'): 0.767,
    ('tiles-q8', 'conv_x3d<64,4>/tiles-q'): 0.539,
    ('tiles-q8', 'conv_x3d<64,8>/tiles-q'): 0.824,
    ('tiles-t', 'conv_bfd<128>', 'flip'): 0.121,
    ('tiles-t', 'conv_bfd<128>/tiles-t', 'flip'): 0.121,
    ('tiles-t', 'conv_bfd<64>', 'flip'): 0.121,
    ('tiles-t', 'conv_bfd<64>/tiles-t', 'flip'): 0.128,
    ('tiles-t', 'conv_x3d<128,8>/tiles-t'): 0.767,
    ('tiles-t', 'conv_x3d<64,4>/tiles-t'): 0.539,
    ('tiles-t', 'conv_x3d<64,8>/tiles-t'): 0.824,
    ('wgrad', 'conv_bfg<128>', 'flip'): 0.058,
    ('wgrad', 'conv_igemm<bf16,1x1>', 'flip'): 0.196,
    ('wgrad', 'conv_x3_gemm<1x1>'): 0.548,
    ('wgrad', 'conv_x3_gemm<gather>'): 0.492,
    ('wgrad', 'wgrad8<bf16>'): 0.066,
    ('wgrad', 'wgrad<bf16,gather>/f32mma'): 0.143,
    ('wgrad', 'wgrad<f32,gather>'): 0.126,
    ('x3w0', 'conv_x3<32>/cut'): 0.688,
}

_RESULTS = {}
_DEAD = []           # the first child that ended by a signal, an abort or the time limit: nothing is started after it


def _run(case):
    if case in _RESULTS:
        return _RESULTS[case]
    if _DEAD:
        pytest.fail('not started: the child of case %r ended by %s' % tuple(_DEAD[0]))
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(CASES[case]['env'])
    try:
        r = subprocess.run([sys.executable, CHILD, case], env=e, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _DEAD.append((case, 'the 600 s limit'))
        raise
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _DEAD.append((case, 'status %d' % r.returncode))
    lines = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    res = json.loads(lines[-1][7:]) if lines else {'failed': ['no RESULT line'], 'hash': {}}
    res['status'] = r.returncode
    res['tail'] = '' if r.returncode == 0 and lines else 'case %s, status %d\n%s\n%s' % (case, r.returncode, r.stdout[-6000:], r.stderr[-3000:])
    _RESULTS[case] = res          # (a failed child is not started a second time either)
    return res


@pytest.mark.parametrize('case', sorted(CASES))
def test_variant_meets_the_bound_of_its_default_family(eld_lib, case):
    res = _run(case)
    assert res['status'] == 0 and not res['failed'], res['tail']
    print('\n%s  %s' % (case, ' '.join('%s=%s' % kv for kv in sorted(CASES[case]['env'].items())) or '(no switch set)'))
    for n, c in sorted(res['count'].items()):
        print('    %-40s %4d launches' % (n, c))
        assert c > 0, n
    from test_bf16_layers_gpu import FLIP_MAX
    for n, v in sorted(res['ratio'].items()):
        print("    ('%s', '%s'): %.3f," % (case, n, v))
    for n, v in sorted(res['flip'].items()):
        print("    ('%s', '%s', 'flip'): %.3f," % (case, n, v / FLIP_MAX))
    if 'algo' in res:
        print('    eld_conv_fp32_algo(-1) = %d' % res['algo'])


@pytest.mark.parametrize('setting', TILE_SETTINGS)
def test_conv_tiles_change_no_bit(eld_lib, setting):
    a, b = _run('tiles-default'), _run('tiles-' + setting)
    assert a['status'] == 0 and b['status'] == 0, a['tail'] + b['tail']
    assert sorted(a['hash']) == sorted(b['hash']) and a['hash']
    differ = [k for k in sorted(a['hash']) if a['hash'][k] != b['hash'][k] or not a['hash'][k]]
    assert not differ, differ
