"""One interpreter per setting of the kernel switches that eld_amd/csrc reads once per process (tests/test_env_variants_gpu.py starts it; not collected).

    python tests/variant_child.py <case-id>          with the case's environment (CASES[case-id]['env']) already set

The child loads the library and calls the existing per-layer checks of tests/test_f32_layers_gpu.py and tests/test_bf16_layers_gpu.py as plain
functions, with the rows of their shape tables that the setting affects and the family name the variant must record (csrc/common.h
eld_note_conv_variant: "family/suffix" for every non-default instantiation).  Operands, float64 references and bounds are those modules' own; nothing
is compared here.  It prints one line `RESULT {json}`: per recorded name the worst error as a fraction of its bound (the modules' STATS), the
launch counts of the names it expected, and for the tile-shape cases a hash of every convolution output.  Exit status 0: every check passed.

CASES is the table both sides read.  A run is (op, row):
    f32_fwd / f32_bwd / f32_wg / f32_ct       a row of FWD / BWD / WG / CT of test_f32_layers_gpu.py with the expected names in place of the default's
    bf16_fwd / bf16_bwd / bf16_wg / bf16_ct   the same for test_bf16_layers_gpu.py (bf16_fwd rows carry the activation flag: launches that fuse the pool keep
                                              the standard tile; bf16_ct rows carry the weight gradient's expected name)
    bf16_net_uncut                            bf16_net with conv1_1's reference on the uncut fp32 operands (ELD_FIRST_MMA=0: see main)
    f32_net / bf16_net                        the teacher-forced forward (and bf16 backward) of one shape; f32_net carries the family set of the forward
    step                                      test_unet_gpu.py test_unet_all_gradients_vs_oracle: one fp32 step against oracle.unet_ref.loss_and_grads
    codes                                     test_unet_gpu.py test_slope_codes_give_the_gradients_of_the_saved_activations_bit_for_bit
    algo                                      eld_conv_fp32_algo(-1) must answer the value; no kernel runs"""
import hashlib
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

# ---- the settings: case -> environment.  Plain data, readable without torch (tests/test_env_variants_cpu.py reads it) -------------------------------
ENV = {
    'x3w0': {'ELD_X3W': '0'}, 'nosplitk': {'ELD_NO_SPLITK': '1'},
    'tiles-default': {}, 'tiles-f': {'ELD_CONV_TILES': 'f'}, 'tiles-p': {'ELD_CONV_TILES': 'p'}, 'tiles-m16': {'ELD_CONV_TILES': 'm16'},
    'tiles-m36': {'ELD_CONV_TILES': 'm36'}, 'tiles-q8': {'ELD_CONV_TILES': 'q8'}, 'tiles-t': {'ELD_CONV_TILES': 't'},
    'wgrad': {'ELD_WGRADT8': '0', 'ELD_WGRAD_DMA': '0', 'ELD_WGRAD_BF16_MMA': '0'},
    'first-mma0': {'ELD_FIRST_MMA': '0'}, 'fp32conv-unset': {}, 'fp32conv-m': {'ELD_FP32_CONV': 'm'}, 'fp32conv-h': {'ELD_FP32_CONV': 'h'},
}
SWITCHES = sorted({k for e in ENV.values() for k in e})
TILE_SETTINGS = ['f', 'p', 'm16', 'm36', 'q8', 't']      # m16 chooses the default's shape at every pinned row (it shows the switch is read); m36 gives 14 x 36 tiles at 2 x 166 x 420

# ---- rows of the existing tables (copied by value: the modules are the source; they need torch) ---------------------------------------------
import test_bf16_layers_gpu as B     # noqa: E402
import test_f32_layers_gpu as F      # noqa: E402

X3W, X32, D64, D128, D64S = 'conv_x3w', 'conv_x3<32>', 'conv_x3d<64,8>', 'conv_x3d<128,8>', 'conv_x3d<64,4>'


def _f32(table, op, names):
    """rows of FWD / BWD / WG whose default family is a key of names, under the name the variant records"""
    return [(op, (names[r[0]],) + tuple(r[1:])) for r in table if r[0] in names]


def _x3(names):
    return _f32(F.FWD, 'f32_fwd', names) + _f32(F.BWD, 'f32_bwd', names)


def _tiles(sfx):
    """ELD_CONV_TILES: every conv_x3d row of the fp32 tables and every conv_bfd row of the bf16 tables (sfx '': the default's own names)."""
    runs = _x3({k: k + sfx for k in (D64, D128, D64S)})
    for r in B.FWD:
        if r[0].startswith('conv_bfd'):
            runs.append(('bf16_fwd', (r[0],) + tuple(r[1:]) + (1,)))                # the fused pool keeps 16 x 32 tiles: the default's name
            runs.append(('bf16_fwd', (r[0] + sfx,) + tuple(r[1:]) + (0,)))
    runs += [('bf16_bwd', (r[0] + sfx,) + tuple(r[1:])) for r in B.BWD if r[0].startswith('conv_bfd')]
    return runs


NET_SMALL = (3, 4, 48, 80)
NOSPLIT = {'conv_x3d<64,4>', 'conv_x3_gemm<1x1>'}

CASES = {
    # conv_x3w.hip: 0 hands the layers to conv_x3_kernel<32, 4> on fp32 packed weights cut per stage (the cut-fed instantiation's coverage)
    'x3w0': {'env': {'ELD_X3W': '0'}, 'runs': _x3({X3W: X32 + '/cut', X32: X32 + '/cut'})},
    # conv_x3.hip launch_x3d: the 4-wave kernel without the K split
    'nosplitk': {'env': {'ELD_NO_SPLITK': '1'},
                 'runs': [('f32_net', NET_SMALL + (NOSPLIT | {X32},)), ('f32_net', (1, 4, 512, 512, NOSPLIT | {X3W})),      # every shape of F.RAN records the split by default
                          ('f32_net', (2, 4, 272, 560, NOSPLIT | {X3W})), ('f32_net', (2, 9, 272, 560, NOSPLIT | {X3W, X32}))]},
    # conv_igemm.hip conv_tile_shape: the default's outputs are hashed too (tests/test_env_variants_gpu.py compares them bit for bit)
    'tiles-default': {'env': {}, 'runs': _tiles(''), 'hash': True},
    'tiles-f': {'env': {'ELD_CONV_TILES': 'f'}, 'runs': _tiles('/tiles-f'), 'hash': True},
    'tiles-p': {'env': {'ELD_CONV_TILES': 'p'}, 'runs': _tiles('/tiles-p'), 'hash': True},
    'tiles-m16': {'env': {'ELD_CONV_TILES': 'm16'}, 'runs': _tiles('/tiles-m'), 'hash': True},
    'tiles-m36': {'env': {'ELD_CONV_TILES': 'm36'}, 'runs': _tiles('/tiles-m'), 'hash': True},
    'tiles-q8': {'env': {'ELD_CONV_TILES': 'q8'}, 'runs': _tiles('/tiles-q'), 'hash': True},
    'tiles-t': {'env': {'ELD_CONV_TILES': 't'}, 'runs': _tiles('/tiles-t'), 'hash': True},
    # conv_wgrad.hip, three disjoint families in one child: the transposed convs' gradient back on wgrad_kernel; the bf16 128 x 64 blocks on the
    # register-staged kernel; the bf16 gather gradient on the fp32 MFMA
    'wgrad': {'env': {'ELD_WGRADT8': '0', 'ELD_WGRAD_DMA': '0', 'ELD_WGRAD_BF16_MMA': '0'},
              'runs': [('f32_ct', tuple(r[:2]) + ('wgrad<f32,gather>',) + tuple(r[3:])) for r in F.CT if r[2] == 'wgradt8']
              + _f32(B.WG, 'bf16_wg', {'wgrad8d': 'wgrad8<bf16>'})
              + [('bf16_ct', tuple(r) + ('wgrad<bf16,gather>/f32mma',)) for r in B.CT]},
    # conv_first.hip: the packed-raw first layer back on the fp32-MFMA kernel, which writes no slope codes (the backward of conv1_2 reads the saved tensor)
    'first-mma0': {'env': {'ELD_FIRST_MMA': '0'},
                   'runs': [('f32_net', NET_SMALL + ({'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<1x1>', X32},)), ('bf16_net_uncut', NET_SMALL),
                            ('step', NET_SMALL), ('codes', ('fp32', (1, 4, 528, 1072))), ('codes', ('bf16', (1, 4, 256, 512)))],
                   'expect': ['conv_first/mma0']},
    # conv_igemm.hip conv_fp32_algo: the process default of the product scheme
    'fp32conv-unset': {'env': {}, 'runs': [('algo', 1)]},
    'fp32conv-m': {'env': {'ELD_FP32_CONV': 'm'}, 'runs': [('algo', 0)]},
    'fp32conv-h': {'env': {'ELD_FP32_CONV': 'h'}, 'runs': [('algo', 2)]},
}
assert {k: c['env'] for k, c in CASES.items()} == ENV


# ---- the child proper -------------------------------------------------------------------------------------------------------------------------
class Handle:
    """The library handle the checks receive: the library's own, plus a record of what eld_debug_last_conv_kernel answered."""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def eld_debug_last_conv_kernel(self):
        raw = self._lib.eld_debug_last_conv_kernel()
        self.seen.append(raw.decode())
        return raw


def _names_of(op, row):
    if op in ('f32_fwd', 'f32_bwd', 'f32_wg', 'bf16_fwd', 'bf16_bwd', 'bf16_wg'):
        return [row[0]]
    if op == 'f32_ct':
        return [n for n in row[:3] if n]
    if op == 'bf16_ct':
        return [row[0], row[1], row[-1]]
    if op == 'f32_net':
        return sorted(row[4])
    return []


def main(case_id):
    case = CASES[case_id]
    for k in SWITCHES:                                   # the setting is exactly the case's: an inherited switch would test something else
        assert os.environ.get(k) == case['env'].get(k), (k, os.environ.get(k))
    import eld_amd
    lib = Handle(eld_amd.load_library())
    out = {'case': case_id, 'ratio': {}, 'flip': {}, 'count': {}, 'hash': {}, 'failed': []}
    if all(op == 'algo' for op, _ in case['runs']):
        for _, want in case['runs']:
            got = lib.eld_conv_fp32_algo(-1)
            out['algo'] = got
            if got != want:
                out['failed'].append('eld_conv_fp32_algo(-1) = %d, expected %d' % (got, want))
        return out
    import torch
    assert torch.cuda.is_available()
    expect = sorted(set(case.get('expect', [])) | {n for op, row in case['runs'] for n in _names_of(op, row)})
    before = {n: lib.eld_debug_conv_kernel_count(n.encode()) for n in expect}
    lib.eld_conv_fp32_algo(1)                            # the scheme test_f32_layers_gpu.py pins (its `lib` fixture)
    hashes = []
    if case.get('hash'):
        def hashed(orig):
            def f(got, *a, **k):
                hashes.append(hashlib.sha256(got.contiguous().cpu().numpy().tobytes()).hexdigest())
                return orig(got, *a, **k)
            return f
        F.check, B.accept = hashed(F.check), hashed(B.accept)

    def note(stats_key, name, store, mod):
        store[name] = max(store.get(name, 0.0), mod.STATS.get(stats_key, 0.0))

    for op, row in case['runs']:
        F.STATS.clear()
        B.STATS.update(flip=0.0, f32=0.0)
        del hashes[:]
        label = '%s %s' % (op, ' '.join(str(v) for v in row))
        try:
            if op == 'f32_fwd':
                for kind in F.KINDS:
                    for act in (1, 0):
                        F.test_conv3x3_forward_f32(lib, *row, act, kind)
            elif op == 'f32_bwd':
                for kind in F.KINDS:
                    F.test_conv3x3_backward_data_f32(lib, *row, kind)
            elif op == 'f32_wg':
                for kind in F.KINDS:
                    if kind == 'random' or row[1] * row[2] * row[3] <= F.F3.EXPOSURE_MAX_K:      # as WGK of the module
                        F.test_conv3x3_backward_weight_f32(lib, *row, kind)
            elif op == 'f32_ct':
                for kind in F.KINDS:
                    F.test_convt2x2_f32(lib, *row, kind)
            elif op == 'f32_net':
                F.RAN[tuple(row[:4])] = set(row[4])
                F.test_unet_fp32_teacher_forced(lib, *row[:4])
            elif op == 'bf16_fwd':
                B.test_conv3x3_forward_bf16(lib, *row)
            elif op == 'bf16_bwd':
                B.test_conv3x3_backward_data_bf16(lib, *row)
            elif op == 'bf16_wg':
                B.test_conv3x3_backward_weight_bf16(lib, *row)
            elif op == 'bf16_ct':
                B.test_convt2x2_bf16(lib, *row)
            elif op == 'bf16_net':
                B.test_unet_bf16_teacher_forced(lib, *row)
            elif op == 'bf16_net_uncut':
                # test_unet_bf16_teacher_forced models conv1_1 of 4 planes as conv_first.hip's bf16-MFMA kernel computes it: operands cut to two
                # truncated bf16 pieces (bf16_ref.first_cut2), three products.  ELD_FIRST_MMA=0 runs the fp32-MFMA kernel on the uncut fp32 operands,
                # so the float64 layer of the operands THAT kernel read is the one with nothing cut: hi = the operand, lo = 0.  The margin stays the
                # check's own, C_ACC 2^-24 sqrt(27 Cin) ||t||_2 over the same squared magnitudes (sqrt(3) above the 9 Cin products this kernel sums:
                # DESIGN.md section 6a); the rounding rule and every other layer are untouched.
                cut2 = B.R.first_cut2
                B.R.first_cut2 = lambda v: (v.double(), torch.zeros_like(v, dtype=torch.float64))
                try:
                    B.test_unet_bf16_teacher_forced(lib, *row)
                finally:
                    B.R.first_cut2 = cut2
            elif op == 'step':
                import test_unet_gpu as T
                T.test_unet_all_gradients_vs_oracle(lib, tuple(row), 1)
            elif op == 'codes':
                import test_unet_gpu as T
                T.test_slope_codes_give_the_gradients_of_the_saved_activations_bit_for_bit(lib, *row)
            else:
                raise ValueError(op)
        except AssertionError:
            out['failed'].append(label + '\n' + traceback.format_exc()[-1500:])
        torch.cuda.synchronize()
        for k in F.STATS:
            note(k, k, out['ratio'], F)
        if op in ('bf16_wg', 'bf16_ct', 'bf16_net', 'bf16_net_uncut'):
            note('f32', row[-1] if op == 'bf16_ct' else ('unet<bf16>' if op.startswith('bf16_net') else row[0]), out['ratio'], B)
        if op in ('bf16_fwd', 'bf16_bwd', 'bf16_ct', 'bf16_net', 'bf16_net_uncut'):
            note('flip', 'unet<bf16>' if op.startswith('bf16_net') else row[0], out['flip'], B)
        if case.get('hash'):
            fam = row[0].split('/')[0]
            out['hash']['%s %s %s' % (op, fam, ' '.join(str(v) for v in row[1:]))] = list(hashes)
    for n in expect:
        c = lib.eld_debug_conv_kernel_count(n.encode())
        out['count'][n] = c - before[n]
        if not (c != 0xFFFFFFFF and c > before[n]):
            out['failed'].append('no launch recorded under %r' % n)
    return out


if __name__ == '__main__':
    res = main(sys.argv[1])
    for f in res['failed']:
        print('FAILED', f)
    print('RESULT ' + json.dumps(res))
    sys.exit(1 if res['failed'] else 0)
