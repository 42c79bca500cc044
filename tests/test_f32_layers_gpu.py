"""fp32 conv kernel families pinned to a float64 reference, per layer (checker: oracle/f32_ref.py).

Every fp32 kernel family of the default scheme (eld_conv_fp32_algo 1: three bf16 pieces per operand, six products) runs through the
single-layer entry points at the smallest shape that makes a 256-CU dispatcher choose it; eld_debug_last_conv_kernel() names the family
and each case asserts the name.  Outputs are compared element by element, on the GPU in float64, with the float64 layer of the very fp32
operands the kernel read: |got - y64| <= x3_bound (oracle/f32_ref.py: accumulation + dropped products, derived; never looser than the
older layer tests' 2e-6 (1 + sum |t|) on zero-mean data).  Each conv case runs on zero-mean data and on the exposure operands (all terms of
one sign, all three pieces of every operand non-zero: the loss of any one of the six piece products is larger than the bound, see the CPU
proof in tests/test_f32_ref_cpu.py), both with exact +0 / -0 sprinkled into the activations.  Weight gradients run twice and must repeat
bit for bit.  The whole fp32 forward is checked teacher-forced: each of the 23 layers against the reference applied to the kernel's own
saved input (eld_debug_unet_region), pools bit for bit, and the families chosen inside it (split-K among them) by launch counts.

The modes read once per process from the environment (ELD_X3W=0 -> "conv_x3<32>/cut", ELD_CONV_TILES -> ".../tiles-f" etc., ELD_NO_SPLITK, ELD_WGRADT8=0, ...)
run these same checks in one fresh interpreter per setting: tests/test_env_variants_gpu.py.  Out of scope: the other fp32 schemes
(tests/test_unet_gpu.py runs them).  The backward's call sites -- every gradient stage of unet_backward<float>, teacher-forced through the gradient
tap, slope and pool codes live and masked -- are in tests/test_backward_layers_gpu.py.

Every buffer of a call lies between guard bands (tests/guarded.py): outputs, gradients and the workspace (exactly the bytes the library asks
for) start as 0xFF bytes -- NaN, which check() rejects, so an element no kernel wrote fails --, operands are guarded copies; after each call
the bands must be intact and the operands the same bits (done()).

F32_MEASURED: worst error as a fraction of its bound per family, one MI355X (this file)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import bf16_ref as R     # noqa: E402  (checker only)
from oracle import f32_ref as F3     # noqa: E402

from guarded import Guards           # noqa: E402

F32_MEASURED = {'conv_x3w': 0.688, 'conv_x3<32>': 0.461, 'conv_x3d<64,8>': 0.824, 'conv_x3d<128,8>': 0.767, 'conv_x3d<64,4>': 0.539,
                'conv_x3_gemm<1x1>': 0.548, 'conv_x3_gemm<gather>': 0.492, 'conv_igemm<f32>': 0.440, 'wgrad8<f32,128x64>': 0.129,
                'wgrad8<f32,64x64>': 0.091, 'wgrad8<f32,64x32>': 0.101, 'wgrad8<f32,32x64>': 0.097, 'wgrad8<f32,32x32>': 0.072, 'wgradt8': 0.144,
                'wgrad<f32>': 0.058, 'wgrad<f32,gather>': 0.100}
# (zero-mean figures; 'unet', the teacher-forced forward under the zero-mean bound, and the weight gradients' exposure cases: not yet measured)
STATS = {}


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    prev = eld_lib.eld_conv_fp32_algo(1)
    yield eld_lib
    eld_lib.eld_conv_fp32_algo(prev)
    print('\nfp32 layers: worst error / bound per family')
    for k in sorted(STATS):
        print('    %-28s %.3f' % (k, STATS[k]))


def Lb():
    from eld_amd import _lib
    return _lib


def dp(t):
    return Lb().dptr(t)


def ws_for(lib, gd, N, H, W, Cin, Cout):
    """the layer workspace at exactly the size the library asks for, between guard bands, every byte 0xFF"""
    n = lib.eld_layer_workspace_bytes(N, H, W, Cin, Cout)
    assert n > 0
    return gd.new((n,), torch.uint8, 'layer workspace')


def done(gd):
    """after a call, before the numeric check: nothing outside any buffer was written, no operand the kernels only read has changed"""
    torch.cuda.synchronize()
    gd.check()


def family(lib):
    return lib.eld_debug_last_conv_kernel().decode()


def check(got, y, bound, fam, what=''):
    """an element passes only if err <= bound is true: a NaN in got (an element no kernel wrote: the outputs start as NaN) fails, and so does a
    worst ratio that is NaN (recorded as inf: max() would drop it)"""
    err = (got.double() - y).abs()
    r = float((err / bound.clamp_min(1e-300)).max())
    r = r if r == r else float('inf')
    STATS[fam] = max(STATS.get(fam, 0.0), r)
    print('%s %s: worst error / bound %.3f' % (fam, what, r))
    bad = ~(err <= bound)
    assert not bool(bad.any()), '%s %s: %d of %d elements outside the bound (%d of them NaN), worst %.3f of it, first at %s' % (
        fam, what, int(bad.sum()), bad.numel(), int(torch.isnan(got).sum()), r, tuple(bad.nonzero()[0].tolist()))
    assert r != float('inf'), '%s %s: the worst error / bound is not a number' % (fam, what)


def sprinkle(t):
    t.view(-1)[::13] = 0.0
    t.view(-1)[5::29] = -0.0
    return t


def operands(kind, ashape, wshape, K, g):
    """activations (exact zeros sprinkled in) and weights, fp32 on the GPU; K = products per output."""
    if kind == 'exposure':
        a = F3.exposure_operands(ashape, g)
        w = F3.exposure_operands(wshape, g, 2.0 ** -int(K).bit_length())
    else:
        a = torch.randn(*ashape, generator=g)
        w = torch.randn(*wshape, generator=g) / np.sqrt(K)
    return sprinkle(a).cuda(), w.cuda()


def bound_of(op, a, w, K, kind, bias=None):
    """(exact sum, x3_bound) of the layer function op(a, w) on float64 tensors."""
    s = op(a, w)
    return s, F3.x3_bound(op(a * a, w * w), K, op(a.abs(), w.abs()), bias, s if kind == 'exposure' else None,
                          absorb=kind == 'exposure' and K > F3.EXPOSURE_MAX_K)


KINDS = ['random', 'exposure']

# ---- 3x3 convolutions ---------------------------------------------------------------------------------------------------
FWD = [  # family, N, H, W, C0, C1, Cout    (256 CUs decide which launches fill the machine)
    ('conv_x3w', 2, 135, 470, 32, 0, 32),            # 270 tiles of 16 x 32: odd height, ragged last tile row and column, the seam between the images
    ('conv_x3w', 2, 136, 470, 32, 32, 32),
    ('conv_x3w', 2, 136, 470, 64, 0, 32),
    ('conv_x3d<64,8>', 2, 166, 420, 32, 0, 64),
    ('conv_x3d<64,8>', 2, 166, 420, 64, 0, 64),
    ('conv_x3d<64,8>', 2, 100, 350, 64, 64, 128),
    ('conv_x3d<128,8>', 2, 100, 350, 128, 0, 256),
    ('conv_x3d<64,4>', 3, 9, 21, 64, 0, 64),
    ('conv_x3d<64,4>', 1, 6, 10, 256, 256, 256),
    ('conv_x3<32>', 3, 9, 21, 32, 0, 32),
    ('conv_x3<32>', 2, 13, 27, 32, 32, 32),
]


@pytest.mark.parametrize('fam,N,H,W,C0,C1,Cout', FWD)
@pytest.mark.parametrize('act', [1, 0])
@pytest.mark.parametrize('kind', KINDS)
def test_conv3x3_forward_f32(lib, fam, N, H, W, C0, C1, Cout, act, kind):
    g = torch.Generator().manual_seed(N * H * W + C0 + 7 * C1 + Cout + act)
    Cin = C0 + C1
    x, w = operands(kind, (N, H, W, Cin), (Cout, Cin, 3, 3), 9 * Cin, g)
    gd = Guards()
    w, b = gd.ro(w, 'w'), gd.ro((0.5 * torch.randn(Cout, generator=g)).cuda(), 'b')
    x0 = gd.ro(x[..., :C0].contiguous(), 'x0')
    x1 = gd.ro(x[..., C0:].contiguous(), 'x1') if C1 else None
    out = gd.new((N, H, W, Cout), name='out')                   # (NaN everywhere: an element the kernel does not write fails the check)
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    Lb().check(lib.eld_conv3x3_forward(dp(x0), C0, dp(x1), C1, dp(w), dp(b), dp(out), N, H, W, Cout, act, dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    assert family(lib) == fam
    s, m = bound_of(R.conv3x3, x.double(), w.double(), 9 * Cin, kind, b)
    y = s + b.double()
    y, m = R.lrelu_ref(y, m) if act else (y, m)
    check(out, y, m, fam, 'forward %s' % kind)


BWD = [  # family, N, H, W, Cin, Cout, split
    ('conv_x3w', 2, 136, 470, 32, 32, 32),
    ('conv_x3w', 2, 136, 470, 32, 64, 32),
    ('conv_x3d<64,8>', 2, 166, 420, 64, 64, 64),
    ('conv_x3d<64,8>', 2, 100, 350, 128, 64, 64),      # two outputs, the second half without slope
    ('conv_x3d<128,8>', 2, 100, 350, 256, 128, 256),
    ('conv_x3d<64,4>', 3, 9, 21, 64, 64, 64),
    ('conv_x3<32>', 3, 9, 21, 32, 32, 32),
    ('conv_x3d<64,4>', 1, 6, 18, 256, 512, 256),
]


@pytest.mark.parametrize('fam,N,H,W,Cin,Cout,split', BWD)
@pytest.mark.parametrize('kind', KINDS)
def test_conv3x3_backward_data_f32(lib, fam, N, H, W, Cin, Cout, split, kind):
    g = torch.Generator().manual_seed(3 * N * H * W + Cin + Cout + split)
    gy, w = operands(kind, (N, H, W, Cout), (Cout, Cin, 3, 3), 9 * Cout, g)
    gd = Guards()
    gy, w = gd.ro(gy, 'gy'), gd.ro(w, 'w')
    act = gd.ro(sprinkle(torch.randn(N, H, W, split, generator=g)).cuda(), 'act')
    d0 = gd.new((N, H, W, split), name='d0')
    d1 = gd.new((N, H, W, Cin - split), name='d1') if split < Cin else None
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    Lb().check(lib.eld_conv3x3_backward_data(dp(gy), dp(w), dp(d0), dp(d1), split, dp(act), None, N, H, W, Cin, Cout,
                                             dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    assert family(lib) == fam
    y, m = bound_of(R.conv3x3_bwd_data, gy.double(), w.double(), 9 * Cout, kind)
    y0, m0 = R.scale_ref(y[..., :split], m[..., :split], R.slope(act.double()))
    check(d0, y0, m0, fam, 'backward-data %s' % kind)
    if d1 is not None:
        check(d1, y[..., split:], m[..., split:], fam, 'backward-data %s (second tensor)' % kind)


WG = [  # family, N, H, W, C0, C1, Cout: each wgrad8 block shape (output x input channels) at a small ragged shape and at its psplit cap 256 / groups
    ('wgrad8<f32,32x32>', 3, 9, 21, 32, 0, 32),
    ('wgrad8<f32,32x32>', 2, 166, 420, 32, 0, 32),       # one group: psplit = 256
    ('wgrad8<f32,32x64>', 3, 9, 21, 32, 32, 32),
    ('wgrad8<f32,32x64>', 2, 166, 420, 32, 32, 32),      # one group: psplit = 256
    ('wgrad8<f32,64x32>', 3, 9, 21, 32, 0, 64),          # conv2_1
    ('wgrad8<f32,64x32>', 2, 166, 420, 32, 0, 64),       # one group: psplit = 256
    ('wgrad8<f32,64x64>', 3, 9, 21, 64, 0, 64),
    ('wgrad8<f32,64x64>', 2, 166, 420, 64, 0, 64),       # one group: psplit = 256
    ('wgrad8<f32,128x64>', 3, 9, 21, 128, 0, 256),
    ('wgrad8<f32,128x64>', 2, 46, 90, 128, 0, 256),      # four groups, 12 x 12 tiles of 8 x 8: psplit = 64
    ('wgrad<f32>', 1, 21, 70, 16, 0, 32),
]


def wg_bounds(kind, K, y, mag2, mag1):
    return F3.x3_bound(mag2, K, mag1, None, y if kind == 'exposure' else None)


def db_bound(kind, K, y, mag2, mag1):
    """bias gradient = a plain fp32 sum of K terms: f32_bound; same-sign terms add the drift of K roundings (oracle/f32_ref.py, n = K)."""
    if kind != 'exposure':
        return R.f32_bound(mag2, K, mag1)
    return R.margin(mag2, K) + R.C_ACC * R.U32 * (K ** 0.5 / 3.0) * y.abs()


# exposure operands where they separate the piece products (K = N H W <= EXPOSURE_MAX_K): every block shape's own six-product loop at its ragged shape
WGK = [c + (kind,) for c in WG for kind in KINDS if kind == 'random' or c[1] * c[2] * c[3] <= F3.EXPOSURE_MAX_K]


@pytest.mark.parametrize('fam,N,H,W,C0,C1,Cout,kind', WGK)
def test_conv3x3_backward_weight_f32(lib, fam, N, H, W, C0, C1, Cout, kind):
    g = torch.Generator().manual_seed(5 * N * H * W + C0 + C1 + Cout)
    Cin = C0 + C1
    K = N * H * W
    if kind == 'exposure':
        x, gy = operands(kind, (N, H, W, Cin), (N, H, W, Cout), K, g)
    else:
        gy = sprinkle(torch.randn(N, H, W, Cout, generator=g)).cuda()
        x = sprinkle(torch.randn(N, H, W, Cin, generator=g)).cuda()
    gd = Guards()
    gy = gd.ro(gy, 'gy')
    x0 = gd.ro(x[..., :C0].contiguous(), 'x0')
    x1 = gd.ro(x[..., C0:].contiguous(), 'x1') if C1 else None
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    res = []
    for _ in range(2):                  # fixed reduction order, no atomics: the same bits twice (the second time from a used workspace)
        dw = gd.new((Cout, Cin, 3, 3), name='dw')
        db = gd.new((Cout,), name='db')
        Lb().check(lib.eld_conv3x3_backward_weight(dp(gy), dp(x0), C0, dp(x1), C1, dp(dw), dp(db), N, H, W, Cout, dp(ws), ws.numel(),
                                                   Lb().cur_stream()))
        done(gd)
        assert family(lib) == fam
        res.append((dw, db))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    gd, xd = gy.double(), x.double()
    y = R.conv3x3_wgrad(gd, xd)
    check(dw, y, wg_bounds(kind, K, y, R.conv3x3_wgrad(gd * gd, xd * xd), R.conv3x3_wgrad(gd.abs(), xd.abs())), fam, 'dW %s' % kind)
    dims = (0, 1, 2)
    check(db, gd.sum(dims), db_bound(kind, K, gd.sum(dims), (gd * gd).sum(dims), gd.abs().sum(dims)), fam, 'db %s' % kind)


# ---- transposed convolutions --------------------------------------------------------------------------------------------
CT = [  # forward, backward-data and weight-gradient family (None: the entry point does not take the shape), N, H, W (input resolution), Cin, Cout
    ('conv_x3_gemm<1x1>', 'conv_x3_gemm<gather>', 'wgradt8', 2, 45, 67, 128, 64),
    ('conv_x3_gemm<1x1>', 'conv_x3_gemm<gather>', 'wgradt8', 1, 22, 33, 512, 256),
    ('conv_x3_gemm<1x1>', 'conv_x3_gemm<gather>', 'wgrad<f32,gather>', 2, 10, 19, 64, 32),
    # shapes the pixel GEMM does not tile (GEMM N not a multiple of 64): the fp32-MFMA kernel, named only once the GEMM launcher has declined
    # (Cout below 32 forward: the GEMM epilogue needs whole 32-channel blocks per tap -- this case found it writing to the wrong tap)
    ('conv_igemm<f32>', 'conv_igemm<f32>', 'wgrad<f32,gather>', 2, 10, 19, 32, 16),
    ('conv_igemm<f32>', None, None, 2, 10, 19, 64, 8),
]


@pytest.mark.parametrize('ffam,bfam,wfam,N,H,W,Cin,Cout', CT)
@pytest.mark.parametrize('kind', KINDS)
def test_convt2x2_f32(lib, ffam, bfam, wfam, N, H, W, Cin, Cout, kind):
    g = torch.Generator().manual_seed(7 * N * H * W + Cin)
    x, w = operands(kind, (N, H, W, Cin), (Cin, Cout, 2, 2), Cin, g)
    gd = Guards()
    x, w, b = gd.ro(x, 'x'), gd.ro(w, 'w'), gd.ro((0.5 * torch.randn(Cout, generator=g)).cuda(), 'b')
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    st = Lb().cur_stream()
    out = gd.new((N, 2 * H, 2 * W, Cout), name='out')
    Lb().check(lib.eld_convt2x2_forward(dp(x), dp(w), dp(b), dp(out), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == ffam
    s, m = bound_of(R.convt_fwd, x.double(), w.double(), Cin, kind, b)
    check(out, s + b.double(), m, ffam, 'convT forward %s' % kind)
    if bfam is None:
        return
    d, w2 = operands(kind, (N, 2 * H, 2 * W, Cout), (Cin, Cout, 2, 2), 4 * Cout, g)
    d, w2 = gd.ro(d, 'd'), gd.ro(w2, 'w2')
    din = gd.new((N, H, W, Cin), name='din')
    Lb().check(lib.eld_convt2x2_backward_data(dp(d), dp(w2), dp(x), dp(din), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == bfam
    y, m = bound_of(R.convt_bwd_data, d.double(), w2.double(), 4 * Cout, kind)
    check(din, *R.scale_ref(y, m, R.slope(x.double())), bfam, 'convT backward-data %s' % kind)
    K = N * H * W
    if kind == 'exposure':
        if K > F3.EXPOSURE_MAX_K:                     # (2, 45, 67): the exposure operands no longer separate the piece products; zero-mean data only
            return
        d = gd.ro(F3.exposure_operands((N, 2 * H, 2 * W, Cout), g, 2.0 ** -K.bit_length()).cuda(), 'd (exposure)')
    res = []
    for _ in range(2):
        dw = gd.new((Cin, Cout, 2, 2), name='dw')
        dbias = gd.new((Cout,), name='dbias')
        Lb().check(lib.eld_convt2x2_backward_weight(dp(x), dp(d), dp(dw), dp(dbias), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
        done(gd)
        assert family(lib) == wfam
        res.append((dw, dbias))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    xd, dd = x.double(), d.double()
    y = R.convt_wgrad(xd, dd)
    check(dw, y, wg_bounds(kind, K, y, R.convt_wgrad(xd * xd, dd * dd), R.convt_wgrad(xd.abs(), dd.abs())), wfam, 'convT dW %s' % kind)
    dims = (0, 1, 2)
    check(dbias, dd.sum(dims), db_bound(kind, 4 * K, dd.sum(dims), (dd * dd).sum(dims), dd.abs().sum(dims)), wfam, 'convT db %s' % kind)


# ---- the whole network, teacher-forced ------------------------------------------------------------------------------------
NET = [(2, 4, 272, 560), (3, 4, 48, 80), (2, 9, 272, 560), (1, 4, 512, 512)]
RG = {'ea': 0, 'eb': 1, 'pool': 2, 'up': 3, 'da': 4, 'db': 5, 'x16': 6}
NAMES = ['conv_x3w', 'conv_x3<32>', 'conv_x3d<128,8>', 'conv_x3d<64,8>', 'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<1x1>',
         'conv_x3_gemm<gather>', 'conv_igemm<f32>', 'conv_igemm<f32,h2>']
# The families a 256-CU dispatcher chooses inside each forward, from its own conditions (conv_x3.hip x3_slab_bn, launch_x3d; conv_x3w.hip x3w_takes):
#   level 0 (32 channels): conv_x3w from 256 tiles of 16 x 32 on (272 x 560 x 2: 612, 512 x 512: 512), else conv_x3<32> (48 x 80 x 3: 27); conv1_1 of
#     4 planes is conv_first (records no name), of 9 planes the NHWC16 copy with Cin = 16, which conv_x3w does not take: conv_x3<32>;
#   levels 1-4: the 8-wave kernels need 256 tiles of 16 rows x Cout / 64 (or / 128) -- the largest here, level 1 of 272 x 560 x 2, has 162: every
#     such layer is on conv_x3d<64,4>, and K is split where 8-row tiles x Cout / 64 leave half the CUs idle and the layer has four chunks or more
#     (levels 3-4 of the large shapes; 48 x 80 x 3: all but conv2_1).  The 8-wave families are pinned by the single-layer cases above only;
#   the four transposed convs have Cout >= 32: conv_x3_gemm<1x1>.
_SMALL = {'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<1x1>'}
RAN = {(2, 4, 272, 560): _SMALL | {'conv_x3w'}, (3, 4, 48, 80): _SMALL | {'conv_x3<32>'}, (2, 9, 272, 560): _SMALL | {'conv_x3w', 'conv_x3<32>'},
       (1, 4, 512, 512): _SMALL | {'conv_x3w'}}

@pytest.mark.parametrize('N,Cin,H,W', NET)
def test_unet_fp32_teacher_forced(lib, N, Cin, H, W):
    """One fp32 forward (eld_unet_forward_ex, precision 0, scheme 1; it keeps every region): each of the 23 layers against the float64 layer
    applied to the kernel's own saved input -- the wiring and the forward's call-site variants (fused pools, pool-code and slope-code
    epilogues, conv_first from NCHW, the NHWC16 input beyond 4 planes, split-K and its finish kernel); pools bit for bit; the head as the
    bf16 file checks it.  The bound is x3_bound as the single-layer zero-mean cases use it: the weights are zero-mean, so the products are,
    whatever the sign of the activations.  The families launched inside the call are read from the launch counters and must be exactly the
    set the dispatcher's conditions give for the shape (RAN)."""
    Cout = Cin
    offs = (C.c_int64 * 47)()
    assert lib.eld_unet_param_offsets(Cin, Cout, offs) == 0
    g = torch.Generator().manual_seed(N * H + Cin)
    prm = torch.empty(offs[46])
    for i in range(23):
        w0, b0, e = offs[2 * i], offs[2 * i + 1], offs[2 * i + 2]
        fan = (b0 - w0) // (e - b0)
        prm[w0:b0] = torch.randn(b0 - w0, generator=g) * np.sqrt(2.0 / fan)
        prm[b0:e] = 0.1 * torch.randn(e - b0, generator=g)
    gd = Guards()
    prm = gd.ro(prm.cuda(), 'prm')
    x = torch.rand(N, Cin, H, W, generator=g)
    x.view(-1)[::17] = 0.0
    x = gd.ro(x.cuda(), 'x')
    nbytes = lib.eld_unet_workspace_bytes(N, H, W, Cin, Cout)
    ws = gd.new((nbytes,), torch.uint8, 'workspace')           # exactly the bytes the library asks for, every one 0xFF
    out = gd.new((N, Cout, H, W), name='out')
    before = {n: lib.eld_debug_conv_kernel_count(n.encode()) for n in NAMES}
    assert 0xFFFFFFFF not in before.values()           # (the counter's table of names is full: its answers are unknown)
    Lb().check(lib.eld_unet_forward_ex(dp(x), dp(prm), dp(out), dp(ws), nbytes, N, H, W, Cin, Cout, 0, 1, Lb().cur_stream()))
    done(gd)
    ran = {n for n in NAMES if lib.eld_debug_conv_kernel_count(n.encode()) > before[n]}
    print('families in the forward of', (N, Cin, H, W), sorted(ran))
    assert ran == RAN[(N, Cin, H, W)]

    def Wt(i, shape):
        return prm[offs[2 * i]:offs[2 * i + 1]].reshape(shape).double()

    def Bs(i):
        return prm[offs[2 * i + 1]:offs[2 * i + 2]]

    def region(name, lev):
        off, ch, dt = C.c_size_t(), C.c_int(), C.c_int()
        Lb().check(lib.eld_debug_unet_region(N, H, W, Cin, Cout, 0, RG[name], lev, C.byref(off), C.byref(ch), C.byref(dt)))
        lv = lev + 1 if name == 'pool' else lev
        h, w_ = H >> lv, W >> lv
        n = N * ch.value * h * w_
        t = ws[off.value:off.value + 4 * n].view(torch.float32)
        if dt.value == 2:
            return t.reshape(N, ch.value, h, w_).permute(0, 2, 3, 1)
        assert dt.value == 0
        return t.reshape(N, h, w_, ch.value)

    def chan(l):
        return 32 << l

    def conv_chk(got, src, i, shape, what):
        wd, xd = Wt(i, shape), src.double()
        K = 9 * shape[1]
        s = R.conv3x3(xd, wd)
        m = F3.x3_bound(R.conv3x3(xd * xd, wd * wd), K, R.conv3x3(xd.abs(), wd.abs()), Bs(i))
        check(got, *R.lrelu_ref(s + Bs(i).double(), m), 'unet', what)

    x16 = region('x16', 0)
    if Cin <= 4:
        assert torch.equal(x16, x.permute(0, 2, 3, 1))
        conv_chk(region('ea', 0), x16, 0, (32, Cin, 3, 3), 'conv1_1 (conv_first)')
    else:
        assert torch.equal(x16[..., :Cin], x.permute(0, 2, 3, 1)) and not bool(x16[..., Cin:].any())
        conv_chk(region('ea', 0), x16[..., :Cin], 0, (32, Cin, 3, 3), 'conv1_1 (NHWC16)')
    for l in range(5):
        if l:
            conv_chk(region('ea', l), region('pool', l - 1), 2 * l, (chan(l), chan(l - 1), 3, 3), 'conv%d_1' % (l + 1))
        eb = region('eb', l)
        conv_chk(eb, region('ea', l), 2 * l + 1, (chan(l), chan(l), 3, 3), 'conv%d_2' % (l + 1))
        if l < 4:
            assert torch.equal(region('pool', l), R.maxpool_fwd(eb)), 'pool%d' % (l + 1)
    for l in range(3, -1, -1):
        iu = 10 + 3 * (3 - l)
        src = (region('eb', 4) if l == 3 else region('db', l + 1)).double()
        wu = Wt(iu, (chan(l + 1), chan(l), 2, 2))
        s = R.convt_fwd(src, wu)
        m = F3.x3_bound(R.convt_fwd(src * src, wu * wu), chan(l + 1), R.convt_fwd(src.abs(), wu.abs()), Bs(iu))
        check(region('up', l), s + Bs(iu).double(), m, 'unet', 'upv%d' % (9 - l))
        cat = torch.cat([region('up', l), region('eb', l)], dim=3)
        conv_chk(region('da', l), cat, iu + 1, (chan(l), 2 * chan(l), 3, 3), 'conv%d_1' % (9 - l))
        conv_chk(region('db', l), region('da', l), iu + 2, (chan(l), chan(l), 3, 3), 'conv%d_2' % (9 - l))
    db0 = region('db', 0).double()
    wh_ = Wt(22, (Cout, 32))
    yo = torch.einsum('nyxc,oc->noyx', db0, wh_) + Bs(22).double()[None, :, None, None]
    bo = R.f32_bound(torch.einsum('nyxc,oc->noyx', db0 * db0, wh_ * wh_), 32) + R.C_ACC * R.U32 * (yo.abs() + Bs(22).double().abs()[None, :, None, None])
    check(out, yo, bo, 'unet', 'head output')
