"""bf16 U-Net layers pinned to a float64 reference of their rounding (checker: oracle/bf16_ref.py).

Every bf16 kernel family runs through the single-layer entry points (include/eld_amd.h eld_*_bf16) at a shape that makes the dispatcher
choose it; eld_debug_last_conv_kernel() names the family and each case asserts the name.  Outputs are compared element by element with
float64 values computed from the very bf16 operands the kernel read:
  * bf16 outputs: rne_bf16(y64), or within the fp32 accumulation margin m of the rounding midpoint (bf16_ref.bf16_accept);
  * fp32 outputs (dW, db, the head): |got - y64| <= C_ACC 2^-24 sqrt(K) ||terms||_2 elementwise, never looser than 2e-6 (1 + sum |terms|).
Pools are bit-exact.  The whole network is checked teacher-forced: every layer against the reference applied to the kernel's own saved
inputs (eld_debug_unet_region), so errors cannot compound across layers.  Negative controls (host-side tensors only) show that the rule
rejects truncation, a dropped border / seam row, a bf16-rounded bias, a one-ulp change and a weight gradient without one border row.
Every buffer of a call lies between guard bands (tests/guarded.py): outputs, gradients and the workspace (exactly the bytes the library asks
for) start as 0xFF bytes -- 0xFFFF is a bf16 NaN, which the rounding rule rejects, so an element no kernel wrote fails --, operands are guarded
copies; after each call the bands must be intact and the operands the same bits (done()).

FLIP_MAX bounds the fraction of near-tie flips (accepted elements that are not rne_bf16(y64)) of any one tensor at 3x the largest rate
measured on one MI355X; the measured figures are in FLIP_MEASURED / F32_MEASURED (worst fp32 error as a fraction of its bound)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import bf16_ref as R     # noqa: E402  (checker only)

from guarded import Guards           # noqa: E402

FLIP_MEASURED = 3.9e-4               # largest near-tie flip rate of one tensor, one MI355X (this file)
F32_MEASURED = 0.29                  # worst fp32 error as a fraction of its bound, same run
FLIP_MAX = 3 * FLIP_MEASURED
ELD_ENOTSUP = -2
STATS = {'flip': 0.0, 'f32': 0.0}


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    yield eld_lib
    print('\nbf16 layers: worst near-tie flip rate %.3e, worst fp32 error / bound %.3f' % (STATS['flip'], STATS['f32']))


def Lb():
    from eld_amd import _lib
    return _lib


def dp(t):
    return Lb().dptr(t)


def i16(bits):
    """int32 bit patterns 0..0xFFFF -> contiguous device int16 tensor (what the kernels read)."""
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).contiguous()


def bits(t16):
    return t16.to(torch.int32) & 0xFFFF


def rand_bf16(shape, g, scale=1.0):
    """bf16 values (float64, on the GPU) with exact +0 and -0 sprinkled in (slopes 0.6)."""
    t = torch.randn(*shape, generator=g, dtype=torch.float64) * scale
    t.view(-1)[::13] = 0.0
    t.view(-1)[5::29] = -0.0
    return R.rne_bf16(t).cuda()


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


def accept(got16, y, m, what):
    ok, fl = R.bf16_accept(bits(got16), y, m)
    bad = int((~ok).sum())
    rate = float(fl.sum()) / max(fl.numel(), 1)
    STATS['flip'] = max(STATS['flip'], rate)
    assert bad == 0, '%s: %d of %d elements outside the rounding rule, first at %s' % (what, bad, ok.numel(), tuple((~ok).nonzero()[0].tolist()))
    assert rate <= FLIP_MAX, '%s: near-tie flips %.3e > %.3e' % (what, rate, FLIP_MAX)


def rejects(got_bits, y, m):
    return not bool(R.bf16_accept(got_bits, y, m)[0].all())


def f32_check(got, y, bound, what):
    err = (got.double() - y).abs()
    r = float((err / bound.clamp_min(1e-300)).max())
    STATS['f32'] = max(STATS['f32'], r)
    assert bool((err <= bound).all()), '%s: worst error %.3f of its bound' % (what, r)


def conv_ref(x, w, b, lrelu):
    """exact output of conv3x3 + fp32 bias (+ LeakyReLU) on bf16 operands, with its margin; w: fp32 OIHW (packed as rne_bf16(w))."""
    wb = R.rne_bf16(w.double())
    y = R.conv3x3(x, wb) + b.double()
    m = R.margin(R.conv3x3(x * x, wb * wb), 9 * x.shape[3], b)
    return R.lrelu_ref(y, m) if lrelu else (y, m)


def wgrad_ref(g, x):
    K = g.shape[0] * g.shape[1] * g.shape[2]
    return R.conv3x3_wgrad(g, x), R.f32_bound(R.conv3x3_wgrad(g * g, x * x), K, R.conv3x3_wgrad(g.abs(), x.abs()))


def colsum_ref(g):
    K = g.numel() // g.shape[-1]
    return g.sum(dim=tuple(range(g.dim() - 1))), R.f32_bound((g * g).sum(dim=tuple(range(g.dim() - 1))), K, g.abs().sum(dim=tuple(range(g.dim() - 1))))


# ---- 3x3 convolutions ---------------------------------------------------------------------------------------------------
FWD = [  # family, N, H, W, C0, C1, Cout    (one MI355X: 256 CUs decide which launches fill the machine)
    ('conv_bfs', 2, 166, 420, 32, 0, 32),
    ('conv_bfs', 2, 166, 420, 32, 32, 32),          # the decoder concat (conv9_1)
    ('conv_bfw', 2, 166, 420, 32, 0, 64),
    ('conv_bfw', 2, 166, 420, 64, 0, 64),
    ('conv_bfd<64>', 2, 100, 350, 64, 0, 128),
    ('conv_bfd<64>', 2, 100, 350, 64, 64, 128),
    ('conv_bfd<128>', 2, 100, 350, 128, 0, 256),
    ('conv_igemm<bf16>', 3, 9, 21, 32, 0, 32),      # odd H, W; three images
    ('conv_igemm<bf16>', 2, 13, 27, 32, 32, 64),
    ('conv_igemm<bf16>', 1, 6, 10, 64, 0, 128),
]


@pytest.mark.parametrize('fam,N,H,W,C0,C1,Cout', FWD)
@pytest.mark.parametrize('act', [1, 0])
def test_conv3x3_forward_bf16(lib, fam, N, H, W, C0, C1, Cout, act):
    g = torch.Generator().manual_seed(N * H * W + C0 + 7 * C1 + Cout + act)
    gd = Guards()
    x = rand_bf16((N, H, W, C0 + C1), g)
    w = gd.ro((torch.randn(Cout, C0 + C1, 3, 3, generator=g) / np.sqrt(9 * (C0 + C1))).cuda(), 'w')
    b = gd.ro((0.5 * torch.randn(Cout, generator=g)).cuda(), 'b')
    x0 = gd.ro(i16(R.bits_of(x[..., :C0])), 'x0')
    x1 = gd.ro(i16(R.bits_of(x[..., C0:])), 'x1') if C1 else None
    out = gd.new((N, H, W, Cout), torch.int16, 'out')           # (0xFFFF everywhere, a bf16 NaN: an element the kernel does not write fails the rule)
    fuse = act and fam != 'conv_igemm<bf16>'
    pool = gd.new((N, H // 2, W // 2, Cout), torch.int16, 'pool') if fuse else None
    ws = ws_for(lib, gd, N, H, W, C0 + C1, Cout)
    st = Lb().cur_stream()
    if act and not fuse:       # the generic kernel has no pooled epilogue
        assert lib.eld_conv3x3_forward_bf16(dp(x0), C0, dp(x1), C1, dp(w), dp(b), dp(out), dp(out), N, H, W, Cout, act, dp(ws), ws.numel(), st) == ELD_ENOTSUP
        torch.cuda.synchronize()
        assert bool((out == -1).all())                         # the refused call wrote no output (the workspace is scratch: the weights may be packed by then)
    Lb().check(lib.eld_conv3x3_forward_bf16(dp(x0), C0, dp(x1), C1, dp(w), dp(b), dp(out), dp(pool), N, H, W, Cout, act, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == fam
    y, m = conv_ref(x, w, b, act)
    accept(out, y, m, fam)
    if fuse:
        assert bool((R.f64_of_bits(bits(pool)) == R.maxpool_fwd(R.f64_of_bits(bits(out)))).all())


@pytest.mark.parametrize('fam,N,H,W,C,Cout', [('conv_bfs', 2, 166, 420, 32, 32), ('conv_bfd<128>', 2, 100, 350, 128, 256),
                                               ('conv_bfw', 2, 166, 420, 64, 64), ('conv_igemm<bf16>', 3, 9, 21, 32, 32)])
def test_conv3x3_rounds_exact_ties_to_even(lib, fam, N, H, W, C, Cout):
    """Operands whose partial sums are all exact in fp32 -- inputs (1 + j/128) 2^e with e in {-1, 0, 1}, weights in {0, +-1/2, +-1}, zero
    bias: every sum is a multiple of 2^-9 below 2^12, so the accumulator holds y64 exactly in any order and the output must be rne_bf16(y64)
    bit for bit, exact ties included (truncation or round-half-away fail here)."""
    g = torch.Generator().manual_seed(H + C)
    shape = (N, H, W, C)
    x = ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * (1 + torch.randint(0, 128, shape, generator=g) / 128.0)
         * torch.exp2(torch.randint(-1, 2, shape, generator=g).double())).double()
    x.view(-1)[::11] = 0.0
    x = x.cuda()
    gd = Guards()
    w = gd.ro((torch.randint(-2, 3, (Cout, C, 3, 3), generator=g) / 2.0).float().cuda(), 'w')
    b = gd.ro(torch.zeros(Cout, device='cuda'), 'b')
    out = gd.new((N, H, W, Cout), torch.int16, 'out')
    ws = ws_for(lib, gd, N, H, W, C, Cout)
    x16 = gd.ro(i16(R.bits_of(x)), 'x')
    Lb().check(lib.eld_conv3x3_forward_bf16(dp(x16), C, None, 0, dp(w), dp(b), dp(out), None, N, H, W, Cout, 0, dp(ws), ws.numel(),
                                            Lb().cur_stream()))
    done(gd)
    assert family(lib) == fam
    y = R.conv3x3(x, w.double())
    assert bool((R.f64_of_bits(bits(out)) == R.rne_bf16(y)).all())
    ties = int(((y - R.trunc_bf16(y)).abs() * 2 == R.ulp_bf16(y)).sum())
    assert ties >= 100, ties


BWD = [  # family, N, H, W, Cin, Cout, split, slopes
    ('conv_bfs', 2, 166, 420, 32, 32, 32, True),
    ('conv_bfs', 2, 166, 420, 32, 64, 32, False),
    ('conv_bfw', 2, 166, 420, 64, 32, 32, False),       # the decoder concat: 32 + 32 channels into two tensors
    ('conv_bfw', 2, 166, 420, 64, 64, 64, True),
    ('conv_bfd<64>', 2, 100, 350, 128, 128, 128, True),
    ('conv_bfd<64>', 2, 100, 350, 128, 64, 64, False),
    ('conv_bfd<128>', 2, 100, 350, 256, 128, 256, True),
    ('conv_igemm<bf16>', 3, 9, 21, 32, 32, 32, True),
    ('conv_igemm<bf16>', 2, 13, 27, 64, 32, 32, False),
]


@pytest.mark.parametrize('fam,N,H,W,Cin,Cout,split,slopes', BWD)
def test_conv3x3_backward_data_bf16(lib, fam, N, H, W, Cin, Cout, split, slopes):
    g = torch.Generator().manual_seed(3 * N * H * W + Cin + Cout + split)
    gd = Guards()
    gy = rand_bf16((N, H, W, Cout), g)
    w = gd.ro((torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(9 * Cout)).cuda(), 'w')
    act = rand_bf16((N, H, W, Cin), g)
    d0 = gd.new((N, H, W, split), torch.int16, 'd0')
    d1 = gd.new((N, H, W, Cin - split), torch.int16, 'd1') if split < Cin else None
    a0 = gd.ro(i16(R.bits_of(act[..., :split])), 'act') if slopes else None
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    g16 = gd.ro(i16(R.bits_of(gy)), 'gy')
    Lb().check(lib.eld_conv3x3_backward_data_bf16(dp(g16), dp(w), dp(d0), dp(d1), split, dp(a0), None, N, H, W, Cin, Cout,
                                                  dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    assert family(lib) == fam
    wb = R.rne_bf16(w.double())
    y = R.conv3x3_bwd_data(gy, wb)
    m = R.margin(R.conv3x3_bwd_data(gy * gy, wb * wb), 9 * Cout)
    y0, m0 = (R.scale_ref(y[..., :split], m[..., :split], R.slope(act[..., :split])) if slopes else (y[..., :split], m[..., :split]))
    accept(d0, y0, m0, fam)
    if d1 is not None:
        accept(d1, y[..., split:], m[..., split:], fam + ' (second tensor)')


WG = [  # family, N, H, W, C0, C1, Cout
    ('wgrad8d', 2, 46, 90, 64, 0, 128),
    ('wgrad8d', 2, 23, 45, 64, 64, 128),
    ('wgrad8<bf16>', 2, 166, 420, 32, 0, 32),
    ('wgrad8<bf16>', 2, 37, 61, 32, 32, 32),
    ('wgrad8<bf16>', 1, 20, 40, 32, 0, 64),
    ('wgrad8<bf16>', 3, 9, 21, 64, 0, 64),
]


@pytest.mark.parametrize('fam,N,H,W,C0,C1,Cout', WG)
def test_conv3x3_backward_weight_bf16(lib, fam, N, H, W, C0, C1, Cout):
    g = torch.Generator().manual_seed(5 * N * H * W + C0 + C1 + Cout)
    gy = rand_bf16((N, H, W, Cout), g)
    x = rand_bf16((N, H, W, C0 + C1), g)
    gd = Guards()
    dw = gd.new((Cout, C0 + C1, 3, 3), name='dw')
    db = gd.new((Cout,), name='db')
    ws = ws_for(lib, gd, N, H, W, C0 + C1, Cout)
    g16, x0 = gd.ro(i16(R.bits_of(gy)), 'gy'), gd.ro(i16(R.bits_of(x[..., :C0])), 'x0')
    x1 = gd.ro(i16(R.bits_of(x[..., C0:])), 'x1') if C1 else None
    Lb().check(lib.eld_conv3x3_backward_weight_bf16(dp(g16), dp(x0), C0, dp(x1), C1, dp(dw), dp(db),
                                                    N, H, W, Cout, dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    assert family(lib) == fam
    y, bound = wgrad_ref(gy, x)
    f32_check(dw, y, bound, fam + ' dW')
    yb, bb = colsum_ref(gy)
    f32_check(db, yb, bb, fam + ' db')


# ---- transposed convolutions --------------------------------------------------------------------------------------------
CT = [  # forward family, backward-data family, N, H, W (input resolution), Cin, Cout
    ('conv_bfg<128>', 'conv_bfg<64,gather>', 2, 96, 330, 64, 32),
    ('conv_bfg<128>', 'conv_bfg<128,gather>', 2, 96, 330, 128, 64),
    ('conv_igemm<bf16,1x1>', 'conv_igemm<bf16,gather>', 3, 7, 13, 64, 32),
]


@pytest.mark.parametrize('ffam,bfam,N,H,W,Cin,Cout', CT)
def test_convt2x2_bf16(lib, ffam, bfam, N, H, W, Cin, Cout, wfam='wgrad<bf16,gather>'):      # wfam: tests/variant_child.py passes a variant's name
    g = torch.Generator().manual_seed(7 * N * H * W + Cin)
    gd = Guards()
    x = rand_bf16((N, H, W, Cin), g)
    w = gd.ro((torch.randn(Cin, Cout, 2, 2, generator=g) / np.sqrt(Cin)).cuda(), 'w')
    b = gd.ro((0.5 * torch.randn(Cout, generator=g)).cuda(), 'b')
    wb = R.rne_bf16(w.double())
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    st = Lb().cur_stream()
    xb = gd.ro(i16(R.bits_of(x)), 'x')
    out = gd.new((N, 2 * H, 2 * W, Cout), torch.int16, 'out')
    Lb().check(lib.eld_convt2x2_forward_bf16(dp(xb), dp(w), dp(b), dp(out), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == ffam
    accept(out, R.convt_fwd(x, wb) + b.double(), R.margin(R.convt_fwd(x * x, wb * wb), Cin, b), ffam)
    d = rand_bf16((N, 2 * H, 2 * W, Cout), g)
    db16 = gd.ro(i16(R.bits_of(d)), 'd')
    din = gd.new((N, H, W, Cin), torch.int16, 'din')
    Lb().check(lib.eld_convt2x2_backward_data_bf16(dp(db16), dp(w), dp(xb), dp(din), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == bfam
    y, m = R.scale_ref(R.convt_bwd_data(d, wb), R.margin(R.convt_bwd_data(d * d, wb * wb), 4 * Cout), R.slope(x))
    accept(din, y, m, bfam)
    dw = gd.new((Cin, Cout, 2, 2), name='dw')
    dbias = gd.new((Cout,), name='dbias')
    Lb().check(lib.eld_convt2x2_backward_weight_bf16(dp(xb), dp(db16), dp(dw), dp(dbias), N, H, W, Cin, Cout, dp(ws), ws.numel(), st))
    done(gd)
    assert family(lib) == wfam
    f32_check(dw, R.convt_wgrad(x, d), R.f32_bound(R.convt_wgrad(x * x, d * d), N * H * W, R.convt_wgrad(x.abs(), d.abs())), 'convT dW')
    yb, bb = colsum_ref(d)
    f32_check(dbias, yb, bb, 'convT db')


def test_convt2x2_bias_gradient_by_column_sums_bf16(lib):
    """Cout = 8 is below the weight-gradient kernel's 32-channel block, so the bias gradient is not formed inside that launch: it is the column-sum
    kernel's own output (colsum_kernel<bf16>), which no case above reaches.  The gradients are multiples of 1/16 in [-1, 1] (exact in bf16) and
    there are 64 pixels: every fp32 partial sum is exact in any order, so the result must be the float64 sum, bit for bit."""
    N, H, W, Cin, Cout = 1, 4, 4, 32, 8
    g = torch.Generator().manual_seed(7 * N * H * W + Cin)
    gd = Guards()
    x = rand_bf16((N, H, W, Cin), g)
    d = (torch.randint(-16, 17, (N, 2 * H, 2 * W, Cout), generator=g).double() / 16).cuda()
    assert bool((R.rne_bf16(d) == d).all())
    xb, db16 = gd.ro(i16(R.bits_of(x)), 'x'), gd.ro(i16(R.bits_of(d)), 'd')
    ws = ws_for(lib, gd, N, H, W, Cin, Cout)
    dw = gd.new((Cin, Cout, 2, 2), name='dw')
    dbias = gd.new((Cout,), name='dbias')
    Lb().check(lib.eld_convt2x2_backward_weight_bf16(dp(xb), dp(db16), dp(dw), dp(dbias), N, H, W, Cin, Cout, dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    assert torch.equal(dbias.double(), d.sum((0, 1, 2)))


# ---- pools ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Ho,Wo,C', [(2, 45, 77, 32), (3, 8, 13, 64), (1, 20, 33, 256)])
def test_maxpool2x2_bf16_bit_exact(lib, N, Ho, Wo, C):
    g = torch.Generator().manual_seed(Ho * Wo + C)
    x = rand_bf16((N, 2 * Ho, 2 * Wo, C), g).reshape(N, Ho, 2, Wo, 2, C)
    x[:, ::3, 1, :, 1, :] = x[:, ::3, 0, :, 0, :]           # tied maxima: the first in row-major order takes the gradient
    x[:, 1::4, 1, :, 0, :] = x[:, 1::4, 0, :, 1, :]
    x = x.reshape(N, 2 * Ho, 2 * Wo, C).contiguous()
    gd = Guards()
    xb = gd.ro(i16(R.bits_of(x)), 'x')
    out = gd.new((N, Ho, Wo, C), torch.int16, 'out')
    st = Lb().cur_stream()
    Lb().check(lib.eld_maxpool2x2_forward_bf16(dp(xb), dp(out), N, Ho, Wo, C, st))
    dpool = rand_bf16((N, Ho, Wo, C), g)
    skip = rand_bf16((N, 2 * Ho, 2 * Wo, C), g)
    gs = gd.new((N, 2 * Ho, 2 * Wo, C), torch.int16, 'gs')
    gn = gd.new((N, 2 * Ho, 2 * Wo, C), torch.int16, 'gn')
    p16, s16 = gd.ro(i16(R.bits_of(dpool)), 'dpool'), gd.ro(i16(R.bits_of(skip)), 'skip')
    Lb().check(lib.eld_maxpool2x2_backward_bf16(dp(xb), dp(p16), dp(s16), dp(gs), N, Ho, Wo, C, st))
    Lb().check(lib.eld_maxpool2x2_backward_bf16(dp(xb), dp(p16), None, dp(gn), N, Ho, Wo, C, st))
    done(gd)
    assert bool((R.f64_of_bits(bits(out)) == R.maxpool_fwd(x)).all())
    assert bool((R.f64_of_bits(bits(gs)) == R.rne_bf16(R.maxpool_bwd_f32(x, dpool, skip))).all())
    assert bool((R.f64_of_bits(bits(gn)) == R.rne_bf16(R.maxpool_bwd_f32(x, dpool, None))).all())


# ---- negative controls ----------------------------------------------------------------------------------------------------
def test_negative_controls_are_rejected(lib):
    """The acceptance rule is tight enough to see the defects it exists for (all on host-side copies of one real launch)."""
    N, H, W, C, Cout = 2, 100, 350, 64, 128
    g = torch.Generator().manual_seed(99)
    x = rand_bf16((N, H, W, C), g)
    w = (torch.randn(Cout, C, 3, 3, generator=g) / np.sqrt(9 * C)).cuda()
    b = (0.5 * torch.randn(Cout, generator=g)).cuda()
    gd = Guards()
    w, b = gd.ro(w, 'w'), gd.ro(b, 'b')
    out = gd.new((N, H, W, Cout), torch.int16, 'out')
    ws = ws_for(lib, gd, N, H, W, C, Cout)
    x16 = gd.ro(i16(R.bits_of(x)), 'x')
    Lb().check(lib.eld_conv3x3_forward_bf16(dp(x16), C, None, 0, dp(w), dp(b), dp(out), None, N, H, W, Cout, 1, dp(ws), ws.numel(),
                                            Lb().cur_stream()))
    done(gd)
    got = bits(out)
    y, m = conv_ref(x, w, b, 1)
    assert not rejects(got, y, m)
    assert rejects(R.bits_of(R.trunc_bf16(y)), y, m)                        # a kernel that truncates
    for n, r in [(0, 0), (0, H - 1), (1, 0)]:                               # image border / the seam between the two images of the strip
        xd = x.clone()
        xd[n, r] = 0.0
        assert rejects(got, *conv_ref(xd, w, b, 1)), (n, r)
    assert rejects(got, *conv_ref(x, w, R.rne_bf16(b.double()).float(), 1))  # bias rounded to bf16
    unwritten = got.clone()
    unwritten[1, H - 1, W - 1, Cout - 1] = 0xFFFF                            # one element the kernel did not write (the buffers start as 0xFF bytes)
    assert rejects(unwritten, y, m)
    r = R.rne_bf16(y)
    far = ((y - r).abs() < 0.1 * R.ulp_bf16(y)) & (got & 0x7FFF < 0x7F00) & (y.abs() > 1e-3)
    idx = int(far.reshape(-1).nonzero()[0])
    one = got.clone().reshape(-1)
    one[idx] += 1                                                            # one ulp at one element that is not near a tie
    assert rejects(one.reshape(got.shape), y, m)
    # the weight gradient: a reference that leaves one border pixel row out of the contraction
    gy = rand_bf16((N, H, W, Cout), g)
    dw = gd.new((Cout, C, 3, 3), name='dw')
    g16 = gd.ro(i16(R.bits_of(gy)), 'gy')
    Lb().check(lib.eld_conv3x3_backward_weight_bf16(dp(g16), dp(x16), C, None, 0, dp(dw), None, N, H, W, Cout,
                                                    dp(ws), ws.numel(), Lb().cur_stream()))
    done(gd)
    yw, bound = wgrad_ref(gy, x)
    assert bool(((dw.double() - yw).abs() <= bound).all())
    gd = gy.clone()
    gd[0, 0] = 0.0
    assert not bool(((dw.double() - R.conv3x3_wgrad(gd, x)).abs() <= bound).all())


# ---- the whole network, teacher-forced ------------------------------------------------------------------------------------
NET = [(2, 4, 272, 560), (3, 4, 48, 80), (2, 9, 272, 560), (1, 4, 1424, 2128)]
RG = {'ea': 0, 'eb': 1, 'pool': 2, 'up': 3, 'da': 4, 'db': 5, 'x16': 6, 'g11': 7}


@pytest.mark.parametrize('N,Cin,H,W', NET)
def test_unet_bf16_teacher_forced(lib, N, Cin, H, W):
    """One bf16 forward (saved activations) and backward: every saved tensor is checked against the layer reference applied to the kernel's
    own saved inputs -- the network's wiring and its call-site variants (fused pools, slope-code epilogues, conv_first from NCHW, the
    NHWC32 x16 input beyond 4 planes); the head's output and dW / db, and conv1_1's dW / db from the gradient region it consumed."""
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
    st = Lb().cur_stream()
    Lb().check(lib.eld_unet_forward_ex(dp(x), dp(prm), dp(out), dp(ws), nbytes, N, H, W, Cin, Cout, 1, -1, st))
    done(gd)

    def Wt(i, shape):
        return prm[offs[2 * i]:offs[2 * i + 1]].reshape(shape)

    def Bs(i):
        return prm[offs[2 * i + 1]:offs[2 * i + 2]]

    def region(name, lev):
        off, ch, dt = C.c_size_t(), C.c_int(), C.c_int()
        Lb().check(lib.eld_debug_unet_region(N, H, W, Cin, Cout, 1, RG[name], lev, C.byref(off), C.byref(ch), C.byref(dt)))
        lv = lev + 1 if name == 'pool' else lev
        h, w_ = H >> lv, W >> lv
        if dt.value == 2:
            n = N * ch.value * h * w_
            return ws[off.value:off.value + 4 * n].view(torch.float32).reshape(N, ch.value, h, w_)
        assert dt.value == 1
        n = N * h * w_ * ch.value
        return ws[off.value:off.value + 2 * n].view(torch.int16).reshape(N, h, w_, ch.value)

    def val(t16):
        return R.f64_of_bits(bits(t16))

    def chan(l):
        return 32 << l

    xn = x.permute(0, 2, 3, 1).double()
    # conv1_1
    ea0 = region('ea', 0)
    w0 = Wt(0, (32, Cin, 3, 3))
    if Cin <= 4:
        xh, xl = R.first_cut2(xn)
        wh, wl = R.first_cut2(w0)
        y = R.conv3x3(xh, wh) + R.conv3x3(xh, wl) + R.conv3x3(xl, wh) + Bs(0).double()
        mag2 = R.conv3x3(xh * xh, wh * wh) + R.conv3x3(xh * xh, wl * wl) + R.conv3x3(xl * xl, wh * wh)
        accept(ea0, *R.lrelu_ref(y, R.margin(mag2, 27 * Cin, Bs(0))), 'conv1_1 (conv_first)')
    else:
        x16 = val(region('x16', 0))
        assert bool((x16[..., :Cin] == R.rne_bf16(xn)).all()) and not bool(x16[..., Cin:].any())
        w32 = torch.zeros(32, 32, 3, 3, device='cuda')
        w32[:, :Cin] = w0
        accept(ea0, *conv_ref(x16, w32, Bs(0), 1), 'conv1_1 (NHWC32)')
    for l in range(5):
        if l:
            accept(region('ea', l), *conv_ref(val(region('pool', l - 1)), Wt(2 * l, (chan(l), chan(l - 1), 3, 3)), Bs(2 * l), 1), 'conv%d_1' % (l + 1))
        eb = region('eb', l)
        accept(eb, *conv_ref(val(region('ea', l)), Wt(2 * l + 1, (chan(l), chan(l), 3, 3)), Bs(2 * l + 1), 1), 'conv%d_2' % (l + 1))
        if l < 4:
            assert bool((val(region('pool', l)) == R.maxpool_fwd(val(eb))).all()), 'pool%d' % (l + 1)
    for l in range(3, -1, -1):
        iu = 10 + 3 * (3 - l)
        src = val(region('eb', 4) if l == 3 else region('db', l + 1))
        wu = R.rne_bf16(Wt(iu, (chan(l + 1), chan(l), 2, 2)).double())
        accept(region('up', l), R.convt_fwd(src, wu) + Bs(iu).double(), R.margin(R.convt_fwd(src * src, wu * wu), chan(l + 1), Bs(iu)), 'upv%d' % (9 - l))
        cat = torch.cat([val(region('up', l)), val(region('eb', l))], dim=3)
        accept(region('da', l), *conv_ref(cat, Wt(iu + 1, (chan(l), 2 * chan(l), 3, 3)), Bs(iu + 1), 1), 'conv%d_1' % (9 - l))
        accept(region('db', l), *conv_ref(val(region('da', l)), Wt(iu + 2, (chan(l), chan(l), 3, 3)), Bs(iu + 2), 1), 'conv%d_2' % (9 - l))
    db0 = val(region('db', 0))
    wh_ = Wt(22, (Cout, 32)).double()
    yo = torch.einsum('nyxc,oc->noyx', db0, wh_) + Bs(22).double()[None, :, None, None]
    bo = R.f32_bound(torch.einsum('nyxc,oc->noyx', db0 * db0, wh_ * wh_), 32) + R.C_ACC * R.U32 * (yo.abs() + Bs(22).double().abs()[None, :, None, None])
    f32_check(out, yo, bo, 'head output')
    # backward
    dout = gd.ro(torch.randn(N, Cout, H, W, generator=g).cuda(), 'dout')
    grads = gd.new((offs[46],), name='grads')
    Lb().check(lib.eld_unet_backward_ex(dp(dout), dp(prm), dp(grads), dp(ws), nbytes, N, H, W, Cin, Cout, 1, -1, None, None, 0, st))
    done(gd)
    d64 = dout.double()
    K = N * H * W
    yw = torch.einsum('noyx,nyxc->oc', d64, db0)
    bw = R.f32_bound(torch.einsum('noyx,nyxc->oc', d64 * d64, db0 * db0), K, torch.einsum('noyx,nyxc->oc', d64.abs(), db0.abs()))
    f32_check(grads[offs[44]:offs[45]].reshape(Cout, 32), yw, bw, 'head dW')
    f32_check(grads[offs[45]:offs[46]], d64.sum((0, 2, 3)), R.f32_bound((d64 * d64).sum((0, 2, 3)), K, d64.abs().sum((0, 2, 3))), 'head db')
    g11 = val(region('g11', 0))
    if Cin <= 4:
        xs = region('x16', 0).permute(0, 2, 3, 1)
        assert torch.equal(xs, x.permute(0, 2, 3, 1))
        hi, lo = R.wgrad_cut2(xs)
        xs = hi + lo
    else:
        xs = val(region('x16', 0))
    y1, b1 = wgrad_ref(g11, xs)
    f32_check(grads[offs[0]:offs[1]].reshape(32, Cin, 3, 3), y1[:, :Cin], b1[:, :Cin], 'conv1_1 dW')
    yb, bb = colsum_ref(g11)
    f32_check(grads[offs[1]:offs[2]], yb, bb, 'conv1_1 db')
