"""The U-Net backward, teacher-forced: every gradient stage of both engines against float64 (DESIGN.md sections 6 / 6a; checker:
oracle/bwd_ref.py, proved against autograd on the CPU by tests/test_backward_ref_cpu.py).

One forward, then one backward with the gradient tap set (include/eld_amd.h eld_debug_unet_grad_tap) into a NaN-poisoned tap buffer and
NaN-poisoned grads.  Each of the 30 tapped activation gradients and each of the 46 parameter gradients is compared element by element
with the float64 stage applied to the backward's OWN tapped input and the forward's saved regions (eld_debug_unet_region), so an error
cannot compound or cancel across stages and a failure names its stage and element:
  * fp32 (scheme 1): |got - y64| <= x3_bound (oracle/f32_ref.py), bias gradients and the head by f32_bound, pools bit for bit;
  * bf16: activation gradients by bf16_accept with the accumulation margin, dW / db by f32_bound, pools = rne_bf16 of the fp32 expression.
Every case runs with an explicit dout after eld_unet_forward_ex and as eld_unet_forward_loss_ex + backward with dout == NULL (the fused
head's gradient buffer, partials and packed weights; there dout = sign(out - target) * grad_scale / n, exact).  The backward runs twice:
the parameter gradients must repeat bit for bit.  The kernel families launched inside the backward are read from the launch counters and
must be the set the dispatcher's conditions give for the shape (RAN).

Inputs (tests/backward_cases.py): x piecewise constant on 6 x 10 blocks (tied pool windows), one all-zero output channel in conv1_1,
conv1_2, conv2_2, conv5_1 and conv9_1 (exact +0 activations: slope 0.6, four-way ties), exact +0 / -0 in dout.  The codes-live cases run
at shapes where the forward fills slope / pool codes (eld_debug_unet_codes says which) and again with eld_debug_kernel_mask(128): codes are
an encoding of the same slopes and winners, so the reference is the same.

MEASURED: worst error / bound per stage kind (bf16 'g': worst near-tie flip rate of one tensor), one MI355X, this file."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import bf16_ref as R     # noqa: E402  (checker only)
from oracle import bwd_ref as B      # noqa: E402

import backward_cases as BC          # noqa: E402
from guarded import Guards           # noqa: E402
from test_bf16_layers_gpu import FLIP_MAX      # noqa: E402  (the bf16 layer file's cap on near-tie flips of one tensor)

MEASURED = {'fp32 g': 0.970, 'fp32 dw': 0.413, 'fp32 db': 0.240, 'fp32 head_g': 0.357, 'fp32 head_dw': 0.016, 'fp32 head_db': 0.010,
            'bf16 dw': 0.313, 'bf16 db': 0.070, 'bf16 head_dw': 0.018, 'bf16 head_db': 0.010,
            'bf16 g': 5.2e-4, 'bf16 head_g': 5.7e-5}      # the last two: near-tie flip rates.  The bf16 layer file's FLIP_MEASURED is 3.9e-4; these
# backward tensors stay inside its FLIP_MAX (3 x 3.9e-4 = 1.17e-3), so they need no cap of their own.
# 'fp32 g' is d_up0 of the codes shape (conv_x3w, 64 -> 32 + 32 channels, 16 M elements); the next are d_ea0 0.86, d_ea1 0.81, d_da0 0.80, d_up2 0.80.
STATS = {}
ELD_EINVAL, ELD_ENOTSUP = -1, -2
EA0, EA1, DA0, DA1, EB0, EB1 = 1, 2, 4, 8, 16, 32
RG = {'ea': 0, 'eb': 1, 'pool': 2, 'up': 3, 'da': 4, 'db': 5, 'x16': 6}
NAMES = {
    'fp32': ['conv_x3w', 'conv_x3<32>', 'conv_x3d<128,8>', 'conv_x3d<64,8>', 'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<1x1>',
             'conv_x3_gemm<gather>', 'conv_igemm<f32>', 'conv_igemm<f32,h2>', 'wgrad8<f32,128x64>', 'wgrad8<f32,64x64>', 'wgrad8<f32,64x32>',
             'wgrad8<f32,32x64>', 'wgrad8<f32,32x32>', 'wgradt8', 'wgrad<f32>', 'wgrad<f32,gather>'],
    'bf16': ['conv_bfs', 'conv_bfw', 'conv_bfd<128>', 'conv_bfd<64>', 'conv_bfg<128>', 'conv_bfg<64,gather>', 'conv_bfg<128,gather>', 'conv_igemm<bf16>',
             'conv_igemm<bf16,1x1>', 'conv_igemm<bf16,gather>', 'wgrad8d', 'wgrad8<bf16>', 'wgrad<bf16>', 'wgrad<bf16,gather>'],
}
F32_CODES_SHAPE = (1, 4, 496, 1024)       # the smallest shape (by pixels, N = 1) whose fp32 scheme-1 forward reports all six code regions on 256 CUs
BF16_CODES_SHAPE = (1, 4, 256, 512)
# The families a 256-CU dispatcher chooses inside each backward, from its own conditions:
#   weight gradients, fp32 scheme 1 (conv_wgrad.hip wgrad8_shape: the block is a function of the channel counts alone, so every shape sees all five):
#     32x32 conv1_2 / conv9_2, 32x64 conv9_1, 64x32 conv2_1, 64x64 conv2_2 / conv8_1 / conv8_2, 128x64 every layer with Cout >= 128; transposed convs
#     with Cin % 128 == 0 (upv6-8) wgradt8, upv9 (Cin 64) wgrad<f32,gather>; conv1_1 of 4 planes is conv_first (records no name), of 9 planes the
#     NHWC16 copy, C0 = 16, which the 8-wave kernel refuses: wgrad<f32>;
#   backward-data, fp32: the forward's dispatcher with Cin and Cout exchanged (tests/test_f32_layers_gpu.py RAN): 32 output channels conv_x3w from
#     256 tiles of 16 x 32 on (496 x 1024: 992), else conv_x3<32> (48 x 80 x 3: 27); the other layers take the 8-wave kernels where 16-row tiles x
#     output channels / 64 (or / 128) give every CU one (conv_x3.hip x3_slab_bn): level 1 of 496 x 1024 has exactly 256 tiles -- conv_x3d<64,8>, and
#     conv_x3d<128,8> for conv8_1's backward-data, which writes 128 channels there --, the small shapes never do; else conv_x3d<64,4>, with K split
#     where that leaves CUs idle; the four transposed convs conv_x3_gemm<gather>;
#   bf16: weight gradients wgrad8d for the 128-row blocks, wgrad8<bf16> for the others (conv1_1 of 9 planes reads the NHWC32 copy: a 32 x 32 block),
#     transposed convs wgrad<bf16,gather>; backward-data conv_bfs (32 output channels) and conv_bfw (64, K <= 64) from 256 tiles on -- 256 x 512 has
#     256 at level 0 and at level 1 by its two channel blocks --, conv_bfd / conv_bfg need more than these shapes have: conv_igemm<bf16>[,gather].
_WG32 = {'wgrad8<f32,128x64>', 'wgrad8<f32,64x64>', 'wgrad8<f32,64x32>', 'wgrad8<f32,32x64>', 'wgrad8<f32,32x32>', 'wgradt8', 'wgrad<f32,gather>'}
_SMALL32 = _WG32 | {'conv_x3<32>', 'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<gather>'}
_BIG32 = _WG32 | {'conv_x3w', 'conv_x3d<64,8>', 'conv_x3d<128,8>', 'conv_x3d<64,4>', 'conv_x3d<64,4,splitk>', 'conv_x3_gemm<gather>'}
_SMALL16 = {'wgrad8d', 'wgrad8<bf16>', 'wgrad<bf16,gather>', 'conv_igemm<bf16>', 'conv_igemm<bf16,gather>'}
RAN = {('fp32', (3, 4, 48, 80)): _SMALL32, ('fp32', (2, 9, 48, 80)): _SMALL32 | {'wgrad<f32>'}, ('bf16', (3, 4, 48, 80)): _SMALL16,
       ('bf16', (2, 9, 48, 80)): _SMALL16, ('fp32', F32_CODES_SHAPE): _BIG32, ('bf16', BF16_CODES_SHAPE): _SMALL16 | {'conv_bfs', 'conv_bfw'}}

CASES = [  # precision, (N, Cin, H, W), debug mask, codes the forward must report (-1: none)
    ('fp32', (3, 4, 48, 80), 0, -1),            # three images, the small families, split-K in both directions, ragged tiles
    ('fp32', (2, 9, 48, 80), 0, -1),            # conv1_1's weight gradient from the NHWC16 copy, the wide head (unet_wide.hip)
    ('bf16', (3, 4, 48, 80), 0, -1),
    ('bf16', (2, 9, 48, 80), 0, -1),
    ('fp32', F32_CODES_SHAPE, 0, EA0 | EA1 | DA0 | DA1 | EB0 | EB1),
    ('fp32', F32_CODES_SHAPE, 128, -1),
    ('bf16', BF16_CODES_SHAPE, 0, EA0 | DA0),
    ('bf16', BF16_CODES_SHAPE, 128, -1),
]


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    prev = eld_lib.eld_conv_fp32_algo(1)
    yield eld_lib
    eld_lib.eld_conv_fp32_algo(prev)
    eld_lib.eld_debug_unet_grad_tap(None, 0)
    print('\nbackward stages: worst error / bound per stage kind (bf16 g: worst near-tie flip rate of one tensor)')
    for k in sorted(STATS):
        print('    %-18s %.3e' % (k, STATS[k]))


def Lb():
    from eld_amd import _lib
    return _lib


def dp(t):
    return Lb().dptr(t)


def bits(t16):
    return t16.to(torch.int32) & 0xFFFF


def stat(key, v):
    STATS[key] = max(STATS.get(key, 0.0), v)


def check_f32(prec, t, got, y, bound):
    err = (got.double().reshape(y.shape) - y).abs()
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    stat('%s %s' % (prec, t.kind), r)
    print('%s %-16s worst error / bound %.3f' % (prec, t.name, r))
    bad = ~(err <= bound)                                   # (a bound of 0 asks for the exact value; a NaN left in `got` is bad too)
    assert not bool(bad.any()), '%s %s: %d of %d elements outside the bound, worst %.3f of it, first at %s' % (
        prec, t.name, int(bad.sum()), bad.numel(), r, tuple(bad.nonzero()[0].tolist()))


def check_bf16(t, got_bits, y, m):
    ok, fl = R.bf16_accept(got_bits, y, m)
    rate = float(fl.sum()) / max(fl.numel(), 1)
    stat('bf16 %s' % t.kind, rate)
    print('bf16 %-16s near-tie flips %.2e' % (t.name, rate))
    assert bool(ok.all()), 'bf16 %s: %d of %d elements outside the rounding rule, first at %s' % (
        t.name, int((~ok).sum()), ok.numel(), tuple((~ok).nonzero()[0].tolist()))
    assert rate <= FLIP_MAX, 'bf16 %s: near-tie flips %.3e > %.3e' % (t.name, rate, FLIP_MAX)


class Net:
    """one problem: parameters, input, workspace, and the readers of the library's regions and of the tap buffer"""

    def __init__(self, lib, prec, shape):
        self.lib, self.prec, self.p = lib, prec, 1 if prec == 'bf16' else 0
        self.N, self.Cin, self.H, self.W = shape
        N, Cin, H, W = shape
        self.Cout = Cin
        self.offs = (C.c_int64 * 47)()
        assert lib.eld_unet_param_offsets(Cin, Cin, self.offs) == 0
        g = torch.Generator().manual_seed(N * H + Cin + 3)
        self.Ws, self.Bs = BC.make_params(Cin, Cin, g)
        prm = torch.empty(self.offs[46])
        for i in range(23):
            w0, b0, e = self.offs[2 * i], self.offs[2 * i + 1], self.offs[2 * i + 2]
            assert b0 - w0 == self.Ws[i].numel() and e - b0 == self.Bs[i].numel()
            prm[w0:b0] = self.Ws[i].reshape(-1)
            prm[b0:e] = self.Bs[i]
        # every buffer the library writes lies between guard bands and starts as 0xFF bytes (the workspace at exactly the size the library asks
        # for); what it only reads is a guarded copy whose bits are compared after every call (check)
        self.gd = Guards()
        self.prm = self.gd.ro(prm.cuda(), 'prm')
        self.x = self.gd.ro(BC.tied_input(N, Cin, H, W, g).cuda(), 'x')
        self.dout = self.gd.ro(BC.sprinkle(torch.randn(N, Cin, H, W, generator=g)).cuda(), 'dout')
        self.noise = torch.randn(N, Cin, H, W, generator=g).cuda()
        self.nbytes = lib.eld_unet_workspace_bytes(N, H, W, Cin, Cin)
        self.ws = self.gd.new((self.nbytes,), torch.uint8, 'workspace')
        self.out = self.gd.new((N, Cin, H, W), name='out')
        self.tap_bytes = lib.eld_debug_unet_grad_tap_bytes(N, H, W, Cin, Cin, self.p)
        assert self.tap_bytes > 0
        self.algo = -1 if self.p else 1

    def dims(self):
        return self.N, self.H, self.W, self.Cin, self.Cout

    def check(self):
        torch.cuda.synchronize()
        self.gd.check()

    def forward(self, target=None, grad_scale=0.0):
        st = Lb().cur_stream()
        if target is None:
            Lb().check(self.lib.eld_unet_forward_ex(dp(self.x), dp(self.prm), dp(self.out), dp(self.ws), self.nbytes, *self.dims(), self.p, self.algo, st))
        else:
            loss = self.gd.new((1,), name='loss')
            Lb().check(self.lib.eld_unet_forward_loss_ex(dp(self.x), dp(self.prm), dp(target), dp(self.out), dp(loss), dp(self.ws), self.nbytes, *self.dims(),
                                                         self.p, self.algo, 0, grad_scale, st))
        self.check()
        assert target is None or not bool(torch.isnan(loss).any())
        return self.lib.eld_debug_unet_codes(dp(self.ws))

    def backward(self, dout, grads):
        return self.lib.eld_unet_backward_ex(dp(dout), dp(self.prm), dp(grads), dp(self.ws), self.nbytes, *self.dims(), self.p, self.algo, None, None, 0,
                                             Lb().cur_stream())

    def region(self, name, lev):
        """a saved region as float64 NHWC"""
        off, ch, dt = C.c_size_t(), C.c_int(), C.c_int()
        Lb().check(self.lib.eld_debug_unet_region(*self.dims(), self.p, RG[name], lev, C.byref(off), C.byref(ch), C.byref(dt)))
        lv = lev + 1 if name == 'pool' else lev
        h, w_ = self.H >> lv, self.W >> lv
        n = self.N * ch.value * h * w_
        if dt.value == 2:
            return self.ws[off.value:off.value + 4 * n].view(torch.float32).reshape(self.N, ch.value, h, w_).permute(0, 2, 3, 1).double()
        if dt.value == 0:
            return self.ws[off.value:off.value + 4 * n].view(torch.float32).reshape(self.N, h, w_, ch.value).double()
        return R.f64_of_bits(bits(self.ws[off.value:off.value + 2 * n].view(torch.int16).reshape(self.N, h, w_, ch.value)))

    def regions(self, fused):
        f = {k: [self.region(k, l) for l in range(5 if k in ('ea', 'eb') else 4)] for k in ('ea', 'eb', 'pool', 'up', 'da', 'db')}
        xn = self.x.permute(0, 2, 3, 1)
        if self.Cin <= 4:
            if not fused:                                   # (the fused forward leaves the input with the caller)
                assert torch.equal(self.region('x16', 0), xn.double())
            if self.p:                                      # conv_first.hip's weight gradient stages x as two bf16 pieces
                hi, lo = R.wgrad_cut2(xn)
                f['x'] = hi + lo
            else:                                           # three truncated pieces, six products: the scheme x3_bound models
                f['x'] = xn.double()
        else:
            x16 = self.region('x16', 0)
            assert bool((x16[..., :self.Cin] == (R.rne_bf16(xn.double()) if self.p else xn.double())).all()) and not bool(x16[..., self.Cin:].any())
            f['x'] = x16[..., :self.Cin]
        return f

    def weights(self):
        """the weights as the backward's kernels read them: fp32, or packed to bf16 (the head reads fp32 in both engines)"""
        W = [w.cuda().double() for w in self.Ws]
        return [R.rne_bf16(w) if self.p and i != B.HEAD else w for i, w in enumerate(W)]

    def taps(self, buf):
        out = {}
        for s, name in enumerate(B.TAP):
            off, ch, lev, dt = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
            Lb().check(self.lib.eld_debug_unet_grad_tap_layout(*self.dims(), self.p, s, C.byref(off), C.byref(ch), C.byref(lev), C.byref(dt)))
            assert dt.value == self.p and off.value % 256 == 0
            h, w_ = self.H >> lev.value, self.W >> lev.value
            n = self.N * h * w_ * ch.value
            if self.p:
                raw = buf[off.value:off.value + 2 * n].view(torch.int16).reshape(self.N, h, w_, ch.value)
                out[name] = (bits(raw), R.f64_of_bits(bits(raw)))
            else:
                raw = buf[off.value:off.value + 4 * n].view(torch.float32).reshape(self.N, h, w_, ch.value)
                out[name] = (raw, raw.double())
            assert not bool(torch.isnan(out[name][1]).any()), 'tap %s: not (fully) written' % name
        assert off.value + (2 if self.p else 4) * n <= self.tap_bytes
        return out


@pytest.mark.parametrize('fused', [False, True], ids=['dout', 'fused'])
@pytest.mark.parametrize('prec,shape,mask,codes', CASES)
def test_unet_backward_teacher_forced(lib, prec, shape, mask, codes, fused):
    net = Net(lib, prec, shape)
    N, Cin, H, W = shape
    old = lib.eld_debug_kernel_mask(mask) if mask else None
    try:
        have = net.forward()
        if fused:
            # target: the output itself at every 7th element (dout exactly 0 there), else off by noise of either sign; grad_scale = n: dout = +-1
            target = net.out + 0.1 * net.noise
            target.view(-1)[::7] = net.out.view(-1)[::7]
            target = net.gd.ro(target, 'target')
            n = net.out.numel()
            have = net.forward(target, float(n))
            gs = float(np.float32(n) / np.float32(n))
            d64 = torch.sign(net.out.double() - target.double()) * gs
            assert bool((d64 == 0).any()) and bool((d64 > 0).any()) and bool((d64 < 0).any())
        else:
            d64 = net.dout.double()
        assert have == codes, 'the forward reports codes %d' % have
        fwd = net.regions(fused)
        before = {n_: lib.eld_debug_conv_kernel_count(n_.encode()) for n_ in NAMES[prec]}
        assert 0xFFFFFFFF not in before.values()
        tap = net.gd.new((net.tap_bytes,), torch.uint8, 'tap')                             # 0xFF bytes: NaN in fp32 and in bf16
        res = []
        lib.eld_debug_unet_grad_tap(dp(tap), tap.numel())
        try:
            for rep in range(2):
                grads = net.gd.new((net.offs[46],), name='grads')
                Lb().check(net.backward(None if fused else net.dout, grads))
                net.check()
                res.append(grads)
                if rep == 0:
                    ran = {n_ for n_ in NAMES[prec] if lib.eld_debug_conv_kernel_count(n_.encode()) > before[n_]}
                if fused:
                    break                   # (the fused forward's state is for one backward; the repeat runs with the explicit dout)
        finally:
            lib.eld_debug_unet_grad_tap(None, 0)
    finally:
        if mask:
            lib.eld_debug_kernel_mask(old)
    if not fused:
        assert torch.equal(res[0], res[1]), 'parameter gradients of two identical backwards differ at %d elements' % int((res[0] != res[1]).sum())
    grads = res[0]
    assert not bool(torch.isnan(grads).any())
    taps = net.taps(tap)
    index = {n_ + s: 2 * i + k for i, n_ in enumerate(B.LAYERS) for k, s in enumerate(('.weight', '.bias'))}
    rule = B.bf16_rule if net.p else B.f32_rule
    seen = 0
    for step in B.stages(fwd, net.weights(), d64, taps={k: v[1] for k, v in taps.items()}):
        for t in step:
            seen += 1
            if t.kind == 'pool':
                ref = R.maxpool_bwd_f32(*t.y)
                got = taps[t.name][1]
                same = got == (R.rne_bf16(ref) if net.p else ref)
                assert bool(same.all()), '%s %s: %d elements differ, first at %s' % (prec, t.name, int((~same).sum()), tuple((~same).nonzero()[0].tolist()))
                continue
            y, m = rule(t)
            if t.name in index:
                j = index[t.name]
                check_f32(prec, t, grads[net.offs[j]:net.offs[j + 1]], y, m)
            elif net.p:
                check_bf16(t, taps[t.name][0], y, m)
            else:
                check_f32(prec, t, taps[t.name][0], y, m)
    assert seen == 30 + 46
    print('families in the backward of', prec, shape, 'mask', mask, sorted(ran))
    assert ran == RAN[(prec, shape)]                          # (the debug mask switches codes, not kernels)


def test_tap_argument_checks(lib):
    """The tap's refusals are argument checks that return before any launch: a buffer too small for the call's shape (ELD_EINVAL), a stream
    under capture (ELD_ENOTSUP: refused before capture of any kernel, so the rejection runs no GPU work); the layout query rejects what it cannot
    describe.  With the tap unset the same calls go through."""
    net = Net(lib, 'fp32', (1, 4, 16, 16))
    off, ch, lev, dt = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    q = (C.byref(off), C.byref(ch), C.byref(lev), C.byref(dt))
    assert lib.eld_debug_unet_grad_tap_layout(*net.dims(), 0, 30, *q) == ELD_EINVAL
    assert lib.eld_debug_unet_grad_tap_layout(*net.dims(), 0, -1, *q) == ELD_EINVAL
    assert lib.eld_debug_unet_grad_tap_layout(*net.dims(), 2, 0, *q) == ELD_EINVAL
    assert lib.eld_debug_unet_grad_tap_layout(1, 24, 16, 4, 4, 0, 0, *q) == ELD_EINVAL
    assert lib.eld_debug_unet_grad_tap_bytes(1, 24, 16, 4, 4, 0) == 0
    assert lib.eld_debug_unet_grad_tap_bytes(*net.dims(), 1) < lib.eld_debug_unet_grad_tap_bytes(*net.dims(), 0)
    ends = []
    for s in range(30):                                        # the 30 tensors tile the buffer without overlap
        assert lib.eld_debug_unet_grad_tap_layout(*net.dims(), 0, s, *q) == 0 and dt.value == 0
        n = 4 * net.N * (net.H >> lev.value) * (net.W >> lev.value) * ch.value
        assert not ends or off.value >= ends[-1]
        ends.append(off.value + n)
    assert ends[-1] <= net.tap_bytes
    assert lib.eld_debug_unet_codes(dp(torch.empty(16, dtype=torch.uint8, device='cuda'))) == -1       # a workspace no forward ran on
    net.forward()
    grads = torch.zeros(net.offs[46], device='cuda')
    tap = torch.zeros(net.tap_bytes, dtype=torch.uint8, device='cuda')
    try:
        lib.eld_debug_unet_grad_tap(dp(tap), net.tap_bytes - 1)
        assert net.backward(net.dout, grads) == ELD_EINVAL
        torch.cuda.synchronize()
        assert not bool(grads.any()) and not bool(tap.any())      # nothing ran
        lib.eld_debug_unet_grad_tap(dp(tap), net.tap_bytes)
        graph = torch.cuda.CUDAGraph()
        mark = torch.zeros(1, device='cuda')
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                mark.add_(1.0)                                     # (something to capture: the stream is capturing when the call is made)
                rc = net.backward(net.dout, grads)
        torch.cuda.current_stream().wait_stream(s)
        assert rc == ELD_ENOTSUP
        torch.cuda.synchronize()
        assert not bool(grads.any()) and not bool(tap.any())
    finally:
        lib.eld_debug_unet_grad_tap(None, 0)
    Lb().check(net.backward(net.dout, grads))                 # unset: the plain backward
    net.check()
    assert bool(grads.any()) and not bool(tap.any())


def test_negative_controls_are_rejected(lib):
    """The rules reject the defects they exist for: a dW without one border row, a d_eb without the skip term, a slope of 1.0 at the exact
    zeros, a tie routed to the last window element, d_up / skip swapped, one bf16 ulp away from a midpoint.  Arithmetic on float64 reference
    tensors of a small problem (tests/backward_cases.py); no library kernel runs."""
    g = torch.Generator().manual_seed(5)
    Ws, Bs = BC.make_params(4, 4, g, torch.float64)
    x = BC.tied_input(2, 4, 32, 48, g, torch.float64)
    dout = BC.sprinkle(torch.randn(2, 4, 32, 48, generator=g, dtype=torch.float64))
    fwd, _ = BC.forward_regions([w.cuda() for w in Ws], [b.cuda() for b in Bs], x.cuda())
    BC.negative_controls(fwd, [w.cuda() for w in Ws], dout.cuda())
