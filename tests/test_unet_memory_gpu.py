"""What the U-Net entry points and the single-layer entry points do to memory (C ABI, include/eld_amd.h), beside what they compute.

Every buffer of a call lies between guard bands (tests/guarded.py): x, params, target, dout, out, loss, grads and the workspace, the
workspace at exactly eld_unet_workspace_bytes / eld_layer_workspace_bytes bytes.  For every (shape, precision, sequence of calls):
  1. no byte outside any buffer is written, after every call;
  2. x, params, target and dout (the operands a call only reads) keep their bits;
  3. out, loss and grads hold no NaN afterwards: they start as 0xFF bytes, so every element was written;
  4. the sequence runs twice in the same arenas, on a workspace of 0x00 bytes and then on one of 0xFF bytes (NaN in fp32 and in bf16, -1 in
     every counter, all bits set in every code word), out / loss / grads refilled with 0xFF before each run: the results are the same bits.
     The callers hand the library torch.empty scratch, so a region read before it is written (a split-K partial that is not cleared, a bound
     slot, a code word beyond the last pixel) is a result that changes from run to run; here it changes between these two;
  5. a third run on the workspace as the second left it gives the same bits again;
  6. with ws_bytes one less than required every entry point returns ELD_EWS and leaves out, loss, grads and the workspace as they were.
Equality needs no tolerance: the suite already asks weight gradients to repeat bit for bit (tests/test_f32_layers_gpu.py).

The library keeps host bookkeeping per workspace pointer (which forward filled it last: csrc/unet.hip g_ws_state), so the workspace is
refilled between complete sequences only, never between a forward and its backward.

Shapes (N, C, H, W): the smallest legal one (one pixel at level 4); three images with odd tile counts (tests/variant_child.py NET_SMALL); 9 -> 9
planes (the wide head, the first layer through conv_wgrad); and per precision the shape at which tests/test_unet_gpu.py shows the network on
its specialised kernels (bf16 LDS-DMA kernels: 2 x 272 x 560; fp32 conv_x3w and slope / pool codes: 528 x 1072)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import guarded as G                  # noqa: E402

ELD_EWS = -3
SMALL = [(1, 4, 16, 16), (3, 4, 48, 80), (1, 9, 32, 48)]
BIG = {'fp32': (1, 4, 528, 1072), 'bf16': (2, 4, 272, 560)}
SEQUENCES = ['forward+backward', 'loss_l1+backward', 'loss_mse+backward', 'infer']
NET_CASES = [(prec, shape, seq) for prec in ('fp32', 'bf16') for shape in SMALL + [BIG[prec]] for seq in SEQUENCES
             if seq != 'loss_mse+backward' or shape in SMALL[:2]]


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    prev = eld_lib.eld_conv_fp32_algo(1)
    yield eld_lib
    eld_lib.eld_conv_fp32_algo(prev)


def Lb():
    from eld_amd import _lib
    return _lib


def dp(t):
    return Lb().dptr(t)


_PARAMS = {}


def params_for(lib, Cin):
    """He-scaled weights, small biases: one flat buffer per channel count, made once"""
    if Cin not in _PARAMS:
        offs = (C.c_int64 * 47)()
        assert lib.eld_unet_param_offsets(Cin, Cin, offs) == 0
        g = torch.Generator().manual_seed(100 + Cin)
        prm = torch.empty(offs[46])
        for i in range(23):
            w0, b0, e = offs[2 * i], offs[2 * i + 1], offs[2 * i + 2]
            fan = (b0 - w0) // (e - b0)
            prm[w0:b0] = torch.randn(b0 - w0, generator=g) * np.sqrt(2.0 / fan)
            prm[b0:e] = 0.1 * torch.randn(e - b0, generator=g)
        _PARAMS[Cin] = prm
    return _PARAMS[Cin]


class Problem:
    """one shape and precision: every buffer of the calls in its own arena"""

    def __init__(self, lib, prec, shape):
        self.lib, self.p = lib, 1 if prec == 'bf16' else 0
        N, Cc, H, W = shape
        self.dims = (N, H, W, Cc, Cc)
        g = torch.Generator().manual_seed(N * H + W + Cc)
        self.gd = gd = G.Guards()
        self.prm = gd.ro(params_for(lib, Cc).cuda(), 'params')
        x = torch.rand(*shape, generator=g)
        x.view(-1)[::17] = 0.0
        self.x = gd.ro(x.cuda(), 'x')
        self.target = gd.ro(torch.rand(*shape, generator=g).cuda(), 'target')
        self.dout = gd.ro((torch.randn(*shape, generator=g) / x.numel()).cuda(), 'dout')
        self.nbytes = lib.eld_unet_workspace_bytes(*self.dims)
        assert self.nbytes > 0
        self.ws = gd.new((self.nbytes,), torch.uint8, 'workspace')
        self.out = gd.new(shape, name='out')
        self.loss = gd.new((1,), name='loss')
        self.grads = gd.new((self.prm.numel(),), name='grads')
        self.results = (self.out, self.loss, self.grads)

    def done(self, what):
        torch.cuda.synchronize()
        try:
            self.gd.check()                                      # points 1 and 2
        except AssertionError as e:
            raise AssertionError('after %s: %s' % (what, e))

    # the four entry points; nbytes: what the call is told the workspace holds
    def forward(self, nbytes):
        return self.lib.eld_unet_forward_ex(dp(self.x), dp(self.prm), dp(self.out), dp(self.ws), nbytes, *self.dims, self.p, 1, Lb().cur_stream())

    def infer(self, nbytes):
        return self.lib.eld_unet_infer_ex(dp(self.x), dp(self.prm), dp(self.out), dp(self.ws), nbytes, *self.dims, self.p, 1, Lb().cur_stream())

    def forward_loss(self, nbytes, kind):
        return self.lib.eld_unet_forward_loss_ex(dp(self.x), dp(self.prm), dp(self.target), dp(self.out), dp(self.loss), dp(self.ws), nbytes, *self.dims,
                                                 self.p, 1, kind, 1.0, Lb().cur_stream())

    def backward(self, nbytes, dout):
        return self.lib.eld_unet_backward_ex(dp(dout), dp(self.prm), dp(self.grads), dp(self.ws), nbytes, *self.dims, self.p, 1, None, None, 0,
                                             Lb().cur_stream())

    def calls(self, seq, nbytes):
        """the sequence as [(name, thunk)]"""
        if seq == 'forward+backward':
            return [('eld_unet_forward_ex', lambda: self.forward(nbytes)), ('eld_unet_backward_ex', lambda: self.backward(nbytes, self.dout))]
        if seq == 'infer':
            return [('eld_unet_infer_ex', lambda: self.infer(nbytes))]
        kind = {'loss_l1+backward': 0, 'loss_mse+backward': 1}[seq]
        return [('eld_unet_forward_loss_ex', lambda: self.forward_loss(nbytes, kind)), ('eld_unet_backward_ex(dout = NULL)', lambda: self.backward(nbytes, None))]

    def run(self, seq, ws_fill):
        if ws_fill is not None:
            self.ws.guard.fill(ws_fill)
        for t in self.results:
            t.guard.fill(0xFF)
        for name, call in self.calls(seq, self.nbytes):
            Lb().check(call(), name)
            self.done(name)
        written = {'forward+backward': (True, False, True), 'infer': (True, False, False)}.get(seq, (True, True, True))
        for t, w in zip(self.results, written):                  # point 3
            if w:
                bad = torch.isnan(t)
                assert not bool(bad.any()), '%s: %d of %d elements are NaN (not written, or computed from memory nothing wrote), first at flat index %d' % (
                    t.guard.name, int(bad.sum()), t.numel(), int(bad.reshape(-1).nonzero()[0]))
            else:
                assert G.all_bytes(t, 0xFF), '%s: written by a sequence that has no use for it' % t.guard.name
        return [t.clone() for t in self.results]


def differ(a, b):
    return '; '.join('%s: %d of %d elements differ' % (n, int((G._bits(x) != G._bits(y)).sum()), x.numel())
                     for n, x, y in zip(('out', 'loss', 'grads'), a, b) if not G.same_bits(x, y))


@pytest.mark.parametrize('prec,shape,seq', NET_CASES, ids=['%s-%s-%s' % (p, 'x'.join(map(str, s)), q) for p, s, q in NET_CASES])
def test_unet_entry_points_keep_to_their_buffers_and_to_what_they_wrote(lib, prec, shape, seq):
    pb = Problem(lib, prec, shape)
    first = pb.run(seq, 0x00)
    second = pb.run(seq, 0xFF)
    assert not differ(first, second), 'workspace of 0x00 bytes against one of 0xFF bytes: ' + differ(first, second)          # point 4
    third = pb.run(seq, None)
    assert not differ(second, third), 'a repeat on the used workspace: ' + differ(second, third)                              # point 5
    # point 6: one byte short.  Every entry point, whatever the sequence; marked bytes everywhere they could write
    pb.ws.guard.fill(0x5A)
    for t in pb.results:
        t.guard.fill(0xFF)
    short = pb.nbytes - 1
    for name, call in [('eld_unet_forward_ex', lambda: pb.forward(short)), ('eld_unet_infer_ex', lambda: pb.infer(short)),
                       ('eld_unet_forward_loss_ex (L1)', lambda: pb.forward_loss(short, 0)), ('eld_unet_forward_loss_ex (MSE)', lambda: pb.forward_loss(short, 1)),
                       ('eld_unet_backward_ex', lambda: pb.backward(short, pb.dout)), ('eld_unet_backward_ex(dout = NULL)', lambda: pb.backward(short, None))]:
        assert call() == ELD_EWS, name
    pb.done('the calls with a workspace one byte short')
    assert G.all_bytes(pb.ws, 0x5A), 'a refused call wrote to the workspace'
    for t in pb.results:
        assert G.all_bytes(t, 0xFF), 'a refused call wrote to %s' % t.guard.name


# ---- single layers: one row per entry point, the smallest of its table -----------------------------------------------------------------
def f32(shape, g, scale=1.0):
    t = torch.randn(*shape, generator=g) * scale
    t.view(-1)[::13] = 0.0
    return t.cuda()


def b16(shape, g):
    """bf16 bit patterns as the kernels read them (int16)"""
    t = torch.randn(*shape, generator=g)
    t.view(-1)[::13] = 0.0
    return t.bfloat16().view(torch.int16).cuda()


def layer_case(lib, name, gd, g):
    """-> (call(ws, ws_bytes) -> rc, outputs, (N, H, W, Cin, Cout) of the workspace query)"""
    st = Lb().cur_stream()
    bf = name.endswith('_bf16')
    act = b16 if bf else (lambda s, g_: f32(s, g_))
    odt = torch.int16 if bf else torch.float32
    if name.startswith('eld_conv3x3_forward'):
        N, H, W, Ci, Co = 3, 9, 21, 32, 32                       # FWD of both layer files: (3, 9, 21, 32, 0, 32)
        x, w, b = gd.ro(act((N, H, W, Ci), g), 'x'), gd.ro(f32((Co, Ci, 3, 3), g, 1 / np.sqrt(9 * Ci)), 'w'), gd.ro(f32((Co,), g, 0.5), 'b')
        out = gd.new((N, H, W, Co), odt, 'out')
        if bf:
            return (lambda ws, n: lib.eld_conv3x3_forward_bf16(dp(x), Ci, None, 0, dp(w), dp(b), dp(out), None, N, H, W, Co, 1, dp(ws), n, st)), [out], (N, H, W, Ci, Co)
        return (lambda ws, n: lib.eld_conv3x3_forward(dp(x), Ci, None, 0, dp(w), dp(b), dp(out), N, H, W, Co, 1, dp(ws), n, st)), [out], (N, H, W, Ci, Co)
    if name.startswith('eld_conv3x3_backward_data'):
        N, H, W, Ci, Co = 3, 9, 21, 32, 32                       # BWD: (3, 9, 21, 32, 32, 32)
        gy, w, a = gd.ro(act((N, H, W, Co), g), 'gy'), gd.ro(f32((Co, Ci, 3, 3), g, 1 / np.sqrt(9 * Co)), 'w'), gd.ro(act((N, H, W, Ci), g), 'act')
        d0 = gd.new((N, H, W, Ci), odt, 'd0')
        fn = lib.eld_conv3x3_backward_data_bf16 if bf else lib.eld_conv3x3_backward_data
        return (lambda ws, n: fn(dp(gy), dp(w), dp(d0), None, Ci, dp(a), None, N, H, W, Ci, Co, dp(ws), n, st)), [d0], (N, H, W, Ci, Co)
    if name.startswith('eld_conv3x3_backward_weight'):
        N, H, W, Ci, Co = (3, 9, 21, 64, 64) if bf else (3, 9, 21, 32, 32)      # WG: (3, 9, 21, 64, 0, 64) / (3, 9, 21, 32, 0, 32)
        gy, x = gd.ro(act((N, H, W, Co), g), 'gy'), gd.ro(act((N, H, W, Ci), g), 'x')
        dw, db = gd.new((Co, Ci, 3, 3), name='dw'), gd.new((Co,), name='db')
        fn = lib.eld_conv3x3_backward_weight_bf16 if bf else lib.eld_conv3x3_backward_weight
        return (lambda ws, n: fn(dp(gy), dp(x), Ci, None, 0, dp(dw), dp(db), N, H, W, Co, dp(ws), n, st)), [dw, db], (N, H, W, Ci, Co)
    N, H, W, Ci, Co = (3, 7, 13, 64, 32) if bf else (1, 8, 8, 128, 64)          # CT of the bf16 file / test_conv_transpose2x2
    x, w, b = gd.ro(act((N, H, W, Ci), g), 'x'), gd.ro(f32((Ci, Co, 2, 2), g, 1 / np.sqrt(Ci)), 'w'), gd.ro(f32((Co,), g, 0.5), 'b')
    d = gd.ro(act((N, 2 * H, 2 * W, Co), g), 'd')
    if name.startswith('eld_convt2x2_forward'):
        out = gd.new((N, 2 * H, 2 * W, Co), odt, 'out')
        fn = lib.eld_convt2x2_forward_bf16 if bf else lib.eld_convt2x2_forward
        return (lambda ws, n: fn(dp(x), dp(w), dp(b), dp(out), N, H, W, Ci, Co, dp(ws), n, st)), [out], (N, H, W, Ci, Co)
    if name.startswith('eld_convt2x2_backward_data'):
        din = gd.new((N, H, W, Ci), odt, 'din')
        fn = lib.eld_convt2x2_backward_data_bf16 if bf else lib.eld_convt2x2_backward_data
        return (lambda ws, n: fn(dp(d), dp(w), dp(x), dp(din), N, H, W, Ci, Co, dp(ws), n, st)), [din], (N, H, W, Ci, Co)
    assert name.startswith('eld_convt2x2_backward_weight')
    dw, db = gd.new((Ci, Co, 2, 2), name='dw'), gd.new((Co,), name='db')
    fn = lib.eld_convt2x2_backward_weight_bf16 if bf else lib.eld_convt2x2_backward_weight
    return (lambda ws, n: fn(dp(x), dp(d), dp(dw), dp(db), N, H, W, Ci, Co, dp(ws), n, st)), [dw, db], (N, H, W, Ci, Co)


LAYER_ENTRIES = [op + sfx for sfx in ('', '_bf16') for op in ('eld_conv3x3_forward', 'eld_conv3x3_backward_data', 'eld_conv3x3_backward_weight',
                                                                'eld_convt2x2_forward', 'eld_convt2x2_backward_data', 'eld_convt2x2_backward_weight')]


@pytest.mark.parametrize('name', LAYER_ENTRIES)
def test_layer_entry_points_keep_to_their_buffers_and_to_what_they_wrote(lib, name):
    """points 1, 2, 4 and 6 for the single-layer entry points: a zeroed against a dirty layer workspace"""
    gd = G.Guards()
    g = torch.Generator().manual_seed(len(name))
    call, outs, dims = layer_case(lib, name, gd, g)
    nbytes = lib.eld_layer_workspace_bytes(*dims)
    assert nbytes > 0
    ws = gd.new((nbytes,), torch.uint8, 'layer workspace')
    res = []
    for fill in (0x00, 0xFF):
        ws.guard.fill(fill)
        for t in outs:
            t.guard.fill(0xFF)
        Lb().check(call(ws, nbytes), name)
        torch.cuda.synchronize()
        gd.check()
        for t in outs:                                           # an int16 output holds bf16 bits: 0xFFFF is a NaN no kernel computes from finite data
            bad = torch.isnan(t) if t.is_floating_point() else (t == -1)
            assert not bool(bad.any()), '%s: %d of %d elements of %s not written' % (name, int(bad.sum()), t.numel(), t.guard.name)
        res.append([t.clone() for t in outs])
    for t, a, b in zip(outs, *res):
        assert G.same_bits(a, b), '%s: %s differs at %d of %d elements between a zeroed and a dirty workspace' % (
            name, t.guard.name, int((G._bits(a) != G._bits(b)).sum()), a.numel())
    ws.guard.fill(0x5A)
    for t in outs:
        t.guard.fill(0xFF)
    assert call(ws, nbytes - 1) == ELD_EWS
    torch.cuda.synchronize()
    gd.check()
    assert G.all_bytes(ws, 0x5A) and all(G.all_bytes(t, 0xFF) for t in outs)
