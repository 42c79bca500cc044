"""Inputs and negative controls shared by tests/test_backward_ref_cpu.py and tests/test_backward_layers_gpu.py (checker side only: plain
torch on float64 tensors, no library call).

Random data never produces an exact zero or a tied pool window, so:
  * tied_input: piecewise constant on 6 x 10 blocks offset against the 2 x 2 pool windows (inside a block the four window elements of
    conv1_2's output are the same bits; across a block edge two of them are);
  * zero_channel: one output channel of conv1_1, conv1_2, conv2_2, conv5_1 and conv9_1 gets zero weights and bias -- its activation is +0
    everywhere, every slope there is 0.6, every pool window of it is a four-way tie won by its first element;
  * sprinkle: exact +0 / -0 in dout."""
import numpy as np
import torch

from oracle import bf16_ref as R
from oracle import bwd_ref as B

ZERO_LAYERS = (0, 1, 3, 8, B.up_index(0) + 1)          # conv1_1, conv1_2, conv2_2, conv5_1, conv9_1
ZERO_CHANNEL = 5


def layer_shapes(in_ch, out_ch):
    """weight shapes of the 23 layers in parameter order, reference layouts (conv: OIHW; transposed conv: [Cin][Cout][2][2])"""
    s = []
    for l in range(5):
        s += [(B.chan(l), in_ch if l == 0 else B.chan(l - 1), 3, 3), (B.chan(l), B.chan(l), 3, 3)]
    for l in range(3, -1, -1):
        s += [(B.chan(l + 1), B.chan(l), 2, 2), (B.chan(l), 2 * B.chan(l), 3, 3), (B.chan(l), B.chan(l), 3, 3)]
    return s + [(out_ch, 32, 1, 1)]


def bias_len(i, shape):
    return shape[1] if B.LAYERS[i].startswith('upv') else shape[0]


def make_params(in_ch, out_ch, g, dtype=torch.float32):
    """He-scaled weights and small biases (CPU), the zeroed channel applied: (list of weights, list of biases)"""
    Ws, Bs = [], []
    for i, sh in enumerate(layer_shapes(in_ch, out_ch)):
        fan = sh[1] * sh[2] * sh[3] if not B.LAYERS[i].startswith('upv') else sh[0]
        w = (torch.randn(*sh, generator=g, dtype=torch.float64) * np.sqrt(2.0 / fan)).to(dtype)
        b = (0.1 * torch.randn(bias_len(i, sh), generator=g, dtype=torch.float64)).to(dtype)
        if i in ZERO_LAYERS:
            w[ZERO_CHANNEL] = 0.0
            b[ZERO_CHANNEL] = 0.0
        Ws.append(w)
        Bs.append(b)
    return Ws, Bs


def tied_input(N, C, H, W, g, dtype=torch.float32):
    coarse = torch.rand(N, C, (H + 5) // 6 + 1, (W + 9) // 10 + 1, generator=g, dtype=torch.float64).to(dtype)
    x = coarse.repeat_interleave(6, 2).repeat_interleave(10, 3)[:, :, 1:H + 1, 3:W + 3].contiguous()
    assert x.shape == (N, C, H, W)
    return x


def sprinkle(t):
    t.view(-1)[::13] = 0.0
    t.view(-1)[5::29] = -0.0
    return t


def forward_regions(Ws, Bs, x):
    """The forward of oracle/unet_ref.py in the NHWC layer functions of oracle/bf16_ref.py, keeping every region the backward reads.
    x: NCHW.  Returns (fwd, out NCHW)."""
    def act(t):
        return torch.max(0.2 * t, t)
    f = {'x': x.permute(0, 2, 3, 1), 'ea': [], 'eb': [], 'pool': [], 'up': [None] * 4, 'da': [None] * 4, 'db': [None] * 4}
    t = f['x']
    for l in range(5):
        f['ea'].append(act(R.conv3x3(t, Ws[2 * l]) + Bs[2 * l]))
        f['eb'].append(act(R.conv3x3(f['ea'][l], Ws[2 * l + 1]) + Bs[2 * l + 1]))
        if l < 4:
            f['pool'].append(R.maxpool_fwd(f['eb'][l]))
            t = f['pool'][l]
    t = f['eb'][4]
    for l in range(3, -1, -1):
        iu = B.up_index(l)
        f['up'][l] = R.convt_fwd(t, Ws[iu]) + Bs[iu]
        f['da'][l] = act(R.conv3x3(torch.cat([f['up'][l], f['eb'][l]], dim=3), Ws[iu + 1]) + Bs[iu + 1])
        f['db'][l] = act(R.conv3x3(f['da'][l], Ws[iu + 2]) + Bs[iu + 2])
        t = f['db'][l]
    out = torch.einsum('nyxc,oc->noyx', t, Ws[B.HEAD].reshape(-1, 32)) + Bs[B.HEAD][None, :, None, None]
    return f, out


def f32_rejects(got, y, bound):
    """an element is accepted only if err <= bound is true (NaN is rejected)"""
    return not bool(((got.double() - y).abs() <= bound).all())


def negative_controls(fwd, W, dout):
    """The rules of oracle/bwd_ref.py see the defects they exist for.  Everything here is arithmetic on reference tensors (float64, any
    device): the chained stages give each stage a plausible input, the defect is applied to the stage's own reference, and the rule must
    accept the true result as an fp32 / bf16 kernel would round it and reject the defective one."""
    terms = {}
    for step in B.stages(fwd, W, dout, taps=None, mags=True):
        for t in step:
            terms[t.name] = t
    vals = {n: t.value() for n, t in terms.items() if t.kind in ('g', 'head_g', 'pool')}
    assert bool((fwd['ea'][0][..., ZERO_CHANNEL] == 0).all()) and bool((fwd['eb'][1][..., ZERO_CHANNEL] == 0).all())

    # 1. a dW without one border row's contribution (conv9_2: 32 x 32 channels at full size; conv2_1 reads the pooled tensor)
    for name, g, xin in [('conv9_2.weight', vals['g_head'], fwd['da'][0]), ('conv2_1.weight', vals['d_ea1'], fwd['pool'][0])]:
        y, b = B.f32_rule(terms[name])
        assert not f32_rejects(y.float(), y, b), name
        assert f32_rejects(B.wgrad_without_border_row(g, xin).float(), y, b), name
        yb, bb = B.bf16_rule(terms[name])
        assert f32_rejects(B.wgrad_without_border_row(g, xin).float(), yb, bb), name
    # 2. / 4. the pool backward: no skip term; ties routed to the last window element.  The rule is equality (one select, one add, one multiply)
    for l in (0, 1):                                       # eb[0], eb[1]: the zeroed channel's windows are four-way ties
        a, dp, sk = terms['d_eb%d' % l].y
        ref32 = R.maxpool_bwd_f32(a, dp, sk)
        assert torch.equal(ref32, B.maxpool_bwd(a.float(), dp.float(), sk.float()).double())
        assert not torch.equal(ref32, B.pool_bwd_without_skip(a.float(), dp.float(), sk.float()).double()), l
        assert not torch.equal(ref32, B.pool_bwd_last_winner(a.float(), dp.float(), sk.float()).double()), l
        assert not torch.equal(R.rne_bf16(ref32), R.rne_bf16(B.pool_bwd_last_winner(a.float(), dp.float(), sk.float()).double())), l
    # 3. a slope of 1.0 at the exact zeros (the zeroed channel has nothing else)
    for name, a in [('d_da0', fwd['da'][0]), ('d_ea0', fwd['ea'][0]), ('d_ea4', fwd['ea'][4])]:
        t = terms[name]
        assert bool((a == 0).any()), name
        bad = t.y * B.slope_one_at_zero(a)
        for rule in (B.f32_rule, B.bf16_rule):
            y, m = rule(t)
            assert not f32_rejects(y.float(), y, m + R.U32 * y.abs()), name            # (the fp32 rounding of the reference itself)
            assert f32_rejects(bad.float(), y, m + R.U32 * y.abs()), name
        y, m = B.bf16_rule(t)
        assert bool(R.bf16_accept(R.bits_of(R.rne_bf16(y)), y, m)[0].all()), name
        assert not bool(R.bf16_accept(R.bits_of(R.rne_bf16(bad)), y, m)[0].all()), name
    # 5. d0 / skip swapped at a concatenating layer
    for l in (0, 3):
        yu, mu = B.f32_rule(terms['d_up%d' % l])
        ys, ms = B.f32_rule(terms['skip%d' % l])
        assert not f32_rejects(yu.float(), yu, mu + R.U32 * yu.abs()) and not f32_rejects(ys.float(), ys, ms + R.U32 * ys.abs())
        assert f32_rejects(ys.float(), yu, mu + R.U32 * yu.abs()) and f32_rejects(yu.float(), ys, ms + R.U32 * ys.abs()), l
        yb, mb = B.bf16_rule(terms['d_up%d' % l])
        assert not bool(R.bf16_accept(R.bits_of(R.rne_bf16(ys)), yb, mb)[0].all()), l
    # 6. one ulp at one bf16 element that is not near a rounding midpoint
    y, m = B.bf16_rule(terms['d_da1'])
    got = R.bits_of(R.rne_bf16(y))
    assert bool(R.bf16_accept(got, y, m)[0].all())
    far = ((y - R.rne_bf16(y)).abs() < 0.1 * R.ulp_bf16(y)) & ((got & 0x7FFF) < 0x7F00) & (y.abs() > 1e-6)
    idx = int(far.reshape(-1).nonzero()[0])
    one = got.clone().reshape(-1)
    one[idx] += 1
    assert not bool(R.bf16_accept(one.reshape(got.shape), y, m)[0].all())
    return terms
