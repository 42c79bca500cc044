"""CPU proof of the backward's stage references (oracle/bwd_ref.py), which tests/test_backward_layers_gpu.py applies to the kernels' own tensors.

On a tiny float64 network (1 x 4 x 16 x 16, with the zeroed channel and the tied input of tests/backward_cases.py) the stages are CHAINED
from dout down to conv1_1 and every one of the 46 parameter gradients is compared with torch autograd of oracle/unet_ref.py in float64, to
1e-12 of the tensor's largest entry.  That shows the stage list is complete (a missing or mis-wired stage changes every gradient below it)
and that the conventions are autograd's: the slope 0.6 at an exact zero, the first maximum of a tied pool window, cat[up, eb] at the
decoder's conv_1.  The negative controls of the GPU file run here too, on the same reference tensors."""
import pytest

torch = pytest.importorskip('torch')

from oracle import bwd_ref as B        # noqa: E402
from oracle import unet_ref as U       # noqa: E402

import backward_cases as BC            # noqa: E402


@pytest.fixture(scope='module')
def tiny():
    g = torch.Generator().manual_seed(2018)
    Ws, Bs = BC.make_params(4, 4, g, torch.float64)
    x = BC.tied_input(1, 4, 16, 16, g, torch.float64)
    dout = BC.sprinkle(torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float64))
    fwd, out = BC.forward_regions(Ws, Bs, x)
    return Ws, Bs, x, dout, fwd, out


def test_stage_list_matches_the_tap_numbering():
    assert B.TAP[0] == 'g_head' and B.TAP[1:5] == ['d_da0', 'd_up0', 'skip0', 'd_src0'] and B.TAP[16] == 'd_src3'
    assert B.TAP[17:20] == ['d_ea4', 'd_pool3', 'd_eb3'] and B.TAP[29] == 'd_ea0' and len(set(B.TAP)) == 30
    assert B.LAYERS[:2] == ['conv1_1', 'conv1_2'] and B.LAYERS[10:13] == ['upv6', 'conv6_1', 'conv6_2'] and B.LAYERS[21] == 'conv9_2'


def test_chained_stages_equal_autograd(tiny):
    Ws, Bs, x, dout, fwd, out = tiny
    sd = {}
    for i, n in enumerate(B.LAYERS):
        sd[n + '.weight'], sd[n + '.bias'] = Ws[i], Bs[i]
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_out = U.unet_forward(p, x)
    assert float((ref_out.detach() - out).abs().max()) <= 1e-12 * float(out.abs().max())
    (ref_out * dout).sum().backward()
    # the inputs hold what they are meant to exercise
    assert bool((fwd['eb'][0][..., BC.ZERO_CHANNEL] == 0).all()) and not bool(torch.signbit(fwd['eb'][0][..., BC.ZERO_CHANNEL]).any())
    e = fwd['eb'][0][0, :, :, :BC.ZERO_CHANNEL]
    w4 = torch.stack([e[0::2, 0::2], e[0::2, 1::2], e[1::2, 0::2], e[1::2, 1::2]])
    assert bool(((w4 == w4.amax(0)).sum(0) >= 2).any()), 'no pool window with a tied maximum outside the zeroed channel'
    seen_g, seen_p = [], {}
    for step in B.stages(fwd, Ws, dout, taps=None, mags=False, slope=B.slope64):
        for t in step:
            if t.kind in ('g', 'head_g', 'pool'):
                seen_g.append(t.name)
            else:
                seen_p[t.name] = t.value()
    assert sorted(seen_g) == sorted(B.TAP)                     # the 30 activation gradients of the tap, each once
    assert sorted(seen_p) == sorted(sd)                        # the 46 parameter gradients
    for n, got in seen_p.items():
        ref = p[n].grad
        got = got.reshape(ref.shape)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), n


def test_negative_controls_are_rejected(tiny):
    Ws, Bs, x, dout, fwd, out = tiny
    BC.negative_controls(fwd, Ws, dout)
