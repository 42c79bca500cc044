"""GPU tests of the U-Net beyond Bayer: X-Trans 9 -> 9 (models/ELD_model.py:377-391 builds arch.unet(opt.channels, opt.channels)), the
wide head (5..16 output planes, csrc/unet_wide.hip), the bf16 network with 5..16 input planes (NHWC32 bf16 input on the generic bf16 conv),
and the X-Trans dataset pack with black level (dataset/sid_dataset.py:199-239).  Checker: oracle/unet_ref.py (float64 / float32 torch CPU)
and oracle/noise_ref.py (index map)."""
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import noise_ref as O    # noqa: E402  (checker only)
from oracle import unet_ref as U     # noqa: E402  (checker only)


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


@pytest.fixture(params=[0, 1, 2], ids=['fp32mfma', 'bf16x3', 'fp16x2'])
def algo(request, lib):
    prev = lib.eld_conv_fp32_algo(request.param)
    yield request.param
    lib.eld_conv_fp32_algo(prev)


def make_opt(tmp, **kw):
    d = dict(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', netG='unet', channels=9, stage_in='raw', stage_out='raw',
             lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, no_log=False, save_epoch_freq=2, model='eld_model')
    d.update(kw)
    return types.SimpleNamespace(**d)


def new_model(tmp, seed=2018, **kw):
    from eld_amd.model import ELDModel
    torch.manual_seed(seed)
    m = ELDModel()
    m.initialize(make_opt(tmp, **kw))
    return m


def split(flat, net):
    from eld_amd.unet import NAMES
    offs = net._offsets
    names = [n + s for n in NAMES for s in ('.weight', '.bias')]
    return {n: flat[a:b].view(p.shape) for n, a, b, p in zip(names, offs[:-1], offs[1:], net._plist)}


def assert_fp32_grads(grads, ref):
    """test_unet_all_gradients_vs_oracle's bounds: 1e-5 * (1 + max|ref|) and 2e-4 * max|ref| per tensor."""
    assert list(grads) == list(ref)
    for n, r in ref.items():
        err = float((grads[n].detach().cpu().double() - r).abs().max())
        rmax = float(r.abs().max())
        assert err <= 1e-5 * (1 + rmax), (n, err, rmax)
        assert err <= 2e-4 * rmax, (n, err, rmax)


def bf16_grad_failures(grads, ref):
    """test_unet_bf16_training_gradients' criteria: relative L2 <= 8 % and cosine >= 0.997 per tensor, median <= 3 %."""
    fails, rels = [], []
    for n, r in ref.items():
        r = r.reshape(-1)
        got = grads[n].detach().cpu().double().reshape(-1)
        rel = float((got - r).norm() / (r.norm() + 1e-30))
        cos = float(torch.dot(got, r) / (got.norm() * r.norm() + 1e-30))
        rels.append(rel)
        if not (rel <= 0.08 and cos >= 0.997):
            fails.append((n, rel, cos))
    if sorted(rels)[len(rels) // 2] > 0.03:
        fails.append(('median', sorted(rels)[len(rels) // 2], None))
    return fails


_ORACLE = {}


def oracle64(sd, x, t, loss, key):
    if key not in _ORACLE:
        _ORACLE[key] = U.loss_and_grads({k: v.double() for k, v in sd.items()}, x.double(), t.double(), loss=loss)
    return _ORACLE[key]


# ---- fp32 9 -> 9 through ELDModel.optimize_parameters, fused head and ELD_FUSED_HEAD=0 ---------------------------------------------
@pytest.mark.parametrize('fused', [1, 0], ids=['fused', 'unfused'])
@pytest.mark.parametrize('loss', ['l1', 'l2'])
@pytest.mark.parametrize('shape', [(1, 9, 16, 16), (3, 9, 48, 80), (1, 9, 64, 144)])
def test_xtrans_fp32_step_vs_oracle(lib, tmp_path, monkeypatch, shape, loss, fused, algo):
    monkeypatch.setenv('ELD_FUSED_HEAD', str(fused))
    m = new_model(tmp_path, loss=loss)
    assert m.fused_head == bool(fused) and m.netG.in_channels == 9 and m.netG.out_channels == 9
    sd = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x, t = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)
    out_ref, loss_ref, grads_ref = oracle64(sd, x, t, loss, (shape, loss))
    m.set_input({'input': x, 'target': t}, 'train')
    m.optimize_parameters()
    torch.cuda.synchronize()
    assert float((m.output.detach().cpu().double() - out_ref).abs().max()) <= 1e-5
    assert abs(m.get_current_errors()['Pixel'] - loss_ref) < 1e-6
    assert_fp32_grads(split(m.optimizer_G.grads, m.netG), grads_ref)


# ---- channel sweep: partial lane groups, OC = 16, wide inputs with a Bayer head -------------------------------------------------------
@pytest.mark.parametrize('cin,cout', [(1, 5), (9, 9), (16, 16), (8, 4), (4, 9)])
def test_channel_sweep_vs_oracle(lib, cin, cout):
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(cin * 17 + cout)
    net = UNetSeeInDark(cin, cout)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(cin + cout)
    x, t = torch.rand(2, cin, 32, 48, generator=g), torch.rand(2, cout, 32, 48, generator=g)
    out_ref, loss_ref, grads_ref = U.loss_and_grads({k: v.double() for k, v in sd.items()}, x.double(), t.double())
    net = net.cuda()
    # autograd path: plain forward, eld_l1 outside, backward with an explicit dout (the head's separate kernels)
    out = net(x.cuda())
    lv = torch.nn.functional.l1_loss(out, t.cuda())
    lv.backward()
    assert float((out.detach().cpu().double() - out_ref).abs().max()) <= 1e-5
    assert abs(float(lv) - loss_ref) < 1e-6
    assert_fp32_grads({n: p.grad for n, p in net.named_parameters()}, grads_ref)
    # fused head: output, loss and the head's backward in one pass
    loss_buf = torch.zeros(1, device='cuda')
    out1, key, _ = net._engine_forward_loss(x.cuda(), t.cuda(), loss_buf)
    g1 = net._engine_backward(None, key, tuple(x.shape)).clone()
    torch.cuda.synchronize()
    assert torch.equal(out1, out.detach())
    assert abs(float(loss_buf) - loss_ref) < 1e-6
    assert_fp32_grads(split(g1, net), grads_ref)


# ---- same bits: inference forward == fused training forward; state_dict round trip ----------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('oc', [9, 16])
def test_inference_and_fused_training_forward_are_the_same_bits(lib, oc, prec):
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(oc)
    net = UNetSeeInDark(oc, oc).cuda()
    bf16 = prec == 'bf16'
    net.inference_precision = net.train_precision = prec
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.rand(2, oc, 48, 80, device='cuda', generator=g)
    t = torch.rand(2, oc, 48, 80, device='cuda', generator=g)
    with torch.no_grad():
        out0 = net(x).clone()
    for mse in (False, True):
        loss_buf = torch.zeros(1, device='cuda')
        out1, key, _ = net._engine_forward_loss(x, t, loss_buf, bf16=bf16, mse=mse)
        net._engine_backward(None, key, tuple(x.shape))
        torch.cuda.synchronize()
        assert torch.equal(out1, out0), (mse, float((out1 - out0).abs().max()))
        d = out0.double() - t.double()
        ref = float((d * d).mean()) if mse else float(d.abs().mean())
        assert abs(float(loss_buf) - ref) <= 1e-6 * (1 + ref)
    out2, _, _ = net._engine_forward(x, save=True, bf16=bf16)          # plain training forward: same head kernel as inference
    assert torch.equal(out2, out0)
    net2 = UNetSeeInDark(oc, oc)
    net2.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    net2 = net2.cuda()
    net2.inference_precision = prec
    with torch.no_grad():
        assert torch.equal(net2(x), out0)


def test_fused_head_equals_the_separate_kernels_at_oc9(lib):
    """The wide head's training kernel and its forward + backward kernels give the same output and gradients, bit for bit (fp32, L1)."""
    from eld_amd.unet import UNetSeeInDark
    from eld_amd import _lib as L
    torch.manual_seed(9)
    net = UNetSeeInDark(9, 9).cuda()
    g = torch.Generator(device='cuda').manual_seed(2)
    shape = (2, 9, 96, 160)
    x = torch.rand(*shape, device='cuda', generator=g)
    t = torch.rand(*shape, device='cuda', generator=g)
    for bf16 in (False, True):
        out0, key, _ = net._engine_forward(x, save=True, bf16=bf16)
        out0 = out0.clone()
        dout = torch.empty_like(out0)
        loss0 = torch.zeros(1, device='cuda')
        ws = torch.empty(lib.eld_l1_workspace_bytes(), dtype=torch.uint8, device='cuda')
        L.check(lib.eld_l1_loss(L.dptr(out0), L.dptr(t), L.dptr(dout), L.dptr(loss0), L.dptr(ws), out0.numel(), 1.0, L.cur_stream()), 'loss')
        g0 = net._engine_backward(dout, key, shape).clone()
        loss1 = torch.zeros(1, device='cuda')
        out1, key, _ = net._engine_forward_loss(x, t, loss1, bf16=bf16)
        g1 = net._engine_backward(None, key, shape).clone()
        torch.cuda.synchronize()
        assert torch.equal(out1, out0)
        assert abs(float(loss1) - float(loss0)) <= 2e-6 * abs(float(loss0))
        assert torch.equal(g1, g0), bf16


# ---- bf16 with 5..16 input planes and wide heads --------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout', [(9, 9), (8, 4), (16, 4)])
def test_bf16_training_gradients_vs_oracle(lib, cin, cout):
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(7)
    net = UNetSeeInDark(cin, cout)
    sd = {k: v.detach().clone().double() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x, t = torch.rand(2, cin, 32, 48, generator=g), torch.rand(2, cout, 32, 48, generator=g)
    out_ref, loss_ref, grads_ref = U.loss_and_grads(sd, x.double(), t.double())
    net = net.cuda()
    net.train_precision = 'bf16'
    out = net(x.cuda())
    lv = torch.nn.functional.l1_loss(out, t.cuda())
    lv.backward()
    assert abs(float(lv) - loss_ref) < 2e-3
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert not bf16_grad_failures(grads, grads_ref), bf16_grad_failures(grads, grads_ref)
    # the fused bf16 training head: same output bits, gradients within the same criteria
    loss_buf = torch.zeros(1, device='cuda')
    out1, key, _ = net._engine_forward_loss(x.cuda(), t.cuda(), loss_buf, bf16=True)
    g1 = net._engine_backward(None, key, tuple(x.shape)).clone()
    torch.cuda.synchronize()
    assert torch.equal(out1, out.detach())
    assert abs(float(loss_buf) - loss_ref) < 2e-3
    assert not bf16_grad_failures(split(g1, net), grads_ref), bf16_grad_failures(split(g1, net), grads_ref)
    # negative control: a perturbed head weight must fail the same check
    net.conv10_1.weight.data.neg_()
    net.zero_grad()
    out2 = net(x.cuda())
    torch.nn.functional.l1_loss(out2, t.cuda()).backward()
    assert bf16_grad_failures({n: p.grad for n, p in net.named_parameters()}, grads_ref)


@pytest.mark.parametrize('cin,cout,shape', [(9, 9, (1, 32, 48)), (9, 9, (2, 64, 144)), (16, 4, (1, 176, 272)), (8, 16, (2, 64, 144))])
def test_bf16_inference_vs_fp32(lib, cin, cout, shape):
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(11)
    net = UNetSeeInDark(cin, cout).cuda()
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape[0], cin, shape[1], shape[2], generator=g)
    with torch.no_grad():
        ref32 = net(x.cuda())
        net.inference_precision = 'bf16'
        out = net(x.cuda())
        out2 = net(x.cuda())
        net.inference_precision = 'fp32'
        again32 = net(x.cuda())
    assert torch.equal(out, out2) and torch.equal(ref32, again32)
    assert not torch.equal(out, ref32)

    def psnr(a, b):
        mse = torch.mean((a.double() * 255 - b.double() * 255) ** 2)
        return float(10 * torch.log10(255.0 ** 2 / mse))
    assert psnr(out, ref32) >= 60.0, psnr(out, ref32)
    with torch.no_grad():
        ref64 = U.unet_forward(sd, x.double())
    assert psnr(out.cpu(), ref64) >= 60.0
    assert float((out.cpu().double() - ref64).abs().max()) < 2e-2


# ---- frame size: a Fuji X-T2 frame packed and cut to multiples of 16 -------------------------------------------------------------------
def test_xtrans_frame_1344x2000_step_vs_oracle(lib):
    """1 x 9 x 1344 x 2000, fp32 (default scheme): output, loss and all 46 gradients against the oracle with tests/test_parity_full_gpu.py's
    bounds (absolute against the float32 or the float64 oracle, relative 2e-4 of max|ref| or 8x the float32 oracle's own distance)."""
    from eld_amd import _lib as L
    from eld_amd.unet import UNetSeeInDark
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    torch.manual_seed(2018)
    shape = (1, 9, 1344, 2000)
    net = UNetSeeInDark(9, 9)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = torch.floor(65535.0 * torch.rand(*shape, generator=g) ** 2.2) / 65535.0
    t = torch.rand(*shape, generator=g)
    net = net.cuda()
    xd, td = x.cuda(), t.cuda()
    out, key, _ = net._engine_forward(xd, save=True)
    dout = torch.empty_like(out)
    loss = torch.zeros(1, device='cuda')
    ws = torch.empty(lib.eld_l1_workspace_bytes(), dtype=torch.uint8, device='cuda')
    L.check(lib.eld_l1_loss(L.dptr(out), L.dptr(td), L.dptr(dout), L.dptr(loss), L.dptr(ws), out.numel(), 1.0, L.cur_stream()), 'eld_l1_loss')
    grads = net._engine_backward(dout, key, shape)
    torch.cuda.synchronize()
    out, loss, grads = out.cpu(), float(loss), split(grads.cpu(), net)
    del net, xd, td, dout, key
    torch.cuda.empty_cache()
    out32, loss32, g32 = U.loss_and_grads(sd, x, t)
    try:    # the float64 oracle on the GPU's fp64 units through stock torch ops (checker only)
        o64, _, g64 = U.loss_and_grads({k: v.cuda().double() for k, v in sd.items()}, x.cuda().double(), t.cuda().double())
        r64 = (o64.cpu(), {k: v.cpu() for k, v in g64.items()})
    except Exception:     # pragma: no cover  (no fp64 convolution in this torch build)
        r64 = None
    assert abs(loss - loss32) <= 1e-6 * (1 + abs(loss32))
    fails = []

    def check(name, got, ref32, ref64):
        rmax = float(ref32.abs().max())
        bound = 1e-5 * (1.0 + rmax)
        ok = float((got - ref32).abs().max()) <= bound
        ref = ref64 if ref64 is not None else ref32.double()
        err = float((got.double() - ref).abs().max())
        if ref64 is not None:
            ok = ok or err <= bound
        rok = err <= 2e-4 * float(ref.abs().max())
        if not rok and ref64 is not None:
            rok = err <= 8.0 * float((ref32.double() - ref64).abs().max())
        if not (ok and rok):
            fails.append((name, err, rmax))
    check('output', out, out32, r64[0] if r64 else None)
    for n in g32:
        check(n, grads[n], g32[n], r64[1][n] if r64 else None)
    assert not fails, fails


# ---- ELDModel end to end: X-Trans noise model, on-device synthesis, Adam -------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_eldmodel_xtrans_end_to_end(lib, tmp_path, prec):
    from eld_amd.noise import NoiseModel
    m = new_model(tmp_path, precision=prec)
    assert m.netG.in_channels == 9 and m.netG.out_channels == 9
    m.set_noise_model(NoiseModel(model='Pg', cfa='xtrans'))
    sd = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-4, betas=(0.9, 0.999))
    np.random.seed(0)
    for it in range(3):
        g = torch.Generator().manual_seed(it)
        t = torch.floor(65535 * torch.rand(2, 9, 32, 48, generator=g) ** 2.2) / 65535
        m.set_input({'target': t}, 'train')
        x = m.input.detach().cpu().clone()                      # the injected noisy input (on-device sampler + clip)
        assert x.shape == t.shape and float(x.min()) >= 0 and float(x.max()) <= 1 and not torch.equal(x, t)
        m.optimize_parameters()
        loss = m.get_current_errors()['Pixel']
        opt.zero_grad()
        lref = torch.nn.functional.l1_loss(U.unet_forward(params, x), t)
        lref.backward()
        opt.step()
        tol = 2e-6 * (it + 1) + 1e-6 if prec == 'fp32' else 2e-3
        assert abs(loss - float(lref)) < tol, (it, loss, float(lref))
    got = m.netG.state_dict()
    d_all, r_all = [], []
    for k, v in params.items():
        d_ref = (v.detach() - sd[k]).reshape(-1)
        d_got = (got[k].cpu() - sd[k]).reshape(-1)
        if prec == 'fp32':
            assert float((d_got - d_ref).abs().max()) < 3e-5, k
        else:   # bf16 gradients: Adam's early updates are ~lr * sign(grad); only tiny-gradient elements may flip
            cos = float(torch.dot(d_got.double(), d_ref.double()) / (d_got.double().norm() * d_ref.double().norm() + 1e-30))
            assert cos >= 0.8, (k, cos)
        d_all.append(d_got)
        r_all.append(d_ref)
    if prec == 'bf16':
        a, b = torch.cat(d_all).double(), torch.cat(r_all).double()
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) >= 0.95


def test_eldmodel_channel_range_errors(lib, tmp_path):
    with pytest.raises(ValueError):
        new_model(tmp_path, in_channels=17, precision='bf16')
    with pytest.raises(ValueError):
        new_model(tmp_path, channels=17)
    m = new_model(tmp_path, in_channels=16, channels=4, precision='bf16')           # a 4-frame Bayer burst in bf16
    assert m.netG.in_channels == 16 and m.netG.out_channels == 4


# ---- X-Trans pack with black level ----------------------------------------------------------------------------------------------------
def pack_ref(m, black=1024, white=16383):
    return O.pack_raw_xtrans(np.clip((m.astype(np.float32) - black) / np.float32(white - black), 0, 1))


@pytest.mark.parametrize('H,W', [(60, 96), (100, 136), (67, 71), (5, 40)])
def test_pack_raw_xtrans_bit_exact(lib, H, W):
    from eld_amd.noise import pack_raw_xtrans
    rng = np.random.default_rng(H * W)
    m = rng.integers(0, 65536, size=(H, W), dtype=np.uint16)
    got = pack_raw_xtrans(m)
    ref = pack_ref(m)
    assert got.dtype == np.float32 and got.shape == ref.shape == (9, 2 * (H // 6), 2 * (W // 6))
    assert np.array_equal(got, ref)


def test_pack_raw_xtrans_batch_codes_and_tensor_input(lib):
    from eld_amd.noise import pack_raw_xtrans
    rng = np.random.default_rng(7)
    # every one of the 65 536 codes inside the packed area of one mosaic (258 = 43 whole cells per side)
    m0 = rng.integers(0, 65536, size=(258, 258), dtype=np.uint16)
    m0.reshape(-1)[:65536] = rng.permutation(65536).astype(np.uint16)
    batch = np.stack([m0, rng.integers(0, 16384, size=(258, 258), dtype=np.uint16), rng.integers(900, 1200, size=(258, 258), dtype=np.uint16)])
    got = pack_raw_xtrans(batch)
    assert got.shape == (3, 9, 86, 86)
    for i in range(3):
        assert np.array_equal(got[i], pack_ref(batch[i])), i
    t = torch.from_numpy(batch.view(np.int16)).cuda()              # CUDA tensor input (int16 view of the codes): CUDA tensor out
    gt = pack_raw_xtrans(t, black_level=512, white_point=15000)
    assert gt.is_cuda and gt.shape == (3, 9, 86, 86)
    for i in range(3):
        assert np.array_equal(gt[i].cpu().numpy(), pack_ref(batch[i], 512, 15000)), i
    assert np.array_equal(pack_raw_xtrans(t[1])[None].cpu().numpy(), got[1:2])


# ---- metrics: tensor2im's (H, W, 9) layout ---------------------------------------------------------------------------------------------
def test_quality_assess_reads_nine_plane_hwc(lib):
    from eld_amd.metrics import quality_assess
    g = torch.Generator().manual_seed(0)
    a = torch.rand(9, 40, 48, generator=g) * 255
    b = (a + 8 * torch.rand(9, 40, 48, generator=g)).clamp(0, 255)
    chw = quality_assess(a.numpy(), b.numpy())
    hwc = quality_assess(a.permute(1, 2, 0).numpy(), b.permute(1, 2, 0).numpy())
    assert hwc == chw
