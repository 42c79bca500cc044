"""CPU tests of the U-Net's channel range beyond Bayer (X-Trans: 9 -> 9, models/ELD_model.py:377-391; burst inputs): parameter
layout and workspace sizing through the C ABI, which need no device."""
import pytest

torch = pytest.importorskip('torch')

from oracle import unet_ref as U     # noqa: E402  (checker only)


@pytest.mark.parametrize('cin,cout', [(9, 9), (16, 16), (1, 5), (4, 9), (8, 4)])
def test_param_offsets_match_the_torch_module(eld_lib, cin, cout):
    from eld_amd.unet import NAMES, param_offsets
    offs = param_offsets(cin, cout)
    assert len(offs) == 47
    sd = U.seeded_state_dict(cin, cout)
    keys = [n + s for n in NAMES for s in ('.weight', '.bias')]
    assert keys == list(sd.keys())                                   # state_dict order of the reference module
    sizes = [b - a for a, b in zip(offs[:-1], offs[1:])]
    assert sizes == [sd[k].numel() for k in keys]
    assert offs[0] == 0 and offs[-1] == sum(v.numel() for v in sd.values())
    assert sizes[1] == 32 and sizes[0] == 32 * cin * 9 and sizes[-2] == cout * 32 and sizes[-1] == cout


def test_module_builds_for_xtrans_on_the_host(eld_lib):
    """UNetSeeInDark(9, 9) constructs (flat buffer laid out by the library) and loads a reference-shaped state_dict."""
    from eld_amd.unet import UNetSeeInDark
    net = UNetSeeInDark(9, 9)
    assert net.flat_params.numel() == param_count(9, 9)
    sd = U.seeded_state_dict(9, 9)
    net.load_state_dict(sd)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k


def param_count(cin, cout):
    return sum(v.numel() for v in U.seeded_state_dict(cin, cout).values())


def test_channel_range_of_the_abi(eld_lib):
    import ctypes as C
    offs = (C.c_int64 * 47)()
    for cin, cout in [(9, 9), (16, 16), (1, 16), (16, 1)]:
        assert eld_lib.eld_unet_param_offsets(cin, cout, offs) == 0
        assert eld_lib.eld_unet_workspace_bytes(1, 16, 16, cin, cout) > 0
        assert eld_lib.eld_unet_workspace_bytes(8, 1344, 2000, cin, cout) > 0
    for cin, cout in [(4, 17), (0, 4), (17, 4), (4, 0)]:
        assert eld_lib.eld_unet_param_offsets(cin, cout, offs) == -1
        assert eld_lib.eld_unet_workspace_bytes(1, 16, 16, cin, cout) == 0


# eld_unet_workspace_bytes of the Bayer plans as the library computed them before the head took more than 4 planes: the quad-lane head
# and its partial buffers are unchanged, so these stay byte-identical
BAYER_WS = {
    (1, 16, 16): 129025024,
    (3, 48, 80): 169023488,
    (1, 64, 144): 155264256,
    (8, 512, 512): 4126894336,
    (8, 1344, 2000): 40514734336,
}


@pytest.mark.parametrize('shape', sorted(BAYER_WS))
@pytest.mark.parametrize('cout', [4, 3])
def test_bayer_workspace_is_unchanged(eld_lib, shape, cout):
    assert eld_lib.eld_unet_workspace_bytes(*shape, 4, cout) == BAYER_WS[shape]


def test_wide_head_workspace_grows_with_the_planes(eld_lib):
    """The head's partials are 33 * OC floats per block for OC > 4 (dW 32 OC + db OC): the workspace is monotone in OC and the in_ch
    side (NHWC16 / NHWC32 bf16 conversion region) does not depend on in_ch."""
    ws = [eld_lib.eld_unet_workspace_bytes(1, 16, 16, 4, oc) for oc in range(1, 17)]
    assert all(a <= b for a, b in zip(ws, ws[1:]))
    assert ws[8] > ws[3]
    assert eld_lib.eld_unet_workspace_bytes(1, 16, 16, 9, 9) == eld_lib.eld_unet_workspace_bytes(1, 16, 16, 4, 9)
