"""float64 reference of the bf16 network's arithmetic (checker only).

The bf16 U-Net stores activations, activation gradients and packed weights as bfloat16 rounded to nearest even, and accumulates, adds its
bias and writes parameter gradients and the network output in fp32.  This module rebuilds that contract in float64:

  * rne_bf16: ONE rounding of a float64 value to bf16, ties to even (a detour through float32 rounds twice);
  * first_cut2 / wgrad_cut2: the two-piece cuts of the first layer's fp32 operands (csrc/conv_first.hip);
  * conv3x3 / conv3x3_bwd_data / conv3x3_wgrad / convt_*: the layers in float64 on NHWC tensors as GEMMs per tap (products of bf16
    operands are exact, float64 sums), also applied to squared operands for the error model;
  * bf16_accept: the acceptance rule of a bf16 output; f32_bound: the elementwise bound of an fp32 output.

Accumulation-error model (fp32, K products t_k summed in any order):  m = C_ACC * 2^-24 * (sqrt(K) * ||t||_2 + |bias|),
||t||_2 = sqrt(conv(x^2, w^2)).  A bf16 output is accepted when it equals rne_bf16(y64) or when [y64 - m, y64 + m] meets its rounding
cell -- for m below half an ulp: the other neighbour of y64, with y64 within m of the midpoint between the two.  +0 and -0 compare
equal; nothing else is exempt."""
import torch

C_ACC = 4.0                       # constant of the accumulation-error model (module docstring)
U32 = 2.0 ** -24                  # unit roundoff of fp32
F32_02 = float(torch.tensor(0.2, dtype=torch.float32))      # the LeakyReLU slopes as the kernels hold them (fp32 constants)
F32_06 = float(torch.tensor(0.6, dtype=torch.float32))
BF16_MAX = float.fromhex('0x1.fep127')


def _ulp_scale(t):
    """2^-k with 2^k = one bf16 ulp at t (bf16 subnormals: 2^-133), from the float64 exponent bits: exact."""
    e = ((t.view(torch.int64) >> 52) & 0x7FF) - 1023
    k = torch.clamp(e, min=-126) - 7
    return ((1023 - k) << 52).view(torch.float64)


def rne_bf16(t):
    """float64 tensor -> float64 tensor of bf16 values, rounded once to nearest, ties to even (subnormals, +-0, overflow to inf).
    Exact operations only: power-of-two scaling and torch.round (halves to even)."""
    t = t.double()
    s = _ulp_scale(t)
    r = torch.round(t * s) / s
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, float('inf')), t), r)
    return torch.where(torch.isnan(t), t, r)


def trunc_bf16(t):
    """float64 -> bf16 value truncated toward zero (the rounding the contract forbids; negative controls)."""
    t = t.double()
    s = _ulp_scale(t)
    return torch.trunc(t * s) / s


def ulp_bf16(t):
    return 1.0 / _ulp_scale(t.double())


def f64_of_bits(bits):
    """bf16 bit patterns (any integer dtype, low 16 bits used) -> float64 values."""
    b = (bits.to(torch.int32) & 0xFFFF) << 16
    return b.view(torch.float32).double()


def bits_of(v):
    """float64 tensor holding bf16 values -> int32 bit patterns 0 .. 0xFFFF."""
    return (v.float().contiguous().view(torch.int32) >> 16) & 0xFFFF


def _key(bits):
    b = bits.to(torch.int64) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where((b & 0x8000) != 0, -mag, mag)          # monotone in the value; +0 and -0 -> 0


def _val_of_key(k):
    return f64_of_bits(torch.where(k < 0, (-k) | 0x8000, k))


def _trunc_f32(v):
    return (v.view(torch.int32) & -65536).view(torch.float32)


def first_cut2(v):
    """conv_first.hip first_cut<2>: hi = v truncated to bf16, lo = (v - hi) truncated (fp32 arithmetic, exact)."""
    v = v.float().contiguous()
    hi = _trunc_f32(v)
    lo = _trunc_f32((v - hi).contiguous())
    return hi.double(), lo.double()


def wgrad_cut2(v):
    """conv_first.hip weight-gradient staging: hi = v truncated to bf16, lo = v - hi rounded to nearest even."""
    v = v.float().contiguous()
    hi = _trunc_f32(v)
    return hi.double(), rne_bf16((v - hi).double())


def slope(act):
    """d max(0.2x, x) / dx from the saved (rounded) post-activation value: 1, 0.2f, or 0.6f at zero (+0 and -0)."""
    return torch.where(act > 0, 1.0, torch.where(act < 0, F32_02, F32_06)).double()


# ---- layers in float64 on NHWC tensors ----------------------------------------------------------------------------------
def _pad1(x):
    return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))


def conv3x3(x, w):
    """x [N,H,W,Cin], w [Cout,Cin,3,3] -> [N,H,W,Cout] (zero padding 1 around every image)."""
    _, H, W, _ = x.shape
    xp = _pad1(x)
    y = None
    for dy in range(3):
        for dx in range(3):
            t = xp[:, dy:dy + H, dx:dx + W, :] @ w[:, :, dy, dx].t()
            y = t if y is None else y + t
    return y


def conv3x3_bwd_data(g, w):
    """gradient of conv3x3's input: g [N,H,W,Cout], w [Cout,Cin,3,3] -> [N,H,W,Cin]."""
    return conv3x3(g, w.flip(2, 3).transpose(0, 1))


def conv3x3_wgrad(g, x):
    """dW[co][ci][dy][dx] = sum_p g[p][co] x[p + (dy-1, dx-1)][ci]."""
    _, H, W, Co = g.shape
    Ci = x.shape[3]
    xp = _pad1(x)
    g2 = g.reshape(-1, Co).t()
    dw = torch.empty(Co, Ci, 3, 3, dtype=torch.float64, device=g.device)
    for dy in range(3):
        for dx in range(3):
            dw[:, :, dy, dx] = g2 @ xp[:, dy:dy + H, dx:dx + W, :].reshape(-1, Ci)
    return dw


def convt_fwd(x, w):
    """nn.ConvTranspose2d(k=2, s=2) without bias: x [N,H,W,Cin], w [Cin,Cout,2,2] -> [N,2H,2W,Cout]."""
    N, H, W, _ = x.shape
    return torch.einsum('nyxi,ioab->nyaxbo', x, w).reshape(N, 2 * H, 2 * W, w.shape[1])


def convt_bwd_data(d, w):
    """d [N,2H,2W,Cout], w [Cin,Cout,2,2] -> [N,H,W,Cin]."""
    N, H2, W2, Co = d.shape
    return torch.einsum('nyaxbo,ioab->nyxi', d.reshape(N, H2 // 2, 2, W2 // 2, 2, Co), w)


def convt_wgrad(x, d):
    """dW[ci][co][a][b] = sum x[n,y,x,ci] d[n,2y+a,2x+b,co]."""
    N, H, W, _ = x.shape
    return torch.einsum('nyxi,nyaxbo->ioab', x, d.reshape(N, H, 2, W, 2, d.shape[3]))


def maxpool_fwd(x):
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))


def maxpool_bwd_f32(act, dp, skip):
    """The bf16 pool backward as the kernel evaluates it: ((routed dp) + skip) * slope(act), one fp32 rounding per operation, the winner =
    the first maximum of the window in row-major order (as the fp32 pool).  Returns the fp32 results as float64 (round with rne_bf16)."""
    N, H, W, C = act.shape
    a = act.float().reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    hit = a == a.amax(dim=-1, keepdim=True)
    win = hit & (torch.cumsum(hit.int(), dim=-1) == 1)
    routed = torch.where(win, dp.float().unsqueeze(-1), torch.zeros((), dtype=torch.float32, device=act.device))
    routed = routed.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    s = routed + skip.float() if skip is not None else routed
    return (s * slope(act).float()).double()


# ---- acceptance ---------------------------------------------------------------------------------------------------------
def margin(mag2, K, bias=None):
    """fp32 accumulation margin of outputs with K product terms of squared 2-norm mag2 (= conv(x^2, w^2))."""
    m = C_ACC * U32 * (K ** 0.5) * mag2.clamp_min(0).sqrt()
    if bias is not None:
        m = m + C_ACC * U32 * bias.double().abs()
    return m


def lrelu_ref(y, m):
    """max(0.2f * y, y) of an exact pre-activation y with margin m -> (value, margin): the fp32 product adds one rounding; within m of zero
    the kernel may be on either branch (both values lie within m of 0)."""
    z = torch.where(y < 0, y * F32_02, y)
    mz = torch.where(y < 0, m * F32_02 + z.abs() * U32, m)
    return z, torch.where(y.abs() <= m, torch.maximum(mz, m), mz)


def scale_ref(y, m, s):
    """y * s (an fp32 multiply by the slope s) with margin m."""
    z = y * s
    return z, m * s + torch.where(s != 1.0, z.abs() * U32, torch.zeros_like(z))


def bf16_accept(got_bits, y, m):
    """Per element: got is rne_bf16(y), or [y - m, y + m] meets got's rounding cell.  Returns (ok, flipped): flipped = accepted without
    being rne_bf16(y) (near-tie flips of the fp32 summation order)."""
    y = y.double()
    g = f64_of_bits(got_bits)
    exact = g == rne_bf16(y)                                  # +0 == -0
    k = _key(got_bits)
    lo = (g + _val_of_key(k - 1)) * 0.5
    hi = (g + _val_of_key(k + 1)) * 0.5
    ok = exact | ((y + m >= lo) & (y - m <= hi))
    return ok, ok & ~exact


def f32_bound(mag2, K, mag1=None):
    """Elementwise bound of an fp32 output: the model of margin(); with mag1 = sum |t_k|, never looser than the fp32 layer tests'
    2e-6 (1 + sum |t_k|)."""
    b = C_ACC * U32 * (K ** 0.5) * mag2.clamp_min(0).sqrt()
    return b if mag1 is None else torch.minimum(b, 2e-6 * (1.0 + mag1))
