"""float64 stage references of the U-Net backward (checker only; DESIGN.md sections 6 / 6a).

unet_backward<T> (csrc/unet.hip: one schedule for fp32 and bf16 tensors) is 30 stages that write an activation gradient and 23 that write a layer's dW / db.
stages() restates every one of them as the float64 layer functions of oracle/bf16_ref.py applied to
  * the forward's saved regions (`fwd`: x, ea[l], eb[l], pool[l], up[l], da[l], db[l], NHWC float64),
  * the weights as the kernels read them (`W`: reference layouts, float64 -- fp32 values, or their bf16 roundings for the bf16 engine),
  * and the stage's INPUT gradient: the backward's own tapped tensor where `taps` holds one (teacher-forced: include/eld_amd.h
    eld_debug_unet_grad_tap; an error cannot compound or cancel across stages), else the reference's own previous output (chained: the
    CPU proof against autograd, tests/test_backward_ref_cpu.py).
Each output comes back as a Term: the exact sum y of K products with mag2 = sum t^2 and mag1 = sum |t| (what the error models of
bf16_ref.margin / f32_ref.x3_bound take) and the slope the stage multiplies by, or, for the pool backward, the three operands of
bf16_ref.maxpool_bwd_f32.  f32_rule / bf16_rule turn a Term into (y64, bound).

Conventions, all autograd's of oracle/unet_ref.py (the CPU proof shows it): the gradient of max(0.2x, x) is read from the SAVED
post-activation value -- 1, 0.2 or 0.6 at an exact zero (bf16_ref.slope); a pool window with equal maxima sends its gradient to the first
of them in row-major order; the decoder's conv_1 reads cat[up, eb], so its backward-data splits into d_up (first half) and skip.

TAP: the stage names in the order of the tap's stage numbers.  LAYERS: the 23 layers in parameter order (dW = tensor 2i, db = 2i + 1).
The negative controls at the bottom are host-side arithmetic on reference tensors: what a defect of the named kind would have written."""
import torch

from oracle import bf16_ref as R
from oracle import f32_ref as F3

HEAD = 22


def chan(l):
    return 32 << l


def up_index(l):
    """index of upv(9-l); conv(9-l)_1 and conv(9-l)_2 follow it"""
    return 10 + 3 * (3 - l)


TAP = (['g_head'] + [n % l for l in range(4) for n in ('d_da%d', 'd_up%d', 'skip%d', 'd_src%d')]
       + [n for l in range(4, -1, -1) for n in (['d_ea%d' % l] + (['d_pool%d' % (l - 1), 'd_eb%d' % (l - 1)] if l else []))])
assert len(TAP) == 30
LAYERS = (['conv%d_%d' % (l + 1, k) for l in range(5) for k in (1, 2)]
          + [n % (9 - l) for l in range(3, -1, -1) for n in ('upv%d', 'conv%d_1', 'conv%d_2')] + ['conv10_1'])
assert len(LAYERS) == 23 and LAYERS[up_index(0)] == 'upv9' and LAYERS[HEAD] == 'conv10_1'


class Term:
    """One output tensor of a stage.  kind: 'g' (activation gradient of a conv / transposed-conv backward-data), 'head_g', 'dw', 'db',
    'head_dw', 'head_db', or 'pool' (then y = (act, d_pool, skip) and the rest is unused).  slope: what the stage multiplies y by, or None."""

    def __init__(self, name, kind, y, mag2=None, mag1=None, K=0, slope=None, slope_fn=R.slope):
        self.name, self.kind, self.y, self.mag2, self.mag1, self.K, self.slope, self.slope_fn = name, kind, y, mag2, mag1, K, slope, slope_fn

    def part(self, name, lo, hi):
        c = (lambda t: None if t is None else t[..., lo:hi])
        return Term(name, self.kind, c(self.y), c(self.mag2), c(self.mag1), self.K, c(self.slope))

    def value(self):
        """the exact float64 result (slope applied); pools: the float64 pool backward"""
        if self.kind == 'pool':
            return maxpool_bwd(*self.y, slope=self.slope_fn)
        return self.y if self.slope is None else self.y * self.slope


def _lin(name, kind, op, a, b, K, mags, slope=None):
    return Term(name, kind, op(a, b), op(a * a, b * b) if mags else None, op(a.abs(), b.abs()) if mags else None, K, slope)


def _colsum(name, kind, g, K, mags):
    d = tuple(range(g.dim() - 1))
    return Term(name, kind, g.sum(d), (g * g).sum(d) if mags else None, g.abs().sum(d) if mags else None, K)


# Weight gradients contract over every pixel into a small [Cout][Cin] matrix: as ONE matrix product (bf16_ref.conv3x3_wgrad) that is a single
# output tile with K = N H W -- a GEMM library gives it one workgroup.  Here the contraction runs per image row (a batch of N H products over the W
# pixels of a row) and the rows are summed: the same float64 sum in another order, and every CU has work.
def conv3x3_wgrad(g, x):
    """dW[co][ci][dy][dx] = sum_p g[p][co] x[p + (dy-1, dx-1)][ci]: g [N,H,W,Cout], x [N,H,W,Cin] -> [Cout,Cin,3,3]"""
    _, H, W, Co = g.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    gt = g.transpose(2, 3)                                    # [N,H,Cout,W]
    dw = torch.empty(Co, x.shape[3], 3, 3, dtype=g.dtype, device=g.device)
    for dy in range(3):
        for dx in range(3):
            dw[:, :, dy, dx] = torch.matmul(gt, xp[:, dy:dy + H, dx:dx + W, :]).sum((0, 1))
    return dw


def convt_wgrad(x, d):
    """dW[ci][co][a][b] = sum x[n,y,x,ci] d[n,2y+a,2x+b,co]: x [N,H,W,Cin], d [N,2H,2W,Cout] -> [Cin,Cout,2,2]"""
    N, H, W, Ci = x.shape
    d6 = d.reshape(N, H, 2, W, 2, d.shape[3])
    xt = x.transpose(2, 3)                                    # [N,H,Cin,W]
    dw = torch.empty(Ci, d.shape[3], 2, 2, dtype=x.dtype, device=x.device)
    for a in range(2):
        for b in range(2):
            dw[:, :, a, b] = torch.matmul(xt, d6[:, :, a, :, b, :]).sum((0, 1))
    return dw


def head_wgrad(d, a):
    """dW[o][c] = sum_p d[p][o] a[p][c]: NHWC tensors -> [out_ch, 32]"""
    return torch.matmul(d.transpose(2, 3), a).sum((0, 1))


def slope64(act):
    """bf16_ref.slope with the constants of float64 autograd (0.2, 0.6) instead of the kernels' fp32 ones: the CPU proof only"""
    one = torch.ones((), dtype=torch.float64, device=act.device)            # (Python scalars on both sides would give float32)
    return torch.where(act > 0, one, torch.where(act < 0, 0.2 * one, 0.6 * one))


def maxpool_bwd(act, dp, skip, slope=R.slope):
    """(route(dp) + skip) * slope(act) in the dtype of its operands: bf16_ref.maxpool_bwd_f32 without the casts to float32."""
    N, H, W, C = act.shape
    a = act.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    hit = a == a.amax(dim=-1, keepdim=True)
    win = hit & (torch.cumsum(hit.int(), dim=-1) == 1)
    routed = torch.where(win, dp.unsqueeze(-1), torch.zeros((), dtype=dp.dtype, device=dp.device))
    routed = routed.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    return (routed + skip if skip is not None else routed) * slope(act).to(dp.dtype)


def stages(fwd, W, dout, taps=None, mags=True, slope=R.slope):
    """Generator over the backward in its own order: yields (stage inputs consumed so far are final) one list of Terms per step --
    first the step's parameter gradients, then its activation gradients.  fwd / W / dout (NCHW) / taps: module docstring.  With taps the
    input of every step is taps[name]; without, the value() of the Term yielded before.  slope: bf16_ref.slope (the kernels' fp32 constants)
    or slope64."""
    have = {}
    S = slope

    def G(name):
        return taps[name] if taps is not None else have[name]

    def emit(terms):
        if taps is None:
            for t in terms:
                if t.kind in ('g', 'head_g', 'pool'):
                    have[t.name] = t.value()
        return terms

    N, H0, W0, _ = fwd['db'][0].shape
    OC = dout.shape[1]
    dn = dout.permute(0, 2, 3, 1)                               # NHWC
    wh = W[HEAD].reshape(OC, 32)
    K0 = N * H0 * W0
    yield emit([_lin('conv10_1.weight', 'head_dw', head_wgrad, dn, fwd['db'][0], K0, mags),
                _colsum('conv10_1.bias', 'head_db', dn, K0, mags),
                _lin('g_head', 'head_g', lambda d, w: d @ w, dn, wh, OC, mags, S(fwd['db'][0]))])
    g_in = 'g_head'
    for l in range(4):
        iu, C = up_index(l), chan(l)
        K = N * (H0 >> l) * (W0 >> l)
        g = G(g_in)
        yield emit([_lin(LAYERS[iu + 2] + '.weight', 'dw', conv3x3_wgrad, g, fwd['da'][l], K, mags),
                    _colsum(LAYERS[iu + 2] + '.bias', 'db', g, K, mags),
                    _lin('d_da%d' % l, 'g', R.conv3x3_bwd_data, g, W[iu + 2], 9 * C, mags, S(fwd['da'][l]))])
        g = G('d_da%d' % l)
        both = _lin('', 'g', R.conv3x3_bwd_data, g, W[iu + 1], 9 * C, mags)
        yield emit([_lin(LAYERS[iu + 1] + '.weight', 'dw', conv3x3_wgrad, g, torch.cat([fwd['up'][l], fwd['eb'][l]], dim=3), K, mags),
                    _colsum(LAYERS[iu + 1] + '.bias', 'db', g, K, mags),
                    both.part('d_up%d' % l, 0, C), both.part('skip%d' % l, C, 2 * C)])
        g = G('d_up%d' % l)
        src = fwd['eb'][4] if l == 3 else fwd['db'][l + 1]
        yield emit([_lin(LAYERS[iu] + '.weight', 'dw', convt_wgrad, src, g, K // 4, mags),
                    _colsum(LAYERS[iu] + '.bias', 'db', g, K, mags),
                    _lin('d_src%d' % l, 'g', R.convt_bwd_data, g, W[iu], 4 * C, mags, S(src))])
        g_in = 'd_src%d' % l
    for l in range(4, -1, -1):
        C = chan(l)
        K = N * (H0 >> l) * (W0 >> l)
        g = G(g_in)
        yield emit([_lin(LAYERS[2 * l + 1] + '.weight', 'dw', conv3x3_wgrad, g, fwd['ea'][l], K, mags),
                    _colsum(LAYERS[2 * l + 1] + '.bias', 'db', g, K, mags),
                    _lin('d_ea%d' % l, 'g', R.conv3x3_bwd_data, g, W[2 * l + 1], 9 * C, mags, S(fwd['ea'][l]))])
        g = G('d_ea%d' % l)
        first = [_lin(LAYERS[2 * l] + '.weight', 'dw', conv3x3_wgrad, g, fwd['x'] if l == 0 else fwd['pool'][l - 1], K, mags),
                 _colsum(LAYERS[2 * l] + '.bias', 'db', g, K, mags)]
        if l == 0:
            yield emit(first)
            return
        yield emit(first + [_lin('d_pool%d' % (l - 1), 'g', R.conv3x3_bwd_data, g, W[2 * l], 9 * C, mags)])
        yield emit([Term('d_eb%d' % (l - 1), 'pool', (fwd['eb'][l - 1], G('d_pool%d' % (l - 1)), G('skip%d' % (l - 1))), slope_fn=S)])
        g_in = 'd_eb%d' % (l - 1)


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def head_g_margin(t):
    """The head backward forms sum_o w[o][c] d[o] as an fp32 fma chain over the out_ch <= 16 planes in both engines: the accumulation model
    plus one rounding of the sum, as the forward head's output is bounded (tests/test_bf16_layers_gpu.py)."""
    return R.f32_bound(t.mag2, t.K) + R.C_ACC * R.U32 * t.y.abs()


def f32_rule(t):
    """Term of the fp32 engine (three-piece scheme) -> (y64, bound).  Gradients times zero-mean weights, and activations times zero-mean
    gradients, are zero-mean products: x3_bound as the single-layer zero-mean cases use it.  Bias gradients and the head are plain fp32 sums."""
    if t.kind in ('db', 'head_db', 'head_dw'):
        return t.y, R.f32_bound(t.mag2, t.K, t.mag1)
    m = head_g_margin(t) if t.kind == 'head_g' else F3.x3_bound(t.mag2, t.K, t.mag1)
    return (t.y, m) if t.slope is None else R.scale_ref(t.y, m, t.slope)


def bf16_rule(t):
    """Term of the bf16 engine -> (y64, margin or bound): activation gradients are accepted by bf16_ref.bf16_accept with this margin, the
    fp32 outputs (dW, db) are bounded by it."""
    if t.kind in ('dw', 'db', 'head_db', 'head_dw'):
        return t.y, R.f32_bound(t.mag2, t.K, t.mag1)
    m = head_g_margin(t) if t.kind == 'head_g' else R.margin(t.mag2, t.K)
    return (t.y, m) if t.slope is None else R.scale_ref(t.y, m, t.slope)


# ---- negative controls: what a defect would have written, from reference tensors only ----------------------------------------
def wgrad_without_border_row(g, x):
    """a 3x3 weight gradient whose contraction leaves out the first pixel row of the first image"""
    gd = g.clone()
    gd[0, 0] = 0.0
    return conv3x3_wgrad(gd, x)


def pool_bwd_without_skip(act, dp, skip):
    return maxpool_bwd(act, dp, None)


def pool_bwd_last_winner(act, dp, skip):
    """ties routed to the LAST maximum of the window instead of the first"""
    f = (lambda t: None if t is None else t.flip(1, 2))
    return maxpool_bwd(f(act), dp.flip(1, 2), f(skip)).flip(1, 2)


def slope_one_at_zero(act):
    """slopes of a kernel that treats an exact zero as positive"""
    return torch.where(act >= 0, 1.0, R.F32_02).double()
