"""CPU proof of the fp32 error model (oracle/f32_ref.py): no GPU.

An exact emulation of the three-piece scheme -- the six kept products of cut3 pieces, exact in float64, added to an fp32 accumulator as 8-term
blocks (half an MFMA, the unit the instruction rounds at) in a shuffled order, fp32 bias add and LeakyReLU -- must pass x3_bound against the float64 layer at K = 288, 576, 2304 on
zero-mean and on exposure operands.  Every defect the bound exists for must fail it (host tensors only): any one of the six products
removed (exposure operands), a border row / column not zero-padded, a row swapped across the seam of two images, a weight gradient without one
tile row (zero-mean operands too), the bias rounded to bf16, slope 1.0 instead of 0.6 at exact zeros.

Not a control: a2 formed by rounding instead of truncation.  The three pieces still add up to the operand exactly and the dropped products
only shrink (|a3| <= half an ulp of a2 instead of one): the six-product sum of the rounded cut is as close to the exact product as the
truncated one's, within the same 2^-23 sum |t| (test_rounded_a2_is_not_distinguishable); a kernel that rounded a2 would be no less accurate
and no bound on the result can tell the two apart."""
import pytest

torch = pytest.importorskip('torch')

from oracle import bf16_ref as R     # noqa: E402
from oracle import f32_ref as F3     # noqa: E402

N, H, W, CO = 2, 6, 7, 8
KS = [288, 576, 2304]
_CACHE = {}


def patches(x):
    """x [N,H,W,C] -> [N*H*W, 9C], zero padding 1 (column order (dy, dx, c))."""
    n, h, w, c = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.cat([xp[:, dy:dy + h, dx:dx + w, :] for dy in range(3) for dx in range(3)], dim=3).reshape(n * h * w, 9 * c)


def wmat(w):
    """w [Cout,Cin,3,3] -> [9 Cin, Cout] in the column order of patches()."""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


def emulate(pm, wm, g, kept=F3.KEPT, round_a2=False, terms=F3.MFMA_TERMS):
    """What an MFMA kernel of the scheme computes, in a shuffled order: k is cut into blocks of F3.MFMA_TERMS = 8 (half a
    v_mfma_f32_32x32x16_bf16: the instruction rounds its accumulator after each 8-term half, oracle/f32_ref.py), every (block, product) pair adds
    its exact 8-term dot product to the fp32 accumulator with one rounding.  pm [P,K] fp32, wm [K,Co] fp32 -> fp32 [P,Co].  (One rounding per
    single product is not a model of these kernels: a low-order product is below half an ulp of the running sum and would be absorbed whole.)"""
    A, Wc = F3.cut3(pm, round_a2), F3.cut3(wm, round_a2)
    K = pm.shape[1]
    perm = torch.randperm(K, generator=g)
    T = terms
    nb = (K + T - 1) // T
    acc = torch.zeros(pm.shape[0], wm.shape[1], dtype=torch.float32)
    for o in torch.randperm(len(kept) * nb, generator=g).tolist():
        i, j = kept[o // nb]
        idx = perm[T * (o % nb):T * (o % nb) + T]
        acc = (acc.double() + A[i][:, idx] @ Wc[j][idx, :]).float()
    return acc


def case(K, kind):
    """One layer per (K, kind), computed once: operands, the emulated fp32 output and the float64 reference with its bound."""
    key = (K, kind)
    if key in _CACHE:
        return _CACHE[key]
    C = K // 9
    g = torch.Generator().manual_seed(K + (kind == 'exposure'))
    if kind == 'exposure':
        x = F3.exposure_operands((N, H, W, C), g)
        w = F3.exposure_operands((CO, C, 3, 3), g, 2.0 ** -(K.bit_length()))
    else:
        x = torch.randn(N, H, W, C, generator=g)
        w = torch.randn(CO, C, 3, 3, generator=g) / K ** 0.5
    x.view(-1)[::13] = 0.0
    x.view(-1)[5::29] = -0.0
    b = 0.5 * torch.randn(CO, generator=g)
    pre = emulate(patches(x), wmat(w), g)                                  # before the bias
    got = (pre.double() + b.double()).float().reshape(N, H, W, CO)
    c = dict(K=K, kind=kind, x=x, w=w, b=b, g=g, got=got, noise=None)
    c['y'], c['bound'] = ref(c, x, b)
    c['noise'] = got.double() - c['y']                                     # the honest rounding error, re-used by the controls
    _CACHE[key] = c
    return c


def ref(c, x, b):
    xd, wd = x.double(), c['w'].double()
    s = R.conv3x3(xd, wd)
    bound = F3.x3_bound(R.conv3x3(xd * xd, wd * wd), c['K'], R.conv3x3(xd.abs(), wd.abs()), b, s if c['kind'] == 'exposure' else None)
    return s + b.double(), bound


def inside(got, y, bound):
    return bool(((got.double() - y).abs() <= bound).all())


BOTH = [(K, kind) for K in KS for kind in ('random', 'exposure')]


def test_cut3_is_exact_and_as_the_kernel_header_states():
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(4096, generator=g) * torch.exp2(torch.randint(-20, 20, (4096,), generator=g).float()),
                   F3.exposure_operands((4096,), g), torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -120, 3.0e38])])
    a1, a2, a3 = F3.cut3(v)
    assert bool((a1 + a2 + a3 == v.double()).all())
    for p in (a1, a2, a3):
        assert bool((R.rne_bf16(p) == p).all())                            # every piece is a bf16 value
    assert bool((a1 == R.trunc_bf16(v.double())).all()) and bool((a2 == R.trunc_bf16(v.double() - a1)).all())
    assert bool((a2.abs() <= 2.0 ** -7 * v.double().abs()).all()) and bool((a3.abs() <= 2.0 ** -15 * v.double().abs()).all())
    e1, e2, e3 = F3.cut3(F3.exposure_operands((4096,), g, 2.0 ** -5))
    assert bool((e1 == 2.0 ** -5).all()) and bool((e2 >= 1.5 * 2.0 ** -14).all()) and bool((e3 >= 2.0 ** -22).all())
    assert bool((e2 < 2.0 ** -8 * e1).all()) and bool((e3 < 2.0 ** -16 * e1).all())
    terms = F3.x3_product_terms(v[:4096], v[:4096].flip(0))
    drop = F3.x3_dropped_terms(v[:4096], v[:4096].flip(0))
    assert len(terms) == 6 and bool((sum(terms) + sum(drop) == v[:4096].double() * v[:4096].flip(0).double()).all())


@pytest.mark.parametrize('K,kind', BOTH)
def test_exact_emulation_passes_the_bound(K, kind):
    c = case(K, kind)
    r = float((c['noise'].abs() / c['bound']).max())
    print('K %d %s: worst err / bound %.3f' % (K, kind, r))
    assert inside(c['got'], c['y'], c['bound']), r
    z, mz = R.lrelu_ref(c['y'], c['bound'])                                # the fp32 epilogue: max(0.2f * v, v)
    v = c['got']
    act = torch.maximum(torch.tensor(R.F32_02, dtype=torch.float32) * v, v)
    assert inside(act, z, mz)


def test_dropped_products_of_the_exposure_operands_keep_the_header_claim():
    """a2w3 + a3w2 + a3w3 <= (2^-24 + 2^-24 + 2^-32) |a w| termwise on the exposure operands; a truncating cut alone only gives 2^-21."""
    g = torch.Generator().manual_seed(5)
    a, w = F3.exposure_operands((1 << 14,), g), F3.exposure_operands((1 << 14,), g, 2.0 ** -9)
    d = sum(F3.x3_dropped_terms(a, w))
    assert bool((d > 0).all()) and bool((d <= (2.0 ** -23 + 2.0 ** -32) * a.double() * w.double()).all())
    v = torch.full((4,), 1.0 + 2.0 ** -7 - 2.0 ** -23)                    # a2, a3 at their largest: the worst case of the cut
    dv = sum(F3.x3_dropped_terms(v, v))
    assert bool((dv > 2.0 ** -22 * v.double() ** 2).all()) and bool((dv < 2.0 ** -21 * v.double() ** 2).all())


@pytest.mark.parametrize('K', KS)
def test_same_sign_sums_need_the_drift_term(K):
    """Why x3_bound has a term in |y| sqrt(K) for same-sign data: an accumulator that rounds only once per 16-product block (the least an MFMA
    kernel can do) already leaves the bound without that term at every K, and approaches the zero-mean cap 2e-6 (1 + sum |t|) as K grows."""
    c = case(K, 'exposure')
    g = torch.Generator().manual_seed(K)
    pm, wm = patches(c['x']), wmat(c['w'])
    A, Wc = F3.cut3(pm), F3.cut3(wm)
    acc = torch.zeros(pm.shape[0], CO, dtype=torch.float32)
    perm = torch.randperm(K, generator=g)
    for s in range(0, K, 16):
        idx = perm[s:s + 16]
        for i, j in F3.KEPT:
            acc = (acc.double() + A[i][:, idx] @ Wc[j][idx, :]).float()
    xd, wd = c['x'].double(), c['w'].double()
    y = R.conv3x3(xd, wd)
    mag1 = R.conv3x3(xd.abs(), wd.abs())
    err = (acc.reshape(N, H, W, CO).double() - y).abs()
    no_drift = R.margin(R.conv3x3(xd * xd, wd * wd), K) + 2.0 ** -23 * mag1
    assert float((err / no_drift).max()) > 1.0
    assert bool((err <= F3.x3_bound(R.conv3x3(xd * xd, wd * wd), K, mag1, None, y)).all())


PRODUCTS = ['a1w1', 'a1w2', 'a2w1', 'a1w3', 'a2w2', 'a3w1']
SEPARATION = {288: 2.0, 576: 1.6, 2304: 1.05}      # least (lost product) / bound over the elements, the low-order products (module docstring of f32_ref)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('drop', range(6), ids=PRODUCTS)
def test_a_missing_product_fails_on_the_exposure_operands(K, drop):
    c = case(K, 'exposure')
    lost = R.conv3x3(*[p.double() for p in (F3.cut3(c['x'])[F3.KEPT[drop][0]], F3.cut3(c['w'])[F3.KEPT[drop][1]])])      # exact: what the kernel would not add
    got = (c['got'].double() - lost).float()
    assert not inside(got, c['y'], c['bound'])
    ratio = float((lost / c['bound']).min())
    print('K %d without %s: lost / bound >= %.2f' % (K, PRODUCTS[drop], ratio))
    assert ratio > SEPARATION[K]
    bad = float(((got.double() - c['y']).abs() > c['bound']).double().mean())
    print('    elements outside the bound: %.2f' % bad)
    # lost >= s bound and an honest error of at most e bound put EVERY element outside when s - e > 1: e < 0.6 (the emulation above), so up to
    # K = 576 (s >= 1.6) all elements must fail.  At K = 2304 (s = 1.05) the honest error, which 8-term steps bias upwards there, decides per
    # element: the defect must fail the layer (above), on about half of its elements
    if SEPARATION[K] - 0.6 >= 1.0:
        assert bad > 0.9


def test_beyond_exposure_max_k_the_low_order_products_are_absorbed():
    """K = 4608 same-sign terms (conv5_2's length; f32_ref's docstring): an 8-term block of a low-order product is below half an ulp of the
    running sum from about 1800 ... 3600 terms on and is lost whole.  The exact emulation then misses the plain bound by a deficit of several
    hundred 2^-24 sum |t| (an MI355X measures 350 on conv_x3d<64,4>), never more than the three low-order products together: inside
    x3_bound(absorb=True).  With 16-term steps it would not happen (the instruction's rounding granularity is what is seen), and a missing
    second-order product (a1w2, a2w1: 3.5e-3) still fails."""
    K = 4608
    g = torch.Generator().manual_seed(K)
    x = F3.exposure_operands((1, 6, 10, K // 9), g)
    w = F3.exposure_operands((CO, K // 9, 3, 3), g, 2.0 ** -K.bit_length())
    x.view(-1)[::13] = 0.0
    pm, wm = patches(x), wmat(w)
    xd, wd = x.double(), w.double()
    y = R.conv3x3(xd, wd)
    mag1 = R.conv3x3(xd.abs(), wd.abs())
    mag2 = R.conv3x3(xd * xd, wd * wd)
    plain, wide = F3.x3_bound(mag2, K, mag1, None, y), F3.x3_bound(mag2, K, mag1, None, y, absorb=True)
    got = emulate(pm, wm, g).reshape(y.shape)
    err = got.double() - y
    u = err / (R.U32 * mag1)
    print('K 4608, 8-term steps: error %.0f ... %.0f x 2^-24 sum |t|, worst err / plain bound %.2f, / bound with absorption %.2f' % (
        u.min(), u.max(), (err.abs() / plain).max(), (err.abs() / wide).max()))
    assert float((err.abs() / plain).max()) > 1.0 and float(u.min()) < -250
    assert bool((-err <= F3.EXPOSURE_LOW * mag1 + plain).all()) and inside(got, y, wide)
    got16 = emulate(pm, wm, g, terms=16).reshape(y.shape)
    assert inside(got16, y, plain)
    for drop in (1, 2):
        lost = R.conv3x3(F3.cut3(x)[F3.KEPT[drop][0]], F3.cut3(w)[F3.KEPT[drop][1]])
        assert float(((got.double() - lost - y).abs() > wide).double().mean()) > 0.9


@pytest.mark.parametrize('K', KS)
def test_rounded_a2_is_not_distinguishable(K):
    """(module docstring) the exact six-product sum of either cut is within the dropped-product term of the exact product sum."""
    c = case(K, 'exposure')
    pm, wm = patches(c['x']), wmat(c['w'])
    exact = pm.double() @ wm.double()
    mag1 = pm.double().abs() @ wm.double().abs()
    for r in (False, True):
        A, Wc = F3.cut3(pm, r), F3.cut3(wm, r)
        six = sum(A[i] @ Wc[j] for i, j in F3.KEPT)
        assert float(((six - exact).abs() / mag1).max()) <= 2.0 ** -23, r


@pytest.mark.parametrize('K,kind', BOTH)
def test_padding_and_seam_defects_fail(K, kind):
    c = case(K, kind)
    x = c['x']
    defects = {}
    for name, (sl, src) in {'top row of image 1': ((1, 0), (0, H - 1)), 'bottom row of image 0': ((0, H - 1), (1, 0))}.items():
        # the halo row above / below the image holds the neighbouring image's row instead of zeros
        xe = torch.zeros(N, H + 2, W, x.shape[3])
        xe[:, 1:H + 1] = x
        xe[sl[0], 0 if sl[1] == 0 else H + 1] = x[src[0], src[1]]
        xp = torch.nn.functional.pad(xe.double(), (0, 0, 1, 1, 0, 0))
        wd = c['w'].double()
        y = sum(xp[:, dy:dy + H, dx:dx + W, :] @ wd[:, :, dy, dx].t() for dy in range(3) for dx in range(3)) + c['b'].double()
        defects[name] = y
    xc = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    xc[0, 1:H + 1, W + 1] = xc[0, 1:H + 1, 1]                            # right halo column of image 0 wraps to the row's first pixel
    wd = c['w'].double()
    defects['right column of image 0'] = sum(xc[:, dy:dy + H, dx:dx + W, :] @ wd[:, :, dy, dx].t() for dy in range(3) for dx in range(3)) + c['b'].double()
    xs = x.clone()
    xs[0, H - 1], xs[1, 0] = x[1, 0], x[0, H - 1]                          # one row swapped across the seam of the two images
    defects['seam swap'] = R.conv3x3(xs.double(), wd) + c['b'].double()
    for name, yd in defects.items():
        assert not inside((yd + c['noise']).float(), c['y'], c['bound']), name


@pytest.mark.parametrize('K', KS)
def test_bf16_bias_fails(K):
    c = case(K, 'exposure')
    yd = c['y'] - c['b'].double() + R.rne_bf16(c['b'].double())
    assert not inside((yd + c['noise']).float(), c['y'], c['bound'])
    r = case(K, 'random')
    yd = r['y'] - r['b'].double() + R.rne_bf16(r['b'].double())
    assert not inside((yd + r['noise']).float(), r['y'], r['bound'])


@pytest.mark.parametrize('K,kind', BOTH)
def test_slope_one_at_exact_zeros_fails(K, kind):
    """backward-data epilogue: the gradient times slope(act), 0.6 at +-0."""
    c = case(K, kind)
    g = torch.Generator().manual_seed(K)
    act = torch.randn(N, H, W, CO, generator=g)
    act.view(-1)[::13] = 0.0
    act.view(-1)[5::29] = -0.0
    pre, m = c['y'], c['bound']
    z, mz = R.scale_ref(pre, m, R.slope(act.double()))
    good = (c['got'] * R.slope(act.double()).float())
    assert inside(good, z, mz)
    bad = c['got'] * torch.where(act == 0, torch.ones(()), R.slope(act.double()).float())
    assert not inside(bad, z, mz)


@pytest.mark.parametrize('kind', ['random', 'exposure'])
def test_weight_gradient_without_one_tile_row_fails(kind):
    g = torch.Generator().manual_seed(17)
    n, h, w, ci, co = 3, 9, 21, 8, 8
    K = n * h * w
    if kind == 'exposure':
        x, gy = F3.exposure_operands((n, h, w, ci), g), F3.exposure_operands((n, h, w, co), g, 2.0 ** -9)
    else:
        x, gy = torch.randn(n, h, w, ci, generator=g), torch.randn(n, h, w, co, generator=g)
    xd, gd = x.double(), gy.double()
    y = R.conv3x3_wgrad(gd, xd)
    bound = F3.x3_bound(R.conv3x3_wgrad(gd * gd, xd * xd), K, R.conv3x3_wgrad(gd.abs(), xd.abs()), None, y if kind == 'exposure' else None)
    # emulate tap (1, 1): dW[co][ci] = sum_p g[p][co] x[p][ci]
    got = emulate(gy.reshape(K, co).t().contiguous(), x.reshape(K, ci), g)
    assert inside(got, y[:, :, 1, 1], bound[:, :, 1, 1])
    g2 = gd.clone()
    g2[1, 4] = 0.0                                                         # one pixel row of one image left out of the contraction
    yd = R.conv3x3_wgrad(g2, xd)
    assert not inside(yd[:, :, 1, 1] + (got.double() - y[:, :, 1, 1]), y[:, :, 1, 1], bound[:, :, 1, 1])
