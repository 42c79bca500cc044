"""CPU tests of the float64 bf16 reference (oracle/bf16_ref.py): one rounding to nearest even, the first layer's cuts, the acceptance rule."""
import pytest

torch = pytest.importorskip('torch')
from oracle import bf16_ref as R      # noqa: E402  (checker only)


def f(h):
    return float.fromhex(h)


def rne(vals):
    return R.rne_bf16(torch.tensor(vals, dtype=torch.float64)).tolist()


def test_ties_go_to_even():
    one, ulp = 1.0, 2.0 ** -7
    assert rne([one + ulp / 2]) == [one]                                 # tie, even below
    assert rne([one + 3 * ulp / 2]) == [one + 2 * ulp]                   # tie, even above
    assert rne([-(one + ulp / 2), -(one + 3 * ulp / 2)]) == [-one, -(one + 2 * ulp)]
    assert rne([f('0x1.01p+0') + 2.0 ** -40]) == [one + ulp]            # just above a tie
    assert rne([f('0x1.01p+0') - 2.0 ** -40]) == [one]                  # just below
    assert rne([f('0x1.ffp+0')]) == [2.0]                                # carry into the next binade
    assert rne([2.0 ** 100 * (1 + 2.0 ** -8)]) == [2.0 ** 100]


def test_single_rounding_where_float32_rounds_twice():
    """1 + 2^-8 + 2^-30 is above the tie: one rounding gives 1 + 2^-7.  Through float32 it becomes the tie 1 + 2^-8 first and then 1."""
    v = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert rne([v]) == [1.0 + 2.0 ** -7]
    twice = torch.tensor([v], dtype=torch.float64).float().to(torch.bfloat16).double().tolist()
    assert twice == [1.0]
    # and float32 inputs (one rounding already done) agree with torch's float32 -> bf16 conversion everywhere
    g = torch.Generator().manual_seed(3)
    x = torch.randn(100000, generator=g) * torch.exp2(torch.randint(-140, 120, (100000,), generator=g).float())
    assert torch.equal(R.rne_bf16(x.double()), x.to(torch.bfloat16).double())


def test_zeros_subnormals_and_overflow():
    out = R.rne_bf16(torch.tensor([0.0, -0.0], dtype=torch.float64))
    assert out.tolist() == [0.0, 0.0] and torch.signbit(out).tolist() == [False, True]
    sub = 2.0 ** -133                                                    # smallest bf16 subnormal
    assert rne([sub, sub / 2, 3 * sub / 2, sub * 0.5000001, 5 * sub / 2]) == [sub, 0.0, 2 * sub, sub, 2 * sub]
    assert rne([2.0 ** -126 * (1 - 2.0 ** -9)]) == [2.0 ** -126]         # largest subnormal region rounds up into the normals
    big = R.BF16_MAX
    assert rne([big, big * (1 + 2.0 ** -9), -big * (1 + 2.0 ** -8)]) == [big, big, float('-inf')]
    assert R.bits_of(R.rne_bf16(torch.tensor([1.0, -2.0, sub], dtype=torch.float64))).tolist() == [0x3F80, 0xC000, 0x0001]


def test_cuts_of_the_first_layer():
    x = torch.tensor([1.0 + 2.0 ** -10 + 2.0 ** -20, -3.14159, 1e-30, 0.0], dtype=torch.float32)
    hi, lo = R.first_cut2(x)
    assert hi.tolist()[0] == 1.0 and lo.tolist()[0] == 2.0 ** -10        # lo truncated: the 2^-20 is dropped
    assert torch.equal(R.rne_bf16(hi), hi) and torch.equal(R.rne_bf16(lo), lo)
    assert bool(((x.double() - hi - lo).abs() <= x.double().abs() * 2.0 ** -15).all())
    hw, lw = R.wgrad_cut2(x)
    assert torch.equal(hw, hi) and bool(((x.double() - hw - lw).abs() <= x.double().abs() * 2.0 ** -16).all())
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -15 + 2.0 ** -16 + 2.0 ** -20], dtype=torch.float32)
    assert R.first_cut2(y)[1].item() == 2.0 ** -8 + 2.0 ** -15 and R.wgrad_cut2(y)[1].item() == 2.0 ** -8 + 2.0 ** -14      # truncated / rounded


def test_acceptance_rule():
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 + 2.0 ** -12, 3.0, -0.0], dtype=torch.float64)
    m = torch.full_like(y, 2.0 ** -16)
    r = R.bits_of(R.rne_bf16(y))
    ok, fl = R.bf16_accept(r, y, m)
    assert ok.all() and not fl.any()
    other = R.bits_of(torch.tensor([1.0, 1.0, 3.0 + 2.0 ** -6, 0.0], dtype=torch.float64))
    ok, fl = R.bf16_accept(other, y, m)
    assert ok.tolist() == [True, False, False, True] and fl.tolist() == [True, False, False, False]      # only the near tie may flip
    assert R.bf16_accept(R.bits_of(torch.tensor([0.0], dtype=torch.float64)), torch.tensor([-0.0], dtype=torch.float64),
                         torch.zeros(1, dtype=torch.float64))[0].all()                                         # +0 == -0
    assert R.bits_of(R.trunc_bf16(torch.tensor([-1.0 - 2.0 ** -7 + 2.0 ** -12], dtype=torch.float64))).tolist() == [0xBF80]
