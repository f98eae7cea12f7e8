"""The one-pass bf16 form of the forward convolutions (MNK_CONV_BF16 = 8 in `flags`; csrc/mnk_common.h): the loaders round both
operands to bf16 (nearest even), the products of the rounded operands are exact in fp32 and are accumulated in fp32 -- so against
an fp64 convolution of the HOST-rounded operands only the fp32 summation is left, and the tolerance is the one
tests/test_kernels_conv.py holds the fp32 kernels to.  Bias, residual, split-K partials and the stores stay fp32.
The same bodies run on the CPU emulator build (-m "not gpu") and on the MI355X (-m gpu)."""
import pytest
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_kernels_conv import _inputs, _ref_fwd, _run_fwd, CASES, FAST_CASES

BF16 = 8          # MNK_CONV_BF16
TOL = 2e-6        # tests/test_kernels_conv.py::test_conv3x3_forward


def _bf(t):
    """round to nearest even bf16, back in fp32 (None stays None)"""
    return None if t is None else t.bfloat16().float()


def _flagged(case, flag=BF16):
    """the case with MNK_CONV_BF16 in the value _run_fwd passes on as `flags` (its `ups` argument)"""
    return case[:6] + (int(case[6]) | flag,) + case[7:]


@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("case", CASES + FAST_CASES)
def test_one_pass_forward_is_the_convolution_of_the_rounded_operands(be, case, clean):
    """all five 32x32 tiles, both 16x16 tiles, two sources, the up-sampled view, split-K, the residual, ragged M, 1x1 maps, channel
    counts that are no multiple of 16, and NaN pad channels under the generic loader"""
    x0, x1, wt, b, r = _inputs(case)
    Y = _run_fwd(be, _flagged(case), x0, x1, wt, b, r, clean)
    ref = _ref_fwd(case, _bf(x0), _bf(x1), _bf(wt), b, r)             # bias and residual are not rounded
    cout = case[5]
    err = relerr(from_nhwc(Y, cout), ref)
    print("one-pass bf16 %s clean=%s: relerr vs fp64 on rounded operands %.3g" % (case, clean, err))
    assert err < TOL
    assert torch.all(Y[..., cout:] == 0), "pad channels of the output must be written as zero"


TIE_CASES = [(1, 6, 10, 20, 13, 45, 0, True, True),       # 16x16 tiles (BN = 48), two sources, residual
             (2, 8, 8, 16, 10, 70, 1, True, False),       # 32x32 tiles, up-sampled view
             (3, 4, 4, 40, 0, 136, 0, False, False)]      # split-K


@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("case", TIE_CASES)
def test_the_loader_rounds_to_nearest_even(be, case, clean):
    """the flagged output on raw operands equals, bit for bit, the flagged output on operands the host rounded first (torch:
    nearest even) -- with ties planted in both operands: 1 + 2^-8 lies half-way between 1 and 1 + 2^-7 and must act as 1.0
    (truncation agrees, round-half-away does not); 1 + 3 * 2^-8 lies half-way between 1 + 2^-7 and 1 + 2^-6 and must act as
    1 + 2^-6 (round-half-away agrees, truncation does not)"""
    down, up = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8
    assert float(_bf(torch.tensor(down))) == 1.0 and float(_bf(torch.tensor(up))) == 1.0 + 2.0 ** -6
    x0, x1, wt, b, r = _inputs(case, seed=9)
    for t in (x0, x1, wt):
        if t is None:
            continue
        flat = t.view(-1)
        flat[0::7] = down
        flat[3::7] = -up
        flat[5::11] = up
        flat[6::13] = -down
    raw = _run_fwd(be, _flagged(case), x0, x1, wt, b, r, clean)
    pre = _run_fwd(be, _flagged(case), _bf(x0), _bf(x1), _bf(wt), b, r, clean)
    assert not torch.equal(_bf(x0), x0)
    assert torch.equal(raw, pre)
    # and the ties alone: every operand a tie
    ones = [None if t is None else torch.where(torch.arange(t.numel()).view(t.shape) % 2 == 0, torch.full_like(t, down),
                                                 torch.full_like(t, up)) for t in (x0, x1, wt)]
    want = [None if t is None else torch.where(t == down, torch.ones_like(t), torch.full_like(t, 1.0 + 2.0 ** -6)) for t in ones]
    a = _run_fwd(be, _flagged(case), ones[0], ones[1], ones[2], b, r, clean)
    c = _run_fwd(be, _flagged(case), want[0], want[1], want[2], b, r, clean)
    assert torch.equal(a, c)


@pytest.mark.parametrize("case", [CASES[1], CASES[2], FAST_CASES[0], FAST_CASES[2]])
def test_the_flag_engages_the_one_pass_kernels(be, case):
    x0, x1, wt, b, r = _inputs(case, seed=4)
    plain = _run_fwd(be, case, x0, x1, wt, b, r, clean=True)
    flagged = _run_fwd(be, _flagged(case), x0, x1, wt, b, r, clean=True)
    cout = case[5]
    diff = float((plain[..., :cout] - flagged[..., :cout]).abs().max())
    assert diff > 1e-4, "the flagged launch computed the fp32 convolution"
    assert relerr(from_nhwc(flagged, cout), _ref_fwd(case, x0, x1, wt, b, r)) < 2e-2       # (still that convolution)


# ---- sub-pixel form of [nearest x2 -> 3x3 / pad 1]: (n, h_low, w_low, c0, c1, cout) -------------------------------------------
_PHASE_SET = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}       # S(a, u) of csrc/conv3x3.hip


@pytest.mark.parametrize("case", [(2, 8, 8, 16, 10, 70), (1, 2, 2, 32, 0, 10)])
def test_one_pass_subpixel_forward_rounds_the_summed_taps(be, case):
    """mnk_conv3x3_up_pack_fwd sums the 3x3 taps of each phase in fp32 and the loader of mnk_conv3x3_up_fwd rounds the SUMS.
    Weights are integers / 64, so those sums are exact in fp32 whatever their order; the reference sums them in fp64, rounds the
    sums to bf16 and convolves the rounded low-resolution input phase by phase."""
    n, h, w, c0, c1, cout = case
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(n, c0, h, w, generator=g)
    x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    wt = torch.randint(-40, 41, (cout, c0 + c1, 3, 3), generator=g).float() / 64
    b = torch.randn(cout, generator=g)
    x = _bf(x0 if x1 is None else torch.cat([x0, x1], 1)).double()
    xp = F.pad(x, (1, 1, 1, 1))
    ref = torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64)
    for pa in (0, 1):
        for pb in (0, 1):
            w2 = torch.zeros(cout, c0 + c1, 2, 2, dtype=torch.float64)
            for u in (0, 1):
                for v in (0, 1):
                    for ky in _PHASE_SET[(pa, u)]:
                        for kx in _PHASE_SET[(pb, v)]:
                            w2[:, :, u, v] += wt[:, :, ky, kx].double()
            assert torch.equal(w2.float().double(), w2)               # exact in fp32: the pack's order cannot matter
            w2 = w2.float().bfloat16().double()
            ref[:, :, pa::2, pb::2] = F.conv2d(xp[:, :, pa:pa + h + 1, pb:pb + w + 1], w2, b.double())
    wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_up_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X0 = be.t(to_nhwc(x0))
    X1 = be.t(to_nhwc(x1)) if c1 else None
    ldy = ceil4(cout)
    nws = be.query("mnk_conv3x3_up_workspace_floats", n, h, w, c0, c1, cout)
    ws = be.empty(max(nws, 1))
    outs = []
    for flags in (BF16, 0):
        Y = be.empty(n, 2 * h, 2 * w, ldy)
        be.call("mnk_conv3x3_up_fwd", X0, X0.shape[-1], c0, X1, X1.shape[-1] if c1 else 0, c1, flags, wp, be.t(b), Y, ldy,
                n, h, w, cout, ws, nws, None)
        be.sync()
        outs.append(Y.cpu())
    err = relerr(from_nhwc(outs[0], cout), ref)
    print("one-pass bf16 sub-pixel %s: relerr %.3g" % (case, err))
    assert err < TOL
    assert torch.all(outs[0][..., cout:] == 0)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("clean", [0, 2], ids=["generic-loader", "kxk-buffer-loader"])
@pytest.mark.parametrize("case", [(2, 13, 13, 6, 20), (2, 5, 5, 64, 40)])
def test_one_pass_4x4_forward_without_padding(be, case, clean):
    n, hi, wi, cin, cout = case
    g = torch.Generator().manual_seed(17)
    x = torch.randn(n, cin, hi, wi, generator=g)
    wt = torch.randn(cout, cin, 4, 4, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(_bf(x).double(), _bf(wt).double(), b.double())
    ho, wo = ref.shape[2], ref.shape[3]
    wp = be.empty(be.query("mnk_conv2d_packed_floats", cout, cin, 0, 16))
    be.call("mnk_conv2d_pack_fwd", be.t(wt), wp, cout, cin, 0, 16)
    X = be.t(to_nhwc(x))
    Y = be.empty(n, ho, wo, ceil4(cout))
    nws = be.query("mnk_conv2d_workspace_floats", n, ho, wo, cin, 0, cout, 16)
    ws = be.empty(max(nws, 1))
    be.call("mnk_conv2d_fwd", X, ceil4(cin), cin, None, 0, 0, clean | BF16, hi, wi, 4, 4, 0, wp, be.t(b), None, 0, Y, ceil4(cout),
            n, ho, wo, cout, ws, nws, None)
    be.sync()
    err = relerr(from_nhwc(Y.cpu(), cout), ref)
    print("one-pass bf16 4x4 %s flags=%d: relerr %.3g" % (case, clean | BF16, err))
    assert err < TOL
    assert torch.all(Y.cpu()[..., cout:] == 0)


def test_one_pass_deferred_split_k_partials_sum_to_the_undeferred_output(be):
    """MNK_CONV_BF16 | MNK_CONV_DEFER_SPLITK: the partials [split][M][ldw] are fp32 sums of exact products; summed on the host
    in the reduction's order (four interleaved groups, (g0 + g1) + (g2 + g3), then the bias) they are the undeferred flagged
    output bit for bit."""
    case = (3, 4, 4, 40, 0, 136, 0, True, False)
    n, h, w, c0, c1, cout = case[:6]
    x0, _, wt, b, _ = _inputs(case, seed=2)
    want = _run_fwd(be, _flagged(case), x0, None, wt, b, None, clean=True)
    splits = be.query("mnk_conv3x3_splits", n, h, w, c0, c1, cout)
    nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
    assert splits > 1 and nws > 0
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X = be.t(to_nhwc(x0))
    ldy = ceil4(cout)
    Y = be.empty(n, h, w, ldy)
    ws = be.empty(nws)
    be.call("mnk_conv3x3_fwd", X, X.shape[-1], c0, None, 0, 0, 2 | 4 | BF16, wp, be.t(b), None, 0, Y, ldy, n, h, w, cout, ws, nws, None)
    be.sync()
    assert torch.isnan(Y.cpu()).all(), "a deferred launch does not write y"
    m = n * h * w
    part = ws.cpu()[:splits * m * ldy].view(splits, m, ldy)
    groups = []
    for e in range(4):
        acc = torch.zeros(m, ldy)
        for s in range(e, splits, 4):
            acc = acc + part[s]
        groups.append(acc)
    total = ((groups[0] + groups[1]) + (groups[2] + groups[3]))[:, :cout] + b
    assert torch.equal(total, want.view(m, ldy)[:, :cout])


def test_one_pass_launch_refuses_training_statistics(be):
    """`stats_partial` is a training request: with MNK_CONV_BF16 the call is an invalid argument and launches nothing"""
    from mnk._lib import MnkError
    case = (2, 16, 16, 24, 0, 40, 0, True, False)
    n, h, w, c0, c1, cout = case[:6]
    x0, _, wt, b, _ = _inputs(case, seed=1)
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X = be.t(to_nhwc(x0))
    ldy = ceil4(cout)
    nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
    ws = be.empty(max(nws, 1))
    nst = be.query("mnk_conv3x3_stats_floats", n, h, w, c0, c1, cout)
    assert nst > 0
    args = lambda flags, Y, st: ("mnk_conv3x3_fwd", X, X.shape[-1], c0, None, 0, 0, flags, wp, be.t(b), None, 0, Y, ldy, n, h, w,
                                 cout, ws, nws, st)
    Y, st = be.empty(n, h, w, ldy), be.empty(nst)
    with pytest.raises(MnkError, match="invalid argument"):
        be.call(*args(2 | BF16, Y, st))
    be.sync()
    assert torch.isnan(Y.cpu()).all() and torch.isnan(st.cpu()).all(), "a rejected call must not launch"
    be.call(*args(2, Y, st))                                   # the same call without the flag is a valid training launch
    be.sync()
    assert not torch.isnan(Y.cpu()).any()
