"""Mixed-precision TRAINING products of the 3x3 convolutions (include/monkeynet_hip.h): MNK_CONV_BF16_TRAIN = 16 on the forward
and data-gradient launches (the one-pass form of MNK_CONV_BF16, allowed together with the training statistics and the
BatchNorm-backward hand-over) and MNK_WGRAD_BF16 = 8 on the weight-gradient launches (the one-plane form of the tap-major and
sub-pixel kernels).  Operands are rounded to nearest-even bf16 in the loaders, products are exact in fp32 and accumulated in fp32 --
so against an fp64 evaluation on HOST-rounded operands only the fp32 summation is left and the tolerance is the one
tests/test_kernels_conv.py holds the fp32 kernels to.
The same bodies run on the CPU emulator build (-m "not gpu") and on the MI355X (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_kernels_conv import (_inputs, CASES, FAST_CASES, STAT_CASES, SPLIT_STAT_CASES, UP_CASES, BNSTATS_CASES, HALO_CASES,
                               WFAST_CASES, COMPACT_CASES)

BF16 = 8          # MNK_CONV_BF16 (inference)
TRAIN = 16        # MNK_CONV_BF16_TRAIN
WBF16 = 8         # MNK_WGRAD_BF16
TOL = 2e-6        # tests/test_kernels_conv.py: the fp32 kernels against fp64


def _bf(t):
    """round to nearest even bf16, back in fp32 (None stays None)"""
    return None if t is None else t.bfloat16().float()


# ---- forward: flag 16 with the training statistics --------------------------------------------------------------------------------
def _fwd_args(be, case, seed=3):
    n, h, w, c0, c1, cout, ups, _, _ = case
    x0, x1, wt, b, r = _inputs(case, seed=seed)
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X0 = be.t(to_nhwc(x0))
    X1 = be.t(to_nhwc(x1)) if x1 is not None else None
    R = be.t(to_nhwc(r)) if r is not None else None
    B = be.t(b) if b is not None else None
    return lambda flags: (X0, X0.shape[-1], c0, X1, X1.shape[-1] if x1 is not None else 0, c1, int(ups) | flags, wp, B, R,
                          R.shape[-1] if r is not None else 0)


@pytest.mark.parametrize("case", STAT_CASES + SPLIT_STAT_CASES)
def test_training_flag_forward_with_statistics(be, case):
    """flag 16 + stats_partial: y is the inference form's (flag 8, no statistics) bit for bit -- the same kernel, the same plan --
    and the finished statistics are the column sums of that y (epilogue sums of an unsplit launch, the reduction's of a split one)"""
    n, h, w, c0, c1, cout = case[:6]
    args = _fwd_args(be, case)
    ldy = ceil4(cout)
    nst = be.query("mnk_conv3x3_stats_floats", n, h, w, c0, c1, cout)
    nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
    assert nst > 0 and (nws > 0) == (case in SPLIT_STAT_CASES)
    ws = be.empty(nws) if nws else None
    Y, Y8, st = be.empty(n, h, w, ldy), be.empty(n, h, w, ldy), be.empty(nst)
    be.call("mnk_conv3x3_fwd", *args(TRAIN), Y, ldy, n, h, w, cout, ws, nws, st)
    sums = be.empty(2 * cout)
    be.call("mnk_bn_stats_finish", st, nst // (2 * ldy), ldy, cout, sums)
    be.call("mnk_conv3x3_fwd", *args(BF16), Y8, ldy, n, h, w, cout, ws, nws, None)
    be.sync()
    assert torch.equal(Y.cpu(), Y8.cpu())
    assert torch.all(Y.cpu()[..., cout:] == 0)
    y = from_nhwc(Y.cpu(), cout).double()
    err = relerr(sums.cpu(), torch.cat([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))]))
    print("bf16-train forward statistics %s: relerr %.3g" % (case, err))
    assert err < 1e-5          # tests/test_kernels_conv.py::test_conv3x3_fused_bn_statistics
    Yp = be.empty(n, h, w, ldy)
    be.call("mnk_conv3x3_fwd", *args(0), Yp, ldy, n, h, w, cout, ws, nws, None)
    be.sync()
    assert not torch.equal(Y.cpu(), Yp.cpu()), "the flagged launch computed the fp32 convolution"


@pytest.mark.parametrize("case", [c for c in UP_CASES if c[1] >= 16])
def test_training_flag_subpixel_forward_with_statistics(be, case):
    """the sub-pixel forward (mnk_conv3x3_up_fwd) under flag 16 with its fused statistics"""
    n, h, w, c0, c1, cout, bias = case
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(n, c0, h, w, generator=g)
    x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    wt = torch.randn(cout, c0 + c1, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g) if bias else None
    wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_up_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X0 = be.t(to_nhwc(x0))
    X1 = be.t(to_nhwc(x1)) if c1 else None
    ldy = ceil4(cout)
    nws = be.query("mnk_conv3x3_up_workspace_floats", n, h, w, c0, c1, cout)
    ws = be.empty(max(nws, 1))
    nst = be.query("mnk_conv3x3_up_stats_floats", n, h, w, c0, c1, cout)
    assert nst > 0
    st = be.empty(nst)
    Y, Y8 = be.empty(n, 2 * h, 2 * w, ldy), be.empty(n, 2 * h, 2 * w, ldy)
    args = (X0, X0.shape[-1], c0, X1, X1.shape[-1] if c1 else 0, c1)
    be.call("mnk_conv3x3_up_fwd", *args, TRAIN, wp, be.t(b) if bias else None, Y, ldy, n, h, w, cout, ws, nws, st)
    sums = be.empty(2 * cout)
    be.call("mnk_bn_stats_finish", st, nst // (2 * ldy), ldy, cout, sums)
    be.call("mnk_conv3x3_up_fwd", *args, BF16, wp, be.t(b) if bias else None, Y8, ldy, n, h, w, cout, ws, nws, None)
    be.sync()
    assert torch.equal(Y.cpu(), Y8.cpu())
    y = from_nhwc(Y.cpu(), cout).double()
    assert relerr(sums.cpu(), torch.cat([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))])) < 1e-5


def test_training_flag_deferred_split_k_partials_sum_to_the_undeferred_output(be):
    """MNK_CONV_BF16_TRAIN | MNK_CONV_DEFER_SPLITK (what a small training layer leaves to the norm layer behind it): the partials,
    summed on the host in the reduction's order, are the undeferred flagged output bit for bit"""
    case = (3, 4, 4, 40, 0, 136, 0, True, False)
    n, h, w, c0, c1, cout = case[:6]
    _, _, _, b, _ = _inputs(case, seed=3)
    args = _fwd_args(be, case)
    splits = be.query("mnk_conv3x3_splits", n, h, w, c0, c1, cout)
    nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
    assert splits > 1 and nws > 0
    ldy = ceil4(cout)
    want, Y, ws = be.empty(n, h, w, ldy), be.empty(n, h, w, ldy), be.empty(nws)
    be.call("mnk_conv3x3_fwd", *args(2 | TRAIN), want, ldy, n, h, w, cout, ws, nws, None)
    be.sync()
    ws.fill_(float("nan"))
    be.call("mnk_conv3x3_fwd", *args(2 | 4 | TRAIN), Y, ldy, n, h, w, cout, ws, nws, None)
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
    assert torch.equal(total, want.cpu().view(m, ldy)[:, :cout])


# ---- data gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES[:4] + FAST_CASES if not c[6]])
def test_training_flag_data_gradient(be, case):
    """the forward kernel on dy with the data-gradient pack, flag 16, both loader families: against the fp64 transposed convolution
    of host-rounded dy and weights"""
    n, h, w, c0, c1, cout = case[:6]
    x0, x1, wt, _, _ = _inputs(case)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(n, cout, h, w, generator=g)
    x = torch.zeros(n, c0 + c1, h, w, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, _bf(wt).double(), None, padding=1).backward(_bf(dy).double())
    DY = be.t(to_nhwc(dy))
    for c_start, c_cnt in ((0, c0),) + (((c0, c1),) if c1 else ()):
        wp = be.empty(be.query("mnk_conv3x3_packed_floats", c_cnt, cout, 0))
        be.call("mnk_conv3x3_pack_dgrad", be.t(wt), wp, cout, c0 + c1, c_start, c_cnt)
        ld = ceil4(c_cnt)
        nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, cout, 0, c_cnt)
        ws = be.empty(max(nws, 1))
        for flags in (0, 2):
            DX = be.empty(n, h, w, ld)
            be.call("mnk_conv3x3_fwd", DY, DY.shape[-1], cout, None, 0, 0, flags | TRAIN, wp, None, None, 0, DX, ld, n, h, w, c_cnt,
                    ws, nws, None)
            be.sync()
            err = relerr(from_nhwc(DX.cpu(), c_cnt), x.grad[:, c_start:c_start + c_cnt])
            print("bf16-train dgrad %s flags=%d source@%d: relerr %.3g" % (case, flags | TRAIN, c_start, err))
            assert err < TOL
            assert torch.all(DX.cpu()[..., c_cnt:] == 0)


_PHASE_SET = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}       # S(a, u) of csrc/conv3x3.hip


def _subpixel_rounded(xlow, wt64):
    """[nearest x2 -> 3x3 / pad 1] on the low-resolution fp64 input, phase by phase, with the pre-summed 2x2 weights of each phase
    rounded to bf16 (the sums are exact in fp32 for weights that are integers / 64) -- differentiable in xlow"""
    n, c, h, w = xlow.shape
    cout = wt64.shape[0]
    xp = F.pad(xlow, (1, 1, 1, 1))
    rows = []
    for pa in (0, 1):
        cols = []
        for pb in (0, 1):
            w2 = torch.zeros(cout, c, 2, 2, dtype=torch.float64)
            for u in (0, 1):
                for v in (0, 1):
                    for ky in _PHASE_SET[(pa, u)]:
                        for kx in _PHASE_SET[(pb, v)]:
                            w2[:, :, u, v] += wt64[:, :, ky, kx]
            assert torch.equal(w2.float().double(), w2)               # exact in fp32: the pack's order cannot matter
            cols.append(F.conv2d(xp[:, :, pa:pa + h + 1, pb:pb + w + 1], w2.float().bfloat16().double()))
        rows.append(torch.stack(cols, dim=-1).reshape(n, cout, h, 2 * w))          # interleave the two column phases
    return torch.stack(rows, dim=3).reshape(n, cout, 2 * h, 2 * w)                 # ... and the two row phases


@pytest.mark.parametrize("case", UP_CASES)
def test_training_flag_subpixel_data_gradient(be, case):
    """mnk_conv3x3_up_dgrad_ex with flag 16: one 4x4 / stride 2 convolution over rounded dy with the ROUNDED pre-summed packs;
    flag 0 is mnk_conv3x3_up_dgrad bit for bit"""
    n, h, w, c0, c1, cout, _ = case
    g = torch.Generator().manual_seed(31)
    wt = torch.randint(-40, 41, (cout, c0 + c1, 3, 3), generator=g).float() / 64
    dy = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
    x = torch.zeros(n, c0 + c1, h, w, dtype=torch.float64, requires_grad=True)
    _subpixel_rounded(x, wt.double()).backward(_bf(dy).double())
    DY = be.t(to_nhwc(dy))
    ldy = ceil4(cout)
    for c_start, c_cnt in ((0, c0),) + (((c0, c1),) if c1 else ()):
        wd = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cout, c_cnt))
        be.call("mnk_conv3x3_up_pack_dgrad", be.t(wt), wd, cout, c0 + c1, c_start, c_cnt)
        ld = ceil4(c_cnt)
        nws = be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, h, w, cout, c_cnt)
        ws = be.empty(max(nws, 1))
        DX, D0, D1 = be.empty(n, h, w, ld), be.empty(n, h, w, ld), be.empty(n, h, w, ld)
        be.call("mnk_conv3x3_up_dgrad_ex", DY, ldy, cout, wd, DX, ld, n, h, w, c_cnt, ws, nws, TRAIN)
        be.call("mnk_conv3x3_up_dgrad_ex", DY, ldy, cout, wd, D0, ld, n, h, w, c_cnt, ws, nws, 0)
        be.call("mnk_conv3x3_up_dgrad", DY, ldy, cout, wd, D1, ld, n, h, w, c_cnt, ws, nws)
        be.sync()
        err = relerr(from_nhwc(DX.cpu(), c_cnt), x.grad[:, c_start:c_start + c_cnt])
        print("bf16-train sub-pixel dgrad %s source@%d: relerr %.3g" % (case, c_start, err))
        assert err < TOL
        assert torch.all(DX.cpu()[..., c_cnt:] == 0)
        assert torch.equal(D0.cpu(), D1.cpu()) and not torch.equal(D0.cpu(), DX.cpu())


@pytest.mark.parametrize("case", BNSTATS_CASES)
def test_training_flag_data_gradient_with_the_norm_layers_backward_statistics(be, case):
    """mnk_conv3x3_dgrad_bnstats_ex / mnk_conv3x3_up_dgrad_bnstats_ex with flag 16: dx is the plain flagged data gradient bit for
    bit, the finished sums are those of that dx (fp64, the tolerance of the fp32 test); with flag 0 the old entries bit for bit"""
    n, h, w, cout, c, up, use_res, slope = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    wt = torch.randn(cout, c, 3, 3, generator=g) * 0.2
    res = torch.randn(n, c, h, w, generator=g) if use_res else None
    y = torch.randn(n, c, h, w, generator=g)
    mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    scale = gamma * invstd
    DY, Y = be.t(to_nhwc(dy)), be.t(to_nhwc(y))
    ldx = ceil4(c)
    dx_a, dx_b, dx_0, dx_old = (be.empty(n, h, w, ldx) for _ in range(4))
    if up:
        wp = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cout, c))
        be.call("mnk_conv3x3_up_pack_dgrad", be.t(wt), wp, cout, c, 0, c)
        nws = be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, h, w, cout, c)
        nst = be.query("mnk_conv3x3_up_dgrad_stats_floats", n, h, w, cout, c)
    else:
        wp = be.empty(be.query("mnk_conv3x3_packed_floats", c, cout, 0))
        be.call("mnk_conv3x3_pack_dgrad", be.t(wt), wp, cout, c, 0, c)
        nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, cout, 0, c)
        nst = be.query("mnk_conv3x3_stats_floats", n, h, w, cout, 0, c)
    assert nst > 0 and nst % (2 * ldx) == 0
    ws = be.empty(max(nws, 1))
    st, st0, st_old = be.empty(nst), be.empty(nst), be.empty(nst)
    R = be.t(to_nhwc(res)) if use_res else None
    bn = (Y, ldx, be.t(mean), be.t(invstd), be.t(scale), be.t(beta), float(slope))
    if up:
        be.call("mnk_conv3x3_up_dgrad_ex", DY, DY.shape[-1], cout, wp, dx_a, ldx, n, h, w, c, ws, nws, TRAIN)
        head = (DY, DY.shape[-1], cout, wp)
        for name, dx, s, tail in (("mnk_conv3x3_up_dgrad_bnstats_ex", dx_b, st, (TRAIN,)), ("mnk_conv3x3_up_dgrad_bnstats_ex", dx_0, st0, (0,)),
                                  ("mnk_conv3x3_up_dgrad_bnstats", dx_old, st_old, ())):
            be.call(name, *head, dx, ldx, n, h, w, c, ws, nws, s, *bn, *tail)
    else:
        be.call("mnk_conv3x3_fwd", DY, DY.shape[-1], cout, None, 0, 0, 2 | TRAIN, wp, None, R, ldx if use_res else 0, dx_a, ldx, n, h, w,
                c, ws, nws, None)
        head = (DY, DY.shape[-1], cout, wp, R, ldx if use_res else 0)
        for name, dx, s, tail in (("mnk_conv3x3_dgrad_bnstats_ex", dx_b, st, (TRAIN,)), ("mnk_conv3x3_dgrad_bnstats_ex", dx_0, st0, (0,)),
                                  ("mnk_conv3x3_dgrad_bnstats", dx_old, st_old, ())):
            be.call(name, *head, dx, ldx, n, h, w, c, ws, nws, s, *bn, *tail)
    sums = be.empty(2 * c)
    be.call("mnk_bn_stats_finish", st, nst // (2 * ldx), ldx, c, sums)
    be.sync()
    assert torch.equal(dx_a.cpu(), dx_b.cpu()), "the flagged data gradient itself must not change"
    assert torch.equal(dx_0.cpu(), dx_old.cpu()) and torch.equal(st0.cpu(), st_old.cpu())
    assert not torch.equal(dx_0.cpu(), dx_b.cpu())
    dz = from_nhwc(dx_a.cpu(), c).double()
    d = y.double() - mean.double()[None, :, None, None]
    pre = d * scale.double()[None, :, None, None] + beta.double()[None, :, None, None]
    gg = dz if slope < 0 else torch.where(pre > 0, dz, dz * slope)
    want = torch.cat([gg.sum(dim=(0, 2, 3)), (gg * d * invstd.double()[None, :, None, None]).sum(dim=(0, 2, 3))])
    got = sums.cpu().double()
    tol = 2e-5 * (float(want.abs().max()) + float(gg.abs().sum(dim=(0, 2, 3)).max()) * 1e-2)
    assert float((got - want).abs().max()) <= tol, (float((got - want).abs().max()), tol)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
# the cases of HALO_CASES whose comments name the tap-major form
TAP_MAJOR = [c for c in HALO_CASES if c in ((1, 8, 8, 72, 0, 48, 0, False, False), (2, 5, 7, 33, 0, 129, 0, False, False),
                                            (1, 8, 8, 80, 0, 24, 1, False, False), (2, 32, 32, 72, 0, 40, 0, False, False))]
MUST_ROUND = TAP_MAJOR + WFAST_CASES + COMPACT_CASES
assert len(TAP_MAJOR) == 4


def _wgrad(be, case, x0, x1, dy, flags, clean):
    """mnk_conv3x3_wgrad of both sources with `flags` (+ the case's up-sampling and `clean`) -> dw on the host"""
    n, h, w, c0, c1, cout, ups = case[:7]
    DY = be.t(to_nhwc(dy))
    DW = be.empty(cout, c0 + c1, 3, 3)
    for src, c_start, c_cnt in ((x0, 0, c0),) + (((x1, c0, c1),) if c1 else ()):
        X = be.t(to_nhwc(src, pad_value=0.0 if clean else float("nan")))
        nws = be.query("mnk_conv3x3_up_wgrad_workspace_floats" if ups else "mnk_conv3x3_wgrad_workspace_floats", n, h, w, c_cnt, cout)
        ws = be.empty(max(nws, 1))
        be.call("mnk_conv3x3_wgrad", X, X.shape[-1], c_cnt, int(ups) | (2 if clean else 0) | flags, DY, DY.shape[-1], cout, DW,
                c0 + c1, c_start, n, h, w, ws, nws)
    be.sync()
    return DW.cpu()


def _wgrad_ref(case, x0, x1, dy):
    """fp64 weight gradient on host-rounded x and dy"""
    n, h, w, c0, c1, cout, ups = case[:7]
    wd = torch.zeros(cout, c0 + c1, 3, 3, dtype=torch.float64, requires_grad=True)
    x = _bf(x0 if x1 is None else torch.cat([x0, x1], 1))
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    F.conv2d(x.double(), wd, None, padding=1).backward(_bf(dy).double())
    return wd.grad


@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("case", CASES + HALO_CASES + WFAST_CASES + COMPACT_CASES)
def test_weight_gradient_flag(be, case, clean):
    """per source: the flagged gradient is the unflagged one bit for bit (a form that keeps fp32 products: nine-tap, LDS-halo,
    gather), or it is the fp64 gradient on rounded x and dy within the fp32 tolerance and differs from the unflagged one.  The
    tap-major cases, the fast-loader cases and the compact-K cases must round."""
    n, h, w, c0, c1, cout, ups = case[:7]
    x0, x1, _, _, _ = _inputs(case)
    g = torch.Generator().manual_seed(6)
    dy = torch.randn(n, cout, h, w, generator=g)
    plain = _wgrad(be, case, x0, x1, dy, 0, clean)
    flagged = _wgrad(be, case, x0, x1, dy, WBF16, clean)
    ref = _wgrad_ref(case, x0, x1, dy)
    for c_start, c_cnt in ((0, c0),) + (((c0, c1),) if c1 else ()):
        sl = slice(c_start, c_start + c_cnt)
        same = torch.equal(flagged[:, sl], plain[:, sl])
        err = relerr(flagged[:, sl], ref[:, sl])
        print("wgrad bf16 %s clean=%s source@%d: %s, relerr vs fp64 on rounded operands %.3g"
              % (case, clean, c_start, "fp32 form (same bits)" if same else "rounded", err))
        if case in MUST_ROUND:
            assert not same, "a tap-major shape kept the fp32 products"
        assert same or err < TOL


ROUNDING_CASES = [HALO_CASES[5],        # plain tap-major
                  WFAST_CASES[1],       # up-sampled, clean sources: the sub-pixel form
                  COMPACT_CASES[0]]     # compact K


@pytest.mark.parametrize("case", ROUNDING_CASES)
def test_the_weight_gradient_loader_rounds_to_nearest_even(be, case):
    """ties planted in x and dy as tests/test_kernels_conv_bf16_onepass.py plants them: the flagged gradient of the raw operands
    equals, bit for bit, the flagged gradient of operands the host rounded first"""
    down, up = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8
    assert float(_bf(torch.tensor(down))) == 1.0 and float(_bf(torch.tensor(up))) == 1.0 + 2.0 ** -6
    n, h, w, c0, c1, cout, ups = case[:7]
    x0, x1, _, _, _ = _inputs(case, seed=9)
    g = torch.Generator().manual_seed(6)
    dy = torch.randn(n, cout, h, w, generator=g)
    for t in (x0, x1, dy):
        if t is None:
            continue
        flat = t.view(-1)
        flat[0::7] = down
        flat[3::7] = -up
        flat[5::11] = up
        flat[6::13] = -down
    assert not torch.equal(_bf(x0), x0) and not torch.equal(_bf(dy), dy)
    raw = _wgrad(be, case, x0, x1, dy, WBF16, True)
    pre = _wgrad(be, case, _bf(x0), _bf(x1), _bf(dy), WBF16, True)
    assert torch.equal(raw, pre)
    assert not torch.equal(raw, _wgrad(be, case, x0, x1, dy, 0, True))


# ---- grouped launches -------------------------------------------------------------------------------------------------------------
def _grouped_jobs(be, flags_of):
    """three tap-major layers (plain, sub-pixel, plain with the fast loader) as MnkWgradJob records; flags_of(i): extra flag bits"""
    from mnk.optim import JOB
    cases = [HALO_CASES[5], WFAST_CASES[1], WFAST_CASES[3]]
    jobs, meta = [], []
    for i, case in enumerate(cases):
        n, h, w, c0, c1, cout, ups = case[:7]
        x0, _, _, _, _ = _inputs(case)
        g = torch.Generator().manual_seed(100 + i)
        dy = torch.randn(n, cout, h, w, generator=g)
        X, DY = be.t(to_nhwc(x0)), be.t(to_nhwc(dy))
        DW = be.empty(cout, c0, 3, 3)
        jobs.append((X.data_ptr(), DY.data_ptr(), 0, 0, X.shape[-1], c0, int(ups) | 2 | flags_of(i), DY.shape[-1], cout, n, h, w,
                     h, w, 3, 3, 1, 0, 0, 0))
        meta.append((case, x0, dy, X, DY, DW))
    return np.array(jobs, dtype=JOB), meta


_PLAN_FIELDS = ("variant", "splits", "part_floats", "layout")


def test_grouped_weight_gradients_with_the_flag(be):
    """flagged jobs through mnk_wgrad_grouped_plan / _build / _launch + mnk_wgrad_reduce_multi: the plan is the unflagged plan,
    the gradients are the fp64 gradients on rounded operands"""
    from test_kernels_optim import REDUCE_DESC, _table
    rec, meta = _grouped_jobs(be, lambda i: WBF16)
    rec0, _ = _grouped_jobs(be, lambda i: 0)
    assert be.query("mnk_wgrad_grouped_plan", rec.ctypes.data, len(rec)) == 0
    assert be.query("mnk_wgrad_grouped_plan", rec0.ctypes.data, len(rec0)) == 0
    for f in _PLAN_FIELDS:
        assert rec[f].tolist() == rec0[f].tolist(), f
    assert all(0 <= v < 16 for v in rec["variant"].tolist()) and {v % 4 == 3 for v in rec["variant"].tolist()} == {True, False}
    parts, rows, blocks = [], [], 0
    for k, (case, x0, dy, X, DY, DW) in enumerate(meta):
        part = be.empty(int(rec["part_floats"][k]))
        parts.append(part)
        rec["part"][k] = part.data_ptr()
        c0, cout = case[3], case[5]
        rows.append((part.data_ptr(), DW.data_ptr(), int(rec["layout"][k]), int(rec["splits"][k]), 9, cout, c0, c0, 0, 0, blocks, 0))
        blocks += be.query("mnk_wgrad_reduce_blocks", int(rec["splits"][k]), cout, c0)
    nbytes = be.query("mnk_wgrad_grouped_table_bytes", len(rec))
    host = torch.zeros(nbytes, dtype=torch.uint8)
    assert be.query("mnk_wgrad_grouped_build", rec.ctypes.data, len(rec), host.data_ptr(), nbytes) == 0
    dev = be.t(host)
    be.call("mnk_wgrad_grouped_launch", dev, host.data_ptr())
    descs = _table(be, np.array(rows, dtype=REDUCE_DESC))
    be.call("mnk_wgrad_reduce_multi", descs, len(rows), blocks)
    be.sync()
    for case, x0, dy, X, DY, DW in meta:
        err = relerr(DW.cpu(), _wgrad_ref(case, x0, None, dy))
        print("grouped wgrad bf16 %s: relerr %.3g" % (case, err))
        assert err < TOL
        assert not torch.equal(DW.cpu(), _wgrad(be, case, x0, None, dy, 0, True))


def test_a_mixed_grouped_table_is_rejected(be):
    """all tap-major jobs of one table agree on MNK_WGRAD_BF16: a mixed table is an invalid argument; nothing is built or launched"""
    rec, meta = _grouped_jobs(be, lambda i: WBF16 if i == 1 else 0)
    assert be.query("mnk_wgrad_grouped_plan", rec.ctypes.data, len(rec)) == 0
    parts = [be.empty(int(rec["part_floats"][k])) for k in range(len(rec))]
    for k, p in enumerate(parts):
        rec["part"][k] = p.data_ptr()
    nbytes = be.query("mnk_wgrad_grouped_table_bytes", len(rec))
    host = torch.zeros(nbytes, dtype=torch.uint8)
    assert be.query("mnk_wgrad_grouped_build", rec.ctypes.data, len(rec), host.data_ptr(), nbytes) != 0
    assert b"invalid argument" in be.lib.cdll.mnk_last_error()
    be.sync()
    assert all(torch.isnan(p.cpu()).all() for p in parts), "a rejected table must not launch"


# ---- invalid bits -----------------------------------------------------------------------------------------------------------------
def test_invalid_flag_bits_are_rejected(be):
    """32 on a forward launch and on the _ex data gradients, 16 on a weight gradient: invalid arguments, nothing is launched"""
    from mnk._lib import MnkError
    case = (2, 16, 16, 24, 0, 40, 0, True, False)
    n, h, w, c0, c1, cout = case[:6]
    args = _fwd_args(be, case, seed=1)
    ldy = ceil4(cout)
    nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
    ws = be.empty(max(nws, 1))
    Y = be.empty(n, h, w, ldy)
    with pytest.raises(MnkError, match="invalid argument"):
        be.call("mnk_conv3x3_fwd", *args(2 | 32), Y, ldy, n, h, w, cout, ws, nws, None)
    x0, _, _, _, _ = _inputs(case, seed=1)
    g = torch.Generator().manual_seed(6)
    dy = torch.randn(n, cout, h, w, generator=g)
    X, DY = be.t(to_nhwc(x0)), be.t(to_nhwc(dy))
    DW = be.empty(cout, c0, 3, 3)
    nww = be.query("mnk_conv3x3_wgrad_workspace_floats", n, h, w, c0, cout)
    ww = be.empty(max(nww, 1))
    with pytest.raises(MnkError, match="invalid argument"):
        be.call("mnk_conv3x3_wgrad", X, X.shape[-1], c0, 2 | 16, DY, DY.shape[-1], cout, DW, c0, 0, n, h, w, ww, nww)
    wd = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", c0, cout))
    DX = be.empty(n, h // 2, w // 2, ceil4(cout))
    with pytest.raises(MnkError, match="invalid argument"):        # (an _ex data gradient takes 0 or 16 only)
        be.call("mnk_conv3x3_up_dgrad_ex", X, X.shape[-1], c0, wd, DX, ceil4(cout), n, h // 2, w // 2, cout, ws, nws, BF16)
    be.sync()
    assert torch.isnan(Y.cpu()).all() and torch.isnan(DW.cpu()).all() and torch.isnan(DX.cpu()).all()
