"""Feature-matching L1 kernels (mnk_pair_l1_fwd / _bwd) against modules/losses.py::reconstruction_loss semantics:
weight * mean over (C, H, W) of |generated - real| per sample, and its gradient (torch.abs' sign convention, 0 at 0)."""
import pytest
import torch

from _util import to_nhwc, from_nhwc, ceil4, relerr, maxerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)


@pytest.mark.parametrize("shape", [(3, 5, 7, 6), (2, 64, 30, 30), (1, 13, 4, 4), (4, 256, 2, 2)])
def test_pair_l1_forward_backward(be, shape):
    b, c, h, w = shape
    g = torch.Generator().manual_seed(3)
    fake = torch.randn(b, c, h, w, generator=g)
    real = torch.randn(b, c, h, w, generator=g)
    real[0, 0, 0, :2] = fake[0, 0, 0, :2]                  # exact ties: the gradient there is 0
    weight = 10.0
    f64, r64 = fake.double().requires_grad_(True), real.double().requires_grad_(True)
    ref = weight * (f64 - r64).abs().reshape(b, -1).mean(-1)
    gout = torch.randn(b, generator=g).double()
    (ref * gout).sum().backward()
    # pad channels of both halves hold the same garbage-free zeros (acts of this library); poison nothing else
    A = be.t(to_nhwc(torch.cat([fake, real], 0)))
    out = be.empty(b)
    be.call("mnk_pair_l1_fwd", A, ceil4(c), h * w, c, b, weight, out)
    DA = be.empty(2 * b, h, w, ceil4(c)).fill_(float("nan"))
    be.call("mnk_pair_l1_bwd", A, ceil4(c), h * w, c, b, weight, be.t(gout.float()), DA)
    be.sync()
    assert relerr(out.cpu(), ref.detach()) < 2e-6
    d = DA.cpu()
    assert maxerr(from_nhwc(d[:b], c), f64.grad) < 1e-6 * (1 + float(f64.grad.abs().max()))
    assert maxerr(from_nhwc(d[b:], c), r64.grad) < 1e-6 * (1 + float(r64.grad.abs().max()))
    assert torch.all(d[..., c:] == 0)
    assert float(from_nhwc(d[:b], c)[0, 0, 0, 0]) == 0.0


def test_pair_l1_autograd_function(be):
    from mnk import ops
    b, c, h, w = 2, 10, 6, 5
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2 * b, c, h, w, generator=g)
    act = ops.to_act(be.t(x.unsqueeze(2).clone())).detach().requires_grad_(True)
    out = ops.PairL1Fn.apply(act, c, b, 2.5)
    gout = torch.randn(b, generator=g)
    (out * be.t(gout)).sum().backward()
    be.sync()
    x64 = x.double().requires_grad_(True)
    ref = 2.5 * (x64[:b] - x64[b:]).abs().reshape(b, -1).mean(-1)
    (ref * gout.double()).sum().backward()
    assert relerr(out.detach().cpu(), ref.detach()) < 2e-6
    assert maxerr(from_nhwc(act.grad.cpu(), c), x64.grad) < 1e-6


@pytest.mark.parametrize("shape", [(3, 3, 1, 9, 7), (2, 3, 1, 64, 64), (4, 1, 1, 1, 5)])
def test_l1_mean_and_its_autograd_function(be, shape):
    """mnk_l1_mean_fwd / _bwd == weight * mean_batch(|prediction - target|) of modules/losses.py:8-12 on NCDHW frames."""
    from mnk import ops
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    b.view(-1)[:3] = a.view(-1)[:3]                         # exact ties: gradient 0
    n = shape[0]
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = 7.0 * (a64 - b64).abs().reshape(n, -1).mean(-1)
    gout = torch.randn(n, generator=g)
    (ref * gout.double()).sum().backward()
    A, B = be.t(a).requires_grad_(True), be.t(b).requires_grad_(True)
    out = ops.L1MeanFn.apply(A, B, 7)
    (out * be.t(gout)).sum().backward()
    be.sync()
    assert relerr(out.detach().cpu(), ref.detach()) < 2e-6
    assert maxerr(A.grad.cpu(), a64.grad) < 1e-6 * (1 + float(a64.grad.abs().max()))
    assert maxerr(B.grad.cpu(), b64.grad) < 1e-6 * (1 + float(b64.grad.abs().max()))
    assert float(A.grad.cpu().view(-1)[0]) == 0.0
    # only one side asks for a gradient (reconstruction_deformed: the real frames are data)
    A2, B2 = be.t(a), be.t(b).requires_grad_(True)
    (ops.L1MeanFn.apply(A2, B2, 7) * be.t(gout)).sum().backward()
    be.sync()
    assert torch.equal(B2.grad.cpu(), B.grad.cpu())


@pytest.mark.parametrize("shape", [(3, 1, 1, 1, 1), (2, 1, 1, 5, 4)])
def test_gan_terms_match_the_loss_module(be, shape):
    """GanTermsFn == (generator_gan_loss, discriminator_gan_loss) of modules/losses.py on the batched score maps, for the
    three ways the step differentiates them: the generator term alone, the discriminator term alone, both."""
    from mnk import ops
    from modules import losses
    b = shape[0]
    g = torch.Generator().manual_seed(6)
    score = torch.randn((2 * b,) + tuple(shape[1:]), generator=g)
    s64 = score.double().requires_grad_(True)
    ref_g = losses.generator_gan_loss([s64[:b]], 1.5)
    ref_d = losses.discriminator_gan_loss([s64[:b]], [s64[b:]], 0.75)
    gg, gd = torch.randn(b, generator=g), torch.randn(b, generator=g)
    S = be.t(score).requires_grad_(True)
    gen, disc = ops.GanTermsFn.apply(S, b, 1.5, 0.75)
    be.sync()
    assert relerr(gen.detach().cpu(), ref_g.detach()) < 2e-6 and relerr(disc.detach().cpu(), ref_d.detach()) < 2e-6
    for use_g, use_d in ((True, False), (False, True), (True, True)):
        S.grad, s64.grad = None, None
        tot = (gen * be.t(gg)).sum() * float(use_g) + (disc * be.t(gd)).sum() * float(use_d)
        ref = (ref_g * gg.double()).sum() * float(use_g) + (ref_d * gd.double()).sum() * float(use_d)
        if use_g and not use_d:
            tot, ref = (gen * be.t(gg)).sum(), (ref_g * gg.double()).sum()
        if use_d and not use_g:
            tot, ref = (disc * be.t(gd)).sum(), (ref_d * gd.double()).sum()
        tot.backward(retain_graph=True)
        ref.backward(retain_graph=True)
        be.sync()
        assert maxerr(S.grad.cpu(), s64.grad) < 1e-6 * (1 + float(s64.grad.abs().max()))


def test_loss_module_runs_the_l1_kernels_on_the_library_device(be):
    """modules.losses.reconstruction_loss (the function the reference's train.py calls, losses.py:8-12) on fp32 tensors of the
    library's device is the one-launch kernel pair (an L1MeanFn node), equal to the stock arithmetic it replaces; fp64 / CPU
    checks keep the stock arithmetic."""
    from modules import losses
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(3, 4, 1, 6, 5, generator=g), torch.randn(3, 4, 1, 6, 5, generator=g)
    A, B = be.t(a).requires_grad_(True), be.t(b).requires_grad_(True)
    out = losses.reconstruction_loss(A, B, 10)
    assert "L1MeanFn" in type(out.grad_fn).__name__
    gout = torch.randn(3, generator=g)
    (out * be.t(gout)).sum().backward()
    be.sync()
    a64, b64 = a.double().detach().requires_grad_(True), b.double().detach().requires_grad_(True)
    ref = losses.reconstruction_loss(a64, b64, 10)
    assert "L1MeanFn" not in type(ref.grad_fn).__name__
    (ref * gout.double()).sum().backward()
    assert relerr(out.detach().cpu(), ref.detach()) < 2e-6
    assert maxerr(A.grad.cpu(), a64.grad) < 1e-6 and maxerr(B.grad.cpu(), b64.grad) < 1e-6
    assert losses.reconstruction_loss(A, B, 0) == 0


@pytest.mark.parametrize("nvec,length", [(1, 4), (6, 32), (16, 70)])
def test_batch_means_of_the_loss_vectors(be, nvec, length):
    """mnk_vec_means_fwd / _bwd and ops.LossMeansFn against `[v.mean() for v in losses]`, `sum(loss_values)` (train.py:114,116)
    and autograd's gradients of both outputs."""
    import numpy as np
    from mnk import ops
    g = torch.Generator().manual_seed(5)
    vecs = [torch.randn(length, generator=g) * (i + 1) for i in range(nvec)]
    V = [be.t(v) for v in vecs]
    means = be.empty(nvec + 1)
    ptrs = np.array([v.data_ptr() for v in V], dtype=np.uint64)
    be.call("mnk_vec_means_fwd", ptrs.ctypes.data, nvec, length, means)
    ref = torch.stack([v.double().mean() for v in vecs])
    gm, gt = torch.randn(nvec, generator=g), torch.randn(1, generator=g)
    GV = be.empty(nvec, length).fill_(float("nan"))
    be.call("mnk_vec_means_bwd", be.t(gm), be.t(gt), nvec, length, GV)
    GV2 = be.empty(nvec, length)
    be.call("mnk_vec_means_bwd", None, be.t(gt), nvec, length, GV2)
    be.sync()
    assert maxerr(means.cpu()[:nvec], ref) < 1e-6 * (1 + float(ref.abs().max()))
    assert abs(float(means.cpu()[nvec]) - float(ref.sum())) < 1e-5 * (1 + float(ref.abs().sum()))
    want = ((gm.double() + gt.double()) / length).unsqueeze(1).expand(nvec, length)
    assert maxerr(GV.cpu(), want) < 1e-6
    assert maxerr(GV2.cpu(), (gt.double() / length).expand(nvec, length)) < 1e-6
    # the autograd wrapper: same gradients as the stock formulation
    leaves = [be.t(v.clone()).requires_grad_(True) for v in vecs]
    m, tot = ops.LossMeansFn.apply(*leaves)
    (tot * 2.0 + (m * be.t(gm)).sum()).backward()
    leaves2 = [v.detach().double().requires_grad_(True) for v in vecs]
    m2 = torch.stack([v.mean() for v in leaves2])
    (m2.sum() * 2.0 + (m2 * gm.double()).sum()).backward()
    be.sync()
    for a, b in zip(leaves, leaves2):
        assert maxerr(a.grad.cpu(), b.grad) < 1e-6


def test_feature_matching_tap_adds_the_next_blocks_gradient(be):
    """ops.PairL1TapFn: the map goes on to the next block unchanged, and its backward is the L1 gradient PLUS the gradient the
    next block sends (mnk_pair_l1_bwd_add) -- what autograd's accumulation of two consumers gives."""
    from mnk import ops
    b, c, h, w = 2, 10, 6, 5
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2 * b, c, h, w, generator=g)
    nxt = torch.randn(2 * b, h, w, ceil4(c), generator=g)
    nxt[..., c:] = 0
    gl = torch.randn(b, generator=g)
    A = be.t(to_nhwc(x)).requires_grad_(True)
    act, loss = ops.PairL1TapFn.apply(A, c, b, 3.0)
    assert torch.equal(act.detach().cpu(), A.detach().cpu())
    ((act * be.t(nxt)).sum() + (loss * be.t(gl)).sum()).backward()
    A2 = be.t(to_nhwc(x)).requires_grad_(True)
    loss2 = ops.PairL1Fn.apply(A2, c, b, 3.0)
    ((A2 * be.t(nxt)).sum() + (loss2 * be.t(gl)).sum()).backward()
    be.sync()
    assert torch.equal(loss.detach().cpu(), loss2.detach().cpu())
    assert maxerr(A.grad.cpu(), A2.grad.cpu()) < 1e-6
    # only the next block's gradient (the discriminator-loss backward): handed through untouched
    A3 = be.t(to_nhwc(x)).requires_grad_(True)
    act3, _ = ops.PairL1TapFn.apply(A3, c, b, 3.0)
    (act3 * be.t(nxt)).sum().backward()
    be.sync()
    assert torch.equal(A3.grad.cpu(), nxt)


# ---- the entry points called directly on guard-banded buffers (the autograd functions above allocate from torch's pool) -------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 841])
@pytest.mark.parametrize("b", [1, 3])
def test_gan_terms_direct(be, b, n):
    """mnk_gan_terms_fwd / _bwd against fp64 means of (1 - s_f)^2 and (1 - s_r)^2 + s_f^2 and their gradients.  A lane of the
    forward kernel strides by 64: n = 64 +- 1 sits on that stride, 841 (a 29 x 29 score map) gives a lane 14 terms.  Backward
    with the generator term alone, the discriminator term alone and both; the absent one is NULL.  Tolerances: those of
    test_gan_terms_match_the_loss_module."""
    from mnk._lib import MnkError
    g = torch.Generator().manual_seed(60 + n)
    wg, wd = 1.5, 0.75
    score = torch.randn(2 * b, n, generator=g)
    gg, gd = torch.randn(b, generator=g), torch.randn(b, generator=g)
    s64 = score.double().requires_grad_(True)
    ref_g = wg * ((1 - s64[:b]) ** 2).mean(1)
    ref_d = wd * ((1 - s64[b:]) ** 2 + s64[:b] ** 2).mean(1)
    S, GG, GD = be.t(score), be.t(gg), be.t(gd)
    gen, disc = be.empty(b), be.empty(b)
    be.call("mnk_gan_terms_fwd", S, n, b, wg, wd, gen, disc)
    be.sync()
    eg, ed = relerr(gen.cpu(), ref_g.detach()), relerr(disc.cpu(), ref_d.detach())
    print("b %d n %d: relerr gen %.2e disc %.2e" % (b, n, eg, ed))
    assert eg < 2e-6 and ed < 2e-6
    for use_g, use_d in ((True, False), (False, True), (True, True)):
        s64.grad = None
        ref = (ref_g * gg.double()).sum() * float(use_g) + (ref_d * gd.double()).sum() * float(use_d)
        ref.backward(retain_graph=True)
        DS = be.empty(2 * b, n)
        be.call("mnk_gan_terms_bwd", S, n, b, wg, wd, GG if use_g else None, GD if use_d else None, DS)
        be.sync()
        assert maxerr(DS.cpu(), s64.grad) < 1e-6 * (1 + float(s64.grad.abs().max())), (use_g, use_d)
        if not use_d:
            assert torch.all(DS.cpu()[b:] == 0)              # the real frames' scores are in the discriminator term only
    DS = be.empty(2 * b, n)
    with pytest.raises(MnkError):
        be.call("mnk_gan_terms_bwd", S, n, b, wg, wd, None, None, DS)
    be.sync()
    assert torch.isnan(DS.cpu()).all()


def _off_by_one_float(be, x):
    """x as a view that starts one float past a 256-byte boundary (the header promises only `n contiguous floats`)"""
    buf = be.empty(x.numel() + 1)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 12289])
@pytest.mark.parametrize("b", [1, 4])
def test_l1_mean_direct(be, b, n):
    """mnk_l1_mean_fwd / _bwd against fp64 weight * mean |a - b| per sample and torch.abs' gradient (0 at ties), on inputs
    that are not 16-byte aligned.  The forward block strides by 1024.  Backward with da alone, db alone and both: the present
    output has the same bits in all three.  Tolerances: those of test_l1_mean_and_its_autograd_function."""
    g = torch.Generator().manual_seed(70 + n)
    weight = 7.0
    a, bb = torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)
    ties = sorted({0, n // 2, n - 1, min(n - 1, 1024)})      # exact ties, one of them past the block's first stride
    for i in range(b):
        bb[i, ties] = a[i, ties]
    gout = torch.randn(b, generator=g)
    a64, b64 = a.double().requires_grad_(True), bb.double().requires_grad_(True)
    ref = weight * (a64 - b64).abs().mean(1)
    (ref * gout.double()).sum().backward()
    A, B, G = _off_by_one_float(be, a), _off_by_one_float(be, bb), be.t(gout)
    out = be.empty(b)
    be.call("mnk_l1_mean_fwd", A, B, n, b, weight, out)
    be.sync()
    err = relerr(out.cpu(), ref.detach())
    print("b %d n %d: relerr %.2e" % (b, n, err))
    assert err < 2e-6
    DA, DB, DA1, DB1 = (_off_by_one_float(be, torch.full((b, n), float("nan"))) for _ in range(4))
    be.call("mnk_l1_mean_bwd", A, B, n, b, weight, G, DA, DB)
    be.call("mnk_l1_mean_bwd", A, B, n, b, weight, G, DA1, None)
    be.call("mnk_l1_mean_bwd", A, B, n, b, weight, G, None, DB1)
    be.sync()
    da, db = DA.cpu(), DB.cpu()
    assert maxerr(da, a64.grad) < 1e-6 * (1 + float(a64.grad.abs().max()))
    assert maxerr(db, b64.grad) < 1e-6 * (1 + float(b64.grad.abs().max()))
    assert torch.all(da[:, ties] == 0) and torch.all(db[:, ties] == 0)          # +0.0 or -0.0
    assert torch.equal(DA1.cpu().view(torch.int32), da.view(torch.int32))
    assert torch.equal(DB1.cpu().view(torch.int32), db.view(torch.int32))


@pytest.mark.parametrize("shape", [(3, 5, 7, 6), (2, 64, 30, 30), (1, 13, 4, 4), (4, 256, 2, 2)])
def test_pair_l1_bwd_add_direct(be, shape):
    """mnk_pair_l1_bwd_add at test_pair_l1_forward_backward's shapes: without an addend the bits of mnk_pair_l1_bwd, with one
    those of (mnk_pair_l1_bwd's output + addend) formed in fp32 on the host -- one rounding per element either way.  `a`, `g`
    and `addend` are const arguments: the guarded call checks that they are unchanged."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(9)
    fake = torch.randn(b, c, h, w, generator=g)
    real = torch.randn(b, c, h, w, generator=g)
    real[0, 0, 0, :2] = fake[0, 0, 0, :2]                    # exact ties
    add = to_nhwc(torch.randn(2 * b, c, h, w, generator=g))  # an act's gradient: pad channels 0
    weight, ld = 10.0, ceil4(c)
    A, G, ADD = be.t(to_nhwc(torch.cat([fake, real], 0))), be.t(torch.randn(b, generator=g)), be.t(add)
    D0, D1, D2 = (be.empty(2 * b, h, w, ld) for _ in range(3))
    be.call("mnk_pair_l1_bwd", A, ld, h * w, c, b, weight, G, D0)
    be.call("mnk_pair_l1_bwd_add", A, ld, h * w, c, b, weight, G, None, D1)
    be.call("mnk_pair_l1_bwd_add", A, ld, h * w, c, b, weight, G, ADD, D2)
    be.sync()
    d0 = D0.cpu()
    assert not torch.isnan(d0).any()
    assert torch.equal(D1.cpu().view(torch.int32), d0.view(torch.int32))
    want = d0 + add
    assert torch.equal(D2.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.all(D2.cpu()[..., c:] == 0)
