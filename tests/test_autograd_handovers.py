"""Graphs the modules never build, against float64 autograd.

mnk/ops.py decides in every backward pass which kernel runs and where its result lands, through one-shot hand-overs keyed by tensor
identity: _DZ_STATS (a data-gradient GEMM leaves the backward sums of the norm layer in front of it), _DY_SUMS (a norm layer's
backward leaves the bias gradient of the convolution in front of it, or states that it is exactly zero), _BN_OF / _LAST_BN.
tests/test_modules.py checks the "taken" side on Hourglass and ResBlock3D.  Here the same public ops are put together the way a
user's code may: a tensor with a second consumer, a frozen input, a second backward pass, a gradient hook, a norm layer in
evaluation mode with gradients enabled -- every hand-over must then be refused (or taken) so that the gradients are those of

    to_act(X) -> conv3x3(w1, b1) = Y1 -> bn_act(norm1, relu) = Z1 -> conv3x3(w2, b2) = Y2 -> bn_act(norm2, no relu) = Z2
    loss = sum(from_act(Z2) * g2) [+ sum(from_act(Y1) * g0)] [+ sum(from_act(Z1) * g1)]

restated in float64 with F.conv2d / F.batch_norm / F.relu, and so that ops.handover_state() is empty after every pass.

Shapes: cin = 5, c = 12, c2 = 7 (no multiple of 4, of 16 or of each other); maps 16 x 16 and 8 x 8; the batch n is the smallest
one at which 16 x 16 x n rows are MORE than mnk_bn_small_rows (general kernels) -- 8 x 8 x n rows are then within it (the
one-launch norm kernels).  The emulator's 512 rows give n = 3.

Bounds (those of tests/test_modules.py against the same kind of oracle): relative L2 error < 2e-4 for parameter gradients, < 1e-4
for the input gradient, max |error| < 2e-5 for the forward output.  A convolution bias in front of a training-mode norm layer gets
no gradient (it is exactly zero; the reference's is rounding noise, at most 1e-6 * sum |g2|)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

CIN, C1, C, C2 = 5, 3, 12, 7
EPS = 1e-5
TOL_PARAM, TOL_INPUT, TOL_OUT = 2e-4, 1e-4, 2e-5
PARAMS = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2")
WORST = {"param": 0.0, "input": 0.0, "out": 0.0}          # the largest errors of this session, printed by every case


def batch_for(be):
    small = be.query("mnk_bn_small_rows")
    n = small // 256 + 1
    assert n >= 2 and 64 * n <= small < 256 * n, (small, n)
    return n


@functools.lru_cache(maxsize=None)
def host_case(n, hw, second):
    """inputs, parameters and loss weights of one shape, fp32 on the host.  second: the first convolution reads [x | x1] through the
    nearest x2 up-sampling (sources at half the size)."""
    g = torch.Generator().manual_seed(1000 * hw + 10 * n + int(second))
    hs = hw // 2 if second else hw
    cin = CIN + (C1 if second else 0)
    t = {"x": torch.rand(n, CIN, 1, hs, hs, generator=g),
         "w1": torch.randn(C, cin, 1, 3, 3, generator=g) * 0.2, "b1": torch.randn(C, generator=g) * 0.1,
         "w2": torch.randn(C2, C, 1, 3, 3, generator=g) * 0.2, "b2": torch.randn(C2, generator=g) * 0.1,
         # affine parameters away from 1 / 0, as tests/test_modules.py perturbs them
         "gamma1": 1 + 0.3 * torch.randn(C, generator=g), "beta1": 0.3 * torch.randn(C, generator=g),
         "gamma2": 1 + 0.3 * torch.randn(C2, generator=g), "beta2": 0.3 * torch.randn(C2, generator=g),
         # running statistics of norm1 away from 0 / 1 (the evaluation-mode case)
         "mean1": 0.2 * torch.randn(C, generator=g), "var1": 0.5 + torch.rand(C, generator=g),
         "g0": torch.randn(n, C, 1, hw, hw, generator=g), "g1": torch.randn(n, C, 1, hw, hw, generator=g),
         "g2": torch.randn(n, C2, 1, hw, hw, generator=g)}
    if second:
        t["x1"] = torch.rand(n, C1, 1, hs, hs, generator=g)
    return t


@functools.lru_cache(maxsize=None)
def reference(n, hw, tap_y, tap_z, second=False, eval1=False, hook_scale=1.0):
    """the graph of the module docstring in float64: (output, {name: gradient}); computed once per configuration and not modified"""
    t = {k: v.double() for k, v in host_case(n, hw, second).items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in PARAMS + ("x",) + (("x1",) if second else ())}
    x = leaves["x"][:, :, 0]
    if second:
        x = F.interpolate(torch.cat([x, leaves["x1"][:, :, 0]], dim=1), scale_factor=2, mode="nearest")
    y1 = F.conv2d(x, leaves["w1"][:, :, 0], leaves["b1"], padding=1)
    if eval1:
        z1 = F.relu(F.batch_norm(y1, t["mean1"].clone(), t["var1"].clone(), leaves["gamma1"], leaves["beta1"], False, 0.1, EPS))
    else:
        z1 = F.relu(F.batch_norm(y1, None, None, leaves["gamma1"], leaves["beta1"], True, 0.1, EPS))
    if hook_scale != 1.0:
        z1.register_hook(lambda g: g * hook_scale)
    y2 = F.conv2d(z1, leaves["w2"][:, :, 0], leaves["b2"], padding=1)
    z2 = F.batch_norm(y2, None, None, leaves["gamma2"], leaves["beta2"], True, 0.1, EPS)
    loss = (z2 * t["g2"][:, :, 0]).sum()
    if tap_y:
        loss = loss + (y1 * t["g0"][:, :, 0]).sum()
    if tap_z:
        loss = loss + (z1 * t["g1"][:, :, 0]).sum()
    loss.backward()
    return z2.detach(), {k: v.grad.detach() for k, v in leaves.items()}


class Device:
    """the same graph from the public ops on the running backend"""

    def __init__(self, be, n, hw, second=False, eval1=False, frozen=()):
        from mnk import ops
        from sync_batchnorm import SynchronizedBatchNorm3d
        ops.clear_dz_stats()                 # (the start of an iteration: hand-overs that an earlier graph's sums never took)
        self.be, self.n, self.second = be, n, second
        self.host = t = host_case(n, hw, second)
        self.leaves = {k: be.t(t[k]).requires_grad_(k not in frozen) for k in ("x",) + (("x1",) if second else ())}
        for k in ("w1", "b1", "w2", "b2"):
            self.leaves[k] = torch.nn.Parameter(be.t(t[k]), requires_grad=k not in frozen)
        self.norm1, self.norm2 = SynchronizedBatchNorm3d(C, eps=EPS), SynchronizedBatchNorm3d(C2, eps=EPS)
        with torch.no_grad():
            for i, norm in ((1, self.norm1), (2, self.norm2)):
                norm.weight.copy_(t["gamma%d" % i]), norm.bias.copy_(t["beta%d" % i])
            self.norm1.running_mean.copy_(t["mean1"]), self.norm1.running_var.copy_(t["var1"])
        self.norm1.to(be.device).train(not eval1)
        self.norm2.to(be.device).train()
        for i, norm in ((1, self.norm1), (2, self.norm2)):
            self.leaves["gamma%d" % i], self.leaves["beta%d" % i] = norm.weight, norm.bias

    def forward(self, tap_y=False, tap_z=False, hook=None):
        from mnk import ops
        be, L, t, n = self.be, self.leaves, self.host, self.n
        kw = dict(x1=ops.to_act(L["x1"]), c1=C1, ups=True) if self.second else {}
        y1, s1 = ops.conv3x3(ops.to_act(L["x"]), CIN, L["w1"], L["b1"], want_stats=self.norm1.training, **kw)
        z1 = ops.bn_act(y1, C, self.norm1, relu=True, sums=s1)
        if hook is not None:
            z1.register_hook(hook)
        y2, s2 = ops.conv3x3(z1, C, L["w2"], L["b2"], want_stats=True)
        z2 = ops.bn_act(y2, C2, self.norm2, relu=False, sums=s2)
        self.out = ops.from_act(z2, C2, n)
        loss = (self.out * be.t(t["g2"])).sum()
        if tap_y:
            loss = loss + (ops.from_act(y1, C, n) * be.t(t["g0"])).sum()
        if tap_z:
            loss = loss + (ops.from_act(z1, C, n) * be.t(t["g1"])).sum()
        return loss

    def backward(self, loss, **kw):
        """-> DZ_STATS_COUNT of this pass (hand-overs taken, own passes)"""
        from mnk import ops
        ops.DZ_STATS_COUNT[0] = ops.DZ_STATS_COUNT[1] = 0
        loss.backward(**kw)
        self.be.sync()
        assert ops.handover_state() == {}, ops.handover_state()
        return tuple(ops.DZ_STATS_COUNT)


def check(dev, ref, scale=1.0, none=("b2",), tag=""):
    """output and every gradient of `dev` against `ref`; `none`: leaves that must have received NO gradient (the reference's is
    rounding noise around zero, or the leaf is frozen: then the reference's is not looked at)"""
    out64, g64 = ref
    t = dev.host
    err = float((dev.out.detach().cpu()[:, :, 0].double() - out64).abs().max())
    WORST["out"] = max(WORST["out"], err)
    assert err < TOL_OUT, ("forward", err)
    noise = 1e-6 * float(t["g2"].double().abs().sum())
    for k, p in dev.leaves.items():
        if k in none:
            assert p.grad is None, "%s received a gradient" % k
            if p.requires_grad:
                assert float(g64[k].abs().max()) <= noise, (k, float(g64[k].abs().max()), noise)
            continue
        assert p.grad is not None, "%s received no gradient" % k
        r = g64[k] * scale
        e = float((p.grad.detach().cpu().double().reshape(r.shape) - r).norm() / (r.norm() + 1e-30))
        kind = "input" if k in ("x", "x1") else "param"
        WORST[kind] = max(WORST[kind], e)
        assert e < (TOL_INPUT if kind == "input" else TOL_PARAM), (k, e)
    print("%s%s worst so far vs fp64: %s" % (dev.be.kind, tag, {k: "%.2e" % v for k, v in WORST.items()}))


def stats_form(be, n, hw):
    """the data-gradient launch of the second convolution (dy: c2 channels -> c) has a form that leaves norm1's backward sums"""
    from mnk import ops
    return be.query(ops._FORMS["3x3"].stats, n, hw, hw, C2, 0, C) > 0


def general_batch(be):
    """(n, the 16 x 16 plan has a statistics form).  Where the plan of the base batch has none (a split-K plan: few rows for many
    compute units), the batch grows to the nearest one that has -- the map, the channels and the side of the small-layer threshold
    stay."""
    n = batch_for(be)
    for m in range(n, n + 64):
        if stats_form(be, m, 16):
            return m
    raise AssertionError("no batch in [%d, %d) whose 16 x 16 data-gradient plan has a statistics form" % (n, n + 64))


@pytest.mark.parametrize("hw", [16, 8], ids=["general-kernels", "one-launch-norm"])
@pytest.mark.parametrize("tap_y,tap_z", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["untapped", "tap-Y1", "tap-Z1", "tap-Y1-Z1"])
def test_second_consumers_of_the_hand_over_tensors(be, hw, tap_y, tap_z):
    """Y1 (the first convolution's output) and Z1 (the first norm layer's) with a second consumer.  Untapped, the general path
    hands norm1's backward sums over from the second convolution's data-gradient launch; a tap on Z1 makes autograd add two
    gradients, so both norm layers make their own pass; the one-launch norm kernels use no hand-over.  A tap on Y1 makes the bias
    gradient of the first convolution non-zero: the "exactly zero" hand-over of norm1's backward must be refused."""
    n = general_batch(be) if hw == 16 else batch_for(be)
    assert 64 * n <= be.query("mnk_bn_small_rows") < 256 * n
    dev = Device(be, n, hw)
    count = dev.backward(dev.forward(tap_y, tap_z))
    print("DZ_STATS_COUNT", be.kind, "hw=%d n=%d tap_y=%s tap_z=%s" % (hw, n, tap_y, tap_z), count)
    check(dev, reference(n, hw, tap_y, tap_z), none=("b2",) if tap_y else ("b1", "b2"))
    if hw == 8:
        assert count == (0, 0), count
    elif tap_z:
        assert count == (0, 2), count
    else:
        assert count[0] >= 1 and sum(count) == 2, count


@pytest.mark.parametrize("hw", [16, 8], ids=["general-kernels", "one-launch-norm"])
@pytest.mark.parametrize("frozen", ["x", "w1", "b1"])
def test_a_frozen_input_gets_no_gradient_and_the_others_are_unchanged(be, hw, frozen):
    """requires_grad=False on the input, the first weight or the first bias (in front of a training-mode norm layer: nobody takes
    the "exactly zero" note that norm layer leaves, and it must not stay behind)."""
    n = general_batch(be) if hw == 16 else batch_for(be)
    dev = Device(be, n, hw, frozen=(frozen,))
    dev.backward(dev.forward())
    check(dev, reference(n, hw, False, False), none=("b1", "b2", frozen), tag=" frozen " + frozen)


def test_a_second_backward_pass_over_a_retained_graph(be):
    """backward(retain_graph=True) twice: every gradient is twice the reference's.  The hand-overs of the first pass are gone (they
    are one-shot): the second pass makes its own, and leaves nothing behind either."""
    from mnk import ops
    n = general_batch(be)
    dev = Device(be, n, 16)
    loss = dev.forward()
    first = dev.backward(loss, retain_graph=True)
    assert not ops._DZ_STATS and ops._DY_SUMS[0] is None
    second = dev.backward(loss, retain_graph=True)
    print("DZ_STATS_COUNT", be.kind, "retain_graph", first, second)
    assert first == second and first[0] >= 1 and sum(first) == 2, (first, second)
    check(dev, reference(n, 16, False, False), scale=2.0, none=("b1", "b2"), tag=" twice")


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place-hook", "in-place-hook"])
def test_a_gradient_hook_on_the_norm_output_is_seen_by_its_backward_statistics(be, inplace):
    """A hook that doubles the gradient of Z1.  Out of place it returns another tensor: the hand-over's key does not match.  In
    place (g.mul_(2)) the tensor keeps its address and the sums the data-gradient launch left are those of g, not of 2 g: the
    hand-over records the tensor's version and is refused."""
    n = general_batch(be)
    dev = Device(be, n, 16)
    count = dev.backward(dev.forward(hook=(lambda g: g.mul_(2)) if inplace else (lambda g: g * 2)))
    print("DZ_STATS_COUNT", be.kind, "hook in place" if inplace else "hook out of place", count)
    assert count == (0, 2), count
    check(dev, reference(n, 16, False, False, hook_scale=2.0), none=("b1", "b2"), tag=" hook")


def test_first_norm_layer_in_evaluation_mode_with_gradients_enabled(be):
    """norm1.eval(): constant statistics (perturbed running mean / variance), so the bias of the first convolution has a real
    gradient -- the column sums of dy that norm1's backward leaves -- and norm1 has no training record to hand over."""
    n = general_batch(be)
    dev = Device(be, n, 16, eval1=True)
    count = dev.backward(dev.forward())
    print("DZ_STATS_COUNT", be.kind, "norm1 in evaluation mode", count)
    assert count == (0, 2), count
    check(dev, reference(n, 16, False, False, eval1=True), none=("b2",), tag=" eval")
    t = dev.host
    assert torch.equal(dev.norm1.running_mean.cpu(), t["mean1"]) and torch.equal(dev.norm1.running_var.cpu(), t["var1"])


def test_two_sources_read_through_the_up_sampling(be):
    """the first convolution over [x | x1] at half the size, nearest x2 (UpBlock3D's call): both input gradients, and the hand-over
    of norm1's sums from the second convolution as in the plain graph"""
    n = general_batch(be)
    dev = Device(be, n, 16, second=True)
    count = dev.backward(dev.forward())
    print("DZ_STATS_COUNT", be.kind, "two sources, up-sampled", count)
    assert count[0] >= 1 and sum(count) == 2, count
    check(dev, reference(n, 16, False, False, second=True), none=("b1", "b2"), tag=" up")
