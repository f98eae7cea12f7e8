"""mnk.optim.MnkAdam and torch.optim.Adam under the same user actions.

MnkAdam is handed to user-owned loops in place of torch.optim.Adam.  Its gradients do not travel
through `p.grad`: the convolutions' backward writes weight-gradient partials towards optimiser-owned sinks as a side effect
(mnk.ops.wgrad_sink_owner, DeferredReducer.wgrad).  The loops this repository ships call backward(); step(); zero_grad() and
nothing else.  Here the same seeded Hourglass is trained three iterations, once per optimiser class on the same backend, while the
loop does what PyTorch users do: zero_grad(set_to_none=False), a MultiStepLR, a checkpoint loaded into the other class, a gradient
read that asks for the INPUT's gradient only before the normal backward (gradient penalty, saliency), torch.autograd.grad of a
convolution weight, clip_grad_norm_.

Bound on every parameter after every step, the one of tests/test_kernels_optim.py::test_adam_multi_matches_torch_adam_and_emits_
the_packs: 2e-6 * max |p| + 4e-7 * (lr / 2e-4) per step taken (with a scheduler: summed over the steps' learning rates).

The two departures of MnkAdam that INTEGRATION.md lists (3 and 4 of its opening list) are pinned here: `p.grad` of the sunk
weights is None until materialize_grads() (the clip scenario calls it first, as the document says), and the ONE step count in the
device scalars (the strict xfail below)."""
import gc

import pytest
import torch

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

LR, BETAS, ITERS = 1e-3, (0.5, 0.999), 3
WEIGHTS = ("encoder.down_blocks.1.conv.weight", "decoder.up_blocks.0.conv.weight")      # a plain and an up-sampled convolution
WORST = {}                                   # scenario -> the largest |p(MnkAdam) - p(Adam)| seen, printed by every case


def make_net(be):
    from modules.util import Hourglass
    torch.manual_seed(17)
    hg = Hourglass(block_expansion=8, in_features=3, out_features=4, num_blocks=2, max_features=32)
    return hg.to(be.device).train()


def make_opt(mnk, params):
    from mnk.optim import MnkAdam
    return (MnkAdam if mnk else torch.optim.Adam)(params, lr=LR, betas=BETAS)


def loop(be, mnk, extra=None, set_to_none=True, scheduler=False, swap=False, clip=None, x_grad=False, late_param=False):
    """Three iterations of  out = hg(x); loss = sum(out * w) / 10; [extra]; loss.backward(); [clip]; step(); zero_grad().
    -> {"params": per iteration [parameter copies on the host], "lrs": the learning rate of every step, "extra": what `extra`
    returned per iteration, "norms": what clip_grad_norm_ returned, "grad_none": per iteration {name: p.grad is None before the
    step}}"""
    from mnk import ops
    hg = make_net(be)
    params = list(hg.parameters())
    late = torch.nn.Parameter(be.t(torch.tensor([1.0, 0.8, 1.2, 0.9]))) if late_param else None
    if late is not None:
        params.append(late)
    opt = make_opt(mnk, params)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1) if scheduler else None
    g = torch.Generator().manual_seed(23)
    x = be.t(torch.rand(3, 3, 1, 16, 16, generator=g)).requires_grad_(bool(x_grad or extra))
    w = be.t(torch.randn(3, 4, 1, 16, 16, generator=g))
    res = {"params": [], "lrs": [], "extra": [], "norms": [], "grad_none": []}
    for it in range(ITERS):
        out = hg(x)
        if late is not None and it > 0:              # the late parameter takes no part in the first iteration: no gradient there
            out = out * late.view(1, 4, 1, 1, 1)
        loss = (out * w).sum() / 10
        if extra is not None:
            res["extra"].append(extra(hg, out, loss, x))
            x.grad = None
        loss.backward()
        if clip is not None:
            if hasattr(opt, "materialize_grads"):
                opt.materialize_grads()              # before anything reads p.grad between backward() and step()
            res["grad_none"].append({k: p.grad is None for k, p in hg.named_parameters()})
            res["norms"].append(float(torch.nn.utils.clip_grad_norm_(params, clip)))
        res["lrs"].append(float(opt.param_groups[0]["lr"]))
        opt.step()
        opt.zero_grad(set_to_none=set_to_none)
        x.grad = None
        if sched is not None:
            sched.step()
        be.sync()
        res["params"].append([p.detach().cpu().clone() for p in params])
        assert ops.handover_state() == {}, ops.handover_state()
        if swap and it == 0:
            # a checkpoint of this optimiser, loaded into a fresh one of the OTHER class (logger.py:43-66 saves / restores them)
            # (an MnkAdam owns its parameters' weight gradients for as long as it is alive -- the sinks are registered by parameter
            # -- and holds a reference cycle with its reducer: it has to be collected before another optimiser takes over)
            sd = opt.state_dict()
            opt = None
            gc.collect()
            opt = make_opt(not mnk, params)
            opt.load_state_dict(sd)
    opt = sched = None
    gc.collect()                                     # (no sink registration outlives the case)
    return res


def assert_same_trajectory(be, a, b, scenario):
    """every parameter after every step: |a - b| <= 2e-6 * max |b| + 4e-7 * sum over the steps taken of lr / 2e-4"""
    assert a["lrs"] == b["lrs"], (a["lrs"], b["lrs"])
    worst, allowance = 0.0, 0.0
    for it, (pa, pb) in enumerate(zip(a["params"], b["params"])):
        allowance += 4e-7 * b["lrs"][it] / 2e-4
        for k, (u, v) in enumerate(zip(pa, pb)):
            d = float((u - v).abs().max())
            worst = max(worst, d)
            assert d <= 2e-6 * float(v.abs().max()) + allowance, (scenario, "iteration %d parameter %d" % (it, k), d)
    WORST[(be.kind, scenario)] = worst
    print("max |p(MnkAdam) - p(Adam)| %s %s: %.2e" % (be.kind, scenario, worst))


# The input-only reads differentiate ANOTHER scalar than the loss (a saliency map, the inner gradient of a gradient penalty):
# Adam's update does not change when a gradient is scaled, so stray weight-gradient partials of the loss itself -- which would
# exactly double the step's gradient -- could not be seen in the trajectory.
def input_only_grad(hg, out, loss, x):
    return torch.autograd.grad(out.square().sum(), x, retain_graph=True)[0].detach().cpu().clone()


def input_only_backward(hg, out, loss, x):
    out.square().sum().backward(inputs=[x], retain_graph=True)
    return x.grad.detach().cpu().clone()


def weight_grad(hg, out, loss, x):
    named = dict(hg.named_parameters())
    ws = [named[k] for k in WEIGHTS]
    return [t.detach().cpu().clone() for t in torch.autograd.grad(loss, ws, retain_graph=True)]


SCENARIOS = {
    "plain": {},
    "zero_grad(set_to_none=False)": dict(set_to_none=False),
    "MultiStepLR": dict(scheduler=True),
    "input-only autograd.grad(s, x) first": dict(extra=input_only_grad),
    "input-only s.backward(inputs=[x]) first": dict(extra=input_only_backward),
    "autograd.grad(loss, weights) first": dict(extra=weight_grad),
}


@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_same_trajectory_as_adam(be, scenario):
    """MnkAdam against torch.optim.Adam under the same actions.  The reads that ask for the input's gradient only must leave no
    weight-gradient partials in the sinks (they would be added to the next step's gradient); what they return is stock's."""
    kw = SCENARIOS[scenario]
    ours, stock = loop(be, True, **kw), loop(be, False, **kw)
    for a, b in zip(ours["extra"], stock["extra"]):
        for u, v in zip(*((a, b) if isinstance(a, list) else ([a], [b]))):
            # (both sides are this package's kernels: the per-layer gradient path on either; the bound is the parameter-gradient
            # one of the module tests, 2e-4 relative L2 against fp64, for two fp32 results)
            e = float((u - v).norm() / (v.norm() + 1e-30))
            print("returned gradient, relative L2 difference: %.2e" % e)
            assert e < 4e-4, (scenario, e)
    assert_same_trajectory(be, ours, stock, scenario)


@pytest.mark.parametrize("mnk_first", [True, False], ids=["MnkAdam-to-Adam", "Adam-to-MnkAdam"])
def test_state_dict_loads_into_the_other_class(be, mnk_first):
    """After the first iteration a fresh optimiser of the other class loads the first one's state_dict() and continues: the same
    trajectory as stock Adam all the way."""
    swapped, stock = loop(be, mnk_first, swap=True), loop(be, False)
    assert_same_trajectory(be, swapped, stock, "state_dict %s" % ("MnkAdam -> Adam" if mnk_first else "Adam -> MnkAdam"))


def test_clip_grad_norm_after_materialize_grads(be):
    """Departure 3 of INTEGRATION.md: until materialize_grads() the `p.grad` of a sunk convolution weight is None, so
    clip_grad_norm_ between backward() and step() would see a part of the gradient only.  With materialize_grads() first, every
    parameter that has a gradient under stock Adam has one, the norms are stock's and so is the clipped trajectory."""
    ours, stock = loop(be, True, clip=0.05), loop(be, False, clip=0.05)
    assert ours["grad_none"] == stock["grad_none"]
    for a, b in zip(ours["norms"], stock["norms"]):
        print("clip_grad_norm_: %.6f (MnkAdam) %.6f (Adam)" % (a, b))
        assert b > 0.05, "the clip must bite"
        # two fp32 gradients of the same graph, each within 2e-4 relative L2 of fp64 (the module tests' bound): so are their norms
        assert abs(a - b) <= 4e-4 * b, (a, b)
    assert_same_trajectory(be, ours, stock, "materialize_grads + clip_grad_norm_(0.05)")


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="departure 4 of INTEGRATION.md: MnkAdam keeps ONE step count in its device scalars, torch.optim.Adam one "
                   "per parameter -- a parameter whose first gradient arrives at the second step gets the bias correction of step "
                   "2 instead of step 1.  Remove this mark together with a per-parameter step count.")
def test_parameter_without_a_gradient_in_the_first_iteration(be):
    """A parameter that takes no part in the first iteration's loss (p.grad is None at the first step): Adam starts its step count
    at that parameter's own first update.  Measured on the emulator: the parameters differ by 5.8e-5 after that parameter's first
    update and by 7.7e-5 after three iterations, ten times the bound."""
    ours, stock = loop(be, True, late_param=True), loop(be, False, late_param=True)
    assert_same_trajectory(be, ours, stock, "late parameter")


def test_kxk_convolution_under_the_same_requests(be):
    """The discriminator's 4 x 4 convolution node (ops.ConvKxKFn) owned by an MnkAdam, outside the discriminator's own loop (which
    wraps its input-only pass in ops.no_param_grads): an input-only read of another scalar, then torch.autograd.grad of the weight
    itself, then the normal backward() and step(), twice.  The returned gradients are stock's (4e-4 relative L2: two fp32 results,
    each within the module tests' 2e-4 of fp64) and the trajectory is stock Adam's."""
    from mnk import ops
    g = torch.Generator().manual_seed(31)
    cin, cout, n, hw = 5, 9, 3, 11                   # 11 - 4 + 1 = 8 x 8 outputs; odd channel counts, an odd map
    host = {"w": torch.randn(cout, cin, 1, 4, 4, generator=g) * 0.1, "b": torch.randn(cout, generator=g) * 0.1,
            "x": torch.rand(n, cin, 1, hw, hw, generator=g), "g": torch.randn(n, cout, 1, hw - 3, hw - 3, generator=g)}

    def run(mnk):
        w, b = (torch.nn.Parameter(be.t(host[k])) for k in ("w", "b"))
        opt = make_opt(mnk, [w, b])
        x, gw = be.t(host["x"]).requires_grad_(True), be.t(host["g"])
        res = {"params": [], "lrs": [], "extra": []}
        for it in range(2):
            out = ops.from_act(ops.ConvKxKFn.apply(ops.to_act(x), w, b, cin, 4, 4, 0), cout, n)
            loss = (out * gw).sum() / 10
            dx = torch.autograd.grad(out.square().sum(), x, retain_graph=True)[0]
            dw = torch.autograd.grad(loss, [w], retain_graph=True)[0]
            res["extra"].append([dx.detach().cpu().clone(), dw.detach().cpu().clone()])
            loss.backward()
            res["lrs"].append(LR)
            opt.step()
            opt.zero_grad()
            x.grad = None
            be.sync()
            res["params"].append([w.detach().cpu().clone(), b.detach().cpu().clone()])
            assert ops.handover_state() == {}
        opt = None
        gc.collect()
        return res

    ours, stock = run(True), run(False)
    for a, b in zip(ours["extra"], stock["extra"]):
        for u, v in zip(a, b):
            assert float((u - v).norm() / (v.norm() + 1e-30)) < 4e-4
    assert_same_trajectory(be, ours, stock, "4x4 convolution: input-only read, weight read, step")
