"""Opt-in bf16 (mixed-precision) training: mnk.ops.training_precision, TrainStep(precision="bf16"), MNK_TRAIN_PRECISION.  The 3x3
convolutions of generator and key-point detector run forward (MNK_CONV_BF16_TRAIN), data gradient (the same flag) and weight
gradient (MNK_WGRAD_BF16) on operands rounded to nearest-even bf16 with fp32 accumulation; everything else stays fp32.

The reference of the autograd- and model-level tests is an fp64 torch.autograd.Function whose forward convolves rounded x and w
and whose backward uses rounded dy -- patched over oracle.restate.conv for the whole iteration, the pattern of
tests/test_inference_bf16.py::_check_model.

Whole iteration on tests/golden/step_tiny.pt, distance from the fp64 iteration / the rounded restatement's own distance (bound 2):
  CPU emulator   losses 1.56   prediction 1.10   deformed 1.02   updates (per network, Euclidean) generator 1.05, key-point
                 detector 0.93, discriminator 1.05
  MI355X         losses 1.55   prediction 1.12   deformed 1.02   updates: generator 1.07, key-point detector 0.90, discriminator 1.04"""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import cases, restate
from test_modules import build, load
from _util import ceil4, relerr

TOL = 2e-6        # the kernel tolerance of tests/test_kernels_conv_bf16_train.py
PIN = 2e-5        # tests/test_step.py: the constant of its bound on the loss history


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class RoundedConv(torch.autograd.Function):
    """3x3 / pad 1 convolution of rounded x and rounded w; data and weight gradients from rounded dy (the bias gradient is a plain
    column sum of dy: the kernels do not round there)"""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = _bf(x), _bf(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_bias = b is not None
        return F.conv2d(xr, wr, b, padding=1)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = _bf(dy)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, padding=1)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, padding=1)
        return dx, dw, dy.sum(dim=(0, 2, 3)) if ctx.has_bias else None


def _rounded_conv(ctx, x, prefix, padding=1, groups=1):
    """restate.conv with the 3x3 convolutions replaced by RoundedConv"""
    w = ctx.p(prefix + ".weight")[:, :, 0]
    b = ctx.sd.get(prefix + ".bias")
    if tuple(w.shape[-2:]) == (3, 3) and groups == 1 and padding == 1:
        return RoundedConv.apply(x, w, b)
    return F.conv2d(x, w, b, padding=padding, groups=groups)


# ---- scope semantics ----------------------------------------------------------------------------------------------------------------
def _act(be, t):
    """(N, C, H, W) -> the NHWC activation layout with zero pad channels"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, ceil4(c))
    out[..., :c] = t.permute(0, 2, 3, 1)
    return be.t(out)


def _plain_layer(be, seed=0):
    """a tap-major shape (72 -> 48 channels on an 8 x 8 map): its three GEMMs all have a bf16 form"""
    g = torch.Generator().manual_seed(seed)
    x = _act(be, torch.randn(1, 72, 8, 8, generator=g)).requires_grad_(True)
    w = be.t(torch.randn(48, 72, 1, 3, 3, generator=g) * 0.2).requires_grad_(True)
    dy = _act(be, torch.randn(1, 48, 8, 8, generator=g))
    return x, w, dy


def test_training_precision_scope_semantics(be):
    from mnk import ops
    assert ops.current_training_precision() == "fp32"
    with ops.training_precision("bf16"):
        assert ops.current_training_precision() == "bf16" and ops.current_precision() == "fp32"
        with ops.training_precision("fp32"):
            assert ops.current_training_precision() == "fp32"
        assert ops.current_training_precision() == "bf16"
    assert ops.current_training_precision() == "fp32"
    with pytest.raises(ZeroDivisionError):
        with ops.training_precision("bf16"):
            1 / 0
    assert ops.current_training_precision() == "fp32"
    with pytest.raises(ValueError):
        ops.training_precision("fp16")

    x, w, dy = _plain_layer(be)

    def run(inside_backward):
        x.grad = w.grad = None
        with ops.training_precision("bf16"):
            y, _ = ops.conv3x3(x, 72, w)
            if inside_backward:
                y.backward(dy)
        if not inside_backward:
            y.backward(dy)                 # after the scope was left: the node recorded its precision
        be.sync()
        return y.detach().clone(), x.grad.clone(), w.grad.clone()

    inside, outside = run(True), run(False)
    for a, b in zip(inside, outside):
        assert torch.equal(a, b)
    x.grad = w.grad = None
    y32, _ = ops.conv3x3(x, 72, w)
    y32.backward(dy)
    be.sync()
    for a, b in zip(inside, (y32.detach(), x.grad, w.grad)):
        assert not torch.equal(a, b), "the scope changed nothing"
    # no_grad calls inside the scope are not touched, and inference_precision keeps its semantics inside and outside of it
    with torch.no_grad():
        plain, _ = ops.conv3x3(x, 72, w)
        with ops.inference_precision("bf16"):
            inf16, _ = ops.conv3x3(x, 72, w)
    with ops.training_precision("bf16"):
        with torch.no_grad():
            scoped, _ = ops.conv3x3(x, 72, w)
            with ops.inference_precision("bf16"):
                scoped16, _ = ops.conv3x3(x, 72, w)
        with ops.inference_precision("bf16"):
            with pytest.raises(RuntimeError, match="gradients enabled"):
                ops.conv3x3(x, 72, w)
            with pytest.raises(RuntimeError, match="batch statistics"):
                with torch.no_grad():
                    ops.conv3x3(x, 72, w, want_stats=True)
    be.sync()
    assert torch.equal(plain, y32.detach()) and torch.equal(scoped, plain)
    assert torch.equal(scoped16, inf16) and not torch.equal(inf16, plain)
    assert torch.equal(inf16, inside[0]), "training and inference forms share the one-pass forward kernel"
    assert ops.handover_state() == {}


# ---- autograd level -------------------------------------------------------------------------------------------------------------------
# (n, h, w of the source, c0, c1, cout, up-sampled, residual): tap-major / compact-K / sub-pixel shapes of tests/test_kernels_conv.py
AUTOGRAD_CASES = [(1, 8, 8, 72, 0, 48, False, True),
                  (2, 2, 4, 40, 70, 68, False, False),
                  (2, 16, 8, 20, 0, 136, True, False)]


@pytest.mark.parametrize("owned", [False, True], ids=["direct-wgrad", "deferred-wgrad"])
@pytest.mark.parametrize("case", AUTOGRAD_CASES)
def test_conv3x3_under_the_scope_against_the_rounded_fp64_function(be, case, owned):
    """y, dx of every source and dw against RoundedConv in fp64 at the kernel tolerance.  owned: the weight belongs to an
    mnk.optim.MnkAdam, so its gradient takes the deferred / grouped path (MnkWgradJob.flags) instead of mnk_conv3x3_wgrad"""
    from mnk import ops, optim as moptim
    n, h, w, c0, c1, cout, ups, use_res = case
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(n, c0, h, w, generator=g)
    x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    # integers / 64: the pre-summed packs of the sub-pixel forms are exact, their rounding is the rounding of the sums
    wt = torch.randint(-40, 41, (cout, c0 + c1, 3, 3), generator=g).float() / 64
    b = torch.randn(cout, generator=g)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    res = torch.randn(n, cout, ho, wo, generator=g) if use_res else None
    dy = torch.randn(n, cout, ho, wo, generator=g)
    # reference
    xs = [t.double().requires_grad_(True) for t in (x0, x1) if t is not None]
    wd, bd = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    xin = torch.cat(xs, 1)
    if ups:
        from test_kernels_conv_bf16_train import _subpixel_rounded
        # (forward and dx; dw below.  The rounding of x as a detached offset: a cast's backward would round the gradient too)
        ref = _subpixel_rounded(xin + (_bf(xin) - xin).detach(), wd) + bd[None, :, None, None]
    else:
        ref = RoundedConv.apply(xin, wd, bd)
    if use_res:
        ref = ref + res.double()
    ref.backward(_bf(dy).double() if ups else dy.double())
    if ups:       # the weight gradient of the up-sampled layer: rounded x (up-sampled) and rounded dy
        w2 = wt.double().requires_grad_(True)
        F.conv2d(F.interpolate(_bf(torch.cat([x0] + ([x1] if c1 else []), 1)).double(), scale_factor=2, mode="nearest"), w2,
                 None, padding=1).backward(_bf(dy).double())
        dw_ref = w2.grad
    else:
        dw_ref = wd.grad
    # the kernels
    X0 = _act(be, x0).requires_grad_(True)
    X1 = _act(be, x1).requires_grad_(True) if c1 else None
    W = be.t(wt.view(cout, c0 + c1, 1, 3, 3).contiguous()).requires_grad_(True)
    B = be.t(b).requires_grad_(True)
    opt = moptim.MnkAdam([W, B], lr=1e-3, betas=(0.5, 0.999)) if owned else None
    with ops.training_precision("bf16"):
        y, _ = ops.conv3x3(X0, c0, W, B, x1=X1, c1=c1, ups=ups, residual=_act(be, res) if use_res else None)
    y.backward(_act(be, dy))
    if owned:
        opt.materialize_grads()
    be.sync()
    errs = {"y": relerr(y.detach().cpu()[..., :cout].permute(0, 3, 1, 2), ref.detach()),
            "dx0": relerr(X0.grad.cpu()[..., :c0].permute(0, 3, 1, 2), xs[0].grad),
            "dw": relerr(W.grad.cpu().view(cout, c0 + c1, 3, 3), dw_ref)}
    if c1:
        errs["dx1"] = relerr(X1.grad.cpu()[..., :c1].permute(0, 3, 1, 2), xs[1].grad)
    print("conv3x3 under training_precision(bf16) %s %s: %s" % (case, "deferred" if owned else "direct",
                                                                {k: "%.3g" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < TOL, (k, v)
    assert relerr(B.grad.cpu(), dy.double().sum(dim=(0, 2, 3))) < 1e-5
    assert ops.handover_state() == {}


def test_one_reducer_serves_bf16_and_fp32_nodes_of_the_same_backward(be):
    """two tap-major layers of one optimiser, one called inside the scope and one outside: the grouped launch builds one table
    per precision, and each gradient is its own node's"""
    from mnk import ops, optim as moptim
    x, w1, dy = _plain_layer(be, seed=1)
    _, w2, _ = _plain_layer(be, seed=2)

    def grads(scoped1, scoped2, owned):
        for t in (x, w1, w2):
            t.grad = None
        opt = moptim.MnkAdam([w1, w2], lr=1e-3, betas=(0.5, 0.999)) if owned else None
        with ops.training_precision("bf16" if scoped1 else "fp32"):
            y1, _ = ops.conv3x3(x, 72, w1)
        with ops.training_precision("bf16" if scoped2 else "fp32"):
            y2, _ = ops.conv3x3(x, 72, w2)
        torch.autograd.backward([y1, y2], [dy, dy])
        if owned:
            opt.materialize_grads()
        be.sync()
        out = w1.grad.clone(), w2.grad.clone()
        if owned:
            opt.zero_grad()
            del opt
        return out

    a16, _ = grads(True, True, False)
    a32, b32 = grads(False, False, False)
    mixed = grads(True, False, True)             # (last: the optimiser stays registered as the owner of the two weights)
    assert relerr(mixed[0], a16) < TOL and relerr(mixed[1], b32) < TOL          # (grouped and single launches split pixels differently)
    assert relerr(a16, a32) > 1e-4 and relerr(mixed[0], a32) > 1e-4             # ... and the bf16 node did round


# ---- whole iteration ---------------------------------------------------------------------------------------------------------------
def _models(gold, be, cfg=None):
    gen, disc, kpd = build(cfg or gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"])
    disc.load_state_dict(gold["state"]["discriminator"])
    kpd.load_state_dict(gold["state"]["kp_detector"])
    return gen.to(be.device), disc.to(be.device), kpd.to(be.device)


def _batch(gold, be):
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    return {"source": be.t(src), "video": be.t(drv)}


def _run_step(gold, be, **kw):
    """one TrainStep iteration from the golden's weights -> (losses, generated, parameters after, the step object)"""
    from mnk import engine
    gen, disc, kpd = _models(gold, be)
    step = engine.TrainStep(gen, disc, kpd, gold["cfg"]["train_params"], **kw)
    g_l, d_l, generated = step.step(_batch(gold, be))
    be.sync()
    losses = [float(v) for v in g_l] + [float(v) for v in d_l]
    out = {k: generated[k].detach().cpu().clone() for k in ("video_prediction", "video_deformed")}
    params = {n + "." + k: v.detach().cpu().clone() for n, m in (("generator", gen), ("discriminator", disc), ("kp_detector", kpd))
              for k, v in m.named_parameters()}
    return losses, out, params, step


def _restated_iteration(gold):
    """the iteration of train.py:110-136 restated in fp64 (oracle/restate.py + autograd + Adam's first step): losses, generated
    frames and the update of every parameter"""
    cfg = gold["cfg"]
    tp = cfg["train_params"]
    assert tp["detach_kp_discriminator"]
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    sds = restate.to_dtype(gold["state"], torch.float64)
    leaves = {}
    for n in ("generator", "kp_detector", "discriminator"):
        for k, v in sds[n].items():
            if v.is_floating_point() and "running" not in k:
                sds[n][k] = leaves[n + "." + k] = v.clone().requires_grad_(True)
    g_losses, gen, kp_joined, _, _ = restate.generator_full_forward(sds, cfg, src.double(), drv.double())
    g_means = [v.mean() for v in g_losses]
    gk = [k for k in leaves if not k.startswith("discriminator.")]
    g_grads = torch.autograd.grad(sum(g_means), [leaves[k] for k in gk], allow_unused=True)
    d_losses = restate.discriminator_full_forward(sds, cfg, drv.double(), {k: v.detach() for k, v in kp_joined.items()},
                                                  {k: v.detach() for k, v in gen.items()})
    d_means = [v.mean() for v in d_losses]
    dk = [k for k in leaves if k.startswith("discriminator.")]
    d_grads = torch.autograd.grad(sum(d_means), [leaves[k] for k in dk], allow_unused=True)
    lr, eps = tp["lr"], 1e-8
    updates = {}
    for k, g in list(zip(gk, g_grads)) + list(zip(dk, d_grads)):
        if g is not None:
            updates[k] = -lr * g / (g.abs() + eps)          # Adam's first step: m / (1 - b1) = g, sqrt(v / (1 - b2)) = |g|
    return ([float(v.detach()) for v in g_means + d_means],
            {k: gen[k].detach() for k in ("video_prediction", "video_deformed")}, updates)


def _dist(a, b):
    return float((a.double() - b.double()).abs().max())


def test_bf16_iteration_is_within_twice_the_rounded_restatement_error(be, monkeypatch):
    """losses, generated frames and parameter updates of TrainStep(precision="bf16") are off the fp64 iteration by at most twice
    what the fp64 restatement with RoundedConv is off it, plus the pin of tests/test_step.py (updates: plus the fp32 spacing of the
    parameter they are added to).  Biases whose gradient is analytically zero (rounding noise under Adam's sign-like first update,
    cases.is_noise_bias) are left out, as tests/test_step.py leaves them out."""
    from mnk import ops
    gold = load("step_tiny")
    l64, out64, upd64 = _restated_iteration(gold)
    h64 = gold["history64"][0]["generator"] + gold["history64"][0]["discriminator"]
    assert max(abs(a - b) for a, b in zip(l64, h64)) < 1e-9, "the un-patched restatement must reproduce the recorded fp64 iteration"
    monkeypatch.setattr(restate, "conv", _rounded_conv)
    l16, out16, upd16 = _restated_iteration(gold)
    monkeypatch.undo()
    losses, out, params, step = _run_step(gold, be, precision="bf16")
    assert ops.handover_state() == {}
    rel = lambda a, b: abs(a - b) / max(1.0, abs(b))
    e_ref = max(rel(a, b) for a, b in zip(l16, l64))
    err = max(rel(a, b) for a, b in zip(losses, l64))
    report = {"losses": (err, e_ref)}
    assert e_ref > 1e-6, "the rounded restatement did not round"
    assert err <= 2 * e_ref + PIN, ("losses", err, e_ref)
    for k in out64:
        e_ref, err = _dist(out16[k], out64[k]), _dist(out[k], out64[k])
        report[k] = (err, e_ref)
        assert e_ref > 1e-6 and err <= 2 * e_ref + PIN, (k, err, e_ref)
    # Parameter updates: Adam's first update is -lr * sign(g) wherever |g| >> eps, so an update is off by 2 lr where a gradient
    # element changes its sign and by next to nothing elsewhere.  The maximum over a tensor is therefore 2 lr or ~0 -- one
    # realisation of which elements flip (the nearest-neighbour warp makes single pixels of the prediction jump, and the
    # discriminator's gradients with them) -- so the distance is taken per NETWORK in the Euclidean norm, which counts the flipped
    # elements: twice the distance = four times as many flips as the rounded restatement has.
    before = {n + "." + k: v for n in gold["state"] for k, v in gold["state"][n].items()}
    for net in ("generator", "kp_detector", "discriminator"):
        keys = [k for k in upd64 if k.startswith(net + ".") and not cases.is_noise_bias(k.split(".", 1)[1])]
        e_ref = sum(float((upd16[k] - upd64[k]).pow(2).sum()) for k in keys) ** 0.5
        err = sum(float(((params[k] - before[k]).double() - upd64[k]).pow(2).sum()) for k in keys) ** 0.5
        count = sum(upd64[k].numel() for k in keys)
        # the fp32 spacing of the parameters the updates are added to, over all elements
        pin = 2.0 ** -23 * max(1.0, max(float(before[k].abs().max()) for k in keys)) * count ** 0.5
        report["updates of " + net] = (err, e_ref)
        assert err <= 2 * e_ref + pin, (net, err, e_ref)
    print("bf16 iteration on %s: (|out - fp64|, e_ref) %s" % (be.kind, report))


def test_precision_flavours_and_determinism(be):
    """precision="fp32" is the default bit for bit; "bf16" differs from it; two bf16 runs are bit-identical and leave no hand-over"""
    from mnk import ops
    gold = load("step_tiny")
    base = _run_step(gold, be)
    fp32 = _run_step(gold, be, precision="fp32")
    a = _run_step(gold, be, precision="bf16")
    assert ops.handover_state() == {}
    b = _run_step(gold, be, precision="bf16")
    assert ops.handover_state() == {} and ops.current_training_precision() == "fp32"
    assert base[0] == fp32[0] and all(torch.equal(base[1][k], fp32[1][k]) for k in base[1])
    assert all(torch.equal(base[2][k], fp32[2][k]) for k in base[2])
    assert a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert a[0] != base[0] and not torch.equal(a[1]["video_prediction"], base[1]["video_prediction"])
    with pytest.raises(ValueError):
        _run_step(gold, be, precision="fp16")


@pytest.mark.gpu
def test_bf16_hipgraph_replay_equals_the_eager_bf16_iteration():
    """replay 0 of the captured bf16 iteration equals eager iteration 0 bit for bit; the captured step kept its precision"""
    from conftest import Backend
    be = Backend("hip")
    gold = load("step_tiny")
    eager = _run_step(gold, be, precision="bf16")
    graph = _run_step(gold, be, precision="bf16", use_graph=True)
    plain = _run_step(gold, be, use_graph=True)
    assert eager[0] == graph[0]
    assert all(torch.equal(eager[1][k], graph[1][k]) for k in eager[1])
    assert all(torch.equal(eager[2][k], graph[2][k]) for k in eager[2])
    assert graph[0] != plain[0]


def test_train_pair_runner_follows_mnk_train_precision(be, monkeypatch):
    """MNK_TRAIN_PRECISION=bf16 behind the reference's loop (mnk.dropin.TrainPairRunner): a program of its own per precision, and
    one iteration equals TrainStep(precision="bf16")'s within what tests/test_dropin_replay.py allows between the runner and the
    modules run as they are (losses 2e-4; parameters: Adam's sign-like first update, at most ~2 lr on an element whose gradient is
    rounding noise -- that test's 6.5 lr over three steps -- and a mean of 0.25 lr)"""
    from mnk import dropin
    from test_dropin_replay import _reference_loop
    gold = load("step_tiny")
    want_l, _, want_p, _ = _run_step(gold, be, precision="bf16")
    base_l = _run_step(gold, be)[0]
    monkeypatch.setenv("MNK_TRAIN_PRECISION", "bf16")
    hist, nets, _, (gpar, dpar) = _reference_loop(be, "torch", 1, gold)
    runner = dropin.runner_for(gpar.module)
    assert runner is not None and runner.stats["fallbacks"] == 0 and runner.stats["d_fallbacks"] == 0, runner.stats
    for va, vb in zip(hist[0], want_l):
        assert abs(va - vb) <= 2e-4 * max(1.0, abs(vb)), (hist[0], want_l)
    assert max(abs(a - b) for a, b in zip(hist[0], base_l)) > 10 * max(abs(a - b) for a, b in zip(hist[0], want_l))
    lr = gold["cfg"]["train_params"]["lr"]
    for name, m in zip(("generator", "discriminator", "kp_detector"), nets):
        tot = cnt = 0.0
        for k, p in m.named_parameters():
            d = (p.detach().cpu() - want_p[name + "." + k]).abs()
            tot, cnt = tot + float(d.sum()), cnt + d.numel()
            assert float(d.max()) <= 6.5 / 3 * lr, (name, k, float(d.max()))
        assert tot / cnt <= 0.25 * lr, (name, tot / cnt)
    if be.kind == "hip":
        # the precision is part of the program key: the same wrappers under fp32 capture a program of their own instead of
        # replaying the bf16 one
        src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
        x = {"source": src, "video": drv}
        assert runner.stats["captures"] == 1 and [k[-1] for k in runner.programs] == ["bf16"]
        monkeypatch.setenv("MNK_TRAIN_PRECISION", "fp32")
        for p in (q for m in nets for q in m.parameters()):
            p.grad = None
        out = gpar(x)
        sum(v.mean() for v in out[:-2]).backward()
        torch.cuda.synchronize()
        assert runner.stats["captures"] == 2 and runner.stats["fallbacks"] == 0, runner.stats
        assert sorted(k[-1] for k in runner.programs) == ["bf16", "fp32"]
