"""Gradient-level parity of the drop-in runner (mnk.dropin.TrainPairRunner), on the path it serves and on every path where it
hands the call back to the modules as they are.

tests/test_dropin_replay.py compares loss histories and the parameters after three Adam steps: Adam's first steps are sign-like,
so a gradient with the right sign and the wrong magnitude -- or no gradient at all for a few tensors -- passes those bounds.
Here every parameter's `p.grad` is taken right after the `loss.backward()` that completes it and before anything else reads it
(what clip_grad_norm_, a stock optimiser or any other reader of p.grad sees):

  A  one served iteration (eager phases on the emulator, hipGraph replay on the MI355X) against the fp64 oracle
     (oracle/restate.py) on the same weights and batch; tolerance per tensor from the oracle's own fp32-vs-fp64 distance, the
     rule of tests/test_fullsize_oracle.py;
  B  each documented fall-back after a served iteration -- a stale gradient, the discriminator called on other tensors, a
     discriminator weight changed in between, zero_grad(set_to_none=False) -- then backward and step, with stock Adam (adopted
     by mnk.optim.AdoptedAdam), stock SGD and clip_grad_norm_ in front of the step, against the same statements with
     MNK_DROPIN_GRAPH=0 (no runner at all);
  C  train_params['detach_kp_discriminator'] = False (never served: the key-point detector's gradient has two contributions);
  D  storage swaps that keep `_version` (`p.data = ...`) under the frozen-weight EvalRunner and the TrainPairRunner (MI355X);
  E  a failure in the warm-up before the capture (MI355X): the call is served by the modules, nothing of the warm-up is left.
"""
import copy

import pytest
import torch

from oracle import cases, restate
from test_modules import build, load

NETS = ("generator", "discriminator", "kp_detector")


def _setup(be, gold, opt="adam", detach_kp_discriminator=True):
    """train.py:81-105 on the drop-in modules (tests/test_dropin_replay.py::_reference_loop's setup); opt = "adam" (stock
    torch.optim.Adam), "sgd" (stock torch.optim.SGD) or "clip" (stock Adam, clip_grad_norm_ in front of every step)"""
    from mnk.engine import GeneratorFullModel, DiscriminatorFullModel
    from sync_batchnorm import DataParallelWithCallback
    config = copy.deepcopy(gold["cfg"])
    tp = config["train_params"]
    tp["detach_kp_discriminator"] = detach_kp_discriminator
    generator, discriminator, kp_detector = build(config)
    nets = (generator, discriminator, kp_detector)
    for m, k in zip(nets, NETS):
        m.load_state_dict(gold["state"][k])
        m.to(be.device)
    if opt == "sgd":
        opts = [torch.optim.SGD(m.parameters(), lr=tp["lr"]) for m in nets]
    else:
        opts = [torch.optim.Adam(m.parameters(), lr=tp["lr"], betas=(0.5, 0.999)) for m in nets]
    ids = [0] if be.kind == "hip" else None
    pars = (DataParallelWithCallback(GeneratorFullModel(kp_detector, generator, discriminator, tp), device_ids=ids),
            DataParallelWithCallback(DiscriminatorFullModel(kp_detector, generator, discriminator, tp), device_ids=ids))
    return tp, nets, opts, pars


def _grads(m):
    return {n: (p.grad.detach().cpu().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _batch(gold):
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    return src, drv


def _iteration(be, tp, nets, opts, pars, trigger=None, clip=None, set_to_none=True, probe=None):
    """train.py:110-136 (the statements of _reference_loop) -> {network: {name: p.grad}, "norms": [clip_grad_norm_ results],
    "losses": [...]}.  trigger: "stale_grad" (a zero gradient left on one generator parameter), "clone" (the discriminator pass on
    copies of this iteration's outputs), "d_weight" (a discriminator weight changed in place between the two calls).
    probe(nets) runs right after generator_full_par(x) returns."""
    generator, discriminator, kp_detector = nets
    og, od, ok = opts
    gpar, dpar = pars
    detach = tp["detach_kp_discriminator"]
    src, drv = _batch(load("step_tiny"))
    x = {"source": src, "video": drv}
    rec = {"norms": []}
    if trigger == "stale_grad":
        p = next(generator.parameters())
        p.grad = torch.zeros_like(p)

    def step(o, m):
        if clip is not None:
            rec["norms"].append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), clip)))
        o.step()
        o.zero_grad(set_to_none=set_to_none)

    out = gpar(x)
    if probe is not None:
        probe(nets)
    loss_values = [v.mean() for v in out[:-2]]
    generated, kp_joined = out[-2], out[-1]
    sum(loss_values).backward(retain_graph=not detach)
    rec["generator"] = _grads(generator)
    if detach:
        rec["kp_detector"] = _grads(kp_detector)
    losses = [float(v.detach().cpu()) for v in loss_values]
    step(og, generator)
    od.zero_grad(set_to_none=set_to_none)
    if detach:
        step(ok, kp_detector)
    if trigger == "clone":
        generated = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in generated.items()}
    if trigger == "d_weight":
        with torch.no_grad():
            dict(discriminator.named_parameters())["down_blocks.1.conv.weight"].mul_(1.01)
    loss_values = [v.mean() for v in dpar(x, kp_joined, generated)]
    sum(loss_values).backward()
    rec["discriminator"] = _grads(discriminator)
    if not detach:
        rec["kp_detector"] = _grads(kp_detector)
    step(od, discriminator)
    if not detach:
        step(ok, kp_detector)
    rec["losses"] = losses + [float(v.detach().cpu()) for v in loss_values]
    be.sync()
    return rec


def _state(nets, opts):
    """parameters, buffers and optimiser states after an iteration (host copies)"""
    return ([{n: t.detach().cpu().clone() for n, t in m.state_dict().items()} for m in nets],
            [copy.deepcopy(o.state_dict()) for o in opts])


def _load_state(nets, opts, state):
    """the reference run continues from the runner run's state: the gradients of these networks are not continuous in the
    weights at fp32 resolution (nearest-neighbour sampling, LeakyReLU / max kinks) -- two runs whose parameters are 1e-6 apart
    after one step give gradients 1e-3 apart in the next iteration, with or without the runner -- so an iteration is compared
    from identical weights and optimiser state"""
    sds, osds = state
    with torch.no_grad():
        for m, sd in zip(nets, sds):
            for n, t in m.state_dict().items():
                t.copy_(sd[n])
    for o, sd in zip(opts, osds):
        o.load_state_dict(sd)


def _rel(a, b, top):
    return float((a.double() - b.double()).norm()) / (float(b.double().norm()) + 1e-6 * top)


def _check_grads(got, want, tol=1e-4, what=""):
    """every parameter that is not a noise bias (cases.is_noise_bias: analytically zero gradient): a gradient on both sides,
    norm-relative error <= tol per tensor"""
    bad = []
    for net in NETS:
        top = max(float(w.norm()) for n, w in want[net].items() if w is not None and not cases.is_noise_bias(n))
        for n, w in want[net].items():
            if cases.is_noise_bias(n):
                continue
            g = got[net][n]
            assert w is not None, (what, net, n)
            if g is None:
                bad.append((float("inf"), net, n))
                continue
            e = _rel(g, w, top)
            if not e <= tol:
                bad.append((e, net, n))
    assert not bad, "%s: %d gradients off; worst %s" % (what, len(bad), sorted(bad, reverse=True)[:6])


def _check_params(nets1, nets0, opt, lr, before):
    """parameters after ONE step from the same state `before`.  SGD: the update is lr * gradient, so the two runs agree to the
    gradients' tolerance (1e-4 of the update) + fp32 rounding of the two updates (2 x 2^-24 |p|).  Adam (second step): an element
    whose gradient is rounding noise moves by up to |m_hat| / sqrt(v_hat) * lr <= sqrt(10/9) lr either way (betas (0.5, 0.999)),
    hence <= 2.2 lr per element; the mean over a network's elements stays a fraction of lr (the yard-stick of
    test_dropin_replay.py: 0.25 lr)."""
    for net, m1, m0 in zip(NETS, nets1, nets0):
        tot = cnt = 0.0
        for (n, p1), (_, p0) in zip(m1.named_parameters(), m0.named_parameters()):
            if cases.is_noise_bias(n):
                continue
            a, b = p1.detach().cpu().double(), p0.detach().cpu().double()
            if opt == "sgd":
                upd = float((b - before[net][n].double()).norm())
                assert float((a - b).norm()) <= 1e-4 * upd + 2.0 ** -23 * float(b.norm()), (net, n)
            else:
                d = (a - b).abs()
                assert float(d.max()) <= 2.2 * lr, (net, n, float(d.max()) / lr)
                tot, cnt = tot + float(d.sum()), cnt + d.numel()
        if opt != "sgd":
            assert tot / cnt <= 0.25 * lr, (net, tot / cnt / lr)


def _oracle_grads(gold, dtype):
    """oracle/restate.py in `dtype` on the golden's weights and batch: dL_G / d(generator, key-point detector) and
    dL_D / d(discriminator) of train.py:110-131 (detach_kp_discriminator = True)"""
    cfg = gold["cfg"]
    src, drv = _batch(gold)
    src, drv = src.to(dtype), drv.to(dtype)

    def leaves(sd):
        return {n: (t.detach().to(dtype).clone().requires_grad_("running" not in n) if t.is_floating_point() else t.clone())
                for n, t in sd.items()}

    sds = {k: leaves(gold["state"][k]) for k in NETS}
    losses, gen, kp_joined, _, _ = restate.generator_full_forward(sds, cfg, src, drv)
    sum(v.mean() for v in losses).backward()
    out = {m: {n: t.grad for n, t in sds[m].items() if t.grad is not None} for m in ("generator", "kp_detector")}
    sds_d = dict(sds, discriminator=leaves(gold["state"]["discriminator"]))
    d_losses = restate.discriminator_full_forward(sds_d, cfg, drv, kp_joined, gen)
    sum(v.mean() for v in d_losses).backward()
    out["discriminator"] = {n: t.grad for n, t in sds_d["discriminator"].items() if t.grad is not None}
    return out


# ---- A: the served path against the fp64 oracle ---------------------------------------------------------------------------------
def test_served_iteration_gradients_equal_the_fp64_oracle(be):
    """Tolerance per tensor (tests/test_fullsize_oracle.py::check_records): 8 x max(the oracle's own fp32-vs-fp64 relative
    distance of that tensor, the network's median of it) + 2e-4."""
    from mnk import dropin
    gold = load("step_tiny")
    tp, nets, opts, pars = _setup(be, gold)
    rec = _iteration(be, tp, nets, opts, pars)
    runner = dropin.runner_for(pars[0].module)
    st = runner.stats
    assert st["fallbacks"] == 0 and st["d_fallbacks"] == 0, st
    assert (st["graph_calls"] if be.kind == "hip" else st["phase_calls"]) == 1, st
    g64, g32 = _oracle_grads(gold, torch.float64), _oracle_grads(gold, torch.float32)
    bad, checked = [], 0
    for net in NETS:
        names = [n for n, _ in dict(nets[NETS.index(net)].named_parameters()).items() if not cases.is_noise_bias(n)]
        top = max(float(g64[net][n].norm()) for n in names)
        spread = {n: _rel(g32[net][n], g64[net][n], top) for n in names}
        med = sorted(spread.values())[len(spread) // 2]
        for n in names:
            got = rec[net][n]
            assert got is not None, (net, n)          # every parameter that is not a noise bias has a gradient
            e, tol = _rel(got, g64[net][n], top), 8.0 * max(spread[n], med) + 2e-4
            checked += 1
            if not e <= tol:
                bad.append((e / tol, net, n, e, tol))
    assert checked > 60                 # (88 on this configuration)
    assert not bad, "%d gradients off the fp64 oracle; worst %s" % (len(bad), sorted(bad, reverse=True)[:6])


# ---- B: every fall-back, then backward and step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "sgd", "clip"])
@pytest.mark.parametrize("trigger", ["stale_grad", "clone", "d_weight", "zero_grad_keep"])
def test_fallback_backward_and_step_equal_the_modules_run_as_they_are(be, monkeypatch, trigger, opt):
    """one served iteration, then an iteration with the trigger (zero_grad_keep: every zero_grad(set_to_none=False), so the
    second iteration finds zeroed, not cleared, gradients); the same statements with MNK_DROPIN_GRAPH=0 as the reference"""
    from mnk import dropin
    gold = load("step_tiny")
    lr = gold["cfg"]["train_params"]["lr"]
    clip = 1e-3 if opt == "clip" else None        # (below every network's gradient norm: the clip scales)
    keep = trigger != "zero_grad_keep"

    state = {}

    def run():
        tp, nets, opts, pars = _setup(be, gold, "sgd" if opt == "sgd" else "adam")
        r0 = _iteration(be, tp, nets, opts, pars, clip=clip, set_to_none=keep)
        if "after0" in state:
            _load_state(nets, opts, state["after0"])
        else:
            state["after0"] = _state(nets, opts)
        runner = dropin.runner_for(pars[0].module)
        stats0 = dict(runner.stats) if runner else None
        r1 = _iteration(be, tp, nets, opts, pars, trigger=None if trigger == "zero_grad_keep" else trigger, clip=clip,
                        set_to_none=keep)
        return (r0, r1), nets, stats0, (dict(runner.stats) if runner else None)

    got, nets1, s0, s1 = run()
    monkeypatch.setenv("MNK_DROPIN_GRAPH", "0")
    want, nets0, _, none = run()
    assert none is None
    assert s0["fallbacks"] == 0 and s0["d_fallbacks"] == 0, s0           # the first iteration was served
    assert (s0["graph_calls"] if be.kind == "hip" else s0["phase_calls"]) == 1, s0
    if trigger in ("stale_grad", "zero_grad_keep"):                     # the generator call fell back (and so the D call)
        assert s1["fallbacks"] == 1 and s1["d_fallbacks"] == 1, s1
    else:                                                                # the generator call was served, the D call fell back
        assert s1["fallbacks"] == 0 and s1["d_fallbacks"] == 1, s1
    for it in range(2):
        _check_grads(got[it], want[it], what="iteration %d (%s, %s)" % (it, trigger, opt))
        for a, b in zip(got[it]["losses"], want[it]["losses"]):
            assert abs(a - b) <= 2e-4 * max(1.0, abs(b)), (it, got[it]["losses"], want[it]["losses"])
        for a, b in zip(got[it]["norms"], want[it]["norms"]):
            assert abs(a - b) <= 1e-4 * b, (it, got[it]["norms"], want[it]["norms"])
    before = dict(zip(NETS, (dict(p) for p in state["after0"][0])))
    _check_params(nets1, nets0, opt, lr, before)


# ---- C: detach_kp_discriminator = False -----------------------------------------------------------------------------------------
def test_detach_kp_discriminator_false_is_not_served_and_keeps_every_gradient(be, monkeypatch):
    """The discriminator loss reaches the key-point detector through the graph the generator pass retained (train.py:117,131-135):
    two iterations, the gradients and the parameters after the steps equal MNK_DROPIN_GRAPH=0"""
    from mnk import dropin, ops
    gold = load("step_tiny")

    state = {}

    def run():
        tp, nets, opts, pars = _setup(be, gold, detach_kp_discriminator=False)
        recs = [_iteration(be, tp, nets, opts, pars)]
        if "after0" in state:
            _load_state(nets, opts, state["after0"])
        else:
            state["after0"] = _state(nets, opts)
        recs.append(_iteration(be, tp, nets, opts, pars))
        return recs, nets, dropin.runner_for(pars[0].module)

    got, nets1, runner = run()
    monkeypatch.setenv("MNK_DROPIN_GRAPH", "0")
    want, nets0, _ = run()
    assert runner.stats["fallbacks"] == 2 and runner.stats["d_fallbacks"] == 2, runner.stats
    assert runner.owners is None and all(ops.sink_owner(p) is None for m in nets1 for p in m.parameters())
    for it in range(2):
        _check_grads(got[it], want[it], what="iteration %d" % it)
    before = dict(zip(NETS, (dict(p) for p in state["after0"][0])))
    _check_params(nets1, nets0, "adam", gold["cfg"]["train_params"]["lr"], before)


# ---- D: storage swaps that keep _version (graphs: MI355X) ---------------------------------------------------------------------
@pytest.mark.gpu
def test_eval_runner_follows_a_storage_swap(monkeypatch):
    """`p.data = p.data * 1.01` on a 3x3 convolution weight and on a bias: the frozen-weight graph must not go on reading the
    old storage.  The old tensors stay referenced for the whole test: a stale graph reads valid memory and fails on values."""
    from conftest import Backend
    from mnk import dropin
    from sync_batchnorm import DataParallelWithCallback
    be = Backend("hip")
    gold = load("step_tiny")
    _, nets, _, _ = _setup(be, gold)
    gen, _, kpd = nets
    gen.eval(), kpd.eval()
    generator = DataParallelWithCallback(gen)
    generator.eval()
    src, drv = (be.t(t) for t in _batch(gold))
    with torch.no_grad():
        kp_s, kp_d = kpd(src), kpd(drv)

    def call():
        with torch.no_grad():
            out = generator(source_image=src, kp_driving=kp_d, kp_source=kp_s)["video_prediction"].clone()
        be.sync()
        return out

    first = call()
    runner = dropin.eval_runner_for_wrapper(generator)
    assert runner is not None and runner.stats["captures"] == 1
    old = []
    params = dict(gen.named_parameters())
    for n in ("video_decoder.up_blocks.0.conv.weight", "refinement_module.conv-last.bias"):
        old.append(params[n].data)
        params[n].data = params[n].data * 1.01
    got = call()
    assert runner.stats["captures"] == 2, runner.stats
    monkeypatch.setenv("MNK_EVAL_GRAPH", "0")
    want = call()
    assert torch.equal(got, want) and not torch.equal(got, first)
    assert all(t.is_cuda for t in old)


@pytest.mark.gpu
def test_train_pair_runner_follows_a_storage_swap(monkeypatch):
    """a served iteration, then `p.data = p.data * 1.01` on a generator convolution weight and a norm-layer bias, then the next
    iteration: re-captured, and its gradients equal MNK_DROPIN_GRAPH=0 with the same swap (old tensors kept alive)"""
    from conftest import Backend
    from mnk import dropin
    be = Backend("hip")
    gold = load("step_tiny")
    old, state = [], {}

    def run():
        tp, nets, opts, pars = _setup(be, gold)
        r0 = _iteration(be, tp, nets, opts, pars)
        if "after0" in state:
            _load_state(nets, opts, state["after0"])
        else:
            state["after0"] = _state(nets, opts)
        params = dict(nets[0].named_parameters())
        for n in ("video_decoder.up_blocks.1.conv.weight", "video_decoder.up_blocks.1.norm.bias"):
            old.append(params[n].data)
            params[n].data = params[n].data * 1.01
        r1 = _iteration(be, tp, nets, opts, pars)
        return (r0, r1), dropin.runner_for(pars[0].module)

    got, runner = run()
    monkeypatch.setenv("MNK_DROPIN_GRAPH", "0")
    want, _ = run()
    st = runner.stats
    assert st["graph_calls"] == 2 and st["captures"] == 2 and st["fallbacks"] == 0 and st["d_fallbacks"] == 0, st
    for it in range(2):
        _check_grads(got[it], want[it], what="iteration %d" % it)
        for a, b in zip(got[it]["losses"], want[it]["losses"]):
            assert abs(a - b) <= 2e-4 * max(1.0, abs(b)), (it, got[it]["losses"], want[it]["losses"])
    assert len(old) == 4


# ---- E: a failure in the warm-up before the capture (MI355X) ------------------------------------------------------------------
@pytest.mark.gpu
def test_a_warm_up_failure_falls_back_and_leaves_nothing_behind(monkeypatch):
    """The runner's phase C raises on its first call -- in the warm-up on the side stream, before any capture_begin (it never
    raises while a capture is under way: a broken capture cannot be destroyed safely).  The call is served by the modules as
    they are: BatchNorm running statistics as after one forward of the modules, no p.grad left before the loop's own backward,
    gradients equal to MNK_DROPIN_GRAPH=0; the next iteration captures and replays."""
    from conftest import Backend
    from mnk import dropin
    be = Backend("hip")
    gold = load("step_tiny")
    seen = {}

    def probe_into(tag):
        def probe(nets):
            seen[tag] = {"buffers": [b.detach().cpu().clone() for m in nets for b in m.buffers()],
                         "grads": [n for m in nets for n, p in m.named_parameters() if p.grad is not None]}
        return probe

    tp, nets, opts, pars = _setup(be, gold)
    runner = dropin.runner_for(pars[0].module)
    real, calls = runner._phase_c, {"n": 0, "raised_while_capturing": False}

    def failing(st, grads):
        calls["n"] += 1
        if calls["n"] == 1:
            if torch.cuda.is_current_stream_capturing():
                calls["raised_while_capturing"] = True          # (never raise here: reported below)
            else:
                raise RuntimeError("injected warm-up failure")
        return real(st, grads)

    monkeypatch.setattr(runner, "_phase_c", failing)
    with pytest.warns(UserWarning, match="warm-up"):
        r0 = _iteration(be, tp, nets, opts, pars, probe=probe_into("got"))
    assert not calls["raised_while_capturing"]
    assert runner.stats["fallbacks"] == 1 and runner.stats["captures"] == 0 and runner.stats["graph_calls"] == 0, runner.stats
    after0 = _state(nets, opts)
    r1 = _iteration(be, tp, nets, opts, pars)
    assert runner.stats["captures"] == 1 and runner.stats["graph_calls"] == 1 and runner.stats["fallbacks"] == 1, runner.stats
    monkeypatch.setenv("MNK_DROPIN_GRAPH", "0")
    tp, nets, opts, pars = _setup(be, gold)
    want = [_iteration(be, tp, nets, opts, pars, probe=probe_into("want"))]
    _load_state(nets, opts, after0)
    want.append(_iteration(be, tp, nets, opts, pars))
    assert seen["got"]["grads"] == [] and seen["want"]["grads"] == []
    for a, b in zip(seen["got"]["buffers"], seen["want"]["buffers"]):
        assert torch.allclose(a.double(), b.double(), rtol=1e-6, atol=1e-7), (a, b)
    for it, (g, w) in enumerate(zip((r0, r1), want)):
        _check_grads(g, w, what="iteration %d" % it)
