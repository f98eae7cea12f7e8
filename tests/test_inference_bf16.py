"""Opt-in bf16 inference (mnk.ops.inference_precision, Reconstructor / Transfer(precision="bf16"), MNK_EVAL_PRECISION): the 3x3
convolutions round their operands to bf16 (MNK_CONV_BF16), everything else stays fp32.  The model-level reference is the fp64
restatement of the reference (oracle/restate.py) with the operands of every 3x3 convolution rounded to bf16.

Model-level figures, max |out - eval64| / e_ref (e_ref = the same error of the rounded restatement), bound 2:
  CPU emulator   tiny: prediction 0.997, deformed 1.002, key points 1.337      tiny2: 0.930, 1.292, 0.812
  MI355X         tiny and tiny2 as on the emulator      bair: 0.769, 0.300, 1.019      (profiles/bf16_inference.txt)"""
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, restate
from test_modules import build, load

OUTPUTS = ("video_prediction", "video_deformed", "kp_driving_mean")


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _rounded_conv(ctx, x, prefix, padding=1, groups=1):
    """restate.conv with both operands of a 3x3 convolution rounded to bf16 (what MNK_CONV_BF16 does in the loaders)"""
    w = ctx.p(prefix + ".weight")[:, :, 0]
    b = ctx.sd.get(prefix + ".bias")
    if tuple(w.shape[-2:]) == (3, 3) and groups == 1:
        x, w = _bf(x), _bf(w)
    return F.conv2d(x, w, b, padding=padding, groups=groups)


def _restated(sds, cfg, src, drv):
    """oracle/make_golden.py's evaluation-mode run of the restatement in fp64: one joint key-point call, one generator call"""
    mp = cfg["model_params"]
    common = mp["common_params"]
    sd64 = restate.to_dtype(sds, torch.float64)
    with torch.no_grad():
        kp = restate.kp_detector_forward(sd64["kp_detector"], dict(mp["kp_detector_params"], **common),
                                         torch.cat([src, drv], dim=2).double(), training=False)
        res = restate.generator_forward(sd64["generator"], mp["generator_params"], common, src.double(),
                                        {k: v[:, 1:] for k, v in kp.items()}, {k: v[:, :1] for k, v in kp.items()}, training=False)
    return {"video_prediction": res["video_prediction"], "video_deformed": res["video_deformed"], "kp_driving_mean": kp["mean"][:, 1:]}


def _gold_outputs(gold):
    ref = gold["eval64"]
    return {"video_prediction": ref["video_prediction"].double(), "video_deformed": ref["video_deformed"].double(),
            "kp_driving_mean": ref["kp_mean"][:, 1:].double()}


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


def _tiny_models(gold, be):
    gen, disc, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    return gen.to(be.device).eval(), kpd.to(be.device).eval()


def _check_model(be, monkeypatch, gold, gen, kpd, sds, pin):
    from mnk import engine
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    want = _gold_outputs(gold)
    plain = _restated(sds, gold["cfg"], src, drv)
    for k in OUTPUTS:
        assert _err(plain[k], want[k]) <= pin, ("the un-patched restatement must reproduce eval64", k, _err(plain[k], want[k]))
    monkeypatch.setattr(restate, "conv", _rounded_conv)
    rounded = _restated(sds, gold["cfg"], src, drv)
    monkeypatch.undo()
    e_ref = {k: _err(rounded[k], want[k]) for k in OUTPUTS}
    out = engine.Reconstructor(kpd, gen, precision="bf16")(be.t(src), be.t(drv))
    out32 = engine.Reconstructor(kpd, gen)(be.t(src), be.t(drv))
    be.sync()
    out = {k: out[k].cpu() for k in OUTPUTS}
    ratios = {k: _err(out[k], want[k]) / e_ref[k] for k in OUTPUTS}
    l1 = float((out["video_prediction"].double() - drv.double()).abs().mean())
    l1_ref = float((want["video_prediction"] - drv.double()).abs().mean())
    print("bf16 inference on %s: e_ref %s   max |out - eval64| / e_ref %s   |L1_bf16 - L1_ref64| %.3g" % (
        be.kind, {k: "%.3g" % v for k, v in e_ref.items()}, {k: "%.3f" % v for k, v in ratios.items()}, abs(l1 - l1_ref)))
    for k in OUTPUTS:
        assert e_ref[k] > 1e-6, "the rounded reference did not round"
        assert ratios[k] <= 2.0, (k, ratios[k], e_ref[k])
    assert abs(l1 - l1_ref) < 1e-4                      # reconstruction L1 criterion (tests/test_inference.py)
    assert not torch.equal(out["video_prediction"], out32["video_prediction"].cpu())


@pytest.mark.parametrize("name", ["tiny", "tiny2"])
def test_bf16_reconstructor_is_within_twice_the_rounded_restatement_error(be, monkeypatch, name):
    """max |out - eval64| <= 2 e_ref per output, e_ref = the error of the fp64 restatement with bf16-rounded 3x3 operands.
    Why 2: perturbing the inputs by 1e-7 or running the rounded restatement in fp32 flips individual bf16 roundings; on the CPU
    that moved single outputs by at most 0.58 e_ref and the maximum by 1.5 % -- a form that rounds twice or truncates has 2 ...
    several e_ref."""
    gold = load(name)
    gen, kpd = _tiny_models(gold, be)
    _check_model(be, monkeypatch, gold, gen, kpd, gold["state"], 1e-12)


@pytest.mark.gpu
def test_bf16_reconstructor_on_bair(monkeypatch):
    """bair.yaml with the construction of tests/test_inference.py::_models; the rounded restatement on that state dict is the
    reference.  (The compact golden keeps eval64 rounded to fp32: the un-patched restatement is pinned to that rounding, 2^-24
    of values in [-1, 1], plus the 1e-7 oracle/make_golden.py holds restatement and reference to.)"""
    from conftest import Backend
    from test_inference import _models
    be = Backend("hip")
    gold = load("bair")
    gen, kpd = _models(gold, be)
    sds = {"generator": {k: v.detach().cpu().clone() for k, v in gen.state_dict().items()},
           "kp_detector": {k: v.detach().cpu().clone() for k, v in kpd.state_dict().items()}}
    _check_model(be, monkeypatch, gold, gen.eval(), kpd.eval(), sds, 2.0 ** -24 + 1e-7)


def test_inference_precision_scope_semantics(be):
    from mnk import engine, ops
    gold = load("tiny")
    gen, kpd = _tiny_models(gold, be)
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    src, drv = be.t(src), be.t(drv)
    rec = engine.Reconstructor(kpd, gen)
    before = {k: v.clone() for k, v in rec(src, drv).items()}
    assert ops.current_precision() == "fp32"
    with ops.inference_precision("bf16"):
        assert ops.current_precision() == "bf16"
        inside = {k: v.clone() for k, v in rec(src, drv).items()}      # (an fp32 Reconstructor is a scope of its own: fp32)
        with torch.no_grad():
            scoped = kpd(drv)["mean"].clone()
        with ops.inference_precision("fp32"):
            assert ops.current_precision() == "fp32"
        assert ops.current_precision() == "bf16"
    assert ops.current_precision() == "fp32"
    with torch.no_grad():
        assert not torch.equal(scoped, kpd(drv)["mean"])
    with pytest.raises(ZeroDivisionError):
        with ops.inference_precision("bf16"):
            1 / 0
    assert ops.current_precision() == "fp32"
    with pytest.raises(ValueError):
        ops.inference_precision("fp16")
    after = rec(src, drv)
    be.sync()
    for k in before:
        assert torch.equal(before[k], inside[k]) and torch.equal(before[k], after[k]), k
    # gradients enabled inside the scope: the backward kernels are fp32 and would not differentiate what was computed
    x = ops.to_act(drv[:, :, :1])
    w = be.t(torch.randn(5, 3, 1, 3, 3) * 0.3).requires_grad_(True)
    with ops.inference_precision("bf16"):
        with pytest.raises(RuntimeError, match="gradients enabled"):
            ops.conv3x3(x, 3, w)
        with pytest.raises(RuntimeError, match="gradients enabled"):
            kpd(drv)
        with torch.no_grad():
            y16, _ = ops.conv3x3(x, 3, w)
    with torch.no_grad():
        y32, _ = ops.conv3x3(x, 3, w)
    y, _ = ops.conv3x3(x, 3, w)                      # outside the scope gradients work as before
    y.sum().backward()
    be.sync()
    assert w.grad is not None and torch.equal(y.detach(), y32) and not torch.equal(y16, y32)


def test_bf16_transfer_equals_the_frame_loop_inside_the_scope(be):
    """Transfer(precision="bf16") == the detector and the generator driven frame by frame inside inference_precision("bf16")"""
    from mnk import engine, ops
    gold = load("tiny")
    gen, kpd = _tiny_models(gold, be)
    src, _ = cases.smooth_pair(2, gold["size"], gold["size"], seed=11)
    driving = torch.cat([cases.smooth_pair(2, gold["size"], gold["size"], seed=20 + i)[1] for i in range(3)], dim=2)
    src, driving = be.t(src), be.t(driving)
    params = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)
    got = engine.Transfer(kpd, gen, params, precision="bf16")(src, driving)
    plain = engine.Transfer(kpd, gen, params)(src, driving)
    with torch.no_grad(), ops.inference_precision("bf16"):
        kp_d = {k: torch.cat([kpd(driving[:, :, i:i + 1])[k] for i in range(3)], dim=1) for k in ("mean", "var")}
        kp_s = kpd(src)
        kp_n = engine.normalize_kp(kp_d, kp_s, **params)
        frames = [gen(src, kp_driving={k: v[:, i:i + 1] for k, v in kp_n.items()}, kp_source=kp_s)["video_prediction"]
                  for i in range(3)]
        loop = torch.cat(frames, dim=2)
    be.sync()
    assert torch.equal(got["kp_driving"]["mean"], kp_d["mean"]) and torch.equal(got["kp_source"]["mean"], kp_s["mean"])
    assert torch.equal(got["video_prediction"], loop)
    assert not torch.equal(got["video_prediction"], plain["video_prediction"])


@pytest.mark.gpu
def test_bf16_hipgraph_replay_equals_eager_bf16():
    from conftest import Backend
    from mnk import engine
    from test_inference import _models
    be = Backend("hip")
    gold = load("bair")
    gen, kpd = _models(gold, be)
    g = torch.Generator().manual_seed(3)
    eager = engine.Reconstructor(kpd, gen, use_graph=False, precision="bf16")
    graphed = engine.Reconstructor(kpd, gen, use_graph=True, precision="bf16")
    plain = engine.Reconstructor(kpd, gen)
    for it in range(2):
        src = torch.rand(16, 3, 1, 64, 64, generator=g).to(be.device)
        drv = torch.rand(16, 3, 1, 64, 64, generator=g).to(be.device)
        a = eager(src, drv)
        b = graphed(src, drv)
        c = plain(src, drv)
        torch.cuda.synchronize()
        assert torch.equal(a["video_prediction"], b["video_prediction"]), it
        assert torch.equal(a["kp_driving_mean"], b["kp_driving_mean"])
        assert not torch.equal(a["video_prediction"], c["video_prediction"])      # the captured graph kept its precision


@pytest.mark.gpu
def test_eval_runner_captures_one_program_per_precision(monkeypatch):
    """the reference's per-frame loop behind DataParallelWithCallback: MNK_EVAL_PRECISION picks the precision the EvalRunner
    captures in; flipping it between calls re-captures (one capture per flip) instead of replaying the other form, and each
    output is bit-equal to eager launches inside the respective scope"""
    from conftest import Backend
    from sync_batchnorm import DataParallelWithCallback
    from mnk import dropin, ops
    from test_inference import _models
    be = Backend("hip")
    gold = load("bair")
    gen, kpd = _models(gold, be)
    gen.eval(), kpd.eval()
    kp_detector = DataParallelWithCallback(kpd)
    kp_detector.eval()
    frame = torch.rand(1, 3, 1, 64, 64, generator=torch.Generator().manual_seed(5)).to(be.device)
    want = {}
    with torch.no_grad():
        for precision in ("fp32", "bf16"):
            with ops.inference_precision(precision):
                want[precision] = kpd(frame)["mean"].clone()
    assert not torch.equal(want["fp32"], want["bf16"])
    with torch.no_grad():
        for precision, captures in (("fp32", 1), ("bf16", 2), ("fp32", 2), ("bf16", 2)):
            monkeypatch.setenv("MNK_EVAL_PRECISION", precision)
            for _ in range(2):                                        # the second call with the same setting replays
                got = kp_detector(frame)["mean"]
                torch.cuda.synchronize()
                runner = dropin.eval_runner_for_wrapper(kp_detector)
                assert runner is not None
                assert torch.equal(got, want[precision]), precision
                # one capture per flip to a precision; flipping back finds that precision's own program under its key
                assert runner.stats["captures"] == captures, (precision, runner.stats)


@pytest.mark.gpu
def test_wrapper_follows_the_enclosing_scope_and_its_eager_fallback_the_variable(monkeypatch):
    """a DataParallelWithCallback wrapper called inside inference_precision("bf16") captures and replays bf16 although
    MNK_EVAL_PRECISION is at its default (the scope has precedence and is part of the program key), and with MNK_EVAL_GRAPH=0
    the eager fall-back runs in the precision the variable names"""
    from conftest import Backend
    from sync_batchnorm import DataParallelWithCallback
    from mnk import dropin, ops
    from test_inference import _models
    be = Backend("hip")
    gold = load("bair")
    gen, kpd = _models(gold, be)
    kpd.eval()
    kp_detector = DataParallelWithCallback(kpd)
    kp_detector.eval()
    frame = torch.rand(1, 3, 1, 64, 64, generator=torch.Generator().manual_seed(6)).to(be.device)
    monkeypatch.delenv("MNK_EVAL_PRECISION", raising=False)
    with torch.no_grad():
        want = {}
        for precision in ("fp32", "bf16"):
            with ops.inference_precision(precision):
                want[precision] = kpd(frame)["mean"].clone()
        assert not torch.equal(want["fp32"], want["bf16"])
        plain = kp_detector(frame)["mean"]
        with ops.inference_precision("bf16"):
            scoped = [kp_detector(frame)["mean"] for _ in range(2)]
        again = kp_detector(frame)["mean"]
        torch.cuda.synchronize()
        runner = dropin.eval_runner_for_wrapper(kp_detector)
        assert runner.stats["captures"] == 2 and runner.stats["replays"] == 4, runner.stats
        assert torch.equal(plain, want["fp32"]) and torch.equal(again, want["fp32"])
        assert torch.equal(scoped[0], want["bf16"]) and torch.equal(scoped[1], want["bf16"])
        monkeypatch.setenv("MNK_EVAL_GRAPH", "0")
        eager = {}
        for precision in ("fp32", "bf16"):
            monkeypatch.setenv("MNK_EVAL_PRECISION", precision)
            eager[precision] = kp_detector(frame)["mean"]
        torch.cuda.synchronize()
        assert runner.stats["replays"] == 4, runner.stats
        assert torch.equal(eager["fp32"], want["fp32"]) and torch.equal(eager["bf16"], want["bf16"])
    assert ops.current_precision() == "fp32"
