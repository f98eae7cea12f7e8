"""MotionTransferGenerator with d > 1 driving frames per source image (generator.py:51-82): the source is encoded once, the
warps share it among the frames of its video (mnk_warp_levels_shared_* / mnk_deform_shared_*).

e. against the goldens recorded from the unmodified reference at B = 2, d = 3 (tools/make_golden_multiframe.py), with the bounds
   of tests/test_modules.py: outputs in eval and training mode, the gradients of every parameter, of the source image and of
   both key-point dicts, the running statistics after one training forward;
f. against this package's own d = 1 path, frame by frame (forward and deform_input);
g. mnk.engine.Transfer(shared_source=True) against the repeated-source form;
h. the d = 3 training forward + backward gives the same bits twice;
i. (where the reference tree exists) a golden still equals a fresh run of the reference."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import cases, ref_shim
from test_modules import check_grads, load, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = [(name, mode) for name in ("tiny", "tiny2") for mode in ("nearest", "trilinear")]
OUTPUTS = ("video_prediction", "video_deformed")


def _gold(name, mode):
    return torch.load(os.path.join(GOLD, "multiframe_%s_%s.pt" % (name, mode)), weights_only=False)


def _generator(cfg, be):
    """the tool's construction: seed 0, the generator first (run.py:50-62), cases.perturb_state_dict(seed 7)"""
    from modules.generator import MotionTransferGenerator
    mp = cfg["model_params"]
    torch.manual_seed(0)
    gen = MotionTransferGenerator(**mp["generator_params"], **mp["common_params"])
    sd = gen.state_dict()
    cases.perturb_state_dict(sd, 7)
    gen.load_state_dict(sd)
    return gen.to(be.device)


def _inputs(gold, be, grad):
    k = gold["cfg"]["model_params"]["common_params"]["num_kp"]
    b, d, size = gold["batch"], gold["frames"], gold["size"]
    leaf = lambda t: be.t(t).requires_grad_(grad)
    src = leaf(cases.smooth_pair(b, size, size)[0])
    kp_d = {key: leaf(v) for key, v in cases.random_kp(b, d, k, seed=1).items()}
    kp_s = {key: leaf(v) for key, v in cases.random_kp(b, 1, k, seed=2).items()}
    return src, kp_d, kp_s


def _check_outputs(out, gold, mode, factor, floor):
    """tests/test_modules.py::check_outputs for the two outputs a generator-only golden has"""
    for k in OUTPUTS:
        assert out[k].shape == gold[mode + "64"][k].shape == (gold["batch"], 3, gold["frames"], gold["size"], gold["size"])
        ref64, spread = gold[mode + "64"][k].double(), gold[mode + "_spread"][k]
        err = float((out[k].double() - ref64).abs().max())
        print("%s.%s: |hip - ref64| = %.3e, reference's own fp32 noise %.3e" % (mode, k, err, spread))
        assert err <= factor * spread + floor, "%s.%s: |hip - ref64| = %.3e, reference's own fp32 noise %.3e" % (
            mode, k, err, spread)
    l1 = float((out["video_prediction"].double() - gold[mode + "64"]["video_prediction"].double()).abs().mean())
    assert l1 < 1e-4


def _train_run(be, gold):
    gen = _generator(gold["cfg"], be).train()
    src, kp_d, kp_s = _inputs(gold, be, True)
    res = gen(src, kp_driving=kp_d, kp_source=kp_s)
    r1, r2 = gold["loss_weights"]
    ((res["video_prediction"] * be.t(r1)).sum() + (res["video_deformed"] * be.t(r2)).sum()).backward()
    be.sync()
    grads = {"generator": {k: p.grad.cpu() for k, p in gen.named_parameters() if p.grad is not None}, "kp_detector": {},
             "inputs": {"source_image": src.grad.cpu()}}
    for tag, kp in (("kp_driving", kp_d), ("kp_source", kp_s)):
        for k, v in kp.items():
            if v.grad is not None:
                grads["inputs"]["%s.%s" % (tag, k)] = v.grad.cpu()
    return {k: res[k].detach().cpu() for k in OUTPUTS}, grads, gen


@pytest.mark.parametrize("name,mode", CASES)
def test_three_driving_frames_eval_against_the_reference(be, name, mode):
    gold = _gold(name, mode)
    gen = _generator(gold["cfg"], be).eval()
    src, kp_d, kp_s = _inputs(gold, be, False)
    with torch.no_grad():
        res = gen(src, kp_driving=kp_d, kp_source=kp_s)
    be.sync()
    _check_outputs({k: res[k].cpu() for k in OUTPUTS}, gold, "eval", factor=8.0, floor=5e-6)


@pytest.mark.parametrize("name,mode", CASES)
def test_three_driving_frames_train_against_the_reference(be, name, mode):
    """training mode: the encoder's BatchNorm layers see B rows, the decoder's B*d (the reference's BatchNorm3d over
    (B, C, d, H, W)); every gradient sums over the d frames where a tensor is shared by them (source image, kp_source, the
    encoder's parameters)."""
    gold = _gold(name, mode)
    out, grads, gen = _train_run(be, gold)
    _check_outputs(out, gold, "train", factor=4.0, floor=2e-6)
    assert all(cases.is_noise_bias(k) for k in set(grads["generator"]) ^ set(gold["grad64"]["generator"]))
    worst = check_grads(grads, gold)                                 # the parameters: factor 6, floor 1e-4
    print("parameters: worst ratio %.3f (%s)" % (worst[0][0], worst[0][2]))
    assert set(gold["grad64"]["inputs"]) <= set(grads["inputs"])
    for k in set(grads["inputs"]) - set(gold["grad64"]["inputs"]):  # ('gaussian' heat maps never read kp_source's variance: the
        assert torch.all(grads["inputs"][k] == 0), k                 # reference leaves its gradient unset, here it is zeros)
    for k, g64 in gold["grad64"]["inputs"].items():                  # the inputs, by the same criterion
        spread = gold["grad_ref32_vs_ref64_rel"]["inputs"][k]
        assert grads["inputs"][k].shape == g64.shape, k
        err = float((grads["inputs"][k].double() - g64.double()).norm() / (g64.double().norm() + 1e-6))
        print("d %s: rel err %.3e, the reference's own fp32 noise %.3e" % (k, err, spread))
        assert err <= 6.0 * spread + 1e-4, "gradient of %s: rel err %.3e vs the reference's own fp32 noise %.3e" % (k, err, spread)
    sd = gen.state_dict()
    for k, v in gold["running_after_train"]["generator"].items():
        assert float((sd[k].cpu() - v).abs().max()) < 1e-4 * (1 + float(v.abs().max())), k


@pytest.mark.parametrize("name,mode", CASES)
def test_three_driving_frames_equal_three_calls_with_one(be, name, mode):
    """eval mode (running statistics: frames are independent): one d = 3 call against three d = 1 calls, and deform_input"""
    gold = _gold(name, mode)
    gen = _generator(gold["cfg"], be).eval()
    src, kp_d, kp_s = _inputs(gold, be, False)
    d = gold["frames"]
    with torch.no_grad():
        one = gen(src, kp_driving=kp_d, kp_source=kp_s)
        loop = [gen(src, kp_driving={k: v[:, i:i + 1] for k, v in kp_d.items()}, kp_source=kp_s) for i in range(d)]
        field = gen.dense_motion_module(src, kp_d, kp_s)                       # (B, d, h, w, 3)
        skip = be.t(torch.rand(gold["batch"], 5, 1, 8, 8, generator=torch.Generator().manual_seed(4)))
        warped = gen.deform_input(skip, field)
        warped_loop = torch.cat([gen.deform_input(skip, field[:, i:i + 1].contiguous()) for i in range(d)], dim=2)
    be.sync()
    for k in OUTPUTS:
        want = torch.cat([o[k] for o in loop], dim=2)
        assert one[k].shape == want.shape
        err = float((one[k] - want).abs().max())
        print("%s: max |d = 3 call - frame loop| = %.3e" % (k, err))
        assert err < 2e-6, k
    assert warped.shape == warped_loop.shape == (gold["batch"], 5, d, 8, 8)
    assert float((warped - warped_loop).abs().max()) < 2e-6


def test_a_source_with_several_frames_still_raises(be):
    gold = _gold("tiny", "nearest")
    gen = _generator(gold["cfg"], be).eval()
    src, kp_d, kp_s = _inputs(gold, be, False)
    two = torch.cat([src, src], dim=2)
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            gen(two, kp_driving=kp_d, kp_source=kp_s)
        with pytest.raises(NotImplementedError):
            gen.deform_input(two, gen.dense_motion_module(src, kp_d, kp_s))


def test_transfer_with_a_shared_source_equals_the_repeated_source(be):
    """the inputs of test_batched_transfer_equals_the_frame_loop_and_normalize_kp_its_formulas"""
    from mnk import engine
    gold = load("tiny")
    gen, _, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    gen.to(be.device).eval(), kpd.to(be.device).eval()
    src, _ = cases.smooth_pair(2, gold["size"], gold["size"], seed=11)
    driving = torch.cat([cases.smooth_pair(2, gold["size"], gold["size"], seed=20 + i)[1] for i in range(3)], dim=2)
    src, driving = be.t(src), be.t(driving)
    params = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)
    rep = engine.Transfer(kpd, gen, params)(src, driving)
    shared = engine.Transfer(kpd, gen, params, shared_source=True)(src, driving)
    be.sync()
    assert set(rep) == set(shared)
    for k in OUTPUTS:
        assert shared[k].shape == rep[k].shape == (2, 3, 3, gold["size"], gold["size"])
        err = float((shared[k] - rep[k]).abs().max())
        print("%s: max |shared - repeated| = %.3e" % (k, err))
        assert err < 2e-6, k
    for k in ("kp_driving", "kp_source", "kp_norm"):
        assert set(shared[k]) == set(rep[k])
        for kk in rep[k]:
            assert torch.equal(shared[k][kk], rep[k][kk]), (k, kk)


def test_three_driving_frames_training_step_is_deterministic(be):
    gold = _gold("tiny", "nearest")
    a = _train_run(be, gold)
    b = _train_run(be, gold)
    bits = lambda t: t.contiguous().view(torch.int32)
    for k in OUTPUTS:
        assert torch.equal(bits(a[0][k]), bits(b[0][k])), k
    for m in ("generator", "inputs"):
        assert set(a[1][m]) == set(b[1][m])
        for k in a[1][m]:
            assert torch.equal(bits(a[1][m][k]), bits(b[1][m][k])), (m, k)


@pytest.mark.skipif(not ref_shim.available(), reason="the reference tree only exists where the goldens are made")
def test_live_reference_agrees_with_the_multiframe_golden():
    """one case re-run on the real reference (a process of its own: the reference's `modules` package shadows this one's)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_multiframe.py"), "--check", "tiny_trilinear"],
                         capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
