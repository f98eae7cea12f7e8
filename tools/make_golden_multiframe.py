#!/usr/bin/env python
"""Records tests/golden/multiframe_<config>_<mode>.pt: the UNMODIFIED reference generator (imported through oracle.ref_shim;
works only where the reference tree exists) called with d = 3 driving frames per source image (generator.py:51-82), for
tests/test_multiframe_generator.py.

    python tools/make_golden_multiframe.py            # writes the four fixtures
    python tools/make_golden_multiframe.py --check    # re-runs the reference and compares with the committed fixtures
    python tools/make_golden_multiframe.py --check tiny_trilinear     # ... one case only

Cases: oracle.cases.TINY and TINY2, interpolation_mode 'nearest' and 'trilinear', B = 2, d = 3, 32 x 32; the source is
cases.smooth_pair's first image, the key points cases.random_kp (seed 1: driving, (B, 3); seed 2: source, (B, 1)), the weights
are the seed-0 initialisation with cases.perturb_state_dict(seed 7) -- nothing of that is stored, the tests rebuild it.

One file per case (a file holds tensors and settings only and stays under 1 MiB), in the key layout that
tests/test_modules.py::check_outputs / check_grads read from the compact goldens:
  cfg, batch, frames, size, interpolation_mode, loss_weights (r1, r2)
  eval64 / train64            fp64 outputs rounded to fp32: video_prediction, video_deformed  (B, C, d, H, W)
  eval_spread / train_spread  max |reference fp32 - reference fp64| per output
  grad64                      {"generator": parameters, "kp_detector": {}, "inputs": source_image, kp_driving.mean / .var,
                              kp_source.mean / .var}: fp64 gradients of sum(prediction * r1) + sum(deformed * r2) in training
                              mode, rounded to fp32
  grad_ref32_vs_ref64_rel     the reference's own fp32-versus-fp64 relative error per gradient
  running_after_train         the generator's running statistics after ONE fp32 training forward"""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLD = os.path.join(ROOT, "tests", "golden")
BATCH, FRAMES, SIZE = 2, 3, 32
CASES = [(name, mode) for name in ("tiny", "tiny2") for mode in ("nearest", "trilinear")]
OUTPUTS = ("video_prediction", "video_deformed")


def path_of(name, mode):
    return os.path.join(GOLD, "multiframe_%s_%s.pt" % (name, mode))


def case_config(name, mode):
    from oracle import cases
    cfg = copy.deepcopy({"tiny": cases.TINY, "tiny2": cases.TINY2}[name])
    cfg["model_params"]["generator_params"]["interpolation_mode"] = mode
    return cfg


def case_inputs(cfg):
    """source (B, C, 1, H, W), kp_driving (B, d, K, .), kp_source (B, 1, K, .), loss weights r1, r2 (B, C, d, H, W)"""
    from oracle import cases
    common = cfg["model_params"]["common_params"]
    src, _ = cases.smooth_pair(BATCH, SIZE, SIZE)
    kp_d = cases.random_kp(BATCH, FRAMES, common["num_kp"], seed=1)
    kp_s = cases.random_kp(BATCH, 1, common["num_kp"], seed=2)
    g = torch.Generator().manual_seed(99)
    r1 = torch.randn(BATCH, common["num_channels"], FRAMES, SIZE, SIZE, generator=g)
    r2 = torch.randn(BATCH, common["num_channels"], FRAMES, SIZE, SIZE, generator=g)
    return src, kp_d, kp_s, (r1, r2)


def build_generator(cls, cfg):
    """the generator is the first module run.py:50-62 constructs: seed 0, then the shared perturbation with seed 7"""
    from oracle import cases
    mp = cfg["model_params"]
    torch.manual_seed(0)
    gen = cls(**mp["generator_params"], **mp["common_params"])
    sd = gen.state_dict()
    cases.perturb_state_dict(sd, 7)
    gen.load_state_dict(sd)
    return gen


def relerr(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-6))


def run(gen, state, inputs, dtype, train):
    src, kp_d, kp_s, (r1, r2) = inputs
    gen.load_state_dict(state)
    gen.to(dtype).train(train)
    gen.zero_grad()
    leaf = lambda t: t.to(dtype).clone().requires_grad_(train)
    src, kp_d, kp_s = leaf(src), {k: leaf(v) for k, v in kp_d.items()}, {k: leaf(v) for k, v in kp_s.items()}
    with torch.enable_grad() if train else torch.no_grad():
        res = gen(src, kp_driving=kp_d, kp_source=kp_s)
    out = {k: res[k].detach() for k in OUTPUTS}
    grads = None
    if train:
        ((res["video_prediction"] * r1.to(dtype)).sum() + (res["video_deformed"] * r2.to(dtype)).sum()).backward()
        grads = {"generator": {k: p.grad.clone() for k, p in gen.named_parameters() if p.grad is not None}, "kp_detector": {},
                 "inputs": {"source_image": src.grad.clone()}}
        for tag, kp in (("kp_driving", kp_d), ("kp_source", kp_s)):
            for k, v in kp.items():
                if v.grad is not None:            # ('gaussian' heat maps never read kp_source's variance)
                    grads["inputs"]["%s.%s" % (tag, k)] = v.grad.clone()
    running = {k: v.detach().clone().float() for k, v in gen.state_dict().items() if "running" in k}
    gen.float()
    return out, grads, running


def record(ref, name, mode):
    from oracle import cases
    cfg = case_config(name, mode)
    inputs = case_inputs(cfg)
    gen = build_generator(ref.MotionTransferGenerator, cfg)
    state = copy.deepcopy(gen.state_dict())
    rec = {"cfg": cfg, "batch": BATCH, "frames": FRAMES, "size": SIZE, "interpolation_mode": mode, "loss_weights": inputs[3]}
    for tag, train in (("train", True), ("eval", False)):
        o32, g32, running = run(gen, state, inputs, torch.float32, train)
        o64, g64, _ = run(gen, state, inputs, torch.float64, train)
        rec[tag + "64"] = {k: v.float() for k, v in o64.items()}
        rec[tag + "_spread"] = {k: float((o32[k].double() - o64[k]).abs().max()) for k in OUTPUTS}
        if train:
            rec["running_after_train"] = {"generator": running, "kp_detector": {}}
            rec["grad64"] = {m: {k: v.float() for k, v in d.items()} for m, d in g64.items()}
            rec["grad_ref32_vs_ref64_rel"] = {m: {k: relerr(g32[m][k], v) for k, v in d.items() if not cases.is_noise_bias(k)}
                                              for m, d in g64.items()}
    return rec


def compare(rec, gold):
    """a fresh reference run against a stored fixture: fp64 results rounded to fp32, so equal up to the last bit of that"""
    worst = 0.0
    for tag in ("train64", "eval64"):
        for k in OUTPUTS:
            worst = max(worst, float((rec[tag][k].double() - gold[tag][k].double()).abs().max()))
    for m, d in gold["grad64"].items():
        assert set(d) == set(rec["grad64"][m]), m
        for k, v in d.items():
            worst = max(worst, relerr(rec["grad64"][m][k], v))
    for k, v in gold["running_after_train"]["generator"].items():
        worst = max(worst, float((rec["running_after_train"]["generator"][k] - v).abs().max()))
    return worst


def main():
    from oracle import ref_shim
    assert ref_shim.available(), "needs the reference tree (oracle.ref_shim.REFERENCE_ROOT)"
    torch.set_num_threads(8)
    ref = ref_shim.load()
    check = "--check" in sys.argv[1:]
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    assert all(a in ["%s_%s" % c for c in CASES] for a in only), only
    for name, mode in CASES:
        if only and "%s_%s" % (name, mode) not in only:
            continue
        rec = record(ref, name, mode)
        path = path_of(name, mode)
        if check:
            worst = compare(rec, torch.load(path, weights_only=False))
            print("%s %s: fresh reference run vs fixture, worst difference %.3e" % (name, mode, worst))
            assert worst < 1e-6, (name, mode, worst)
        else:
            torch.save(rec, path)
            size = os.path.getsize(path)
            print("%s  %d bytes; spreads eval %s train %s" % (path, size, rec["eval_spread"], rec["train_spread"]))
            assert size < (1 << 20), "a committed file stays under 1 MiB"
    print("ok")


if __name__ == "__main__":
    main()
