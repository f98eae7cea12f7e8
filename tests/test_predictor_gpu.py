"""The prediction task on the MI355X at the shape every shipped configuration uses (rnn_params num_features 1024, num_kp 10 with
'matrix' variance: 60 input features; batch 256, 32 frames): forward and every gradient, prediction.py's batch-1 roll-out, ten
iterations of its training loop with stock Adam, and the batched KPDetector call the roll-out starts from.  References are
float64 restatements in this file and in tests/test_predictor.py."""
import pytest
import torch

from test_predictor import _build, _module_case, make_kp, predictor64

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(make_backend):
    return make_backend("hip")


def test_full_size_forward_and_gradients(hip):
    """B = 256, T = 32, I = 60, H = 1024 (prediction.py:97-107's shape): output, h_n and the gradients of W_ih, W_hh, both
    biases, the linear layer, the key-point inputs and h0 against float64 autograd, within a small factor of the float32
    nn.GRU's own error"""
    torch.set_num_threads(16)
    _module_case(hip, 256, 32, 10, True, 1024, with_h0=True, seed=1)


def test_batch1_rollout(hip):
    """prediction.py:116-132: kp_init of a 32-frame video with the frames after init_frames zeroed, the predictor under no_grad in
    evaluation mode (the GEMV form of the step), the first frames restored and `var` replaced by the last initial frame's"""
    init_frames = 1
    mod = _build(10, True, 1024, seed=4).eval()
    params64 = {k: v.detach().double() for k, v in mod.named_parameters()}
    kp_init = make_kp(1, 32, 10, True, 6)
    for k in kp_init:
        kp_init[k][:, init_frames:] = 0
    mod.to(hip.device)
    with torch.no_grad():
        kp_dev = {k: v.to(hip.device) for k, v in kp_init.items()}
        kp_video = mod(kp_dev)
        for k in kp_video:
            kp_video[k][:, :init_frames] = kp_dev[k][:, :init_frames]
        kp_video['var'] = kp_dev['var'][:, (init_frames - 1):init_frames].repeat(1, kp_video['var'].shape[1], 1, 1, 1)
    torch.cuda.synchronize()
    ref, _ = predictor64(params64, {k: v.double() for k, v in kp_init.items()}, 1)
    ref["mean"][:, :init_frames] = kp_init["mean"][:, :init_frames].double()
    assert kp_video["mean"].shape == (1, 32, 10, 2) and kp_video["var"].shape == (1, 32, 10, 2, 2)
    assert (kp_video["mean"].cpu().double() - ref["mean"]).abs().max() < 2e-5
    assert torch.equal(kp_video["var"][:, 5].cpu(), kp_init["var"][:, 0])


def test_ten_training_iterations_with_adam(hip):
    """ten iterations of prediction.py:97-107's loop body (mask the frames after init_frames, forward, L1 on both keys, backward,
    torch.optim.Adam(lr=1e-3) step): the native module on the GPU and the float64 restatement on the CPU agree on the loss history
    and on the parameters' movement"""
    torch.set_num_threads(16)
    B, T, H, num_kp, init_frames = 32, 32, 256, 10, 1
    mod = _build(num_kp, True, H, seed=7)
    start = {k: v.detach().clone() for k, v in mod.named_parameters()}
    p64 = {k: v.detach().double().requires_grad_() for k, v in mod.named_parameters()}
    mod.to(hip.device)
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3)
    opt64 = torch.optim.Adam(list(p64.values()), lr=1e-3)
    losses, losses64 = [], []
    for it in range(10):
        x = make_kp(B, T, num_kp, True, 100 + it)
        gt = {k: v.clone() for k, v in x.items()}
        for k in x:
            x[k][:, init_frames:] = 0
        xd = {k: v.to(hip.device) for k, v in x.items()}
        gtd = {k: v.to(hip.device) for k, v in gt.items()}
        prediction = mod(xd)
        loss = sum([torch.abs(gtd[k][:, init_frames:] - prediction[k][:, init_frames:]).mean() for k in xd])
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))

        pred64, _ = predictor64(p64, {k: v.double() for k, v in x.items()}, 1)
        loss64 = sum([torch.abs(gt[k][:, init_frames:].double() - pred64[k][:, init_frames:]).mean() for k in x])
        loss64.backward()
        opt64.step()
        opt64.zero_grad()
        losses64.append(float(loss64.detach()))
    for a, b in zip(losses, losses64):
        assert abs(a - b) <= 1e-5 * abs(b), (losses, losses64)
    assert losses[-1] < losses[0]
    for k, p in mod.named_parameters():
        moved64 = p64[k].detach() - start[k].double()
        moved = p.detach().cpu().double() - start[k].double()
        assert float((moved - moved64).norm()) <= 1e-2 * float(moved64.norm()), k


def test_kp_detector_on_32_frames_at_once_equals_the_frame_loop(hip):
    """prediction.py:120 runs the detector on the whole 32-frame clip in one call (the training-set loop of prediction.py:66-71
    one frame at a time); behind DataParallelWithCallback in evaluation mode under no_grad both give the same key points"""
    from oracle import cases
    from modules.keypoint_detector import KPDetector
    from sync_batchnorm import DataParallelWithCallback
    mp = cases.TINY["model_params"]
    torch.manual_seed(0)
    kpd = KPDetector(**mp["kp_detector_params"], **mp["common_params"])
    sd = kpd.state_dict()
    cases.perturb_state_dict(sd, 3)
    kpd.load_state_dict(sd)
    kp_detector = DataParallelWithCallback(kpd.to(hip.device))
    kp_detector.eval()
    g = torch.Generator().manual_seed(2)
    video = torch.rand(1, 3, 32, 32, 32, generator=g).to(hip.device)
    with torch.no_grad():
        whole = {k: v.clone() for k, v in kp_detector(video).items()}
        frames = [{k: v.clone() for k, v in kp_detector(video[:, :, i:i + 1]).items()} for i in range(32)]
    torch.cuda.synchronize()
    for k in whole:
        loop = torch.cat([f[k] for f in frames], dim=1)
        assert whole[k].shape == loop.shape
        assert (whole[k] - loop).abs().max() <= 1e-5 * max(1.0, float(loop.abs().max())), k
