"""mnk.engine.Prediction (mnk/prediction.py): extract, fit and predict of the prediction task.

a. fit against tests/golden/prediction_loop.npz (tools/make_golden_prediction.py: the unmodified reference's KPDataset +
   DataLoader batches over three epochs and its float64 PredictionModule run through prediction.py:94-111): the batches bit for
   bit, every iteration's loss and the parameters' movement within the bounds of
   tests/test_predictor_gpu.py::test_ten_training_iterations_with_adam;
b. patience = 0: a lowered learning rate reaches the next iteration (under graph replay too, on the GPU);
c. two runs from the same seeds give the same bits;
d. extract against the per-frame detector loop, predict against predictor64 and the per-frame generator loop;
e. (-m gpu) the full-size iteration: graph replay equals eager bit for bit; ten iterations against float64.
The same bodies run on the CPU emulator and, with -m gpu, on the MI355X."""
import os

import numpy as np
import pytest
import torch
from _guard import be  # noqa: F401  (the backend fixture: emu / hip)

from test_predictor import predictor64, perturbed, make_kp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "prediction_loop.npz")


def modes(be):
    """use_graph values a test walks through: the emulator always runs eager"""
    return [False, True] if be.kind == "hip" else [False]


def rows_of(mean, var):
    n = mean.shape[0]
    return torch.cat([mean.reshape(n, -1), var.reshape(n, -1)], -1)


def gold_pool(gold, device):
    from mnk.engine import KeyPointPool
    rows, index, off = [], [], 0
    for i, f in enumerate(gold["frames"].tolist()):
        rows.append(rows_of(torch.from_numpy(gold["kp_mean_v%d" % i]), torch.from_numpy(gold["kp_var_v%d" % i])))
        index.append((off, f))
        off += f
    return KeyPointPool(torch.cat(rows).to(device).contiguous(), index)


def gold_engine(gold, device, use_graph, patience=50):
    from mnk.engine import Prediction
    params = {"rnn_params": {"num_features": 16}, "predict_variance": False, "num_epochs": int(gold["epochs"]),
              "lr": float(gold["lr"]), "batch_size": int(gold["batch_size"]), "num_frames": int(gold["num_frames"]),
              "init_frames": int(gold["init_frames"]), "train_size": None}
    eng = Prediction(None, None, params, num_kp=int(gold["num_kp"]), kp_variance="matrix", use_graph=use_graph, patience=patience)
    torch.manual_seed(0)
    eng.predictor                               # created here: the seed-0 initialisation the fixture recorded
    return eng


def fit_recorded(eng, pool, epochs):
    """(losses of every iteration, parameters after every epoch, learning rate after every epoch)"""
    losses, params, lrs = [], [], []

    def on_epoch(e, loss):
        losses.extend(eng.iteration_losses().cpu().tolist())
        params.append({k: v.detach().cpu().clone() for k, v in eng.predictor.named_parameters()})
        lrs.append(eng.optimizer.param_groups[0]["lr"])
    np.random.seed(3)
    means = eng.fit(pool, num_epochs=epochs, on_epoch=on_epoch)
    return losses, params, lrs, means


def test_batches_equal_the_reference_dataloader(be):
    """np.random.seed(3): the windows the engine gathers over three epochs are the gt batches the reference's KPDataset + DataLoader
    yield, bit for bit, the short last batch (one video) included"""
    gold = np.load(GOLD)
    eng = gold_engine(gold, be.device, False)
    pool = gold_pool(gold, be.device)
    seen, inner = [], eng._iteration

    def recording(plan, starts):
        inner(plan, starts)
        seen.append((plan.gt.cpu().clone(), plan.x.cpu().clone()))
    eng._iteration = recording
    np.random.seed(3)
    eng.fit(pool)
    assert len(seen) == 6
    init = int(gold["init_frames"])
    for n, (gt, x) in enumerate(seen):
        e, j = divmod(n, 2)
        mean, var = (torch.from_numpy(gold["gt_%s_e%d_b%d" % (k, e, j)]) for k in ("mean", "var"))
        b, t = mean.shape[:2]
        assert b == (3, 1)[j]
        ref = torch.cat([mean.reshape(b, t, -1), var.reshape(b, t, -1)], -1)
        assert torch.equal(gt, ref), (e, j)
        assert torch.equal(x[:, :init], ref[:, :init]) and (x[:, init:] == 0).all()


def test_losses_and_parameters_follow_the_reference_loop(be):
    """every iteration's loss to 1e-5 relative and |moved - moved64| <= 1e-2 |moved64| per parameter against the recorded float64
    run of prediction.py:94-111 (Adam, ReduceLROnPlateau), eager and -- on the GPU -- replayed"""
    gold = np.load(GOLD)
    for graph in modes(be):
        eng = gold_engine(gold, be.device, graph)
        start = {k: v.detach().cpu().clone() for k, v in eng.predictor.named_parameters()}
        for k, v in start.items():
            assert torch.equal(v, torch.from_numpy(gold["before." + k])), k
        losses, params, _, means = fit_recorded(eng, gold_pool(gold, be.device), 3)
        ref = gold["losses"].tolist()
        print(graph, losses, ref)
        assert len(losses) == len(ref) == 6
        for a, b in zip(losses, ref):
            assert abs(a - b) <= 1e-5 * abs(b), (graph, losses, ref)
        for e in range(3):
            assert abs(means[e] - (ref[2 * e] + ref[2 * e + 1]) / 2) <= 1e-5
        for k, p in params[-1].items():
            moved64 = torch.from_numpy(gold["after." + k]) - start[k].double()
            moved = p.double() - start[k].double()
            assert float((moved - moved64).norm()) <= 1e-2 * float(moved64.norm()), (graph, k)


def float64_loop(gold, pool_rows, videos, epochs, patience):
    """prediction.py:94-111 in float64 on the engine's own windows (np.random.seed(3)): parameters and lr after every epoch"""
    T, init, bs = int(gold["num_frames"]), int(gold["init_frames"]), int(gold["batch_size"])
    K = int(gold["num_kp"])
    p64 = {k[len("before."):]: torch.from_numpy(gold[k]).double().requires_grad_() for k in gold.files if k.startswith("before.")}
    opt = torch.optim.Adam(list(p64.values()), lr=float(gold["lr"]))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=patience)
    np.random.seed(3)
    params, lrs = [], []
    for _ in range(epochs):
        starts = [o + int(np.random.choice(max(1, n - T + 1), size=1)[0]) for o, n in videos]
        loss_list = []
        for i in range(0, len(starts), bs):
            rows = torch.stack([pool_rows[s:s + T] for s in starts[i:i + bs]]).double()
            gt = {"mean": rows[..., :2 * K].reshape(-1, T, K, 2), "var": rows[..., 2 * K:].reshape(-1, T, K, 2, 2)}
            x = {k: v.clone() for k, v in gt.items()}
            for k in x:
                x[k][:, init:] = 0
            out, _ = predictor64(p64, x, 1)
            loss = sum([torch.abs(gt[k][:, init:] - out[k][:, init:]).mean() for k in x])
            loss.backward()
            opt.step()
            opt.zero_grad()
            loss_list.append(float(loss.detach()))
        sched.step(np.mean(loss_list))
        params.append({k: v.detach().clone() for k, v in p64.items()})
        lrs.append(opt.param_groups[0]["lr"])
    return params, lrs


def test_a_lowered_learning_rate_reaches_the_next_iteration(be):
    """patience = 0: the third epoch's mean loss is no improvement, so ReduceLROnPlateau lowers lr tenfold behind it; the fourth
    epoch then moves the parameters as the float64 loop with the same scheduler does (a stale device scalar under graph replay
    would move them ten times as far)"""
    gold = np.load(GOLD)
    pool = gold_pool(gold, be.device)
    ref_params, ref_lrs = float64_loop(gold, pool.rows.cpu(), pool.videos, 4, 0)
    lr = float(gold["lr"])
    assert ref_lrs[1] == lr and ref_lrs[2] == pytest.approx(0.1 * lr) and ref_lrs[3] <= ref_lrs[2]
    for graph in modes(be):
        eng = gold_engine(gold, be.device, graph, patience=0)
        _, params, lrs, _ = fit_recorded(eng, pool, 4)
        assert lrs == ref_lrs, (graph, lrs, ref_lrs)
        for k in params[3]:
            moved64 = ref_params[3][k] - ref_params[2][k]
            moved = params[3][k].double() - params[2][k].double()
            assert float((moved - moved64).norm()) <= 1e-2 * float(moved64.norm()), (graph, k)


def test_two_fits_from_the_same_seeds_are_bit_identical(be):
    gold = np.load(GOLD)
    pool = gold_pool(gold, be.device)
    for graph in modes(be):
        runs = []
        for _ in range(2):
            eng = gold_engine(gold, be.device, graph)
            losses, params, _, _ = fit_recorded(eng, pool, 3)
            runs.append((losses, params[-1]))
        assert runs[0][0] == runs[1][0], graph
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), (graph, k)


@pytest.mark.parametrize("matrix", [True, False])
def test_two_stacked_layers_gradients_against_fp64(be, matrix):
    """num_layers 2 (dropout 0), with and without 'var': the gradients one iteration leaves in the optimiser's flat buffer (p.grad
    is its slice) against float64 autograd of the loop body on the same windows, 1e-4 of each gradient's largest element (an
    fp32 chain of two GRU layers of 5 steps; the module tests' bound for such gradients is of this size)"""
    from mnk.engine import Prediction, KeyPointPool
    B, T, K, init = 4, 5, 3, 2
    params = {"rnn_params": {"num_features": 24, "num_layers": 2, "dropout": 0}, "predict_variance": False, "num_epochs": 1,
              "lr": 1e-3, "batch_size": B, "num_frames": T, "init_frames": init, "train_size": None}
    eng = Prediction(None, None, params, num_kp=K, kp_variance="matrix" if matrix else 0.01, use_graph=False)
    torch.manual_seed(2)
    perturbed(eng.predictor, 12)
    p64 = {k: v.detach().double().requires_grad_() for k, v in eng.predictor.named_parameters()}
    kp = make_kp(B, T, K, matrix, 8)
    rows = torch.cat([kp[k].reshape(B * T, -1) for k in ("mean", "var") if k in kp], -1)
    eng.fit(KeyPointPool(rows.to(be.device).contiguous(), [(i * T, T) for i in range(B)]))
    be.sync()
    gt = {k: v.double() for k, v in kp.items()}
    x = {k: v.clone() for k, v in gt.items()}
    for k in x:
        x[k][:, init:] = 0
    out, _ = predictor64(p64, x, 2)
    loss = sum([torch.abs(gt[k][:, init:] - out[k][:, init:]).mean() for k in x])
    loss.backward()
    assert abs(float(eng.iteration_losses()[0]) - float(loss.detach())) <= 1e-5 * float(loss.detach())
    for k, p in eng.predictor.named_parameters():
        ref = p64[k].grad
        assert p.grad is not None and (p.grad.cpu().double() - ref).abs().max() <= 1e-4 * float(ref.abs().max()), k


# ---- extract / predict on the TINY networks --------------------------------------------------------------------------------------
def tiny_networks(device, generator=False):
    from oracle import cases
    from modules.keypoint_detector import KPDetector
    mp = cases.TINY["model_params"]
    torch.manual_seed(0)
    gen = None
    if generator:
        from modules.generator import MotionTransferGenerator
        gen = MotionTransferGenerator(**mp["generator_params"], **mp["common_params"])
        sd = gen.state_dict()
        cases.perturb_state_dict(sd, 7)
        gen.load_state_dict(sd)
        gen = gen.to(device).eval()
    kpd = KPDetector(**mp["kp_detector_params"], **mp["common_params"])
    sd = kpd.state_dict()
    cases.perturb_state_dict(sd, 3)
    kpd.load_state_dict(sd)
    return kpd.to(device).eval(), gen, mp["common_params"]


def tiny_params(**kw):
    p = {"rnn_params": {"num_features": 16, "num_layers": 1, "dropout": 0}, "predict_variance": True, "num_epochs": 1, "lr": 1e-3,
         "batch_size": 2, "num_frames": 5, "init_frames": 2, "train_size": None}
    p.update(kw)
    return p


def test_extract_equals_the_frame_loop(be):
    """three videos of 5, 7 and 12 frames at 32 x 32, four frames per detector call (chunks straddle the videos): the pool's rows
    against the per-frame loop of prediction.py:70-73 to 1e-5 max(1, |.|), offsets and counts; train_size = 1 keeps two videos
    (prediction.py:65-67 breaks on it > train_size); a 3-frame video with num_frames 5 raises"""
    from mnk.engine import Prediction
    kpd, _, common = tiny_networks(be.device)
    g = torch.Generator().manual_seed(2)
    videos = [torch.rand(1, 3, f, 32, 32, generator=g).to(be.device) for f in (5, 7, 12)]
    eng = Prediction(kpd, None, tiny_params(), **{k: common[k] for k in ("num_kp", "kp_variance")}, frames_per_call=4)
    pool = eng.extract(iter(videos))
    be.sync()
    assert pool.videos == [(0, 5), (5, 7), (12, 12)] and pool.rows.shape == (24, 6 * common["num_kp"])
    assert pool.rows.device == videos[0].device
    with torch.no_grad():
        for i, v in enumerate(videos):
            loop = [kpd(v[:, :, f:f + 1]) for f in range(v.shape[2])]
            ref = torch.cat([rows_of(kp["mean"][0], kp["var"][0]) for kp in loop])
            got = pool.video(i)
            assert (got - ref).abs().max() <= 1e-5 * max(1.0, float(ref.abs().max())), i
    eng1 = Prediction(kpd, None, tiny_params(train_size=1), **{k: common[k] for k in ("num_kp", "kp_variance")}, frames_per_call=4)
    assert eng1.extract(iter(videos)).videos == [(0, 5), (5, 7)]
    with pytest.raises(ValueError, match="video 1"):
        eng.extract([videos[0], videos[1][:, :, :3]])
    with pytest.raises(ValueError):
        Prediction(kpd, None, tiny_params(num_frames=2), **{k: common[k] for k in ("num_kp", "kp_variance")})


@pytest.mark.parametrize("init_frames", [1, 2])
def test_predict_equals_the_reference_statements(be, init_frames):
    """B = 2, num_frames 4 (prediction.py:119-133): given the engine's own kp_init the predicted means are within 2e-5 of
    predictor64 (tests/test_predictor_gpu.py::test_batch1_rollout's bound), the initial frames and the predict_variance copy are
    exact, and given the engine's own key points video_prediction equals the per-frame generator loop of reconstruction.generate
    to 2e-6 (the bound of the batched-transfer test)"""
    from mnk.engine import Prediction
    kpd, gen, common = tiny_networks(be.device, generator=True)
    K, T, B = common["num_kp"], 4, 2
    eng = Prediction(kpd, gen, tiny_params(num_frames=T, init_frames=init_frames),
                     **{k: common[k] for k in ("num_kp", "kp_variance")})
    torch.manual_seed(5)
    perturbed(eng.predictor.cpu(), 9).to(be.device)
    g = torch.Generator().manual_seed(4)
    video = torch.rand(B, 3, T + 2, 32, 32, generator=g).to(be.device)
    out = eng.predict(video)
    be.sync()
    assert out["video_prediction"].shape == out["video_deformed"].shape == (B, 3, T, 32, 32)
    kp_init = {k: v.cpu() for k, v in out["kp_init"].items()}
    kp_video = {k: v.cpu() for k, v in out["kp_driving"].items()}
    with torch.no_grad():
        whole = kpd(video[:, :, :T])
    for k in kp_init:
        assert torch.equal(kp_init[k][:, :init_frames], whole[k][:, :init_frames].cpu()) and (kp_init[k][:, init_frames:] == 0).all()
        assert torch.equal(out["kp_source"][k].cpu(), whole[k][:, :1].cpu())
    params64 = {k: v.detach().cpu().double() for k, v in eng.predictor.named_parameters()}
    ref, _ = predictor64(params64, {k: v.double() for k, v in kp_init.items()}, 1)
    assert (kp_video["mean"][:, init_frames:].double() - ref["mean"][:, init_frames:]).abs().max() < 2e-5
    assert torch.equal(kp_video["mean"][:, :init_frames], kp_init["mean"][:, :init_frames])
    for t in range(T):                                   # predict_variance: copied from frame init_frames - 1, not predicted
        assert torch.equal(kp_video["var"][:, t], kp_init["var"][:, init_frames - 1])
    # the generator, frame by frame (reconstruction.py:12-25)
    src = video[:, :, :1].contiguous()
    with torch.no_grad():
        frames = [gen(src, kp_driving={k: v[:, i:i + 1].contiguous() for k, v in out["kp_driving"].items()},
                      kp_source={k: v.contiguous() for k, v in out["kp_source"].items()})["video_prediction"] for i in range(T)]
    be.sync()
    loop = torch.cat(frames, dim=2)
    assert (out["video_prediction"] - loop).abs().max() <= 2e-6
    # the output side takes the tensors as they are (prediction.py:135-141)
    from mnk.visualizer import Visualizer, png_strip
    assert png_strip(out["video_prediction"]).shape == (32, T * 32, 3)
    grid = Visualizer(kp_size=2).visualize_reconstruction({"video": video[:, :, :T], "source": video[:, :, :1]}, out)
    assert grid.dtype == np.uint8 and grid.shape[0] == T


def test_predicted_variance_is_kept_when_the_flag_is_unset(be):
    """predict_variance unset: the GRU's own covariances V^T V behind the initial frames, kp_init's in them"""
    from mnk.engine import Prediction
    kpd, gen, common = tiny_networks(be.device, generator=True)
    eng = Prediction(kpd, gen, tiny_params(num_frames=4, init_frames=2, predict_variance=False),
                     **{k: common[k] for k in ("num_kp", "kp_variance")})
    torch.manual_seed(5)
    perturbed(eng.predictor.cpu(), 9).to(be.device)
    g = torch.Generator().manual_seed(4)
    out = eng.predict(torch.rand(1, 3, 4, 32, 32, generator=g).to(be.device))
    be.sync()
    kp_init = {k: v.cpu() for k, v in out["kp_init"].items()}
    params64 = {k: v.detach().cpu().double() for k, v in eng.predictor.named_parameters()}
    ref, _ = predictor64(params64, {k: v.double() for k, v in kp_init.items()}, 1)
    var = out["kp_driving"]["var"].cpu()
    assert torch.equal(var[:, :2], kp_init["var"][:, :2])
    assert (var[:, 2:].double() - ref["var"][:, 2:]).abs().max() < 2e-5 * max(1.0, float(ref["var"].abs().max()))


# ---- full size, MI355X only -----------------------------------------------------------------------------------------------------
def synthetic_pool(device, videos, frames, K, seed):
    from mnk.engine import KeyPointPool
    kp = make_kp(videos, frames, K, True, seed)
    rows = torch.cat([kp["mean"].reshape(videos * frames, -1), kp["var"].reshape(videos * frames, -1)], -1)
    return KeyPointPool(rows.to(device).contiguous(), [(i * frames, frames) for i in range(videos)])


def full_engine(device, H, B, T, K, use_graph, seed):
    from mnk.engine import Prediction
    params = {"rnn_params": {"num_features": H, "num_layers": 1, "dropout": 0}, "predict_variance": True, "num_epochs": 1,
              "lr": 1e-3, "batch_size": B, "num_frames": T, "init_frames": 1, "train_size": None}
    eng = Prediction(None, None, params, num_kp=K, kp_variance="matrix", use_graph=use_graph)
    torch.manual_seed(seed)
    perturbed(eng.predictor.cpu(), seed + 100).to(device)
    return eng


@pytest.mark.gpu
def test_full_size_graph_replay_equals_eager_bit_for_bit(make_backend):
    """B = 256, T = 32, K = 10 with 'var', H = 1024 (every shipped configuration's shape), three iterations: graph replay i equals
    eager iteration i bit for bit, in the losses and in a sample of every parameter.  No CPU reference at this size."""
    hip = make_backend("hip")
    B, T, K, H = 256, 32, 10, 1024
    pool = synthetic_pool(hip.device, 3 * B, T + 3, K, 21)
    runs = []
    for graph in (False, True):
        eng = full_engine(hip.device, H, B, T, K, graph, 7)
        np.random.seed(5)
        eng.fit(pool, num_epochs=1)
        torch.cuda.synchronize()
        runs.append((eng.iteration_losses().cpu(), {k: v.detach().flatten()[::97].cpu().clone()
                                                    for k, v in eng.predictor.named_parameters()}))
    assert runs[0][0].numel() == 3 and torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.gpu
def test_ten_iterations_against_fp64(make_backend):
    """B = 32, T = 32, H = 256, K = 10: ten iterations (one epoch of ten batches) against the float64 restatement with stock Adam,
    with the bounds of tests/test_predictor_gpu.py::test_ten_training_iterations_with_adam"""
    hip = make_backend("hip")
    torch.set_num_threads(16)
    B, T, K, H = 32, 32, 10, 256
    pool = synthetic_pool(hip.device, 10 * B, T, K, 33)               # windows of T frames in videos of T frames: start 0
    eng = full_engine(hip.device, H, B, T, K, None, 7)
    start = {k: v.detach().cpu().clone() for k, v in eng.predictor.named_parameters()}
    p64 = {k: v.double().requires_grad_() for k, v in start.items()}
    np.random.seed(1)
    eng.fit(pool, num_epochs=1)
    torch.cuda.synchronize()
    losses = eng.iteration_losses().cpu().tolist()
    opt64 = torch.optim.Adam(list(p64.values()), lr=1e-3)
    rows, losses64 = pool.rows.cpu().double(), []
    for it in range(10):
        r = rows[it * B * T:(it + 1) * B * T].view(B, T, -1)
        gt = {"mean": r[..., :2 * K].reshape(B, T, K, 2), "var": r[..., 2 * K:].reshape(B, T, K, 2, 2)}
        x = {k: v.clone() for k, v in gt.items()}
        for k in x:
            x[k][:, 1:] = 0
        out, _ = predictor64(p64, x, 1)
        loss64 = sum([torch.abs(gt[k][:, 1:] - out[k][:, 1:]).mean() for k in x])
        loss64.backward()
        opt64.step()
        opt64.zero_grad()
        losses64.append(float(loss64.detach()))
    print(losses, losses64)
    for a, b in zip(losses, losses64):
        assert abs(a - b) <= 1e-5 * abs(b), (losses, losses64)
    assert losses[-1] < losses[0]
    for k, p in eng.predictor.named_parameters():
        moved64 = p64[k].detach() - start[k].double()
        moved = p.detach().cpu().double() - start[k].double()
        assert float((moved - moved64).norm()) <= 1e-2 * float(moved64.norm()), k
