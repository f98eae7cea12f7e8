#!/usr/bin/env python
"""Records tests/golden/prediction_loop.npz: the data path and the training loop of the UNMODIFIED reference's prediction.py
(imported from MNK_REFERENCE_ROOT through oracle.ref_shim; works only where the reference tree exists), for
tests/test_prediction_engine.py.

    python tools/make_golden_prediction.py            # writes the fixture
    python tools/make_golden_prediction.py --check    # re-runs the reference and compares with the committed fixture

`tqdm`, `imageio` and `logger` are stubbed where the import of prediction.py needs them (its loop never calls them here).  What
runs is the reference's own code: prediction.KPDataset (augmentation.SelectRandomFrames inside), torch's DataLoader and
modules.prediction_module.PredictionModule; the loop body around them follows prediction.py:94-111 statement by statement.

Setup: a synthetic key-point array in the format prediction.py:64-74 builds (per video a list of per-frame dicts of numpy
arrays, mean (1, 1, K, 2), var (1, 1, K, 2, 2)): four videos of 5, 7, 12 and 5 frames, K = 3; num_frames 5, init_frames 2,
batch_size 3, lr 1e-3; np.random.seed(3) in front of the first epoch.

Stored (numpy arrays only):
  frames, num_kp, num_frames, init_frames, batch_size, lr, epochs
  kp_mean_v{i} (F, K, 2), kp_var_v{i} (F, K, 2, 2)         the synthetic key points of video i
  gt_mean_e{e}_b{j}, gt_var_e{e}_b{j}                       the batches KPDataset + DataLoader yield in epoch e (the short last one too)
  losses (epochs * batches)                                 the loss of every iteration: PredictionModule(num_features 16) in
                                                            float64, created after torch.manual_seed(0), Adam + ReduceLROnPlateau
  before.<name>, after.<name>                               its parameters in front of the first and behind the last iteration"""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "prediction_loop.npz")
FRAMES, NUM_KP, NUM_FRAMES, INIT_FRAMES, BATCH, LR, EPOCHS, FEATURES = (5, 7, 12, 5), 3, 5, 2, 3, 1e-3, 3, 16


def reference_prediction():
    from oracle import ref_shim
    ref_shim.install()
    passthrough = lambda it=None, *a, **k: it
    for name, attrs in (("tqdm", {"tqdm": passthrough, "trange": lambda n, *a, **k: range(n)}),
                        ("imageio", {"mimread": None, "imsave": None, "mimsave": None}),
                        ("logger", {"Logger": None, "Visualizer": None})):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)      # (torch looks optional packages up with find_spec)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    import prediction
    from modules.prediction_module import PredictionModule
    return prediction, PredictionModule


def synthetic_keypoints():
    rng = np.random.RandomState(11)                      # (its own stream: the global np.random is the loop's)
    out = []
    for f in FRAMES:
        video = []
        for _ in range(f):
            v = rng.randn(1, 1, NUM_KP, 2, 2).astype(np.float32) * 0.3
            video.append({"mean": rng.uniform(-1, 1, (1, 1, NUM_KP, 2)).astype(np.float32),
                          "var": (np.swapaxes(v, -1, -2) @ v + 0.05 * np.eye(2, dtype=np.float32)).astype(np.float32)})
        out.append(video)
    return out


def record():
    from torch.utils.data import DataLoader
    prediction, PredictionModule = reference_prediction()
    keypoints_array = synthetic_keypoints()
    res = {"frames": np.array(FRAMES), "num_kp": np.array(NUM_KP), "num_frames": np.array(NUM_FRAMES),
           "init_frames": np.array(INIT_FRAMES), "batch_size": np.array(BATCH), "lr": np.array(LR), "epochs": np.array(EPOCHS)}
    for i, video in enumerate(keypoints_array):
        res["kp_mean_v%d" % i] = np.concatenate([f["mean"][0] for f in video], axis=0)
        res["kp_var_v%d" % i] = np.concatenate([f["var"][0] for f in video], axis=0)

    torch.manual_seed(0)
    predictor = PredictionModule(num_kp=NUM_KP, kp_variance="matrix", num_features=FEATURES)
    for k, v in predictor.state_dict().items():
        res["before." + k] = v.numpy().copy()
    predictor = predictor.double()
    optimizer = torch.optim.Adam(predictor.parameters(), lr=LR)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=50)
    kp_dataloader = DataLoader(prediction.KPDataset(keypoints_array, num_frames=NUM_FRAMES), batch_size=BATCH)
    np.random.seed(3)
    losses = []
    for e in range(EPOCHS):                              # prediction.py:94-111
        loss_list = []
        for j, x in enumerate(kp_dataloader):
            for k, v in x.items():
                res["gt_%s_e%d_b%d" % (k, e, j)] = v.numpy().copy()
            x = {k: v.double() for k, v in x.items()}
            gt = {k: v.clone() for k, v in x.items()}
            for k in x:
                x[k][:, INIT_FRAMES:] = 0
            out = predictor(x)
            loss = sum([torch.abs(gt[k][:, INIT_FRAMES:] - out[k][:, INIT_FRAMES:]).mean() for k in x])
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            loss_list.append(loss.detach().numpy())
        losses += [float(v) for v in loss_list]
        scheduler.step(np.mean(loss_list))
    res["losses"] = np.array(losses, dtype=np.float64)
    for k, v in predictor.state_dict().items():
        res["after." + k] = v.numpy().copy()
    return res


def main():
    res = record()
    if "--check" in sys.argv[1:]:
        gold = np.load(OUT)
        assert sorted(gold.files) == sorted(res), "the fixture's keys differ"
        for k in gold.files:
            assert np.array_equal(gold[k], res[k]) if k.startswith(("gt_", "kp_", "before.")) else \
                np.allclose(gold[k], res[k], rtol=1e-9, atol=1e-12), k
        print("prediction_loop.npz equals a fresh run of the reference")
        return
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
