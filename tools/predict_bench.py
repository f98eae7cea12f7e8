#!/usr/bin/env python
"""Time the prediction task's key-point GRU on the GPU: the native mnk.predictor.PredictionModule against the stock one (nn.GRU +
nn.Linear, the reference's modules/prediction_module.py restated) on the same device, in the same process, alternating after
warm-up, each timing closed by a device synchronise.

  training:  one iteration of prediction.py:97-107 at B=256, T=32, I=60, H=1024 (mask the frames after init_frames, forward,
             L1 on both keys, backward, torch.optim.Adam step)
  inference: prediction.py:116-132's batch-1, 32-frame roll-out under no_grad in evaluation mode

Prints one JSON line: median milliseconds of both forms for both shapes, and the training iteration's algorithmic GFLOP over time
against the 157.3 TFLOP/s fp32 matrix peak.

With --engine the line also carries train_ms_engine_eager / train_ms_engine_graph: mnk.engine.Prediction.fit on a device-resident
key-point pool (window gather, forward, the L1 loss fused with the head, backward, MnkAdam; eager launches / one hipGraph replay
per iteration), timed in the same alternation as one fit() of --engine-epochs epochs of --engine-iters iterations -- window
draws, the epoch mean read by the host and the scheduler step included -- divided by the iterations.  (The windows of an epoch
are drawn on the host while the device works on the epoch before; only the first epoch's draws of a fit() are exposed.)  Its
yard-stick is train_ms_native of the same run.

  python tools/predict_bench.py [--iters 20] [--warmup 3] [--batch 256] [--frames 32] [--hidden 1024] [--num-kp 10] [--engine]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monkey-net_amd"))

import torch                                         # noqa: E402
from torch import nn                                 # noqa: E402

PEAK_TFLOPS = 157.3


class StockPredictor(nn.Module):
    """modules/prediction_module.py on stock torch (nn.GRU runs MIOpen on ROCm)"""

    def __init__(self, num_kp, kp_variance, num_features):
        super().__init__()
        input_size = num_kp * (2 + 4 * (kp_variance == 'matrix'))
        self.rnn = nn.GRU(input_size=input_size, hidden_size=num_features, num_layers=1, dropout=0, batch_first=True)
        self.linear = nn.Linear(num_features, input_size)

    def forward(self, kp_batch):
        bs, d, num_kp, _ = kp_batch['mean'].shape
        inputs = [kp_batch['mean'].contiguous().view(bs, d, -1)]
        if 'var' in kp_batch:
            inputs.append(kp_batch['var'].contiguous().view(bs, d, -1))
        output, _ = self.rnn(torch.cat(inputs, dim=-1))
        init_shape = output.shape
        output = self.linear(output.contiguous().view(-1, output.shape[-1])).view(init_shape[0], init_shape[1], -1)
        output = output.view(bs, d, num_kp, -1)
        res = {'mean': torch.tanh(output[:, :, :, :2])}
        if 'var' in kp_batch:
            var = output[:, :, :, 2:].view(bs, d, num_kp, 2, 2)
            res['var'] = torch.matmul(var.permute(0, 1, 2, 4, 3), var)
        return res


def train_gflop(B, T, I, H):
    rows = B * T
    fwd = 2.0 * rows * H * 3 * H + 2.0 * rows * I * 3 * H + 2.0 * rows * H * I
    bwd = 2 * (2.0 * rows * 3 * H * H) + 2 * (2.0 * rows * 3 * H * I) + 2 * (2.0 * rows * I * H)
    return (fwd + bwd) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--num-kp", type=int, default=10)
    ap.add_argument("--init-frames", type=int, default=1)
    ap.add_argument("--engine", action="store_true", help="also time mnk.engine.Prediction.fit, eager and as hipGraph replay")
    ap.add_argument("--engine-iters", type=int, default=4, help="iterations per epoch of the engine forms")
    ap.add_argument("--engine-epochs", type=int, default=8, help="epochs per timed fit() of the engine forms")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("predict_bench.py times the GPU: no device found")
    from mnk.predictor import PredictionModule
    dev = torch.device("cuda:0")
    B, T, H, K = a.batch, a.frames, a.hidden, a.num_kp
    I = 6 * K
    torch.manual_seed(0)
    native = PredictionModule(num_kp=K, kp_variance="matrix", num_features=H, num_layers=1, dropout=0).to(dev)
    stock = StockPredictor(K, "matrix", H).to(dev)
    stock.load_state_dict(native.state_dict())
    opts = {"native": torch.optim.Adam(native.parameters(), lr=1e-3), "stock": torch.optim.Adam(stock.parameters(), lr=1e-3)}
    mods = {"native": native, "stock": stock}

    g = torch.Generator().manual_seed(1)

    def batch(b):
        v = torch.randn(b, T, K, 2, 2, generator=g) * 0.3
        return {"mean": (torch.rand(b, T, K, 2, generator=g) * 2 - 1).to(dev), "var": (v.transpose(-1, -2) @ v).to(dev)}

    train_x = batch(B)
    infer_x = batch(1)
    for k in infer_x:
        infer_x[k][:, a.init_frames:] = 0

    def train_iter(name):
        mod, opt = mods[name], opts[name]
        mod.train()
        x = {k: v.clone() for k, v in train_x.items()}
        gt = {k: v.clone() for k, v in x.items()}
        for k in x:
            x[k][:, a.init_frames:] = 0
        prediction = mod(x)
        loss = sum([torch.abs(gt[k][:, a.init_frames:] - prediction[k][:, a.init_frames:]).mean() for k in x])
        loss.backward()
        opt.step()
        opt.zero_grad()

    def infer(name):
        mod = mods[name]
        mod.eval()
        with torch.no_grad():
            kp_video = mod(infer_x)
            for k in kp_video:
                kp_video[k][:, :a.init_frames] = infer_x[k][:, :a.init_frames]

    def timed(fn, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    engines = {}
    if a.engine:
        from mnk.engine import Prediction, KeyPointPool
        videos = a.engine_iters * B
        rows = torch.cat([torch.cat([v.reshape(B * T, -1) for v in batch(B).values()], -1) for _ in range(a.engine_iters)])
        pool = KeyPointPool(rows.contiguous(), [(i * T, T) for i in range(videos)])
        params = {"rnn_params": {"num_features": H, "num_layers": 1, "dropout": 0}, "predict_variance": True, "num_epochs": 1,
                  "lr": 1e-3, "batch_size": B, "num_frames": T, "init_frames": a.init_frames, "train_size": None}
        for form, graph in (("engine_eager", False), ("engine_graph", True)):
            eng = Prediction(None, None, params, num_kp=K, kp_variance="matrix", use_graph=graph)
            eng.predictor.load_state_dict(native.state_dict())
            engines[form] = eng

    def engine_epoch(form):
        engines[form].fit(pool, num_epochs=a.engine_epochs)

    times = {(w, n): [] for w in ("train", "infer") for n in mods}
    times.update({("train", form): [] for form in engines})
    for i in range(a.warmup + a.iters):
        for form in (sorted(engines) if i % 2 == 0 else sorted(engines, reverse=True)):
            ms = timed(engine_epoch, form) / (a.engine_iters * a.engine_epochs)
            if i >= a.warmup:
                times[("train", form)].append(ms)
        for w, fn in (("train", train_iter), ("infer", infer)):
            for n in (("native", "stock") if i % 2 == 0 else ("stock", "native")):
                ms = timed(fn, n)
                if i >= a.warmup:
                    times[(w, n)].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    gf = train_gflop(B, T, I, H)
    floor_ms = gf / (PEAK_TFLOPS * 1e3) * 1e3
    res = {
        "workload": "prediction_gru", "batch": B, "frames": T, "input": I, "hidden": H, "iters": a.iters,
        "train_ms_native": round(med[("train", "native")], 3), "train_ms_stock": round(med[("train", "stock")], 3),
        "infer_ms_native": round(med[("infer", "native")], 3), "infer_ms_stock": round(med[("infer", "stock")], 3),
        "train_gflop": round(gf, 2), "floor_ms_at_peak": round(floor_ms, 3),
        "train_tflops_native": round(gf / med[("train", "native")], 2),
        "train_tflops_stock": round(gf / med[("train", "stock")], 2),
        "train_frac_of_peak_native": round(floor_ms / med[("train", "native")], 4),
        "train_frac_of_peak_stock": round(floor_ms / med[("train", "stock")], 4),
        "train_speedup": round(med[("train", "stock")] / med[("train", "native")], 3),
        "infer_speedup": round(med[("infer", "stock")] / med[("infer", "native")], 3),
    }
    for form in engines:
        res["train_ms_" + form] = round(med[("train", form)], 3)
    if engines:
        res["engine_iters_per_epoch"], res["engine_epochs_per_fit"] = a.engine_iters, a.engine_epochs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
