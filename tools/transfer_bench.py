#!/usr/bin/env python
"""Time mnk.engine.Transfer on the GPU box with the source repeated per driving frame (shared_source=False: the appearance
encoder runs on B*d identical rows) and with the source shared by the frames of its video (shared_source=True: it runs on B rows,
the warps read source row v for every frame of video v).

  moving-gif model (mnk.configs), 64 x 64, B = 1, d = 8 and d = 32 driving frames, eval mode, seeded weights and inputs

Each d runs in a fresh process of its own under `timeout -k 10`; a d that fails ends the run.  Per d: the two forms are compared
first (max |difference| of both outputs is reported), then timed alternately after warm-up -- every call between two HIP events
on the stream, median and minimum of >= 20 calls -- and the peak of torch's allocated memory over one call of each form is read
after a reset.  ONE JSON line for the whole run.

  python tools/transfer_bench.py [--iters 30] [--warmup 5] [--timeout 300] [--forms repeated,shared]

`--forms repeated` times the repeated form alone (a tree whose Transfer has no `shared_source` yet: the baseline)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (8, 32)
CONFIG, SIZE, BATCH = "moving-gif", 64, 1


def child(d, iters, warmup, forms):
    for p in (ROOT, os.path.join(ROOT, "monkey-net_amd")):
        sys.path.insert(0, p)
    import torch
    from mnk import configs, engine
    from modules.generator import MotionTransferGenerator
    from modules.keypoint_detector import KPDetector
    from oracle import cases
    assert torch.cuda.is_available(), "transfer_bench needs the GPU: a CPU timing says nothing about it"
    dev = torch.device("cuda:0")
    mp = configs.get(CONFIG)["model_params"]
    torch.manual_seed(0)
    gen = MotionTransferGenerator(**mp["generator_params"], **mp["common_params"])
    kpd = KPDetector(**mp["kp_detector_params"], **mp["common_params"])
    for i, m in enumerate((gen, kpd)):
        sd = m.state_dict()
        cases.perturb_state_dict(sd, 7 + i)
        m.load_state_dict(sd)
    gen.to(dev), kpd.to(dev)
    src = cases.smooth_pair(BATCH, SIZE, SIZE, seed=11)[0].to(dev)
    driving = torch.cat([cases.smooth_pair(BATCH, SIZE, SIZE, seed=20 + i)[1] for i in range(d)], dim=2).to(dev)
    params = dict(movement_mult=False, move_location=True, adapt_variance=True, clip_mean=True)
    runs = {}
    if "repeated" in forms:
        runs["repeated"] = engine.Transfer(kpd, gen, params)
    if "shared" in forms:
        runs["shared"] = engine.Transfer(kpd, gen, params, shared_source=True)
    outs = {name: t(src, driving) for name, t in runs.items()}
    torch.cuda.synchronize()
    rec = {"frames": d}
    if len(outs) == 2:
        for k in ("video_prediction", "video_deformed"):
            rec["max_abs_diff_" + k] = float((outs["shared"][k] - outs["repeated"][k]).abs().max())
            assert rec["max_abs_diff_" + k] < 1e-4, "the two forms differ: no timing"
    del outs
    times = {name: [] for name in runs}
    for i in range(warmup + iters):
        for name, t in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t(src, driving)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    for name, t in runs.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = t(src, driving)
        torch.cuda.synchronize()
        rec[name + "_ms_median"] = round(statistics.median(times[name]), 4)
        rec[name + "_ms_min"] = round(min(times[name]), 4)
        rec[name + "_peak_allocated_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        del out
    if len(runs) == 2:
        rec["shared_over_repeated"] = round(rec["shared_ms_median"] / rec["repeated_ms_median"], 4)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per d")
    ap.add_argument("--forms", default="repeated,shared")
    ap.add_argument("--child", type=int, choices=FRAMES)
    a = ap.parse_args()
    forms = [f for f in a.forms.split(",") if f]
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if not forms or any(f not in ("repeated", "shared") for f in forms):
        ap.error("--forms takes repeated, shared or both")
    if a.child:
        return child(a.child, a.iters, a.warmup, forms)
    results = []
    for d in FRAMES:
        run = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(d),
                              "--iters", str(a.iters), "--warmup", str(a.warmup), "--forms", ",".join(forms)],
                             stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, text=True)
        if run.returncode != 0:
            sys.exit("transfer_bench: d = %d ended with status %d; nothing more is started" % (d, run.returncode))
        results.append(json.loads(run.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "transfer_bench", "config": CONFIG, "size": [SIZE, SIZE], "batch": BATCH, "mode": "eval",
                      "calls": a.iters, "warmup": a.warmup, "timer": "hip events, median over calls", "results": results}))


if __name__ == "__main__":
    main()
