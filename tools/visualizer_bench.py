#!/usr/bin/env python
"""Time the visualiser on the GPU box: mnk.visualizer.Visualizer (one launch on the device, only the uint8 grid crosses PCIe)
against the numpy restatement of the reference's logger.Visualizer (tests/test_visualizer.py::reference_grid, pinned to the
recorded reference grids) on the same machine, fed the same device tensors -- its `.cpu()` copies are part of its time, as
they are part of logger.py:155-164.

  reconstruction: one visualize_reconstruction call on a 32-frame 64 x 64 video with 10 key points (reconstruction.py:70)
  training:       the batch-32 training grid (train.py's Logger.visualize_rec: 32 videos of one frame)

Each shape runs in a fresh process of its own under `timeout -k 10`; a shape that fails ends the run.  Per shape: the two grids
are compared for equality first, then both forms are timed alternately after warm-up -- median wall milliseconds of >= 20 calls,
every call closed by a device synchronise -- and the grid launch alone between two HIP events.  One JSON line per shape.

  python tools/visualizer_bench.py [--iters 30] [--warmup 5] [--timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"reconstruction": (1, 32), "training": (32, 1)}          # name: (batch, frames)


def child(shape, iters, warmup):
    for p in (ROOT, os.path.join(ROOT, "monkey-net_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from mnk import ops
    from mnk.visualizer import Visualizer
    from test_visualizer import colors_for, random_kp, reconstruction_columns, reference_grid, to_numpy, tricky_frames
    assert torch.cuda.is_available(), "visualizer_bench needs the GPU: a CPU timing says nothing about it"
    dev = torch.device("cuda:0")
    b, d = SHAPES[shape]
    h = w = 64
    k = 10
    inp = {"source": tricky_frames(1, b, 3, 1, h, w).to(dev), "video": tricky_frames(2, b, 3, d, h, w).to(dev)}
    out = {"video_prediction": tricky_frames(3, b, 3, d, h, w).to(dev), "video_deformed": tricky_frames(4, b, 3, d, h, w).to(dev),
           "kp_source": {"mean": random_kp(5, b, 1, k).to(dev)}, "kp_driving": {"mean": random_kp(6, b, d, k).to(dev)}}
    vis = Visualizer()
    colors = colors_for(k).numpy()

    def native():
        return vis.visualize_reconstruction(inp, out)

    def host():
        return reference_grid(to_numpy(reconstruction_columns(inp, out)), d, 2, False, colors)

    assert np.array_equal(native(), host()), "the two forms differ: no timing"
    t_native, t_host = [], []
    for i in range(warmup + iters):
        for fn, acc in ((native, t_native), (host, t_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                acc.append((time.perf_counter() - t0) * 1e3)
    # the launch alone, between two HIP events on the stream
    cols = reconstruction_columns(inp, out)
    dcolors = vis.colors(k, dev)
    grid = torch.empty(d, b * h, 5 * w, 3, dtype=torch.uint8, device=dev)
    t_kernel = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.vis_grid(cols, d, 2, False, dcolors, out=grid)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            t_kernel.append(e0.elapsed_time(e1))
    read_bytes = (2 * b * 3 * h * w + 3 * b * 3 * d * h * w) * 4         # the source frame once (it is repeated d times from cache)
    print(json.dumps({"shape": shape, "batch": b, "frames": d, "size": [h, w], "num_kp": k, "calls": iters,
                      "native_ms_median": round(statistics.median(t_native), 4), "native_ms_min": round(min(t_native), 4),
                      "host_restatement_ms_median": round(statistics.median(t_host), 3), "host_restatement_ms_min": round(min(t_host), 3),
                      "grid_launch_event_ms_median": round(statistics.median(t_kernel), 4),
                      "grid_bytes": int(grid.numel()), "fp32_bytes_read": read_bytes, "bytes_equal": True}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--child", choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    if a.child:
        return child(a.child, a.iters, a.warmup)
    for shape in SHAPES:
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", shape,
                             "--iters", str(a.iters), "--warmup", str(a.warmup)], stdin=subprocess.DEVNULL).returncode
        if rc != 0:
            sys.exit("visualizer_bench: shape %r ended with status %d; nothing more is started" % (shape, rc))


if __name__ == "__main__":
    main()
