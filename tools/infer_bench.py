#!/usr/bin/env python
"""Evaluation-mode forward (kp detector on source + driving frames, generator) through mnk.engine.Reconstructor.
Default (BASELINE config 5): bair 64x64, batch 512 -- frames/s for eager launches and for hipGraph replay.
--precision-ab: fp32 against the opt-in bf16 inference mode (precision="bf16": the 3x3 convolutions round their operands to
bf16) at four configurations -- bair batch 512 @ 64 eager, moving-gif batch 64 @ 64, vox batch 8 @ 256, and the reference's
batch-1 frame loop behind DataParallelWithCallback (mnk.dropin.EvalRunner under MNK_EVAL_PRECISION).  The two forms alternate,
`--reps` timings each; median and spread (max - min) per form, one JSON line per configuration.
--fuse-ab: the default against the opt-in evaluation-mode norm fusion (fuse_norm=True / MNK_EVAL_FUSE_NORM=1: unsplit convolutions
apply the norm layer, ReLU and pool behind them in their own epilogue) at the same four configurations, in fp32 and in bf16;
alternating timings as above, plus -- for the batched configurations -- the conv and norm-apply kernel groups of the library's
event recorder per forward in either form (what the separate norm passes cost) and the count of fused / deferred / separate
conv -> norm pairs.
--skinny-ab: the default against the opt-in weight-streaming convolutions (skinny=True / MNK_EVAL_SKINNY=1: conv -> norm pairs
with at most `skinny_rows` output rows) -- the batch-1 frame loop through EvalRunner (moving-gif, taichi @ 64, vox @ 256), where
the form applies, and the batched configurations, where no layer is under the threshold; fp32 and bf16, alternating timings as
above, the count of layers that took the form, and the largest difference of the outputs."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "monkey-net_amd"))
import torch
from mnk import configs, engine
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="bair"); ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--size", type=int, default=64); ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--precision-ab", action="store_true"); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fuse-ab", action="store_true")
ap.add_argument("--skinny-ab", action="store_true")
ap.add_argument("--only", default="", help="--precision-ab / --fuse-ab / --skinny-ab: comma-separated subset of bair,moving-gif,vox,frame-loop")
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn, iters):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(forms, iters, reps):
    """forms: {name: callable}; -> {name: {"ms": median, "spread_ms": max - min}}, the forms timed in turn `reps` times"""
    for fn in forms.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    return {k: {"ms": round(sorted(v)[len(v) // 2], 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in times.items()}


def reconstructor_ab(config, batch, size, iters, field, values, precision="fp32", extras=None):
    """Reconstructor(precision=precision, field=value) for each of values = {form: value}, the baseline first, alternating;
    extras(res, recs, src, drv) adds what the A/B reports besides the timings"""
    gen, disc, kpd = bench.build_models(configs.get(config), dev)
    src = torch.rand(batch, 3, 1, size, size, device=dev)
    drv = torch.rand(batch, 3, 1, size, size, device=dev)
    recs = {f: engine.Reconstructor(kpd, gen, **{"precision": precision, field: v}) for f, v in values.items()}
    res = alternate({f: (lambda r=r: r(src, drv)) for f, r in recs.items()}, iters, args.reps)
    if extras:
        extras(res, recs, src, drv)
    base, other = values
    tag = "" if field == "precision" else " %s," % precision
    return {"workload": "%s Reconstructor eager,%s batch %d @ %dx%d" % (config, tag, batch, size, size), **res,
            "speedup": round(res[base]["ms"] / res[other]["ms"], 3)}


def frame_loop_ab(config, size, frames, iters, variable, values, precision=None, extras=None):
    """reconstruction.py:45-62: both networks behind DataParallelWithCallback, one frame per call under no_grad, with the
    environment `variable` alternating over values = {form: value}, the baseline first (precision: MNK_EVAL_PRECISION of both);
    extras(res, last) adds what the A/B reports besides the timings, last = {form: the last prediction}"""
    from sync_batchnorm import DataParallelWithCallback
    gen, disc, kpd = bench.build_models(configs.get(config), dev)
    generator, kp_detector = DataParallelWithCallback(gen), DataParallelWithCallback(kpd)
    generator.eval(), kp_detector.eval()
    video = torch.rand(1, 3, frames, size, size, device=dev)
    if precision:
        os.environ["MNK_EVAL_PRECISION"] = precision
    last = {}

    def loop(form):
        os.environ[variable] = values[form]
        with torch.no_grad():
            kp_source = kp_detector(video[:, :, :1])
            for i in range(frames):
                kp_driving = kp_detector(video[:, :, i:i + 1])
                last[form] = generator(source_image=video[:, :, :1], kp_driving=kp_driving, kp_source=kp_source)["video_prediction"]

    res = alternate({f: (lambda f=f: loop(f)) for f in values}, iters, args.reps)
    if extras:
        extras(res, last)
    os.environ.pop(variable, None); os.environ.pop("MNK_EVAL_PRECISION", None)
    base, other = values
    for f in values:
        res[f]["ms_per_frame"] = round(res[f]["ms"] / frames, 4)
    tag = " %s," % precision if precision else ""
    return {"workload": "%s frame loop through EvalRunner,%s batch 1 @ %dx%d, %d frames per loop" % (config, tag, size, size, frames), **res,
            "speedup": round(res[base]["ms"] / res[other]["ms"], 3)}


def precision_extras(res, recs, src, drv):
    a, b = recs["fp32"](src, drv)["video_prediction"], recs["bf16"](src, drv)["video_prediction"]
    res["max_abs_prediction_difference"] = float((a - b).abs().max())


def fuse_extras(res, recs, src, drv):
    from mnk import _lib, ops
    a, b = recs["default"](src, drv), recs["fused"](src, drv)
    res["outputs_equal"] = all(torch.equal(a[k], b[k]) for k in a)
    for f, r in recs.items():
        ops.clear_eval_norm_count()
        r(src, drv)
        res[f]["pairs_fused_elem_pool_deferred_separate"] = list(ops.EVAL_NORM_COUNT)
        groups = bench.prof_collect(_lib.lib(), lambda r=r: r(src, drv), 3)
        res[f]["groups"] = {k: {"launches": round(v["launches_per_step"], 1), "ms": round(v["ms_per_step"], 4)}
                            for k, v in groups.items() if k in ("conv3x3_igemm", "bn_act_apply", "conv3x3_reduce_pack")}
        res[f]["all_groups_ms"] = round(sum(v["ms_per_step"] for v in groups.values()), 4)


def skinny_extras(res, recs, src, drv):
    from mnk import ops
    a, b = recs["default"](src, drv), recs["skinny"](src, drv)
    res["max_abs_output_difference"] = max(float((a[k] - b[k]).abs().max()) for k in a)
    ops.clear_eval_skinny_count()
    recs["skinny"](src, drv)
    res["skinny_layers"] = ops.EVAL_SKINNY_COUNT[0]


def skinny_loop_extras(res, last):
    from mnk import ops
    res["skinny_layers_captured"] = ops.EVAL_SKINNY_COUNT[0]      # counted while the programs were captured (warm-up + capture passes)
    res["max_abs_prediction_difference"] = float((last["default"] - last["skinny"]).abs().max())


def frame_loop_skinny_ab(*job):
    from mnk import ops
    ops.clear_eval_skinny_count()
    return frame_loop_ab(*job, "MNK_EVAL_SKINNY", {"default": "0", "skinny": "1"}, precision, skinny_loop_extras)


FUSED, SKINNY = {"default": False, "fused": True}, {"default": False, "skinny": True}
if args.skinny_ab:
    only = set(filter(None, args.only.split(",")))
    for precision in ("fp32", "bf16"):
        jobs = [("frame-loop", lambda: frame_loop_skinny_ab("moving-gif", 64, 16, max(2, args.iters // 2))),
                ("frame-loop-taichi", lambda: frame_loop_skinny_ab("taichi", 64, 16, max(2, args.iters // 2))),
                ("frame-loop-vox", lambda: frame_loop_skinny_ab("vox", 256, 8, max(2, args.iters // 2))),
                ("bair", lambda: reconstructor_ab("bair", 512, 64, args.iters, "skinny", SKINNY, precision, skinny_extras)),
                ("moving-gif", lambda: reconstructor_ab("moving-gif", 64, 64, args.iters, "skinny", SKINNY, precision, skinny_extras))]
        for name, job in jobs:
            if not only or name in only:
                print(json.dumps(job()), flush=True)
    sys.exit(0)

if args.fuse_ab:
    only = set(filter(None, args.only.split(",")))
    for precision in ("fp32", "bf16"):
        jobs = [("bair", lambda: reconstructor_ab("bair", 512, 64, args.iters, "fuse_norm", FUSED, precision, fuse_extras)),
                ("moving-gif", lambda: reconstructor_ab("moving-gif", 64, 64, args.iters, "fuse_norm", FUSED, precision, fuse_extras)),
                ("vox", lambda: reconstructor_ab("vox", 8, 256, max(2, args.iters // 2), "fuse_norm", FUSED, precision, fuse_extras)),
                ("frame-loop", lambda: frame_loop_ab("moving-gif", 64, 16, max(2, args.iters // 2), "MNK_EVAL_FUSE_NORM",
                                                     {"default": "0", "fused": "1"}, precision))]
        for name, job in jobs:
            if not only or name in only:
                print(json.dumps(job()), flush=True)
    sys.exit(0)

if args.precision_ab:
    only = set(filter(None, args.only.split(",")))
    forms = {"fp32": "fp32", "bf16": "bf16"}
    jobs = [("bair", lambda: reconstructor_ab("bair", 512, 64, args.iters, "precision", forms, extras=precision_extras)),
            ("moving-gif", lambda: reconstructor_ab("moving-gif", 64, 64, args.iters, "precision", forms, extras=precision_extras)),
            ("vox", lambda: reconstructor_ab("vox", 8, 256, max(2, args.iters // 2), "precision", forms, extras=precision_extras)),
            ("frame-loop", lambda: frame_loop_ab("moving-gif", 64, 16, max(2, args.iters // 2), "MNK_EVAL_PRECISION", forms))]
    for name, job in jobs:
        if not only or name in only:
            print(json.dumps(job()), flush=True)
    sys.exit(0)

gen, disc, kpd = bench.build_models(configs.get(args.config), dev)
src = torch.rand(args.batch, 3, 1, args.size, args.size, device=dev)
drv = torch.rand(args.batch, 3, 1, args.size, args.size, device=dev)
res = {}
for mode in ("eager", "graph"):
    r = engine.Reconstructor(kpd, gen, use_graph=(mode == "graph"))
    for _ in range(3):
        r(src, drv)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(args.iters):
        r(src, drv)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / args.iters
    res[mode] = {"ms_per_batch": round(dt * 1e3, 3), "frames_per_s": round(args.batch / dt, 1)}
print(json.dumps({"workload": "%s eval forward (kp x2 + generator), batch %d @ %dx%d" % (args.config, args.batch, args.size, args.size), **res}))
