#!/usr/bin/env python
"""Per-layer table of the weight-streaming ("skinny") 3x3 convolutions against today's launch plans, on the batch-1 layer shapes
of the per-frame evaluation loop: every distinct 3x3 conv -> norm layer of moving-gif, taichi (64 x 64) and vox (256 x 256) with
at most 64 output rows.  Per layer and precision (fp32, bf16) two forms alternate, `--reps` timings of `--iters` cold launches each
(a cache-sized buffer is rewritten before every timed launch, as tools/plan_tune.py does):

  skinny   mnk_conv3x3_skinny_fwd + mnk_bn_eval_split_fwd
  today    the plan ops._conv_launch takes (sub-pixel packs for up-sampled layers, deferred split-K) + the same second stage
           (mnk_bn_eval_split_fwd behind a split launch, mnk_bn_act_fwd behind an unsplit one)

median and spread (max - min) in microseconds, and the weight bytes each form reads over its time.  The last lines name, per
precision, the largest row count R such that the skinny form is faster than today's by more than the larger spread on EVERY
measured shape with at most R rows that the library's class rule takes (up-sampled layers with short weight streams are excluded:
"skinny_up_min_weights"; the table times them all the same and marks them): the `skinny_rows` default (0: faster nowhere).
Usage on the GPU box:  python tools/skinny_bench.py [--configs moving-gif,taichi,vox] [--reps 5] [--iters 20]
                       [--precisions fp32,bf16] [--tuning skinny_blocks=256,skinny_min_k=256]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "monkey-net_amd"))
import torch  # noqa: E402

from mnk import configs, ops, _lib, workload  # noqa: E402

SIZES = {"vox": 256}


def time_cold(fn, iters, flush):
    fn()
    evs = []
    for _ in range(iters):
        flush.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / iters * 1e3          # microseconds


def shapes(names):
    """distinct (cin, cout, h, w, ups, pool) with h * w <= 64, even maps, of the 3x3 conv -> norm layers at batch 1"""
    out = {}
    for cfg_name in names:
        size = SIZES.get(cfg_name, 64)
        for name, cin, cout, h, w, k, _ in workload.conv_flops_hot_path(configs.get(cfg_name), size, size)["layers"]:
            if k != 3 or name.endswith(".last") or ".ref" in name or h * w > 64 or h % 2 or w % 2:
                continue
            key = (cin, cout, h, w, ".dec" in name, ".enc" in name or ".app" in name)
            out.setdefault(key, []).append("%s:%s" % (cfg_name, name))
    return sorted(out.items(), key=lambda kv: (kv[0][2] * kv[0][3], kv[0][0] * kv[0][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="moving-gif,taichi,vox")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--tuning", default="", help="name=value,name=value set through mnk_set_tuning first (skinny_blocks, skinny_min_k)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    import ctypes
    rows_default = ctypes.c_int(0)
    lib.call("mnk_get_tuning", b"skinny_rows", ctypes.byref(rows_default))
    rows_default = rows_default.value
    lib.call("mnk_set_tuning", b"skinny_rows", 64)
    for kv in filter(None, args.tuning.split(",")):
        name, value = kv.split("=")
        lib.call("mnk_set_tuning", name.encode(), int(value))
    if args.tuning:
        print("# tuning: " + args.tuning)
    up_default = ctypes.c_int(0)
    lib.call("mnk_get_tuning", b"skinny_up_min_weights", ctypes.byref(up_default))
    up_default = up_default.value
    lib.call("mnk_set_tuning", b"skinny_up_min_weights", 0)             # time every shape; the library's own rule is the last column
    print("# library defaults: skinny_rows %d, skinny_up_min_weights %d; last column = what the library does with the shape" % (
        rows_default, up_default))
    flush = torch.empty(320 << 20, dtype=torch.uint8, device=dev)       # larger than the 256 MiB Infinity Cache
    verdict = {}
    with torch.no_grad():
        for precision in args.precisions.split(","):
            print("== %s: cold launches, median of %d x %d (spread = max - min), microseconds; GB/s = weight bytes of the form / time"
                  % (precision, args.reps, args.iters))
            print("%5s %5s %3s %3s %4s | %9s %7s %7s %4s | %9s %7s %7s %4s | %6s  %s" % (
                "cin", "cout", "h", "R", "kind", "skinny us", "spread", "GB/s", "spl", "today us", "spread", "GB/s", "spl", "x", "layers"))
            for (cin, cout, h, w, ups, pool), names in shapes(args.configs.split(",")):
                hs, ws_ = (h // 2, w // 2) if ups else (h, w)
                x = torch.randn(1, hs, ws_, ops.ceil4(cin), device=dev)
                x[..., cin:] = 0
                wt = torch.randn(cout, cin, 1, 3, 3, device=dev) * 0.05
                bias = torch.randn(cout, device=dev)
                mean, scale, beta = (torch.randn(cout, device=dev) for _ in range(3))
                ld = ops.ceil4(cout)
                z = torch.empty(1, h // 2 if pool else h, w // 2 if pool else w, ld, device=dev)
                bf = precision == "bf16" and not ops.bf16_excluded(cin, cout)
                flags = int(ups) | 2 | (8 if bf else 0)
                # skinny
                wps = ops._packed_skinny_weight(wt, cout, cin, 0, bf)
                size = (1, h, w, cin, 0, cout)
                nws, spl_s = ops._query("mnk_conv3x3_skinny_workspace_floats", *size), ops._query("mnk_conv3x3_skinny_splits", *size)
                wss = torch.empty(nws, device=dev)

                def skinny():
                    ops._call("mnk_conv3x3_skinny_fwd", x, x.data_ptr(), x.shape[-1], cin, None, 0, 0, flags, wps.data_ptr(), 1, h, w,
                              cout, wss.data_ptr(), nws)
                    ops._call("mnk_bn_eval_split_fwd", x, wss.data_ptr(), spl_s, ld, 1, bias.data_ptr(), mean.data_ptr(), scale.data_ptr(),
                              beta.data_ptr(), z.data_ptr(), ld, 1, h, w, cout, 1, int(pool))

                # today
                up = ops.subpixel(ups)
                wpt = ops._packed_fwd_weight(wt, cout, cin, 0, up)
                plan = {}

                def today():
                    with ops.inference_precision(precision):
                        y, _ = ops._conv_launch(x, cin, None, 0, ups, wpt, bias, None, 1, h, w, cout, False, up, eval_defer=True)
                    pend = ops._SPLIT_PENDING.pop(y.data_ptr(), None)
                    plan["splits"] = pend.splits if pend is not None else 1
                    if pend is not None:
                        ops._call("mnk_bn_eval_split_fwd", x, pend.ws.data_ptr(), pend.splits, ld, pend.phases, bias.data_ptr(),
                                  mean.data_ptr(), scale.data_ptr(), beta.data_ptr(), z.data_ptr(), ld, 1, h, w, cout, 1, int(pool))
                    else:
                        ops._call("mnk_bn_act_fwd", x, y.data_ptr(), ld, mean.data_ptr(), scale.data_ptr(), beta.data_ptr(), z.data_ptr(),
                                  ld, 0, 1, h, w, cout, 1, int(pool))

                skinny(), today()
                zs = z.clone()
                skinny()
                torch.cuda.synchronize()
                diff = float((z - zs).abs().max() / zs.abs().max().clamp_min(1e-30))       # today's z against the skinny z
                times = {"skinny": [], "today": []}
                for _ in range(args.reps):
                    for k, fn in (("skinny", skinny), ("today", today)):
                        times[k].append(time_cold(fn, args.iters, flush))
                med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
                spread = {k: max(v) - min(v) for k, v in times.items()}
                bytes_s = wps.numel() * 4
                bytes_t = wpt.numel() * 4
                faster = med["today"] - med["skinny"] > max(spread.values())
                lib.call("mnk_set_tuning", b"skinny_up_min_weights", up_default)
                in_class = bool(ops._query("mnk_conv3x3_skinny_form", 1, h, w, cin, 0, cout, flags, int(pool)))
                lib.call("mnk_set_tuning", b"skinny_up_min_weights", 0)
                taken = "taken" if in_class and h * w <= rows_default else ("rows > %d" % rows_default if in_class else "excluded class")
                if in_class:
                    verdict.setdefault(precision, []).append((h * w, faster))
                print("%5d %5d %3d %3d %4s | %9.2f %7.2f %7.0f %4d | %9.2f %7.2f %7.0f %4d | %6.2f  %s%s  [rel. diff %.1e]" % (
                    cin, cout, h, h * w, "up" if ups else ("pool" if pool else "-"), med["skinny"], spread["skinny"],
                    bytes_s / med["skinny"] / 1e3, spl_s, med["today"], spread["today"], bytes_t / med["today"] / 1e3, plan["splits"],
                    med["today"] / med["skinny"], ",".join(names), "" if faster else "  (NOT faster by more than the spread)", diff) + "  " + taken,
                    flush=True)
    for precision, rows in verdict.items():
        best = 0
        for r in sorted({r for r, _ in rows}):
            if all(f for rr, f in rows if rr <= r):
                best = r
            else:
                break
        print("skinny_rows by the rule, %s: %d   (rows measured: %s)" % (precision, best, sorted({r for r, _ in rows})))


if __name__ == "__main__":
    main()
