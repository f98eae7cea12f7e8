#!/usr/bin/env python
"""Per-layer micro-benchmark of the conv3x3 kernels (forward / dgrad / wgrad) on the layer shapes of one config.
Usage on the GPU box:  python tools/conv_bench.py --config taichi --batch 32 [--size 64]
--onepass: the forward launches only, at an inference batch, fp32 against the one-pass bf16 form (MNK_CONV_BF16) -- the two forms
alternate, `--reps` timings each, median and spread (max - min) per form; the exit status is 1 when a gated layer is not faster."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "monkey-net_amd"))
import torch  # noqa: E402

from mnk import configs, ops, _lib, workload  # noqa: E402


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


STATS = bool(int(os.environ.get('CB_STATS', '0')))


def discriminator_rows(cfg, args, dev):
    """the patch discriminator's four 4x4 / pad 0 convolutions (modules/discriminator.py) on the batched [generated | real]
    pass: forward and data gradient (a pad-3 correlation over dy) with the executed rate next to the algorithmic one -- the
    data gradients skip the K steps of taps that only read padding (tuning value ktap_skip; not part of the totals below)"""
    import ctypes
    dp, cp = cfg["model_params"]["discriminator_params"], cfg["model_params"]["common_params"]
    frames = 2 * args.batch
    from modules.discriminator import Discriminator
    blocks = [(b.in_features, b.out_features) for b in Discriminator(**dp, **cp).down_blocks]
    lib = _lib.lib()

    def executed(fn):
        lib.cdll.mnk_prof_reset()
        lib.cdll.mnk_prof_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.cdll.mnk_prof_enable(0)
        v = ctypes.c_double()
        lib.cdll.mnk_prof_query_executed(0, ctypes.byref(v))
        lib.cdll.mnk_prof_reset()
        return v.value

    print("%-16s %5s %5s %4s %7s | %8s %8s  (alg. TFLOP/s, ms) | executed: %6s %6s" % (
        "discriminator", "cin", "cout", "hi", "frames", "fwd", "dgrad", "fwd", "dgrad"))
    hi = args.size // dp.get("scale_factor", 1)
    for i, (c, cout) in enumerate(blocks):
        ho = hi - 3
        if ho < 1:
            break
        x = torch.randn(frames, hi, hi, ops.ceil4(c), device=dev)
        x[..., c:] = 0
        dy = torch.randn(frames, ho, ho, ops.ceil4(cout), device=dev)
        dy[..., cout:] = 0
        wt = torch.randn(cout, c, 1, 4, 4, device=dev) * 0.05
        wp = torch.empty(ops._query("mnk_conv2d_packed_floats", cout, c, 0, 16), device=dev)
        wd = torch.empty(ops._query("mnk_conv2d_packed_floats", c, cout, 0, 16), device=dev)
        ops._call("mnk_conv2d_pack_all", x, wt.data_ptr(), wp.data_ptr(), wd.data_ptr(), None, cout, c, 0, 16)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        nwf = ops._query("mnk_conv2d_workspace_floats", frames, ho, ho, c, 0, cout, 16)
        nwd = ops._query("mnk_conv2d_workspace_floats", frames, hi, hi, cout, 0, c, 16)
        ws = torch.empty(max(nwf, nwd, 1), device=dev)

        def fwd():
            ops._call("mnk_conv2d_fwd", x, x.data_ptr(), x.shape[-1], c, None, 0, 0, 2, hi, hi, 4, 4, 0, wp.data_ptr(), None, None, 0,
                      y.data_ptr(), y.shape[-1], frames, ho, ho, cout, ws.data_ptr(), nwf, None)

        def dgrad():
            ops._call("mnk_conv2d_fwd", dy, dy.data_ptr(), dy.shape[-1], cout, None, 0, 0, 2, ho, ho, 4, 4, 3, wd.data_ptr(), None, None,
                      0, dx.data_ptr(), dx.shape[-1], frames, hi, hi, c, ws.data_ptr(), nwd, None)

        fl = 2.0 * 16 * c * cout * ho * ho * frames
        t_f, t_d = timeit(fwd, args.iters), timeit(dgrad, args.iters)
        print("%-16s %5d %5d %4d %7d | %5.1f %5.3f  %5.1f %5.3f | %15.1f %6.1f" % (
            "disc.block%d" % i, c, cout, hi, frames, fl / t_f / 1e12, t_f * 1e3, fl / t_d / 1e12, t_d * 1e3,
            executed(fwd) / t_f / 1e12, executed(dgrad) / t_d / 1e12))
        hi = ho // 2


def onepass_rows(cfg, args, dev):
    """every distinct 3x3 forward launch of mnk.engine.Reconstructor at batch `args.batch` (the key-point detector sees source
    and driving frames in one call: 2 x batch frames; the generator sees batch): fp32 and one-pass bf16 timed alternately.
    GATE rows: M >= 8192 pixel rows and Cin >= 64 -- the one-pass form must be faster by more than three times the larger of
    the two spreads.  Layers ops._conv_launch keeps fp32 inside the scope (ops.bf16_excluded) are marked and not gated.
    Returns the number of gated layers that are not faster."""
    layers = workload.conv_flops_hot_path(cfg, args.size, args.size)["layers"]
    print("one-pass bf16 against fp32, %s batch %d @ %d: median ms of %d x %d launches, (spread = max - min)" % (
        args.config, args.batch, args.size, args.reps, args.iters))
    print("%-16s %5s %5s %4s %8s | %9s %9s | %9s %9s | %6s  %s" % ("layer", "cin", "cout", "hw", "M", "fp32 ms", "spread", "bf16 ms",
                                                                  "spread", "x", "gate (M >= 8192, cin >= 64)"))
    seen, tot, failed = set(), [0.0, 0.0], 0
    for name, cin, cout, h, w, k, flops in layers:
        ups = ".dec" in name
        frames = args.batch * (2 if name.startswith("kp") else 1)
        key = (cin, cout, h, w, frames, ups)
        if k != 3 or key in seen:
            continue
        seen.add(key)
        hs, ws_ = (h // 2, w // 2) if ups else (h, w)
        x = torch.randn(frames, hs, ws_, ops.ceil4(cin), device=dev)
        x[..., cin:] = 0
        wt = torch.randn(cout, cin, 1, 3, 3, device=dev) * 0.05
        bias = torch.randn(cout, device=dev)
        up = ops.subpixel(ups)
        wp = ops._packed_fwd_weight(wt, cout, cin, 0, up)

        def run(precision):
            with ops.inference_precision(precision):
                ops._conv_launch(x, cin, None, 0, ups, wp, bias, None, frames, h, w, cout, False, up)

        times = {"fp32": [], "bf16": []}
        for _ in range(args.reps):
            for precision in ("fp32", "bf16"):
                times[precision].append(timeit(lambda: run(precision), args.iters) * 1e3)
        med = {p: sorted(v)[len(v) // 2] for p, v in times.items()}
        spread = {p: max(v) - min(v) for p, v in times.items()}
        m = frames * h * w
        excluded = ops.bf16_excluded(cin, cout)       # ops._conv_launch keeps these heads fp32: both columns time the fp32 form
        gated = m >= 8192 and cin >= 64 and not excluded
        ok = med["fp32"] - med["bf16"] > 3.0 * max(spread.values())
        failed += gated and not ok
        tot[0] += med["fp32"]
        tot[1] += med["bf16"]
        print("%-16s %5d %5d %4d %8d | %9.4f %9.4f | %9.4f %9.4f | %6.2f  %s" % (
            name, cin, cout, h, m, med["fp32"], spread["fp32"], med["bf16"], spread["bf16"], med["fp32"] / med["bf16"],
            "excluded: fp32 in both columns" if excluded else ("PASS" if ok else "FAIL") if gated else ("-" if ok else "- (not faster)")))
    print("TOTAL fwd fp32 %.3f ms, one-pass bf16 %.3f ms (%.2f x); gated layers that are not faster: %d" % (
        tot[0], tot[1], tot[0] / tot[1], failed))
    return failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="taichi")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--onepass", action="store_true", help="forward only: fp32 against the one-pass bf16 form, alternating")
    ap.add_argument("--reps", type=int, default=5, help="--onepass: timings per form")
    args = ap.parse_args()
    cfg = configs.get(args.config)
    if args.onepass:
        with torch.no_grad():
            failed = onepass_rows(cfg, args, torch.device("cuda:0"))
        sys.exit(1 if failed else 0)
    layers = workload.conv_flops_hot_path(cfg, args.size, args.size)["layers"]
    dev = torch.device("cuda:0")
    tot = {"fwd": [0.0, 0.0, 0.0], "dgrad": [0.0, 0.0, 0.0], "wgrad": [0.0, 0.0, 0.0]}
    print("algorithmic TFLOP/s (the reference's 3x3 convolution, whatever form computes it) | executed TFLOP/s (multiply-adds issued:\n"
          "the sub-pixel forms of the up-sampled layers run 4/9 of them) -- the executed column is what the 157.3 TFLOP/s pipe does")
    print("%-16s %5s %5s %4s %7s | %8s %8s %8s  (alg. TFLOP/s, ms) | executed: %6s %6s %6s" % (
        "layer", "cin", "cout", "hw", "frames", "fwd", "dgrad", "wgrad", "fwd", "dgrad", "wgrad"))
    seen = {}
    for name, cin, cout, h, w, k, flops in layers:
        if k != 3:
            continue
        frames = args.batch * (2 if name.startswith("kp") else 1)
        ups = ".dec" in name
        key = (cin, cout, h, w, frames, ups)
        if key not in seen:
            hs, ws_ = (h // 2, w // 2) if ups else (h, w)
            x = torch.randn(frames, hs, ws_, ops.ceil4(cin), device=dev)
            wt = torch.randn(cout, cin, 1, 3, 3, device=dev) * 0.05
            bias = torch.randn(cout, device=dev)
            dy = torch.randn(frames, h, w, ops.ceil4(cout), device=dev)
            fl = 2.0 * 9 * cin * cout * h * w * frames
            up = ops.subpixel(ups)          # UpBlock3D layers: the sub-pixel forms (MNK_UP_SUBPIXEL=0: the up-sampled view)
            wp = ops._packed_fwd_weight(wt, cout, cin, 0, up)
            t_f = timeit(lambda: ops._conv_launch(x, cin, None, 0, ups, wp, bias, None, frames, h, w, cout, STATS, up), args.iters)
            if up:
                wpd = torch.empty(ops._query("mnk_conv3x3_up_dgrad_packed_floats", cout, cin), device=dev)
                ops._call("mnk_conv3x3_up_pack_dgrad", dy, wt.data_ptr(), wpd.data_ptr(), cout, cin, 0, cin)
                dxl = torch.empty(frames, hs, ws_, ops.ceil4(cin), device=dev)
                nwd = ops._query("mnk_conv3x3_up_dgrad_workspace_floats", frames, hs, ws_, cout, cin)
                wsd = torch.empty(max(nwd, 1), device=dev)
                t_d = timeit(lambda: ops._call("mnk_conv3x3_up_dgrad", dy, dy.data_ptr(), dy.shape[-1], cout, wpd.data_ptr(),
                                               dxl.data_ptr(), dxl.shape[-1], frames, hs, ws_, cin, wsd.data_ptr(), nwd), args.iters)
            else:
                npk = ops._query("mnk_conv3x3_packed_floats", cin, cout, 0)
                wpd = torch.empty(npk, device=dev)
                ops._call("mnk_conv3x3_pack_dgrad", dy, wt.data_ptr(), wpd.data_ptr(), cout, cin, 0, cin)
                t_d = timeit(lambda: ops._conv_launch(dy, cout, None, 0, 0, wpd, None, None, frames, h, w, cin), args.iters)
            dw = torch.empty_like(wt)
            nws = ops._query("mnk_conv3x3_up_wgrad_workspace_floats" if ups else "mnk_conv3x3_wgrad_workspace_floats", frames, h, w,
                             cin, cout)
            ws = torch.empty(max(nws, 1), device=dev)

            def wg():
                ops._call("mnk_conv3x3_wgrad", dy, x.data_ptr(), x.shape[-1], cin, int(ups) | 2, dy.data_ptr(), dy.shape[-1], cout,
                          dw.data_ptr(), cin, 0, frames, h, w, ws.data_ptr(), nws)
            t_w = timeit(wg, args.iters)
            seen[key] = (fl, t_f, t_d, t_w, fl * (4.0 / 9.0 if up else 1.0))
        fl, t_f, t_d, t_w, ex = seen[key]
        print("%-16s %5d %5d %4d %7d | %5.1f %5.2f  %5.1f %5.2f  %5.1f %5.2f | %15.1f %6.1f %6.1f" % (
            name, cin, cout, h, frames, fl / t_f / 1e12, t_f * 1e3, fl / t_d / 1e12, t_d * 1e3, fl / t_w / 1e12, t_w * 1e3,
            ex / t_f / 1e12, ex / t_d / 1e12, ex / t_w / 1e12))
        for kk, t in (("fwd", t_f), ("dgrad", t_d), ("wgrad", t_w)):
            tot[kk][0] += fl
            tot[kk][1] += t
            tot[kk][2] += ex
    discriminator_rows(cfg, args, dev)
    for kk, (fl, t, ex) in tot.items():
        print("TOTAL %-6s %.1f GFLOP in %.2f ms = %.1f TFLOP/s (%.1f%% of 157.3) algorithmic; executed %.1f GFLOP = %.1f TFLOP/s "
              "(%.1f%% of 157.3)" % (kk, fl / 1e9, t * 1e3, fl / t / 1e12, fl / t / 1e12 / 157.3 * 100, ex / 1e9, ex / t / 1e12,
                                     ex / t / 1e12 / 157.3 * 100))


if __name__ == "__main__":
    main()
