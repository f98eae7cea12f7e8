#!/usr/bin/env python
"""Time the ways of animating ONE source image from a 64-frame driving video on the GPU box (eval mode, batch 1, seeded weights and
inputs), for the moving-gif (64 x 64) and vox (256 x 256) models of mnk.configs:

  (a) loop      the reference's per-frame loop (transfer.py:65-79) on the drop-in modules behind DataParallelWithCallback, served
                by mnk.dropin.EvalRunner: detector per frame, normalize_kp on the whole video, generator per frame;
  (b) transfer  mnk.engine.Transfer(shared_source=True) on the whole video;
  (c) session   mnk.engine.AnimationSession, pushes of n = 1, 8, 64 frames, eager and captured: set_source + 64 / n pushes
                (`total`), and the pushes alone from a fresh anchor (`pushes`).

Each video is timed between two HIP events after warm-up; median and minimum over the repetitions, frames per second from the
median.  For (b) and (c) the peak of torch's allocated memory over one video is read after a reset -- for a session over a NEW
session's first video (set_source, captures, pushes), so the buffers a captured program keeps are counted.  Each configuration
runs in a fresh process under `timeout -k 10`; one that fails ends the run.  The output is a table and one JSON line per configuration.

  python tools/animate_bench.py [--reps 7] [--warmup 2] [--timeout 420] [--out profiles/animation_session.txt]

--u8: host uint8 frame in -> host uint8 frame out (what demo.py:60-71 does around the networks), per video, two ways on one build:

  fp32   numpy img_as_float32 arithmetic (uint8 * float32(1 / 255)) + transpose + H2D of the fp32 (1, 3, n, H, W) tensor, the push,
         D2H of the fp32 prediction, numpy transpose + `(255 * x).astype(np.uint8)`;
  uint8  H2D of the uint8 (1, n, H, W, 3) bytes, the push of a session with output="uint8", D2H of the uint8 prediction.

Pushes of n = 1, 8, 64 frames, eager and captured; the source is set before the clock starts.  `host ms` is the wall clock of one
video (64 frames), first byte in to last byte out; `device ms / push` is the time between two HIP events around each push, mean
over the video's pushes.  The two ways alternate video by video; median, minimum and spread (max - min) over the repetitions.
The bytes of the two ways are compared before anything is timed.

  python tools/animate_bench.py --u8 [--reps 7] [--warmup 2] [--out profiles/animation_session_u8.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"moving-gif": 64, "vox": 256}
FRAMES, BATCH = 64, 1
CHUNKS = (1, 8, 64)
PARAMS = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)


def models_and_inputs(name):
    """-> (generator, detector, source (1, 3, 1, H, W), driving (1, 3, 64, H, W)) on cuda:0: seeded weights and inputs"""
    for p in (ROOT, os.path.join(ROOT, "monkey-net_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from mnk import configs
    from modules.generator import MotionTransferGenerator
    from modules.keypoint_detector import KPDetector
    from oracle import cases
    assert torch.cuda.is_available(), "animate_bench needs the GPU: a CPU timing says nothing about it"
    dev = torch.device("cuda:0")
    size = CASES[name]
    mp = configs.get(name)["model_params"]
    torch.manual_seed(0)
    gen = MotionTransferGenerator(**mp["generator_params"], **mp["common_params"])
    kpd = KPDetector(**mp["kp_detector_params"], **mp["common_params"])
    for i, m in enumerate((gen, kpd)):
        sd = m.state_dict()
        cases.perturb_state_dict(sd, 7 + i)
        m.load_state_dict(sd)
    gen.to(dev).eval(), kpd.to(dev).eval()
    src = cases.smooth_pair(BATCH, size, size, seed=11)[0].to(dev)
    # eight distinct frames, repeated: the timing does not depend on the content
    eight = torch.cat([cases.smooth_pair(BATCH, size, size, seed=20 + i)[1] for i in range(8)], dim=2)
    driving = eight.repeat(1, 1, FRAMES // 8, 1, 1).contiguous().to(dev)
    return gen, kpd, src, driving


def child_u8(name, reps, warmup):
    gen, kpd, src, driving = models_and_inputs(name)
    import time
    import numpy as np
    import torch
    from mnk import engine
    size = CASES[name]
    to_bytes = lambda t: (t.cpu() * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous().numpy()
    src8, frames8 = to_bytes(src), to_bytes(driving)[0]             # (1, 1, H, W, 3), (64, H, W, 3): what a decoder hands over
    k255 = np.float32(1.0 / 255.0)
    # the fp32 way's source: img_as_float32 of the same source bytes, so that the two ways compute the same frames
    srcq = torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.multiply(src8[0], k255, dtype=np.float32), 3, 0)[np.newaxis])).cuda()
    rec = {"config": name, "size": size, "frames": FRAMES, "batch": BATCH, "reps": reps, "warmup": warmup, "mode": "u8", "rows": {}}

    def video_fp32(s, n, keep=None):
        """-> (host seconds, device ms per push)"""
        dev_ms, t0 = 0.0, time.perf_counter()
        for i in range(0, FRAMES, n):
            x = np.multiply(frames8[i:i + n], k255, dtype=np.float32)                        # img_as_float32
            x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 3, 0)[np.newaxis])).cuda()   # (1, 3, n, H, W), H2D
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = s.push(x)
            e1.record()
            y = out["video_prediction"].cpu().numpy()                                        # D2H (synchronises)
            y8 = (255 * np.transpose(y, [0, 2, 3, 4, 1])[0]).astype(np.uint8)                # demo.py:69-71
            dev_ms += e0.elapsed_time(e1)
            if keep is not None:
                keep.append(y8)
        return time.perf_counter() - t0, dev_ms / (FRAMES // n)

    def video_u8(s, n, keep=None):
        dev_ms, t0 = 0.0, time.perf_counter()
        for i in range(0, FRAMES, n):
            x = torch.from_numpy(frames8[i:i + n][np.newaxis]).cuda()                        # (1, n, H, W, 3) bytes, H2D
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = s.push(x)
            e1.record()
            y8 = out["video_prediction"].cpu().numpy()[0]                                    # D2H (synchronises)
            dev_ms += e0.elapsed_time(e1)
            if keep is not None:
                keep.append(y8)
        return time.perf_counter() - t0, dev_ms / (FRAMES // n)

    for n in CHUNKS:
        for captured in (False, True):
            sf = engine.AnimationSession(kpd, gen, PARAMS, use_graph=captured)
            s8 = engine.AnimationSession(kpd, gen, PARAMS, use_graph=captured, output="uint8")
            sf.set_source(srcq)
            s8.set_source(torch.from_numpy(src8))
            a, b = [], []                                            # (these two videos also capture the programs)
            video_fp32(sf, n, a)
            video_u8(s8, n, b)
            diff = max(int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max()) for x, y in zip(a, b))
            assert diff == 0, "n=%d %s: the uint8 way's bytes differ from the fp32 way's by %d: no timing" % (n, captured, diff)
            del a, b
            times = {"fp32": [], "uint8": []}
            for i in range(warmup + reps):
                for way, fn, s in (("fp32", video_fp32, sf), ("uint8", video_u8, s8)):
                    s.reset()
                    torch.cuda.synchronize()
                    t = fn(s, n)
                    if i >= warmup:
                        times[way].append(t)
            key = "n=%d %s" % (n, "captured" if captured else "eager")
            for way, ts in times.items():
                host, devp = [1e3 * t[0] for t in ts], [t[1] for t in ts]
                rec["rows"]["%s %s" % (key, way)] = {
                    "host_ms_median": round(statistics.median(host), 3), "host_ms_min": round(min(host), 3),
                    "host_ms_spread": round(max(host) - min(host), 3),
                    "device_ms_per_push_median": round(statistics.median(devp), 4), "device_ms_per_push_min": round(min(devp), 4),
                    "device_ms_per_push_spread": round(max(devp) - min(devp), 4), "pushes": FRAMES // n, "max_byte_diff": diff}
            del sf, s8
            torch.cuda.empty_cache()
    print(json.dumps(rec))


def table_u8(rec):
    lines = ["%s %dx%d, batch %d, %d driving frames per video, host uint8 frames in -> host uint8 frames out; median / min / spread "
             "(max - min) over %d videos after %d warm-up, the two ways alternating"
             % (rec["config"], rec["size"], rec["size"], rec["batch"], rec["frames"], rec["reps"], rec["warmup"]),
             "  %-24s %34s   %40s" % ("", "host ms / video (wall clock)", "device ms / push (HIP events)"),
             "  %-24s %12s %10s %10s   %14s %12s %12s" % ("form", "median", "min", "spread", "median", "min", "spread")]
    for key, r in rec["rows"].items():
        lines.append("  %-24s %12.3f %10.3f %10.3f   %14.4f %12.4f %12.4f" % (
            key, r["host_ms_median"], r["host_ms_min"], r["host_ms_spread"], r["device_ms_per_push_median"],
            r["device_ms_per_push_min"], r["device_ms_per_push_spread"]))
    return "\n".join(lines)


def child(name, reps, warmup):
    gen, kpd, src, driving = models_and_inputs(name)
    import torch
    from mnk import engine
    from sync_batchnorm import DataParallelWithCallback
    size = CASES[name]

    wrapped_gen, wrapped_kpd = DataParallelWithCallback(gen), DataParallelWithCallback(kpd)
    wrapped_gen.eval(), wrapped_kpd.eval()

    def loop():
        with torch.no_grad():
            kp_source = wrapped_kpd(src)
            kps = [wrapped_kpd(driving[:, :, i:i + 1]) for i in range(FRAMES)]
            kp_driving = {k: torch.cat([kp[k] for kp in kps], dim=1) for k in kps[0]}
            kp_norm = engine.normalize_kp(kp_driving, kp_source, **PARAMS)
            out = [wrapped_gen(source_image=src, kp_driving={k: v[:, i:i + 1] for k, v in kp_norm.items()},
                               kp_source=kp_source)["video_prediction"] for i in range(FRAMES)]
        return out[-1]

    transfer = engine.Transfer(kpd, gen, PARAMS, shared_source=True)
    runs = {"loop": loop, "transfer": lambda: transfer(src, driving)["video_prediction"]}
    sessions = {}
    for n in CHUNKS:
        for captured in (False, True):
            s = engine.AnimationSession(kpd, gen, PARAMS, use_graph=captured)
            key = "session n=%d %s" % (n, "captured" if captured else "eager")
            sessions[key] = (s, n)

            def total(s=s, n=n):
                s.set_source(src)
                for i in range(0, FRAMES, n):
                    out = s.push(driving[:, :, i:i + n])
                return out["video_prediction"]

            def pushes(s=s, n=n):
                s.reset()
                for i in range(0, FRAMES, n):
                    out = s.push(driving[:, :, i:i + n])
                return out["video_prediction"]
            runs[key + " total"] = total
            runs[key + " pushes"] = pushes

    # the last frame of every form against Transfer's: a form that computes something else is not timed
    want = transfer(src, driving)["video_prediction"][:, :, -1:].clone()
    rec = {"config": name, "size": size, "frames": FRAMES, "batch": BATCH, "reps": reps, "warmup": warmup, "rows": {}}
    for key, fn in runs.items():
        got = fn()[:, :, -1:]
        torch.cuda.synchronize()
        err = float((got - want).abs().max())
        assert err < 1e-4, "%s differs from Transfer by %.3e: no timing" % (key, err)
        times = []
        for i in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
        row = {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
               "frames_per_s": round(FRAMES * 1000.0 / statistics.median(times), 1), "max_abs_diff_last_frame": err}
        if key == "transfer" or key.endswith(" total"):
            # a session is measured from its construction: a captured program's buffers are allocated at capture and kept
            fresh = fn
            if key != "transfer":
                s, n = sessions[key[:-len(" total")]]
                new = engine.AnimationSession(kpd, gen, PARAMS, use_graph=s.use_graph)

                def fresh(new=new, n=n):
                    new.set_source(src)
                    for i in range(0, FRAMES, n):
                        new.push(driving[:, :, i:i + n])      # (nothing is kept: one push's results are alive at a time)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fresh()
            torch.cuda.synchronize()
            row["peak_allocated_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
            del out, fresh
        rec["rows"][key] = row
    print(json.dumps(rec))


def table(rec):
    lines = ["%s %dx%d, batch %d, %d driving frames, eval mode; median / min over %d videos after %d warm-up (HIP events)"
             % (rec["config"], rec["size"], rec["size"], rec["batch"], rec["frames"], rec["reps"], rec["warmup"]),
             "  %-34s %12s %10s %10s %12s" % ("form", "ms / video", "min", "frames/s", "peak MiB")]
    for key, r in rec["rows"].items():
        lines.append("  %-34s %12.3f %10.3f %10.1f %12s" % (key, r["ms_median"], r["ms_min"], r["frames_per_s"],
                                                            r.get("peak_allocated_mib", "-")))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per configuration")
    ap.add_argument("--out", default=None, help="also write the output to this file")
    ap.add_argument("--child", choices=sorted(CASES))
    ap.add_argument("--u8", action="store_true", help="time host uint8 frames in -> host uint8 frames out, fp32 way against uint8 way")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    if a.child:
        return (child_u8 if a.u8 else child)(a.child, a.reps, a.warmup)
    text = []
    for name in CASES:
        run = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name,
                              "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--u8"] if a.u8 else []), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                             text=True)
        if run.returncode != 0:
            text.append("animate_bench: %s ended with status %d; nothing more is started" % (name, run.returncode))
            break
        rec = json.loads(run.stdout.strip().splitlines()[-1])
        text += [(table_u8 if a.u8 else table)(rec), json.dumps(rec), ""]
    out = "\n".join(text)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    if text and text[-1].startswith("animate_bench:"):
        sys.exit(text[-1])


if __name__ == "__main__":
    main()
