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

  python tools/animate_bench.py [--reps 7] [--warmup 2] [--timeout 420] [--out profiles/animation_session.txt]"""
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


def child(name, reps, warmup):
    for p in (ROOT, os.path.join(ROOT, "monkey-net_amd")):
        sys.path.insert(0, p)
    import torch
    from mnk import configs, engine
    from modules.generator import MotionTransferGenerator
    from modules.keypoint_detector import KPDetector
    from sync_batchnorm import DataParallelWithCallback
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
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    if a.child:
        return child(a.child, a.reps, a.warmup)
    text = []
    for name in CASES:
        run = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name,
                              "--reps", str(a.reps), "--warmup", str(a.warmup)], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                             text=True)
        if run.returncode != 0:
            text.append("animate_bench: %s ended with status %d; nothing more is started" % (name, run.returncode))
            break
        rec = json.loads(run.stdout.strip().splitlines()[-1])
        text += [table(rec), json.dumps(rec), ""]
    out = "\n".join(text)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    if text and text[-1].startswith("animate_bench:"):
        sys.exit(text[-1])


if __name__ == "__main__":
    main()
