#!/usr/bin/env python
"""fp32 against opt-in bf16 training (mnk.engine.TrainStep(precision=...)): the whole train.py:110-136
iteration as a hipGraph replay, both precisions in the SAME process on two model triples built from the same seed.

Per configuration (moving-gif batch 32 @ 64, taichi batch 32 @ 64, vox batch 8 @ 256):
  * step time: 3 warm-up replays per form, then the two forms alternate `--reps` times, `--iters` replays per timing (host clock
    around work that ends in a device synchronise); median and spread (max - min) per form;
  * kernel groups: two profiled EAGER iterations per form under the library's per-launch event recorder (bench.prof_collect), no
    background weight-gradient launches -- ms per iteration of the forward / data-gradient GEMMs ("conv3x3_igemm"), the
    weight-gradient GEMMs ("conv3x3_wgrad") and the reductions / packs ("conv3x3_reduce_pack").
Every configuration runs in a child process of its own under a time limit; one JSON line per configuration, and with --out the
lines are also written to that file (profiles/bf16_training.txt is made this way)."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "monkey-net_amd"))

CONFIGS = {"moving-gif": ("moving-gif", 32, 64), "taichi": ("taichi", 32, 64), "vox256": ("vox", 8, 256)}
GROUPS = ("conv3x3_igemm", "conv3x3_wgrad", "conv3x3_reduce_pack")


def timed(step, x, iters):
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        step.step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def child(name, iters, reps):
    import torch
    import bench
    from mnk import configs, engine, workload, _lib
    cfg_name, batch, size = CONFIGS[name]
    dev = torch.device("cuda:0")
    cfg = configs.get(cfg_name)
    src, drv = workload.synthetic_pair(batch, size, size, seed=777)
    x = {"source": src.to(dev), "video": drv.to(dev)}
    forms = ("fp32", "bf16")
    steps, models = {}, {}
    for p in forms:
        models[p] = bench.build_models(cfg, dev)           # (seeded: the same weights for both forms)
        gen, disc, kpd = models[p]
        steps[p] = engine.TrainStep(gen, disc, kpd, cfg["train_params"], use_graph=True, precision=p)
        for _ in range(3):
            steps[p].step(x)
    times = {p: [] for p in forms}
    for _ in range(reps):
        for p in forms:
            times[p].append(timed(steps[p], x, iters))
    out = {"workload": "%s, batch %d @ %dx%d: full train.py:110-136 iteration, hipGraph replay" % (cfg_name, batch, size, size),
           "iters_per_timing": iters, "reps": reps}
    for p in forms:
        v = times[p]
        out[p] = {"ms": round(sorted(v)[len(v) // 2], 4), "spread_ms": round(max(v) - min(v), 4)}
    out["speedup"] = round(out["fp32"]["ms"] / out["bf16"]["ms"], 3)
    out["faster_by_more_than_the_spread"] = bool(out["fp32"]["ms"] - out["bf16"]["ms"] > max(out["fp32"]["spread_ms"], out["bf16"]["spread_ms"]))
    lib = _lib.lib()
    for p in forms:
        gen, disc, kpd = models[p]
        eager = engine.TrainStep(gen, disc, kpd, cfg["train_params"], use_graph=False, precision=p)
        for o in (eager.opt_g, eager.opt_d, eager.opt_k):
            if hasattr(o, "reducer"):
                o.reducer.bg_macs = 0.0                    # no weight-gradient GEMMs running under the kernels that are timed
        eager.step(x)
        k = bench.prof_collect(lib, lambda: eager.step(x), 2)
        out[p]["kernel_groups_ms"] = {g: round(k[g]["ms_per_step"], 4) for g in GROUPS if g in k}
        out[p]["kernel_groups_launches"] = {g: k[g]["launches_per_step"] for g in GROUPS if g in k}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="comma-separated subset of " + ",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per configuration (a child process of its own)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters, args.reps)
    only = set(filter(None, args.only.split(",")))
    lines = []
    for name in CONFIGS:
        if only and name not in only:
            continue
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", name,
               "--iters", str(args.iters if name != "vox256" else max(5, args.iters // 2)), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        got = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not got:
            # a fault, an abort or a time limit: nothing more is started on the device
            print("%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            if args.out and lines:
                open(args.out, "w").write("\n".join(lines) + "\n")
            return r.returncode or 1
        print(got[-1], flush=True)
        lines.append(got[-1])
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
