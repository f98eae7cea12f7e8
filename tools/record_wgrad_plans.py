#!/usr/bin/env python
"""Record what the weight-gradient planners decide for a sweep of jobs: tests/golden/wgrad_plans.npz, the fixture of
tests/test_wgrad_plans.py.  The planners are host code, so the CPU emulator build of the library answers (no GPU needed).

A row is a job (N, Ho, Wo, Hi, Wi, C, Cout, kh, kw, pad, ld_x, ld_dy, flags), the `up_subpixel` tuning value it was planned
under, and the answers of mnk_conv2d_wgrad_plan2 (layout, splits, part_floats) and mnk_wgrad_grouped_plan (variant, splits,
part_floats) under otherwise default tuning.  Re-record ONLY when a plan rule or a tuning default is changed on purpose; the diff
of the fixture's summary (printed here) is then what a reviewer looks at.

Usage: tools/record_wgrad_plans.py [--library libmnk_emu.so] [--out tests/golden/wgrad_plans.npz]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monkey-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

COLUMNS = ("N", "Ho", "Wo", "Hi", "Wi", "C", "Cout", "kh", "kw", "pad", "ld_x", "ld_dy", "flags", "up_subpixel",
           "plan_layout", "plan_splits", "plan_part_floats", "grouped_variant", "grouped_splits", "grouped_part_floats")
N_IN = 14
UPSAMPLED, CLEAN_PADS = 1, 2
# The LDS-halo and the gather form both leave layout 1 and the grouped launch takes neither: the answers cannot tell them apart.
# One shape of each by the rules (csrc/conv3x3_wgrad.hip), (N, H, W, C, Cout) -- both narrower than a 64-wide tile (not
# tap-major) and not on 8-aligned maps (not nine-tap); the first fills its 64 x 64 slab on 32-pixel rows, the second has 10-pixel
# rows (the halo form needs 16) -- and one of the nine-tap form.  Their results: tests/test_kernels_conv.py's HALO_CASES.
KNOWN_FORMS = {"halo": (4, 20, 32, 64, 64), "gather": (8, 12, 10, 20, 45), "nine-tap": (2, 64, 64, 40, 60)}


def _up(v, m):
    return (v + m - 1) // m * m


def _lds(c):
    odd = c + 1 if (c + 1) % 4 else c + 2            # one row stride that is not a multiple of 4
    return sorted({_up(c, 4), _up(c, 16), odd})


def _job(n, ho, wo, c, cout, flags, ld_x, k=3, pad=1, subpixel=1):
    return (n, ho, wo, ho - 2 * pad + k - 1, wo - 2 * pad + k - 1, c, cout, k, k, pad, ld_x, _up(cout, 4), flags, subpixel)


def sweep():
    from mnk import configs, workload
    import test_kernels_conv as kc
    rows = []

    def conv3(n, h, w, c, cout, up):
        for ld_x in _lds(c):
            for flags in (0, CLEAN_PADS) + ((UPSAMPLED, UPSAMPLED | CLEAN_PADS) if up and h % 2 == 0 and w % 2 == 0 else ()):
                rows.append(_job(n, h, w, c, cout, flags, ld_x))

    # every convolution of the hot path for the benchmark's configurations and batch sizes, at b and 2 b frames (the key-point
    # detector sees both frames of a pair); decoder layers read two sources (the skip connection): whole and per source
    for name, size, batch in (("moving-gif", 64, 32), ("taichi", 64, 32), ("vox", 256, 8), ("bair", 64, 512)):
        for lname, cin, cout, h, w, k, _ in workload.conv_flops_hot_path(configs.get(name), size, size)["layers"]:
            if k != 3:
                continue
            up = ".dec" in lname
            for c in sorted({cin, cin // 2, cin - cin // 2} if up else {cin}):
                for n in (batch, 2 * batch):
                    conv3(n, h, w, c, cout, up)
    # the discriminator's 4x4 / pad 0 ladder (modules/discriminator.py: 3 + kp channels -> 64 -> 128 -> 256 -> 512, halved maps)
    for size, batch in ((64, 32), (256, 8)):
        hi, cin = size, 13
        for cout in (64, 128, 256, 512):
            if hi < 4:
                break
            for ld_x in _lds(cin):
                for flags in (0, CLEAN_PADS):
                    rows.append(_job(batch, hi - 3, hi - 3, cin, cout, flags, ld_x, k=4, pad=0))
            hi, cin = (hi - 3) // 2, cout
    # the shapes of the kernel tests
    for n, h, w, c0, c1, cout, ups, _, _ in kc.CASES + kc.HALO_CASES + kc.WFAST_CASES + kc.COMPACT_CASES:
        for c in (c0, c1) if c1 else (c0,):
            conv3(n, h, w, c, cout, ups)
    for n, h, w, c, cout in KNOWN_FORMS.values():
        conv3(n, h, w, c, cout, False)
    for n, hi, wi, cin, cout in kc.K4_CASES:
        for ld_x in _lds(cin):
            for flags in (0, CLEAN_PADS):
                rows.append((n, hi - 3, wi - 3, hi, wi, cin, cout, 4, 4, 0, ld_x, _up(cout, 4), flags, 1))
    # a grid over the rules' thresholds
    for n in (1, 4, 32):
        for hw in (2, 4, 6, 8, 16, 24, 32, 64, 128):
            for c in (3, 13, 16, 20, 35, 45, 64, 72, 130, 256):
                for cout in (1, 10, 20, 45, 64, 70, 136):
                    for flags in (0, CLEAN_PADS, UPSAMPLED | CLEAN_PADS):
                        for ld_x in (_up(c, 4), _up(c, 16)):
                            rows.append(_job(n, hw, hw, c, cout, flags, ld_x))
    # up-sampled layers without the sub-pixel form: the tap-major kernel's up-sampled-view loader (mode 2)
    for n, hw, c, cout in ((2, 16, 70, 70), (4, 32, 130, 45), (32, 64, 64, 136), (1, 8, 72, 48), (8, 16, 256, 256), (2, 4, 40, 136)):
        for flags in (UPSAMPLED, UPSAMPLED | CLEAN_PADS):
            rows.append(_job(n, hw, hw, c, cout, flags, _up(c, 4), subpixel=0))
    return np.array(sorted(set(rows)), dtype=np.int64)


class _Plan(ctypes.Structure):
    _fields_ = [("layout", ctypes.c_int), ("splits", ctypes.c_int), ("part_floats", ctypes.c_size_t)]


def answers(lib, jobs):
    """The planners' answers for the rows of `jobs` (the first N_IN columns): an int64 array of 6 columns per row.
    lib: a mnk._lib.Library."""
    from mnk.optim import JOB
    out = np.zeros((len(jobs), 6), dtype=np.int64)
    try:
        for subpixel in sorted(set(int(v) for v in jobs[:, 13])):
            sel = np.flatnonzero(jobs[:, 13] == subpixel)
            lib.call("mnk_set_tuning", b"up_subpixel", subpixel)
            rec = np.zeros(len(sel), dtype=JOB)
            for f, col in (("N", 0), ("Ho", 1), ("Wo", 2), ("Hi", 3), ("Wi", 4), ("C", 5), ("Cout", 6), ("kh", 7), ("kw", 8),
                           ("pad", 9), ("ld_x", 10), ("ld_dy", 11), ("flags", 12)):
                rec[f] = jobs[sel, col]
            if lib.query("mnk_wgrad_grouped_plan", rec.ctypes.data, len(rec)) != 0:
                raise RuntimeError("mnk_wgrad_grouped_plan failed")
            out[sel, 3], out[sel, 4], out[sel, 5] = rec["variant"], rec["splits"], rec["part_floats"]
            plan = _Plan()
            for i in sel:
                n, ho, wo, _, _, c, cout, kh, kw, pad, ld_x, _, flags, _ = (int(v) for v in jobs[i, :N_IN])
                if lib.query("mnk_conv2d_wgrad_plan2", n, ho, wo, c, cout, kh, kw, pad, ld_x, flags, ctypes.byref(plan)) != 0:
                    raise RuntimeError("mnk_conv2d_wgrad_plan2 failed")
                out[i, 0], out[i, 1], out[i, 2] = plan.layout, plan.splits, plan.part_floats
    finally:
        lib.call("mnk_set_tuning", b"up_subpixel", 1)
    return out


def summary(table):
    v = table[:, 17]
    tap = v[(v >= 0) & (v < 16)]
    return ("%d rows; plan layouts %s; direct-write %d; grouped tap-major (tile, mode) %s; nine-tap variants %s; not grouped %d"
            % (len(table), {int(k): int((table[:, 14] == k).sum()) for k in np.unique(table[:, 14])}, int((table[:, 15] == 0).sum()),
               sorted(set((int(t) // 4, int(t) % 4) for t in tap)), sorted(set(int(t) for t in v[v >= 16])), int((v < 0).sum())))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--library", default=os.path.join(ROOT, "tests", "hipemu", "build", "libmnk_emu.so"),
                    help="the build that answers (default: this tree's CPU emulator build, tests/hipemu/build.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wgrad_plans.npz"))
    args = ap.parse_args()
    from mnk import _lib
    lib = _lib.Library(args.library, strict=False)
    jobs = sweep()
    table = np.concatenate([jobs, answers(lib, jobs)], axis=1)
    np.savez_compressed(args.out, columns=np.array(COLUMNS), table=table)
    print(summary(table))
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
