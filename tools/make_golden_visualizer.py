#!/usr/bin/env python
"""Records tests/golden/visualizer.npz: inputs and the uint8 grids of the UNMODIFIED reference `logger.Visualizer`
(imported through oracle.ref_shim; works only where the reference tree exists), for tests/test_visualizer.py.

matplotlib is the real, installed one.  scikit-image is not installed here (oracle.ref_shim stubs it), so `logger.circle` is
bound to `circle` below: a numpy restatement, written here, of scikit-image 0.14's skimage/draw/draw.py `circle` -> `ellipse` ->
`_ellipse_in_shape` (the version the reference's requirements.txt pins), statement by statement and in the same order of
float64 operations.  This follows the precedent of oracle/augment_restate.py, which restates the pinned skimage / Pillow /
torchvision transforms for the input path.  Everything else that runs is the reference's own code: draw_video_with_kp,
create_video_column[_with_kp], create_image_grid, visualize_reconstruction, visualize_transfer and their uint8 conversion.

    python tools/make_golden_visualizer.py          # writes tests/golden/visualizer.npz
    python tools/make_golden_visualizer.py --lut    # also rewrites monkey-net_amd/mnk/gist_rainbow_lut.txt from matplotlib

A case i is stored as c{i}_kind ('reconstruction' | 'transfer'), c{i}_kp_size, c{i}_border, c{i}_key ('video' | 'driving'), the
input tensors c{i}_<name> and c{i}_grid (+ c{i}_strip: the PNG strip of reconstruction.py:66-68 for the case's prediction)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---- scikit-image 0.14, skimage/draw/draw.py, restated -------------------------------------------------------------------------
def _ellipse_in_shape(shape, center, radii, rotation=0.):
    r_lim, c_lim = np.ogrid[0:float(shape[0]), 0:float(shape[1])]
    r_org, c_org = center
    r_rad, c_rad = radii
    rotation %= np.pi
    sin_alpha, cos_alpha = np.sin(rotation), np.cos(rotation)
    r, c = (r_lim - r_org), (c_lim - c_org)
    distances = ((r * cos_alpha + c * sin_alpha) / r_rad) ** 2 + ((r * sin_alpha - c * cos_alpha) / c_rad) ** 2
    return np.nonzero(distances < 1)


def ellipse(r, c, r_radius, c_radius, shape=None, rotation=0.):
    center = np.array([r, c])
    radii = np.array([r_radius, c_radius])
    rotation %= np.pi
    r_radius_rot = abs(r_radius * np.cos(rotation)) + c_radius * abs(np.sin(rotation))
    c_radius_rot = r_radius * abs(np.sin(rotation)) + c_radius * abs(np.cos(rotation))
    radii_rot = np.array([r_radius_rot, c_radius_rot])
    upper_left = np.ceil(center - radii_rot).astype(int)
    lower_right = np.floor(center + radii_rot).astype(int)
    if shape is not None:
        upper_left = np.maximum(upper_left, np.array([0, 0]))
        lower_right = np.minimum(lower_right, np.array(shape[:2]) - 1)
    shifted_center = center - upper_left
    bounding_shape = lower_right - upper_left + 1
    rr, cc = _ellipse_in_shape(bounding_shape, shifted_center, radii, rotation)
    rr = rr + upper_left[0]
    cc = cc + upper_left[1]
    return rr, cc


def circle(r, c, radius, shape=None):
    return ellipse(r, c, radius, radius, shape)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def frames(rng, *shape):
    """float32 frames in [0, 1]: uniform values mixed with 0, 1, k / 255 and the float32 just below (k + 1) / 255 -- the values
    where the truncating `(255 * image).astype(np.uint8)` is decided by the last bit of a float32 product"""
    n = int(np.prod(shape))
    k = rng.integers(0, 256, n)
    exact = (k / 255).astype(np.float32)
    below = np.nextafter(((k + 1) / 255).astype(np.float32), np.float32(0))
    below = np.minimum(below, np.float32(1))
    uni = rng.random(n, dtype=np.float32)
    pick = rng.integers(0, 6, n)
    v = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [exact, below, np.zeros(n, np.float32), np.ones(n, np.float32)], uni)
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def keypoints(rng, b, d, k, h, w, special):
    """(b, d, k, 2) float32 means: random ones incl. positions outside [-1, 1] (clipped circles); with `special`, centres exactly
    on integers and half-integers (h, w powers of two: 2 c / size - 1 and the centre are exact), overlapping pairs (paint
    order) and far-off positions"""
    kp = (rng.random((b, d, k, 2)) * 2.5 - 1.25).astype(np.float32)
    if special:
        size = np.array([w, h], dtype=np.float64)
        for i in range(b):
            for f in range(d):
                c0 = rng.integers(0, [w + 1, h + 1])                         # integer centre (incl. the far edge)
                kp[i, f, 0] = 2 * c0 / size - 1
                c1 = rng.integers(0, [w, h]) + 0.5                           # half-integer centre
                kp[i, f, 1] = 2 * c1 / size - 1
                kp[i, f, 2] = kp[i, f, 0] + 2 * np.array([1.0, 0.0]) / size  # one pixel beside key point 0: overlap
                kp[i, f, 3] = kp[i, f, 1]                                    # exactly on key point 1: the later one wins
                kp[i, f, 4] = [-1.0, -1.0]                                   # the corner: three quarters clipped
                kp[i, f, 5] = [1.0, 2 * 3.5 / h - 1]                         # centre on column W: half clipped
                kp[i, f, 6] = [7.0, -9.0]                                    # far outside: nothing drawn
                kp[i, f, 7] = kp[i, f, 0] + 2 * np.array([0.5, 0.5]) / size  # half a pixel off an integer centre
    return torch.from_numpy(kp.astype(np.float32))


CASES = [
    # kind, B, d, H, W, K, kp_size, border, key, special, strip
    ("reconstruction", 1, 4, 32, 32, 10, 2, False, "video", False, True),
    ("reconstruction", 3, 1, 32, 32, 10, 2, True, "driving", False, False),
    ("transfer", 1, 3, 40, 24, 15, 3, False, "video", False, False),
    ("transfer", 2, 2, 24, 40, 10, 1, True, "video", False, False),
    ("reconstruction", 1, 2, 16, 16, 10, 1, False, "video", True, False),
    ("reconstruction", 2, 2, 16, 32, 10, 2, True, "driving", True, False),
    ("transfer", 1, 2, 32, 16, 10, 3, True, "video", True, False),
    ("reconstruction", 1, 2, 40, 24, 15, 3, False, "video", False, False),
    ("reconstruction", 2, 1, 21, 13, 10, 2.5, True, "driving", False, False),       # odd sizes: the unvectorised kernel form
]


def main():
    from oracle import ref_shim
    ref_shim.install()
    import logger                                   # the reference's logger.py
    import matplotlib
    logger.circle = circle
    rng = np.random.default_rng(20240521)
    rec = {"matplotlib_version": np.array(matplotlib.__version__), "num_cases": np.array(len(CASES))}
    for i, (kind, b, d, h, w, k, kp_size, border, key, special, strip) in enumerate(CASES):
        vis = logger.Visualizer(kp_size=kp_size, draw_border=border, colormap="gist_rainbow")
        t = {"source": frames(rng, b, 3, 1, h, w), "video": frames(rng, b, 3, d, h, w),
             "video_prediction": frames(rng, b, 3, d, h, w), "video_deformed": frames(rng, b, 3, d, h, w),
             "kp_source": keypoints(rng, b, 1, k, h, w, special), "kp_driving": keypoints(rng, b, d, k, h, w, special),
             "kp_norm": keypoints(rng, b, d, k, h, w, special)}
        out = {"video_prediction": t["video_prediction"], "video_deformed": t["video_deformed"],
               "kp_source": {"mean": t["kp_source"]}, "kp_driving": {"mean": t["kp_driving"]}, "kp_norm": {"mean": t["kp_norm"]}}
        if kind == "reconstruction":
            grid = vis.visualize_reconstruction({"source": t["source"], key: t["video"]}, out)
            del t["kp_norm"]
        else:
            # transfer.py hands the whole source video over; Visualizer takes its frame 0 (logger.py:132)
            grid = vis.visualize_transfer(t["video"], t["source"], out)
        assert grid.dtype == np.uint8
        for name, v in t.items():
            rec["c%d_%s" % (i, name)] = v.numpy()
        rec.update({"c%d_kind" % i: np.array(kind), "c%d_kp_size" % i: np.array(float(kp_size)), "c%d_border" % i: np.array(border),
                    "c%d_key" % i: np.array(key), "c%d_grid" % i: grid})
        if strip:
            # reconstruction.py:66-68 / prediction.py:137-139, restated here (two statements of a script's main loop)
            o = t["video_prediction"].data.cpu().numpy()
            o = np.concatenate(np.transpose(o, [0, 2, 3, 4, 1])[0], axis=1)
            rec["c%d_strip" % i] = (255 * o).astype(np.uint8)
        print("case %d: %s B=%d d=%d %dx%d K=%d kp_size=%s border=%s -> grid %s, %d key-point pixels" % (
            i, kind, b, d, h, w, k, kp_size, border, grid.shape, int(_painted(vis, t, grid))))
    vis = logger.Visualizer()
    for k in (10, 15):
        rec["colors_%d" % k] = np.array([np.array(vis.colormap(j / k))[:3] for j in range(k)]).astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "visualizer.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")
    if "--lut" in sys.argv[1:]:
        import matplotlib.pyplot as plt
        lut = np.asarray(plt.get_cmap("gist_rainbow")(np.arange(256)))[:, :3].astype(np.float64)
        lut_path = os.path.join(ROOT, "monkey-net_amd", "mnk", "gist_rainbow_lut.txt")
        with open(lut_path, "w") as f:
            f.write("# matplotlib 'gist_rainbow', N = 256: R G B per entry as float64 repr (tools/make_golden_visualizer.py --lut)\n")
            for row in lut:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
        print(lut_path, os.path.getsize(lut_path), "bytes")


def _painted(vis, t, grid):
    """pixels of the first column that differ from the plain frames: a case that draws nothing would test nothing"""
    plain = logger_free_column(t["source"], grid.shape[0], vis.draw_border)
    w = t["source"].shape[-1]
    return (grid[:, :, :w] != plain).any(axis=-1).sum()


def logger_free_column(source, d, border):
    v = np.transpose(source.numpy().repeat(d, axis=2), [0, 2, 3, 4, 1]).copy()
    if border:
        v[:, :, [0, -1]] = 1
        v[:, :, :, [0, -1]] = 1
    return (255 * np.concatenate(list(v), axis=1)).astype(np.uint8)


if __name__ == "__main__":
    main()
