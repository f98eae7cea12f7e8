"""The device-side output path (csrc/visualizer.hip, mnk/visualizer.py): uint8 grids of the reference's logger.Visualizer and the
PNG strip of its evaluation loops, compared for EQUALITY (np.array_equal, no tolerance) with

* tests/golden/visualizer.npz: grids recorded from the unmodified reference Visualizer by tools/make_golden_visualizer.py
  (every case: reconstruction with d > 1, the d = 1 training batch under the 'driving' key, transfer, draw_border on / off,
  kp_size 1 / 2 / 3 / 2.5, 40 x 24 and 21 x 13 frames, key points outside [-1, 1], overlapping ones, centres exactly on integers
  and half-integers, pixel values 0, 1, k / 255 and just below (k + 1) / 255; the strip of case 0);
* `reference_grid` below, a numpy restatement of logger.py:97-175 (with scikit-image 0.14's circle restated next to it), on
  .cpu() copies of tensors that include the outputs of a real eval forward of the TINY configuration;
* the live reference class where the reference tree exists.

Kernel tests run through the guard-banded `be` fixture on the CPU emulator and, with -m gpu, on the MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cases
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_modules import build, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "visualizer.npz"))
NUM_CASES = int(GOLD["num_cases"])


# ---- numpy restatement of the reference ----------------------------------------------------------------------------------------
def circle_pixels(r, c, radius, shape):
    """skimage.draw.circle(r, c, radius, shape) of scikit-image 0.14 (circle -> ellipse -> _ellipse_in_shape with rotation 0), in
    its order of float64 operations: a bounding box from ceil / floor of centre -+ radius, clipped to the frame; the centre
    shifted into the box; ((r' - r0) / radius)^2 + ((c' - c0) / radius)^2 < 1 over the box"""
    centre = np.array([r, c])
    radii = np.array([radius, radius])
    upper_left = np.maximum(np.ceil(centre - radii).astype(int), 0)
    lower_right = np.minimum(np.floor(centre + radii).astype(int), np.array(shape[:2]) - 1)
    shifted = centre - upper_left
    box = lower_right - upper_left + 1
    rows, cols = np.ogrid[0:float(box[0]), 0:float(box[1])]
    dr, dc = rows - shifted[0], cols - shifted[1]
    dist = ((dr * 1.0 + dc * 0.0) / radii[0]) ** 2 + ((dr * 0.0 - dc * 1.0) / radii[1]) ** 2
    rr, cc = np.nonzero(dist < 1)
    return rr + upper_left[0], cc + upper_left[1]


def reference_grid(columns, d, kp_size, draw_border, colors):
    """logger.py:97-126 + the uint8 conversion of :151 / :174 on numpy arrays.  columns: `video` or `(video, kp)`, video
    (B, 3, d | 1, H, W) float32, kp (B, d | 1, K, 2) float32; one-frame entries are repeated over d frames as the reference's
    `.repeat(1, 1, d, 1, 1)` / `.repeat(1, d, 1, 1)` do.  colors: (K, 3) float32 = float32(colormap(k / K)[:3])."""
    out = []
    for col in columns:
        video, kp = col if isinstance(col, tuple) else (col, None)
        if video.shape[2] == 1 and d > 1:
            video = np.tile(video, (1, 1, d, 1, 1))
        videos = np.transpose(video, [0, 2, 3, 4, 1])                       # (B, d, H, W, 3)
        if kp is not None:
            if kp.shape[1] == 1 and d > 1:
                kp = np.tile(kp, (1, d, 1, 1))
            drawn = []
            for v, k in zip(videos, kp):
                frames = np.copy(v)
                size = np.array(frames.shape[2:0:-1])[np.newaxis, np.newaxis]       # (W, H): int64
                centres = size * (k + 1) / 2                                        # float32 + 1, then float64
                for i in range(len(frames)):
                    for ind, p in enumerate(centres[i]):
                        rr, cc = circle_pixels(p[1], p[0], kp_size, frames.shape[1:3])
                        frames[i][rr, cc] = colors[ind]
                drawn.append(frames)
            videos = np.array(drawn)
        if draw_border:
            videos = np.copy(videos)
            videos[:, :, [0, -1]] = (1, 1, 1)
            videos[:, :, :, [0, -1]] = (1, 1, 1)
        out.append(np.concatenate(list(videos), axis=1))
    image = np.concatenate(out, axis=2)
    assert image.dtype == np.float32
    return (255 * image).astype(np.uint8)


def reconstruction_columns(inp, out):
    """the columns of visualize_reconstruction (logger.py:154-173)"""
    gt = inp["driving"] if "driving" in inp else inp["video"]
    return [(inp["source"], out["kp_source"]["mean"]), (gt, out["kp_driving"]["mean"]), out["video_prediction"],
            out["video_deformed"], gt]


def transfer_columns(driving, source, out):
    """the columns of visualize_transfer (logger.py:128-150)"""
    return [(source[:, :, 0:1], out["kp_source"]["mean"]), (driving[:, :, 0:1], out["kp_driving"]["mean"][:, :1]),
            (driving, out["kp_driving"]["mean"]), (out["video_prediction"], out["kp_norm"]["mean"]), out["video_prediction"],
            out["video_deformed"]]


def to_numpy(columns):
    f = lambda t: t.detach().cpu().numpy()
    return [(f(c[0]), f(c[1])) if isinstance(c, tuple) else f(c) for c in columns]


def reference_strip(video):
    """reconstruction.py:66-68 / prediction.py:137-139 on a (B, 3, D, H, W) float32 array"""
    frames = np.transpose(video, [0, 2, 3, 4, 1])[0]
    return (255 * np.concatenate(frames, axis=1)).astype(np.uint8)


def tricky_frames(seed, *shape):
    """float32 frames in [0, 1] mixing uniform values with 0, 1, k / 255 and the float32 just below (k + 1) / 255"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    k = rng.integers(0, 256, n)
    exact = (k / 255).astype(np.float32)
    below = np.minimum(np.nextafter(((k + 1) / 255).astype(np.float32), np.float32(0)), np.float32(1))
    pick = rng.integers(0, 6, n)
    v = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [exact, below, np.zeros(n, np.float32), np.ones(n, np.float32)],
                  rng.random(n, dtype=np.float32))
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def random_kp(seed, b, d, k):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, d, k, 2, generator=g) * 2.5 - 1.25                  # incl. positions outside the frame


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def gold_case(i):
    g = lambda name: torch.from_numpy(GOLD["c%d_%s" % (i, name)])
    kind, key = str(GOLD["c%d_kind" % i]), str(GOLD["c%d_key" % i])
    t = {n: g(n) for n in ("source", "video", "video_prediction", "video_deformed", "kp_source", "kp_driving")}
    if kind == "transfer":
        t["kp_norm"] = g("kp_norm")
    return {"kind": kind, "key": key, "kp_size": float(GOLD["c%d_kp_size" % i]), "border": bool(GOLD["c%d_border" % i]),
            "t": t, "grid": GOLD["c%d_grid" % i]}


def case_inputs(case, conv=lambda x: x):
    """(inp / (driving, source), out) of a fixture case as the Visualizer's methods take them"""
    t = {k: conv(v) for k, v in case["t"].items()}
    out = {"video_prediction": t["video_prediction"], "video_deformed": t["video_deformed"],
           "kp_source": {"mean": t["kp_source"]}, "kp_driving": {"mean": t["kp_driving"]}}
    if case["kind"] == "transfer":
        out["kp_norm"] = {"mean": t["kp_norm"]}
        return (t["video"], t["source"]), out
    return {"source": t["source"], case["key"]: t["video"]}, out


def case_columns(case, conv=lambda x: x):
    first, out = case_inputs(case, conv)
    return transfer_columns(first[0], first[1], out) if case["kind"] == "transfer" else reconstruction_columns(first, out)


def kernel_grid(be, columns, d, kp_size, border, colors, materialise=False):
    """mnk_vis_grid through the checked `be.call` on guard-banded buffers.  materialise: one-frame videos / key points are
    repeated into d-frame tensors first (the reference's own form) instead of travelling as stride-0 columns."""
    from mnk.ops import VIS_COLUMN
    cols = [c if isinstance(c, tuple) else (c, None) for c in columns]
    rec = np.zeros(len(cols), dtype=VIS_COLUMN)
    keep, K = [], 0
    b, _, _, h, w = cols[0][0].shape
    for i, (v, kp) in enumerate(cols):
        if materialise and v.shape[2] == 1:
            v = v.repeat(1, 1, d, 1, 1)
        v = be.t(v)
        keep.append(v)
        rec[i]["video"], rec[i]["batch_stride"], rec[i]["chan_stride"] = v.data_ptr(), v.stride(0), v.stride(1)
        rec[i]["frame_stride"] = v.stride(2) if v.shape[2] > 1 else 0
        if kp is not None:
            if materialise and kp.shape[1] == 1:
                kp = kp.repeat(1, d, 1, 1)
            kp = be.t(kp)
            keep.append(kp)
            K = kp.shape[2]
            rec[i]["kp"], rec[i]["kp_batch_stride"] = kp.data_ptr(), kp.stride(0)
            rec[i]["kp_frame_stride"] = kp.stride(1) if kp.shape[1] > 1 else 0
    out = be.empty_int(d, b * h, len(cols) * w, 3, dtype=torch.uint8)
    be.call("mnk_vis_grid", int(rec.ctypes.data), len(cols), b, 3, d, h, w, K, float(kp_size), int(border), be.t(colors), out)
    be.sync()
    return out.cpu().numpy()


def colors_for(k):
    from mnk.visualizer import keypoint_colors
    return torch.from_numpy(keypoint_colors("gist_rainbow", k))


def assert_same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    diff = got != want
    print("%s: %d of %d bytes differ" % (what, int(diff.sum()), diff.size))
    assert np.array_equal(got, want), "%s: %d of %d bytes differ, first at %s (got %d, reference %d)" % (
        what, int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])],
        want[tuple(np.argwhere(diff)[0])])


# ---- kernels against the recorded reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NUM_CASES))
def test_vis_grid_kernel_equals_the_recorded_reference_grid(be, i):
    case = gold_case(i)
    d = case["t"]["video_prediction"].shape[2]
    k = case["t"]["kp_driving"].shape[2]
    got = kernel_grid(be, case_columns(case), d, case["kp_size"], case["border"], colors_for(k))
    assert_same_bytes(got, case["grid"], "case %d (%s) on %s" % (i, case["kind"], be.kind))


@pytest.mark.parametrize("i", range(NUM_CASES))
def test_restatement_equals_the_recorded_reference_grid(i):
    """`reference_grid` (what the class-level and MI355X-sized tests compare with) reproduces every recorded grid"""
    case = gold_case(i)
    d = case["t"]["video_prediction"].shape[2]
    k = case["t"]["kp_driving"].shape[2]
    want = reference_grid(to_numpy(case_columns(case)), d, case["kp_size"], case["border"], GOLD["colors_%d" % k])
    assert_same_bytes(want, case["grid"], "restatement, case %d" % i)


@pytest.mark.parametrize("i", [0, 2, 5, 8])
def test_stride_zero_columns_equal_materialised_repeats(be, i):
    case = gold_case(i)
    d = case["t"]["video_prediction"].shape[2]
    k = case["t"]["kp_driving"].shape[2]
    args = (case_columns(case), d, case["kp_size"], case["border"], colors_for(k))
    assert_same_bytes(kernel_grid(be, *args), kernel_grid(be, *args, materialise=True), "stride 0 against repeat, case %d" % i)


def test_frames_to_strip_kernel_equals_the_recorded_strip(be):
    strips = [i for i in range(NUM_CASES) if "c%d_strip" % i in GOLD.files]
    assert strips
    for i in strips:
        video = be.t(torch.from_numpy(GOLD["c%d_video_prediction" % i]))
        _, c, d, h, w = video.shape
        out = be.empty_int(h, d * w, 3, dtype=torch.uint8)
        be.call("mnk_frames_to_strip", video, c, video.stride(1), video.stride(2), d, h, w, out)
        be.sync()
        assert_same_bytes(out.cpu().numpy(), GOLD["c%d_strip" % i], "strip of case %d" % i)


@pytest.mark.parametrize("i", range(NUM_CASES))
def test_frames_to_strip_kernel_equals_the_restated_strip(be, i):
    """every case's prediction (incl. the 21 x 13 frames: the unvectorised form), video 0 of the batch"""
    video = be.t(torch.from_numpy(GOLD["c%d_video_prediction" % i]))
    _, c, d, h, w = video.shape
    out = be.empty_int(h, d * w, 3, dtype=torch.uint8)
    be.call("mnk_frames_to_strip", video, c, video.stride(1), video.stride(2), d, h, w, out)
    be.sync()
    assert_same_bytes(out.cpu().numpy(), reference_strip(GOLD["c%d_video_prediction" % i]), "strip of case %d" % i)


# ---- colours -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 15])
def test_shipped_colour_table_equals_the_recorded_colours(k):
    from mnk.visualizer import keypoint_colors
    got = keypoint_colors("gist_rainbow", k)
    assert got.dtype == np.float32 and np.array_equal(got, GOLD["colors_%d" % k])
    try:
        import matplotlib.pyplot as plt
    except ImportError:
        return
    cmap = plt.get_cmap("gist_rainbow")
    for n in (1, 3, 7, 10, 15, 32):
        live = np.array([np.array(cmap(j / n))[:3] for j in range(n)]).astype(np.float32)
        assert np.array_equal(keypoint_colors("gist_rainbow", n), live), n
        assert np.array_equal(keypoint_colors(cmap, n), live), n


def test_another_colormap_needs_matplotlib(monkeypatch):
    from mnk.visualizer import Visualizer
    monkeypatch.setitem(sys.modules, "matplotlib", None)
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
    with pytest.raises(ImportError, match="needs matplotlib"):
        Visualizer(colormap="viridis")
    Visualizer()                                                    # the default needs nothing but the shipped table


# ---- argument validation -------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_before_launch(be):
    from mnk._lib import MnkError
    from mnk.ops import VIS_COLUMN
    b, d, h, w, k = 1, 2, 8, 8, 3
    video = be.t(torch.rand(b, 3, d, h, w))
    kp = be.t(torch.rand(b, d, k, 2))
    colors = be.t(torch.rand(k, 3))
    out = be.empty_int(d, b * h, 9 * w, 3, dtype=torch.uint8)
    before = out.clone()
    rec = np.zeros(9, dtype=VIS_COLUMN)
    for r in rec:
        r["video"], r["kp"], r["batch_stride"], r["chan_stride"], r["frame_stride"] = video.data_ptr(), kp.data_ptr(), 3 * d * h * w, \
            d * h * w, h * w
        r["kp_batch_stride"], r["kp_frame_stride"] = d * k * 2, k * 2
    ptr = int(rec.ctypes.data)
    good = dict(cols=ptr, ncol=2, B=b, C=3, d=d, H=h, W=w, K=k, kp_size=2.0, border=0, colors=colors, out=out)
    be.call("mnk_vis_grid", *good.values())                          # (the valid call goes through)
    be.sync()
    assert not torch.equal(out, before)
    before = out.clone()
    for bad in (dict(C=4), dict(C=1), dict(K=33), dict(ncol=9), dict(ncol=0), dict(cols=None), dict(out=None), dict(colors=None),
                dict(B=0), dict(d=0), dict(H=0), dict(W=-1), dict(K=0), dict(kp_size=0.0), dict(kp_size=-1.0)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_vis_grid", *{**good, **bad}.values())
    norec = rec.copy()
    norec[1]["video"] = 0
    with pytest.raises(MnkError, match="invalid argument"):
        be.call("mnk_vis_grid", *{**good, "cols": int(norec.ctypes.data)}.values())
    strip = be.empty_int(h, d * w, 3, dtype=torch.uint8)
    sgood = dict(video=video, C=3, cs=d * h * w, fs=h * w, D=d, H=h, W=w, out=strip)
    be.call("mnk_frames_to_strip", *sgood.values())
    for bad in (dict(C=4), dict(C=1), dict(video=None), dict(out=None), dict(D=0), dict(H=0), dict(W=0), dict(cs=-1)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_frames_to_strip", *{**sgood, **bad}.values())
    be.sync()
    assert torch.equal(out, before)                                  # no rejected call wrote anything


def test_wrappers_reject_what_the_kernel_cannot_read(be):
    from mnk import ops
    v = be.t(torch.rand(1, 3, 2, 8, 8))
    with pytest.raises(ValueError):
        ops.vis_grid([v, be.t(torch.rand(1, 3, 2, 8, 4))], 2, 2, False, None)
    with pytest.raises(ValueError):
        ops.vis_grid([v.double()], 2, 2, False, None)
    with pytest.raises(ValueError):
        ops.vis_grid([(v, be.t(torch.rand(1, 2, 4, 2)))], 2, 2, False, be.t(torch.rand(5, 3)))
    with pytest.raises(ValueError):
        ops.frames_to_strip(v)
    from mnk.visualizer import Visualizer
    with pytest.raises(ValueError, match="one frame"):
        Visualizer().visualize_reconstruction({"source": v, "video": v}, {"video_prediction": v, "video_deformed": v,
                                              "kp_source": {"mean": None}, "kp_driving": {"mean": None}})


# ---- the class -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NUM_CASES))
def test_visualizer_class_equals_the_recorded_reference_grid(be, i):
    """mnk.visualizer.Visualizer with the reference's constructor and method arguments; in half of the cases `inp` / the driving
    video are HOST tensors next to device outputs (copied to the device by the class)"""
    from mnk.visualizer import Visualizer
    case = gold_case(i)
    vis = Visualizer(kp_size=case["kp_size"] if case["kp_size"] != int(case["kp_size"]) else int(case["kp_size"]),
                     draw_border=case["border"], colormap="gist_rainbow")
    first, out = case_inputs(case, be.t)
    if i % 2:
        host, _ = case_inputs(case)
        first = host
    if case["kind"] == "transfer":
        got = vis.visualize_transfer(first[0], first[1], out)
    else:
        got = vis.visualize_reconstruction(first, out)
    assert isinstance(got, np.ndarray)
    assert_same_bytes(got, case["grid"], "Visualizer, case %d" % i)
    dev = vis.visualize_transfer(first[0], first[1], out, as_tensor=True) if case["kind"] == "transfer" else \
        vis.visualize_reconstruction(first, out, as_tensor=True)
    assert torch.is_tensor(dev) and dev.device.type == be.device.type and dev.dtype == torch.uint8
    assert np.array_equal(dev.cpu().numpy(), case["grid"])


def test_png_strip_equals_the_recorded_strip(be):
    from mnk.visualizer import png_strip
    video = be.t(torch.from_numpy(GOLD["c0_video_prediction"]))
    assert_same_bytes(png_strip(video), GOLD["c0_strip"], "png_strip")
    assert_same_bytes(png_strip(video[0]), GOLD["c0_strip"], "png_strip of one video")
    assert png_strip(video, as_tensor=True).device.type == be.device.type


def _tiny_models(be):
    gold = load("tiny")
    gen, disc, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    return gen.to(be.device).eval(), kpd.to(be.device).eval(), gold["size"]


@pytest.mark.parametrize("kp_size,border", [(2, False), (3, True)])
def test_visualizer_on_a_real_transfer_forward_equals_the_restatement(be, kp_size, border):
    """mnk.engine.Transfer's dict (permuted views of the folded generator output, device key points) goes straight into
    visualize_transfer; the restatement runs on .cpu() copies of the same tensors"""
    from mnk import engine
    from mnk.visualizer import Visualizer, png_strip
    gen, kpd, size = _tiny_models(be)
    src, _ = cases.smooth_pair(2, size, size, seed=11)
    driving = torch.cat([cases.smooth_pair(2, size, size, seed=20 + i)[1] for i in range(3)], dim=2)
    src, driving = be.t(src), be.t(driving)
    out = engine.Transfer(kpd, gen, dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True))(src, driving)
    be.sync()
    vis = Visualizer(kp_size=kp_size, draw_border=border)
    got = vis.visualize_transfer(driving, src, out)
    k = out["kp_driving"]["mean"].shape[2]
    want = reference_grid(to_numpy(transfer_columns(driving, src, out)), 3, kp_size, border, colors_for(k).numpy())
    assert got.shape == (3, 2 * size, 6 * size, 3)
    assert_same_bytes(got, want, "transfer forward")
    assert (got != reference_grid(to_numpy(transfer_columns(driving, src, out)), 3, kp_size, border,
                                  np.zeros((k, 3), np.float32))).any(), "no key point was drawn: the case tests nothing"
    assert_same_bytes(png_strip(out["video_prediction"]), reference_strip(out["video_prediction"].cpu().numpy()), "strip")


@pytest.mark.parametrize("key", ["video", "driving"])
def test_visualizer_on_a_real_reconstruction_forward_equals_the_restatement(be, key):
    """mnk.engine.Reconstructor's eval forward (reconstruction.py:57-64's tensors, batch 2, one frame) into
    visualize_reconstruction, under either key of `inp`"""
    from mnk import engine
    from mnk.visualizer import Visualizer
    gen, kpd, size = _tiny_models(be)
    src, drv = cases.smooth_pair(2, size, size)
    src, drv = be.t(src), be.t(drv)
    r = engine.Reconstructor(kpd, gen)(src, drv)
    be.sync()
    out = {"video_prediction": r["video_prediction"], "video_deformed": r["video_deformed"],
           "kp_driving": {"mean": r["kp_driving_mean"]}, "kp_source": {"mean": r["kp_source_mean"]}}
    inp = {"source": src, key: drv}
    got = Visualizer(draw_border=True).visualize_reconstruction(inp, out)
    k = r["kp_driving_mean"].shape[2]
    want = reference_grid(to_numpy(reconstruction_columns(inp, out)), 1, 2, True, colors_for(k).numpy())
    assert got.shape == (1, 2 * size, 5 * size, 3)
    assert_same_bytes(got, want, "reconstruction forward")


# ---- the launcher switch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["1", "0", None])
def test_native_visualizer_switch(tmp_path, switch):
    """run_reference.py on a stand-in script directory with its own logger.py: with MNK_NATIVE_VISUALIZER=1 the script sees
    mnk.visualizer.Visualizer under `logger.Visualizer` (also inside that module, where Logger looks it up); unset or 0, the
    file's own class"""
    (tmp_path / "logger.py").write_text("class Visualizer:\n    origin = 'stand-in'\n\n"
                                        "def inside():\n    return Visualizer\n")
    script = tmp_path / "probe.py"
    script.write_text("import sys\nbefore = 'mnk.visualizer' in sys.modules\n"
                      "from logger import Visualizer, inside\n"
                      "print(Visualizer.__module__, inside() is Visualizer, before)\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MNK_NATIVE_VISUALIZER")}
    if switch is not None:
        env["MNK_NATIVE_VISUALIZER"] = switch
    out = subprocess.run([sys.executable, os.path.join(ROOT, "monkey-net_amd", "run_reference.py"), str(script)],
                         capture_output=True, text=True, timeout=300, env=env, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    want = "mnk.visualizer True True" if switch == "1" else "logger True False"
    assert out.stdout.strip().splitlines()[-1] == want, out.stdout
    from mnk import knobs
    assert knobs.KNOBS["MNK_NATIVE_VISUALIZER"][0] == "0"


# ---- the live reference --------------------------------------------------------------------------------------------------------
_LIVE = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tools")
from oracle import ref_shim
ref_shim.install()
import logger
from make_golden_visualizer import circle          # scikit-image is not installed: its circle, restated in the tool
logger.circle = circle
z = np.load(sys.argv[2])
t = {k: torch.from_numpy(z[k]) for k in z.files}
out = {"video_prediction": t["video_prediction"], "video_deformed": t["video_deformed"], "kp_source": {"mean": t["kp_source"]},
       "kp_driving": {"mean": t["kp_driving"]}, "kp_norm": {"mean": t["kp_norm"]}}
vis = logger.Visualizer(kp_size=3, draw_border=True)
np.savez(sys.argv[3], rec=vis.visualize_reconstruction({"source": t["source"], "video": t["video"]}, out),
         tra=vis.visualize_transfer(t["video"], t["source"], out))
"""


def _reference_available():
    from oracle import ref_shim
    return ref_shim.available()


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not on this machine")
def test_visualizer_equals_the_live_reference_class(be, tmp_path):
    """fresh inputs (not the fixture's) through the unmodified reference Visualizer in a process of its own"""
    from mnk.visualizer import Visualizer
    b, d, h, w, k = 2, 3, 24, 32, 10
    t = {"source": tricky_frames(1, b, 3, 1, h, w), "video": tricky_frames(2, b, 3, d, h, w),
         "video_prediction": tricky_frames(3, b, 3, d, h, w), "video_deformed": tricky_frames(4, b, 3, d, h, w),
         "kp_source": random_kp(5, b, 1, k), "kp_driving": random_kp(6, b, d, k), "kp_norm": random_kp(7, b, d, k)}
    np.savez(tmp_path / "in.npz", **{n: v.numpy() for n, v in t.items()})
    run = subprocess.run([sys.executable, "-c", _LIVE, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                         capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert run.returncode == 0, run.stderr[-3000:]
    ref = np.load(tmp_path / "out.npz")
    t = {n: be.t(v) for n, v in t.items()}
    out = {"video_prediction": t["video_prediction"], "video_deformed": t["video_deformed"], "kp_source": {"mean": t["kp_source"]},
           "kp_driving": {"mean": t["kp_driving"]}, "kp_norm": {"mean": t["kp_norm"]}}
    vis = Visualizer(kp_size=3, draw_border=True)
    assert_same_bytes(vis.visualize_reconstruction({"source": t["source"], "video": t["video"]}, out), ref["rec"], "live, rec")
    assert_same_bytes(vis.visualize_transfer(t["video"], t["source"], out), ref["tra"], "live, transfer")
