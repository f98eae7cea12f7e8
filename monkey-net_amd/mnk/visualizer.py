"""The reference's `logger.Visualizer` (logger.py:91-175) and the PNG strip of its evaluation loops on the device.

The reference copies four to six fp32 videos to the host, transposes them, rasterises every key point of every frame with
`skimage.draw.circle` in a Python loop, concatenates and converts to uint8.  Here the videos stay on the device; ONE launch
(`mnk_vis_grid`, csrc/visualizer.hip) reads every column through its own strides -- the repeated source frame, first driving
frame and source key points are stride-0 columns, never materialised -- and writes the uint8 grid, the only bytes that cross
PCIe.  Same constructor, same method arguments, same numpy uint8 array (shape and every byte) as the reference.

    from mnk.visualizer import Visualizer           # instead of `from logger import Visualizer`

or, for the reference's own scripts under run_reference.py, MNK_NATIVE_VISUALIZER=1."""
import os

import numpy as np
import torch

from . import ops

_LUT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gist_rainbow_lut.txt")
_LUTS = {}


def _gist_rainbow_lut():
    """the 256 x 3 float64 look-up table of matplotlib's 'gist_rainbow' (tools/make_golden_visualizer.py --lut wrote it from the
    installed matplotlib; tests/test_visualizer.py compares it with the live one where matplotlib is importable)"""
    if "gist_rainbow" not in _LUTS:
        with open(_LUT_FILE) as f:          # one entry per line: R G B as float64 repr (exact round trip)
            lut = np.array([[float(x) for x in line.split()] for line in f if not line.startswith("#")], dtype=np.float64)
        assert lut.shape == (256, 3)
        _LUTS["gist_rainbow"] = lut
    return _LUTS["gist_rainbow"]


def keypoint_colors(colormap, num_kp):
    """(num_kp, 3) float32: `np.array(colormap(k / num_kp))[:3]` as it lands in a float32 frame (logger.py:105).  `colormap`:
    'gist_rainbow' (the shipped table: matplotlib maps a float x in [0, 1) to lut[int(x * 256)]) or a matplotlib colormap
    object."""
    if isinstance(colormap, str):
        lut = _gist_rainbow_lut()
        return np.stack([lut[int(k / num_kp * 256)] for k in range(num_kp)]).astype(np.float32).reshape(num_kp, 3)
    return np.array([np.array(colormap(k / num_kp))[:3] for k in range(num_kp)], dtype=np.float64).astype(np.float32) \
        .reshape(num_kp, 3)


class Visualizer:
    def __init__(self, kp_size=2, draw_border=False, colormap='gist_rainbow'):
        self.kp_size = kp_size
        self.draw_border = draw_border
        if colormap == 'gist_rainbow':
            self.colormap = colormap
        else:
            try:
                import matplotlib.pyplot as plt
            except ImportError as e:
                raise ImportError("mnk.visualizer ships the colour table of 'gist_rainbow' only; colormap %r needs matplotlib, "
                                  "which is not importable here (%s)" % (colormap, e)) from e
            self.colormap = plt.get_cmap(colormap)
        self._colors = {}

    def colors(self, num_kp, device):
        key = (num_kp, str(device))
        if key not in self._colors:
            self._colors[key] = torch.from_numpy(keypoint_colors(self.colormap, num_kp)).to(device)
        return self._colors[key]

    def create_image_grid(self, *args, as_tensor=False):
        """logger.py:119-126 on (B, 3, d | 1, H, W) DEVICE tensors (not the reference's transposed numpy arrays): each argument is
        a video or a `(video, kp_mean)` tuple; a one-frame video / key-point tensor is repeated over the d frames of the others.
        Returns uint8 (d, B * H, ncol * W, 3) values in [0, 255] -- the reference's grid after its `(255 * image).astype(np.uint8)`."""
        cols = [a if isinstance(a, tuple) else (a, None) for a in args]
        dev = next((v.device for v, _ in cols if v.is_cuda), cols[0][0].device)
        cols = [(v.detach().to(dev), None if k is None else k.detach().to(dev)) for v, k in cols]
        d = max(v.shape[2] for v, _ in cols)
        num_kp = next((k.shape[2] for _, k in cols if k is not None), 0)
        grid = ops.vis_grid(cols, d, self.kp_size, self.draw_border, self.colors(num_kp, dev) if num_kp else None)
        return grid if as_tensor else grid.cpu().numpy()

    def visualize_transfer(self, driving_video, source_image, out, as_tensor=False):
        """logger.py:128-152"""
        prediction = out['video_prediction']
        kp_driving = out['kp_driving']['mean']
        return self.create_image_grid((_one_frame(source_image[:, :, 0:1], "source_image"), out['kp_source']['mean']),
                                      (driving_video[:, :, 0:1], kp_driving[:, :1]),
                                      (driving_video, kp_driving),
                                      (prediction, out['kp_norm']['mean']), prediction, out['video_deformed'],
                                      as_tensor=as_tensor)

    def visualize_reconstruction(self, inp, out, as_tensor=False):
        """logger.py:154-175"""
        prediction = out['video_prediction']
        gt = inp['driving'] if 'driving' in inp else inp['video']
        return self.create_image_grid((_one_frame(inp['source'], "inp['source']"), out['kp_source']['mean']),
                                      (gt, out['kp_driving']['mean']), prediction, out['video_deformed'], gt,
                                      as_tensor=as_tensor)


def _one_frame(video, what):
    if video.shape[2] != 1:
        raise ValueError("%s must hold one frame (the reference repeats it over the frames of the prediction), got %d"
                         % (what, video.shape[2]))
    return video


def png_strip(video, as_tensor=False):
    """The uint8 (H, D * W, 3) frame strip the evaluation loops save as .png (reconstruction.py:66-68, prediction.py:137-139:
    video 0 of the batch, frames side by side).  video: (B, 3, D, H, W) -- video 0 is taken -- or (3, D, H, W), float32."""
    v = video.detach()
    strip = ops.frames_to_strip(v[0] if v.dim() == 5 else v)
    return strip if as_tensor else strip.cpu().numpy()
