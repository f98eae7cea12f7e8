"""The device-side visualiser at the sizes the reference's loops run it, on the MI355X: byte equality (np.array_equal) with the
numpy restatement of logger.py:97-175 (tests/test_visualizer.py::reference_grid, itself pinned to the recorded reference grids)
at a reconstruction-sized video (32 frames x 64 x 64, 10 key points, batch 1: reconstruction.py:70) and at the batch-32 training
grid (train.py's Logger.visualize_rec: d = 1), and a hipGraph capture of the grid launch."""
import numpy as np
import pytest
import torch

from test_visualizer import (assert_same_bytes, colors_for, random_kp, reconstruction_columns, reference_grid, reference_strip,
                             to_numpy, tricky_frames)

pytestmark = pytest.mark.gpu


def _inputs(b, d, h, w, k, seed, key="video"):
    dev = torch.device("cuda:0")
    inp = {"source": tricky_frames(seed, b, 3, 1, h, w).to(dev), key: tricky_frames(seed + 1, b, 3, d, h, w).to(dev)}
    out = {"video_prediction": tricky_frames(seed + 2, b, 3, d, h, w).to(dev),
           "video_deformed": tricky_frames(seed + 3, b, 3, d, h, w).to(dev),
           "kp_source": {"mean": random_kp(seed + 4, b, 1, k).to(dev)}, "kp_driving": {"mean": random_kp(seed + 5, b, d, k).to(dev)}}
    return inp, out


@pytest.fixture
def hip(make_backend):
    return make_backend("hip")


@pytest.mark.parametrize("kp_size,border", [(2, False), (2, True)])
def test_reconstruction_sized_video_equals_the_restatement(hip, kp_size, border):
    from mnk.visualizer import Visualizer, png_strip
    inp, out = _inputs(1, 32, 64, 64, 10, seed=100)
    got = Visualizer(kp_size=kp_size, draw_border=border).visualize_reconstruction(inp, out)
    want = reference_grid(to_numpy(reconstruction_columns(inp, out)), 32, kp_size, border, colors_for(10).numpy())
    assert got.shape == (32, 64, 5 * 64, 3)
    assert_same_bytes(got, want, "32 x 64 x 64 reconstruction")
    assert_same_bytes(png_strip(out["video_prediction"]), reference_strip(out["video_prediction"].cpu().numpy()), "strip")


@pytest.mark.parametrize("kp_size,border", [(2, False), (3, True)])
def test_batch_32_training_grid_equals_the_restatement(hip, kp_size, border):
    from mnk.visualizer import Visualizer
    inp, out = _inputs(32, 1, 64, 64, 10, seed=200, key="driving")
    got = Visualizer(kp_size=kp_size, draw_border=border).visualize_reconstruction(inp, out)
    want = reference_grid(to_numpy(reconstruction_columns(inp, out)), 1, kp_size, border, colors_for(10).numpy())
    assert got.shape == (1, 32 * 64, 5 * 64, 3)
    assert_same_bytes(got, want, "batch-32 training grid")


def test_grid_launch_is_capturable_and_a_replay_gives_the_same_bytes(hip):
    """the column table travels in the kernel arguments: a captured launch reads the live tensors on every replay"""
    from mnk import ops
    inp, out = _inputs(2, 4, 64, 64, 10, seed=300)
    cols = reconstruction_columns(inp, out)
    colors = colors_for(10).to("cuda:0")
    grid = torch.zeros(4, 2 * 64, 5 * 64, 3, dtype=torch.uint8, device="cuda:0")
    eager = ops.vis_grid(cols, 4, 2, True, colors).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.vis_grid(cols, 4, 2, True, colors, out=grid)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.vis_grid(cols, 4, 2, True, colors, out=grid)
    for _ in range(2):
        grid.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(grid, eager)
    want = reference_grid(to_numpy(cols), 4, 2, True, colors.cpu().numpy())
    assert_same_bytes(grid.cpu().numpy(), want, "replayed grid")
    # new frames and key points in the same tensors: the replay draws them
    inp2, out2 = _inputs(2, 4, 64, 64, 10, seed=400)
    for a, b in zip(reconstruction_columns(inp, out), reconstruction_columns(inp2, out2)):
        if isinstance(a, tuple):
            a[0].copy_(b[0]), a[1].copy_(b[1])
        else:
            a.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    want2 = reference_grid(to_numpy(reconstruction_columns(inp2, out2)), 4, 2, True, colors.cpu().numpy())
    assert not np.array_equal(want, want2)
    assert_same_bytes(grid.cpu().numpy(), want2, "replay after new inputs")
