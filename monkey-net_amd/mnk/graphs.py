"""hipGraph capture: the one file of the package that calls torch's capture API.  Every captured program here is the same
sequence -- warm up on a side stream, join it back, synchronise, capture, and leave the stream out of capture mode whatever goes
wrong.  The sites differ in the number of warm-up runs, the stream, whether weights are frozen and when garbage is collected:
they say so in their arguments and keep the rest (snapshots, static buffers, program containers) to themselves."""
import contextlib
import gc

import torch

from . import ops as mops


def warm_up(fn, times, stream=None):
    """`fn()` `times` times on `stream` (None: a fresh side stream), which first waits for the current stream and which the
    current stream waits for afterwards -- also when `fn` raises.  Returns the last result."""
    side = torch.cuda.Stream() if stream is None else stream
    side.wait_stream(torch.cuda.current_stream())
    out = None
    try:
        with torch.cuda.stream(side):
            for _ in range(times):
                out = fn()
    finally:
        torch.cuda.current_stream().wait_stream(side)
    return out


@contextlib.contextmanager
def frozen_weights():
    """A capture inside this scope takes the cached packed weights and evaluation-mode norm coefficients and records their
    addresses instead of re-making them inside the graph (ops.FROZEN_CAPTURE: this is its only writer)."""
    before = mops.FROZEN_CAPTURE[0]
    try:
        mops.FROZEN_CAPTURE[0] = True
        yield
    finally:
        mops.FROZEN_CAPTURE[0] = before


def capture(fn, stream=None, frozen=False):
    """`fn()` captured as one hipGraph on `stream` (None: torch's own capture stream), with frozen_weights() if `frozen`:
    (graph, what fn returned)"""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with frozen_weights() if frozen else contextlib.nullcontext(), torch.cuda.graph(graph, stream=stream):
        out = fn()
    return graph, out


def settle():
    """what torch.cuda.graph() does before a capture, for the sites that begin their graphs by hand, where THEY need it"""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()


_PARKED = []       # graphs whose capture_end raised (their destructor would abort the process: keep them)


class Segments:
    """A program of LINEAR hipGraphs over one memory pool, captured on the caller's current stream, with host calls between them:
    `pieces` lists graphs and host callables in replay order.  A context manager: no garbage collection -- no finaliser -- runs
    inside it, and an exception leaves the stream out of capture mode (the open graph is ended, or parked if that fails too)."""

    def __init__(self):
        self.pool, self.open, self.pieces = torch.cuda.graph_pool_handle(), None, []

    def __enter__(self):
        self._gc_was_on = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, exc_type, exc, tb):
        if self._gc_was_on:
            gc.enable()
        if exc_type is not None and self.open is not None:
            try:
                self.open.capture_end()
            except Exception:
                _PARKED.append(self.open)
            self.open = None

    def begin(self):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(pool=self.pool)
        self.open = g

    def end(self):
        self.open.capture_end()
        self.pieces.append(self.open)
        self.open = None
        return self.pieces[-1]

    def cut(self, host_call, last=False):
        """the open graph ends here; `host_call()` now and between two graphs at every replay (last: nothing that launches follows,
        no further graph is begun)"""
        self.end()
        self.pieces.append(host_call)
        host_call()
        if not last:
            self.begin()

    def captured(self, fn):
        """`fn()` as one graph of its own"""
        self.begin()
        fn()
        return self.end()
