"""mnk.graphs, the package's one hipGraph capture module: the order of begin / end / host calls of a segmented capture and its
exception paths against a recording stub of torch's graph class (no device), the frozen-weight scope, ops.weights_fingerprint;
and on the MI355X the three forms on 64 floats of plain torch arithmetic: warm_up, capture (torch's capture stream and one of
the caller's, live and frozen) and a Segments program with a host call between its two graphs."""
import gc

import pytest
import torch

from mnk import graphs, ops


# ---- against a stub: no device ----------------------------------------------------------------------------------------------------
class StubGraph:
    log = []                         # ("begin" | "end", graph) of every stub, in call order
    end_raises = False

    def capture_begin(self, pool=None):
        assert pool == "pool"
        StubGraph.log.append(("begin", self))

    def capture_end(self):
        StubGraph.log.append(("end", self))
        if StubGraph.end_raises:
            raise RuntimeError("capture_end failed")


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(graphs.torch.cuda, "CUDAGraph", StubGraph)
    monkeypatch.setattr(graphs.torch.cuda, "graph_pool_handle", lambda: "pool")
    monkeypatch.setattr(StubGraph, "log", [])
    monkeypatch.setattr(StubGraph, "end_raises", False)
    monkeypatch.setattr(graphs, "_PARKED", [])
    return StubGraph


def _alternates(log):
    """begin, end, begin, end, ... and every end closes the graph the begin in front of it opened"""
    assert len(log) % 2 == 0
    for (a, ga), (b, gb) in zip(log[0::2], log[1::2]):
        assert (a, b) == ("begin", "end") and ga is gb
    return True


@pytest.mark.parametrize("last", [True, False])
def test_segments_with_two_cuts(stub, last):
    calls = []
    first, second = (lambda: calls.append(1)), (lambda: calls.append(2))
    with graphs.Segments() as seg:
        seg.begin()
        seg.cut(first)
        assert calls == [1]                         # the host call runs during the capture too, between the two graphs
        assert [k for k, _ in stub.log] == ["begin", "end", "begin"]
        seg.cut(second, last=last)
        if seg.open is not None:
            seg.end()
    assert calls == [1, 2]                          # each exactly once
    kinds = [type(p) for p in seg.pieces]
    assert kinds[:4] == [stub, type(first), stub, type(second)] and seg.pieces[1] is first and seg.pieces[3] is second
    assert len(seg.pieces) == (4 if last else 5) and all(k is stub for k in kinds[4:])
    graphs_made = [p for p in seg.pieces if isinstance(p, stub)]
    assert len(set(map(id, graphs_made))) == len(graphs_made) == (2 if last else 3)
    assert _alternates(stub.log) and len(stub.log) == 2 * len(graphs_made)
    assert seg.open is None and graphs._PARKED == []


def test_captured_is_begin_fn_end(stub):
    ran = []
    with graphs.Segments() as seg:
        g = seg.captured(lambda: ran.append([k for k, _ in stub.log]))
    assert ran == [["begin"]] and seg.pieces == [g] and stub.log == [("begin", g), ("end", g)]


@pytest.mark.parametrize("gc_on", [True, False])
def test_exception_in_the_captured_function_ends_the_open_graph(stub, gc_on):
    was_on = gc.isenabled()
    (gc.enable if gc_on else gc.disable)()
    try:
        with pytest.raises(KeyError, match="from the captured function"):
            with graphs.Segments() as seg:
                assert not gc.isenabled()
                seg.captured(lambda: None)
                seg.begin()
                raise KeyError("from the captured function")
        assert gc.isenabled() == gc_on              # re-enabled if it was enabled before, and only then
    finally:
        (gc.enable if was_on else gc.disable)()
    assert _alternates(stub.log) and len(stub.log) == 4          # the open graph got its capture_end
    assert seg.open is None and len(seg.pieces) == 1 and graphs._PARKED == []


def test_a_graph_whose_capture_end_raises_is_parked_and_the_original_exception_propagates(stub):
    was_on = gc.isenabled()
    with pytest.raises(KeyError, match="the original"):
        with graphs.Segments() as seg:
            seg.begin()
            opened = seg.open
            stub.end_raises = True
            raise KeyError("the original")
    assert gc.isenabled() == was_on
    assert graphs._PARKED == [opened] and seg.pieces == []
    assert stub.log == [("begin", opened), ("end", opened)]


def test_no_exception_no_capture_end_from_the_scope(stub):
    """a normal exit ends nothing by itself: the caller ended what it began"""
    with graphs.Segments() as seg:
        seg.captured(lambda: None)
    assert len(stub.log) == 2


def test_frozen_weights_scope():
    assert ops.FROZEN_CAPTURE[0] is False
    with graphs.frozen_weights():
        assert ops.FROZEN_CAPTURE[0] is True
        with graphs.frozen_weights():               # nested: restores the OUTER value
            assert ops.FROZEN_CAPTURE[0] is True
        assert ops.FROZEN_CAPTURE[0] is True
    assert ops.FROZEN_CAPTURE[0] is False
    with pytest.raises(ValueError):
        with graphs.frozen_weights():
            assert ops.FROZEN_CAPTURE[0] is True
            raise ValueError("inside")
    assert ops.FROZEN_CAPTURE[0] is False
    assert ops.handover_state() == {}


def test_weights_fingerprint():
    a, b, other = torch.zeros(4), torch.zeros(3), torch.zeros(5)
    fp = ops.weights_fingerprint([a, b])
    assert fp[2] == ((a._version, a.data_ptr()), (b._version, b.data_ptr())) and len(fp) == 3
    other.add_(1)                                   # a tensor that is not listed
    assert ops.weights_fingerprint([a, b]) == fp    # unchanged
    b.add_(1)                                       # an in-place write
    fp1 = ops.weights_fingerprint([a, b])
    assert fp1 != fp
    version = a._version
    a.data = torch.ones(4)                          # new storage, same version
    assert a._version == version
    fp2 = ops.weights_fingerprint([a, b])
    assert fp2 != fp1 and fp2[:2] == fp1[:2]
    ops.bump_inference_epoch()                      # the pack epoch (optimiser steps, replayed iterations)
    fp3 = ops.weights_fingerprint([a, b])
    assert fp3 != fp2 and fp3[0] != fp2[0] and fp3[1:] == fp2[1:]
    ops.invalidate_packed_weights()                 # the pack epoch again
    fp4 = ops.weights_fingerprint([a, b])
    assert fp4[0] != fp3[0] and fp4[1:] == fp3[1:]
    ops._BN_EVAL_EPOCH[0] += 1                      # what a training-mode norm forward does (running statistics written)
    fp5 = ops.weights_fingerprint([a, b])
    assert fp5[1] != fp4[1] and (fp5[0], fp5[2]) == (fp4[0], fp4[2])
    assert ops.weights_fingerprint([a, b]) == fp5
    assert ops.weights_fingerprint(iter([a, b])) == fp5          # any iterable: module.parameters()


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def hip(make_backend):
    return make_backend("hip")


@pytest.mark.gpu
def test_warm_up_runs_fn_and_joins_the_side_stream(hip):
    x = torch.arange(64, dtype=torch.float32, device="cuda:0")
    acc = torch.zeros(64, device="cuda:0")
    ran, streams = [], []

    def fn():
        ran.append(len(ran))
        streams.append(torch.cuda.current_stream())
        acc.add_(x)
        return acc * 2

    here = torch.cuda.current_stream()
    out = graphs.warm_up(fn, 3)
    assert ran == [0, 1, 2] and torch.cuda.current_stream() == here
    assert all(s != here for s in streams) and len(set(streams)) == 1        # one side stream, not the caller's
    assert torch.equal(out.cpu(), torch.arange(64, dtype=torch.float32) * 6)  # (a copy on the current stream: it waited)
    mine = torch.cuda.Stream()
    assert graphs.warm_up(lambda: torch.cuda.current_stream(), 1, stream=mine) == mine


@pytest.mark.gpu
@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("frozen", [False, True])
def test_capture_replays_on_the_static_input(hip, own_stream, frozen):
    x = torch.ones(64, device="cuda:0")
    seen = []

    def fn():
        seen.append((ops.FROZEN_CAPTURE[0], torch.cuda.is_current_stream_capturing(), torch.cuda.current_stream()))
        return x * 2 + 1

    stream = torch.cuda.Stream() if own_stream else None
    graph, out = graphs.capture(fn, stream=stream, frozen=frozen)
    assert ops.FROZEN_CAPTURE[0] is False
    assert len(seen) == 1 and seen[0][:2] == (frozen, True) and (stream is None or seen[0][2] == stream)
    assert isinstance(graph, torch.cuda.CUDAGraph)
    for v in (3.0, -5.0):
        x.fill_(v)
        graph.replay()
        assert torch.equal(out.cpu(), torch.full((64,), 2 * v + 1))
    assert len(seen) == 1                           # a replay runs no Python


@pytest.mark.gpu
def test_segments_program_with_a_host_call_between_two_graphs(hip):
    x = torch.arange(64, dtype=torch.float32, device="cuda:0")
    count = [0]

    def host_call():
        count[0] += 1

    def run(cut):
        y = x * 2
        cut(host_call)
        return y + 1

    graphs.warm_up(lambda: run(lambda call: call()), 1)
    assert count[0] == 1
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with graphs.Segments() as seg, torch.cuda.stream(cap):
        seg.begin()
        out = run(seg.cut)
        seg.end()
    torch.cuda.current_stream().wait_stream(cap)
    assert count[0] == 2                            # once during the capture
    assert [isinstance(p, torch.cuda.CUDAGraph) for p in seg.pieces] == [True, False, True] and seg.pieces[1] is host_call
    for i in range(2):
        x.copy_(torch.arange(64, dtype=torch.float32) * (i + 3) - 7)
        for piece in seg.pieces:
            piece.replay() if isinstance(piece, torch.cuda.CUDAGraph) else piece()
        assert count[0] == 3 + i                    # once per replay
        got = out.cpu()
        eager = run(lambda call: None)
        assert torch.equal(got, eager.cpu())
