"""mnk_kp_anchor_update / mnk_kp_normalize_anchored (transfer.py:31-62 for a driving video that arrives in pieces): the first
frame's key-points live in anchor buffers behind a device flag.

a. a video normalised piece by piece equals mnk_kp_normalize on the whole video, bit for bit (one kernel serves both entries);
b. the update fills the anchor once: frame 0, the hull area of [0, 0], flag = 1; a second update changes nothing; a cleared flag
   anchors again;
c. the rejected argument combinations raise and write nothing.
Guard-banded buffers (tests/_guard.py); inputs from oracle.cases.random_kp."""
import itertools

import pytest
import torch

from oracle import cases
from _guard import be  # noqa: F401  (the guard-banded backend fixture)


def bits(t):
    return t.contiguous().cpu().view(torch.int32)


def _kp(B, D, K, seed):
    kp = cases.random_kp(B, D, K, seed)
    return kp["mean"].contiguous(), kp["var"].reshape(B, D, K, 4).contiguous()


def _flag(be):
    f = be.empty_int(1)
    f.zero_()
    return f


SPLITS = [((3, 7, 5), [7]), ((3, 7, 5), [1, 2, 4]), ((3, 7, 5), [1] * 7), ((9, 2, 32), [1, 1]), ((2, 3, 3), [2, 1])]


@pytest.mark.parametrize("shape,splits", SPLITS, ids=["%dx%dx%d-%s" % (s + ("+".join(map(str, p)),)) for s, p in SPLITS])
def test_pieces_equal_the_whole_video_bit_for_bit(be, shape, splits):
    """every move_location / clip_mean / adapt_variance combination mnk_kp_normalize accepts x with / without covariances (not with
    adapt_variance) x with / without hull areas.  9 x 32 = 288 (b, k) pairs exceed one 256-thread pass of the update block."""
    B, D, K = shape
    assert sum(splits) == D
    mv, vv = _kp(B, D, K, seed=3)
    ma, va = _kp(B, 1, K, seed=4)
    MV, VV, MA, VA = be.t(mv), be.t(vv), be.t(ma), be.t(va)
    area_a, area_v = be.empty(1), be.empty(1)
    be.call("mnk_kp_hull_area", MA, K, area_a)
    be.call("mnk_kp_hull_area", MV, K, area_v)
    edges = [0] + list(itertools.accumulate(splits))
    pieces = [(be.t(mv[:, s:e]), be.t(vv[:, s:e]), e - s) for s, e in zip(edges[:-1], edges[1:])]
    ran = 0
    for ml, cm, av in itertools.product((0, 1), repeat=3):
        for with_var, areas in itertools.product((True, False), repeat=2):
            if av and not with_var:
                continue
            WM, WV = be.empty(B, D, K, 2), (be.empty(B, D, K, 4) if with_var else None)
            be.call("mnk_kp_normalize", MV, VV if with_var else None, MA, VA if with_var else None, B, D, K, area_a if areas else None,
                    area_v if areas else None, ml, cm, av, WM, WV)
            AM, AV_, AA, F = be.empty(B, K, 2), (be.empty(B, K, 4) if with_var else None), be.empty(1), _flag(be)
            got_m, got_v = [], []
            for PM, PV, n in pieces:
                be.call("mnk_kp_anchor_update", PM, PV if with_var else None, B, n, K, int(areas), AM, AV_, AA if areas else None, F)
                OM, OV = be.empty(B, n, K, 2), (be.empty(B, n, K, 4) if with_var else None)
                be.call("mnk_kp_normalize_anchored", PM, PV if with_var else None, AM, AV_, MA, VA if with_var else None, B, n, K,
                        area_a if areas else None, AA if areas else None, ml, cm, av, OM, OV)
                got_m.append(OM)
                got_v.append(OV)
            be.sync()
            assert not torch.isnan(WM.cpu()).any()
            assert torch.equal(bits(torch.cat(got_m, dim=1)), bits(WM)), (ml, cm, av, with_var, areas)
            if with_var:
                assert torch.equal(bits(torch.cat(got_v, dim=1)), bits(WV)), (ml, cm, av, with_var, areas)
            if areas:
                assert torch.equal(bits(AA), bits(area_v))
            assert int(F.cpu()[0]) == 1
            ran += 1
    assert ran == 24


@pytest.mark.parametrize("B,D,K", [(3, 7, 5), (9, 2, 32)])
def test_anchor_update_fills_the_anchor_once(be, B, D, K):
    mv, vv = _kp(B, D, K, seed=5)
    mv2, vv2 = _kp(B, D, K, seed=6)
    MV, VV, MV2, VV2 = be.t(mv), be.t(vv), be.t(mv2), be.t(vv2)
    AM, AV, AA, F = be.empty(B, K, 2), be.empty(B, K, 4), be.empty(1), _flag(be)
    area, area2 = be.empty(1), be.empty(1)
    be.call("mnk_kp_hull_area", MV, K, area)                     # [0, 0]: the first K points of the buffer
    be.call("mnk_kp_hull_area", MV2, K, area2)
    assert not torch.equal(bits(area), bits(area2))

    def holds(m, v, a):
        be.sync()
        assert torch.equal(bits(AM), bits(m[:, 0])) and torch.equal(bits(AV), bits(v[:, 0]))
        assert torch.equal(bits(AA), bits(a)) and int(F.cpu()[0]) == 1

    be.call("mnk_kp_anchor_update", MV, VV, B, D, K, 1, AM, AV, AA, F)
    holds(mv, vv, area)
    be.call("mnk_kp_anchor_update", MV2, VV2, B, D, K, 1, AM, AV, AA, F)        # anchored: nothing is written
    holds(mv, vv, area)
    F.zero_()
    be.call("mnk_kp_anchor_update", MV2, VV2, B, D, K, 1, AM, AV, AA, F)        # a cleared flag anchors again
    holds(mv2, vv2, area2)
    # means only, no area: the other buffers are not touched
    AM2, F2 = be.empty(B, K, 2), _flag(be)
    be.call("mnk_kp_anchor_update", MV, None, B, D, K, 0, AM2, None, None, F2)
    be.sync()
    assert torch.equal(bits(AM2), bits(mv[:, 0])) and int(F2.cpu()[0]) == 1


def test_rejected_arguments_raise_and_write_nothing(be):
    from mnk._lib import MnkError
    B, D = 2, 3
    for K in (2, 5, 33):
        mv, vv = _kp(B, D, K, seed=7)
        ma, va = _kp(B, 1, K, seed=8)
        MV, VV, MA, VA = be.t(mv), be.t(vv), be.t(ma), be.t(va)
        AM, AV, AA, F = be.empty(B, K, 2), be.empty(B, K, 4), be.empty(1), _flag(be)
        MO, VO = be.empty(B, D, K, 2), be.empty(B, D, K, 4)
        bad_updates = [(MV, VV, B, D, K, 0, AM, AV, None, None)]                # no flag
        if K == 5:
            bad_updates.append((MV, VV, B, D, K, 1, AM, AV, None, F))           # want_area without anchor_area
            bad_updates.append((MV, None, B, D, K, 0, AM, AV, None, F))         # an anchor for covariances that are not given
        else:
            bad_updates.append((MV, VV, B, D, K, 1, AM, AV, AA, F))             # want_area with K outside 3..32
        for args in bad_updates:
            with pytest.raises(MnkError):
                be.call("mnk_kp_anchor_update", *args)
        bad_norm = [(MV, VV, AM, None, MA, VA, B, D, K, None, None, 1, 0, 1, MO, VO),      # adapt_variance without anchor_var
                    (MV, VV, AM, AV, MA, VA, B, D, K, AA, None, 1, 0, 0, MO, VO),          # one area without the other
                    (MV, VV, AM, AV, MA, VA, B, D, K, None, None, 1, 0, 1, MO, None),      # adapt_variance without an output
                    (MV, VV, None, AV, MA, VA, B, D, K, None, None, 1, 0, 0, MO, VO)]      # no anchor
        for args in bad_norm:
            with pytest.raises(MnkError):
                be.call("mnk_kp_normalize_anchored", *args)
        be.sync()
        for t in (AM, AV, AA, MO, VO):
            assert torch.isnan(t.cpu()).all()
        assert int(F.cpu()[0]) == 0
