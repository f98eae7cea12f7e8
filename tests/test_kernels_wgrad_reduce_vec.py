"""The vector thread maps of mnk_wgrad_reduce_multi ("wgrad_reduce_vec" = 1: every global load a float4) against the maps
they replace ("wgrad_reduce_vec" = 0: the flat and the tile map), on made-up partials.  Only which lane loads what differs --
the sum of a gradient element keeps its groups, its two chains per group and their order -- so the two runs must leave the
same BITS in the whole gradient buffer, columns of other sources and the gaps between layers included."""
import numpy as np
import pytest
import torch

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_kernels_optim import REDUCE_DESC, _table

SPLITS = (1, 2, 3, 4, 5, 31, 32, 33, 67)                # 4 and 32: the thresholds between 1, 4 and 16 thread groups
SHAPES = ((5, 8), (9, 12), (13, 3), (16, 16), (45, 45), (33, 20), (6, 66))      # (Cout, C)
FORMS = ((0, 9), (0, 16), (1, 9), (1, 16), (2, 9))      # (layout, gradient taps); layout 2 reads 16 pseudo taps
MAP_FLAT, MAP_TILE, MAP_VEC_TAP, MAP_VEC_PARAM = 0, 1, 2, 3


def _cases():
    out = []
    for layout, nt in FORMS:
        for splits in SPLITS:
            for cout, c in SHAPES:
                c_start = 3 if len(out) % 2 else 0       # unaligned slices of a wider gradient: Cin_total > C either way
                out.append((layout, nt, splits, cout, c, c_start, c + c_start + 2))
    return out


def _set_vec(be, v):
    be.lib.call("mnk_set_tuning", b"wgrad_reduce_vec", v)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_vector_maps_leave_the_bits_of_the_flat_and_tile_maps(be, accumulate):
    cases = _cases()
    g = torch.Generator().manual_seed(77)
    # every layer reads a prefix of ONE buffer of random partials (inputs only; 16-byte aligned)
    need = max(s * (16 if lay == 2 else nt) * co * c for lay, nt, s, co, c, _, _ in cases)
    P = be.t(torch.randn(need, generator=g))
    # ... and owns a (Cout, Cin_total, taps) piece of ONE gradient buffer, an odd number of floats after the piece before it
    offs, total = [], 1
    for lay, nt, s, co, c, c_start, cin_total in cases:
        offs.append(total)
        total += co * cin_total * nt + 1 + 2 * (len(offs) % 2)
    init = torch.randn(total, generator=g) if accumulate else torch.full((total,), float("nan"))
    try:
        _set_vec(be, 0)
        old_maps = [be.query("mnk_wgrad_reduce_map", lay, s, nt, co, c) for lay, nt, s, co, c, _, _ in cases]
        _set_vec(be, 1)
        new_maps = [be.query("mnk_wgrad_reduce_map", lay, s, nt, co, c) for lay, nt, s, co, c, _, _ in cases]
        # the case list reaches each new map, in every class of the tap-major one, and the layers that keep the old maps
        assert set(old_maps) == {MAP_FLAT, MAP_TILE}
        assert all(n == o or (o == MAP_TILE and n in (MAP_VEC_TAP, MAP_VEC_PARAM)) for o, n in zip(old_maps, new_maps))
        taken = {}
        for (lay, nt, s, co, c, _, _), m in zip(cases, new_maps):
            taken.setdefault(m, set()).add((lay, nt, 1 if s < 4 else (4 if s < 32 else 16)))
        assert set(taken) == {MAP_FLAT, MAP_TILE, MAP_VEC_TAP, MAP_VEC_PARAM}, sorted(taken)
        # (the sub-pixel form with four thread groups measured slower on the vector map and keeps the tile map)
        assert taken[MAP_VEC_TAP] == {(lay, nt, G) for lay, nt in FORMS if lay != 1 for G in (1, 4, 16)} - {(2, 9, 4)}, taken[MAP_VEC_TAP]
        assert (2, 9, 4) in taken[MAP_TILE]
        # (nine taps with fewer than four splits: C * 9 % 4 == 0 means C % 4 == 0, the flat map's layers)
        assert taken[MAP_VEC_PARAM] == {(1, nt, G) for nt in (9, 16) for G in (1, 4, 16)} - {(1, 9, 1)}, taken[MAP_VEC_PARAM]
        assert {lay for lay, _, _ in taken[MAP_TILE]} == {0, 1, 2}          # ragged planes fall back, in every layout
        for (lay, nt, s, co, c, _, _), m in zip(cases, new_maps):
            if (co, c) == (45, 45) and lay != 1:
                assert m == MAP_TILE                                         # 2025-float planes are not 16-byte aligned
        got = []
        for vec in (0, 1):
            _set_vec(be, vec)
            DW = be.t(init.clone())
            rows, blocks = [], 0
            for (lay, nt, s, co, c, c_start, cin_total), off in zip(cases, offs):
                rows.append((P.data_ptr(), DW.data_ptr() + 4 * off, lay, s, nt, co, c, cin_total, c_start, accumulate, blocks, 0))
                blocks += be.query("mnk_wgrad_reduce_blocks", s, co, c)      # (the same count under either value)
            rec = np.array(rows, dtype=REDUCE_DESC)
            be.call("mnk_wgrad_reduce_multi", _table(be, rec), len(rec), blocks)
            be.sync()
            got.append(DW.cpu())
    finally:
        _set_vec(be, 1)
    ref, new = got
    assert torch.equal(ref.view(torch.int32), new.view(torch.int32)), \
        [cases[i] for i, off in enumerate(offs)
         if not torch.equal(ref[off:off + 1 + cases[i][3] * cases[i][6] * cases[i][1]].view(torch.int32),
                            new[off:off + 1 + cases[i][3] * cases[i][6] * cases[i][1]].view(torch.int32))][:8]
    # what neither run may touch: other sources' columns and the floats between the layers; what both must write: the slice
    written = torch.zeros(total, dtype=torch.bool)
    for (lay, nt, s, co, c, c_start, cin_total), off in zip(cases, offs):
        written[off:off + co * cin_total * nt].view(co, cin_total, nt)[:, c_start:c_start + c] = True
    assert torch.equal(new.view(torch.int32)[~written], init.view(torch.int32)[~written])
    assert bool(torch.isfinite(new[written]).all())
    # the values themselves, for one layer on each new map (the old maps are tested against fp64 sums in test_kernels_optim.py)
    for want_map in (MAP_VEC_TAP, MAP_VEC_PARAM):
        i = max(k for k, m in enumerate(new_maps) if m == want_map and cases[k][0] != 2)
        lay, nt, s, co, c, c_start, cin_total = cases[i]
        part = P.cpu()[:s * nt * co * c].double()
        part = part.view(s, co, c, nt) if lay == 1 else part.view(s, nt, co, c).permute(0, 2, 3, 1)
        have = new[offs[i]:offs[i] + co * cin_total * nt].view(co, cin_total, nt)[:, c_start:c_start + c].double()
        base = init[offs[i]:offs[i] + co * cin_total * nt].view(co, cin_total, nt)[:, c_start:c_start + c].double()
        base = base if accumulate else torch.zeros_like(base)
        # any order of n fp32 additions is within (n - 1) u sum|x| (1 + O(n u)) of the exact sum, u = 2^-24; n = splits + 2
        # counts the 0.f a chain starts from and dw
        bound = (s + 2) * 2.0 ** -24 * (part.abs().sum(0) + base.abs())
        assert bool(((have - (part.sum(0) + base)).abs() <= bound).all()), cases[i]


def test_unaligned_partials_keep_the_tile_map_and_its_bits(be):
    """`part` one float past a 16-byte boundary: the vector maps do not apply (their contract is aligned partials), the kernel
    must notice by itself -- mnk_wgrad_reduce_map sees no pointer -- and sum such layers with the tile map: the same bits under
    either tuning value, and no float4 read of an unaligned address (a fault on the device)."""
    cases = [(lay, nt, s, co, c, 3, c + 5) for lay, nt in FORMS for s in (2, 5, 33) for co, c in ((9, 12), (6, 66))]
    g = torch.Generator().manual_seed(78)
    need = max(s * (16 if lay == 2 else nt) * co * c for lay, nt, s, co, c, _, _ in cases)
    P = be.t(torch.randn(need + 1, generator=g))
    offs, total = [], 0
    for lay, nt, s, co, c, c_start, cin_total in cases:
        offs.append(total)
        total += co * cin_total * nt
    init = torch.full((total,), float("nan"))
    got = []
    try:
        for vec in (0, 1):
            _set_vec(be, vec)
            DW = be.t(init.clone())
            rows, blocks = [], 0
            for (lay, nt, s, co, c, c_start, cin_total), off in zip(cases, offs):
                rows.append((P.data_ptr() + 4, DW.data_ptr() + 4 * off, lay, s, nt, co, c, cin_total, c_start, 0, blocks, 0))
                blocks += be.query("mnk_wgrad_reduce_blocks", s, co, c)
            rec = np.array(rows, dtype=REDUCE_DESC)
            be.call("mnk_wgrad_reduce_multi", _table(be, rec), len(rec), blocks)
            be.sync()
            got.append(DW.cpu())
        assert {be.query("mnk_wgrad_reduce_map", lay, s, nt, co, c) for lay, nt, s, co, c, _, _ in cases} >= {MAP_VEC_TAP, MAP_VEC_PARAM}
    finally:
        _set_vec(be, 1)
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    lay, nt, s, co, c, c_start, cin_total = cases[2]            # (and the values: layout 0, nine taps, 33 splits)
    part = P.cpu()[1:1 + s * nt * co * c].double().view(s, nt, co, c).permute(0, 2, 3, 1)
    have = got[1][offs[2]:offs[2] + co * cin_total * nt].view(co, cin_total, nt)[:, c_start:c_start + c].double()
    assert bool(((have - part.sum(0)).abs() <= (s + 2) * 2.0 ** -24 * part.abs().sum(0)).all())
