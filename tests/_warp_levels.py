"""mnk_warp_levels_fwd / _bwd (and the _shared_ forms) on hand-built level tables against fp64 autograd: the tables, the cached
references and the body of the test, shared by test_kernels_motion.py (the power-of-two tables) and
test_kernels_geometry_ratios.py (field, embedding and level sizes off that grid).  Test infrastructure, not a conftest."""
import numpy as np
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr, maxerr, within
from oracle import restate

# (C, h, w, the key-point embedding behind the warp, d input wanted); "decoder": the levels of
# test_all_warps_in_one_launch_equal_the_per_level_launches; "edges": one texel, channel slices (C = 300), a level without d input
WARP_TABLES = {
    "decoder": [(8, 4, 4, True, True), (5, 8, 8, False, True), (4, 16, 16, True, True), (3, 32, 32, False, True)],
    "edges": [(7, 1, 1, True, True), (300, 4, 4, False, True), (5, 8, 8, True, False)],
}
# off the power-of-two grid (test_kernels_geometry_ratios.py).  "odd": non-integer ratios both ways, nothing square;
# "wide-window": up-ratios 9 ... 17 from the embedding (the second 16-pixel step of the bilinear embedding gradient) and a
# one-texel level; "down": every level smaller than field and embedding; "float-index": size pairs at which
# floorf(dst * (float)in / (float)out) is not floor(dst * in / out) -- (26,22) (14,46) (62,14) (39,33) of the embedding and field
WARP_TABLES_RATIOS = {
    "odd": [(8, 3, 2, True, True), (5, 6, 5, False, True), (4, 12, 10, True, True), (3, 25, 21, True, True)],
    "wide-window": [(4, 37, 41, True, True), (8, 9, 50, True, True), (3, 1, 1, True, True)],
    "down": [(4, 7, 5, True, True), (8, 13, 13, True, False), (3, 1, 2, True, True)],
    "float-index": [(4, 22, 46, True, True), (4, 14, 33, True, True)],
}
# table: ((hf, wf) of the field, (He, We) of the embedding); the power-of-two tables: a 16 x 16 field, an 8 x 8 embedding
WARP_GEOMETRY = {"odd": ((12, 10), (5, 7)), "wide-window": ((4, 5), (4, 3)), "down": ((30, 27), (33, 29)),
                 "float-index": ((26, 14), (62, 39))}
PROJECT_BOUND = 1e-5          # test_deform's tolerance
_WARP_REFS = {}


def identity_field(hf, wf):
    """restate.make_coordinate_grid with 0 (the centre) along an axis of one texel, where its 0 / 0 is NaN"""
    return torch.nan_to_num(restate.make_coordinate_grid(hf, wf), nan=0.0)


def resize_embedding(e4, h, w, name):
    """generator.py:72 on a depth of one: F.interpolate(emb, size=(d, h, w), mode); the nearest pick in the reference's fp32
    arithmetic for every dtype (restate.nearest_index)"""
    if name == "nearest":
        return e4[:, :, restate.nearest_index(e4.shape[2], h)][:, :, :, restate.nearest_index(e4.shape[3], w)]
    return F.interpolate(e4.unsqueeze(2), size=(1, h, w), mode=name)[:, :, 0]


def _autograd(dtype, name, frames, field, emb, inps, douts, levels):
    n, hf, wf = field.shape[:3]
    f = torch.cat([field, torch.zeros(n, hf, wf, 1)], -1).view(n, 1, hf, wf, 3).to(dtype).requires_grad_(True)
    e = emb.to(dtype).requires_grad_(True)
    xs = [x.to(dtype).requires_grad_(True) for x in inps]
    outs = []
    for x, (c, h, w, ke, _) in zip(xs, levels):
        rep = x.repeat_interleave(frames, dim=0) if frames > 1 else x
        o = restate.deform_input(rep.unsqueeze(2), f, name)[:, :, 0]
        if ke:
            o = torch.cat([o, resize_embedding(e, h, w, name)], 1)
        outs.append(o)
    torch.autograd.backward(outs, [d.to(dtype) for d in douts])
    return dict(outs=[o.detach() for o in outs], dinps=[x.grad for x in xs], dfield=f.grad[:, 0, :, :, :2], demb=e.grad)


def warp_case(table, mode, with_emb, frames=1):
    """inputs of the levels (test_deform's kinds: uniform images, identity + 0.4 * noise field) and fp64 autograd through
    restate.deform_input and the resized embedding (generator.py:60-78), cached for the parameters that share it.  frames > 1:
    field, embedding and gradient rows v * frames + f belong to source image v.  The tables off the power-of-two grid also get
    the same autograd in fp32 (key "ref32"): the rounding of the reference's own arithmetic at these sizes."""
    key = (table, mode, with_emb, frames)
    if key not in _WARP_REFS:
        g = torch.Generator().manual_seed(16)
        (hf, wf), (he, we) = WARP_GEOMETRY.get(table, ((16, 16), (8, 8)))
        sources = 2 if frames == 1 else 1
        n, emb_ch = sources * frames, 6
        name = "nearest" if mode == 0 else "trilinear"
        field = identity_field(hf, wf).view(1, hf, wf, 2).repeat(n, 1, 1, 1) + 0.4 * torch.randn(n, hf, wf, 2, generator=g)
        emb = torch.randn(n, emb_ch, he, we, generator=g)
        rows = WARP_TABLES[table] if table in WARP_TABLES else WARP_TABLES_RATIOS[table]
        levels = [(c, h, w, emb_ch if (k and with_emb) else 0, di) for c, h, w, k, di in rows]
        inps = [torch.rand(sources, c, h, w, generator=g) for c, h, w, _, _ in levels]
        douts = [torch.randn(n, c + ke, h, w, generator=g) for c, h, w, ke, _ in levels]
        r = dict(n=n, sources=sources, frames=frames, hf=hf, wf=wf, he=he, we=we, emb_ch=emb_ch, levels=levels, field=field,
                 emb=emb, inps=inps, douts=douts)
        r.update(_autograd(torch.float64, name, frames, field, emb, inps, douts, levels))
        if table in WARP_TABLES_RATIOS:
            r["ref32"] = _autograd(torch.float32, name, frames, field, emb, inps, douts, levels)
        _WARP_REFS[key] = r
    return _WARP_REFS[key]


def run_warp_levels(be, table, mode, want, frames=1):
    """mnk_warp_levels_fwd / _bwd with hand-built level tables whose buffers are all guard-banded, directly against fp64
    autograd (tolerances of test_deform): every channel of every out_l written (pad channels 0), d input written with pad
    channels 0 (or absent), d field summed over the levels, d embedding over the levels that carry it; emb / dfield / demb
    NULL in turn.  The tables' pointers are host data the guarded call cannot see: inputs are compared with copies, the
    guards checked after the launches.  A table that carries "ref32" is held to max(1e-5, 4 x the fp32 reference's own error
    against fp64) per output, with the same metric; the others to 1e-5.  Returns [(what, error, e_ref)]."""
    from test_multiframe_kernels import WARP_LEVEL
    r = warp_case(table, mode, want != "no-emb", frames)
    n, hf, wf, he, we, emb_ch, levels = r["n"], r["hf"], r["wf"], r["he"], r["we"], r["emb_ch"], r["levels"]
    sources, r32 = r["sources"], r.get("ref32")
    with_emb = want != "no-emb"
    lde = ceil4(emb_ch) if with_emb else 0
    FL = be.t(r["field"])
    EMB = be.t(to_nhwc(r["emb"])) if with_emb else None
    XS = [be.t(to_nhwc(x)) for x in r["inps"]]
    DOS = [be.t(to_nhwc(d)) for d in r["douts"]]
    OUTS = [be.empty(n, h, w, ceil4(c + ke)) for c, h, w, ke, _ in levels]
    DIS = [be.empty(sources, h, w, ceil4(c)) if di else None for c, h, w, _, di in levels]
    lv = np.zeros(len(levels), dtype=WARP_LEVEL)
    for i, (c, h, w, ke, _) in enumerate(levels):
        lv[i] = (XS[i].data_ptr(), OUTS[i].data_ptr(), DOS[i].data_ptr(), DIS[i].data_ptr() if DIS[i] is not None else 0,
                 XS[i].shape[-1], c, h, w, OUTS[i].shape[-1], ke, c, 0)
    keep = [t.clone() for t in XS + DOS]
    h_e, w_e = (he, we) if with_emb else (0, 0)
    sfx, tail = ("_shared", (n, frames)) if frames > 1 else ("", (n,))
    be.call("mnk_warp_levels%s_fwd" % sfx, lv.ctypes.data, len(levels), FL, hf, wf, mode, EMB, lde, h_e, w_e, *tail)
    nws = be.query("mnk_warp_levels_bwd_workspace_floats", lv.ctypes.data, len(levels), n)
    assert nws > 0
    DF = be.empty(n, hf, wf, 2) if want != "no-dfield" else None
    DE = be.empty(n, he, we, lde) if with_emb and want != "no-demb" else None
    be.call("mnk_warp_levels%s_bwd" % sfx, lv.ctypes.data, len(levels), FL, hf, wf, mode, DF, DE, lde, h_e, w_e, *tail,
            be.empty(nws), nws)
    be.sync()
    be.check_all("after the launches")
    for t, k in zip(XS + DOS, keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), "an input named in the level table was written"
    figures = []

    def ok(what, metric, got, ref64, ref32):
        good, err, e_ref = within("warp-levels %s mode %d %s %s [%s]" % (table, mode, want, what, be.kind), metric, got, ref64,
                                  ref32, PROJECT_BOUND)
        figures.append((what, err, e_ref))
        return good

    for i, ((c, h, w, ke, di), O, DI, ro, rdi) in enumerate(zip(levels, OUTS, DIS, r["outs"], r["dinps"])):
        o = O.cpu()
        assert ok("out%d" % i, maxerr, from_nhwc(o, c + ke), ro, r32["outs"][i] if r32 else None), (c, h, w)
        assert torch.all(o[..., c + ke:] == 0), (c, h, w)
        if di:
            d = DI.cpu()
            assert torch.all(d[..., c:] == 0), (c, h, w)
            assert ok("dinp%d" % i, relerr, from_nhwc(d, c), rdi, r32["dinps"][i] if r32 else None), (c, h, w)
    if DF is not None:
        assert ok("dfield", relerr, DF.cpu(), r["dfield"], r32["dfield"] if r32 else None)
    if DE is not None:
        de = DE.cpu()
        assert torch.all(de[..., emb_ch:] == 0)
        assert ok("demb", relerr, from_nhwc(de, emb_ch), r["demb"], r32["demb"] if r32 else None)
    return figures
