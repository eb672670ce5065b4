"""-m gpu: the cross entropy + Dice / Jaccard / Tversky region term (csrc/ce_region.hip) through the C ABI
(vmtl_ce_region_fwd / vmtl_ce_region_bwd) and through the node (ops.segm_region_loss[_with_argmax]) against the fp64
oracle of tests/region_oracle.py, every launch under poison.patched("guard") and launch_guard.patched().

Bounds.  Loss and both terms within 1e-5 absolute and the gradient within 1e-5 of its magnitude: the bounds of
tests/test_loss_ignore_gpu.py for the same softmax arithmetic.  The term adds fp64 sums of fp32 probabilities (each
within a few fp32 ulps of its fp64 value, so the class sums keep a relative error of a few 2^-24) and 2C coefficients
rounded to fp32 once; every present class of the cases has D_c >= 1.2 (asserted in tests/test_region_loss_cpu.py), so
T_c, a_c and b_c inherit that relative error unamplified - the coefficient table is held to 1e-5 of its magnitude too.
Exact: the counts, the zeros of an absent class, the +0.0f rows of void pixels, the argmax, the written lanes, and two
runs of the same launch."""
import contextlib

import pytest
import torch

from tests import launch_guard, poison, region_oracle as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GOUT = R.GOUT


def _ops():
    from vision_mtl_amd import ops

    return ops


def _ceil4(c):
    return (c + 3) // 4 * 4


def _bits(x):
    return x.contiguous().view(torch.int32)


@contextlib.contextmanager
def _guarded():
    with poison.patched("guard") as p, launch_guard.patched():
        yield p


def _abi(dev, z, t, w, ign, setting, cw=1.0, rw=1.0, ld=None, nchw=False, want_argmax=False, backward=True):
    """vmtl_ce_region_fwd + vmtl_ce_region_bwd on device tensors; the gradient in NHWC rows of `ld` floats (default: the
    node's ceil4(C+1)) or NCHW, in a sentinel-filled buffer.  Everything comes back as it was written, on the device."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    al, be, sm = setting
    B, C, H, W = z.shape
    HW, P = H * W, B * H * W
    loss, terms, stats, coef = (torch.empty(s, device=dev) for s in ((), (2,), (2,), (2 * C,)))
    counts = torch.empty(C + 1, dtype=torch.int64, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_argmax else None
    ws = torch.empty(lib().raw("vmtl_ce_region_workspace_bytes")(P, C) // 8, dtype=torch.float64, device=dev)
    ign = ops.NO_IGNORE if ign is None else ign
    dims = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    ops._k("vmtl_ce_region_fwd", logits=z, target=t, weight=w, ignore_index=ign, alpha=al, beta=be, smooth=sm,
           ce_weight=cw, region_weight=rw, loss=loss, terms=terms, stats=stats, coef=coef, counts=counts, workspace=ws,
           argmax=pred, **dims)
    out = dict(loss=loss, terms=terms, stats=stats, coef=coef, counts=counts, pred=pred)
    if not backward:
        return out
    if nchw:
        d = torch.empty(B, C, H, W, device=dev)
        ds = dict(dsb=C * HW, dsc=HW, dsp=1)
    else:
        ld = _ceil4(C + 1) if ld is None else ld
        d = torch.empty(B, H, W, ld, device=dev)
        ds = dict(dsb=HW * ld, dsc=1, dsp=ld)
    _bits(d).fill_(poison.SENTINEL)
    gout = torch.tensor(GOUT, device=dev)
    ops._k("vmtl_ce_region_bwd", logits=z, target=t, weight=w, ignore_index=ign, stats=stats, coef=coef, grad_out=gout,
           ce_weight=cw, region_weight=rw, dlogits=d, **dims, **ds)
    out["grad"] = d
    return out


def _no_void(c):
    """the case's labels with every void pixel given a class: what the launches without an ignore index take"""
    t = c["t"].clone()
    void = ~c["valid"]
    t[void] = (torch.arange(int(void.sum())) * 5 + 1) % c["C"]
    return t


def _check(c, out, r, rows, C, cw, what):
    """out: _abi's result, rows: its gradient as (B,H,W,C); r: the oracle's.  Returns the measured errors."""
    loss, terms = float(out["loss"]), out["terms"].cpu().tolist()
    e_loss, e_ce, e_rg = abs(loss - float(r["loss"])), abs(terms[0] - float(r["ce"])), abs(terms[1] - float(r["region"]))
    ref = r["grad"].permute(0, 2, 3, 1)
    e_grad = float((rows.double() - ref).abs().max()) / float(ref.abs().max())
    coef = out["coef"].cpu()
    e_coef = float((coef.double() - r["coef"]).abs().max()) / float(r["coef"].abs().max())
    print(f"{what}: loss {loss:.8g} (fp64 {float(r['loss']):.8g}), errors: loss {e_loss:.2e}, CE {e_ce:.2e}, L_region "
          f"{e_rg:.2e}, gradient {e_grad:.2e} and coef {e_coef:.2e} of their magnitudes; min D_c "
          f"{float(r['D'][r['N'] > 0].min()):.3g}")
    assert e_loss < 1e-5 and e_ce < 1e-5 and e_rg < 1e-5, (loss, terms, float(r["loss"]), float(r["ce"]), float(r["region"]))
    assert out["counts"].cpu().tolist() == r["N"].tolist() + [r["V"]]
    absent = (r["N"] == 0).repeat(2)
    assert bool((_bits(coef[absent]) == 0).all())  # exactly +0.0f
    assert_close(coef, r["coef"], tol=1e-5, what=what + " coef")
    stats = out["stats"].cpu().tolist()
    if cw != 0:
        assert abs(stats[0] - r["den"]) <= 1e-6 * r["den"] and abs(stats[1] - r["num"]) <= 1e-5 * max(1.0, abs(r["num"]))
    else:
        assert stats == [0.0, 0.0] and terms[0] == 0.0
    assert not torch.isnan(rows).any()
    assert_close(rows, ref, tol=1e-5, what=what + " gradient")
    assert bool((_bits(rows[~r["valid"]]) == 0).all())  # void rows: +0.0f bit for bit
    return e_loss, e_ce, e_rg, e_grad, e_coef


@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("name", R.SMALL + R.VARIANTS + ("f",))
def test_matches_the_fp64_oracle(dev, name, setting):
    c = R.case(name)
    C = c["C"]
    z, wd = c["z"].to(dev), c["w"].to(dev)
    al, be, sm = setting
    worst = [0.0] * 5
    with _guarded():
        for ign, t in ((c["ign"], c["t"]), (None, _no_void(c))):
            td = t.to(dev)
            for weighted in (False, True):
                for cw, rw in ((1.0, 1.0), (0.0, 1.0), (0.5, 2.0)):
                    if name == "f" and (weighted != (ign is not None) or rw == 2.0):
                        continue  # the large case: the two corners of the sweep, with and without the cross entropy
                    w = c["w"] if weighted else None
                    r = R.reference(c["z"], t, al, be, sm, w, ign, cw, rw)
                    out = _abi(dev, z, td, wd if weighted else None, ign, setting, cw, rw)
                    rows = out["grad"].cpu()[..., :C]
                    errs = _check(c, out, r, rows, C, cw, f"{name} {setting} ign={ign} weighted={weighted} cw={cw} rw={rw}")
                    worst = [max(a, b) for a, b in zip(worst, errs)]
    print(f"{name} {setting}: worst errors loss {worst[0]:.2e}, CE {worst[1]:.2e}, L_region {worst[2]:.2e}, gradient "
          f"{worst[3]:.2e}, coef {worst[4]:.2e}")


class _Probe(torch.autograd.Function):
    """Identity whose backward records the gradient it is handed, as a head's data-gradient node receives it."""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        _Probe.seen = (dy.stride(), tuple(dy.shape), getattr(dy, "_vmtl_nhwc", None))
        return dy


@pytest.mark.parametrize("name", R.SMALL + R.VARIANTS)
def test_node_matches_the_c_abi_hands_off_nhwc_and_predicts(dev, name):
    ops = _ops()
    from vision_mtl_amd._lib import lib

    c = R.case(name)
    C, (B, H, W) = c["C"], c["shape"]
    z, t, w = c["z"].to(dev), c["t"].to(dev), c["w"].to(dev)
    ld = _ceil4(C + 1)
    setting, cw, rw = (0.3, 0.7, 1.0), 0.5, 2.0
    kw = dict(region_weight=rw, alpha=setting[0], beta=setting[1], smooth=setting[2], weight=w, ignore_index=c["ign"],
              ce_weight=cw)
    with _guarded() as p:
        ref = _abi(dev, z, t, w, c["ign"], setting, cw, rw, want_argmax=True)
        z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
        l1 = ops.segm_region_loss(_Probe.apply(z1), t, **kw)
        l2, pred = ops.segm_region_loss_with_argmax(z2, t, **kw)
        _Probe.seen = None
        (l1 * GOUT).backward()
        (l2 * GOUT).backward()
        assert p.count >= 10  # loss, terms, stats, coef and the gradient storage of both nodes came from ops._empty
        # the prediction of vmtl_ce_fwd_argmax on the same logits
        loss = torch.empty((), device=dev)
        ws = torch.empty(lib().raw("vmtl_ce_workspace_bytes")(B * H * W) // 8, dtype=torch.float64, device=dev)
        plain = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        ops._k("vmtl_ce_fwd_argmax", logits=z, target=t.clamp(0, C - 1), loss=loss, workspace=ws, argmax=plain, B=B,
               HW=H * W, C=C, sb=C * H * W, sc=H * W, sp=1)
    stride, shape, st = _Probe.seen
    assert shape == (B, C, H, W) and stride == (H * W * ld, 1, W * ld, ld)
    assert st is not None and tuple(st.shape) == (B, H, W, ld)
    assert torch.equal(_bits(l1.detach()), _bits(ref["loss"])) and torch.equal(_bits(l1.detach()), _bits(l2.detach()))
    assert torch.equal(_bits(z1.grad), _bits(z2.grad))
    assert torch.equal(_bits(z1.grad), _bits(ref["grad"][..., :C].permute(0, 3, 1, 2)))
    assert not poison.is_sentinel(z1.grad).any() and not poison.is_sentinel(l1.detach().reshape(1)).any()
    assert torch.equal(pred, plain) and torch.equal(pred, ref["pred"])  # every pixel, ignored ones included
    assert torch.equal(pred.cpu(), c["z"].argmax(dim=1))


@pytest.mark.parametrize("name", R.SMALL)
def test_c_abi_layouts_write_the_lanes_the_ex_kernels_write(dev, name):
    """vmtl_ce_region_bwd in the three layouts - NHWC rows of exactly ceil4(C) floats, NHWC with a wider ld (the node's
    ceil4(C+1) among them), NCHW - on sentinel-filled buffers: the oracle's values in each, and the elements still
    holding the sentinel are those a vmtl_ce_bwd_ex launch into an identically prepared buffer leaves."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    c = R.case(name)
    C, (B, H, W) = c["C"], c["shape"]
    HW, P = H * W, B * H * W
    z, t, w = c["z"].to(dev), c["t"].to(dev), c["w"].to(dev)
    setting, cw, rw = (0.3, 0.7, 1.0), 1.0, 0.5
    r = R.reference(c["z"], c["t"], *setting, c["w"], c["ign"], cw, rw)
    with _guarded():
        loss, stats = torch.empty((), device=dev), torch.empty(2, device=dev)
        ws = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
        dims = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
        ops._k("vmtl_ce_fwd_ex", logits=z, target=t, weight=w, ignore_index=c["ign"], loss=loss, stats=stats,
               workspace=ws, argmax=None, **dims)
        gout = torch.tensor(GOUT, device=dev)
        first = None
        for ld in (_ceil4(C), _ceil4(C + 1), _ceil4(C) + 4, _ceil4(C) + 8, None):
            out = _abi(dev, z, t, w, c["ign"], setting, cw, rw, ld=ld, nchw=ld is None)
            d = torch.empty_like(out["grad"])
            _bits(d).fill_(poison.SENTINEL)
            ds = dict(dsb=C * HW, dsc=HW, dsp=1) if ld is None else dict(dsb=HW * ld, dsc=1, dsp=ld)
            ops._k("vmtl_ce_bwd_ex", logits=z, target=t, weight=w, ignore_index=c["ign"], stats=stats, grad_out=gout,
                   dlogits=d, **dims, **ds)
            assert torch.equal(poison.is_sentinel(out["grad"]), poison.is_sentinel(d)), f"ld={ld}: other lanes written"
            g = out["grad"].cpu()
            if ld is None:
                g = g.permute(0, 2, 3, 1)
            else:
                pad = g[..., C:_ceil4(C)]
                assert pad.numel() == 0 or bool((_bits(pad) == 0).all())  # the pad lanes of a row are zeros
            rows = g[..., :C]
            _check(c, out, r, rows, C, cw, f"{name} ld={ld}")
            if first is None:
                first = rows
            assert torch.equal(_bits(rows), _bits(first)), f"ld={ld}: the layouts compute different bits"


@pytest.mark.parametrize("C", [3, 19])
def test_all_void_and_out_of_range_labels(dev, C):
    ops = _ops()
    IGN = R.IGN
    g = torch.Generator().manual_seed(C)
    z = (torch.randn(2, C, 5, 13, generator=g) * 3).to(dev)
    t = torch.randint(0, C, (2, 5, 13), generator=g).to(dev)
    t[1, 2, 3] = IGN
    w = (0.1 + 1.9 * torch.rand(C, generator=g)).to(dev)
    void = torch.full_like(t, IGN)
    setting = (0.3, 0.7, 1.0)
    with _guarded():
        # every pixel void, the term alone: exactly 0.0f, every written lane +0.0f
        for ld in (_ceil4(C), None):
            out = _abi(dev, z, void, None, IGN, setting, cw=0.0, rw=2.0, ld=ld, nchw=ld is None)
            assert int(_bits(out["loss"].reshape(1))) == 0 and int(_bits(out["terms"][1:2])) == 0
            assert out["counts"].tolist() == [0] * (C + 1) and bool((_bits(out["coef"]) == 0).all())
            assert bool((_bits(out["grad"]) == 0).all())  # both layouts write every element of these buffers
        zd = z.clone().requires_grad_(True)
        loss = ops.segm_region_loss(zd, void, alpha=0.3, beta=0.7, smooth=1.0, ignore_index=IGN, ce_weight=0.0)
        (loss * GOUT).backward()
        assert int(_bits(loss.detach().reshape(1))) == 0 and bool((_bits(zd.grad) == 0).all())
        # ... with the cross entropy: 0 / 0, as vmtl_ce_fwd_ex; the rows stay +0.0f (a select, not 0 * inf)
        out = _abi(dev, z, void, w, IGN, setting, cw=1.0, rw=2.0)
        assert torch.isnan(out["loss"]) and torch.isnan(out["terms"][0]) and float(out["terms"][1]) == 0.0
        assert bool((_bits(out["grad"][..., :_ceil4(C)]) == 0).all())
        zd = z.clone().requires_grad_(True)
        loss = ops.segm_region_loss(zd, void, weight=w, ignore_index=IGN)
        (loss * GOUT).backward()
        assert torch.isnan(loss) and bool((_bits(zd.grad) == 0).all())
        # one valid label outside [0, C): the loss and the whole table are NaN, with and without the cross entropy
        for bad in (C, -1):
            for wt in (None, w):
                for cw in (1.0, 0.0):
                    tb = t.clone()
                    tb[0, 1, 2] = bad
                    out = _abi(dev, z, tb, wt, IGN, setting, cw=cw)
                    assert torch.isnan(out["loss"]) and torch.isnan(out["terms"][1]) and torch.isnan(out["coef"]).all()
                    assert out["counts"][C].item() == 2 * 5 * 13 - 1
                    rows = out["grad"][..., :C]
                    assert torch.isnan(rows[0, 1, 2]).all() and bool((_bits(rows[1, 2, 3]) == 0).all())


def test_more_than_32_classes_are_refused_without_a_launch(dev):
    ops = _ops()
    C = 33
    z = torch.randn(2, C, 5, 13, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.zeros(2, 5, 13, dtype=torch.int64, device=dev)
    loss, terms, stats, coef = (torch.empty(s, device=dev) for s in ((), (2,), (2,), (2 * C,)))
    counts = torch.empty(C + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(1024, dtype=torch.float64, device=dev)
    d = torch.empty(2, 5, 13, 36, device=dev)
    outs = (loss, terms, stats, coef, d)
    for o in outs:
        _bits(o).fill_(poison.SENTINEL)
    counts.fill_(-7)
    dims = dict(B=2, HW=65, C=C, sb=C * 65, sc=65, sp=1)
    gout = torch.tensor(GOUT, device=dev)
    with _guarded():
        with pytest.raises(RuntimeError, match="unsupported"):
            ops._k("vmtl_ce_region_fwd", logits=z, target=t, weight=None, ignore_index=ops.NO_IGNORE, alpha=0.5, beta=0.5,
                   smooth=0.0, ce_weight=1.0, region_weight=1.0, loss=loss, terms=terms, stats=stats, coef=coef,
                   counts=counts, workspace=ws, argmax=None, **dims)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops._k("vmtl_ce_region_bwd", logits=z, target=t, weight=None, ignore_index=ops.NO_IGNORE, stats=stats,
                   coef=coef, grad_out=gout, ce_weight=1.0, region_weight=1.0, dlogits=d, **dims, dsb=65 * 36, dsc=1,
                   dsp=36)
        with pytest.raises(ValueError, match="2 to 32 classes"):
            ops.segm_region_loss(z.clone().requires_grad_(True), t)
    torch.cuda.synchronize()
    assert all(bool(poison.is_sentinel(o).all()) for o in outs) and bool((counts == -7).all())


def test_two_runs_are_bit_identical(dev):
    c = R.case("f")
    z, t, w = c["z"].to(dev), c["t"].to(dev), c["w"].to(dev)
    with _guarded():
        runs = [_abi(dev, z, t, w, c["ign"], (0.3, 0.7, 1.0), 1.0, 0.5) for _ in range(2)]
    a, b = runs
    for key in ("loss", "terms", "stats", "coef", "grad"):
        assert torch.equal(_bits(a[key]), _bits(b[key])), key
    assert torch.equal(a["counts"], b["counts"])
