"""-m gpu: online hard example mining in the cross entropy (csrc/ce_ohem.hip) through the C ABI (vmtl_ce_ohem_fwd /
vmtl_ce_ohem_bwd) and through the node (ops.cross_entropy_ohem[_with_argmax]), every launch under poison.patched("guard")
and launch_guard.patched().

What is exact and what is rounded are checked apart.  SELECTION is checked on the device's own nll buffer against
ohem_oracle.select (torch.sort): the cut bit for bit, the counts exactly, the non-zero gradient rows exactly the kept
set.  ARITHMETIC is checked against fp64 with the device's kept mask: per-pixel nll within 2^-19 * max(1, max_c |z_c|)
(16 fp32 ulps at the logits' magnitude: one exactly rounded subtraction, an exp / log pair on a sum in [1, C] and one
addition), loss within 1e-5 absolute and gradient within 1e-5 of its magnitude (the bounds of tests/test_loss_ignore_gpu.py
for the same arithmetic).  Against the pure fp64 oracle, membership included, only where the fp64 nll keeps a margin
above twice the nll bound around both decisions (asserted first)."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import launch_guard, ohem_oracle as O, poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GOUT = O.GOUT
IGN = O.IGN
NLL_TOL = 2.0 ** -19


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


@functools.lru_cache(maxsize=None)
def _unit_grad(name):
    """softmax - onehot in fp64, (B,H,W,C); the rows of void pixels are not used"""
    c = O.case(name)
    sm = F.softmax(c["z"].double(), dim=1).permute(0, 2, 3, 1).contiguous()
    tt = c["t"].clamp(0, c["C"] - 1)
    sm.scatter_add_(3, tt.unsqueeze(3), -torch.ones_like(sm[..., :1]))
    return sm


def _abi(dev, z, t, w, ign, total, tau, ld=None, nchw=False, want_argmax=False):
    """vmtl_ce_ohem_fwd + vmtl_ce_ohem_bwd on device tensors; the gradient in NHWC rows of `ld` floats (default: the
    node's ceil4(C+1)) or NCHW.  Everything comes back as it was written, on the device."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    B, C, H, W = z.shape
    HW, P = H * W, B * H * W
    loss, stats = torch.empty((), device=dev), torch.empty(4, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    nll = torch.empty(B, H, W, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_argmax else None
    ws = torch.empty(lib().raw("vmtl_ce_ohem_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    ign = ops.NO_IGNORE if ign is None else ign
    dims = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    ops._k("vmtl_ce_ohem_fwd", logits=z, target=t, weight=w, ignore_index=ign, nll_thresh=tau, min_kept_total=total,
           loss=loss, stats=stats, counts=counts, nll=nll, workspace=ws, argmax=pred, **dims)
    if nchw:
        d = torch.empty(B, C, H, W, device=dev)
        ds = dict(dsb=C * HW, dsc=HW, dsp=1)
    else:
        ld = _ceil4(C + 1) if ld is None else ld
        d = torch.empty(B, H, W, ld, device=dev)
        ds = dict(dsb=HW * ld, dsc=1, dsp=ld)
    _bits(d).fill_(poison.SENTINEL)
    gout = torch.tensor(GOUT, device=dev)
    ops._k("vmtl_ce_ohem_bwd", logits=z, target=t, weight=w, ignore_index=ign, stats=stats, nll=nll, grad_out=gout,
           dlogits=d, **dims, **ds)
    return dict(loss=loss, stats=stats, counts=counts, nll=nll, grad=d, pred=pred)


def _dev_case(c, dev):
    return c["z"].to(dev), c["t"].to(dev), c["w"].to(dev)


def _check_selection_and_arithmetic(c, unit, out, total, tau32, w, sorted_desc=None):
    """out: _abi's result for the case c in an NHWC layout.  Returns the device's kept mask (CPU)."""
    C, valid, V = c["C"], c["valid"], c["V"]
    nll = out["nll"].cpu()
    stats, counts = out["stats"].cpu(), out["counts"].cpu()
    # ---- selection, on the device's own nll
    cut, kept = O.select(nll, valid, total, tau32, sorted_desc)
    assert int(_bits(stats[2:3])) == int(_bits(cut.reshape(1))), (float(stats[2]), float(cut))
    assert counts.tolist() == [V, int(kept.sum())]
    assert int(kept.sum()) >= min(total, V)
    rows = out["grad"].cpu()[..., :C]
    nonzero = (_bits(rows) != 0).any(dim=3)
    ref_nonzero = valid & (unit != 0).any(dim=3)  # where the fp64 gradient row of a kept pixel would not vanish
    assert torch.equal(nonzero[ref_nonzero], kept[ref_nonzero])
    assert bool((_bits(rows[~kept]) == 0).all())  # +0.0f bit for bit
    # ---- arithmetic, with the device's kept mask
    wt = torch.ones_like(c["nll"]) if w is None else w.double()[c["t"].clamp(0, C - 1)]
    num, den = float((wt * c["nll"])[kept].sum()), float(wt[kept].sum())
    assert abs(float(out["loss"]) - num / den) < 1e-5, (float(out["loss"]), num / den)
    assert abs(float(stats[0]) - den) <= 1e-6 * den and abs(float(stats[1]) - num) <= 1e-5 * max(1.0, abs(num))
    assert float(stats[3]) == 0.0
    ref = unit * (wt * kept * (GOUT / den)).unsqueeze(3)
    assert not torch.isnan(rows).any()
    assert_close(rows, ref, tol=1e-5, what="OHEM gradient")
    return kept


def _check_nll(c, nll):
    valid = c["valid"]
    assert bool((nll[~valid] == -1.0).all())
    err = (nll.double() - c["nll"])[valid].abs()
    bound = NLL_TOL * c["zmax"].clamp_min(1.0)[valid]
    assert bool((err <= bound).all()), f"nll error {float((err / bound).max()):.3f} of its bound"
    assert bool((_bits(nll[valid]) >= 0).all())  # +0.0f or above: never -0.0f, never negative


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("thresh", O.THRESHOLDS)
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_selection_is_exact_and_arithmetic_matches_fp64(dev, name, thresh, weighted):
    c, unit = O.case(name), _unit_grad(name)
    z, t, wd = _dev_case(c, dev)
    tau32 = float(torch.tensor(O.tau_of(thresh), dtype=torch.float32))
    sorted_desc = None
    with _guarded():
        for total in O.kept_totals(c["V"]):
            out = _abi(dev, z, t, wd if weighted else None, IGN, total, tau32)
            nll = out["nll"].cpu()
            if sorted_desc is None:  # the nll buffer does not depend on K, tau or the weights
                _check_nll(c, nll)
                sorted_desc, first = O.sort_desc(nll, c["valid"]), nll
            assert torch.equal(_bits(nll), _bits(first))
            kept = _check_selection_and_arithmetic(c, unit, out, total, tau32, c["w"] if weighted else None, sorted_desc)
            if thresh == 1.0 or total >= c["V"]:
                assert torch.equal(kept, c["valid"])
            print(f"{name}: V {c['V']}, K {min(total, c['V'])}, thresh {thresh}: cut {float(out['stats'][2]):.8g}, kept "
                  f"{int(out['counts'][1])}, loss {float(out['loss']):.8g}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", O.SMALL)
def test_against_the_pure_fp64_oracle_membership_included(dev, name, weighted):
    c = O.case(name)
    z, t, wd = _dev_case(c, dev)
    w = c["w"] if weighted else None
    need = 2 * NLL_TOL * float(c["zmax"].max())
    with _guarded():
        for total in O.kept_totals(c["V"]):
            for thresh in O.THRESHOLDS:
                tau = O.tau_of(thresh)
                m = O.margin(c["nll"], c["valid"], total, tau)
                assert m > need, f"{name}: K {total}, thresh {thresh}: margin {m:.3e} <= {need:.3e}"
                r = O.reference(c["z"], c["t"], total, thresh, w, IGN)
                out = _abi(dev, z, t, wd if weighted else None, IGN, total, float(torch.tensor(tau, dtype=torch.float32)))
                nll, cut = out["nll"].cpu(), out["stats"][2].cpu()
                kept = c["valid"] & ~(nll < cut)
                assert torch.equal(kept, r["kept"])
                assert out["counts"].tolist() == [c["V"], int(r["kept"].sum())]
                if math.isfinite(float(r["cut"])):
                    assert abs(float(cut) - float(r["cut"])) <= NLL_TOL * max(1.0, float(c["zmax"].max()))
                else:
                    assert float(cut) == float(r["cut"])
                assert abs(float(out["loss"]) - float(r["loss"])) < 1e-5
                assert_close(out["grad"].cpu()[..., :c["C"]].permute(0, 3, 1, 2), r["grad"], tol=1e-5,
                             what="OHEM gradient vs fp64 oracle")


@pytest.mark.parametrize("K", [1, 64, 129])
def test_the_last_radix_round_decides(dev, K):
    """C = 2, target 0, logits (0, i * 2^-20): nll = log(1 + exp(i 2^-20)) = log 2 + i 2^-21 + O(i^2 2^-43), steps of 8
    fp32 ulps at 0.69 against a few ulps of expf / logf error - 130 distinct keys that differ only in their low 11 bits,
    so the first two histograms each put every pixel in one bin and only the last digits separate them."""
    n = 130
    z = torch.zeros(1, 2, 1, n)
    z[0, 1, 0] = torch.arange(n, dtype=torch.float32) * 2.0 ** -20
    t = torch.zeros(1, 1, n, dtype=torch.int64)
    host = _bits(F.cross_entropy(z, t, reduction="none"))
    assert host.unique().numel() == n and (host >> 11).unique().numel() == 1
    with _guarded():
        out = _abi(dev, z.to(dev), t.to(dev), None, None, K, math.inf)
    nll = out["nll"].cpu()
    keys = _bits(nll)
    assert keys.unique().numel() == n and (keys >> 11).unique().numel() == 1
    valid = torch.ones_like(t, dtype=torch.bool)
    cut, kept = O.select(nll, valid, K, math.inf)
    assert int(_bits(out["stats"][2:3].cpu())) == int(_bits(cut.reshape(1)))
    assert out["counts"].tolist() == [n, K] and int(kept.sum()) == K
    nonzero = (_bits(out["grad"].cpu()[..., :2]) != 0).any(dim=3)
    assert torch.equal(nonzero, kept)


@pytest.mark.parametrize("name", ["a", "c"])
def test_ties_at_the_cut_are_all_kept(dev, name):
    """The logits row and the label of the rank-K pixel copied into four pixels outside the kept set: five pixels tie
    at the cut bit for bit, and all of them stay - kept = K + 4."""
    c = O.case(name)
    C, V = c["C"], c["V"]
    K = V // 2
    need = 2 * NLL_TOL * float(c["zmax"].max())  # ranks K-1, K, K+1 keep their order in fp32
    assert min(O.margin(c["nll"], c["valid"], K, math.inf), O.margin(c["nll"], c["valid"], K - 1, math.inf)) > need
    flat = torch.where(c["valid"], c["nll"], torch.full_like(c["nll"], -1.0)).flatten()
    order = torch.argsort(flat, descending=True)
    src, dst = int(order[K - 1]), order[V - 4:V]  # the four easiest valid pixels
    z = c["z"].permute(0, 2, 3, 1).reshape(-1, C).clone()
    t = c["t"].flatten().clone()
    z[dst], t[dst] = z[src].clone(), t[src].clone()
    B, H, W = c["shape"]
    z = z.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    t = t.reshape(B, H, W)
    with _guarded():
        out = _abi(dev, z.to(dev), t.to(dev), c["w"].to(dev), IGN, K, math.inf)
    nll = out["nll"].cpu()
    assert _bits(nll.flatten()[dst]).tolist() == [int(_bits(nll.flatten()[src:src + 1]))] * 4
    cut, kept = O.select(nll, c["valid"], K, math.inf)
    assert int(kept.sum()) == K + 4
    assert out["counts"].tolist() == [V, K + 4]
    assert int(_bits(out["stats"][2:3].cpu())) == int(_bits(cut.reshape(1)))
    nonzero = (_bits(out["grad"].cpu()[..., :C]) != 0).any(dim=3)
    assert torch.equal(nonzero, kept)


@pytest.mark.parametrize("C", [19, 33])
def test_all_ignored_and_out_of_range_labels(dev, C):
    ops = _ops()
    g = torch.Generator().manual_seed(C)
    z = (torch.randn(2, C, 5, 13, generator=g) * 3).to(dev)
    t = torch.randint(0, C, (2, 5, 13), generator=g).to(dev)
    t[1, 2, 3] = IGN
    w = (0.1 + 1.9 * torch.rand(C, generator=g)).to(dev)
    with _guarded():
        # every pixel ignored: 0 / 0, nothing kept, every lane +0.0f (a select, not 0 * inf)
        out = _abi(dev, z, torch.full_like(t, IGN), w, IGN, 7, 0.5)
        assert torch.isnan(out["loss"]) and out["counts"].tolist() == [0, 0]
        assert bool((_bits(out["grad"][..., :_ceil4(C)]) == 0).all())
        zd = z.clone().requires_grad_(True)
        loss = ops.cross_entropy_ohem(zd, torch.full_like(t, IGN), 3, thresh=0.7, weight=w, ignore_index=IGN)
        loss.backward()
        assert torch.isnan(loss) and bool((_bits(zd.grad) == 0).all())
        # one label outside [0, C) that is not the ignore index: NaN ranks hardest, the pixel is kept, the loss is NaN
        for bad in (C, -1):
            for wt in (None, w):
                for tau in (math.inf, 0.5):
                    tb = t.clone()
                    tb[0, 1, 2] = bad
                    out = _abi(dev, z, tb, wt, IGN, 2, tau)
                    nll = out["nll"].cpu()
                    assert math.isnan(float(nll[0, 1, 2]))
                    cut, kept = O.select(nll, tb.cpu() != IGN, 2, tau)
                    assert bool(kept[0, 1, 2]) and out["counts"].tolist() == [2 * 5 * 13 - 1, int(kept.sum())]
                    assert int(_bits(out["stats"][2:3].cpu())) == int(_bits(cut.reshape(1)))
                    assert torch.isnan(out["loss"])
                    rows = out["grad"].cpu()[..., :C]
                    assert torch.isnan(rows[0, 1, 2]).all()
                    assert bool((_bits(rows[~kept]) == 0).all()) and bool((_bits(rows[1, 2, 3]) == 0).all())
        # K NaN pixels or more: kappa is NaN and the cut is tau
        tb = t.clone()
        tb[0, 0, :3] = C
        out = _abi(dev, z, tb, None, IGN, 2, math.inf)
        assert float(out["stats"][2]) == math.inf and out["counts"].tolist() == [2 * 5 * 13 - 1, 3]


@pytest.mark.parametrize("name", ["a", "c", "d", "e"])
def test_identities_keep_every_valid_pixel(dev, name):
    """thresh = 1.0, or min_kept * B >= V: the weighted / ignoring cross entropy of ops.cross_entropy."""
    ops = _ops()
    c = O.case(name)
    B = c["shape"][0]
    z, t, w = _dev_case(c, dev)
    with _guarded():
        for wt in (None, w):
            zr = z.clone().requires_grad_(True)
            ref = ops.cross_entropy(zr, t, weight=wt, ignore_index=IGN)
            (ref * GOUT).backward()
            for min_kept, thresh in ((1, 1.0), (-(-c["V"] // B), None), (c["V"], 0.7)):
                zd = z.clone().requires_grad_(True)
                loss = ops.cross_entropy_ohem(zd, t, min_kept, thresh=thresh, weight=wt, ignore_index=IGN)
                (loss * GOUT).backward()
                assert abs(float(loss.detach()) - float(ref.detach())) < 1e-5
                assert_close(zd.grad, zr.grad, tol=1e-5, what="identity gradient")
                assert bool((_bits(zd.grad.permute(0, 2, 3, 1)[t == IGN]) == 0).all())
        # no ignore index at all: every pixel is valid (labels as they are: 255 would be out of range, so drawn anew)
        tt = torch.randint(0, c["C"], c["shape"], generator=torch.Generator().manual_seed(3)).to(dev)
        out = _abi(dev, z, tt, None, None, 10 ** 9, 0.25)
        assert out["counts"].tolist() == [tt.numel(), tt.numel()]
        assert abs(float(out["loss"]) - float(ops.cross_entropy(z, tt))) < 1e-5


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


@pytest.mark.parametrize("name", ["a", "c", "d", "e"])
def test_node_matches_the_c_abi_and_hands_off_nhwc(dev, name):
    ops = _ops()
    c = O.case(name)
    C, (B, H, W), V = c["C"], c["shape"], c["V"]
    z, t, w = _dev_case(c, dev)
    ld = _ceil4(C + 1)
    min_kept, thresh = max(1, V // (2 * B)), 0.7
    tau32 = float(torch.tensor(O.tau_of(thresh), dtype=torch.float32))
    with _guarded() as p:
        ref = _abi(dev, z, t, w, IGN, min_kept * B, tau32, want_argmax=True)
        z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
        l1 = ops.cross_entropy_ohem(_Probe.apply(z1), t, min_kept, thresh=thresh, weight=w, ignore_index=IGN)
        l2, pred = ops.cross_entropy_ohem_with_argmax(z2, t, min_kept, thresh=thresh, weight=w, ignore_index=IGN)
        _Probe.seen = None
        (l1 * GOUT).backward()
        (l2 * GOUT).backward()
        assert p.count >= 8  # loss, stats, nll and the gradient storage of both nodes came from ops._empty
    stride, shape, st = _Probe.seen
    assert shape == (B, C, H, W) and stride == (H * W * ld, 1, W * ld, ld)
    assert st is not None and tuple(st.shape) == (B, H, W, ld)
    assert torch.equal(_bits(l1.detach()), _bits(ref["loss"])) and torch.equal(_bits(l1.detach()), _bits(l2.detach()))
    assert torch.equal(_bits(z1.grad), _bits(z2.grad))
    assert torch.equal(_bits(z1.grad), _bits(ref["grad"][..., :C].permute(0, 3, 1, 2)))
    assert not poison.is_sentinel(z1.grad).any() and not poison.is_sentinel(l1.detach().reshape(1)).any()
    # the prediction: every pixel, ignored ones included
    assert torch.equal(pred, ops.argmax_channels(z)) and torch.equal(pred, ref["pred"])
    assert torch.equal(pred.cpu(), c["z"].argmax(dim=1))


@pytest.mark.parametrize("name", O.SMALL)
def test_c_abi_layouts_write_the_lanes_the_ex_kernels_write(dev, name):
    """vmtl_ce_ohem_bwd in the three layouts - NHWC rows of exactly ceil4(C) floats, NHWC with a wider ld, NCHW - on
    sentinel-filled buffers: the same values in each, and the written elements are those vmtl_ce_bwd_ex writes."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    c, unit = O.case(name), _unit_grad(name)
    C, (B, H, W), V = c["C"], c["shape"], c["V"]
    HW, P = H * W, B * H * W
    z, t, w = _dev_case(c, dev)
    tau32 = float(torch.tensor(O.tau_of(0.7), dtype=torch.float32))
    total = V // 3
    with _guarded():
        loss, stats = torch.empty((), device=dev), torch.empty(2, device=dev)
        ws = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
        dims = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
        ops._k("vmtl_ce_fwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, loss=loss, stats=stats, workspace=ws,
               argmax=None, **dims)
        gout = torch.tensor(GOUT, device=dev)
        for ld in (_ceil4(C), _ceil4(C) + 4, _ceil4(C) + 8, None):
            out = _abi(dev, z, t, w, IGN, total, tau32, ld=ld, nchw=ld is None)
            d = torch.empty_like(out["grad"])
            _bits(d).fill_(poison.SENTINEL)
            ds = dict(dsb=C * HW, dsc=HW, dsp=1) if ld is None else dict(dsb=HW * ld, dsc=1, dsp=ld)
            ops._k("vmtl_ce_bwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, stats=stats, grad_out=gout,
                   dlogits=d, **dims, **ds)
            assert torch.equal(poison.is_sentinel(out["grad"]), poison.is_sentinel(d)), f"ld={ld}: other lanes written"
            if ld is None:
                out["grad"] = out["grad"].permute(0, 2, 3, 1)
            else:
                pad = out["grad"][..., C:_ceil4(C)]
                assert pad.numel() == 0 or bool((_bits(pad) == 0).all())  # the pad lanes of a row are zeros
            _check_selection_and_arithmetic(c, unit, out, total, tau32, c["w"])


@pytest.mark.parametrize("name", ["c", "f"])
def test_two_runs_are_bit_identical(dev, name):
    c = O.case(name)
    z, t, w = _dev_case(c, dev)
    tau32 = float(torch.tensor(O.tau_of(0.7), dtype=torch.float32))
    with _guarded():
        runs = [_abi(dev, z, t, w, IGN, c["V"] // 2, math.inf if k >= 2 else tau32) for k in (0, 1, 2, 3)]
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        for key in ("loss", "stats", "nll", "grad"):
            assert torch.equal(_bits(a[key]), _bits(b[key])), key
        assert torch.equal(a["counts"], b["counts"])
