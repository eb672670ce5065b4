"""-m gpu: every production conv node at its production shape against a float64 CPU restatement, plus the route list.

tests/production.py takes a census of one eager training step of each BASELINE configuration.  Every unique signature of the
conv nodes (ops.conv2d, ops.bn_act_conv, ops.up2_conv) is then replayed on its own, at exactly that shape and with the same
flags, on seeded random inputs, and compared with F.conv2d / F.batch_norm in float64 on the CPU:
  - the forward output (1e-4 of the reference's maximum);
  - the statistics partial rows the node emits, merged over rows with the node's own rows-per-block into a per-channel mean
    AND variance (1e-5), separately for an ordinary channel set and, where the node has a bias, a large-mean / small-std
    set (bias ~100, output std ~0.05: the partial-row merge is where cancellation bites);
  - the BatchNorm running buffers (1e-5) and num_batches_tracked;
  - every input and parameter gradient for a seeded dy (2e-4).
A node that consumes statistics partials is replayed on that path: the rows are built from the synthetic input in the
kernels' (mean_b, M2_b) layout, rows_per_blk pixels per row.  If a tensor misses its bar, the float32 CPU restatement's own
error is measured and the bar becomes max(bar, 4 x that error); every such case is printed.
BatchNorm inputs are nudged so that no normalised value lies within 1e-3 of an activation kink (ReLU 0, hard-swish /
hard-sigmoid +-3): a mask flip between two fp32 implementations would otherwise move a gradient by O(|g|).

The replays' launches are recorded too: every production launch of a replayed node (entry point + integer / float
arguments: shapes, ep_mode, splits, nblk / rows_per_blk, ...) must be among its replay's launches, which proves the replays
ran the kernels, split counts and merge geometries the benchmark runs.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.production import CONFIGS, fmt_launch, fmt_sig, production_census, recording, sig_args
from tests.util import ceil4

pytestmark = pytest.mark.gpu

BAR_OUT, BAR_STATS, BAR_GRAD = 1e-4, 1e-5, 2e-4
KINKS = {0: (), 1: (0.0,), 2: (-3.0, 3.0), 3: (-3.0, 3.0), 4: ()}
ACTS = {0: lambda z: z, 1: F.relu, 2: F.hardswish, 3: F.hardsigmoid, 4: torch.sigmoid}


@pytest.fixture(scope="module")
def censuses(dev):
    out = {}
    for name in CONFIGS:
        c = production_census(name)
        print(c.report())
        out[name] = c
    return out


def _signatures(censuses, op):
    """unique signatures of one node across the configurations -> production launches (set) of each.  conv2d also gets
    the image-gradient variant of every stride-2 signature whose input has no gradient (the ResNet stem: its data gradient
    runs when the image requires one), with no production launches of its own"""
    sigs = {}
    for c in censuses.values():
        for sig in c.nodes:
            if sig[0] == op:
                sigs.setdefault(sig, set()).update(c.node_launches(sig))
    if op == "conv2d":
        for sig in list(sigs):
            v = _dx_variant(sig)
            if v is not None:
                sigs.setdefault(v, set())
    return sigs


def _s2_dgrad(a):
    """a stride-2 conv2d whose data gradient the phase decomposition supports (vmtl_conv2d_dgrad_s2)"""
    from vision_mtl_amd._lib import lib

    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    ws, st, pd = a["weight"][1], pair(a["stride"]), pair(a["pad"])
    return (st == (2, 2) and ws[2] == ws[3] and pd[0] == pd[1] and a["stitch"] is None
            and bool(lib().raw("vmtl_conv2d_dgrad_s2_supported")(ws[2], pd[0])))


def _dx_variant(sig):
    """the signature with x requiring a gradient, for a stride-2 conv2d whose x has none; else None"""
    a = sig_args(sig)
    if a["x"][2] or not _s2_dgrad(a):
        return None
    return (sig[0], tuple((k, (v[0], v[1], True) + tuple(v[3:])) if k == "x" else (k, v) for k, v in sig[1]))


def _nhwc(x, dev):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, ceil4(C), dtype=torch.float32)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out.to(dev)


def _nchw(y, C):
    return y[..., :C].permute(0, 3, 1, 2).cpu()


def _merge(stats, rpb, M, C):
    """per-channel (mean, biased variance) of (mean_b, M2_b) rows, block b holding min(rpb, M - b*rpb) pixels (fp64)"""
    st = stats.detach().double().cpu()
    nb = (M - torch.arange(st.shape[0], dtype=torch.float64) * rpb).clamp(0, rpb)[:, None]
    assert float(nb.sum()) == M, f"statistics rows cover {float(nb.sum())} pixels, the output has {M}"
    m, m2 = st[:, 0, :C], st[:, 1, :C]
    mean = (nb * m).sum(0) / M
    return mean, (m2 + nb * (m - mean) ** 2).sum(0) / M


def _stats_rows(x, rows, rpb):
    """(rows, 2, Cs) partial rows of x (B, C, H, W fp32) in NHWC pixel order, rpb pixels per row, as the conv epilogues emit"""
    B, C, H, W = x.shape
    M = B * H * W
    assert rows * rpb >= M, (rows, rpb, M)
    flat = torch.zeros(rows * rpb, C, dtype=torch.float64)
    flat[:M] = x.double().permute(0, 2, 3, 1).reshape(-1, C)
    nb = (M - torch.arange(rows, dtype=torch.float64) * rpb).clamp(0, rpb)[:, None]
    blk = flat.view(rows, rpb, C)
    mb = blk.sum(1) / nb.clamp_min(1)
    valid = (torch.arange(rows * rpb) < M).view(rows, rpb, 1)
    m2 = (((blk - mb[:, None]) ** 2) * valid).sum(1)
    out = torch.zeros(rows, 2, ceil4(C), dtype=torch.float64)
    out[:, 0, :C], out[:, 1, :C] = mb, m2
    return out.float()


class Checker:
    """bars against fp64, with the fp32 CPU restatement's own error as the fallback bar (computed on demand)"""

    def __init__(self, label, ref32_fn):
        self.label, self.ref32_fn, self._ref32 = label, ref32_fn, None
        self.failures, self.relaxed, self.worst = [], [], {}

    def __call__(self, what, got, ref, bar, ref_key=None, sel=None):
        got, ref = got.double(), ref.double()
        if sel is not None:
            got, ref = got[sel], ref[sel]
        mag = float(ref.abs().max())
        err = float((got - ref).abs().max()) / max(mag, 1e-30)
        fam = what.split("[")[0]
        self.worst[fam] = max(self.worst.get(fam, 0.0), err)
        if err <= bar:
            return
        e32 = None
        if ref_key is not None:
            if self._ref32 is None:
                self._ref32 = self.ref32_fn()
            r32 = self._ref32[ref_key].double()
            if sel is not None:
                r32 = r32[sel]
            e32 = float((r32 - ref).abs().max()) / max(mag, 1e-30)
            if err <= 4 * e32:
                self.relaxed.append(f"{self.label} {what}: {err:.2e} (bar {bar:.0e}, fp32 CPU {e32:.2e})")
                return
        self.failures.append(f"{self.label} {what}: max-abs error {err:.2e} of the reference's maximum (bar {bar:.0e}"
                             + (f", fp32 CPU restatement {e32:.2e})" if e32 is not None else ")"))


def _check_buffers(chk, label, m, spec_training, rm0, rv0, ref_rm, ref_rv, rm_key, rv_key, stage):
    """the running buffers of one replayed BatchNorm after the call.  Training replays (stage None) and the "val" stage
    (train mode under no_grad): against the fp64 restatement at BAR_STATS, num_batches_tracked moved once in train mode.
    The "predict" stage: bitwise what was uploaded, num_batches_tracked still 0."""
    if stage is not None and spec_training != (stage == "val"):
        chk.failures.append(f"{chk.label}: BatchNorm {label} is in {'train' if spec_training else 'eval'} mode in a {stage} step")
    if stage == "predict":
        if not (torch.equal(m.running_mean.cpu(), rm0) and torch.equal(m.running_var.cpu(), rv0)):
            chk.failures.append(f"{chk.label}: the running buffers of {label} moved in a predict step")
        if int(m.num_batches_tracked) != 0:
            chk.failures.append(f"{chk.label}: num_batches_tracked of {label} moved in a predict step")
        return
    sfx = f"[{label}]" if label else ""
    chk(f"running_mean{sfx}", m.running_mean.cpu(), ref_rm, BAR_STATS, rm_key)
    chk(f"running_var{sfx}", m.running_var.cpu(), ref_rv, BAR_STATS, rv_key)
    if int(m.num_batches_tracked) != (1 if spec_training else 0):
        chk.failures.append(f"{chk.label}: num_batches_tracked of {label or 'the BatchNorm'}")


def _check_stats(chk, what, stats, rpb, y64, C, sets, ref_key):
    B, _, H, W = y64.shape
    mean, var = _merge(stats, rpb, B * H * W, C)
    m64, v64 = y64.mean((0, 2, 3)), y64.var((0, 2, 3), unbiased=False)
    for tag, idx in sets:
        if len(idx):
            chk(f"{what} mean[{tag}]", mean, m64, BAR_STATS, ref_key + ("mean",), sel=idx)
            chk(f"{what} var[{tag}]", var, v64, BAR_STATS, ref_key + ("var",), sel=idx)


# ------------------------------------------------------------------------------------------------ conv2d
def _conv2d_case(sig, g):
    a = sig_args(sig)
    xs, ws = a["x"][1], a["weight"][1]
    B, H, W, Cs = xs
    Cout, Cin = ws[0], ws[1]
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(ws, generator=g) / (Cin * ws[2] * ws[3]) ** 0.5
    big = list(range(Cout // 4)) if a["bias"] is not None and a["want_stats"] else []
    bias = None
    if a["bias"] is not None:
        bias = torch.randn(Cout, generator=g) * 0.1
        bias[big] += 100.0  # large-mean / small-std output channels (mean / std ~ 2000, as test_bn_large_mean_small_std)
        w[big] *= 0.05
    st = None
    if a["stitch"] is not None:
        st = 1.0 + 0.1 * torch.randn(a["stitch"][0][1], generator=g)
    return a, x, w, bias, st, big


def _conv2d_ref(a, x, w, bias, st, dy, dtype):
    xr = x.to(dtype).requires_grad_(a["x"][2])
    wr, br = w.to(dtype).requires_grad_(True), None if bias is None else bias.to(dtype).requires_grad_(True)
    sr, xin = None, xr
    if st is not None:
        sr = st.to(dtype).requires_grad_(True)
        task = a["stitch"][1]
        s = sr[task, task]
        xin = xr * (s.view(1, -1, 1, 1) if s.dim() else s)
    y = F.conv2d(xin, wr, br, a["stride"], a["pad"])
    if dy is not None:  # None: a forward-only replay
        y.backward(dy.to(dtype))
    yd = y.detach()
    return {("y",): yd, ("mean",): yd.mean((0, 2, 3)), ("var",): yd.var((0, 2, 3), unbiased=False),
            ("dx",): None if xr.grad is None else xr.grad, ("dw",): wr.grad, ("db",): None if br is None else br.grad,
            ("dst",): None if sr is None else sr.grad}


def _replay_conv2d(sig, dev, stage=None):
    """stage None: forward + backward of a training signature; "val" / "predict": forward only under no_grad"""
    from vision_mtl_amd import ops

    g = torch.Generator().manual_seed(zlib.crc32(repr(sig).encode()))
    a, x, w, bias, st, big = _conv2d_case(sig, g)
    Cout = w.shape[0]
    xd = _nhwc(x, dev).requires_grad_(a["x"][2])
    wd = w.to(dev).requires_grad_(True)
    bd = None if bias is None else bias.to(dev).requires_grad_(True)
    sd = None if st is None else st.to(dev).requires_grad_(True)
    with recording() as rec, torch.set_grad_enabled(stage is None):
        out = ops.conv2d(xd, wd, bd, a["stride"], a["pad"], want_stats=a["want_stats"], zero_bias_grad=a["zero_bias_grad"],
                         stitch=None if sd is None else (sd, a["stitch"][1]))
        y, stats = out if a["want_stats"] else (out, None)
        dy = None
        if stage is None:
            dy = torch.randn(y.shape[0], Cout, y.shape[1], y.shape[2], generator=g)
            y.backward(_nhwc(dy, dev))
        torch.cuda.synchronize()
    ref = _conv2d_ref(a, x, w, bias, st, dy, torch.float64)
    chk = Checker(fmt_sig(sig), lambda: _conv2d_ref(a, x, w, bias, st, dy, torch.float32))
    chk("y", _nchw(y, Cout), ref[("y",)], BAR_OUT, ("y",))
    if stats is not None:
        norm = [c for c in range(Cout) if c not in big]
        _check_stats(chk, "stats", stats, stats._vmtl_rpb, ref[("y",)], Cout, [("ordinary", norm), ("large-mean", big)], ())
    if stage is not None:
        if stage == "predict" and stats is not None:
            chk.failures.append(f"{chk.label}: a predict step's conv returned statistics rows")
        return chk, rec
    if a["x"][2]:
        chk("dx", _nchw(xd.grad, x.shape[1]), ref[("dx",)], BAR_GRAD, ("dx",))
    chk("dw", wd.grad.cpu(), ref[("dw",)], BAR_GRAD, ("dw",))
    if bd is not None:
        if a["zero_bias_grad"]:
            assert float(bd.grad.abs().max()) == 0.0, f"{fmt_sig(sig)}: zero_bias_grad bias got a non-zero gradient"
        else:
            chk("db", bd.grad.cpu(), ref[("db",)], BAR_GRAD, ("db",))
    if sd is not None:
        chk("dstitch", sd.grad.cpu(), ref[("dst",)], BAR_GRAD, ("dst",))
    return chk, rec


# ------------------------------------------------------------------------------------------------ bn_act_conv / up2_conv
def _nudge(x, gamma, beta, eps, act, training, rm, rv, band=1e-3):
    """move the few inputs whose normalised value lies within `band` of an activation kink to 2*band away from it"""
    kinks = KINKS[act]
    if not kinks:
        return x
    x = x.double()
    for _ in range(2):
        if training:
            mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        else:
            mean, var = rm.double(), rv.double()
        sc = (gamma.double() / (var + eps).sqrt()).view(1, -1, 1, 1)
        z = (x - mean.view(1, -1, 1, 1)) * sc + beta.double().view(1, -1, 1, 1)
        for k in kinks:
            d = z - k
            bad = d.abs() < band
            if bad.any():
                s = torch.where(d >= 0, 1.0, -1.0).double()
                x = torch.where(bad, x + (k + 2 * band * s - z) / sc, x)
        x = x.float().double()
    return x.float()


def _bn_case(C, g, training):
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rm = torch.randn(C, generator=g) * 0.1
    rv = torch.rand(C, generator=g) + 0.5
    return gamma, beta, rm, rv


def _bnconv_ref(a, op, x, skip, bn, w, dy, dtype):
    C0 = x.shape[1]
    outs = {}
    xr = x.to(dtype).requires_grad_(a["x" if op == "bn_act_conv" else "xl"][2])
    wr = w.to(dtype).requires_grad_(True)
    sk = None if skip is None else skip.to(dtype).requires_grad_(True)
    if op == "bn_act_conv":
        gamma, beta, rm, rv, training, momentum, eps, act = bn
        gr, br = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
        rmr, rvr = rm.to(dtype).clone(), rv.to(dtype).clone()
        z = F.batch_norm(xr, rmr, rvr, gr, br, training=training, momentum=momentum, eps=eps)
        h = ACTS[act](z)
        up2 = a["up2"]
    else:
        h, up2 = xr, True
    if up2:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    if sk is not None:
        h = torch.cat([h, sk], 1)
    y = F.conv2d(h, wr, None, 1, 1)
    if dy is not None:  # None: a forward-only replay
        y.backward(dy.to(dtype))
    outs[("y",)] = yd = y.detach()
    outs[("mean",)], outs[("var",)] = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    outs[("dx",)] = xr.grad
    outs[("dw",)] = wr.grad
    outs[("dskip",)] = None if sk is None else sk.grad
    if op == "bn_act_conv":
        outs[("dgamma",)], outs[("dbeta",)] = gr.grad, br.grad
        outs[("rm",)], outs[("rv",)] = rmr, rvr
    return outs


def _replay_bnconv(sig, dev, op, stage=None):
    """stage None: forward + backward of a training signature; "val" / "predict": forward only under no_grad"""
    from vision_mtl_amd import ops

    g = torch.Generator().manual_seed(zlib.crc32(repr(sig).encode()))
    a = sig_args(sig)
    xkey = "x" if op == "bn_act_conv" else "xl"
    B, H, W, Cs = a[xkey][1]
    C = a["C"] if op == "bn_act_conv" else a["C0"]
    ws = a["weight"][1]
    Cout, Cin = ws[0], ws[1]
    w = torch.randn(ws, generator=g) / (Cin * 9) ** 0.5
    skip = None
    if a["skip"] is not None:
        sb, sh, sw, _ = a["skip"][1]
        skip = torch.randn(sb, Cin - C, sh, sw, generator=g)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    big, bn = [], None
    if op == "bn_act_conv":
        _, nf, training, momentum, eps = a["bn"]
        assert nf == C
        gamma, beta, rm, rv = _bn_case(C, g, training)
        big = list(range(C - C // 4, C))
        x[:, big] = 100.0 + 0.1 * torch.randn(B, len(big), H, W, generator=g)  # large-mean / small-std input channels
        act = a["act"]
        x = _nudge(x, gamma, beta, eps, act, training, rm, rv)
        bn = (gamma, beta, rm, rv, training, momentum, eps, act)
    xd = _nhwc(x, dev).requires_grad_(a[xkey][2])
    wd = w.to(dev).requires_grad_(True)
    skd = None if skip is None else _nhwc(skip, dev).requires_grad_(a["skip"][2])
    Hy, Wy = (2 * H, 2 * W) if (op == "up2_conv" or a.get("up2")) else (H, W)
    dy = torch.randn(B, Cout, Hy, Wy, generator=g) if stage is None else None
    bnd = None
    if op == "bn_act_conv":
        bnd = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).to(dev).train(training)
        with torch.no_grad():
            bnd.weight.copy_(gamma)
            bnd.bias.copy_(beta)
            bnd.running_mean.copy_(rm)
            bnd.running_var.copy_(rv)
        st_in, rpb_in = None, a["rpb"]
        if a["stats"] is not None:
            st_in = _stats_rows(x, a["stats"][1][0], rpb_in).to(dev)
    with recording() as rec, torch.set_grad_enabled(stage is None):
        if op == "bn_act_conv":
            y, stats, orpb = ops.bn_act_conv(xd, st_in, rpb_in, bnd, C, a["act"], wd, skip=skd, up2=a["up2"],
                                             want_stats=a["want_stats"])
        else:
            y, stats = ops.up2_conv(xd, C, skd, wd, want_stats=a["want_stats"])
            orpb = None if stats is None else stats._vmtl_rpb
        if stage is None:
            y.backward(_nhwc(dy, dev))
        torch.cuda.synchronize()
    ref = _bnconv_ref(a, op, x, skip, bn, w, dy, torch.float64)
    chk = Checker(fmt_sig(sig), lambda: _bnconv_ref(a, op, x, skip, bn, w, dy, torch.float32))
    chk("y", _nchw(y, Cout), ref[("y",)], BAR_OUT, ("y",))
    if stats is not None:
        _check_stats(chk, "stats", stats, orpb, ref[("y",)], Cout, [("all", list(range(Cout)))], ())
    if stage is not None:
        if stage == "predict" and stats is not None:
            chk.failures.append(f"{chk.label}: a predict step's conv returned statistics rows")
        if op == "bn_act_conv":
            _check_buffers(chk, "", bnd, training, rm, rv, ref[("rm",)], ref[("rv",)], ("rm",), ("rv",), stage)
        return chk, rec
    if a[xkey][2]:
        dx = _nchw(xd.grad, C)
        chk("dx", dx, ref[("dx",)], BAR_GRAD, ("dx",))
        if big:  # judged on their own scale too
            chk("dx[large-mean]", dx, ref[("dx",)], BAR_GRAD, ("dx",), sel=(slice(None), big))
    chk("dw", wd.grad.cpu(), ref[("dw",)], BAR_GRAD, ("dw",))
    if skd is not None and a["skip"][2]:
        chk("dskip", _nchw(skd.grad, skip.shape[1]), ref[("dskip",)], BAR_GRAD, ("dskip",))
    if op == "bn_act_conv":
        chk("dgamma", bnd.weight.grad.cpu(), ref[("dgamma",)], BAR_GRAD, ("dgamma",))
        chk("dbeta", bnd.bias.grad.cpu(), ref[("dbeta",)], BAR_GRAD, ("dbeta",))
        chk("running_mean", bnd.running_mean.cpu(), ref[("rm",)], BAR_STATS, ("rm",))
        chk("running_var", bnd.running_var.cpu(), ref[("rv",)], BAR_STATS, ("rv",))
        assert int(bnd.num_batches_tracked) == (1 if training else 0), f"{fmt_sig(sig)}: num_batches_tracked"
    return chk, rec


# ------------------------------------------------------------------------------------------------ the other node families
class _RefBN:
    """one BatchNorm of a reference: leaves gamma / beta, cloned running buffers"""

    def __init__(self, spec, dtype):
        C, training, momentum, eps, gamma, beta, rm, rv = spec
        self.training, self.momentum, self.eps = training, momentum, eps
        self.gamma, self.beta = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
        self.rm, self.rv = rm.to(dtype).clone(), rv.to(dtype).clone()

    def __call__(self, x):
        return F.batch_norm(x, self.rm, self.rv, self.gamma, self.beta, self.training, self.momentum, self.eps)


def _dev_bn(spec, dev):
    C, training, momentum, eps, gamma, beta, rm, rv = spec
    m = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).to(dev).train(training)
    with torch.no_grad():
        m.weight.copy_(gamma)
        m.bias.copy_(beta)
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    return m


def _bn_spec(C, training, momentum, eps, g):
    return (C, training, momentum, eps) + _bn_case(C, g, training)


def _away_from_kinks(x, act, band=1e-3):
    """an activation applied to x itself (no BatchNorm in front): move the inputs within `band` of a kink away from it"""
    for k in KINKS[act]:
        d = x - k
        x = torch.where(d.abs() < band, k + 2 * band * torch.where(d >= 0, 1.0, -1.0), x)
    return x


def _spread_windows(x, gap=0.05):
    """add rank * gap inside every 2x2 window: no near-tie arg-max for two fp32 implementations to disagree on"""
    B, C, H, W = x.shape
    w = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    rank = w.argsort(-1).argsort(-1).float()
    w = w + rank * gap
    return w.reshape(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W).contiguous()


class Case:
    """inputs of one replay.  acts: NCHW activations (NHWC-padded on the device), ws: plain tensors, bns: BatchNorm specs,
    grad: names that require a gradient, stats_in: {activation name: (rows, rpb)} partial rows handed in"""

    def __init__(self):
        self.acts, self.ws, self.bns, self.grad, self.zero, self.stats_in = {}, {}, {}, set(), set(), {}


def _run_generic(sig, dev, make, ref_fn, dev_fn, identity=False, used=None, stage=None):
    """make(a, g) -> Case; ref_fn(a, case, T, bns) -> {output: NCHW tensor}; dev_fn(a, case, T, bns) -> ({output: (tensor,
    'nhwc' | 'nchw', C)}, [(output, stats, rpb)]).  Forward, backward with seeded dy per output, then every output, gradient,
    running buffer against fp64.  used: the outputs that receive a gradient (default: all).  stage "val" / "predict": a
    forward-only replay under no_grad (no dy, no gradient; the buffers as _check_buffers holds them).  The statistics rows a node
    emits are merged and held against the moments of the output the node wrote (fp64 over the HIP output; bar max(1e-5,
    4 x the error of fp32 torch moments of it)): the forward error of the output has its own check."""
    import contextlib

    from tests.util import identity_activations

    g = torch.Generator().manual_seed(zlib.crc32(repr(sig).encode()))
    a = sig_args(sig)
    case = make(a, g)
    ctx = identity_activations if identity else contextlib.nullcontext
    dys = {}

    def reference(dtype):
        T = {k: v.to(dtype).requires_grad_(k in case.grad) for k, v in list(case.acts.items()) + list(case.ws.items())}
        bns = {k: _RefBN(v, dtype) for k, v in case.bns.items()}
        with ctx(), torch.set_grad_enabled(stage is None):
            outs = ref_fn(a, case, T, bns)
        outs = {k: y for k, y in outs.items() if used is None or k in used}
        if stage is None:
            for k, y in outs.items():
                if k not in dys:
                    dys[k] = torch.randn(y.shape, generator=g)
            torch.autograd.backward([outs[k] for k in outs], [dys[k].to(dtype) for k in outs])
        res = {("y", k): y.detach() for k, y in outs.items()}
        for k, y in outs.items():
            res[("mean", k)], res[("var", k)] = y.detach().mean((0, 2, 3)), y.detach().var((0, 2, 3), unbiased=False)
        for k, t in T.items():
            if t.grad is not None:
                res[("d", k)] = t.grad
        for k, b in bns.items():
            res[("dgamma", k)], res[("dbeta", k)], res[("rm", k)], res[("rv", k)] = b.gamma.grad, b.beta.grad, b.rm, b.rv
        return res

    ref = reference(torch.float64)  # also draws the dy of every output
    Td = {k: _nhwc(v, dev).requires_grad_(k in case.grad) for k, v in case.acts.items()}
    Td.update({k: v.to(dev).requires_grad_(k in case.grad or k in case.zero) for k, v in case.ws.items()})
    bnd = {k: _dev_bn(v, dev) for k, v in case.bns.items()}
    for k, (rows, rpb) in case.stats_in.items():
        Td["stats:" + k] = _stats_rows(case.acts[k], rows, rpb).to(dev)
    with recording() as rec, torch.set_grad_enabled(stage is None):
        with ctx():
            outs, stats = dev_fn(a, case, Td, bnd)
            outs = {k: v for k, v in outs.items() if used is None or k in used}
            if stage is None:
                ys = [t for t, _, _ in outs.values()]
                gs = [(_nhwc(dys[k], dev) if lay == "nhwc" else dys[k].to(dev)) for k, (_, lay, _) in outs.items()]
                torch.autograd.backward(ys, gs)
        torch.cuda.synchronize()
    chk = Checker(fmt_sig(sig), lambda: reference(torch.float32))
    for k, (t, lay, C) in outs.items():
        chk(f"y[{k}]", _nchw(t, C) if lay == "nhwc" else t.detach().cpu(), ref[("y", k)], BAR_OUT, ("y", k))
    for k, st, rpb in stats:
        t, lay, C = outs[k]
        yh = _nchw(t.detach(), C) if lay == "nhwc" else t.detach().cpu()
        B, _, H, W = yh.shape
        mean, var = _merge(st, rpb, B * H * W, C)
        for what, got, r64, r32 in (("mean", mean, yh.double().mean((0, 2, 3)), yh.mean((0, 2, 3))),
                                    ("var", var, yh.double().var((0, 2, 3), unbiased=False), yh.var((0, 2, 3), unbiased=False))):
            mag = float(r64.abs().max())
            err, e32 = float((got - r64).abs().max()) / mag, float((r32.double() - r64).abs().max()) / mag
            chk.worst[f"stats {what}"] = max(chk.worst.get(f"stats {what}", 0.0), err)
            if err > max(BAR_STATS, 4 * e32):
                chk.failures.append(f"{chk.label} stats {what}[{k}]: {err:.2e} of the maximum (fp32 torch moments {e32:.2e})")
    if stage is not None:
        if stage == "predict" and stats:
            chk.failures.append(f"{chk.label}: a predict step's node returned statistics rows")
        for k, m in bnd.items():
            spec = case.bns[k]
            _check_buffers(chk, k, m, spec[1], spec[6], spec[7], ref[("rm", k)], ref[("rv", k)], ("rm", k), ("rv", k), stage)
        return chk, rec
    for k in case.zero:
        if float(Td[k].grad.abs().max()) != 0.0:
            chk.failures.append(f"{chk.label}: {k} feeds a train-mode BatchNorm, its gradient must be exactly zero")
    for k in case.grad:
        t = Td[k]
        got = (_nchw(t.grad, case.acts[k].shape[1]) if k in case.acts else t.grad.cpu())
        chk(f"d[{k}]", got, ref[("d", k)], BAR_GRAD, ("d", k))
    for k, m in bnd.items():
        chk(f"dgamma[{k}]", m.weight.grad.cpu(), ref[("dgamma", k)], BAR_GRAD, ("dgamma", k))
        chk(f"dbeta[{k}]", m.bias.grad.cpu(), ref[("dbeta", k)], BAR_GRAD, ("dbeta", k))
        chk(f"running_mean[{k}]", m.running_mean.cpu(), ref[("rm", k)], BAR_STATS, ("rm", k))
        chk(f"running_var[{k}]", m.running_var.cpu(), ref[("rv", k)], BAR_STATS, ("rv", k))
        if int(m.num_batches_tracked) != (1 if case.bns[k][1] else 0):
            chk.failures.append(f"{chk.label}: num_batches_tracked of {k}")
    return chk, rec


def _bn_input(case, a, g, name, C, bn_key_spec, act, B, H, W, stats_arg=None, rpb=0, pool=False):
    """random BatchNorm input with a large-mean / small-std quarter, nudged off the activation's kinks"""
    spec = bn_key_spec
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    big = list(range(C - C // 4, C))
    x[:, big] = 100.0 + 0.1 * torch.randn(B, len(big), H, W, generator=g)
    if pool:
        x = _spread_windows(x, gap=0.05 * 1.5)
        x[:, big] = _spread_windows(100.0 + 0.1 * torch.randn(B, len(big), H, W, generator=g), gap=0.005)
    x = _nudge(x, spec[4], spec[5], spec[3], act, spec[1], spec[6], spec[7])
    case.acts[name] = x
    if a[name][2]:
        case.grad.add(name)
    if stats_arg is not None:
        case.stats_in[name] = (stats_arg[1][0], rpb)
    return x


def _stats_rpb(a, key, rpb_key, B, H, W, Cs):
    from vision_mtl_amd._lib import lib

    st = a[key]
    if st is None:
        return None, 0
    rpb = a.get(rpb_key) or (st[3][1] if len(st) > 3 else 0) or lib().raw("vmtl_conv2d_stats_block")(B, H, W, Cs)
    return st, rpb


def _w(case, a, name, shape, g, fan):
    case.ws[name] = torch.randn(shape, generator=g) / fan ** 0.5
    if a[name][2]:
        case.grad.add(name)


def _b(case, a, name, n, g):
    if a.get(name) is not None:
        case.ws[name] = torch.randn(n, generator=g) * 0.1
        if a[name][2]:
            # zero_bias_grad: a train-mode BatchNorm follows, the gradient is exactly zero
            (case.zero if a.get("zero_bias_grad") else case.grad).add(name)


# bn_act(x, gamma, beta, running_mean, running_var, nbt, C, training, momentum, eps, act, mul, res, stats, stats_rpb) and
# activation(x, act, C, mul): y = act(BN(x)) [* mul] [+ res]
def _make_bn_act(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    C, act = a["C"], a["act"]
    if a.get("gamma") is not None:
        spec = _bn_spec(C, a["training"], a["momentum"], a["eps"], g)
        case.bns["bn"] = spec
        st, rpb = _stats_rpb(a, "stats", "stats_rpb", B, H, W, Cs)
        _bn_input(case, a, g, "x", C, spec, act, B, H, W, st, rpb)
    else:
        case.acts["x"] = _away_from_kinks(torch.randn(B, C, H, W, generator=g) * 2, act)
        if a["x"][2]:
            case.grad.add("x")
    for k in ("mul", "res"):
        if a.get(k) is not None:
            case.acts[k] = torch.rand(B, C, H, W, generator=g) + 0.5
            if a[k][2]:
                case.grad.add(k)
    return case


def _ref_bn_act(a, case, T, bns):
    z = bns["bn"](T["x"]) if "bn" in bns else T["x"]
    y = ACTS[a["act"]](z)
    if "mul" in T:
        y = y * T["mul"]
    if "res" in T:
        y = y + T["res"]
    return {"y": y}


def _dev_bn_act(a, case, T, bns):
    from vision_mtl_amd import ops

    C = a["C"]
    if "bn" in bns:
        m = bns["bn"]
        y = ops.bn_act(T["x"], m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked, C, a["training"],
                       a["momentum"], a["eps"], a["act"], mul=T.get("mul"), res=T.get("res"), stats=T.get("stats:x"),
                       stats_rpb=case.stats_in.get("x", (0, 0))[1])
    else:
        y = ops.activation(T["x"], a["act"], C, mul=T.get("mul"))
    return {"y": (y, "nhwc", C)}, []


# bn_act_pool2(x, gamma, beta, running_mean, running_var, nbt, C, training, momentum, eps, act, stats, stats_rpb)
def _make_bn_act_pool2(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    spec = _bn_spec(a["C"], a["training"], a["momentum"], a["eps"], g)
    case.bns["bn"] = spec
    st, rpb = _stats_rpb(a, "stats", "stats_rpb", B, H, W, Cs)
    _bn_input(case, a, g, "x", a["C"], spec, a["act"], B, H, W, st, rpb, pool=True)
    return case


def _ref_bn_act_pool2(a, case, T, bns):
    return {"y": F.max_pool2d(ACTS[a["act"]](bns["bn"](T["x"])), 2)}


def _dev_bn_act_pool2(a, case, T, bns):
    from vision_mtl_amd import ops

    m = bns["bn"]
    y = ops.bn_act_pool2(T["x"], m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked, a["C"],
                         a["training"], a["momentum"], a["eps"], a["act"], stats=T.get("stats:x"),
                         stats_rpb=case.stats_in.get("x", (0, 0))[1])
    return {"y": (y, "nhwc", a["C"])}, []


# bn_act_conv1x1(x, stats, rpb, bn, C, act, weight, bias, want_stats, zero_bias_grad, res, return_act)
def _make_bn_act_conv1x1(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    _, C, training, momentum, eps = a["bn"]
    spec = _bn_spec(C, training, momentum, eps, g)
    case.bns["bn"] = spec
    st = a["stats"]
    _bn_input(case, a, g, "x", C, spec, a["act"], B, H, W, st, a["rpb"])
    Cout, Cin = a["weight"][1][:2]
    _w(case, a, "weight", a["weight"][1], g, Cin)
    _b(case, a, "bias", Cout, g)
    if a["res"] is not None:
        case.acts["res"] = torch.randn(B, C, H, W, generator=g)
        if a["res"][2]:
            case.grad.add("res")
    return case


def _ref_bn_act_conv1x1(a, case, T, bns):
    h = ACTS[a["act"]](bns["bn"](T["x"]))
    if "res" in T:
        h = h + T["res"]
    out = {"y": F.conv2d(h, T["weight"], T.get("bias"))}
    if a["return_act"]:
        out["a"] = h
    return out


def _dev_bn_act_conv1x1(a, case, T, bns):
    from vision_mtl_amd import ops

    out = ops.bn_act_conv1x1(T["x"], T.get("stats:x"), a["rpb"], bns["bn"], a["C"], a["act"], T["weight"], bias=T.get("bias"),
                             want_stats=a["want_stats"], zero_bias_grad=a["zero_bias_grad"], res=T.get("res"),
                             return_act=a["return_act"])
    Cout = a["weight"][1][0]
    outs = {"y": (out[0], "nhwc", Cout)}
    if a["return_act"]:
        outs["a"] = (out[3], "nhwc", a["C"])
    return outs, ([("y", out[1], out[2])] if out[1] is not None else [])


# bn_act_dwconv(x, stats, rpb, bn, C, act, weight, stride, pad, want_stats, return_act) / dwconv(x, weight, stride, pad)
def _make_dw(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    ws = a["weight"][1]
    C = ws[0]
    if a.get("bn") is not None:
        _, nf, training, momentum, eps = a["bn"]
        spec = _bn_spec(nf, training, momentum, eps, g)
        case.bns["bn"] = spec
        _bn_input(case, a, g, "x", nf, spec, a["act"], B, H, W, a["stats"], a["rpb"])
    else:
        case.acts["x"] = torch.randn(B, C, H, W, generator=g)
        if a["x"][2]:
            case.grad.add("x")
    _w(case, a, "weight", ws, g, ws[2] * ws[3])
    return case


def _ref_dw(a, case, T, bns):
    h = ACTS[a["act"]](bns["bn"](T["x"])) if "bn" in bns else T["x"]
    out = {"y": F.conv2d(h, T["weight"], None, a["stride"], a["pad"], 1, h.shape[1])}
    if a.get("return_act"):
        out["a"] = h
    return out


def _dev_dw(a, case, T, bns):
    from vision_mtl_amd import ops

    C = a["weight"][1][0]
    if "bn" not in bns:
        return {"y": (ops.dwconv(T["x"], T["weight"], a["stride"], a["pad"]), "nhwc", C)}, []
    out = ops.bn_act_dwconv(T["x"], T.get("stats:x"), a["rpb"], bns["bn"], a["C"], a["act"], T["weight"], a["stride"], a["pad"],
                            want_stats=a["want_stats"], return_act=a["return_act"])
    outs = {"y": (out[0], "nhwc", C)}
    if a["return_act"]:
        outs["a"] = (out[3], "nhwc", a["C"])
    return outs, ([("y", out[1], out[2])] if out[1] is not None else [])


# conv1x1_cat(xa, xb, Cb, weight, bias, want_stats, zero_bias_grad): conv1x1(cat[xa, xb[:Cb]])
def _make_cat(a, g):
    case = Case()
    B, H, W, Ca = a["xa"][1]
    for k, C in (("xa", Ca), ("xb", a["Cb"])):
        case.acts[k] = torch.randn(B, C, H, W, generator=g)
        if a[k][2]:
            case.grad.add(k)
    Cout, Cin = a["weight"][1][:2]
    _w(case, a, "weight", a["weight"][1], g, Cin)
    _b(case, a, "bias", Cout, g)
    return case


def _ref_cat(a, case, T, bns):
    return {"y": F.conv2d(torch.cat([T["xa"], T["xb"]], 1), T["weight"], T.get("bias"))}


def _dev_cat(a, case, T, bns):
    from vision_mtl_amd import ops

    y, st = ops.conv1x1_cat(T["xa"], T["xb"], a["Cb"], T["weight"], bias=T.get("bias"), want_stats=a["want_stats"],
                            zero_bias_grad=a["zero_bias_grad"])
    return {"y": (y, "nhwc", a["weight"][1][0])}, ([("y", st, st._vmtl_rpb)] if st is not None else [])


# conv_transpose2x2(x, weight, bias): weight (Cin, Cout, 2, 2), stride 2
def _make_convt(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    Cin, Cout = a["weight"][1][:2]
    case.acts["x"] = torch.randn(B, Cin, H, W, generator=g)
    if a["x"][2]:
        case.grad.add("x")
    _w(case, a, "weight", a["weight"][1], g, Cin)
    _b(case, a, "bias", Cout, g)
    return case


def _ref_convt(a, case, T, bns):
    return {"y": F.conv_transpose2d(T["x"], T["weight"], T.get("bias"), stride=2)}


def _dev_convt(a, case, T, bns):
    from vision_mtl_amd import ops

    return {"y": (ops.conv_transpose2x2(T["x"], T["weight"], T.get("bias")), "nhwc", a["weight"][1][1])}, []


# squeeze_excite(x, w_reduce, b_reduce, w_expand, b_expand, act1, act2): x * act2(W_e act1(W_r mean_hw(x) + b_r) + b_e)
def _make_se(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    R, C = a["w_reduce"][1][:2]
    case.acts["x"] = torch.randn(B, C, H, W, generator=g) + 0.2
    if a["x"][2]:
        case.grad.add("x")
    _w(case, a, "w_reduce", a["w_reduce"][1], g, C)
    _b(case, a, "b_reduce", R, g)
    _w(case, a, "w_expand", a["w_expand"][1], g, R / 9.0)  # gate pre-activations of order 1
    _b(case, a, "b_expand", C, g)
    return case


def _ref_se(a, case, T, bns):
    s = T["x"].mean((2, 3), keepdim=True)
    s = ACTS[a["act1"]](F.conv2d(s, T["w_reduce"], T["b_reduce"]))
    s = ACTS[a["act2"]](F.conv2d(s, T["w_expand"], T["b_expand"]))
    return {"y": T["x"] * s}


def _dev_se(a, case, T, bns):
    from vision_mtl_amd import ops

    y = ops.squeeze_excite(T["x"], T["w_reduce"], T["b_reduce"], T["w_expand"], T["b_expand"], a["act1"], a["act2"])
    return {"y": (y, "nhwc", a["w_reduce"][1][1])}, []


# decoder_tail(x1, stats1, rpb1, bn1, conv2_weight, bn2, wa, ba, wb, bb) -> (head_a, head_b) NCHW.  Two ReLUs inside the
# node cannot both be kept off their kink by choosing x1: replayed under identity activations (tests/util.py)
def _make_tail(a, g):
    case = Case()
    B, H, W, Cs = a["x1"][1]
    _, C1, tr1, m1, e1 = a["bn1"]
    _, C2, tr2, m2, e2 = a["bn2"]
    case.bns["bn1"], case.bns["bn2"] = _bn_spec(C1, tr1, m1, e1, g), _bn_spec(C2, tr2, m2, e2, g)
    _bn_input(case, a, g, "x1", C1, case.bns["bn1"], 0, B, H, W, a["stats1"], a["rpb1"])
    _w(case, a, "conv2_weight", a["conv2_weight"][1], g, C1 * 9)
    for w, b in (("wa", "ba"), ("wb", "bb")):
        _w(case, a, w, a[w][1], g, C2 * 9)
        _b(case, a, b, a[w][1][0], g)
    return case


def _ref_tail(a, case, T, bns):
    h = F.relu(bns["bn1"](T["x1"]))
    h = F.relu(bns["bn2"](F.conv2d(h, T["conv2_weight"], None, 1, 1)))
    return {"a": F.conv2d(h, T["wa"], T.get("ba"), 1, 1), "b": F.conv2d(h, T["wb"], T.get("bb"), 1, 1)}


def _dev_tail(a, case, T, bns):
    from vision_mtl_amd import ops

    ya, yb = ops.decoder_tail(T["x1"], T.get("stats:x1"), a["rpb1"], bns["bn1"], T["conv2_weight"], bns["bn2"], T["wa"],
                              T.get("ba"), T["wb"], T.get("bb"))
    return {"a": (ya, "nchw", None), "b": (yb, "nchw", None)}, []


# bn_act_pool3(x, bn, C, act, stats, stats_rpb) -> (act(BN(x)), maxpool3x3/s2/p1 of it): the ResNet stem
def _pool3_ladder(B, C, H, W, spec, g, big, hole=16):
    """BatchNorm input of the stem pool: every (b, c) plane is a random permutation of one ladder of H*W values, so no two
    values of a plane (hence of any overlapping 3x3/s2 window) are closer than one step: 2^-11 around 0.3 (2048 ulps at
    magnitude 2) on ordinary channels, 2^-14 around 100 (8 ulps at that magnitude) on the large-mean / small-std quarter
    `big`.  The ladder has a `hole`-step gap, and beta is chosen so that the BatchNorm maps the ReLU kink to the middle of
    it: every normalised value lies >= hole/2 steps (>= 1.6e-3 after normalisation) from the kink.  Exact ties between ReLU
    zeros stay (both sides take the first maximum)."""
    _, training, momentum, eps, gamma, beta, rm, rv = spec
    N = H * W
    x = torch.empty(B, C, H, W, dtype=torch.float64)
    beta = beta.clone()
    for c in range(C):
        step, centre = (2.0 ** -14, 100.0) if c in big else (2.0 ** -11, 0.3 + 0.25 * (c % 5))
        kh = int(N * (0.3 + 0.4 * float(torch.rand(1, generator=g))))  # the ReLU zeros: 30..70 % of the plane
        k = torch.arange(N, dtype=torch.float64)
        ladder = centre + step * torch.round(k - N / 2 + hole * (k >= kh))
        if training:
            mean, var = float(ladder.mean()), float(ladder.var(unbiased=False))
        else:
            mean, var = float(rm[c]), float(rv[c])
        kink = float(ladder[kh - 1] + ladder[kh]) / 2  # the hole's centre
        beta[c] = -float(gamma[c]) * (kink - mean) / (var + eps) ** 0.5
        perm = torch.rand(B, N, generator=g).argsort(1)
        x[:, c] = ladder[perm].view(B, H, W)
    return x.float(), spec[:5] + (beta,) + spec[6:]


def _make_bn_act_pool3(a, g):
    case = Case()
    B, H, W, Cs = a["x"][1]
    _, C, training, momentum, eps = a["bn"]
    assert a["act"] == 1, "the stem pool's inputs are laid out around the ReLU kink"
    big = list(range(C - C // 4, C))
    x, spec = _pool3_ladder(B, C, H, W, _bn_spec(C, training, momentum, eps, g), g, big)
    case.bns["bn"] = spec
    case.acts["x"] = x
    if a["x"][2]:
        case.grad.add("x")
    st, rpb = _stats_rpb(a, "stats", "stats_rpb", B, H, W, Cs)
    if st is not None:
        case.stats_in["x"] = (st[1][0], rpb)
    return case


def _ref_bn_act_pool3(a, case, T, bns):
    h = ACTS[a["act"]](bns["bn"](T["x"]))
    return {"a": h, "y": F.max_pool2d(h, 3, 2, 1)}


def _dev_bn_act_pool3(a, case, T, bns):
    from vision_mtl_amd import ops

    h, y = ops.bn_act_pool3(T["x"], bns["bn"], a["C"], a["act"], stats=T.get("stats:x"),
                            stats_rpb=case.stats_in.get("x", (0, 0))[1])
    return {"a": (h, "nhwc", a["C"]), "y": (y, "nhwc", a["C"])}, []


# bn_add_act(z, stats, rpb, bn, C, act, res, zd, statsd, rpbd, bn_d) -> act(BN_a(z) + res)  or  act(BN_a(z) + BN_d(zd)):
# the close of a ResNet BasicBlock, each BatchNorm fed its own conv's partial rows
def _bn_affine64(x, spec):
    """(BN(x) in fp64 with the statistics this spec uses, per-channel scale gamma * invstd)"""
    C, training, momentum, eps, gamma, beta, rm, rv = spec
    x = x.double()
    mean, var = (x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)) if training else (rm.double(), rv.double())
    sc = (gamma.double() / (var + eps).sqrt()).view(1, -1, 1, 1)
    return (x - mean.view(1, -1, 1, 1)) * sc + beta.double().view(1, -1, 1, 1), sc


def _make_bn_add_act(a, g):
    case = Case()
    B, H, W, Cs = a["z"][1]
    C, act = a["C"], a["act"]
    _, nf, training, momentum, eps = a["bn"]
    case.bns["a"] = _bn_spec(nf, training, momentum, eps, g)
    st, rpb = _stats_rpb(a, "stats", "rpb", B, H, W, Cs)
    _bn_input(case, a, g, "z", C, case.bns["a"], 0, B, H, W, st, rpb)
    if a["zd"] is not None:
        _, nf, training, momentum, eps = a["bn_d"]
        case.bns["d"] = _bn_spec(nf, training, momentum, eps, g)
        std, rpbd = _stats_rpb(a, "statsd", "rpbd", B, H, W, Cs)
        _bn_input(case, a, g, "zd", C, case.bns["d"], 0, B, H, W, std, rpbd)
        short = "zd"
    else:
        case.acts["res"] = torch.randn(B, C, H, W, generator=g)
        if a["res"][2]:
            case.grad.add("res")
        short = "res"
    # the kink is on the SUM: move the shortcut's input until no BN_a(z) + r lies within 1e-3 of it
    za = _bn_affine64(case.acts["z"], case.bns["a"])[0]
    band = 1e-3
    for k in KINKS[act]:
        for _ in range(3):
            r, sc = _bn_affine64(case.acts["zd"], case.bns["d"]) if short == "zd" else (case.acts["res"].double(), 1.0)
            d = za + r - k
            bad = d.abs() < band
            if not bad.any():
                break
            t = k + 2 * band * torch.where(d >= 0, 1.0, -1.0).double()
            case.acts[short] = torch.where(bad, case.acts[short].double() + (t - d - k) / sc, case.acts[short].double()).float()
    return case


def _ref_bn_add_act(a, case, T, bns):
    r = bns["d"](T["zd"]) if "d" in bns else T["res"]
    return {"y": ACTS[a["act"]](bns["a"](T["z"]) + r)}


def _dev_bn_add_act(a, case, T, bns):
    from vision_mtl_amd import ops

    y = ops.bn_add_act(T["z"], T.get("stats:z"), case.stats_in.get("z", (0, 0))[1], bns["a"], a["C"], a["act"],
                       res=T.get("res"), zd=T.get("zd"), statsd=T.get("stats:zd"), rpbd=case.stats_in.get("zd", (0, 0))[1],
                       bn_d=bns.get("d"))
    return {"y": (y, "nhwc", a["C"])}, []


GENERIC = {
    "bn_act": (_make_bn_act, _ref_bn_act, _dev_bn_act, False),
    "activation": (_make_bn_act, _ref_bn_act, _dev_bn_act, False),
    "bn_act_pool2": (_make_bn_act_pool2, _ref_bn_act_pool2, _dev_bn_act_pool2, False),
    "bn_act_conv1x1": (_make_bn_act_conv1x1, _ref_bn_act_conv1x1, _dev_bn_act_conv1x1, False),
    "bn_act_dwconv": (_make_dw, _ref_dw, _dev_dw, False),
    "dwconv": (_make_dw, _ref_dw, _dev_dw, False),
    "conv1x1_cat": (_make_cat, _ref_cat, _dev_cat, False),
    "conv_transpose2x2": (_make_convt, _ref_convt, _dev_convt, False),
    "squeeze_excite": (_make_se, _ref_se, _dev_se, False),
    "decoder_tail": (_make_tail, _ref_tail, _dev_tail, True),
    "bn_act_pool3": (_make_bn_act_pool3, _ref_bn_act_pool3, _dev_bn_act_pool3, False),
    "bn_add_act": (_make_bn_add_act, _ref_bn_add_act, _dev_bn_add_act, False),
}
REPLAYED = ("conv2d", "bn_act_conv", "up2_conv") + tuple(GENERIC)
IDENTITY_REPLAYED = tuple(k for k, v in GENERIC.items() if v[3])


@functools.lru_cache(maxsize=None)
def _replay(sig, stage=None):
    """stage None: the training replay (forward + backward).  "val" / "predict": the forward-only replay of a signature
    of that stage's census, under no_grad and with the activations as they are (a forward value is continuous in its
    inputs: no node needs identity activations)."""
    dev = torch.device("cuda:0")
    if sig[0] == "conv2d":
        chk, rec = _replay_conv2d(sig, dev, stage)
    elif sig[0] in GENERIC:
        make, ref_fn, dev_fn, identity = GENERIC[sig[0]]
        identity = identity and stage is None
        chk, rec = _run_generic(sig, dev, make, ref_fn, dev_fn, identity, stage=stage)
        if stage is None and sig_args(sig).get("return_act"):  # the activation handed back may also receive no gradient at all
            chk2, rec2 = _run_generic(sig, dev, make, ref_fn, dev_fn, identity, used=("y",))
            chk.failures += chk2.failures
            chk.relaxed += chk2.relaxed
            rec.launches += rec2.launches
            chk2.ref32_fn = chk2._ref32 = None
    else:
        chk, rec = _replay_bnconv(sig, dev, sig[0], stage)
    chk.ref32_fn = chk._ref32 = None  # the cache keeps the verdict, not the tensors
    torch.cuda.empty_cache()
    norm = _no_act if sig[0] in IDENTITY_REPLAYED and stage is None else (lambda k: k)
    return chk, set((n, norm(k)) for _, n, k, _ in rec.launches)


@pytest.mark.parametrize("op", REPLAYED)
def test_production_nodes_match_fp64(censuses, op):
    sigs = _signatures(censuses, op)
    assert sigs, f"the census found no {op} node"
    failures, relaxed, worst, uncovered = [], [], {}, []
    for sig, prod in sigs.items():
        chk, launched = _replay(sig)
        failures += chk.failures
        relaxed += chk.relaxed
        for k, v in chk.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if op in IDENTITY_REPLAYED:
            prod = {(n, _no_act(k)) for n, k in prod}
        miss = sorted(prod - launched)
        if miss:
            uncovered.append(f"{fmt_sig(sig)}: production launches the replay did not: "
                             + "; ".join(fmt_launch(n, k) for n, k in miss))
    print(f"{op}: {len(sigs)} unique production signatures; worst error per tensor vs fp64: "
          + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
    for r in relaxed:
        print("  needed the fp32-CPU bar:", r)
    assert not failures, "\n".join(failures)
    assert not uncovered, "\n".join(uncovered)


FAMILIES = ("vmtl_conv", "vmtl_bn_", "vmtl_dwconv", "vmtl_pack", "vmtl_unpack", "vmtl_fc_")


def _no_act(key):
    """a launch key without its activation codes (nodes replayed under identity activations)"""
    return tuple((k, v) for k, v in key if not (k == "act" or k.endswith("_act") or k.startswith("act")))


def test_every_production_launch_is_replayed(censuses):
    """Every production launch of the conv, BatchNorm, depthwise, pack / unpack and pointwise families - whichever node it
    belongs to, launches outside any node included - is among the launches of the fp64-checked replays."""
    replayed = set()
    for op in REPLAYED:
        for sig in _signatures(censuses, op):
            launched = _replay(sig)[1]
            replayed |= launched
            if op in IDENTITY_REPLAYED:
                replayed |= {(n, _no_act(k)) for n, k in launched}
    missing = {}
    for name, c in censuses.items():
        for tag, n, k, phase in c.launches:
            if not n.startswith(FAMILIES):
                continue
            key = _no_act(k) if tag is not None and tag[0] in IDENTITY_REPLAYED else k
            if (n, key) not in replayed:
                missing.setdefault(f"{name} {'(no node)' if tag is None else fmt_sig(tag)} [{phase}]", set()).add(fmt_launch(n, k))
    n_fam = sum(1 for c in censuses.values() for _, n, _, _ in c.launches if n.startswith(FAMILIES))
    print(f"family launches in the census: {n_fam}; unique replayed launches: {len(replayed)}")
    assert not missing, "production launches no replay made:\n" + "\n".join(f"{k}: {sorted(v)}" for k, v in missing.items())


# ------------------------------------------------------------------------------------------------ intended routes
def _fwd_entries(census, sig):
    return {n for n, _ in census.node_launches(sig, phase="fwd")}


def _narrow3x3(a):
    B, H, W, Cs = a["x"][1]
    return (a["weight"][1][2:] == (3, 3) and a["stride"] == 1 and Cs <= 36 and ceil4(a["weight"][1][0]) <= 36
            and B * H * W >= 1 << 16)


# (configuration, node, predicate on its arguments, entry point its launches must include, description[, phase 'fwd' | 'bwd'])
def _route(cfg, op, pred, entry, what, phase="fwd"):
    return cfg, op, pred, entry, what, phase


ROUTES = [
    _route("csnet_layer_128x256_bs32", "conv2d", lambda a: _narrow3x3(a) and a["want_stats"],
           "vmtl_conv3x3_small", "narrow full-resolution 3x3 convs with the statistics epilogue"),
    _route("csnet_layer_128x256_bs32", "conv2d", lambda a: _narrow3x3(a) and not a["want_stats"],
           "vmtl_conv3x3_small", "narrow full-resolution 3x3 heads without the statistics epilogue"),
    _route("basic_128x256_bs32", "decoder_tail", lambda a: True,
           "vmtl_conv3x3_small", "the decoder tail's narrow full-resolution conv and heads"),
    _route("basic_128x256_bs32", "bn_act_conv", lambda a: not a["up2"] and a["x"][1][3] in (64, 68),
           "vmtl_conv3x3_halo", "64/68-channel decoder 3x3 convs"),
    _route("mtan_256x256_bs16", "bn_act_conv", lambda a: not a["up2"] and a["x"][1][3] in (64, 68) and a["weight"][1][0] in (64, 68),
           "vmtl_conv3x3_halo", "64/68-channel 3x3 convs"),
    _route("basic_128x256_bs32", "bn_act_conv", lambda a: a["up2"] and a["weight"][1][0] <= 36,
           "vmtl_conv2d_up2_halo", "narrow UP2 decoder convs"),
    _route("mtan_256x256_bs16", "conv2d", lambda a: a["weight"][1][2:] == (1, 1) and a["x"][1][0] * a["x"][1][1] * a["x"][1][2] == 1 << 20,
           "vmtl_conv1x1_fwd", "M = 2^20 1x1 convs on the pointwise kernel"),
    _route("basic_resnet34_128x256_bs32", "bn_add_act", lambda a: True,
           "vmtl_bn_add_act_fwd", "ResNet residual closes"),
    _route("basic_resnet34_128x256_bs32", "bn_act_pool3", lambda a: True,
           "vmtl_bn_act_pool3s2_fwd", "ResNet stem BatchNorm + ReLU + max-pool"),
    _route("basic_resnet34_128x256_bs32", "conv2d", lambda a: a["x"][2] and _s2_dgrad(a),
           "vmtl_conv2d_dgrad_s2", "ResNet stride-2 data gradients", "bwd"),
    _route("basic_resnet34_128x256_bs8", "conv2d", lambda a: a["x"][2] and _s2_dgrad(a),
           "vmtl_conv2d_dgrad_s2", "ResNet stride-2 data gradients at bs 8", "bwd"),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[4] for r in ROUTES])
def test_production_layers_take_the_intended_route(censuses, route):
    cfg, op, pred, entry, what, phase = route
    c = censuses[cfg]
    layers = [sig for sig in c.nodes if sig[0] == op and pred(sig_args(sig))]
    assert layers, f"{cfg}: no {op} layer matches '{what}' (the census changed: revisit this list)"
    ran = lambda sig: {n for n, _ in c.node_launches(sig, phase=phase)}
    wrong = [f"{fmt_sig(sig)} ran {sorted(ran(sig))} in its {phase}" for sig in layers if entry not in ran(sig)]
    assert not wrong, f"{cfg}: {what} should run on {entry}:\n" + "\n".join(wrong)


@pytest.mark.parametrize("cfg", [k for k in CONFIGS if "resnet" in k])
def test_resnet_encoder_has_no_2x2_pool(censuses, cfg):
    """the stem pool is the fused 3x3/s2 node; the 2x2 max-pool of the MobileNet / MTAN paths never runs"""
    pools = sorted({n for _, n, _, _ in censuses[cfg].launches if n.startswith(("vmtl_maxpool2", "vmtl_bn_act_pool2"))})
    assert not pools, f"{cfg}: {pools}"


# ------------------------------------------------------------------------------------------------ stride-2 phase routes
def _s2_dim(a, K, pad):
    """csrc/resnet.hip s2_dim: (taps, correlation pad) of phase a (0 / 1) of one axis"""
    k0 = (a + pad) & 1
    T = (K - k0 + 1) // 2 if k0 < K else 0
    return T, (T - 1) - (a + pad - k0) // 2 if T else 0


def _s2_phases(B, H, W, Cs, Ho, Wo, ldy, K, pad):
    """csrc/resnet.hip s2_geometry restated: ([(taps h, taps w), launch pad, e, Hp, Wp] per phase with pixels, workspace
    floats).  The launch route of a phase follows vmtl_conv2d_dgrad_s2_p (fp32)."""
    from vision_mtl_amd._lib import lib

    ksplit = lib().raw("vmtl_conv2d_ksplit")
    d = [_s2_dim(a, K, pad) for a in (0, 1)]
    pc = d[0][1] if d[0][0] else d[1][1]
    phases, ws, split = [], 0, 0
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        T = (d[a][0], d[b][0])
        Ha, Wa = (H - a + 1) // 2, (W - b + 1) // 2
        if 0 in T or Ha == 0 or Wa == 0:
            continue
        e = max(0, Ha + T[0] - 1 - Ho - 2 * pc, Wa + T[1] - 1 - Wo - 2 * pc)
        p = pc + e
        Hp, Wp = Ho + 2 * p - T[0] + 1, Wo + 2 * p - T[1] + 1
        ws += B * Cs * Hp * Wp
        ks = ksplit(B, Hp, Wp, Cs, T[0] * T[1] * ldy)
        if ks > 1:
            split = max(split, ks * B * Hp * Wp * Cs)
        if T == (1, 1) and p == 0 and B * Hp * Wp <= 1 << 21:
            route = "pointwise"
        else:
            route = "split-K" if ks > 1 else "implicit GEMM"
        phases.append((ph, T, p, e, Hp, Wp, ks, route))
    return phases, ws + split


def test_stride2_data_gradient_phase_routes(censuses):
    """Every replayed stride-2 data gradient, phase by phase: the route vmtl_conv2d_dgrad_s2 takes (the pointwise GEMM for
    unpadded single-tap phases, split-K implicit GEMM where vmtl_conv2d_ksplit > 1, else the plain implicit GEMM), from
    the phase geometry restated here and the library's split count.  The restatement's workspace size must equal
    vmtl_conv2d_dgrad_s2_ws; across the production replays all three routes must occur, each in a replay that passed fp64."""
    from vision_mtl_amd._lib import lib

    wsf = lib().raw("vmtl_conv2d_dgrad_s2_ws")
    routes, lines, failed = {}, [], []
    for sig in _signatures(censuses, "conv2d"):
        a = sig_args(sig)
        if not (a["x"][2] and _s2_dgrad(a)):
            continue
        B, H, W, Cs = a["x"][1]
        Cout, _, K, _ = a["weight"][1]
        pad = a["pad"][0] if isinstance(a["pad"], (tuple, list)) else a["pad"]
        Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
        ldy = ceil4(Cout)
        phases, ws = _s2_phases(B, H, W, Cs, Ho, Wo, ldy, K, pad)
        assert ws == wsf(B, H, W, Cs, Ho, Wo, ldy, K, pad), f"{fmt_sig(sig)}: phase geometry restatement drifted"
        chk, launched = _replay(sig)
        assert any(n == "vmtl_conv2d_dgrad_s2" for n, _ in launched), f"{fmt_sig(sig)}: no vmtl_conv2d_dgrad_s2 launch"
        if chk.failures:
            failed.append(fmt_sig(sig))
        for ph, T, p, e, Hp, Wp, ks, route in phases:
            routes.setdefault(route, []).append(fmt_sig(sig))
            lines.append(f"  {fmt_sig(sig)} phase {ph}: taps {T[0]}x{T[1]} pad {p} (e {e}) -> {Hp}x{Wp}, ksplit {ks}: {route}")
    print("stride-2 data-gradient phases:\n" + "\n".join(lines))
    assert not failed, f"replays that failed fp64: {failed}"
    missing = {"pointwise", "split-K", "implicit GEMM"} - set(routes)
    assert not missing, f"no replayed stride-2 data-gradient phase takes the {sorted(missing)} route"
