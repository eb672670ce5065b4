"""-m gpu: every node of the forward-only production steps at its production shape against a float64 CPU restatement.

The validation / test step (train mode under no_grad: batch statistics, the running buffers move) and the predict step (eval
mode: running statistics, nothing moves) are what GraphedEval captures.  They run other launches than the training step:
every conv of a predict step runs without the statistics epilogue, so ops.conv_plan may route a shape to a kernel the
training step never uses for it; eval-mode BatchNorm feeds the fused prologues from vmtl_bn_eval_stats / _coef; a node that
needs no backward keeps no activation (a_out absent).  tests/production.py takes the census of one eager step per BASELINE
configuration and stage; every unique signature of the nodes in REPLAYED is replayed alone, forward only under no_grad, by
the replays of tests/test_production_layers_gpu.py in their forward-only mode (same case builders, same fp64 restatements,
same bars, real activations) and held to
  - the output and the activation a node hands back (1e-4 of the reference's maximum);
  - val: the statistics rows merged with the node's own rows-per-block (1e-5; ordinary and large-mean channel sets), the
    running buffers after the call (1e-5) and num_batches_tracked + 1;
  - predict: running buffers and num_batches_tracked bitwise unchanged, no statistics rows returned.
A tensor that misses its bar is held to max(bar, 4 x the fp32 CPU restatement's own error); every such case is printed.
Every val / predict production launch of the conv, BatchNorm, depthwise, pack / unpack and pointwise families must be among
the replays' launches, and the route list at the end names the entry points ops.conv_plan / ops.up2_plan intend for the
forward-only launches (read from that code by hand, not computed by calling it).
"""
import pytest

from tests.production import CONFIGS, fmt_launch, fmt_sig, production_census, sig_args
from tests.test_production_layers_gpu import FAMILIES, REPLAYED, _narrow3x3, _replay
from tests.util import ceil4

pytestmark = pytest.mark.gpu

STAGES = ("val", "predict")
# covered by tests/test_production_eval_step_gpu.py (the captured predict step): the table launch replaces the per-layer ones
ELSEWHERE = ("vmtl_bn_eval_stats_batch",)


@pytest.fixture(scope="module")
def censuses(dev):
    """{stage: {configuration: census}}, 'train' included (the route comparison needs it)"""
    out = {}
    for stage in ("train",) + STAGES:
        out[stage] = {}
        for name in CONFIGS:
            c = production_census(name, stage)
            if stage != "train":
                print(c.report())
            out[stage][name] = c
    return out


def _signatures(censuses, stage, op):
    """unique signatures of one node across the configurations of a stage -> production launches (set) of each"""
    sigs = {}
    for c in censuses[stage].values():
        for sig in c.nodes:
            if sig[0] == op:
                sigs.setdefault(sig, set()).update(c.node_launches(sig))
    return sigs


@pytest.mark.parametrize("op", REPLAYED)
@pytest.mark.parametrize("stage", STAGES)
def test_forward_only_nodes_match_fp64(censuses, stage, op):
    sigs = _signatures(censuses, stage, op)
    if not sigs:  # the coverage proof below holds whatever the step launched instead
        print(f"{stage} {op}: no such node in this stage")
        return
    failures, relaxed, worst, uncovered = [], [], {}, []
    for sig, prod in sigs.items():
        chk, launched = _replay(sig, stage)
        failures += chk.failures
        relaxed += chk.relaxed
        for k, v in chk.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
        miss = sorted(prod - launched)
        if miss:
            uncovered.append(f"{fmt_sig(sig)}: production launches the replay did not: "
                             + "; ".join(fmt_launch(n, k) for n, k in miss))
    print(f"{stage} {op}: {len(sigs)} unique forward-only signatures; worst error per tensor vs fp64: "
          + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
    for r in relaxed:
        print("  needed the fp32-CPU bar:", r)
    assert not failures, "\n".join(failures)
    assert not uncovered, "\n".join(uncovered)


@pytest.mark.parametrize("stage", STAGES)
def test_every_forward_only_production_launch_is_replayed(censuses, stage):
    """Every val / predict production launch of the conv, BatchNorm, depthwise, pack / unpack and pointwise families -
    whichever node it belongs to, launches outside any node included - is among the launches of the fp64-checked
    forward-only replays of that stage."""
    replayed, nsig = set(), 0
    for op in REPLAYED:
        for sig in _signatures(censuses, stage, op):
            replayed |= _replay(sig, stage)[1]
            nsig += 1
    missing, n_fam = {}, 0
    for name, c in censuses[stage].items():
        for tag, n, k, phase in c.launches:
            if not n.startswith(FAMILIES) or n in ELSEWHERE:
                continue
            n_fam += 1
            assert phase != "bwd", f"{name}: a backward launch in a {stage} step: {fmt_launch(n, k)}"
            if (n, k) not in replayed:
                missing.setdefault(f"{name} {'(no node)' if tag is None else fmt_sig(tag)}", set()).add(fmt_launch(n, k))
    print(f"{stage}: {nsig} unique forward-only signatures replayed; family launches in the census: {n_fam}; unique "
          f"replayed launches: {len(replayed)}")
    assert n_fam, f"the {stage} census holds no family launch"
    assert not missing, f"{stage} production launches no replay made:\n" + "\n".join(f"{k}: {sorted(v)}" for k, v in missing.items())


# ------------------------------------------------------------------------------------------------ intended routes
# ops.conv_plan without an epilogue (every conv of a predict step; the heads of a val step), read from the code: a 1x1 /
# stride 1 / pad 0 conv of <= 2^21 rows is "pw"; else a 3x3 / stride 1 / pad 1 conv with ceil4(Cout) <= 36, >= 2^16 rows and
# vmtl_conv3x3_small_supported is "small" (the whole-4x32-tile condition binds only with an epilogue); else, fp32, >= 2^16
# rows, no K split and vmtl_conv3x3_halo_supported (64/68 storage channels in and out) is "mid_halo" (stat_rows > 0 binds
# only with an epilogue); else split K or the implicit GEMM.  ops.up2_plan: the route does not depend on want_stats.
def _route(cfg, stage, op, pred, entry, what):
    return cfg, stage, op, pred, entry, what


_mid = lambda a: not a["up2"] and a["x"][1][3] in (64, 68)
ROUTES = [
    _route("csnet_layer_128x256_bs32", "predict", "conv2d", lambda a: _narrow3x3(a) and not a["want_stats"],
           "vmtl_conv3x3_small", "predict: narrow full-resolution 3x3 convs and heads"),
    _route("csnet_channel_128x256_bs32", "predict", "conv2d", lambda a: _narrow3x3(a) and not a["want_stats"],
           "vmtl_conv3x3_small", "predict: narrow full-resolution 3x3 convs and heads, channel-wise stitching"),
    _route("csnet_layer_128x256_bs32", "val", "conv2d", lambda a: _narrow3x3(a),
           "vmtl_conv3x3_small", "val: narrow full-resolution 3x3 convs (statistics epilogue) and heads (none)"),
    _route("basic_128x256_bs32", "predict", "decoder_tail", lambda a: True,
           "vmtl_conv3x3_small", "predict: the decoder tail's narrow full-resolution conv and heads"),
    _route("basic_128x256_bs8", "predict", "decoder_tail", lambda a: True,
           "vmtl_conv3x3_small", "predict: the decoder tail at bs 8"),
    _route("basic_128x256_bs32", "val", "decoder_tail", lambda a: True,
           "vmtl_conv3x3_small", "val: the decoder tail's narrow full-resolution conv and heads"),
    _route("basic_128x256_bs32", "predict", "bn_act_conv", _mid,
           "vmtl_conv3x3_halo", "predict: 64/68-channel decoder 3x3 convs"),
    _route("basic_resnet34_128x256_bs32", "predict", "bn_act_conv", _mid,
           "vmtl_conv3x3_halo", "predict: 64/68-channel decoder 3x3 convs behind the ResNet encoder"),
    _route("mtan_256x256_bs16", "predict", "bn_act_conv", lambda a: _mid(a) and a["weight"][1][0] in (64, 68),
           "vmtl_conv3x3_halo", "predict: 64/68-channel 3x3 convs of MTAN"),
    _route("basic_128x256_bs32", "val", "bn_act_conv", _mid,
           "vmtl_conv3x3_halo", "val: 64/68-channel decoder 3x3 convs"),
    _route("basic_128x256_bs32", "predict", "bn_act_conv", lambda a: a["up2"] and a["weight"][1][0] <= 36,
           "vmtl_conv2d_up2_halo", "predict: narrow UP2 decoder convs"),
    _route("basic_128x256_bs32", "val", "bn_act_conv", lambda a: a["up2"] and a["weight"][1][0] <= 36,
           "vmtl_conv2d_up2_halo", "val: narrow UP2 decoder convs"),
    _route("mtan_256x256_bs16", "predict", "conv2d",
           lambda a: a["weight"][1][2:] == (1, 1) and a["x"][1][0] * a["x"][1][1] * a["x"][1][2] == 1 << 20,
           "vmtl_conv1x1_fwd", "predict: M = 2^20 1x1 convs on the pointwise kernel"),
    _route("basic_resnet34_128x256_bs32", "predict", "bn_add_act", lambda a: True,
           "vmtl_bn_add_act_fwd", "predict: ResNet residual closes"),
    _route("basic_resnet34_128x256_bs32", "predict", "bn_act_pool3", lambda a: True,
           "vmtl_bn_act_pool3s2_fwd", "predict: ResNet stem BatchNorm + ReLU + max-pool"),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[5] for r in ROUTES])
def test_forward_only_layers_take_the_intended_route(censuses, route):
    cfg, stage, op, pred, entry, what = route
    c = censuses[stage][cfg]
    layers = [sig for sig in c.nodes if sig[0] == op and pred(sig_args(sig))]
    assert layers, f"{cfg}: no {op} layer matches '{what}' (the census changed: revisit this list)"
    ran = lambda sig: {n for n, _ in c.node_launches(sig, phase="fwd")}
    wrong = [f"{fmt_sig(sig)} ran {sorted(ran(sig))}" for sig in layers if entry not in ran(sig)]
    assert not wrong, f"{cfg}: {what} should run on {entry}:\n" + "\n".join(wrong)


# the entry points a dense / UP2 conv plan dispatches to (fp32)
PLAN_ENTRIES = ("vmtl_conv1x1_fwd", "vmtl_conv3x3_small", "vmtl_conv3x3_halo", "vmtl_conv2d_fwd", "vmtl_conv2d_fwd_ws",
                "vmtl_conv2d_up2_halo", "vmtl_conv2d_up2_fwd", "vmtl_conv2d_up2_fwd_ws")
PLANNED = ("conv2d", "bn_act_conv", "up2_conv")


def _geometry(sig):
    """a conv node signature without what the stage changes: requires_grad, BatchNorm mode, want_stats, statistics rows"""
    out = [sig[0]]
    for k, v in sig[1]:
        if "stats" in k or "rpb" in k or k == "zero_bias_grad":
            continue
        if isinstance(v, tuple) and v and v[0] == "T":
            v = ("T", v[1])
        elif isinstance(v, tuple) and v and v[0] == "BN":
            v = ("BN", v[1])
        elif isinstance(v, tuple) and v and isinstance(v[0], tuple):  # stitch = (weights, task)
            v = tuple(x[:2] if isinstance(x, tuple) else x for x in v)
        out.append((k, v))
    return tuple(out)


def _routes_by_geometry(c):
    out = {}
    for sig in c.nodes:
        if sig[0] in PLANNED:
            ran = {n for n, _ in c.node_launches(sig, phase="fwd") if n in PLAN_ENTRIES}
            out.setdefault(_geometry(sig), (set(), sig))[0].update(ran)
    return out


def test_shapes_whose_predict_route_differs_from_the_train_route(censuses):
    """Lists every conv shape of the production configurations whose predict launch runs on another entry point than its
    training launch, and holds each to the only two rules of ops.conv_plan that look at the epilogue (read by hand): a
    narrow 3x3 launch (ceil4(Cout) <= 36, >= 2^16 rows) without an epilogue runs on vmtl_conv3x3_small also where the
    output is not whole 4 x 32 tiles; a 64/68-channel one runs on vmtl_conv3x3_halo also where the kernel has no
    statistics rows for the shape.  In both the training launch is the implicit GEMM.  Anything else is unexplained."""
    lines, unexplained = [], []
    for name in CONFIGS:
        tr, pr = _routes_by_geometry(censuses["train"][name]), _routes_by_geometry(censuses["predict"][name])
        for g in sorted(set(tr) ^ set(pr), key=repr):  # a conv only one of the two steps runs: listed, nothing to compare
            lines.append(f"{name} {fmt_sig((tr.get(g) or pr[g])[1])}: only in the {'training' if g in tr else 'predict'} step")
        for g, (ran_p, sig) in pr.items():
            if g not in tr:
                continue
            ran_t = tr[g][0]
            assert ran_p and ran_t, f"{name} {fmt_sig(sig)}: no planned conv launch ({sorted(ran_t)} / {sorted(ran_p)})"
            if ran_p == ran_t:
                continue
            line = f"{name} {fmt_sig(sig)}: train {sorted(ran_t)}, predict {sorted(ran_p)}"
            lines.append(line)
            a = sig_args(sig)
            ok = False
            if sig[0] in ("conv2d", "bn_act_conv") and not a.get("up2") and a["weight"][1][2:] == (3, 3):
                B, H, W, Cs = a["x"][1]
                ldy = ceil4(a["weight"][1][0])
                igemm = ran_t <= {"vmtl_conv2d_fwd", "vmtl_conv2d_fwd_ws"}
                if ldy <= 36 and B * H * W >= 1 << 16:
                    ok = igemm and ran_p == {"vmtl_conv3x3_small"} and (H % 4 != 0 or W % 32 != 0)
                elif Cs in (64, 68) and ldy in (64, 68) and B * H * W >= 1 << 16:
                    ok = igemm and ran_p == {"vmtl_conv3x3_halo"}
            if not ok:
                unexplained.append(line)
    if lines:
        print("shapes whose predict route differs from the train route:\n" + "\n".join("  " + l for l in lines))
    else:
        print("shapes whose predict route differs from the train route: none (every production conv shape runs on the "
              "entry point of its training launch)")
    assert not unexplained, "predict routes ops.conv_plan's epilogue rules do not explain:\n" + "\n".join(unexplained)
