"""Test-only helper (not a conftest, no GPU needed to import): a census of what one eager step of a production
configuration calls: the training step, or (stage "val" / "predict") the forward-only steps GraphedEval captures.

census(name) builds the model with build_model exactly as the other tests do, runs forward + training_step + backward on
oracle.losses.synthetic_batch, and records
  - nodes:    the unique calls of the model-facing autograd nodes of vision_mtl_amd.ops (signature -> call count).  A
              signature holds the op name and, per argument, the shape / requires_grad of tensors (plus the rows-per-block a
              statistics tensor carries), the configuration of BatchNorm modules, and every scalar.
  - launches: every kernel launch as (node signature it belongs to or None, entry point, launch key, phase).  The phase
              is 'fwd' / 'bwd' inside a node's forward / backward, None outside any node.  The key is the entry point's integer / float keyword arguments plus, for tensor arguments, only whether one was passed:
              pointers and the stream are left out.  Launches of a node's backward are attributed to it through hooks on
              its autograd node.
Launches are taken by wrapping ops._k (as tests/util.py::identity_activations does); ops._RECORD is not touched.
"""
import argparse
import contextlib
import functools
import inspect

import torch

# the BASELINE configurations: name -> (model, batch, height, width, classes, channel-wise stitching)
CONFIGS = {
    "basic_128x256_bs8": ("basic", 8, 128, 256, 19, None),
    "basic_128x256_bs32": ("basic", 32, 128, 256, 19, None),
    "basic_256x256_bs32": ("basic", 32, 256, 256, 19, None),
    "csnet_channel_128x256_bs32": ("csnet", 32, 128, 256, 19, True),
    "csnet_layer_128x256_bs32": ("csnet", 32, 128, 256, 19, False),  # the reference CLI's default
    "mtan_256x256_bs16": ("mtan", 16, 256, 256, 14, None),
    # `basic` with a torchvision ResNet-34 encoder as tools/bench_resnet.py builds it (resnet18's signatures at these shapes
    # are a subset of resnet34's: same stem, same first block of every stage, fewer identity blocks)
    "basic_resnet34_128x256_bs32": ("basic_resnet34", 32, 128, 256, 19, None),
    "basic_resnet34_128x256_bs8": ("basic_resnet34", 8, 128, 256, 19, None),
}

# model-facing autograd nodes of vision_mtl_amd.ops (the models call them as ops.X(...))
NODES = ("conv2d", "bn_act_conv", "up2_conv", "bn_act_conv1x1", "conv1x1_cat", "bn_act_dwconv", "dwconv", "bn_act",
         "bn_act_pool2", "decoder_tail", "dual_head", "squeeze_excite", "conv_transpose2x2", "stitch", "concat2", "maxpool2",
         "bilinear_up2", "spatial_mean", "channel_scale", "activation", "sigmoid", "fork", "to_nhwc", "to_nchw",
         "hwc_to_model_input", "cross_entropy", "cross_entropy_with_argmax", "silog", "l1_loss", "add_losses",
         "argmax_channels", "bn_act_pool3", "maxpool3s2", "bn_add_act")


def describe(v):
    """Hashable description of one node argument."""
    if isinstance(v, torch.Tensor):
        d = ("T", tuple(v.shape), bool(v.requires_grad))
        rpb = getattr(v, "_vmtl_rpb", None)
        return d + (("rpb", int(rpb)),) if rpb is not None else d
    if isinstance(v, torch.nn.modules.batchnorm._BatchNorm):
        return ("BN", int(v.num_features), bool(v.training), float(v.momentum), float(v.eps))
    if isinstance(v, torch.nn.Module):
        return ("M", type(v).__name__, bool(v.training))
    if isinstance(v, (tuple, list)):
        return tuple(describe(x) for x in v)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return ("?", type(v).__name__)


def launch_key(kw):
    """(sorted (name, value)) of a launch: numbers as they are, tensor arguments as 'T', absent ones as None."""
    out = []
    for k, v in sorted(kw.items()):
        if isinstance(v, torch.Tensor):
            v = "T"
        elif v is not None and not isinstance(v, (bool, int, float)):
            continue
        out.append((k, v))
    return tuple(out)


def sig_args(sig):
    """{argument name: description} of a node signature."""
    return dict(sig[1])


def fmt_sig(sig):
    def f(d):
        if isinstance(d, tuple) and d and d[0] == "T":
            s = "x".join(map(str, d[1])) + ("" if d[2] else "(nograd)")
            return s + (f"@rpb{d[3][1]}" if len(d) > 3 else "")
        if isinstance(d, tuple) and d and d[0] == "BN":
            return f"BN{d[1]}{'' if d[2] else '(eval)'}"
        if isinstance(d, tuple):
            return "(" + ",".join(f(x) for x in d) + ")"
        return repr(d)

    return sig[0] + "(" + ", ".join(f"{k}={f(v)}" for k, v in sig[1] if v is not None) + ")"


def fmt_launch(name, key):
    nums = [f"{k}={v}" for k, v in key if v is not None and v != "T" and k not in ("eps", "momentum")]
    return f"{name}[{' '.join(nums)}]"


class Recorder:
    """Context manager: wraps the model-facing nodes of ops and ops._k; .nodes / .launches as described above."""

    def __init__(self, nodes=NODES):
        self.names = nodes
        self.nodes = {}
        self.launches = []
        self._tag = None
        self._phase = None
        self._depth = 0

    def _wrap(self, ops, name, orig):
        psig = inspect.signature(orig)

        @functools.wraps(orig)
        def w(*args, **kwargs):
            if self._depth:  # a node called by another node: part of its caller
                return orig(*args, **kwargs)
            b = psig.bind(*args, **kwargs)
            b.apply_defaults()
            sig = (name, tuple((k, describe(v)) for k, v in b.arguments.items()))
            self.nodes[sig] = self.nodes.get(sig, 0) + 1
            prev, self._tag, self._phase = self._tag, sig, "fwd"
            self._depth += 1
            try:
                out = orig(*args, **kwargs)
            finally:
                self._depth -= 1
                self._tag, self._phase = prev, None
            outs = out if isinstance(out, (tuple, list)) else (out,)
            gf = next((t.grad_fn for t in outs if isinstance(t, torch.Tensor) and t.grad_fn is not None), None)
            if gf is not None:
                gf.register_prehook(lambda go, s=sig: self._set(s, "bwd"))
                gf.register_hook(lambda gi, go: self._set(None, None))
            return out

        return w

    def _set(self, tag, phase):
        self._tag, self._phase = tag, phase

    def __enter__(self):
        from vision_mtl_amd import ops

        self._ops = ops
        self._saved = {n: getattr(ops, n) for n in self.names if hasattr(ops, n)}
        for n, f in self._saved.items():
            setattr(ops, n, self._wrap(ops, n, f))
        self._orig_k = ops._k

        def _k(name, _flop=None, _xflop=None, **kw):
            self.launches.append((self._tag, name, launch_key(kw), self._phase))
            return self._orig_k(name, _flop=_flop, _xflop=_xflop, **kw)

        ops._k = _k
        return self

    def __exit__(self, *exc):
        self._ops._k = self._orig_k
        for n, f in self._saved.items():
            setattr(self._ops, n, f)
        return False


def build(kind, C, channel_wise=None, seed=11):
    """build_model's model of this kind; "basic_<encoder>": BasicMTLModel with that encoder and its default decoder"""
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(seed)
    if kind.startswith("basic_"):
        from vision_mtl_amd.models.basic_model import BasicMTLModel

        return BasicMTLModel(C, encoder_name=kind[len("basic_"):], encoder_weights=None)
    ns = argparse.Namespace(model_name=kind, backbone_weights=None)
    if channel_wise is not None:
        ns.channel_wise_stitching = channel_wise
    return build_model(ns, argparse.Namespace(num_classes=C))


class Census:
    def __init__(self, name, nodes, launches):
        self.name, self.nodes, self.launches = name, nodes, launches

    def node_launches(self, sig, phase=None):
        """(entry point, key) of the launches of one node; phase 'fwd' / 'bwd' restricts them to its forward / backward"""
        return [(n, k) for t, n, k, p in self.launches if t == sig and (phase is None or p == phase)]

    def report(self):
        lines = [f"== census {self.name}: {len(self.nodes)} unique node signatures, {len(self.launches)} launches "
                 f"({len(set((n, k) for _, n, k, _ in self.launches))} unique)"]
        for sig in self.nodes:
            seen = []
            for n, k, p in [(n, k, p) for t, n, k, p in self.launches if t == sig]:
                s = f"{p} {fmt_launch(n, k)}"
                if s not in seen:
                    seen.append(s)
            lines.append(f"  {fmt_sig(sig)} x{self.nodes[sig]}")
            lines += [f"      {s}" for s in seen]
        return "\n".join(lines)


STAGES = ("train", "val", "predict")


def census(kind, B, H, W, C=19, channel_wise=None, dev="cuda:0", name=None, stage="train"):
    """One eager step of this configuration under a Recorder -> Census.  stage "train": training_step + backward;
    "val": validation_step in train mode under no_grad (the reference validates that way: batch statistics, the running
    buffers move); "predict": predict_step in eval mode under no_grad, targets in the batch (losses and metrics run)."""
    from oracle.losses import synthetic_batch
    from vision_mtl_amd.lit_module import MTLModule

    if stage not in STAGES:
        raise ValueError(f"census: stage must be one of {STAGES}, got {stage!r}")
    model = build(kind, C, channel_wise).to(dev).train(stage != "predict")
    module = MTLModule(model, num_classes=C, device=str(dev))
    module.train(stage != "predict")
    batch = {k: v.to(dev) for k, v in synthetic_batch(B, H, W, C, seed=11).items()}
    with Recorder() as rec:
        if stage == "train":
            loss = module.training_step(batch, 0)
            loss.backward()
        else:
            with torch.no_grad():
                if stage == "val":
                    loss = module.validation_step(batch, 0)
                else:
                    module.predict_step(batch)
                    loss = module.step_outputs["predict"]["loss"][-1]
        torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    del module, model, batch, loss
    torch.cuda.empty_cache()
    return Census(name or f"{kind} {B}x{H}x{W}" + ("" if stage == "train" else f" [{stage}]"), rec.nodes, rec.launches)


@functools.lru_cache(maxsize=None)
def _production_census(name, stage):
    kind, B, H, W, C, cw = CONFIGS[name]
    return census(kind, B, H, W, C=C, channel_wise=cw, name=name if stage == "train" else f"{name} [{stage}]", stage=stage)


def production_census(name, stage="train"):
    """The census of one CONFIGS entry and stage, once per session."""
    if stage not in STAGES:
        raise ValueError(f"production_census: stage must be one of {STAGES}, got {stage!r}")
    return _production_census(name, stage)


@contextlib.contextmanager
def recording():
    with Recorder() as rec:
        yield rec
