"""Autograd bindings of the vmtl C ABI (include/vmtl.h).

Everything here is host plumbing: allocate output / workspace tensors with the torch
allocator, hand raw device pointers + the current HIP stream to libvmtl.so, register
the matching backward call with autograd.  No arithmetic happens in Python and there
is no fallback: tensors must live on a GPU and the extension must load.

Internal activation format: contiguous fp32 [B, H, W, Cs] (NHWC) with
Cs = ceil4(C) and zero padding channels; the logical channel count C travels with
the calling module.
"""
from __future__ import annotations

import contextlib
import functools
import math
import os
import struct
import weakref
from typing import NamedTuple

import torch

from ._lib import lib
from .precision import conv_prec_code, pw_prec_code

ACT_NONE, ACT_RELU, ACT_HSWISH, ACT_HSIGMOID, ACT_SIGMOID = 0, 1, 2, 3, 4
ACT_CODES = {None: 0, "none": 0, "relu": 1, "hardswish": 2, "hardsigmoid": 3, "sigmoid": 4}


def ceil4(c: int) -> int:
    return (c + 3) // 4 * 4


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the vmtl hot path only runs as HIP kernels on an MI355X "
            "(there is deliberately no CPU fallback)"
        )
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


_RECORD = None  # bench.py sets this to a list to capture the GEMM-kernel launches of one step


def _k(name, _flop=None, _xflop=None, **kw):
    if _RECORD is not None and _flop is not None:
        # _flop: algorithmic FLOPs of the reference formulation (logical channels); _xflop: FLOPs the launch
        # really executes when an algebraic rewrite makes them differ (up2_conv)
        _RECORD.append((name, dict(kw), float(_flop), float(_flop if _xflop is None else _xflop)))
    lib().callk(name, stream=_stream(), **kw)


def _kp(name, prec, _flop=None, _xflop=None, **kw):
    """A launch of an entry point that has a precision variant (include/vmtl.h VMTL_PREC_*).  fp32 (0) calls the legacy
    entry point with its legacy keywords - bench.py sorts the launches it records into families BY NAME - and only
    bf16 calls the `_p` variant.  `prec` is what the autograd node recorded in its forward: precision.conv_prec_code for the
    implicit-GEMM convolutions and the weight gradients, precision.pw_prec_code for the pointwise GEMMs (vmtl_conv1x1_*
    forward and data gradient), which only the "bf16_pw" mode moves to bf16."""
    if prec:
        _k(name + "_p", _flop, _xflop, precision=prec, **kw)
    else:
        _k(name, _flop, _xflop, **kw)


# (the launch-dropping ablation switches of round 2 - VMTL_DBG_SKIP_SIDE / VMTL_DBG_SKIP / VMTL_DBG_EXTRA - produce WRONG
# results by design and are no longer part of the product: tools/dbg_hooks.py installs them around _k on request)
_STAMPS = None  # bench.py (VMTL_STAMPS=1) sets this to a list to collect a two-stream timeline


def stamp(tag):
    """Tuning aid: device wall-clock probe on the current stream (no-op unless _STAMPS is a list)."""
    if _STAMPS is None:
        return
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib().callk("vmtl_timestamp", out=t, stream=_stream())
    _STAMPS.append((tag, t))


def _slot(p):
    """Gradient slot of a parameter inside a dp.FlatArena (None when no arena is attached).  When a
    slot exists the backward kernels write the parameter gradient straight into it and autograd is
    told there is nothing to accumulate: gradients of the whole model then form ONE contiguous buffer
    (one RCCL all-reduce, one fused Adam launch) without per-parameter add / copy kernels."""
    if p is None:
        return None
    slot = getattr(p, "_vmtl_gslot", None)
    if slot is not None:
        p._vmtl_arena._kernel_written.add(id(p))  # dp.FlatArena's guard against mixed gradient paths
    return slot


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _reduce_rows(M: int) -> int:
    return lib().raw("vmtl_reduce_rows")(M)


def _grad_buf(shape, slot, like):
    """The buffer a parameter gradient is written into: the parameter's arena slot (_slot), else a fresh tensor."""
    return _empty(shape, like) if slot is None else slot


def _grad_ret(g, slot):
    """What autograd is told about the gradient in _grad_buf's buffer: nothing when the slot took it (handing it back as
    well would put it into the arena twice)."""
    return None if slot is not None else g


# ----------------------------------------------------------------------------- weight layouts / conv geometry
class Layout(NamedTuple):
    """How a torch-layout parameter becomes a packed GEMM operand (vmtl_pack_weights, formula in csrc/pack.hip) and how the
    operand's gradient goes back (vmtl_unpack_weights, the exact inverse):
        packed[r1 * R0 + r0][t' * Cs + c] = src[r1 * sr1 + r0 * sr0 + t * st + c * sc]  (c < C, else 0),  t' = T-1-t if flip.
    A plain tuple to everything that consumes it: the pack-cache keys, the descriptor table, pack(src, *layout).
    The constructors are pure functions of a few integers that a model repeats every step, so they are memoised: on the
    eager launch path a layout is a dictionary lookup, not a tuple built per call.
    The two heads of decoder_tail / dual_head use fwd / dgrad per head, with the GROUP's row width as Cs / ldy."""
    R1: int
    R0: int
    T: int
    C: int
    Cs: int
    sr1: int
    sr0: int
    st: int
    sc: int
    flip: int

    @classmethod
    @functools.lru_cache(maxsize=None)
    def fwd(cls, Cout, Cin, KK, Cs, Cw=None):
        """Forward operand [Cout][KK][Cs] of a dense conv with a (Cout, Cin, KH, KW) weight, KK = KH * KW.  Cw: the weight
        holds Cw > Cin input channels and Cin consecutive ones are read (pack with offset = first channel * KK)."""
        return cls(1, Cout, KK, Cin, Cs, 0, (Cin if Cw is None else Cw) * KK, 1, KK, 0)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def dgrad(cls, Cout, Cin, KK, ldy, Cw=None):
        """Data-gradient operand [Cin][KK][ldy] of the same conv: transposed, taps flipped.  Cw as in fwd."""
        return cls(1, Cin, KK, Cout, ldy, 0, KK, 1, (Cin if Cw is None else Cw) * KK, 1)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def ct_fwd(cls, Cin, Cout, Cs):
        """ConvTranspose2d(k=2, s=2), (Cin, Cout, 2, 2) weight: one [Cout][Cs] block per output phase."""
        return cls(4, Cout, 1, Cin, Cs, 1, 4, 0, Cout * 4, 0)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def ct_bwd(cls, Cin, Cout, ldy):
        """Its data gradient, a 2x2 / stride-2 conv over dy: [Cin][4][ldy]."""
        return cls(1, Cin, 4, Cout, ldy, 0, Cout * 4, 1, 4, 0)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def dw(cls, C, K, Cs):
        """Depthwise (C, 1, K, K) weight as [K * K][Cs]."""
        return cls(1, 1, K * K, C, Cs, 0, 0, 1, K * K, 0)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def vec(cls, n):
        """A bias / per-channel vector of n entries, copied as it is."""
        return cls(1, 1, 1, n, n, 0, 0, 0, 1, 0)


class ConvGeom(NamedTuple):
    """One dense conv launch [B, H, W, Cs] -> [B, Ho, Wo, ldy] (storage channel widths), KH x KW taps."""
    B: int
    H: int
    W: int
    Cs: int
    Ho: int
    Wo: int
    ldy: int
    KH: int
    KW: int
    stride: int
    pad: int

    @classmethod
    def of(cls, xshape, ldy, KH, KW, stride=1, pad=0):
        B, H, W, Cs = xshape
        return cls(B, H, W, Cs, (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1, ldy, KH, KW, stride, pad)

    @property
    def M(self):
        """Rows of the GEMM: output pixels."""
        return self.B * self.Ho * self.Wo

    def dgrad(self):
        """The data gradient of this (stride-1) conv as a conv launch of its own, dy -> dx on the Layout.dgrad operand:
        extents and channel widths swapped, pad K - 1 - pad."""
        B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad = self
        assert stride == 1, "ConvGeom.dgrad: stride-1 convs only (a stride-2 conv goes through _dgrad_s2)"
        return ConvGeom(B, Ho, Wo, ldy, H, W, Cs, KH, KW, 1, KH - 1 - pad)


# ----------------------------------------------------------------------------- weight-gradient branch
class _SideBranch:
    """Second HIP stream for the parameter-gradient launches of the backward pass.

    The data-gradient chain (dgrad -> BN backward -> dgrad ...) is the critical path of the backward pass;
    the weight gradients hang off it as leaves whose results nobody needs before the optimizer /
    all-reduce.  On the MobileNetV3 encoder those launches are small (tens of workgroups), so running
    them on a second stream lets them fill CUs the critical path leaves idle.  Inside a hipGraph capture
    the fork/join events become parallel graph branches.  Only used when the gradient goes to a
    FlatArena slot (nothing is handed back to autograd, which would expect it on the main stream).
    The side stream is joined by an end-of-backward engine callback (and by FlatArena before it reads
    the gradient buffer).  VMTL_SIDE_STREAM=0 turns the branch off; VMTL_SIDE_MAX_ROWS bounds the GEMM
    rows (pixels) of a launch that may leave the main stream."""

    def __init__(self):
        self.enabled = os.environ.get("VMTL_SIDE_STREAM", "1") != "0"
        self.max_rows = int(os.environ.get("VMTL_SIDE_MAX_ROWS", str(1 << 30)))
        self.nstreams = max(1, int(os.environ.get("VMTL_SIDE_STREAMS", "1")))
        self.streams = {}
        self.pending = None  # side streams with un-joined work (dict: stream -> True)
        self.in_branch = False
        self.rr = 0
        self.task_streams = {}  # device index -> stream that runs the second task network of CSNet
        # CSNet's two task networks as two parallel graph branches.  Measured on MI355X (csnet 128x256 bs 32): 17.7 ms/step
        # on one stream with the weight gradients on the side stream, 17.7 with task streams AND the side branch (three
        # hardware queues), 15.4 with the task streams alone - so while a task-parallel model is stepping (task_mode,
        # set by its forward through packs.refresh) the weight gradients stay on their task's stream
        self.task_parallel = os.environ.get("VMTL_TASK_STREAMS", "1") != "0"
        self.task_mode = False

    def task_stream(self, device):
        """Stream for the second of two independent task networks (CSNet: the cross-stitch layers of the
        reference only scale each task's own features, so the two U-Nets never exchange data; a CSNet with the opt-in
        full stitch mixing does exchange data at every site and keeps both networks on the calling stream).  join() also
        waits for it: gradients written into arena slots from that stream have no AccumulateGrad node the
        autograd engine could synchronise on."""
        s = self.task_streams.get(device.index)
        if s is None:
            s = self.task_streams[device.index] = torch.cuda.Stream(device=device)
        return s

    def stream(self, device):
        """One side stream by default.  VMTL_SIDE_STREAMS > 1 spreads branches round-robin over several;
        measured on MI355X that LOSES (16.4 -> 18.3 ms/step with 2, 19.2 with 4): every extra hardware
        queue adds cross-queue dependency latency to the graph's critical path."""
        pool = self.streams.get(device.index)
        if pool is None:
            pool = self.streams[device.index] = [torch.cuda.Stream(device=device) for _ in range(self.nstreams)]
        self.rr = (self.rr + 1) % len(pool)
        return pool[self.rr]

    def join(self):
        pend, self.pending = self.pending, None
        if pend is not None:
            for s in pend:
                torch.cuda.current_stream(s.device).wait_stream(s)
            for s in self.task_streams.values():
                torch.cuda.current_stream(s.device).wait_stream(s)
        packs.join()

    def join_at_end_of_backward(self):
        """Called from a backward function: the stream that called backward() waits for the side / task streams
        when the engine is done (gradients written into arena slots have no AccumulateGrad node it could sync on)."""
        if self.pending is None:
            self.pending = {}
            torch.autograd.Variable._execution_engine.queue_callback(self.join)

    def mark(self):
        """Record the fork point on the current (main) stream.  Taken on entry of a backward function so the
        branch depends on what was queued BEFORE the function's own main-stream launches, while those
        launches are still issued first (inside a hipGraph capture the main-stream node then precedes the
        branch node in creation order, which keeps the critical path on one hardware queue)."""
        if not self.enabled:
            return None
        ev = torch.cuda.Event()
        ev.record()
        return ev

    @contextlib.contextmanager
    def branch(self, use, rows, mark, *tensors):
        """Run the enclosed launches on the side stream, ordered after `mark`.  `tensors` are main-stream
        tensors the launches read: the allocator must not recycle them for main-stream work until the
        side stream is past these launches."""
        if not (self.enabled and use and mark is not None and rows <= self.max_rows) or self.task_mode:
            yield
            return
        main = torch.cuda.current_stream()
        s = self.stream(main.device)
        s.wait_event(mark)
        for t in tensors:
            if t is not None:
                t.record_stream(s)
        self.join_at_end_of_backward()
        self.pending[s] = True
        with torch.cuda.stream(s):

            self.in_branch = True
            try:
                yield
            finally:
                self.in_branch = False


side = _SideBranch()


def _remember_mode(ctx):
    """Output nodes of a model (the first nodes its backward pass runs) keep the stream mode their FORWARD was built in:
    side.task_mode is process-global and another model's forward may have flipped it before this graph's backward."""
    ctx.task_mode = side.task_mode


def _restore_mode(ctx):
    side.task_mode = ctx.task_mode
    if ctx.task_mode:  # task streams were used by this graph: the calling stream joins them when the engine is done
        side.join_at_end_of_backward()


# ----------------------------------------------------------------------------- packing
class _PackCache:
    """Packed GEMM operands of the model's weights, refreshed by ONE batched launch per step.

    get() hands out a persistent packed buffer for (weight, layout).  An entry is valid while the weight's
    storage, autograd version and the global epoch are unchanged (torch optimizers bump the version;
    FlatArena.adam_step() and refresh() bump the epoch).  refresh() re-packs every known entry with a
    single vmtl_pack_weights_batch launch; a miss falls back to an individual pack and marks the
    descriptor table for a rebuild (done outside graph capture, during warm-up).

    Weights are held by WEAK reference: the entries (and their packed device buffers) of a model that has
    been dropped are purged by the next refresh() instead of being re-packed forever - a process that
    builds several models (the reference's hyperparam_tuning.py loop, a train-then-eval pair, the test
    session) neither leaks device memory nor slows down with the number of dead models."""

    def __init__(self):
        self.entries = {}  # key -> dict(dst, params, wref, ptr, version, epoch)
        self.custom = {}   # key -> dict(dst, fn, wref, ptr, version, epoch): operands with their own pack kernel
        self.shared_bufs = {}  # key -> (weakref of the anchoring weight, buffer)
        self.epoch = 0
        self.table = None  # (device uint8 tensor, n, total): entries packed on the main stream
        self.table_side = None  # the large entries, packed on the side stream
        self.live = []
        self.dirty = True
        self.custom_ready = None  # event: this step's custom operands are packed (side stream)

    def invalidate(self):
        self.epoch += 1

    @staticmethod
    def _alive(e):
        w = e["wref"]()
        if "sref" in e and e["sref"]() is None:
            return False
        return w is not None and w.data_ptr() == e["ptr"]

    def purge(self):
        """Drop the entries of weights that no longer exist (or moved, e.g. into a FlatArena)."""
        n = len(self.entries) + len(self.custom)
        self.entries = {k: e for k, e in self.entries.items() if self._alive(e)}
        self.custom = {k: e for k, e in self.custom.items() if self._alive(e)}
        self.shared_bufs = {k: e for k, e in self.shared_bufs.items() if e[0]() is not None}
        if len(self.entries) + len(self.custom) != n:
            self.dirty = True

    def get(self, weight, kind, params, offset=0, out=None, scale=None):
        """params = the operand's Layout; offset = first element of the weight to read;
        out: destination for a NEW entry (a slice of a caller-owned persistent buffer, see shared());
        scale = (tensor, first element, stride, smode): a cross-stitch factor folded into the operand
        (vmtl_pack_weights_scaled) - the entry is then also invalidated by a change of that tensor."""
        key = (id(weight), kind, params, offset)
        e = self.entries.get(key)
        if e is not None and e["wref"]() is not weight:  # id() of a dead tensor reused by a new one
            e = None
        sver = None if scale is None else (scale[0].data_ptr(), scale[0]._version, scale[1], scale[2], scale[3])
        if (e is not None and e["ptr"] == weight.data_ptr() and e["version"] == weight._version and e["epoch"] == self.epoch
                and e.get("sver") == sver):
            if e.get("side"):
                self.join()  # packed on the side stream this step: wait for its event (no-op after the first time)
            return e["dst"]
        R1, R0, T, C, Cs = params[:5]
        if (e is None or e["ptr"] != weight.data_ptr() or (out is not None and e["dst"].data_ptr() != out.data_ptr())
                or (e.get("sver") or (None,))[0] != (sver or (None,))[0]):
            e = {"dst": _empty((R1 * R0, T * Cs), weight) if out is None else out, "params": params,
                 "wref": weakref.ref(weight), "ptr": weight.data_ptr(), "offset": offset}
            if scale is not None:  # the table needs the factor's address; weak: the cache must not keep parameters alive
                e["sref"], e["scale"] = weakref.ref(scale[0]), (scale[0].data_ptr() + 4 * scale[1], scale[2], scale[3])
            self.entries[key] = e
            self.dirty = True
        src = weight.view(-1)[offset:] if offset else weight
        if scale is None:
            pack(src, *params, out=e["dst"])
        else:
            R1, R0, T, C, Cs, sr1, sr0, st, sc, flip = params
            _k("vmtl_pack_weights_scaled", src=src, dst=e["dst"], R1=R1, R0=R0, T=T, C=C, Cs=Cs, sr1=sr1, sr0=sr0, st=st,
               sc=sc, flip=flip, scale=scale[0].view(-1)[scale[1]:], sstride=scale[2], smode=scale[3])
        e["version"], e["epoch"], e["sver"] = weight._version, self.epoch, sver
        return e["dst"]

    def shared(self, anchor, kind, shape):
        """A persistent buffer several entries pack into (e.g. the two heads' weights as ONE GEMM operand); it lives as
        long as `anchor` (a weight) does."""
        key = (id(anchor), kind, tuple(shape))
        e = self.shared_bufs.get(key)
        if e is None or e[0]() is not anchor:
            e = (weakref.ref(anchor), _empty(shape, anchor))
            self.shared_bufs[key] = e
        return e[1]

    def get_custom(self, weight, kind, shape, fn, deps=()):
        """Operand built by its own kernel (fn(weight, dst) launches it): cached like get(); refresh() rebuilds
        all of them on the side stream at the start of a step, so inside the step this is a lookup (+ one
        event wait on first use).  deps: further tensors fn reads (through weak references of its own: the cache must
        not keep parameters alive) - a change of any of them invalidates the entry like a change of `weight`."""
        key = (id(weight), kind)
        e = self.custom.get(key)
        if e is not None and e["wref"]() is not weight:
            e = None
        ver = (weight._version,) + tuple((d.data_ptr(), d._version) for d in deps)
        if e is not None and e["ptr"] == weight.data_ptr() and e["version"] == ver and e["epoch"] == self.epoch:
            self.join()
            return e["dst"]
        if e is None or e["ptr"] != weight.data_ptr():
            e = {"dst": _empty(shape, weight), "wref": weakref.ref(weight), "ptr": weight.data_ptr()}
            self.custom[key] = e
        e["fn"], e["deps"] = fn, tuple(weakref.ref(d) for d in deps)
        fn(weight, e["dst"])
        e["version"], e["epoch"] = ver, self.epoch
        return e["dst"]

    def join(self):
        """Make the current stream wait for the side-stream packing of this step (no-op when already waited)."""
        ev, self.custom_ready = self.custom_ready, None
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    # entries at least this large are packed on the SIDE stream (second table): the decoder's operands are 50 of the
    # 54 MB and are not needed before the encoder has run (~1.5 ms into the step); packing them on the main stream put
    # 0.12 ms in front of the first conv
    SIDE_TABLE_MIN_ELEMS = 1 << 18

    def _build_table(self):
        import struct

        def table(live):
            if not live:
                return None
            recs, start = [], 0
            for e in live:
                R1, R0, T, C, Cs, sr1, sr0, st, sc, flip = e["params"]
                if R1 * R0 * T * Cs >= 1 << 31:
                    raise ValueError("packed operand too large for the batched pack kernel (32-bit offsets inside one operand)")
                sptr, sstride, smode = e.get("scale", (0, 0, 0))
                recs.append(struct.pack("<QQqqqqqQiiiiiiii", e["ptr"] + 4 * e.get("offset", 0), e["dst"].data_ptr(), sr1, sr0,
                                        st, sc, start, sptr, R1, R0, T, C, Cs, flip, sstride, smode))
                start += R1 * R0 * T * Cs
            size = lib().raw("vmtl_pack_desc_bytes")()
            blob = b"".join(r.ljust(size, b"\0") for r in recs)
            dev = live[0]["dst"].device
            return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), len(recs), start

        live = list(self.entries.values())
        big = lambda e: e["params"][0] * e["params"][1] * e["params"][2] * e["params"][4] >= self.SIDE_TABLE_MIN_ELEMS
        for e in live:
            e["side"] = bool(side.enabled and big(e))
        self.live = live
        self.table = table([e for e in live if not e["side"]])
        self.table_side = table([e for e in live if e["side"]])
        self.dirty = False

    def refresh(self, task_mode=False):
        """Re-pack every known weight (call once at the start of a step, before the forward).  task_mode: the model
        stepping runs its task networks on parallel streams (see _SideBranch.task_parallel)."""
        side.task_mode = bool(task_mode)
        self.join()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.purge()  # never while capturing: the captured table must keep describing the same launches
        if not self.entries and not self.custom:
            return
        self.epoch += 1
        if self.dirty:
            if capturing:
                return  # keep per-call packing inside this capture; the table is rebuilt on the next eager step
            self._build_table()
        if self.table is not None:
            table, n, total = self.table
            _k("vmtl_pack_weights_batch", descs=table, n=n, total=total)
        for e in self.live:
            w = e["wref"]()
            if w is not None:
                e["version"], e["epoch"] = w._version, self.epoch
                if "sref" in e:  # the batched launch read the stitch factor as it is now
                    sw = e["sref"]()
                    if sw is not None and e.get("sver") is not None:
                        e["sver"] = (sw.data_ptr(), sw._version) + tuple(e["sver"][2:])
        # the large operands and the ones with their own pack kernels (up2 phase / gradient matrices): none is needed
        # before the decoder, so they are built on the side stream while the encoder runs; get() / get_custom() make
        # the consuming stream wait for the event on first use
        if self.custom or self.table_side is not None:
            # task_mode: both task streams consume packed operands, and only the first get() waits for the side
            # stream's event - pack on the calling stream instead
            use_side = side.enabled and not side.task_mode
            if use_side:
                main = torch.cuda.current_stream()
                s = side.stream(main.device)
                s.wait_stream(main)
                ctx = torch.cuda.stream(s)
            else:
                ctx = contextlib.nullcontext()
            with ctx:
                if self.table_side is not None:
                    table, n, total = self.table_side
                    _k("vmtl_pack_weights_batch", descs=table, n=n, total=total)
                for e in self.custom.values():
                    w = e["wref"]()
                    if w is None:
                        continue
                    deps = [d() for d in e.get("deps", ())]
                    if any(d is None for d in deps):
                        continue
                    e["fn"](w, e["dst"])
                    e["version"] = (w._version,) + tuple((d.data_ptr(), d._version) for d in deps)
                    e["epoch"] = self.epoch
                if use_side:
                    ev = torch.cuda.Event()
                    ev.record()
                    self.custom_ready = ev


packs = _PackCache()


# ----------------------------------------------------------------------------- eval-mode BatchNorm statistics
class _EvalBNTable:
    """(mean, invstd, coef_a, coef_c) of every eval-mode BatchNorm of a model from ONE vmtl_bn_eval_stats_batch launch.

    Outside eval_bn_table() each eval-mode BatchNorm derives them from its running buffers with a launch of its own
    (vmtl_bn_eval_stats / _coef).  Inside, the launch at the head of the step fills persistent buffers (one flat
    tensor per model) and the call sites look them up by the address of the layer's running_mean: no launch.  The
    descriptor table is built and uploaded once per model and re-used while the layers' buffers and parameters stay
    where they are; it is never built inside a graph capture.  Models are held by weak reference: the tables of a
    dropped model go with it."""

    DESC = "<QQQQQQQQiifi"

    def __init__(self):
        self.tables = weakref.WeakKeyDictionary()  # model -> table (dict)
        self.active = None  # running_mean address -> (mean, invstd, coef_a, coef_c, C, eps, gamma addr, beta addr)

    @staticmethod
    def _layers(model):
        return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d) and not m.training
                and m.running_mean is not None]

    @staticmethod
    def _signature(layers):
        ptr = lambda t: 0 if t is None else t.data_ptr()
        return tuple((id(m), m.running_mean.data_ptr(), m.running_var.data_ptr(), ptr(m.weight), ptr(m.bias),
                      m.num_features, float(m.eps)) for m in layers)

    def table(self, model):
        """The descriptor table of model's eval-mode BatchNorms as they are now (None: there are none); built here when
        missing or stale."""
        import struct

        layers = self._layers(model)
        if not layers:
            return None
        sig = self._signature(layers)
        t = self.tables.get(model)
        if t is not None and t["sig"] == sig:
            return t
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("eval_bn_table: the BatchNorm table of this model must be built before the capture "
                               "(enter eval_bn_table once eagerly, e.g. in a warm-up step)")
        dev = layers[0].running_mean.device
        sizes = [ceil4(m.num_features) for m in layers]
        buf = torch.zeros(4 * sum(sizes), dtype=torch.float32, device=dev)
        recs, lookup, off = [], {}, 0
        for m, Cs in zip(layers, sizes):
            _req(m.running_mean, "running_mean"), _req(m.running_var, "running_var")
            mean, invstd, ca, cc = (buf[off + i * Cs: off + (i + 1) * Cs] for i in range(4))
            off += 4 * Cs
            g = 0 if m.weight is None else m.weight.data_ptr()
            b = 0 if m.bias is None else m.bias.data_ptr()
            recs.append(struct.pack(self.DESC, m.running_mean.data_ptr(), m.running_var.data_ptr(), g, b,
                                    mean.data_ptr(), invstd.data_ptr(), ca.data_ptr(), cc.data_ptr(), m.num_features,
                                    Cs, float(m.eps), 0))
            lookup[m.running_mean.data_ptr()] = (mean, invstd, ca, cc, m.num_features, float(m.eps), g, b)
        size = lib().raw("vmtl_bn_eval_desc_bytes")()
        blob = b"".join(r.ljust(size, b"\0") for r in recs)
        t = {"sig": sig, "descs": torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), "n": len(recs),
             "max_cs": max(sizes), "buf": buf, "lookup": lookup}
        self.tables[model] = t
        return t

    def get(self, rm, C, eps, coef=None):
        """The precomputed (mean, invstd, coef_a, coef_c) of the layer whose running_mean is `rm`, or None (no table
        in force, or it does not describe this call).  coef: the (gamma, beta) the caller's coefficients fold in."""
        if self.active is None:
            return None
        e = self.active.get(rm.data_ptr())
        if e is None or e[4] != C or e[5] != float(eps):
            return None
        if coef is not None and tuple(0 if t is None else t.data_ptr() for t in coef) != e[6:8]:
            return None
        return e[:4]


eval_bn = _EvalBNTable()


@contextlib.contextmanager
def eval_bn_table(model):
    """Eval-mode BatchNorm statistics of `model` for the enclosed step from ONE launch, issued here on the current
    stream (the eval-stats call sites then launch nothing).  Yields the table (None when no BatchNorm of the model is
    in eval mode: the step then runs exactly as without the context).  The running buffers are read at entry: enter
    it once per step."""
    t = eval_bn.table(model)
    prev = eval_bn.active
    if t is not None:
        _k("vmtl_bn_eval_stats_batch", descs=t["descs"], n=t["n"], max_cs=t["max_cs"])
        eval_bn.active = t["lookup"] if prev is None else {**prev, **t["lookup"]}
    try:
        yield t
    finally:
        eval_bn.active = prev


# ----------------------------------------------------------------------------- BatchNorm steps the nodes share
# (which node uses which, and who resolves the row block)
def stats_rpb(stats):
    """Pixels each row of conv-epilogue statistics rows covers: the `_vmtl_rpb` tag their producer put on them, else 0
    (no rows, or rows nobody tagged)."""
    return 0 if stats is None else getattr(stats, "_vmtl_rpb", 0)


def _resolve_rpb(stats, rpb, shape):
    """Pixels per row of `stats` for the wrappers that accept untagged rows (bn_act, bn_act_pool2, bn_act_pool3,
    bn_add_act): the explicit argument, else the rows' tag, else the implicit-GEMM kernel's row block for the activation
    shape (B, H, W, Cs); 0 without rows.  The pre-activation nodes (bn_act_conv, bn_act_conv1x1, bn_act_dwconv,
    decoder_tail) do not call this: they hand their rpb argument to the launch as given, and the library refuses a 0."""
    if stats is None:
        return 0
    return rpb or stats_rpb(stats) or lib().raw("vmtl_conv2d_stats_block")(*shape)


def _bn_args(bn):
    """((weight, bias, running_mean, running_var, num_batches_tracked), (training, momentum, eps)) of an nn.BatchNorm2d."""
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative moving average) is not implemented")
    return ((bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked),
            (bn.training, float(bn.momentum), bn.eps))


def _bn_stats(x, stats, rpb, rm, rv, nbt, C, training, momentum, eps, affine=None):
    """(mean, invstd) of a BatchNorm over x; with affine = (gamma, beta) also (coef_a, coef_c), BN(x) = coef_a * x + coef_c
    per channel (zeros on pad channels).  Train: batch statistics from the producing conv's partial rows `stats` (rpb
    pixels each, as the caller resolved them) or from a sweep of x, the running buffers moved as torch moves them.
    Eval: the running statistics, from the eval_bn_table in force (no launch) or one launch."""
    B, H, W, Cs = x.shape
    if not training:
        e = eval_bn.get(rm, C, eps, affine)
        if e is not None:
            return e[:2] if affine is None else e
    mean, invstd = _empty((Cs,), x), _empty((Cs,), x)
    if affine is None:
        out, kw = (mean, invstd), {}
    else:
        ca, cc = _empty((Cs,), x), _empty((Cs,), x)
        out, kw = (mean, invstd, ca, cc), {"gamma": affine[0], "beta": affine[1], "coef_a": ca, "coef_c": cc}
    if training:
        M = B * H * W
        if stats is not None:
            partial, nblk = stats, stats.shape[0]
        else:
            partial, nblk, rpb = _empty((_reduce_rows(M), 2, Cs), x), 0, 0
        _k("vmtl_bn_stats" if affine is None else "vmtl_bn_stats_coef", x=x, M=M, C=C, Cs=Cs, partial=partial,
           nblk_from_conv=nblk, rows_per_blk_from_conv=rpb, eps=eps, momentum=momentum, running_mean=rm, running_var=rv,
           num_batches_tracked=nbt, save_mean=mean, save_invstd=invstd, **kw)
    else:
        _k("vmtl_bn_eval_stats" if affine is None else "vmtl_bn_eval_stats_coef", running_mean=rm, running_var=rv, C=C,
           Cs=Cs, eps=eps, save_mean=mean, save_invstd=invstd, **kw)
    return out


def _bn_apply(x, stats, rpb, gamma, beta, rm, rv, nbt, C, training, momentum, eps, act, mul=None, res=None):
    """(y, mean, invstd) with y = act(BN(x)) [* mul] [+ res], materialised.  Few statistics rows: every thread of the apply
    launch merges them itself (vmtl_bn_apply_fused), no separate finalize launch."""
    B, H, W, Cs = x.shape
    M = B * H * W
    y = _empty(x.shape, x)
    if training and stats is not None and stats.shape[0] <= _BN_FUSE_ROWS:
        mean, invstd = _empty((Cs,), x), _empty((Cs,), x)
        _k("vmtl_bn_apply_fused", x=x, partial=stats, nblk=stats.shape[0], rows_per_blk=rpb, eps=eps, momentum=momentum,
           running_mean=rm, running_var=rv, num_batches_tracked=nbt, save_mean=mean, save_invstd=invstd, gamma=gamma,
           beta=beta, mul=mul, res=res, y=y, M=M, C=C, Cs=Cs, act=act)
    else:
        mean, invstd = _bn_stats(x, stats, rpb, rm, rv, nbt, C, training, momentum, eps)
        _k("vmtl_bn_apply", x=x, mean=mean, invstd=invstd, gamma=gamma, beta=beta, mul=mul, res=res, y=y, M=M, C=C, Cs=Cs,
           act=act)
    return y, mean, invstd


def _bn_bwd_tail(part, rows, x, dz, mean, invstd, gamma, C, training, slots, want_dx):
    """(dx, dgamma, dbeta) of a BatchNorm whose backward reduction came out of the producing data gradient's epilogue:
    dz and its `rows` partial rows `part`.  Finalize the column sums, then (want_dx) the backward-apply sweep.
    slots = the arena slots of (gamma, beta): a gradient a slot took is handed back as None."""
    B, H, W, Cs = x.shape
    M, tr = B * H * W, 1 if training else 0
    dgamma, dbeta = _grad_buf((C,), slots[0], x), _grad_buf((C,), slots[1], x)
    _k("vmtl_bn_bwd_finalize", partial=part, nblk=rows, M=M, C=C, Cs=Cs, sum_dz=dbeta, sum_dzx=dgamma, mean=None,
       invstd=None, gamma=None, training=tr, coef_a=None, coef_b=None, coef_c=None)
    dx = None
    if want_dx:
        dx = _empty(x.shape, x)
        _k("vmtl_bn_bwd_apply", x=x, dz=dz, mean=mean, invstd=invstd, gamma=gamma, sum_dz=dbeta, sum_dzx=dgamma, dx=dx, M=M,
           C=C, Cs=Cs, training=tr)
    return dx, _grad_ret(dgamma, slots[0]), _grad_ret(dbeta, slots[1])


def _bn_bwd(x, dy, mean, invstd, gamma, beta, C, training, act, slots, mul=None, want_dmul=False):
    """(dx, dgamma, dbeta, dmul) of y = act(BN(x)) [* mul] from dy in one launch (reduce + apply); gamma None: of the plain
    activation.  slots as in _bn_bwd_tail; the kernels write exactly C entries of each sum."""
    B, H, W, Cs = x.shape
    M = B * H * W
    dmul = _empty(x.shape, x) if want_dmul else None
    partial = dgamma = dbeta = None
    if gamma is not None or dmul is not None:
        partial = _empty((_reduce_rows(M), 2, Cs), x)
    if gamma is not None:
        dgamma, dbeta = _grad_buf((C,), slots[0], x), _grad_buf((C,), slots[1], x)
    dx = _empty(x.shape, x)
    _k("vmtl_bn_bwd", x=x, dy=dy, mean=mean, invstd=invstd, gamma=gamma, beta=beta, mul=mul, dmul=dmul, partial=partial,
       sum_dz=dbeta, sum_dzx=dgamma, dx=dx, M=M, C=C, Cs=Cs, act=act, training=1 if training else 0)
    return dx, _grad_ret(dgamma, slots[0]), _grad_ret(dbeta, slots[1]), dmul


def _ez_kw(ez):
    """Keywords of a data-gradient launch whose epilogue runs act' and the BatchNorm-backward reduction of the conv's own
    input: ez = (x, mean, invstd, gamma, beta, act) of that BatchNorm, None for a launch without the epilogue."""
    x, mean, invstd, gamma, beta, act = ez or (None, None, None, None, None, ACT_NONE)
    return dict(ez_x=x, ez_mean=mean, ez_invstd=invstd, ez_gamma=gamma, ez_beta=beta, ez_act=act)


def pack(src, R1, R0, T, C, Cs, sr1, sr0, st, sc, flip=0, out=None):
    dst = _empty((R1 * R0, T * Cs), src) if out is None else out
    _k("vmtl_pack_weights", src=src, dst=dst, R1=R1, R0=R0, T=T, C=C, Cs=Cs, sr1=sr1, sr0=sr0, st=st, sc=sc, flip=flip)
    return dst


def unpack(packed, layout, out, nslabs=1, slab_stride=0):
    """Sum the nslabs weight-gradient slabs of an operand into `out` in the torch layout; `layout` is the Layout the
    operand of that GEMM was (or would be) packed with - the unpack is its inverse."""
    R1, R0, T, C, Cs, sr1, sr0, st, sc, flip = layout
    _k("vmtl_unpack_weights", packed=packed, grad=out, R1=R1, R0=R0, T=T, C=C, Cs=Cs, sr1=sr1, sr0=sr0, st=st,
       sc=sc, flip=flip, nslabs=nslabs, slab_stride=slab_stride)
    return out


def _wgrad(x, dy, g, *, Nw, flop, xflop=None, prec=0):
    """Weight-gradient slabs [splits][Nw][KH*KW*Cs] of the conv g (summed later by unpack).  prec applies to the dense
    kernel only (the narrow halo-tile kernel stays fp32)."""
    B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad = g
    if (KH == 3 and KW == 3 and stride == 1 and pad == 1 and B * H * W * max(Cs, ldy) * 4 < 1 << 32
            and lib().raw("vmtl_conv3x3_wgrad_small_supported_p")(Cs, ldy, W, B * H * W, prec)):
        # narrow full-resolution layers: the strip-walking halo kernel reads x once instead of once per tap (fp32 in every
        # mode; the query keeps a launch on the dense kernel where this one was not measured against it: bf16, small maps)
        ns = lib().raw("vmtl_conv3x3_wgrad_small_slabs_for")(B, H, W, Cs, ldy, Nw)
        slabs = _empty((ns, Nw, 9 * Cs), x)
        _k("vmtl_conv3x3_wgrad_small", _flop=flop, _xflop=xflop, x=x, dy=dy, slabs=slabs, nslabs=ns, B=B, H=H, W=W, Cs=Cs, ldy=ldy,
           Nw=Nw)
        return slabs, ns
    splits = lib().raw("vmtl_conv2d_wgrad_splits")(B * Ho * Wo, Nw, KH * KW * Cs)
    slabs = _empty((splits, Nw, KH * KW * Cs), x)
    _kp("vmtl_conv2d_wgrad", prec, _flop=flop, _xflop=xflop, x=x, dy=dy, slabs=slabs, splits=splits, B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo,
       ldy=ldy, Nw=Nw, KH=KH, KW=KW, stride=stride, pad=pad)
    return slabs, splits


def _colsum(a, b, M, C, Cs, mode=0, reduce_all=0, out=None):
    partial = _empty((_reduce_rows(M) + 1, Cs), a)  # + 1: scratch row of the reduce_all form
    if out is None:
        out = _empty((1 if reduce_all else C,), a)
    _k("vmtl_colsum", a=a, b=b, M=M, C=C, Cs=Cs, mode=mode, reduce_all=reduce_all, partial=partial, out=out)
    return out


def _wgrad_into(x, dy, g, layout, dw, flop, prec=0):
    """Weight gradient of the dense conv g into dw (torch layout): `layout` is the weight's FORWARD Layout in that conv."""
    slabs, ns = _wgrad(x, dy, g, Nw=layout.R1 * layout.R0, flop=flop, prec=prec)
    unpack(slabs, layout, dw, nslabs=ns)


def _wgrad_two_heads(x, dy, g, lay_a, lay_b, wa, wb, slots, flop, prec):
    """Parameter gradients of two heads run as ONE conv g of N = Ca + Cb output channels: one weight-gradient launch whose
    slabs are unpacked per head (lay_a / lay_b: each head's forward Layout), one column sum of dy split into the two biases.
    slots = the arena slots of (weight a, bias a, weight b, bias b); returns what autograd is told, in that order."""
    swa, sba, swb, sbb = slots
    Ca, Cb, row = lay_a.R0, lay_b.R0, lay_a.T * lay_a.Cs
    N = Ca + Cb
    slabs, ns = _wgrad(x, dy, g, Nw=N, flop=flop, prec=prec)
    dwa, dwb = _grad_buf(wa.shape, swa, x), _grad_buf(wb.shape, swb, x)
    unpack(slabs, lay_a, dwa, nslabs=ns, slab_stride=N * row)
    unpack(slabs.view(-1)[Ca * row:], lay_b, dwb, nslabs=ns, slab_stride=N * row)
    db = _colsum(dy, None, g.M, N, g.ldy)
    dba, dbb = _grad_buf((Ca,), sba, x), _grad_buf((Cb,), sbb, x)
    _copy_vec(db, dba, Ca)
    _copy_vec(db[Ca:], dbb, Cb)
    return _grad_ret(dwa, swa), _grad_ret(dba, sba), _grad_ret(dwb, swb), _grad_ret(dbb, sbb)


def _bias_grad(bias, slot, dy, M, Cout, ldy, zero, fork):
    """dL/dbias of a conv (column sums of dy), into its arena slot when there is one (returns None then).
    zero: the conv feeds a TRAIN-mode BatchNorm - the batch mean absorbs the bias, its gradient is exactly 0.  This
    function is the slot's only writer, so the zero is written ONCE (first backward pass) and remembered
    (FlatArena._zero_bias): eager steps launch nothing afterwards (MTAN: 56 memset launches per step before).  Column
    sums written later (an eval-mode BatchNorm step) or FlatArena.slots_clobbered() forget it.
    Inside a hipGraph CAPTURE the (4..2048-byte) memset is still recorded, on the side branch: measured on MI355X /
    ROCm 7.0 runtime (MTAN 256x256 bs 16, round 3), the replayed graph runs its side branch CONCURRENTLY with the main
    chain only when these memset nodes are part of it - 52.3 ms/step with them, 55.7-57.8 without (side branch started
    after the last main-chain kernel: two-stream timeline of VMTL_STAMPS=1); one memset per step, one per branch entry
    and DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 did not reproduce it.  They are off the critical path (side branch, ~2 us)."""
    arena = getattr(bias, "_vmtl_arena", None) if slot is not None else None
    if zero:
        if slot is None:
            db = _empty((Cout,), dy)
            _k("vmtl_fill_zero", p=db, n=Cout)
            return db
        capturing = torch.cuda.is_current_stream_capturing()
        if arena is None or id(bias) not in arena._zero_bias or (capturing and side.enabled and not side.task_mode):
            with side.branch(True, M, fork, dy):
                _k("vmtl_fill_zero", p=slot, n=Cout)
            if arena is not None and not capturing:
                arena._zero_bias.add(id(bias))
        return None
    with side.branch(slot is not None, M, fork, dy):
        db = _colsum(dy, None, M, Cout, ldy, out=slot)
    if slot is not None:
        if arena is not None:
            arena._zero_bias.discard(id(bias))
        return None
    return db


FUSE_DW = os.environ.get("VMTL_FUSE_DW", "1") != "0"  # encoder: bn1 + act + depthwise conv as one node (vmtl_dwconv_bn_fwd)
_PW = os.environ.get("VMTL_PW", "1") != "0"  # pointwise GEMM kernel for 1x1 convs (csrc/conv_pw.hip)
_PW_MAX_ROWS = int(os.environ.get("VMTL_PW_MAX_ROWS", str(1 << 21)))  # measured on MTAN (M = 2^20): 57.1 -> 55.5 ms/step
_SMALL_MIN_ROWS = int(os.environ.get("VMTL_SMALL_MIN_ROWS", str(1 << 16)))  # plain narrow 3x3 launches on the halo-tile kernel
_SMALL_STATS = os.environ.get("VMTL_SMALL_STATS", "1") != "0"  # statistics-epilogue launches of narrow layers there too
_MID_HALO = os.environ.get("VMTL_MID_HALO", "1") != "0"  # halo-tile kernel for the 64/68-channel 3x3 convs (csrc/conv3x3_halo.hip)
_MID_HALO_MIN_ROWS = int(os.environ.get("VMTL_MID_HALO_MIN_ROWS", str(1 << 16)))
_UP2_HALO = os.environ.get("VMTL_UP2_HALO", "1") != "0"  # halo-tile kernel for the narrow UP2 convs (csrc/conv_up2_halo.hip)


class ConvPlan(NamedTuple):
    """How one dense or UP2 conv launch runs: decided once (conv_plan / up2_plan), then only dispatched on.
    route: "pw" pointwise GEMM (csrc/conv_pw.hip), "small" narrow halo tile (vmtl_conv3x3_small), "mid_halo" 64/68-channel
    halo tile (vmtl_conv3x3_halo), "up2_halo" (vmtl_conv2d_up2_halo), "ksplit" implicit GEMM in K slices, "igemm" implicit
    GEMM.  ksplit: the K slices the implicit GEMM takes for this shape (1 = none; pointwise and shuffle launches count as 1).
    stats_rows: partial rows the epilogue writes (0 = no epilogue), rpb: the pixels each row covers (0 without rows)."""
    route: str
    ksplit: int
    stats_rows: int
    rpb: int


def conv_plan(B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad, shuffle=0, prec=0, epilogue=None) -> ConvPlan:
    """The plan of a dense conv launch [B, H, W, Cs] -> [B, Ho, Wo, ldy] under precision `prec`.  epilogue: None, "stats"
    (BatchNorm partial rows of y) or "bnbwd" (the fused activation + BatchNorm backward of a data gradient, ep_mode 2).
    A launch that splits K drops its epilogue (the BatchNorm sweeps the small output itself / runs its own backward reduce);
    only then is the route chosen, in this order: pointwise, narrow halo tile (not gated on precision: tools/bench_small.py),
    64/68-channel halo tile (fp32 only: tools/bench_halo3.py), split K, implicit GEMM.  A halo tile with an epilogue needs
    whole 4 x 32 tiles.  The switches are read here on every call (tests patch them), so a plan is never cached."""
    raw = lib().raw
    M = B * Ho * Wo
    pw = _PW and KH == 1 and KW == 1 and stride == 1 and pad == 0 and not shuffle and M <= _PW_MAX_ROWS
    ks = 1 if shuffle or pw else raw("vmtl_conv2d_ksplit")(B, Ho, Wo, ldy, KH * KW * Cs)
    if ks > 1 or (epilogue == "bnbwd" and os.environ.get("VMTL_BNBWD_FUSE", "1") == "0"):
        epilogue = None
    tap3 = KH == 3 and KW == 3 and stride == 1 and pad == 1 and not shuffle
    if pw:
        route = "pw"
    elif (tap3 and ldy <= 36 and M >= _SMALL_MIN_ROWS and M * 36 <= 0x7FFFFFFF  # 32-bit element offsets
          and conv3x3_small_supported(Cs, ldy) and (not epilogue or (_SMALL_STATS and Ho % 4 == 0 and Wo % 32 == 0))):
        route = "small"
    elif (_MID_HALO and prec == 0 and tap3 and M >= _MID_HALO_MIN_ROWS and ks == 1
          and raw("vmtl_conv3x3_halo_supported")(B, Ho, Wo, Cs, ldy, ldy)
          and (not epilogue or raw("vmtl_conv3x3_halo_stat_rows")(B, Ho, Wo) > 0)):
        route = "mid_halo"
    else:
        route = "ksplit" if ks > 1 else "igemm"
    if not epilogue:
        return ConvPlan(route, ks, 0, 0)
    if route == "small":
        rows, rpb = raw("vmtl_conv3x3_small_stat_rows")(B, Ho, Wo), raw("vmtl_conv3x3_small_stat_block")(B, Ho, Wo)
    elif route == "mid_halo":
        rows, rpb = raw("vmtl_conv3x3_halo_stat_rows")(B, Ho, Wo), raw("vmtl_conv3x3_halo_stat_block")(B, Ho, Wo)
    elif route == "pw":
        rows, rpb = raw("vmtl_conv1x1_stats_rows")(M, ldy, Cs, 0), raw("vmtl_conv1x1_stats_block")(M, ldy, Cs, 0)
    else:
        rows, rpb = raw("vmtl_conv2d_stats_rows")(B, Ho, Wo, ldy), raw("vmtl_conv2d_stats_block")(B, Ho, Wo, ldy)
    return ConvPlan(route, ks, rows, rpb)


def up2_plan(B, H2, W2, C0s, C1s, ldy, Cout, prec, want_stats) -> ConvPlan:
    """The plan of an UP2 conv (low-res source [B, H2, W2, C0s], skip of C1s storage channels): the halo-tile kernel when
    fp32, supported and not split (the tile-starved small-batch launches keep their split-K form; bf16 stays on the
    implicit GEMM), else split K, else the implicit GEMM.  The two kernels tile differently, so the
    statistics rows follow the route; the implicit GEMM has them only when its row block divides B * H2 * W2."""
    raw = lib().raw
    ks = raw("vmtl_conv2d_up2_ksplit")(B, H2, W2, ldy, 4 * C0s + 9 * C1s)
    rows = rpb = 0
    if _UP2_HALO and prec == 0 and ks == 1 and raw("vmtl_conv2d_up2_halo_supported")(B, H2, W2, C0s, C1s, ldy, Cout):
        route = "up2_halo"
        if want_stats:
            rows = raw("vmtl_conv2d_up2_halo_stat_rows")(B, H2, W2, C0s, C1s, ldy, Cout)
            rpb = raw("vmtl_conv2d_up2_halo_stat_block")(C0s, C1s, ldy, Cout) if rows else 0
    elif ks > 1:
        route = "ksplit"
    else:
        route = "igemm"
        if want_stats:
            bm, Mq = raw("vmtl_conv2d_up2_stats_block")(B, H2, W2, ldy), B * H2 * W2
            if Mq % bm == 0:
                rows, rpb = 4 * (Mq // bm), bm
    return ConvPlan(route, ks, rows, rpb)


def _mid_halo(x, wp, y, B, H, W, Cs, ldy, Nw, Cout, flop, pa=None, pc=None, act_in=ACT_NONE, a_out=None, bias=None,
              stats=None, ep_mode=0, ez=None):
    """One vmtl_conv3x3_halo launch; ez = (x, mean, invstd, gamma, beta, act) for ep_mode 2."""
    _k("vmtl_conv3x3_halo", _flop=flop, x=x, pa=pa, pc=pc, act_in=act_in, a_out=a_out, wp=wp, bias=bias, y=y, stats=stats,
       ep_mode=ep_mode, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Cout, **_ez_kw(ez))


def _halo_launch(route, x, wp, y, g, Nw, Cout, flop, **kw):
    """The conv g (3x3 / stride 1 / pad 1) on the halo-tile kernel of its plan's route: "small" narrow full-resolution
    layers, "mid_halo" 64/68-channel layers; both read each input pixel once."""
    (_small if route == "small" else _mid_halo)(x, wp, y, g.B, g.H, g.W, g.Cs, g.ldy, Nw, Cout, flop, **kw)


def _conv_launch(x, wp, bias, y, g, *, Cout, Nw=None, shuffle=0, cin=None, algo_flop=None, prec=0, plan=None, stats=None,
                 pw_prec=0):
    """One dense conv launch of geometry g, dispatched on its plan; a launch without an epilogue may leave the planning to
    this function.  Cout: logical output channels, Nw: rows of the operand wp (Cout unless given).
    stats: the [plan.stats_rows][2][ldy] rows of a plan with the statistics epilogue.  prec: the implicit GEMM's precision,
    pw_prec: the pointwise GEMM's (the plan itself does not depend on pw_prec)."""
    B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad = g
    if Nw is None:
        Nw = Cout
    if plan is None:
        plan = conv_plan(B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad, shuffle, prec)
    xflop = 2.0 * B * Ho * Wo * Nw * KH * KW * (Cs if cin is None else cin)
    flop = xflop if algo_flop is None else algo_flop
    if plan.route == "pw":
        _kp("vmtl_conv1x1_fwd", pw_prec, _flop=flop, _xflop=xflop, x=x, wp=wp, bias=bias, y=y, stats=stats, M=B * Ho * Wo,
            Ks=Cs, ldy=ldy, Nw=Nw, Cout=Cout)
    elif plan.route in ("small", "mid_halo"):
        _halo_launch(plan.route, x, wp, y, g, Nw, Cout, flop, bias=bias, stats=stats, ep_mode=1 if stats is not None else 0)
    elif plan.route == "ksplit":  # tile-starved contraction: split K when the tile grid alone cannot fill the chip
        _kp("vmtl_conv2d_fwd_ws", prec, _flop=flop, _xflop=xflop, x=x, wp=wp, bias=bias, y=y,
            ws=_empty((plan.ksplit, B * Ho * Wo, ldy), x), B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo, ldy=ldy, Nw=Nw, Cout=Cout,
            KH=KH, KW=KW, stride=stride, pad=pad)
    else:
        _kp("vmtl_conv2d_fwd", prec, _flop=flop, _xflop=xflop, x=x, wp=wp, bias=bias, y=y, stats=stats, B=B, H=H, W=W,
            Cs=Cs, Ho=Ho, Wo=Wo, ldy=ldy, Nw=Nw, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, act=0, shuffle=shuffle)


def _up2_fwd(plan, xl, skip, weight, C0, prec):
    """(y, stats) of an UP2 conv on its plan: conv3x3(cat[nearest_x2(xl), skip]) as four 2x2 phase convolutions on xl.
    FLOPs: the reference formulation (9 taps on every channel); executed: 4 taps on xl's."""
    B, H2, W2, C0s = xl.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    C1, C1s = Cin - C0, 0 if skip is None else skip.shape[3]
    ldy = ceil4(Cout)
    wp = packs.get_custom(weight, "up2_fwd", (4, Cout, 4 * C0s + 9 * C1s), lambda w, dst: _k(
        "vmtl_pack_up2_fwd", w=w, dst=dst, Cout=Cout, C0=C0, C0s=C0s, C1=C1, C1s=C1s))
    y = _empty((B, 2 * H2, 2 * W2, ldy), xl)
    stats = _empty((plan.stats_rows, 2, ldy), xl) if plan.stats_rows else None
    M = B * 4 * H2 * W2
    kw = dict(_flop=2.0 * M * Cout * 9 * Cin, _xflop=2.0 * M * Cout * (4 * C0 + 9 * C1), xl=xl, skip=skip, wp_eff=wp, y=y,
              B=B, H2=H2, W2=W2, C0s=C0s, C1s=C1s, ldy=ldy, Cout=Cout)
    if plan.route == "up2_halo":
        _k("vmtl_conv2d_up2_halo", stats=stats, **kw)
    elif plan.route == "ksplit":  # tile-starved (deep decoder blocks at small batch): split K, no statistics epilogue
        _kp("vmtl_conv2d_up2_fwd_ws", prec, ws=_empty((plan.ksplit, B, 2 * H2, 2 * W2, ldy), xl), **kw)
    else:
        _kp("vmtl_conv2d_up2_fwd", prec, stats=stats, **kw)
    return y, stats


def _up2_dskip(dy, weight, skip, C0, prec):
    """Data gradient of an UP2 conv's skip source: the plain 3x3 data gradient restricted to the skip channels."""
    B, H, W, ldy = dy.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    C1, C1s = Cin - C0, skip.shape[3]
    wds = packs.get(weight, "up2_dskip", Layout.dgrad(Cout, C1, 9, ldy, Cw=Cin), offset=C0 * 9)
    dskip = _empty((B, H, W, C1s), dy)
    _conv_launch(dy, wds, None, dskip, ConvGeom(B, H, W, ldy, H, W, C1s, 3, 3, 1, 1), Cout=C1, cin=Cout, prec=prec)
    return dskip


def _up2_wgrad(dy, xl, skip, weight, C0, dw, prec):
    """Weight gradient of an UP2 conv into dw: the low-res part as the weight gradient of the 4x4/s2/p1 convolution of
    the data gradient (dY in the role of its input), the skip part as a plain 3x3 one."""
    B, H, W, ldy = dy.shape
    _, H2, W2, C0s = xl.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    slabs, ns = _wgrad(dy, xl, ConvGeom(B, H, W, ldy, H2, W2, C0s, 4, 4, 2, 1), Nw=C0, flop=2.0 * B * H * W * Cout * 9 * C0,
                       xflop=2.0 * B * H2 * W2 * C0 * 16 * Cout, prec=prec)
    _k("vmtl_unpack_up2", slabs=slabs, grad=dw, Cout=Cout, Cos=ldy, C0=C0, Cin=Cin, nslabs=ns)
    if skip is not None:
        C1, C1s = Cin - C0, skip.shape[3]
        _wgrad_into(skip, dy, ConvGeom(B, H, W, C1s, H, W, ldy, 3, 3, 1, 1), Layout.fwd(Cout, C1, 9, C1s, Cw=Cin),
                    dw.view(-1)[C0 * 9:], 2.0 * B * H * W * Cout * 9 * C1, prec)


# ----------------------------------------------------------------------------- conv2d
def _stitch_view(stitch_w, task, C):
    """(first element, stride) of the diagonal w[task, task, (c)] inside the flattened CrossStitchLayer parameter
    (reference models/cross_stitch_model.py:21-37: (T, T, C) channel-wise or (T, T) layer-wise)."""
    T = stitch_w.shape[0]
    if stitch_w.dim() == 3:
        if stitch_w.shape[2] != C:
            raise ValueError(f"stitched conv: the stitch layer has {stitch_w.shape[2]} channels, the conv reads {C}")
        return (task * T + task) * C, 1
    return task * T + task, 0


class _Conv2d(torch.autograd.Function):
    """y = conv2d(x, weight) (+ bias); weight stays in torch (Cout, Cin, KH, KW) layout.
    stitch_w (optional): the CrossStitchLayer parameter whose diagonal entry of `stitch_task` scales x first
    (y = conv(w[a,a,(c)] * x): reference models/cross_stitch_model.py:32-37 + the conv that follows every stitch site in
    the CSNet walk :108-142).  The scale is FOLDED into the packed operands (forward and data gradient) and its weight
    gradient is taken from the conv's own weight-gradient slabs: no pass over the activations for the stitch at all."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, plan, zero_bias_grad=False, stitch_w=None, stitch_task=0):
        x = _req(x, "x")
        weight = _req(weight, "weight")
        B, H, W, Cs = x.shape
        Cout, Cin, KH, KW = weight.shape
        if ceil4(Cin) != Cs:
            raise ValueError(f"conv2d: input has {Cs} storage channels, weight expects Cin={Cin}")
        ldy = ceil4(Cout)
        g = ConvGeom.of(x.shape, ldy, KH, KW, stride, pad)
        if stitch_w is None:
            wp = packs.get(weight, "fwd", Layout.fwd(Cout, Cin, KH * KW, Cs))
        else:
            stitch_w = _req(stitch_w, "stitch weights")
            soff, sstride = _stitch_view(stitch_w, stitch_task, Cin)
            wp = packs.get(weight, f"fwd_st{stitch_task}", Layout.fwd(Cout, Cin, KH * KW, Cs),
                           scale=(stitch_w, soff, sstride, 1))
        y = _empty((B, g.Ho, g.Wo, ldy), x)
        stats = _empty((plan.stats_rows, 2, ldy), x) if plan.stats_rows else None
        prec = ctx.prec = conv_prec_code()  # backward runs under the precision of this forward
        pw_prec = ctx.pw_prec = pw_prec_code()  # (a 1x1 conv on the pointwise route: forward and data gradient)
        _conv_launch(x, wp, bias, y, g, Cout=Cout, cin=Cin, prec=prec, plan=plan, stats=stats, pw_prec=pw_prec)
        ctx.save_for_backward(x, weight, stitch_w)
        ctx.cfg = (stride, pad, bias is not None)
        ctx.zero_bias_grad = bool(zero_bias_grad)
        ctx.slots = (_slot(weight), _slot(bias))
        ctx.stitch = (stitch_task, _slot(stitch_w))
        ctx.bias = bias
        ctx.set_materialize_grads(False)  # no zero-filled "gradient" tensor for the stats output
        if stats is not None:
            ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, weight, stitch_w = ctx.saved_tensors
        stride, pad, has_bias = ctx.cfg
        stitch_task, stitch_slot = ctx.stitch
        if dy is None:
            return (None,) * 9
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        Cout, Cin, KH, KW = weight.shape
        KK = KH * KW
        _, Ho, Wo, ldy = dy.shape
        g = ConvGeom(B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad)
        dx = dw = db = dst_w = None
        if stitch_w is not None:
            soff, sstride = _stitch_view(stitch_w, stitch_task, Cin)
        stamp(f"main conv M={B * Ho * Wo} N={Cout} K={KK * Cin}")
        fork = side.mark()  # parameter gradients branch off here, before the data gradient
        if ctx.needs_input_grad[0]:
            if stride != 1:
                # phase-decomposed data gradient (csrc/resnet.hip): stride 2, square kernels, the pads a ResNet uses
                if stitch_w is not None or stride != 2 or KH != KW or not lib().raw("vmtl_conv2d_dgrad_s2_supported")(KH, pad):
                    raise NotImplementedError(f"data gradient of a stride-{stride} {KH}x{KW} / pad {pad} dense conv"
                                              + (" with a stitch scale" if stitch_w is not None else ""))
                dx = _dgrad_s2(dy, weight, g, ctx.prec)
            elif stitch_w is None:
                wd = packs.get(weight, "dgrad", Layout.dgrad(Cout, Cin, KK, ldy))
            else:  # rows of the data-gradient operand are the input channels: d(x) = s * d(s * x)
                wd = packs.get(weight, f"dgrad_st{stitch_task}", Layout.dgrad(Cout, Cin, KK, ldy),
                               scale=(stitch_w, soff, sstride, 2))
            if stride == 1:
                dx = _empty((B, H, W, Cs), x)
                _conv_launch(dy, wd, None, dx, g.dgrad(), Cout=Cin, cin=Cout, prec=ctx.prec, pw_prec=ctx.pw_prec)
        if ctx.needs_input_grad[1] or (stitch_w is not None and ctx.needs_input_grad[7]):
            use_side = ctx.slots[0] is not None and (stitch_w is None or stitch_slot is not None)
            with side.branch(use_side, B * Ho * Wo, fork, x, dy):
                dw = _grad_buf(weight.shape, ctx.slots[0], x)
                flop = 2.0 * B * Ho * Wo * Cout * KK * Cin
                if stitch_w is None:
                    _wgrad_into(x, dy, g, Layout.fwd(Cout, Cin, KK, Cs), dw, flop, ctx.prec)
                else:
                    # the slabs hold dL/d(W*s): dW = slabs * s, and the stitch weight's gradient is their contraction
                    # with W (one small launch pair on the weight-sized tensor; off-diagonal entries stay zero)
                    slabs, ns = _wgrad(x, dy, g, Nw=Cout, flop=flop, prec=ctx.prec)
                    n = Cin if sstride else 1
                    if stitch_slot is not None:
                        ds = stitch_slot.view(-1)[soff:soff + n]
                    else:
                        dst_w = torch.zeros_like(stitch_w)
                        ds = dst_w.view(-1)[soff:soff + n]
                    _k("vmtl_unpack_weights_stitch", packed=slabs, grad=dw, w=weight, scale=stitch_w.view(-1)[soff:],
                       sstride=sstride, ds=ds, work=_empty((Cout * Cin * KK + Cin,), x), R0=Cout, T=KK, C=Cin, Cs=Cs,
                       nslabs=ns, slab_stride=0, reduce_all=0 if sstride else 1)
                stamp(f"side conv M={B * Ho * Wo} N={Cout} K={KK * Cin}")
            dw = _grad_ret(dw, ctx.slots[0])
        if has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(ctx.bias, ctx.slots[1], dy, B * Ho * Wo, Cout, ldy, ctx.zero_bias_grad, fork)
        return dx, dw, db, None, None, None, None, dst_w, None


def _dgrad_s2(dy, weight, g, prec):
    """dx of the stride-2 K x K dense conv g by phase decomposition (vmtl_conv2d_dgrad_s2): four stride-1 implicit-GEMM
    correlations of dy with the phases' tap subsets, interleaved into dx.  Runs under the forward's precision."""
    B, H, W, Cs, Ho, Wo, ldy, K, _, _, pad = g
    Cout, Cin = weight.shape[0], weight.shape[1]
    n = lib().raw("vmtl_pack_dgrad_s2_size")(Cin, ldy, K, pad)
    wd = packs.get_custom(weight, "dgrad_s2", (n,), lambda w, dst: _k(
        "vmtl_pack_dgrad_s2", w=w, dst=dst, Cout=Cout, Cin=Cin, ldy=ldy, K=K, pad=pad))
    ws = _empty((lib().raw("vmtl_conv2d_dgrad_s2_ws")(B, H, W, Cs, Ho, Wo, ldy, K, pad),), dy)
    dx = _empty((B, H, W, Cs), dy)
    _kp("vmtl_conv2d_dgrad_s2", prec, _flop=2.0 * B * Ho * Wo * Cout * K * K * Cin, dy=dy, wp=wd, dx=dx, ws=ws, B=B, H=H,
        W=W, Cs=Cs, Ho=Ho, Wo=Wo, ldy=ldy, Cin=Cin, K=K, pad=pad)
    return dx


class _BNActPw(torch.autograd.Function):
    """(y, stats) = conv1x1(act(BN(x))) (+ bias): a 1x1 conv that owns the BatchNorm + activation of its producer
    (timm InvertedResidual bn2 + act -> conv_pwl [3P]; MTAN attention bn1 + ReLU -> conv2, reference
    models/mtan_model.py:60-66,142-148) - the pointwise counterpart of _BNActConv.  x is the RAW output of the
    producing conv with its BatchNorm partial rows; normalise + activation run on the GEMM's operand fragments
    (vmtl_conv1x1_bn_fwd; the activated matrix is written back once for the weight gradient), and the data gradient
    ends with the activation's and BatchNorm's backward reduction (vmtl_conv1x1_bnbwd): no apply pass forward, no
    reduce pass backward."""

    @staticmethod
    def forward(ctx, x, stats, rpb, gamma, beta, rm, rv, nbt, weight, bias, res, cfg):
        C, training, momentum, eps, act, want_stats, zero_bias_grad, return_act = cfg
        x, weight = _req(x, "x"), _req(weight, "weight")
        B, H, W, Cs = x.shape
        M = B * H * W
        Cout, Cin = weight.shape[0], weight.shape[1]
        if ceil4(C) != Cs or Cin != C or tuple(weight.shape[2:]) != (1, 1):
            raise ValueError("bn_act_conv1x1: (Cout, C, 1, 1) weight over x's channels expected")
        if res is not None:
            res = _req(res, "res")
            if tuple(res.shape) != tuple(x.shape) or act != ACT_NONE:
                raise ValueError("bn_act_conv1x1: the residual operand needs x's shape and no activation (bn3 + skip)")
        mean, invstd, ca, cc = _bn_stats(x, stats, rpb, rm, rv, nbt, C, training, momentum, eps, (gamma, beta))
        wp = packs.get(weight, "fwd", Layout.fwd(Cout, Cin, 1, Cs))
        ldy = ceil4(Cout)
        a, y = _empty(x.shape, x), _empty((B, H, W, ldy), x)
        ostats = None
        if want_stats:
            ostats = _empty((lib().raw("vmtl_conv1x1_stats_rows")(M, ldy, Cs, 0 if res is None else 1), 2, ldy), x)
        # the weight gradient runs under conv_prec_code, the pointwise GEMMs (this one and the data gradient) under
        # pw_prec_code: fp32 unless the mode is "bf16_pw"
        ctx.prec, pw_prec = conv_prec_code(), pw_prec_code()
        ctx.pw_prec = pw_prec
        if res is None:
            _kp("vmtl_conv1x1_bn_fwd", pw_prec, _flop=2.0 * M * Cout * Cin, x=x, coef_a=ca, coef_c=cc, act_in=act, a_out=a,
                wp=wp, bias=bias, y=y, stats=ostats, M=M, Ks=Cs, ldy=ldy, Nw=Cout, Cout=Cout)
        else:
            _kp("vmtl_conv1x1_bn_res_fwd", pw_prec, _flop=2.0 * M * Cout * Cin, x=x, coef_a=ca, coef_c=cc, act_in=act, res=res,
                a_out=a, wp=wp, bias=bias, y=y, stats=ostats, M=M, Ks=Cs, ldy=ldy, Nw=Cout, Cout=Cout)
        ctx.save_for_backward(x, a, weight, mean, invstd, gamma, beta)
        ctx.cfg = (C, training, act, bias is not None, bool(zero_bias_grad), res is not None)
        ctx.slots = (_slot(gamma), _slot(beta), _slot(weight), _slot(bias))
        ctx.bias = bias
        ctx.set_materialize_grads(False)
        if ostats is not None:
            ctx.mark_non_differentiable(ostats)
        if return_act:  # a = act(BN(x)) [+ res] as a differentiable output: the block's own skip branch / a decoder tap
            return y, ostats, a
        return y, ostats

    @staticmethod
    def backward(ctx, dy, _dstats, d_a=None):
        x, a, weight, mean, invstd, gamma, beta = ctx.saved_tensors
        C, training, act, has_bias, zero_bias, has_res = ctx.cfg
        sg, sb, sw, sbias = ctx.slots
        if dy is None:
            if d_a is not None:
                raise NotImplementedError("bn_act_conv1x1: gradient through the activation output only")
            return (None,) * 12
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        M = B * H * W
        Cout, Cin = weight.shape[0], weight.shape[1]
        ldy = dy.shape[3]
        fork = side.mark()
        # ---- data gradient w.r.t. a = act(BN(x)), with act' and the BatchNorm-backward column sums in the epilogue
        wd = packs.get(weight, "dgrad", Layout.dgrad(Cout, Cin, 1, ldy))
        dz = _empty(x.shape, x)
        rows = lib().raw("vmtl_conv1x1_stats_rows")(M, Cs, ldy, 0 if d_a is None else 1)
        part = _empty((rows, 2, Cs), x)
        ez = _ez_kw((x, mean, invstd, gamma, beta, act))
        if d_a is None:
            _kp("vmtl_conv1x1_bnbwd", ctx.pw_prec, _flop=2.0 * M * Cin * Cout, dy=dy, wp=wd, dz=dz, stats=part, M=M, Ks=ldy,
                ldy=Cs, Nw=Cin, Cout=Cin, **ez)
        else:  # + the gradient that reached a through its other consumers, added before act' and the reduction
            if act != ACT_NONE:
                raise NotImplementedError("bn_act_conv1x1: a second consumer of the activation needs act = none")
            _kp("vmtl_conv1x1_bnbwd_add", ctx.pw_prec, _flop=2.0 * M * Cin * Cout, dy=dy, wp=wd, addend=_req(d_a, "d_a"), dz=dz,
                stats=part, M=M, Ks=ldy, ldy=Cs, Nw=Cin, Cout=Cin, **ez)
        dx, dgamma, dbeta = _bn_bwd_tail(part, rows, x, dz, mean, invstd, gamma, C, training, (sg, sb),
                                         ctx.needs_input_grad[0])
        # ---- parameter gradients (side stream when they go to arena slots)
        dw = _grad_buf(weight.shape, sw, x)
        with side.branch(sw is not None, M, fork, dy, a):
            _wgrad_into(a, dy, ConvGeom(B, H, W, Cs, H, W, ldy, 1, 1, 1, 0), Layout.fwd(Cout, Cin, 1, Cs), dw,
                        2.0 * M * Cout * Cin, ctx.prec)
        db = None
        if has_bias and ctx.needs_input_grad[9]:
            db = _bias_grad(ctx.bias, sbias, dy, M, Cout, ldy, zero_bias, fork)
        # act = none with a residual: d(res) is the gradient w.r.t. a itself = dz (no activation derivative in it)
        dres = dz if has_res and ctx.needs_input_grad[10] else None
        return dx, None, None, dgamma, dbeta, None, None, None, _grad_ret(dw, sw), db, dres, None


_BN_PW_MAX_ROWS = int(os.environ.get("VMTL_BN_PW_MAX_ROWS", str(1 << 30)))


def bn_act_conv1x1_supported(x, act):
    """Pointwise pre-activation node: pointwise-GEMM sized problems, activations with act(0) == 0."""
    return (_PW and x.shape[0] * x.shape[1] * x.shape[2] <= min(_PW_MAX_ROWS, _BN_PW_MAX_ROWS)
            and act in (ACT_NONE, ACT_RELU, ACT_HSWISH) and os.environ.get("VMTL_BN_PW", "1") != "0")


def bn_act_conv1x1(x, stats, rpb, bn, C, act, weight, bias=None, want_stats=True, zero_bias_grad=False, res=None,
                   return_act=False):
    """(y_raw, stats, rows_per_block[, a]) = conv1x1(a) (+ bias) with a = act(bn(x_raw)) [+ res]; bn = the nn.BatchNorm2d
    container of x's layer; res (act = none only): the skip connection added to the normalised map; return_act: also
    hand back a (differentiable) for its other consumers (the block's own skip branch, a decoder tap)."""
    tensors, mode = _bn_args(bn)
    cfg = (C, *mode, act, bool(want_stats), bool(zero_bias_grad), bool(return_act))
    out = _BNActPw.apply(x, stats, rpb, *tensors, weight, bias, res, cfg)
    y, ostats = out[0], out[1]
    orpb = 0
    if ostats is not None:
        orpb = lib().raw("vmtl_conv1x1_stats_block")(y.shape[0] * y.shape[1] * y.shape[2], y.shape[3], x.shape[3],
                                                     0 if res is None else 1)
    return (y, ostats, orpb, out[2]) if return_act else (y, ostats, orpb)


class _Conv1x1Cat(torch.autograd.Function):
    """(y, stats) = conv1x1(cat[xa, xb], weight) (+ bias) WITHOUT the concat (MTAN attention modules, reference
    models/mtan_model.py:57-59,139-141): the pointwise GEMM reads its K axis from two tensors, its data gradient
    writes the two input gradients directly, the weight gradient is taken per source into the two column ranges of dW.
    xa must fill its storage (Ca % 4 == 0) so that the ordinary packing of the (Cout, Ca + Cb) weight is the operand."""

    @staticmethod
    def forward(ctx, xa, xb, weight, bias, Cb, want_stats, zero_bias_grad):
        xa, xb, weight = _req(xa, "xa"), _req(xb, "xb"), _req(weight, "weight")
        B, H, W, Ca = xa.shape
        Cbs = xb.shape[3]
        Cout, Cin = weight.shape[0], weight.shape[1]
        if tuple(xb.shape[:3]) != (B, H, W) or tuple(weight.shape[2:]) != (1, 1) or Cin != Ca + Cb or ceil4(Cb) != Cbs:
            raise ValueError("conv1x1_cat: weight must be (Cout, Ca + Cb, 1, 1) over two maps of equal extent")
        M, Ks, ldy = B * H * W, Ca + Cbs, ceil4(Cout)
        wp = packs.get(weight, "fwd", Layout.fwd(Cout, Cin, 1, Ks))
        y = _empty((B, H, W, ldy), xa)
        stats = None
        if want_stats:
            stats = _empty((lib().raw("vmtl_conv1x1_stats_rows")(M, ldy, Ks, 0), 2, ldy), xa)
        # the weight gradient's precision, and the pointwise GEMMs' (forward here, data gradient in backward)
        ctx.prec, ctx.pw_prec = conv_prec_code(), pw_prec_code()
        _kp("vmtl_conv1x1_cat_fwd", ctx.pw_prec, _flop=2.0 * M * Cout * Cin, x=xa, K1=Ca, x2=xb, K2s=Cbs, wp=wp, bias=bias, y=y,
            stats=stats, M=M, ldy=ldy, Nw=Cout, Cout=Cout)
        ctx.save_for_backward(xa, xb, weight)
        ctx.cfg = (Cb, bias is not None, bool(zero_bias_grad))
        ctx.slots = (_slot(weight), _slot(bias))
        ctx.bias = bias
        ctx.set_materialize_grads(False)
        if want_stats:
            ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        xa, xb, weight = ctx.saved_tensors
        Cb, has_bias, zero_bias = ctx.cfg
        if dy is None:
            return (None,) * 7
        dy = _req(dy, "dy")
        B, H, W, Ca = xa.shape
        Cbs = xb.shape[3]
        Cout, Cin = weight.shape[0], weight.shape[1]
        M, ldy = B * H * W, dy.shape[3]
        sw, sbias = ctx.slots
        dxa = dxb = dw = db = None
        fork = side.mark()
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            wd = packs.get(weight, "dgrad", Layout.dgrad(Cout, Cin, 1, ldy))  # [Cin][ldy]
            dxa, dxb = _empty(xa.shape, xa), _empty(xb.shape, xa)
            _kp("vmtl_conv1x1_cat_dgrad", ctx.pw_prec, _flop=2.0 * M * Cin * Cout, dy=dy, wp=wd, dx=dxa, N1=Ca, dx2=dxb, N2s=Cbs,
                N2=Cb, M=M, Ks=ldy)
        if ctx.needs_input_grad[2]:
            with side.branch(sw is not None, M, fork, xa, xb, dy):
                dwt = _grad_buf(weight.shape, sw, xa)
                Ks = Ca + Cbs
                ns = lib().raw("vmtl_conv2d_wgrad_splits")(M, Cout, Ks)
                slabs = _empty((ns, Cout, Ks), xa)
                _kp("vmtl_conv1x1_cat_wgrad", ctx.prec, _flop=2.0 * M * Cout * Cin, x=xa, K1=Ca, x2=xb, K2s=Cbs, dy=dy, slabs=slabs,
                   splits=ns, M=M, ldy=ldy, Nw=Cout)
                unpack(slabs, Layout.fwd(Cout, Cin, 1, Ks), dwt.view(-1), nslabs=ns)
            dw = _grad_ret(dwt, sw)
        if has_bias and ctx.needs_input_grad[3]:
            db = _bias_grad(ctx.bias, sbias, dy, M, Cout, ldy, zero_bias, fork)
        return dxa, dxb, dw, db, None, None, None


def conv1x1_cat_supported(xa, Ca, xb):
    return _PW and Ca % 4 == 0 and xa.shape[3] == Ca and xa.shape[0] * xa.shape[1] * xa.shape[2] <= _PW_MAX_ROWS \
        and tuple(xa.shape[:3]) == tuple(xb.shape[:3]) and os.environ.get("VMTL_CAT_CONV", "1") != "0"


def conv1x1_cat(xa, xb, Cb, weight, bias=None, want_stats=False, zero_bias_grad=False):
    """conv1x1(cat[xa, xb]) without materialising the concat; returns (y, stats-or-None)."""
    y, stats = _Conv1x1Cat.apply(xa, xb, weight, bias, Cb, want_stats, zero_bias_grad)
    if stats is not None:
        stats._vmtl_rpb = lib().raw("vmtl_conv1x1_stats_block")(y.shape[0] * y.shape[1] * y.shape[2], y.shape[3],
                                                                xa.shape[3] + xb.shape[3], 0)
    return y, stats


class _Up2Conv(torch.autograd.Function):
    """conv3x3(pad 1, no bias)(cat[nearest_x2(xl), skip]) - the entry of every smp U-Net decoder block
    (reference utils/model_utils.py:25-34) - without materialising the upsample or the concat and with 4
    instead of 9 taps on the upsampled channels (four 2x2 phase convolutions on the low-res map).
    weight keeps the torch layout (Cout, C0 + C1, 3, 3), input channels ordered [xl | skip]."""

    @staticmethod
    def forward(ctx, xl, skip, weight, C0, plan):
        xl, weight = _req(xl, "xl"), _req(weight, "weight")
        B, H2, W2, C0s = xl.shape
        Cin = weight.shape[1]
        if tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("up2_conv: 3x3 kernels only")
        if skip is not None:
            skip = _req(skip, "skip")
            C1s = skip.shape[3]
            if tuple(skip.shape[:3]) != (B, 2 * H2, 2 * W2):
                raise ValueError("up2_conv: skip must be at twice the resolution of xl")
        else:
            C1s = 0
        C1 = Cin - C0
        if ceil4(C0) != C0s or ceil4(C1) != C1s or (C1 > 0) != (skip is not None):
            raise ValueError(f"up2_conv: weight has {Cin} input channels, sources hold {C0s}+{C1s} storage channels")
        prec = ctx.prec = conv_prec_code()
        y, stats = _up2_fwd(plan, xl, skip, weight, C0, prec)
        ctx.save_for_backward(xl, skip, weight)
        ctx.C0 = C0
        ctx.slot = _slot(weight)
        ctx.set_materialize_grads(False)
        if stats is not None:
            ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        xl, skip, weight = ctx.saved_tensors
        C0 = ctx.C0
        if dy is None:
            return None, None, None, None
        dy = _req(dy, "dy")
        B, H2, W2, C0s = xl.shape
        Cout, Cin = weight.shape[0], weight.shape[1]
        H, W, ldy = 2 * H2, 2 * W2, dy.shape[3]
        dxl = dskip = dw = None
        stamp(f"main up2 M={B * H * W} N={Cout} Cin={Cin}")
        fork = side.mark()
        if ctx.needs_input_grad[0]:  # 4x4 / stride 2 / pad 1 convolution over dY with pre-summed taps
            wd = packs.get_custom(weight, "up2_dgrad", (C0, 16 * ldy), lambda w, dst: _k(
                "vmtl_pack_up2_dgrad", w=w, dst=dst, Cout=Cout, Cos=ldy, C0=C0, Cin=Cin))
            dxl = _empty((B, H2, W2, C0s), xl)
            _conv_launch(dy, wd, None, dxl, ConvGeom(B, H, W, ldy, H2, W2, C0s, 4, 4, 2, 1), Cout=C0, cin=Cout,
                         algo_flop=2.0 * B * H * W * C0 * 9 * Cout, prec=ctx.prec)
        if skip is not None and ctx.needs_input_grad[1]:
            dskip = _up2_dskip(dy, weight, skip, C0, ctx.prec)
        if ctx.needs_input_grad[2]:
            dw = _grad_buf(weight.shape, ctx.slot, xl)
            with side.branch(ctx.slot is not None, B * H * W, fork, dy, xl, skip):
                _up2_wgrad(dy, xl, skip, weight, C0, dw, ctx.prec)
                stamp(f"side up2 M={B * H * W} N={Cout} Cin={Cin}")
            dw = _grad_ret(dw, ctx.slot)
        return dxl, dskip, dw, None, None


class _BNActConv(torch.autograd.Function):
    """(y, stats) = conv3x3(act(BN(x)))   or, with up2,   conv3x3(cat[nearest_x2(act(BN(x))), skip])
    - one smp `Conv2dReLU` boundary (reference utils/model_utils.py:25-34, 72-76) taken in PRE-activation form:
    x is the RAW output of the previous conv (stats = its BatchNorm partial rows from the conv epilogue, rpb pixels
    each), y the raw output of this one.  Owning BatchNorm+activation AND the consuming conv in one autograd node
    lets the backward pass fuse them: the data gradient of the conv ends with the activation + BatchNorm backward of
    its own input (dz and its per-row-block column sums come out of the implicit GEMM's epilogue,
    vmtl_conv2d_bnbwd), so the BatchNorm backward keeps only its finalize and apply launches - no reduce pass."""

    @staticmethod
    def forward(ctx, x, stats, rpb, gamma, beta, rm, rv, nbt, weight, skip, cfg):
        C, training, momentum, eps, act, up2, plan = cfg
        x, weight = _req(x, "x"), _req(weight, "weight")
        B, H, W, Cs = x.shape
        M = B * H * W
        Cout, Cin = weight.shape[0], weight.shape[1]
        if ceil4(C) != Cs or tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("bn_act_conv: 3x3 weight over x's channels expected")
        prec = ctx.prec = conv_prec_code()
        ldy = ceil4(Cout)
        # a 64/68-channel layer on the halo-tile kernel applies BatchNorm + activation as the conv's prologue (once per
        # input element, written back to a); everything else materialises a first
        pro = not up2 and skip is None and Cin == C and act in (ACT_NONE, ACT_RELU) and plan.route == "mid_halo"
        # ---- BatchNorm + activation (materialised: the weight gradient reads it)
        if pro:
            a = _empty(x.shape, x)
            mean, invstd, ca, cc = _bn_stats(x, stats, rpb, rm, rv, nbt, C, training, momentum, eps, (gamma, beta))
        else:
            a, mean, invstd = _bn_apply(x, stats, rpb, gamma, beta, rm, rv, nbt, C, training, momentum, eps, act)
        # ---- the conv on a
        if up2:
            if skip is not None:
                skip = _req(skip, "skip")
                C1s = skip.shape[3]
                if tuple(skip.shape[:3]) != (B, 2 * H, 2 * W):
                    raise ValueError("bn_act_conv(up2): skip must be at twice the resolution of x")
            else:
                C1s = 0
            C1 = Cin - C
            if ceil4(C1) != C1s or (C1 > 0) != (skip is not None):
                raise ValueError("bn_act_conv(up2): weight channels do not match x + skip")
            y, ostats = _up2_fwd(plan, a, skip, weight, C, prec)
        else:
            if Cin != C or skip is not None:
                raise ValueError("bn_act_conv: weight expects x's channels (skip only with up2)")
            wp = packs.get(weight, "fwd", Layout.fwd(Cout, Cin, 9, Cs))
            g = ConvGeom(B, H, W, Cs, H, W, ldy, 3, 3, 1, 1)
            y = _empty((B, H, W, ldy), x)
            ostats = _empty((plan.stats_rows, 2, ldy), x) if plan.stats_rows else None
            if pro:
                _halo_launch("mid_halo", x, wp, y, g, Cout, Cout, 2.0 * M * Cout * 9 * Cin, pa=ca, pc=cc, act_in=act, a_out=a,
                             stats=ostats, ep_mode=1 if ostats is not None else 0)
            else:
                _conv_launch(a, wp, None, y, g, Cout=Cout, cin=Cin, prec=prec, plan=plan, stats=ostats)
        ctx.save_for_backward(x, a, skip, weight, mean, invstd, gamma, beta)
        ctx.cfg = (C, training, act, up2)
        ctx.slots = (_slot(gamma), _slot(beta), _slot(weight))
        ctx.set_materialize_grads(False)
        if ostats is not None:
            ctx.mark_non_differentiable(ostats)
        return y, ostats

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, a, skip, weight, mean, invstd, gamma, beta = ctx.saved_tensors
        C, training, act, up2 = ctx.cfg
        sg, sb, sw = ctx.slots
        if dy is None:
            return (None,) * 11
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        M = B * H * W
        Cout, Cin = weight.shape[0], weight.shape[1]
        ldy = dy.shape[3]
        stamp(f"main bnconv M={dy.shape[0] * dy.shape[1] * dy.shape[2]} N={Cout} Cin={Cin}")
        fork = side.mark()
        gfwd = ConvGeom(B, H, W, Cs, H, W, ldy, 3, 3, 1, 1)  # the plain (not up2) forward conv
        # ---- data gradient w.r.t. a = act(BN(x)), with act' and the BatchNorm-backward column sums in the epilogue
        if up2:
            Hd, Wd = 2 * H, 2 * W  # dy's extent
            wd = packs.get_custom(weight, "up2_dgrad", (C, 16 * ldy), lambda w, dst: _k(
                "vmtl_pack_up2_dgrad", w=w, dst=dst, Cout=Cout, Cos=ldy, C0=C, Cin=Cin))
            geo = ConvGeom(B, Hd, Wd, ldy, H, W, Cs, 4, 4, 2, 1)
            flop, xflop = 2.0 * B * Hd * Wd * C * 9 * Cout, 2.0 * M * C * 16 * Cout
        else:
            Hd, Wd = H, W
            wd = packs.get(weight, "dgrad", Layout.dgrad(Cout, Cin, 9, ldy))
            geo = gfwd.dgrad()
            flop = xflop = 2.0 * M * Cin * 9 * Cout
        plan = conv_plan(*geo, prec=ctx.prec, epilogue="bnbwd")
        if plan.stats_rows:  # fused: the halo-tile kernels (ep_mode 2) or the implicit GEMM's BatchNorm-backward epilogue
            dz = _empty(x.shape, x)
            part = _empty((plan.stats_rows, 2, Cs), x)
            ez = (x, mean, invstd, gamma, beta, act)
            if plan.route in ("small", "mid_halo"):
                _halo_launch(plan.route, dy, wd, dz, geo, C, C, flop, stats=part, ep_mode=2, ez=ez)
            else:
                _kp("vmtl_conv2d_bnbwd", ctx.prec, _flop=flop, _xflop=xflop, x=dy, wp=wd, y=dz, stats=part, Nw=C, Cout=C,
                    **_ez_kw(ez), **geo._asdict())
            dx, dgamma, dbeta = _bn_bwd_tail(part, plan.stats_rows, x, dz, mean, invstd, gamma, C, training, (sg, sb),
                                             ctx.needs_input_grad[0])
        else:  # split-K data gradient (tile-starved layers) or VMTL_BNBWD_FUSE=0: unfused BatchNorm backward
            da = _empty(x.shape, x)
            _conv_launch(dy, wd, None, da, geo, Cout=C, cin=Cout, algo_flop=flop, prec=ctx.prec, plan=plan)
            dx, dgamma, dbeta, _ = _bn_bwd(x, da, mean, invstd, gamma, beta, C, training, act, (sg, sb))
        dskip = None
        if up2 and skip is not None and ctx.needs_input_grad[9]:
            dskip = _up2_dskip(dy, weight, skip, C, ctx.prec)
        # ---- weight gradient (side stream when it goes to an arena slot)
        dw = _grad_buf(weight.shape, sw, x)
        with side.branch(sw is not None, B * Hd * Wd, fork, dy, a, skip):
            if up2:
                _up2_wgrad(dy, a, skip, weight, C, dw, ctx.prec)
            else:
                _wgrad_into(a, dy, gfwd, Layout.fwd(Cout, Cin, 9, Cs), dw, 2.0 * M * Cout * 9 * Cin, ctx.prec)
            stamp(f"side bnconv N={Cout} Cin={Cin}")
        return dx, None, None, dgamma, dbeta, None, None, None, _grad_ret(dw, sw), dskip, None


def bn_act_conv(x, stats, rpb, bn, C, act, weight, skip=None, up2=False, want_stats=True):
    """(y_raw, stats, rows_per_block) = conv3x3(act(bn(x_raw)))  (up2: nearest-x2 of it, concatenated with skip, first);
    bn is the nn.BatchNorm2d parameter container of x's layer, C its logical channel count."""
    tensors, mode = _bn_args(bn)
    B, H, W, Cs = x.shape
    Cout, prec = weight.shape[0], conv_prec_code()
    if up2:
        plan = up2_plan(B, H, W, Cs, 0 if skip is None else skip.shape[3], ceil4(Cout), Cout, prec, want_stats)
    else:
        plan = conv_plan(B, H, W, Cs, H, W, ceil4(Cout), 3, 3, 1, 1, prec=prec, epilogue="stats" if want_stats else None)
    y, ostats = _BNActConv.apply(x, stats, rpb, *tensors, weight, skip, (C, *mode, act, bool(up2), plan))
    return y, ostats, plan.rpb


def up2_conv(xl, C0, skip, weight, want_stats=False):
    """(y, stats) = conv3x3(cat[nearest_x2(xl), skip]); C0 = logical channels of xl; stats may be None.  Like conv2d's, the
    statistics rows carry the pixels each covers (`_vmtl_rpb`: the UP2 plan's row block, not conv_pick_tile's)."""
    B, H2, W2, C0s = xl.shape
    Cout = weight.shape[0]
    plan = up2_plan(B, H2, W2, C0s, 0 if skip is None else skip.shape[3], ceil4(Cout), Cout, conv_prec_code(), want_stats)
    y, stats = _Up2Conv.apply(xl, skip, weight, C0, plan)
    if stats is not None:
        stats._vmtl_rpb = plan.rpb
    return y, stats


def conv2d(x, weight, bias=None, stride=1, pad=0, want_stats=False, zero_bias_grad=False, stitch=None):
    """zero_bias_grad: the caller normalises y with a TRAIN-mode BatchNorm next, which makes dL/dbias exactly zero.
    stitch = (CrossStitchLayer weights, task index): y = conv(w[task, task, (c)] * x), the scale folded into the operand."""
    Cout, _, KH, KW = weight.shape
    plan = conv_plan(*ConvGeom.of(x.shape, ceil4(Cout), KH, KW, stride, pad), prec=conv_prec_code(),
                     epilogue="stats" if want_stats else None)
    y, stats = _Conv2d.apply(x, weight, bias, stride, pad, plan, zero_bias_grad,
                             None if stitch is None else stitch[0], 0 if stitch is None else int(stitch[1]))
    if stats is not None:  # pixels per statistics row, for whoever finalizes them (bn_act)
        stats._vmtl_rpb = plan.rpb
    return (y, stats) if want_stats else y


# ----------------------------------------------------------------------------- ConvTranspose2d(k=2, s=2)
class _ConvT2x2(torch.autograd.Function):
    """weight in torch (Cin, Cout, 2, 2) layout; reference models/mtan_model.py:214-216."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _req(x, "x")
        weight = _req(weight, "weight")
        B, H, W, Cs = x.shape
        Cin, Cout = weight.shape[0], weight.shape[1]
        if tuple(weight.shape[2:]) != (2, 2) or ceil4(Cin) != Cs:
            raise ValueError("conv_transpose2x2: weight must be (Cin, Cout, 2, 2) matching the input channels")
        ldy = ceil4(Cout)
        wp = packs.get(weight, "ct_fwd", Layout.ct_fwd(Cin, Cout, Cs))
        y = _empty((B, 2 * H, 2 * W, ldy), x)
        _conv_launch(x, wp, bias, y, ConvGeom(B, H, W, Cs, H, W, ldy, 1, 1, 1, 0), Cout=Cout, Nw=4 * Cout, shuffle=1, cin=Cin)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.slots = (_slot(weight), _slot(bias))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        Cin, Cout = weight.shape[0], weight.shape[1]
        ldy = dy.shape[3]
        dx = dw = db = None
        # the data gradient is a 2x2 / stride-2 conv over dy
        g, lay = ConvGeom(B, 2 * H, 2 * W, ldy, H, W, Cs, 2, 2, 2, 0), Layout.ct_bwd(Cin, Cout, ldy)
        fork = side.mark()
        if ctx.needs_input_grad[0]:
            wd = packs.get(weight, "ct_bwd", lay)
            dx = _empty((B, H, W, Cs), x)
            _conv_launch(dy, wd, None, dx, g, Cout=Cin, cin=Cout)
        if ctx.needs_input_grad[1]:  # weight gradient of that same conv, with x in the role of its output gradient
            with side.branch(ctx.slots[0] is not None, B * H * W, fork, x, dy):
                dw = _grad_buf(weight.shape, ctx.slots[0], x)
                _wgrad_into(dy, x, g, lay, dw, 2.0 * B * H * W * Cin * 4 * Cout)
            dw = _grad_ret(dw, ctx.slots[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            with side.branch(ctx.slots[1] is not None, B * 4 * H * W, fork, dy):
                db = _colsum(dy, None, B * 4 * H * W, Cout, ldy, out=ctx.slots[1])
            db = _grad_ret(db, ctx.slots[1])
        return dx, dw, db


def conv_transpose2x2(x, weight, bias=None):
    return _ConvT2x2.apply(x, weight, bias)


# ----------------------------------------------------------------------------- depthwise conv
class _DwConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        x = _req(x, "x")
        weight = _req(weight, "weight")
        B, H, W, Cs = x.shape
        C, one, K, K2 = weight.shape
        if one != 1 or K != K2 or ceil4(C) != Cs:
            raise ValueError("dwconv: weight must be (C, 1, K, K) matching the input channels")
        Ho = (H + 2 * pad - K) // stride + 1
        Wo = (W + 2 * pad - K) // stride + 1
        wp = packs.get(weight, "dw", Layout.dw(C, K, Cs))
        y = _empty((B, Ho, Wo, Cs), x)
        _k("vmtl_dwconv_fwd", x=x, wp=wp, y=y, B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo, K=K, stride=stride, pad=pad)
        ctx.save_for_backward(x, weight, wp)
        ctx.cfg = (stride, pad)
        ctx.slot = _slot(weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, wp = ctx.saved_tensors
        stride, pad = ctx.cfg
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        C, _, K, _ = weight.shape
        _, Ho, Wo, _ = dy.shape
        dx = dw = None
        stamp(f"main dw M={B * Ho * Wo} C={C}")
        fork = side.mark()
        if ctx.needs_input_grad[0]:
            dx = _empty(x.shape, x)
            _k("vmtl_dwconv_bwd_data", dy=dy, wp=wp, dx=dx, B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo, K=K, stride=stride,
               pad=pad)
        if ctx.needs_input_grad[1]:
            with side.branch(ctx.slot is not None, B * Ho * Wo, fork, x, dy):
                partial = _empty((lib().raw("vmtl_dwconv_bwd_weight_rows")(B * Ho * Wo, Cs), K * K, Cs), x)
                dw = _grad_buf(weight.shape, ctx.slot, x)
                _k("vmtl_dwconv_bwd_weight", x=x, dy=dy, partial=partial, dw=dw, B=B, H=H, W=W, C=C, Cs=Cs, Ho=Ho,
                   Wo=Wo, K=K, stride=stride, pad=pad)
                stamp(f"side dw M={B * Ho * Wo} C={C}")
            dw = _grad_ret(dw, ctx.slot)
        return dx, dw, None, None


class _BNActDw(torch.autograd.Function):
    """(y, stats) = dwconv(act(BN(x))): timm InvertedResidual's conv_pw -> bn1 -> act -> conv_dw boundary (reference
    utils/model_utils.py:25-34 [3P]) as a pre-activation node.  x is the RAW pointwise-conv output with its BatchNorm
    partial rows; normalise + activation run while the depthwise taps are loaded and the output's own BatchNorm
    partial rows come from the same pass (vmtl_dwconv_bn_fwd): two launches fewer per block than apply / dwconv /
    statistics sweep.  The activated input is written back once (a) for the weight gradient."""

    @staticmethod
    def forward(ctx, x, stats, rpb, gamma, beta, rm, rv, nbt, weight, cfg):
        C, training, momentum, eps, act, stride, pad, want_stats, return_act = cfg
        x, weight = _req(x, "x"), _req(weight, "weight")
        B, H, W, Cs = x.shape
        Cw, one, K, K2 = weight.shape
        if one != 1 or K != K2 or Cw != C or ceil4(C) != Cs or pad != (K - 1) // 2:
            raise ValueError("bn_act_dwconv: weight must be (C, 1, K, K) over x's channels with pad (K-1)//2")
        Ho = (H + 2 * pad - K) // stride + 1
        Wo = (W + 2 * pad - K) // stride + 1
        mean, invstd, ca, cc = _bn_stats(x, stats, rpb, rm, rv, nbt, C, training, momentum, eps, (gamma, beta))
        wp = packs.get(weight, "dw", Layout.dw(C, K, Cs))
        need_bwd = any(ctx.needs_input_grad)
        a = _empty(x.shape, x) if need_bwd or return_act else None
        y = _empty((B, Ho, Wo, Cs), x)
        ostats = None
        if want_stats:
            ostats = _empty((lib().raw("vmtl_dwconv_bn_stats_rows")(B * Ho * Wo, Cs), 2, Cs), x)
        _k("vmtl_dwconv_bn_fwd", x=x, coef_a=ca, coef_c=cc, act=act, wp=wp, y=y, a_out=a, partial=ostats, B=B, H=H, W=W,
           Cs=Cs, Ho=Ho, Wo=Wo, K=K, stride=stride, pad=pad)
        ctx.save_for_backward(x, a, weight, wp, mean, invstd, gamma, beta)
        ctx.cfg = (C, training, act, stride, pad)
        ctx.slots = (_slot(gamma), _slot(beta), _slot(weight))
        ctx.set_materialize_grads(False)
        if ostats is not None:
            ctx.mark_non_differentiable(ostats)
        if return_act:  # a = act(BN(x)) as a second differentiable output (the residual branch of the block reads it)
            return y, ostats, a
        return y, ostats

    @staticmethod
    def backward(ctx, dy, _dstats, d_a=None):
        x, a, weight, wp, mean, invstd, gamma, beta = ctx.saved_tensors
        C, training, act, stride, pad = ctx.cfg
        sg, sb, sw = ctx.slots
        if dy is None:
            if d_a is not None:
                raise NotImplementedError("bn_act_dwconv: gradient through the activation output only")
            return (None,) * 10
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        K = weight.shape[2]
        _, Ho, Wo, _ = dy.shape
        stamp(f"main bndw M={B * Ho * Wo} C={C}")
        fork = side.mark()
        da = _empty(x.shape, x)
        if d_a is not None:  # + the gradient that reached a through its other consumer, added on the way out
            _k("vmtl_dwconv_bwd_data_add", dy=dy, wp=wp, addend=_req(d_a, "d_a"), dx=da, B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo,
               K=K, stride=stride, pad=pad)
        else:
            _k("vmtl_dwconv_bwd_data", dy=dy, wp=wp, dx=da, B=B, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo, K=K, stride=stride, pad=pad)
        dx, dgamma, dbeta, _ = _bn_bwd(x, da, mean, invstd, gamma, beta, C, training, act, (sg, sb))
        dw = _grad_buf(weight.shape, sw, x)
        with side.branch(sw is not None, B * Ho * Wo, fork, a, dy):
            partial = _empty((lib().raw("vmtl_dwconv_bwd_weight_rows")(B * Ho * Wo, Cs), K * K, Cs), x)
            _k("vmtl_dwconv_bwd_weight", x=a, dy=dy, partial=partial, dw=dw, B=B, H=H, W=W, C=C, Cs=Cs, Ho=Ho, Wo=Wo, K=K,
               stride=stride, pad=pad)
            stamp(f"side bndw C={C}")
        return dx, None, None, dgamma, dbeta, None, None, None, _grad_ret(dw, sw), None


def bn_act_dwconv(x, stats, rpb, bn, C, act, weight, stride=1, pad=1, want_stats=True, return_act=False):
    """(y_raw, stats, rows_per_block[, a]) = dwconv(act(bn(x_raw))); bn = the nn.BatchNorm2d container of x's layer;
    return_act: also hand back a = act(bn(x_raw)) (differentiable) for a second consumer of the activation."""
    tensors, mode = _bn_args(bn)
    cfg = (C, *mode, act, stride, pad, bool(want_stats), bool(return_act))
    out = _BNActDw.apply(x, stats, rpb, *tensors, weight, cfg)
    y, ostats = out[0], out[1]
    orpb = lib().raw("vmtl_dwconv_bn_stats_block")(y.shape[0] * y.shape[1] * y.shape[2], y.shape[3]) if ostats is not None else 0
    return (y, ostats, orpb, out[2]) if return_act else (y, ostats, orpb)


def dwconv(x, weight, stride=1, pad=1):
    return _DwConv.apply(x, weight, stride, pad)


# ----------------------------------------------------------------------------- BatchNorm + act (+ gate, + residual)
# statistics rows up to which BatchNorm finalize is folded into the apply launch (VMTL_BN_FUSE_ROWS overrides;
# the library accepts at most vmtl_bn_fuse_max_rows())
_BN_FUSE_ROWS = int(os.environ.get("VMTL_BN_FUSE_ROWS", "16"))  # measured: 16 rows neutral, 64 rows +0.5 ms/step (redundant fp64 merges)


class _BNAct(torch.autograd.Function):
    """y = act(BN(x)) [* mul] [+ res].  gamma/beta None -> plain activation (no normalisation)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, nbt, mul, res, stats, C, training, momentum, eps,
                act, stats_rpb=0):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        if mul is not None:
            mul = _req(mul, "mul")
        if res is not None:
            res = _req(res, "res")
        if gamma is None:  # plain activation: nothing to normalise with
            y, mean, invstd = _empty(x.shape, x), None, None
            _k("vmtl_bn_apply", x=x, mean=None, invstd=None, gamma=None, beta=beta, mul=mul, res=res, y=y, M=B * H * W, C=C,
               Cs=Cs, act=act)
        else:
            y, mean, invstd = _bn_apply(x, stats, stats_rpb, gamma, beta, running_mean, running_var, nbt, C, training,
                                        momentum, eps, act, mul, res)
        ctx.save_for_backward(x, gamma, beta, mean, invstd, mul)
        ctx.cfg = (C, training, act, res is not None)
        ctx.slots = (_slot(gamma), _slot(beta))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd, mul = ctx.saved_tensors
        C, training, act, has_res = ctx.cfg
        dy = _req(dy, "dy")
        dx, dgamma, dbeta, dmul = _bn_bwd(x, dy, mean, invstd, gamma, beta, C, training, act, ctx.slots, mul,
                                          mul is not None and ctx.needs_input_grad[6])
        return (dx, dgamma, dbeta, None, None, None, dmul, dy if has_res else None, None, None, None, None, None,
                None, None)


def bn_act(x, gamma, beta, running_mean, running_var, nbt, C, training, momentum=0.1, eps=1e-5, act=ACT_NONE,
           mul=None, res=None, stats=None, stats_rpb=0):
    """stats: BatchNorm partial rows from the producing conv's epilogue, stats_rpb pixels each (0: _resolve_rpb)."""
    return _BNAct.apply(x, gamma, beta, running_mean, running_var, nbt, mul, res, stats, C, training, momentum, eps,
                        act, _resolve_rpb(stats, stats_rpb, x.shape))


class _BNActPool(torch.autograd.Function):
    """maxpool2(act(BN(x))) as one node: the full-resolution activation and the full-resolution gradient of the pool never exist
    (vmtl_bn_act_pool2_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, nbt, stats, C, training, momentum, eps, act, stats_rpb):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        mean, invstd = _bn_stats(x, stats, stats_rpb, running_mean, running_var, nbt, C, training, momentum, eps)
        y = _empty((B, H // 2, W // 2, Cs), x)
        _k("vmtl_bn_act_pool2_fwd", x=x, mean=mean, invstd=invstd, gamma=gamma, beta=beta, y=y, B=B, H=H, W=W, C=C, Cs=Cs,
           act=act)
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.cfg = (C, training, act)
        ctx.slots = (_slot(gamma), _slot(beta))
        return y

    @staticmethod
    def backward(ctx, dyp):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        C, training, act = ctx.cfg
        dyp = _req(dyp, "dy")
        B, H, W, Cs = x.shape
        partial = _empty((_reduce_rows(B * (H // 2) * (W // 2)), 2, Cs), x)
        sum_dzx, sum_dz = _grad_buf((C,), ctx.slots[0], x), _grad_buf((C,), ctx.slots[1], x)  # exactly C entries each
        dx = _empty(x.shape, x)
        _k("vmtl_bn_act_pool2_bwd", x=x, dyp=dyp, mean=mean, invstd=invstd, gamma=gamma, beta=beta, partial=partial,
           sum_dz=sum_dz, sum_dzx=sum_dzx, dx=dx, B=B, H=H, W=W, C=C, Cs=Cs, act=act, training=1 if training else 0)
        return (dx, _grad_ret(sum_dzx, ctx.slots[0]), _grad_ret(sum_dz, ctx.slots[1]), None, None, None, None, None, None, None,
                None, None, None)


FUSE_BN_POOL = os.environ.get("VMTL_FUSE_BN_POOL", "1") != "0"  # MTAN encoder attention: BN + ReLU + MaxPool2d as one node


def bn_act_pool2(x, gamma, beta, running_mean, running_var, nbt, C, training, momentum=0.1, eps=1e-5, act=ACT_NONE,
                 stats=None, stats_rpb=0):
    """maxpool2(act(BN(x))); falls back to the two separate nodes for odd extents (MaxPool2d floors) or when switched off."""
    B, H, W, Cs = x.shape
    stats_rpb = _resolve_rpb(stats, stats_rpb, x.shape)
    if not FUSE_BN_POOL or (H & 1) or (W & 1) or H < 2 or W < 2:
        return maxpool2(bn_act(x, gamma, beta, running_mean, running_var, nbt, C, training, momentum, eps, act, stats=stats,
                               stats_rpb=stats_rpb))
    return _BNActPool.apply(x, gamma, beta, running_mean, running_var, nbt, stats, C, training, momentum, eps, act, stats_rpb)


class _BNActPool3(torch.autograd.Function):
    """(a, p) = (act(BN(x)), maxpool3x3/s2/p1(a)) as one node - the ResNet stem's bn1 + relu + maxpool, whose activation is
    also the decoder's stride-2 skip.  gamma None: the plain pool of an already activated x (no BatchNorm; a is not
    returned then).  Backward: one gather per input pixel (skip gradient + the windows whose arg-max it is), then act' and
    the BatchNorm backward sweeps (vmtl_bn_act_pool3s2_bwd)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, stats, cfg):
        C, training, momentum, eps, act, stats_rpb = cfg
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        bn = rm is not None
        mean = invstd = None
        if bn:
            mean, invstd = _bn_stats(x, stats, stats_rpb, rm, rv, nbt, C, training, momentum, eps)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        a = _empty(x.shape, x) if bn else None
        p = _empty((B, Ho, Wo, Cs), x)
        idx = torch.empty((B, Ho, Wo, Cs), dtype=torch.uint8, device=x.device)
        _k("vmtl_bn_act_pool3s2_fwd", x=x, mean=mean, invstd=invstd, gamma=gamma, beta=beta, a_out=a, y=p, idx=idx, B=B,
           H=H, W=W, C=C, Cs=Cs, act=act)
        ctx.save_for_backward(x, idx, mean, invstd, gamma, beta)
        ctx.cfg = (C, training, act, bn)
        ctx.slots = (_slot(gamma), _slot(beta))
        ctx.set_materialize_grads(False)
        return (a, p) if bn else p

    @staticmethod
    def backward(ctx, *grads):
        x, idx, mean, invstd, gamma, beta = ctx.saved_tensors
        C, training, act, bn = ctx.cfg
        da, dp = grads if bn else (None, grads[0])
        B, H, W, Cs = x.shape
        if dp is None:
            dp = torch.zeros(idx.shape, dtype=torch.float32, device=x.device)
        dp = _req(dp, "dy")
        da = None if da is None else _req(da, "dskip")
        dx = _empty(x.shape, x)
        dgamma = dbeta = None
        if bn:
            M = B * H * W
            dgamma, dbeta = _grad_buf((C,), ctx.slots[0], x), _grad_buf((C,), ctx.slots[1], x)  # exactly C entries each
            _k("vmtl_bn_act_pool3s2_bwd", x=x, dskip=da, dyp=dp, idx=idx, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
               dz=_empty(x.shape, x), partial=_empty((_reduce_rows(M), 2, Cs), x), sum_dz=dbeta, sum_dzx=dgamma, dx=dx,
               B=B, H=H, W=W, C=C, Cs=Cs, act=act, training=1 if training else 0)
            dgamma, dbeta = _grad_ret(dgamma, ctx.slots[0]), _grad_ret(dbeta, ctx.slots[1])
        else:
            _k("vmtl_bn_act_pool3s2_bwd", x=x, dskip=None, dyp=dp, idx=idx, mean=None, invstd=None, gamma=None, beta=None,
               dz=None, partial=None, sum_dz=None, sum_dzx=None, dx=dx, B=B, H=H, W=W, C=C, Cs=Cs, act=act, training=0)
        return dx, dgamma, dbeta, None, None, None, None, None


FUSE_STEM_POOL = os.environ.get("VMTL_FUSE_STEM_POOL", "1") != "0"  # ResNet stem: BN + ReLU + MaxPool2d(3, 2, 1) as one node


def bn_act_pool3(x, bn, C, act, stats=None, stats_rpb=0):
    """(act(bn(x)), maxpool3x3/s2/p1 of it): the activated map and its pool from one node (FUSE_STEM_POOL), else a
    BatchNorm node followed by the plain pool node."""
    stats_rpb = _resolve_rpb(stats, stats_rpb, x.shape)
    tensors, mode = _bn_args(bn)
    if not FUSE_STEM_POOL:
        a = bn_act(x, *tensors, C, *mode, act, stats=stats, stats_rpb=stats_rpb)
        return a, maxpool3s2(a, C)
    return _BNActPool3.apply(x, *tensors, stats, (C, *mode, act, stats_rpb))


def maxpool3s2(x, C):
    """MaxPool2d(3, stride 2, padding 1) of an activation (floor mode, torch's tie / NaN rule)."""
    return _BNActPool3.apply(x, None, None, None, None, None, None, (C, False, 0.0, 0.0, ACT_NONE, 0))


class _BNAddAct(torch.autograd.Function):
    """y = act(BN_a(z) + r) - the close of a torchvision BasicBlock - with r = res (the block input) or BN_b(zd) (the
    downsample branch's raw 1x1 conv output); both BatchNorms are applied in the same sweep.  z / zd come with their conv
    epilogue partial rows.  Backward: g = dy * act'(.) once; it is the identity gradient, and both BatchNorm backwards run
    off it (vmtl_bn_add_act_bwd)."""

    @staticmethod
    def forward(ctx, z, stats, ga, ba, rma, rva, nbta, res, zd, statsd, gb, bb, rmb, rvb, nbtb, cfg):
        C, training, mom_a, eps_a, rpb, mom_b, eps_b, rpbd, act = cfg
        z = _req(z, "z")
        B, H, W, Cs = z.shape
        M = B * H * W
        mean_a, invstd_a = _bn_stats(z, stats, rpb, rma, rva, nbta, C, training, mom_a, eps_a)
        mean_b = invstd_b = None
        if zd is not None:
            zd = _req(zd, "zd")
            if zd.shape != z.shape:
                raise ValueError(f"bn_add_act: downsample branch {tuple(zd.shape)} vs main branch {tuple(z.shape)}")
            mean_b, invstd_b = _bn_stats(zd, statsd, rpbd, rmb, rvb, nbtb, C, training, mom_b, eps_b)
        else:
            res = _req(res, "res")
            if res.shape != z.shape:
                raise ValueError(f"bn_add_act: residual {tuple(res.shape)} vs main branch {tuple(z.shape)}")
        y = _empty(z.shape, z)
        _k("vmtl_bn_add_act_fwd", z=z, mean_a=mean_a, invstd_a=invstd_a, gamma_a=ga, beta_a=ba, res=res, zd=zd,
           mean_b=mean_b, invstd_b=invstd_b, gamma_b=gb, beta_b=bb, y=y, M=M, C=C, Cs=Cs, act=act)
        ctx.save_for_backward(z, mean_a, invstd_a, ga, ba, res, zd, mean_b, invstd_b, gb, bb)
        ctx.cfg = (C, training, act)
        ctx.slots = (_slot(ga), _slot(ba), _slot(gb), _slot(bb))
        return y

    @staticmethod
    def backward(ctx, dy):
        z, mean_a, invstd_a, ga, ba, res, zd, mean_b, invstd_b, gb, bb = ctx.saved_tensors
        C, training, act = ctx.cfg
        sga, sba, sgb, sbb = ctx.slots
        dy = _req(dy, "dy")
        B, H, W, Cs = z.shape
        M = B * H * W
        g = _empty(z.shape, z)
        dga, dba = _grad_buf((C,), sga, z), _grad_buf((C,), sba, z)
        dgb = dbb = dzd = None
        if zd is not None:
            dgb, dbb = _grad_buf((C,), sgb, z), _grad_buf((C,), sbb, z)
            dzd = _empty(z.shape, z)
        dz = _empty(z.shape, z)
        _k("vmtl_bn_add_act_bwd", z=z, mean_a=mean_a, invstd_a=invstd_a, gamma_a=ga, beta_a=ba, res=res, zd=zd,
           mean_b=mean_b, invstd_b=invstd_b, gamma_b=gb, beta_b=bb, dy=dy, g=g, partial=_empty((_reduce_rows(M), 3, Cs), z),
           sum_dz_a=dba, sum_dzx_a=dga, sum_dz_b=dbb, sum_dzx_b=dgb, dz=dz, dzd=dzd, M=M, C=C, Cs=Cs, act=act,
           training=1 if training else 0)
        return (dz, None, _grad_ret(dga, sga), _grad_ret(dba, sba), None, None, None, g if res is not None else None, dzd,
                None, _grad_ret(dgb, sgb), _grad_ret(dbb, sbb), None, None, None, None)


def bn_add_act(z, stats, rpb, bn, C, act, res=None, zd=None, statsd=None, rpbd=0, bn_d=None):
    """act(bn(z) + res)  or  act(bn(z) + bn_d(zd)): z / zd raw conv outputs with their statistics rows (rpb pixels each)."""
    ta, (training, mom_a, eps_a) = _bn_args(bn)
    tb, (_, mom_b, eps_b) = _bn_args(bn_d) if bn_d is not None else ((None,) * 5, (training, 0.1, 1e-5))
    if (res is None) == (zd is None):
        raise ValueError("bn_add_act: give exactly one of res (identity) and zd (downsample branch)")
    # zd has z's shape (the node checks it)
    cfg = (C, training, mom_a, eps_a, _resolve_rpb(stats, rpb, z.shape), mom_b, eps_b, _resolve_rpb(statsd, rpbd, z.shape),
           act)
    return _BNAddAct.apply(z, stats, *ta, res, zd, statsd, *tb, cfg)


def activation(x, act, C, mul=None):
    """Plain activation (optionally times a gate operand) through the same fused kernel."""
    return _BNAct.apply(x, None, None, None, None, None, mul, None, None, C, False, 0.0, 0.0, act, 0)


# ----------------------------------------------------------------------------- concat / upsample / pad
class _Concat2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, Ca, Cb, up_a, up_b, H, W, off_a, off_b):
        a = _req(a, "a")
        B, Ha, Wa, Csa = a.shape
        if b is not None:
            b = _req(b, "b")
            _, Hb, Wb, Csb = b.shape
        else:
            Hb = Wb = Csb = 0
            Cb = 0
        Cd = ceil4(Ca + Cb)
        y = _empty((B, H, W, Cd), a)
        _k("vmtl_concat2", a=a, Ha=Ha, Wa=Wa, Ca=Ca, Csa=Csa, upa=up_a, oha=off_a[0], owa=off_a[1], b=b, Hb=Hb, Wb=Wb,
           Cb=Cb, Csb=Csb, upb=up_b, ohb=off_b[0], owb=off_b[1], y=y, B=B, H=H, W=W, Cd=Cd)
        ctx.cfg = (a.shape, None if b is None else b.shape, Ca, Cb, up_a, up_b, H, W, off_a, off_b)
        return y

    @staticmethod
    def backward(ctx, dy):
        ashape, bshape, Ca, Cb, up_a, up_b, H, W, off_a, off_b = ctx.cfg
        dy = _req(dy, "dy")
        B, _, _, Cd = dy.shape
        da = db = None
        if ctx.needs_input_grad[0]:
            da = _empty(ashape, dy)
            _k("vmtl_concat2_bwd", dy=dy, dx=da, B=B, H=H, W=W, Cd=Cd, c_off=0, Hs=ashape[1], Ws=ashape[2], C=Ca,
               Cs=ashape[3], up=up_a, oh=off_a[0], ow=off_a[1])
        if bshape is not None and ctx.needs_input_grad[1]:
            db = _empty(bshape, dy)
            _k("vmtl_concat2_bwd", dy=dy, dx=db, B=B, H=H, W=W, Cd=Cd, c_off=Ca, Hs=bshape[1], Ws=bshape[2], C=Cb,
               Cs=bshape[3], up=up_b, oh=off_b[0], ow=off_b[1])
        return da, db, None, None, None, None, None, None, None, None


def concat2(a, Ca, b=None, Cb=0, up_a=1, up_b=1, out_hw=None, off_a=(0, 0), off_b=(0, 0)):
    """Channel concat [a | b] into an (H, W) canvas; each source may be nearest-x2 upsampled
    and/or placed at an offset (zeros elsewhere).  b=None: pure upsample / pad of a."""
    if out_hw is None:
        out_hw = (a.shape[1] * up_a, a.shape[2] * up_a)
    return _Concat2.apply(a, b, Ca, Cb, up_a, up_b, out_hw[0], out_hw[1], tuple(off_a), tuple(off_b))


# ----------------------------------------------------------------------------- pooling / bilinear
class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        y = _empty((B, H // 2, W // 2, Cs), x)
        _k("vmtl_maxpool2_fwd", x=x, y=y, B=B, H=H, W=W, Cs=Cs)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        dx = _empty(x.shape, x)
        _k("vmtl_maxpool2_bwd", x=x, dy=dy, dx=dx, B=B, H=H, W=W, Cs=Cs)
        return dx


def maxpool2(x):
    return _MaxPool2.apply(x)


class _BilinearUp2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        y = _empty((B, 2 * H, 2 * W, Cs), x)
        _k("vmtl_bilinear_up2_fwd", x=x, y=y, B=B, H=H, W=W, Cs=Cs)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        B, H, W, Cs = ctx.shape
        dx = _empty(ctx.shape, dy)
        _k("vmtl_bilinear_up2_bwd", dy=dy, dx=dx, B=B, H=H, W=W, Cs=Cs)
        return dx


def bilinear_up2(x):
    return _BilinearUp2.apply(x)


# ----------------------------------------------------------------------------- squeeze-excite pieces
class _SpatialMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        y = _empty((B, 1, 1, Cs), x)
        _k("vmtl_spatial_mean", x=x, y=y, B=B, HW=H * W, Cs=Cs)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        B, H, W, Cs = ctx.shape
        dx = _empty(ctx.shape, dy)
        _k("vmtl_channel_bcast", x=None, s=dy, y=dx, B=B, HW=H * W, Cs=Cs, mode=1)
        return dx


def spatial_mean(x):
    return _SpatialMean.apply(x)


class _ChannelScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        x, s = _req(x, "x"), _req(s, "s")
        B, H, W, Cs = x.shape
        y = _empty(x.shape, x)
        _k("vmtl_channel_bcast", x=x, s=s, y=y, B=B, HW=H * W, Cs=Cs, mode=0)
        ctx.save_for_backward(x, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, s = ctx.saved_tensors
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        dx = ds = None
        if ctx.needs_input_grad[0]:
            dx = _empty(x.shape, x)
            _k("vmtl_channel_bcast", x=dy, s=s, y=dx, B=B, HW=H * W, Cs=Cs, mode=0)
        if ctx.needs_input_grad[1]:
            ds = _empty(s.shape, x)
            _k("vmtl_channel_scale_bwd_s", x=x, dy=dy, ds=ds, B=B, HW=H * W, Cs=Cs)
        return dx, ds


def channel_scale(x, s):
    return _ChannelScale.apply(x, s)


# ----------------------------------------------------------------------------- cross-stitch (diagonal scale)
class _SqueezeExcite(torch.autograd.Function):
    """y = x * act2(W_e act1(W_r mean_hw(x) + b_r) + b_e) - timm SqueezeExcite (ReLU / hard-sigmoid in
    MobileNetV3), the gate of the `basic` encoder's inverted-residual blocks - as two launches: the gate of every
    image (spatial mean and both GEMVs, vmtl_se_gate_fwd) and one scale pass.  Backward: the gate's gradient
    (sum_hw dy*x and both transposed GEMVs with the activation backward, vmtl_se_gate_bwd), one pass
    dx = dy*g + dmean/HW; the four parameter gradients come from one small launch in the torch layout (side
    stream when they go to arena slots).  Weights are the torch (R, C, 1, 1) / (C, R, 1, 1) conv parameters, read
    as they are.  vmtl_se_gate_supported decides per shape and direction: the forward gate of the blocks with large
    weights (480 channels and up) stays on the earlier sequence - per-image partial sums over HW, two batch-sized GEMMs
    (vmtl_fc_fwd) - which reads the weights once instead of once per image.  VMTL_SE_FUSED=0 restores that sequence
    everywhere (backward: the GEMMs on packed transposes, two vmtl_fc_wgrad), VMTL_SE_FUSED=2 fuses everything."""

    @staticmethod
    def forward(ctx, x, wr, br, we, be, act1, act2):
        x, wr, we = _req(x, "x"), _req(wr, "reduce weight"), _req(we, "expand weight")
        B, H, W, Cs = x.shape
        HW = H * W
        R, C = wr.shape[0], wr.shape[1]
        if ceil4(C) != Cs or tuple(we.shape[:2]) != (C, R) or br is None or be is None:
            raise ValueError("squeeze_excite: weights must be (R, C, 1, 1) / (C, R, 1, 1) with biases, matching x")
        if B > lib().raw("vmtl_fc_max_rows")():
            raise ValueError("squeeze_excite: batch too large for the batch-sized GEMM kernels")
        Rs = ceil4(R)
        ctx.acts = (act1, act2)
        ctx.slots = (_slot(wr), _slot(br), _slot(we), _slot(be))
        route = lib().raw("vmtl_se_gate_supported")(B, C, R)  # bit 0: backward + weight gradient, bit 1: forward
        ctx.fused = bool(route & 1)
        if route & 2:
            pooled, z1, h = _empty((B, Cs), x), _empty((B, Rs), x), _empty((B, Rs), x)
            z2, g = _empty((B, Cs), x), _empty((B, Cs), x)
            _k("vmtl_se_gate_fwd", x=x, wr=wr, br=br, we=we, be=be, pooled=pooled, z1=z1, h=h, z2=z2, g=g, B=B, HW=HW,
               C=C, R=R, act1=act1, act2=act2)
            y = _empty(x.shape, x)
            _k("vmtl_channel_scale_add", x=x, s=g, t=None, t_scale=0.0, y=y, B=B, HW=HW, Cs=Cs)
            ctx.save_for_backward(x, pooled, z1, h, z2, g, wr, we)
            return y
        S = lib().raw("vmtl_hw_reduce_parts")(B, HW, Cs)
        parts = _empty((S, B, Cs), x)
        _k("vmtl_hw_reduce", x=x, y=None, part=parts, B=B, HW=HW, Cs=Cs)
        z1, h = _empty((B, Rs), x), _empty((B, Rs), x)
        pooled = _empty((B, Cs), x)  # finished mean (a_out): every [b][c < Cs] is written since Cs <= ceil16(C)
        _k("vmtl_fc_fwd", a=parts, a_parts=S, a_part_stride=B * Cs, a_scale=1.0 / HW, a_z=None, a_act=0, a_out=pooled,
           w=wr, bias=br, z=z1, y=h, M=B, K=C, N=R, lda=Cs, ldw=C, ldy=Rs, act=act1)
        z2, g = _empty((B, Cs), x), _empty((B, Cs), x)
        _k("vmtl_fc_fwd", a=h, a_parts=1, a_part_stride=0, a_scale=1.0, a_z=None, a_act=0, a_out=None, w=we, bias=be,
           z=z2, y=g, M=B, K=R, N=C, lda=Rs, ldw=R, ldy=Cs, act=act2)
        y = _empty(x.shape, x)
        _k("vmtl_channel_scale_add", x=x, s=g, t=None, t_scale=0.0, y=y, B=B, HW=HW, Cs=Cs)
        ctx.save_for_backward(x, pooled, z1, h, z2, g, wr, we)
        ctx.S = S
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pooled, z1, h, z2, g, wr, we = ctx.saved_tensors
        act1, act2 = ctx.acts
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        HW = H * W
        R, C = wr.shape[0], wr.shape[1]
        Rs = ceil4(R)
        slots, shapes = ctx.slots, (wr.shape, (R,), we.shape, (C,))
        all_slots = all(s is not None for s in slots)
        if ctx.fused:
            dg, dh = _empty((B, Cs), x), _empty((B, Rs), x)  # both finished, for the weight gradients
            dmean = _empty((B, Cs), x) if ctx.needs_input_grad[0] else None
            _k("vmtl_se_gate_bwd", dy=dy, x=x, z1=z1, z2=z2, wr=wr, we=we, dg=dg, dh=dh, dmean=dmean, B=B, HW=HW, C=C, R=R,
               act1=act1, act2=act2)
            fork = side.mark()
            dx = None
            if dmean is not None:
                dx = _empty(x.shape, x)
                _k("vmtl_channel_scale_add", x=dy, s=g, t=dmean, t_scale=1.0 / HW, y=dx, B=B, HW=HW, Cs=Cs)
            with side.branch(all_slots, B, fork, dg, dh, pooled, z1, h, z2):
                dwr, dbr, dwe, dbe = grads = [_grad_buf(s, sl, x) for s, sl in zip(shapes, slots)]
                _k("vmtl_se_wgrad", pooled=pooled, h=h, dg=dg, dh=dh, z1=z1, z2=z2, dwr=dwr, dbr=dbr, dwe=dwe, dbe=dbe,
                   B=B, C=C, R=R, act1=act1, act2=act2)
            return (dx, *map(_grad_ret, grads, slots), None, None)
        S = ctx.S
        # dg[b][c] = sum_hw dy*x, left as per-slice partial sums for the GEMM to finish
        dparts = _empty((S, B, Cs), x)
        _k("vmtl_hw_reduce", x=dy, y=x, part=dparts, B=B, HW=HW, Cs=Cs)
        weT = packs.get(we, "dgrad", Layout.dgrad(C, R, 1, Cs))   # [R][Cs]
        dh = _empty((B, Rs), x)
        dg = _empty((B, Cs), x)  # finished sum_hw dy*x (a_out), for the weight gradient
        _k("vmtl_fc_fwd", a=dparts, a_parts=S, a_part_stride=B * Cs, a_scale=1.0, a_z=z2, a_act=act2, a_out=dg, w=weT,
           bias=None, z=None, y=dh, M=B, K=C, N=R, lda=Cs, ldw=Cs, ldy=Rs, act=0)
        fork = side.mark()
        dx = None
        if ctx.needs_input_grad[0]:
            wrT = packs.get(wr, "dgrad", Layout.dgrad(R, C, 1, Rs))  # [C][Rs]
            dmean = _empty((B, Cs), x)
            _k("vmtl_fc_fwd", a=dh, a_parts=1, a_part_stride=0, a_scale=1.0, a_z=z1, a_act=act1, a_out=None, w=wrT,
               bias=None, z=None, y=dmean, M=B, K=R, N=C, lda=Rs, ldw=Rs, ldy=Cs, act=0)
            dx = _empty(x.shape, x)
            _k("vmtl_channel_scale_add", x=dy, s=g, t=dmean, t_scale=1.0 / HW, y=dx, B=B, HW=HW, Cs=Cs)
        with side.branch(all_slots, B, fork, dg, dh, pooled, z1, h, z2):
            dwr, dbr, dwe, dbe = grads = [_grad_buf(s, sl, x) for s, sl in zip(shapes, slots)]
            _k("vmtl_fc_wgrad", x=h, x_parts=1, x_part_stride=0, x_scale=1.0, dyo=dg, dy_parts=1, dy_part_stride=0,
               zo=z2, dw=dwe, db=dbe, M=B, K=R, N=C, lda=Rs, ldn=Cs, act=act2)
            _k("vmtl_fc_wgrad", x=pooled, x_parts=1, x_part_stride=0, x_scale=1.0, dyo=dh, dy_parts=1,
               dy_part_stride=0, zo=z1, dw=dwr, db=dbr, M=B, K=C, N=R, lda=Cs, ldn=Rs, act=act1)
        return (dx, *map(_grad_ret, grads, slots), None, None)


def squeeze_excite(x, w_reduce, b_reduce, w_expand, b_expand, act1=ACT_RELU, act2=ACT_HSIGMOID):
    return _SqueezeExcite.apply(x, w_reduce, b_reduce, w_expand, b_expand, act1, act2)


def squeeze_excite_max_batch() -> int:
    return lib().raw("vmtl_fc_max_rows")()


class _Stitch(torch.autograd.Function):
    """y = w[a, a, (c)] * x for task a; `weights` is the full (T,T[,C]) parameter
    (reference models/cross_stitch_model.py:21-37).  Off-diagonal entries get zero gradient."""

    @staticmethod
    def forward(ctx, x, weights, task, C):
        x = _req(x, "x")
        weights = _req(weights, "weights")
        B, H, W, Cs = x.shape
        T = weights.shape[0]
        channel_wise = weights.dim() == 3
        # element offset of w[task, task, 0] and the stride between channels
        off = (task * T + task) * (weights.shape[2] if channel_wise else 1)
        wview = weights.view(-1)[off:]
        y = _empty(x.shape, x)
        # _flop slot = algorithmic BYTES here (8 B per element: read + write) for bench.py's HBM roofline
        _k("vmtl_stitch", _flop=8.0 * B * H * W * C, x=x, w=wview, y=y, M=B * H * W, C=C, Cs=Cs, wstride=1 if channel_wise else 0)
        ctx.save_for_backward(x, weights)
        ctx.cfg = (task, C, channel_wise, off)
        ctx.slot = _slot(weights)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weights = ctx.saved_tensors
        task, C, channel_wise, off = ctx.cfg
        dy = _req(dy, "dy")
        B, H, W, Cs = x.shape
        M = B * H * W
        dx = dw = None
        wv = weights.view(-1)[off:]
        ws = 1 if channel_wise else 0
        if ctx.needs_input_grad[1]:
            n = C if channel_wise else 1
            if ctx.slot is not None:  # arena slot (off-diagonal entries stay at their initial zero)
                out = ctx.slot.view(-1)[off:off + n]
            else:
                dw = torch.zeros_like(weights)
                out = dw.view(-1)[off:off + n]
            dx = _empty(x.shape, x) if ctx.needs_input_grad[0] else None
            # one sweep: dx = w * dy and the column sums of x * dy
            _k("vmtl_stitch_bwd", x=x, dy=dy, w=wv, dx=dx, partial=_empty((_reduce_rows(M) + 1, Cs), x), dw=out, M=M, C=C, Cs=Cs,
               wstride=ws, reduce_all=0 if channel_wise else 1)
        elif ctx.needs_input_grad[0]:
            dx = _empty(x.shape, x)
            _k("vmtl_stitch", x=dy, w=wv, y=dx, M=M, C=C, Cs=Cs, wstride=ws)
        return dx, dw, None, None


def stitch(x, weights, task, C):
    return _Stitch.apply(x, weights, task, C)


class _StitchMix(torch.autograd.Function):
    """The full cross-stitch unit of two tasks (csrc/stitch_mix.hip): y_a = sum_b w[a, b, (c)] * x_b, `weights` the whole
    (2,2[,C]) parameter.  The opt-in mode the reference's einsum never reaches: every entry of the
    parameter gets a gradient, written by ONE launch (into the arena slot when there is one - overwritten, not added)."""

    @staticmethod
    def forward(ctx, x0, x1, weights, C):
        x0, x1 = _req(x0, "x0"), _req(x1, "x1")
        weights = _req(weights, "weights")
        if weights.shape[:2] != (2, 2):
            raise NotImplementedError(f"stitch_mix: two tasks only, got weights of shape {tuple(weights.shape)}")
        channel_wise = weights.dim() == 3
        if channel_wise and weights.shape[2] != C:
            raise ValueError(f"stitch_mix: the stitch layer has {weights.shape[2]} channels, the activations {C}")
        if x0.shape != x1.shape:
            raise ValueError(f"stitch_mix: the two tasks' activations differ in shape: {tuple(x0.shape)} / {tuple(x1.shape)}")
        B, H, W, Cs = x0.shape
        y0, y1 = _empty(x0.shape, x0), _empty(x0.shape, x0)
        # no _flop: bench.py files every recorded name it does not know under the conv forward family
        _k("vmtl_stitch_mix", x0=x0, x1=x1, w=weights, y0=y0, y1=y1, M=B * H * W, C=C, Cs=Cs, wstride=1 if channel_wise else 0)
        ctx.save_for_backward(x0, x1, weights)
        ctx.cfg = (C, channel_wise)
        ctx.slot = _slot(weights)
        return y0, y1

    @staticmethod
    def backward(ctx, dy0, dy1):
        x0, x1, weights = ctx.saved_tensors
        C, channel_wise = ctx.cfg
        dy0, dy1 = _req(dy0, "dy0"), _req(dy1, "dy1")
        B, H, W, Cs = x0.shape
        M = B * H * W
        want_dx = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx0 = dx1 = dw = out = partial = None
        if want_dx:
            dx0, dx1 = _empty(x0.shape, x0), _empty(x0.shape, x0)
        if ctx.needs_input_grad[2]:
            out = ctx.slot
            if out is None:
                out = dw = _empty(weights.shape, weights)
            partial = _empty((4 * _reduce_rows(M) + 4, Cs), x0)
        if want_dx or out is not None:  # one sweep: both data gradients and the four weight-gradient blocks
            _k("vmtl_stitch_mix_bwd", x0=x0, x1=x1, dy0=dy0, dy1=dy1, w=weights, dx0=dx0, dx1=dx1, partial=partial, dw=out,
               M=M, C=C, Cs=Cs, wstride=1 if channel_wise else 0)
        return (dx0 if ctx.needs_input_grad[0] else None, dx1 if ctx.needs_input_grad[1] else None, dw, None)


def stitch_mix(x0, x1, weights, C):
    """(y0, y1) = the full 2x2 cross-stitch mix of two tasks' activations."""
    return _StitchMix.apply(x0, x1, weights, C)


# ----------------------------------------------------------------------------- boundary layout + postprocess
class _ToNHWC(torch.autograd.Function):
    """(B,C,H,W) contiguous -> internal [B,H,W,Cs]."""

    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        B, C, H, W = x.shape
        Cs = ceil4(C)
        y = _empty((B, H, W, Cs), x)
        _k("vmtl_nchw_to_nhwc", x=x, y=y, B=B, C=C, HW=H * W, Cs=Cs, Cw=Cs)
        ctx.C = C
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "dy")
        B, H, W, Cs = dy.shape
        dx = _empty((B, ctx.C, H, W), dy)
        _k("vmtl_nhwc_to_nchw", x=dy, y=dx, B=B, C=ctx.C, HW=H * W, Cs=Cs)
        return dx


def to_nhwc(x):
    st = getattr(x, "_vmtl_nhwc", None)
    if st is not None and st.shape[0] == x.shape[0] and tuple(st.shape[1:3]) == tuple(x.shape[2:]) and not x.requires_grad:
        return st  # produced by hwc_to_model_input: already the internal storage, no relayout
    return _ToNHWC.apply(x)


def hwc_to_model_input(x_hwc, scale: float = 1.0):
    """(B,H,W,C) device tensor in dataset sample layout -> the reference's (B,C,H,W) input tensor, backed by the
    model's internal NHWC storage (zero pad channels) which to_nhwc() picks up without a second relayout."""
    x_hwc = _req(x_hwc, "img")
    B, H, W, C = x_hwc.shape
    Cs = ceil4(C)
    st = _empty((B, H, W, Cs), x_hwc)
    _k("vmtl_hwc_to_nhwc_pad", x=x_hwc, y=st, P=B * H * W, C=C, Cs=Cs, scale=scale)
    view = st[..., :C].permute(0, 3, 1, 2)
    view._vmtl_nhwc = st
    return view



def _req_dtype(t: torch.Tensor, name: str, dtypes: tuple) -> torch.Tensor:
    """_req for the non-float inputs of the input side: a device tensor of one of `dtypes`, contiguous, 16-byte aligned
    (the kernels read it in 16-byte granules; a misaligned view is copied)."""
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the vmtl hot path only runs as HIP kernels on an MI355X "
            "(there is deliberately no CPU fallback)"
        )
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be one of {[str(d) for d in dtypes]}, got {t.dtype}")
    t = t if t.is_contiguous() else t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


DEPTH_DTYPES = {torch.uint16: 0, torch.int32: 1}  # VMTL_DEPTH_U16 / VMTL_DEPTH_I32


def nyuv2_resize(img, mask, depth, size, max_depth: float = 10.0):
    """The reference's NYUv2 sample transform (cfg.py:144-155: ToTensor + Resize(size, antialias=True)) and loader value
    rules (nyuv2.py:100-141) on a raw device batch, as two launches (csrc/resize.hip).

    img uint8 (B,Hi,Wi,3), mask uint8 (B,Hi,Wi), depth uint16 or int32 (B,Hi,Wi) -> img (B,3,Ho,Wo) float32 (a
    channels-last view of the model's NHWC input storage, as hwc_to_model_input returns it), mask (B,Ho,Wo) int64,
    depth (B,Ho,Wo,1) float32."""
    img = _req_dtype(img, "img", (torch.uint8,))
    mask = _req_dtype(mask, "mask", (torch.uint8,))
    depth = _req_dtype(depth, "depth", tuple(DEPTH_DTYPES))
    if img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError(f"nyuv2_resize: img must be (B, H, W, 3), got {tuple(img.shape)}")
    B, Hi, Wi, _ = img.shape
    if tuple(mask.shape) != (B, Hi, Wi) or tuple(depth.shape) != (B, Hi, Wi):
        raise ValueError(f"nyuv2_resize: mask {tuple(mask.shape)} and depth {tuple(depth.shape)} must be {(B, Hi, Wi)}")
    Ho, Wo = (int(v) for v in size)
    code = DEPTH_DTYPES[depth.dtype]
    nparts = lib().raw("vmtl_nyuv2_resize_parts")(B, Hi, Wi, Ho, Wo, code)
    if nparts < 0:
        lib()._raise("vmtl_nyuv2_resize_parts", nparts)
    st = _empty((B, Ho, Wo, 4), img)
    m = torch.empty((B, Ho, Wo), dtype=torch.int64, device=img.device)
    d = _empty((B, Ho, Wo, 1), img)
    part = _empty((nparts,), img)
    _k("vmtl_nyuv2_resize", img=img, mask=mask, depth=depth, depth_dtype=code, img_out=st, mask_out=m, depth_out=d,
       part=part, B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, max_depth=float(max_depth))
    view = st[..., :3].permute(0, 3, 1, 2)
    view._vmtl_nhwc = st
    return view, m, d


AUGMENT_MAX_SCALES = 8  # csrc/augment.hip AUG_MAX_S


def augment_draw(state, params, crop_hw, H: int, W: int, p_flip: float = 0.5, brightness: float = 0.0):
    """One launch (csrc/augment.hip): fill params int32 (B, 8) = {scale_idx, top, left, flip, gain bits, 0, 0, 0} from
    the device state int64 (2,) = {seed, counter} and advance the counter on the device.  crop_hw int32 (S, 2): the crop
    size per scale.  The generator is restated on the host by data.augment_params_host."""
    for name, v, dt in (("state", state, torch.int64), ("params", params, torch.int32)):
        if _req_dtype(v, name, (dt,)) is not v:  # both are written: a contiguous, aligned copy would take the result
            raise ValueError(f"augment_draw: {name} must be contiguous and 16-byte aligned")
    crop_hw = _req_dtype(crop_hw, "crop_hw", (torch.int32,))
    if state.numel() != 2 or params.dim() != 2 or params.shape[1] != 8 or crop_hw.dim() != 2 or crop_hw.shape[1] != 2:
        raise ValueError(f"augment_draw: state (2,), params (B, 8), crop_hw (S, 2) expected, got {tuple(state.shape)}, "
                         f"{tuple(params.shape)}, {tuple(crop_hw.shape)}")
    _k("vmtl_augment_draw", state=state, params=params, crop_hw=crop_hw, B=params.shape[0], H=int(H), W=int(W),
       S=crop_hw.shape[0], flip_threshold=int(round(float(p_flip) * (1 << 24))), brightness=float(brightness))
    return params


def augment_apply(img, mask, depth, params, scales, crop_hw):
    """Random scale-crop + flip (+ gain) of one batch by the rows of `params`, as one launch (csrc/augment.hip).

    img: a (B,3,H,W) view over the model's NHWC input storage (hwc_to_model_input, nyuv2_resize), a (B,H,W,3) tensor in
    dataset sample layout, or a plain (B,3,H,W) tensor (re-laid first by the existing kernel); mask int64 (B,H,W); depth
    float32 (B,H,W,1) or (B,H,W); params int32 (B,8); scales float32 (S,); crop_hw int32 (S,2).  Returns (img, mask, depth)
    in the model's input contract: img a (B,3,H,W) view of a NEW NHWC storage (pad lane 0), mask int64 (B,H,W), depth
    (B,H,W,1)."""
    st = getattr(img, "_vmtl_nhwc", None)
    if (st is not None and img.dim() == 4 and st.dim() == 4 and st.shape[-1] == 4 and st.shape[0] == img.shape[0]
            and tuple(st.shape[1:3]) == tuple(img.shape[2:])):
        src, ld = _req(st, "img"), 4
    elif img.dim() == 4 and img.shape[-1] == 3 and img.shape[1] != 3:
        src, ld = _req(img, "img"), 3
    elif img.dim() == 4 and img.shape[1] == 3:
        src, ld = to_nhwc(_req(img, "img")), 4
    else:
        raise ValueError(f"augment_apply: img must be (B, 3, H, W) or (B, H, W, 3), got {tuple(img.shape)}")
    B, H, W, _ = src.shape
    mask = _req_dtype(mask, "mask", (torch.int64,))
    depth = _req(depth, "depth")
    params = _req_dtype(params, "params", (torch.int32,))
    scales = _req(scales, "scales")
    crop_hw = _req_dtype(crop_hw, "crop_hw", (torch.int32,))
    if tuple(mask.shape) != (B, H, W) or tuple(depth.shape) not in ((B, H, W, 1), (B, H, W)):
        raise ValueError(f"augment_apply: mask {tuple(mask.shape)} must be {(B, H, W)} and depth {tuple(depth.shape)} "
                         f"{(B, H, W, 1)}")
    S = scales.numel()
    if (tuple(params.shape) != (B, 8) or scales.dim() != 1 or tuple(crop_hw.shape) != (S, 2)
            or not 1 <= S <= AUGMENT_MAX_SCALES):
        raise ValueError(f"augment_apply: params {(B, 8)}, scales (S,), crop_hw (S, 2) with 1 <= S <= "
                         f"{AUGMENT_MAX_SCALES} expected, got {tuple(params.shape)}, {tuple(scales.shape)}, "
                         f"{tuple(crop_hw.shape)}")
    out = _empty((B, H, W, 4), src)
    m = torch.empty((B, H, W), dtype=torch.int64, device=src.device)
    d = _empty((B, H, W, 1), src)
    _k("vmtl_augment_apply", img=src, ld=ld, mask=mask, depth=depth, params=params, scales=scales, crop_hw=crop_hw,
       img_out=out, mask_out=m, depth_out=d, B=B, H=H, W=W, S=S)
    view = out[..., :3].permute(0, 3, 1, 2)
    view._vmtl_nhwc = out
    return view, m, d


TTA_MAX_CLASSES = 32  # csrc/tta.hip TTA_MAX_C
TTA_MODES = {"prob": 0, "logit": 1}  # include/vmtl.h VMTL_TTA_PROB / VMTL_TTA_LOGIT


def _tta_size(size, what):
    if (not isinstance(size, (tuple, list)) or len(size) != 2
            or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in size)):
        raise ValueError(f"{what} must be two positive ints (H, W), got {size!r}")
    return int(size[0]), int(size[1])


def _tta_mode(mode, what):
    if mode not in TTA_MODES:
        raise ValueError(f"{what}: merge must be one of {tuple(TTA_MODES)}, got {mode!r}")
    return TTA_MODES[mode]


def _tta_classes(C, what):
    if not 1 <= C <= TTA_MAX_CLASSES:
        raise ValueError(f"{what}: 1 <= C <= {TTA_MAX_CLASSES} classes are supported, got {C}")


def tta_view(img, size, flip=False):
    """One view of an image batch for test-time augmentation, as one launch (csrc/tta.hip): bilinear resize to `size`
    (F.interpolate, align_corners=False, no antialias), then mirrored in x when `flip` is set.

    img: what augment_apply takes - a (B,3,H,W) view over the model's NHWC input storage, a (B,H,W,3) tensor in dataset
    sample layout, or a plain (B,3,H,W) tensor (re-laid first).  Returns the (B,3,Ho,Wo) view of a NEW NHWC storage (pad
    lane 0), which the model picks up without a relayout."""
    Ho, Wo = _tta_size(size, "tta_view: size")
    st = getattr(img, "_vmtl_nhwc", None)
    if (st is not None and img.dim() == 4 and st.dim() == 4 and st.shape[-1] == 4 and st.shape[0] == img.shape[0]
            and tuple(st.shape[1:3]) == tuple(img.shape[2:])):
        src, ld = _req(st, "img"), 4
    elif img.dim() == 4 and img.shape[-1] == 3 and img.shape[1] != 3:
        src, ld = _req(img, "img"), 3
    elif img.dim() == 4 and img.shape[1] == 3:
        src, ld = to_nhwc(_req(img, "img")), 4
    else:
        raise ValueError(f"tta_view: img must be (B, 3, H, W) or (B, H, W, 3), got {tuple(img.shape)}")
    B, H, W, _ = src.shape
    out = _empty((B, Ho, Wo, 4), src)
    _k("vmtl_tta_view", img=src, ld=ld, out=out, B=B, H=H, W=W, Ho=Ho, Wo=Wo, flip=int(bool(flip)))
    view = out[..., :3].permute(0, 3, 1, 2)
    view._vmtl_nhwc = out
    return view


def tta_accumulate(logits, depth_logits, acc, acc_depth, flip=False, weight=1.0, depth_gain=1.0, merge="prob",
                   first=False):
    """Merge one view into the accumulators, as one launch (csrc/tta.hip): logits (B,C,h,w) and depth_logits (B,1,h,w)
    (or None, with acc_depth None) as the model returns them for the view are un-mirrored when `flip` is set, resampled
    to the base size and added to acc (B,C,H,W) - weight * softmax ("prob") or weight * logits ("logit") - and to
    acc_depth (B,H,W) - weight * depth_gain * bilinear(sigmoid(depth_logits)).  first=True assigns instead of adding
    (the accumulators need no zeroing).  The accumulators are written in place and returned."""
    mode = _tta_mode(merge, "tta_accumulate")
    logits = _req(logits, "logits")
    if _req(acc, "acc") is not acc:
        raise ValueError("tta_accumulate: acc is written in place and must be contiguous")
    if logits.dim() != 4 or acc.dim() != 4 or acc.shape[:2] != logits.shape[:2]:
        raise ValueError(f"tta_accumulate: logits (B, C, h, w) and acc (B, C, H, W) expected, got {tuple(logits.shape)} "
                         f"and {tuple(acc.shape)}")
    B, C, h, w = logits.shape
    H, W = acc.shape[2:]
    _tta_classes(C, "tta_accumulate")
    if (depth_logits is None) != (acc_depth is None):
        raise ValueError("tta_accumulate: depth_logits and acc_depth are given together or not at all")
    if depth_logits is not None:
        depth_logits = _req(depth_logits, "depth_logits")
        if _req(acc_depth, "acc_depth") is not acc_depth:
            raise ValueError("tta_accumulate: acc_depth is written in place and must be contiguous")
        if tuple(depth_logits.shape) != (B, 1, h, w) or acc_depth.numel() != B * H * W:
            raise ValueError(f"tta_accumulate: depth_logits {(B, 1, h, w)} and acc_depth {(B, H, W)} expected, got "
                             f"{tuple(depth_logits.shape)} and {tuple(acc_depth.shape)}")
    _k("vmtl_tta_accumulate", logits=logits, depth_logits=depth_logits, acc=acc, acc_depth=acc_depth, B=B, C=C, h=h, w=w,
       H=H, W=W, flip=int(bool(flip)), weight=float(weight), depth_gain=float(depth_gain), mode=mode, first=int(bool(first)))
    return acc, acc_depth


def tta_finish(acc, acc_depth, inv_weight, size=None, merge="prob", confidence=False):
    """Predictions from the merged map at any output size, as one launch (csrc/tta.hip): acc (B,C,H,W) and acc_depth
    (B,H,W) or None are resampled to `size` (default: their own) channel by channel and reduced on the fly, so the
    (B,C,Ho,Wo) map never exists.  Returns (segm int64 (B,Ho,Wo), depth float32 (B,Ho,Wo) = inv_weight *
    bilinear(acc_depth) or None, confidence float32 (B,Ho,Wo) - the largest softmax probability of the merged map - or
    None).  merge: the mode the accumulator was filled with."""
    mode = _tta_mode(merge, "tta_finish")
    acc = _req(acc, "acc")
    if acc.dim() != 4:
        raise ValueError(f"tta_finish: acc must be (B, C, H, W), got {tuple(acc.shape)}")
    B, C, H, W = acc.shape
    _tta_classes(C, "tta_finish")
    Ho, Wo = (H, W) if size is None else _tta_size(size, "tta_finish: size")
    inv_weight = float(inv_weight)
    if not (inv_weight > 0 and math.isfinite(inv_weight)):
        raise ValueError(f"tta_finish: inv_weight must be a finite float > 0, got {inv_weight!r}")
    depth = None
    if acc_depth is not None:
        acc_depth = _req(acc_depth, "acc_depth")
        if acc_depth.numel() != B * H * W:
            raise ValueError(f"tta_finish: acc_depth must be {(B, H, W)}, got {tuple(acc_depth.shape)}")
        depth = _empty((B, Ho, Wo), acc)
    segm = torch.empty((B, Ho, Wo), dtype=torch.int64, device=acc.device)
    conf = _empty((B, Ho, Wo), acc) if confidence else None
    _k("vmtl_tta_finish", acc=acc, acc_depth=acc_depth, inv_weight=inv_weight, segm=segm, depth=depth, confidence=conf,
       B=B, C=C, H=H, W=W, Ho=Ho, Wo=Wo, mode=mode)
    return segm, depth, conf


class _ToNCHW(torch.autograd.Function):
    """internal [B,H,W,Cs] -> (B,C,H,W) contiguous, the reference's output layout."""

    @staticmethod
    def forward(ctx, x, C):
        x = _req(x, "x")
        B, H, W, Cs = x.shape
        y = _empty((B, C, H, W), x)
        _k("vmtl_nhwc_to_nchw", x=x, y=y, B=B, C=C, HW=H * W, Cs=Cs)
        ctx.Cs = Cs
        _remember_mode(ctx)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = dy.shape
        ld = ctx.Cs
        _restore_mode(ctx)  # first backward node of a (task) network
        if (dy.is_cuda and dy.dtype == torch.float32 and dy.stride() == (H * W * ld, 1, W * ld, ld) and dy.storage_offset() == 0
                and dy.untyped_storage().nbytes() == 4 * B * H * W * ld and getattr(dy, "_vmtl_nhwc", None) is not None):
            # the cross-entropy backward already wrote this gradient as NHWC rows of exactly our width, pad lanes zero
            return torch.as_strided(dy, (B, H, W, ld), (H * W * ld, W * ld, ld, 1)), None
        dy = _req(dy, "dy")
        dx = _empty((B, H, W, ctx.Cs), dy)
        _k("vmtl_nchw_to_nhwc", x=dy, y=dx, B=B, C=C, HW=H * W, Cs=ctx.Cs, Cw=ctx.Cs)
        return dx, None


def to_nchw(x, C):
    return _ToNCHW.apply(x, C)


# ----------------------------------------------------------------------------- narrow full-resolution tail
def conv3x3_small_supported(Cs: int, Nw: int) -> bool:
    return bool(lib().raw("vmtl_conv3x3_small_supported")(Cs, Nw))


def _small(x, wp, y, B, H, W, Cs, ldy, Nw, Cout, flop, x2=None, pa=None, pb=None, pc=None, act_in=ACT_NONE, a_out=None,
           bias=None, yb=None, Ca=0, stats=None, ep_mode=0, ez=None):
    """One vmtl_conv3x3_small launch (csrc/conv_small.hip); ez = (x, mean, invstd, gamma, beta, act) for ep_mode 2."""
    _k("vmtl_conv3x3_small", _flop=flop, x=x, x2=x2, pa=pa, pb=pb, pc=pc, act_in=act_in, a_out=a_out, wp=wp, bias=bias,
       y=y, yb=yb, Ca=Ca, stats=stats, ep_mode=ep_mode, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Cout, **_ez_kw(ez))


class _DecoderTail(torch.autograd.Function):
    """relu(BN1(x1)) -> conv2 3x3 -> relu(BN2(.)) -> {head a, head b} 3x3 (+bias), returned as the reference's two
    NCHW maps: the narrow full-resolution tail of `basic` (smp DecoderBlock conv2 of the last decoder block via
    reference utils/model_utils.py:25-34, segm_head / depth_head of models/basic_model.py:30-51) on
    vmtl_conv3x3_small.  x1 is the RAW output of the block's first conv (with its BatchNorm partial rows stats1):
    both normalise+ReLU passes run as the consumer conv's prologue, both BatchNorm-backward reductions as the
    producing data-gradient's epilogue, BN2's backward-apply as the prologue of conv2's data gradient."""

    @staticmethod
    def forward(ctx, x1, stats1, rpb1, g1, b1, rm1, rv1, nbt1, w2, g2, b2, rm2, rv2, nbt2, wa, ba, wb, bb, cfg):
        tr1, mom1, eps1, tr2, mom2, eps2 = cfg
        x1, w2, wa, wb = _req(x1, "x1"), _req(w2, "conv2 weight"), _req(wa, "head a weight"), _req(wb, "head b weight")
        B, H, W, Cs1 = x1.shape
        C2, C1 = w2.shape[0], w2.shape[1]
        Ca, Cb = wa.shape[0], wb.shape[0]
        N = Ca + Cb
        ldy2, ldyh = ceil4(C2), ceil4(N)
        if (ceil4(C1) != Cs1 or tuple(w2.shape[2:]) != (3, 3) or tuple(wa.shape[1:]) != (C2, 3, 3)
                or tuple(wb.shape[1:]) != (C2, 3, 3) or ba is None or bb is None):
            raise ValueError("decoder_tail: conv2 must be 3x3 over x1's channels and both heads 3x3 over conv2's, with biases")
        if not (conv3x3_small_supported(Cs1, C2) and conv3x3_small_supported(ldy2, N) and conv3x3_small_supported(ldyh, C2)
                and H % 4 == 0 and W % 32 == 0):
            raise ValueError("decoder_tail: shape not covered by vmtl_conv3x3_small (use decoder_tail_supported())")
        need_bwd = any(ctx.needs_input_grad)
        M = B * H * W
        tiles = lib().raw("vmtl_conv3x3_small_stat_rows")(B, H, W)  # statistics rows ...
        rpb = lib().raw("vmtl_conv3x3_small_stat_block")(B, H, W)   # ... of this many pixels each
        mean1, invstd1, pa1, pc1 = _bn_stats(x1, stats1, rpb1, rm1, rv1, nbt1, C1, tr1, mom1, eps1, (g1, b1))
        wp2 = packs.get(w2, "fwd", Layout.fwd(C2, C1, 9, Cs1))
        a1 = _empty(x1.shape, x1) if need_bwd else None
        x2 = _empty((B, H, W, ldy2), x1)
        stats2 = _empty((tiles, 2, ldy2), x1) if tr2 else None
        _small(x1, wp2, x2, B, H, W, Cs1, ldy2, C2, C2, 2.0 * M * C2 * 9 * C1, pa=pa1, pc=pc1, act_in=ACT_RELU, a_out=a1,
               stats=stats2, ep_mode=1 if tr2 else 0)
        mean2, invstd2, pa2, pc2 = _bn_stats(x2, stats2, rpb, rm2, rv2, nbt2, C2, tr2, mom2, eps2, (g2, b2))
        # both heads as ONE GEMM operand / bias vector, kept packed by the step's batched packing launch
        wph = packs.shared(wa, "heads_fwd", (N, 9 * ldy2))
        packs.get(wa, "heads_fwd", Layout.fwd(Ca, C2, 9, ldy2), out=wph[:Ca])
        packs.get(wb, "heads_fwd", Layout.fwd(Cb, C2, 9, ldy2), out=wph[Ca:])
        bias = packs.shared(wa, "heads_bias", (N,))
        packs.get(ba, "heads_bias", Layout.vec(Ca), out=bias[:Ca])
        packs.get(bb, "heads_bias", Layout.vec(Cb), out=bias[Ca:])
        a2 = _empty(x2.shape, x1) if need_bwd else None
        oa, ob = _empty((B, Ca, H, W), x1), _empty((B, Cb, H, W), x1)
        _small(x2, wph, oa, B, H, W, ldy2, ldyh, N, N, 2.0 * M * N * 9 * C2, pa=pa2, pc=pc2, act_in=ACT_RELU, a_out=a2,
               bias=bias, yb=ob, Ca=Ca)
        ctx.save_for_backward(x1, a1, x2, a2, mean1, invstd1, mean2, invstd2, g1, b1, g2, b2, w2, wa, wb)
        ctx.cfg = (tr1, tr2)
        ctx.prec = conv_prec_code()  # the dense weight gradients' (its convolutions run on the fp32 halo-tile kernel)
        ctx.slots = tuple(_slot(t) for t in (g1, b1, w2, g2, b2, wa, ba, wb, bb))
        _remember_mode(ctx)
        return oa, ob

    @staticmethod
    def backward(ctx, ga, gb):
        x1, a1, x2, a2, mean1, invstd1, mean2, invstd2, g1, b1, g2, b2, w2, wa, wb = ctx.saved_tensors
        tr1, tr2 = ctx.cfg
        _restore_mode(ctx)
        sg1, sb1, sw2, sg2, sb2, swa, sba, swb, sbb = ctx.slots
        B, H, W, Cs1 = x1.shape
        C2, C1 = w2.shape[0], w2.shape[1]
        Ca, Cb = wa.shape[0], wb.shape[0]
        N = Ca + Cb
        ldy2, ldyh = ceil4(C2), ceil4(N)
        M = B * H * W
        tiles = lib().raw("vmtl_conv3x3_small_stat_rows")(B, H, W)
        gb = torch.zeros((B, Cb, H, W), device=x1.device) if gb is None else _req(gb, "grad b")
        # head a's gradient may already sit in NHWC storage of the right width (the cross-entropy backward writes it so)
        dy = None
        if ga is not None and ga.stride() == (H * W * ldyh, 1, W * ldyh, ldyh) and ga.storage_offset() == 0 \
                and ga.dtype == torch.float32 and ga.untyped_storage().nbytes() == 4 * B * H * W * ldyh:
            dy = torch.as_strided(ga, (B, H, W, ldyh), (H * W * ldyh, W * ldyh, ldyh, 1))
        if dy is None:
            ga = torch.zeros((B, Ca, H, W), device=x1.device) if ga is None else _req(ga, "grad a")
            dy = _empty((B, H, W, ldyh), x1)
            _k("vmtl_nchw_to_nhwc", x=ga, y=dy.view(-1), B=B, C=Ca, HW=H * W, Cs=ldyh, Cw=Ca)
        dyf = dy.view(-1)
        _k("vmtl_nchw_to_nhwc", x=gb, y=dyf[Ca:], B=B, C=Cb, HW=H * W, Cs=ldyh, Cw=ldyh - Ca)  # also zeroes pad lanes
        stamp("main tail heads")
        fork = side.mark()
        # heads' data gradient; epilogue = ReLU + BatchNorm-2 backward reduction (dz2 and its per-tile column sums)
        wb_ref = weakref.ref(wb)  # the cache entry must not keep a parameter (and through it the whole model) alive

        def pack_heads_dgrad(w, dst):  # both heads' flipped weights as ONE dgrad operand [C2][9][ldyh]
            pack(w, *Layout.dgrad(Ca, C2, 9, ldyh), out=dst)
            _k("vmtl_pack_weights_slice", src=wb_ref(), dst=dst.view(-1)[Ca:], R0=C2, T=9, C=Cb, group=ldyh, sr0=9, st=1,
               sc=C2 * 9, flip=1)

        wd = packs.get_custom(wa, "heads_dgrad", (C2, 9 * ldyh), pack_heads_dgrad, deps=(wb,))
        dz2, part2 = _empty((B, H, W, ldy2), x1), _empty((tiles, 2, ldy2), x1)
        _small(dy, wd, dz2, B, H, W, ldyh, ldy2, C2, C2, 2.0 * M * C2 * 9 * N, stats=part2, ep_mode=2,
               ez=(x2, mean2, invstd2, g2, b2, ACT_RELU))
        with side.branch(all(s is not None for s in (swa, sba, swb, sbb)), M, fork, a2, dy):
            dwa, dba, dwb, dbb = _wgrad_two_heads(
                a2, dy, ConvGeom(B, H, W, ldy2, H, W, ldyh, 3, 3, 1, 1), Layout.fwd(Ca, C2, 9, ldy2),
                Layout.fwd(Cb, C2, 9, ldy2), wa, wb, (swa, sba, swb, sbb), 2.0 * M * N * 9 * C2, ctx.prec)
            stamp("side tail heads")
        # BatchNorm-2 parameter gradients + its backward-apply as affine coefficients of (dz2, x2)
        dbeta2, dgamma2 = _grad_buf((C2,), sb2, x1), _grad_buf((C2,), sg2, x1)
        cA, cB, cC = _empty((ldy2,), x1), _empty((ldy2,), x1), _empty((ldy2,), x1)
        _k("vmtl_bn_bwd_finalize", partial=part2, nblk=tiles, M=M, C=C2, Cs=ldy2, sum_dz=dbeta2, sum_dzx=dgamma2, mean=mean2,
           invstd=invstd2, gamma=g2, training=1 if tr2 else 0, coef_a=cA, coef_b=cB, coef_c=cC)
        stamp("main tail conv2")
        # conv2's data gradient: prologue dx2 = cA*dz2 + cB*x2 + cC (kept in dx2 for the weight gradient),
        # epilogue = ReLU + BatchNorm-1 backward reduction
        wd2 = packs.get(w2, "dgrad", Layout.dgrad(C2, C1, 9, ldy2))
        dx2 = _empty(x2.shape, x1)
        dz1, part1 = _empty(x1.shape, x1), _empty((tiles, 2, Cs1), x1)
        _small(dz2, wd2, dz1, B, H, W, ldy2, Cs1, C1, C1, 2.0 * M * C1 * 9 * C2, x2=x2, pa=cA, pb=cB, pc=cC, a_out=dx2,
               stats=part1, ep_mode=2, ez=(x1, mean1, invstd1, g1, b1, ACT_RELU))
        fork = side.mark()  # AFTER the launch above: the weight gradient reads the dx2 it wrote
        dx1, dgamma1, dbeta1 = _bn_bwd_tail(part1, tiles, x1, dz1, mean1, invstd1, g1, C1, tr1, (sg1, sb1),
                                            ctx.needs_input_grad[0])
        with side.branch(sw2 is not None, M, fork, a1, dx2):
            dw2 = _grad_buf(w2.shape, sw2, x1)
            _wgrad_into(a1, dx2, ConvGeom(B, H, W, Cs1, H, W, ldy2, 3, 3, 1, 1), Layout.fwd(C2, C1, 9, Cs1), dw2,
                        2.0 * M * C2 * 9 * C1, ctx.prec)
            stamp("side tail conv2")
        return (dx1, None, None, dgamma1, dbeta1, None, None, None, _grad_ret(dw2, sw2),
                _grad_ret(dgamma2, sg2), _grad_ret(dbeta2, sb2), None, None, None, dwa, dba, dwb, dbb, None)


def decoder_tail_supported(x1_shape, C1, C2, N) -> bool:
    B, H, W, Cs1 = x1_shape
    return (ceil4(C1) == Cs1 and conv3x3_small_supported(Cs1, C2) and conv3x3_small_supported(ceil4(C2), N)
            and conv3x3_small_supported(ceil4(N), C2) and H % 4 == 0 and W % 32 == 0
            and os.environ.get("VMTL_SMALL_TAIL", "1") != "0")


def decoder_tail(x1, stats1, rpb1, bn1, conv2_weight, bn2, wa, ba, wb, bb):
    """(head_a, head_b) NCHW = heads(relu(bn2(conv2(relu(bn1(x1)))))); bn1 / bn2 are nn.BatchNorm2d parameter
    containers, x1 the raw conv output feeding bn1 (stats1 = its conv-epilogue partial rows of rpb1 pixels, or None)."""
    (t1, mode1), (t2, mode2) = _bn_args(bn1), _bn_args(bn2)
    return _DecoderTail.apply(x1, stats1, rpb1, *t1, conv2_weight, *t2, wa, ba, wb, bb, (*mode1, *mode2))


def _copy_vec(src, dst, n):
    """dst[:n] = src[:n] for small per-channel vectors (the pack kernel in its degenerate 1x1x1 form)."""
    pack(src, *Layout.vec(n), out=dst)


class _DualHead(torch.autograd.Function):
    """Two KxK heads reading the same feature map (reference models/basic_model.py:30-51: segm_head and
    depth_head) as ONE implicit GEMM with N = Ca + Cb output channels.  Parameters stay separate torch
    tensors; outputs are the two contiguous NCHW maps the reference returns."""

    @staticmethod
    def forward(ctx, x, wa, ba, wb, bb, pad, surgery=None):
        x, wa, wb = _req(x, "x"), _req(wa, "weight a"), _req(wb, "weight b")
        B, H, W, Cs = x.shape
        Ca, Cin, KH, KW = wa.shape
        Cb = wb.shape[0]
        if tuple(wb.shape[1:]) != (Cin, KH, KW) or ceil4(Cin) != Cs or ba is None or bb is None:
            raise ValueError("dual_head: both heads must share input channels / kernel size and have a bias")
        ctx.surgery = surgery
        N, KK = Ca + Cb, KH * KW
        ldy, Ktot = ceil4(N), KK * Cs
        wp = _empty((N, Ktot), x)
        pack(wa, *Layout.fwd(Ca, Cin, KK, Cs), out=wp[:Ca])
        pack(wb, *Layout.fwd(Cb, Cin, KK, Cs), out=wp[Ca:])
        bias = _empty((N,), x)
        _copy_vec(ba, bias, Ca)
        _copy_vec(bb, bias[Ca:], Cb)
        y = _empty((B, H, W, ldy), x)
        prec = ctx.prec = conv_prec_code()
        pw_prec = ctx.pw_prec = pw_prec_code()  # 1x1 heads take the pointwise route
        _conv_launch(x, wp, bias, y, ConvGeom(B, H, W, Cs, H, W, ldy, KH, KW, 1, pad), Cout=N, cin=Cin, prec=prec,
                     pw_prec=pw_prec)
        oa, ob = _empty((B, Ca, H, W), x), _empty((B, Cb, H, W), x)
        yf = y.view(-1)
        _k("vmtl_nhwc_to_nchw", x=yf, y=oa, B=B, C=Ca, HW=H * W, Cs=ldy)
        _k("vmtl_nhwc_to_nchw", x=yf[Ca:], y=ob, B=B, C=Cb, HW=H * W, Cs=ldy)
        ctx.save_for_backward(x, wa, wb)
        ctx.cfg = (pad, ldy)
        ctx.slots = (_slot(wa), _slot(ba), _slot(wb), _slot(bb))
        _remember_mode(ctx)
        return oa, ob

    @staticmethod
    def backward(ctx, ga, gb):
        x, wa, wb = ctx.saved_tensors
        pad, ldy = ctx.cfg
        _restore_mode(ctx)
        B, H, W, Cs = x.shape
        Ca, Cin, KH, KW = wa.shape
        Cb = wb.shape[0]
        N, KK = Ca + Cb, KH * KW
        g = ConvGeom(B, H, W, Cs, H, W, ldy, KH, KW, 1, pad)
        ga = torch.zeros((B, Ca, H, W), device=x.device) if ga is None else _req(ga, "grad a")
        gb = torch.zeros((B, Cb, H, W), device=x.device) if gb is None else _req(gb, "grad b")
        dy = _empty((B, H, W, ldy), x)
        dyf = dy.view(-1)
        _k("vmtl_nchw_to_nhwc", x=ga, y=dyf, B=B, C=Ca, HW=H * W, Cs=ldy, Cw=Ca)
        _k("vmtl_nchw_to_nhwc", x=gb, y=dyf[Ca:], B=B, C=Cb, HW=H * W, Cs=ldy, Cw=ldy - Ca)  # also zeroes pad lanes
        dx = None
        fork = side.mark()
        if ctx.needs_input_grad[0] and ctx.surgery is not None:
            # the two heads' data gradients kept apart, still ONE launch that reads dy once: a block-diagonal operand of
            # Cs + Cin rows - rows [0, Cin) carry head a's lanes co < Ca, rows [Cs, Cs + Cin) head b's lanes [Ca, Ca + Cb),
            # every other lane and row is zero - whose output is the interleaved map [M][g_a | g_b], 2 * Cs wide
            # (the buffer is the surgery object's, zeroed once: only the two heads' lanes change from step to step)
            wd = ctx.surgery.head_operand(Cs + Cin, KK * ldy, x)
            pack(wa, *Layout.dgrad(Ca, Cin, KK, ldy), out=wd[:Cin])
            _k("vmtl_pack_weights_slice", src=wb, dst=wd[Cs:].view(-1)[Ca:], R0=Cin, T=KK, C=Cb, group=ldy, sr0=KK, st=1,
               sc=Cin * KK, flip=1)
            gab = _empty((B, H, W, 2 * Cs), x)
            _conv_launch(dy, wd, None, gab, g.dgrad()._replace(ldy=2 * Cs), Cout=Cs + Cin, cin=N, prec=ctx.prec,
                         pw_prec=ctx.pw_prec)
            dx = _empty((B, H, W, Cs), x)
            ctx.surgery.apply(gab, dx, B * H * W, Cs)
        elif ctx.needs_input_grad[0]:
            # one tap-flipped, transposed operand [ci][tap'][co]: head a fills co < Ca and zeroes the rest of
            # every ldy-wide group, head b then fills co in [Ca, Ca+Cb)
            wd = pack(wa, *Layout.dgrad(Ca, Cin, KK, ldy))
            _k("vmtl_pack_weights_slice", src=wb, dst=wd.view(-1)[Ca:], R0=Cin, T=KK, C=Cb, group=ldy, sr0=KK, st=1,
               sc=Cin * KK, flip=1)
            dx = _empty((B, H, W, Cs), x)
            _conv_launch(dy, wd, None, dx, g.dgrad(), Cout=Cin, cin=N, prec=ctx.prec, pw_prec=ctx.pw_prec)
        with side.branch(all(s is not None for s in ctx.slots), B * H * W, fork, x, dy):
            dwa, dba, dwb, dbb = _wgrad_two_heads(x, dy, g, Layout.fwd(Ca, Cin, KK, Cs), Layout.fwd(Cb, Cin, KK, Cs), wa, wb,
                                                  ctx.slots, 2.0 * B * H * W * N * KK * Cin, ctx.prec)
            stamp("side head")
        return dx, dwa, dba, dwb, dbb, None, None


def dual_head(x, wa, ba, wb, bb, pad=1, surgery=None):
    """surgery (opt-in, a surgery.GradSurgery): the backward hands x the combination alpha * g_a + beta * g_b of the two
    heads' data gradients that the object's method derives from their Gram matrix, instead of their sum.  The forward
    and the heads' own parameter gradients are those of the plain node."""
    return _DualHead.apply(x, wa, ba, wb, bb, pad, surgery)


class _Sigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        y = _empty(x.shape, x)
        _k("vmtl_eltwise", a=x, b=None, y=y, mode=1, total=x.numel())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _req(dy, "dy")
        dx = _empty(y.shape, y)
        _k("vmtl_eltwise", a=y, b=dy, y=dx, mode=2, total=y.numel())
        return dx


def sigmoid(x):
    return _Sigmoid.apply(x)


class _Fork(torch.autograd.Function):
    """n handles on one tensor for its n consumers (a block's residual branch and its first conv, an encoder feature and
    the next stage; MTAN's shared features feed the shared path AND both task attention modules: reference
    models/mtan_model.py:364-399).  Autograd would sum the gradients with n-1 ATen kernels; here the sum is ONE launch
    of this library (vmtl_add_n, up to 4 operands per launch), so the step runs no kernel the C ABI does not export."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)  # an unused handle contributes None, not a zero tensor to add
        return tuple(x.detach() for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [_req(g, "grad") for g in gs if g is not None]
        if not gs:
            return None, None
        while len(gs) > 1:
            k = min(4, len(gs))
            ops4 = gs[:k] + [None] * (4 - k)
            out = _empty(gs[0].shape, gs[0])
            _k("vmtl_add_n", a=ops4[0], b=ops4[1], c=ops4[2], d=ops4[3], y=out, total=out.numel())
            gs = [out] + gs[k:]
        return gs[0], None


def fork(x, n=2):
    """n independent handles on x (gradients summed by this library's kernel)."""
    return _Fork.apply(x, n)


class _AddScalars(torch.autograd.Function):
    """wa * a + wb * b for two scalar losses (reference lit_module.py:127-129) as one launch of this library."""

    @staticmethod
    def forward(ctx, a, b, wa, wb):
        a, b = _req(a, "a"), _req(b, "b")
        out = _empty(a.shape, a)
        _k("vmtl_axpby", a=a, b=b, y=out, wa=wa, wb=wb, total=a.numel())
        ctx.w = (wa, wb)
        return out

    @staticmethod
    def backward(ctx, g):
        wa, wb = ctx.w
        g = _req(g, "grad")
        if wa == 1.0 and wb == 1.0:
            return g, g, None, None
        ga, gb = _empty(g.shape, g), _empty(g.shape, g)
        zero = g  # b operand unused when its weight is 0
        _k("vmtl_axpby", a=g, b=zero, y=ga, wa=wa, wb=0.0, total=g.numel())
        _k("vmtl_axpby", a=g, b=zero, y=gb, wa=wb, wb=0.0, total=g.numel())
        return ga, gb, None, None


def add_losses(a, b, wa=1.0, wb=1.0):
    return _AddScalars.apply(a, b, float(wa), float(wb))


BALANCE_MODES = {"uncertainty": 0, "dwa": 1, "geometric": 2}  # include/vmtl.h VMTL_BALANCE_*
BALANCE_MAX_TASKS = 4


def balance_state_doubles(T: int) -> int:
    """Length of the fp64 DWA state of T tasks (layout: include/vmtl.h)."""
    n = lib().raw("vmtl_task_balance_state_bytes")(int(T))
    if n <= 0:
        raise ValueError(f"task balancing takes 1..{BALANCE_MAX_TASKS} tasks, got {T}")
    return n // 8


class _BalanceLosses(torch.autograd.Function):
    """The T scalar task losses -> the loss that is differentiated (csrc/balance.hip), in place of add_losses' two host
    floats (reference lit_module.py:127-129): one launch per direction, and every number the kernels use - losses,
    log-variances or DWA weights, grad_out - is read by pointer, so a replayed graph follows the optimizer and the epoch
    update.  Returns (total, weights) with weights_k = d total / d L_k; the gradient of the log-variances goes straight
    into their arena slot when they have one."""

    @staticmethod
    def forward(ctx, param, state, mode, accumulate, *losses):
        T = len(losses)
        losses = [_req(l, f"losses[{k}]") for k, l in enumerate(losses)]
        l4 = losses + [None] * (BALANCE_MAX_TASKS - T)
        total, weights = _empty((), losses[0]), _empty((T,), losses[0])
        _k("vmtl_task_balance_fwd", l0=l4[0], l1=l4[1], l2=l4[2], l3=l4[3], T=T, mode=mode, param=param, state=state,
           accumulate=1 if accumulate else 0, total=total, weights=weights)
        ctx.mark_non_differentiable(weights)
        ctx.save_for_backward(weights, *losses)
        ctx.param = param  # read again by the backward kernel, in place: never a saved copy
        ctx.cfg = (mode, T)
        ctx.slot = _slot(param) if param is not None and param.requires_grad else None
        return total, weights

    @staticmethod
    def backward(ctx, g, _gw):
        weights, *losses = ctx.saved_tensors
        mode, T = ctx.cfg
        g = _req(g, "grad")
        l4 = list(losses) + [None] * (BALANCE_MAX_TASKS - T)
        gs = [_empty((), g) if ctx.needs_input_grad[4 + k] else None for k in range(T)] + [None] * (BALANCE_MAX_TASKS - T)
        dparam = _grad_buf((T,), ctx.slot, g) if ctx.needs_input_grad[0] else None
        if dparam is not None or any(x is not None for x in gs):
            _k("vmtl_task_balance_bwd", grad_out=g, weights=weights, l0=l4[0], l1=l4[1], l2=l4[2], l3=l4[3], param=ctx.param,
               mode=mode, T=T, g0=gs[0], g1=gs[1], g2=gs[2], g3=gs[3], dparam=dparam)
        return (None if dparam is None else _grad_ret(dparam, ctx.slot), None, None, None, *gs[:T])


def balance_losses(losses, mode, param=None, state=None, accumulate=False):
    """(total, weights) of the scalar task losses under `mode` ("uncertainty": param = the log-variances; "dwa": param =
    the weights, state = the fp64 accumulators of balance_state_doubles(T), accumulate = add this step to them;
    "geometric": neither - a loss that is not positive gives NaN).  See vision_mtl_amd.balancing.TaskBalancer."""
    if mode not in BALANCE_MODES:
        raise ValueError(f"balance_losses: mode must be one of {sorted(BALANCE_MODES)}, got {mode!r}")
    losses = list(losses)
    T = len(losses)
    if not 1 <= T <= BALANCE_MAX_TASKS:
        raise ValueError(f"balance_losses: 1..{BALANCE_MAX_TASKS} losses, got {T}")
    if any(l.dim() != 0 for l in losses):
        raise ValueError("balance_losses: every loss must be a 0-dim tensor")
    if mode != "geometric":
        if param is None:
            raise ValueError(f"balance_losses: mode {mode!r} needs `param` ({T} floats)")
        _req(param, "param")
        if param.numel() != T or not param.is_contiguous():
            raise ValueError(f"balance_losses: param must hold {T} contiguous floats, got shape {tuple(param.shape)}")
    else:
        param = None
    if mode == "dwa" and accumulate:
        if state is None or not state.is_cuda or state.dtype != torch.float64 or not state.is_contiguous() \
                or state.numel() != balance_state_doubles(T):
            raise ValueError(f"balance_losses: state must be {balance_state_doubles(T)} contiguous float64 on the GPU")
    else:
        state, accumulate = (state if mode == "dwa" else None), False
    return _BalanceLosses.apply(param, state, BALANCE_MODES[mode], bool(accumulate), *losses)


def dwa_epoch_update(state, weights, temperature):
    """End of a training epoch for the "dwa" mode: one launch (vmtl_dwa_epoch_update), nothing visits the host."""
    T = weights.numel()
    _req(weights, "weights")
    if not state.is_cuda or state.dtype != torch.float64 or state.numel() != balance_state_doubles(T):
        raise ValueError(f"dwa_epoch_update: state must be {balance_state_doubles(T)} float64 on the GPU")
    if not float(temperature) > 0.0:
        raise ValueError(f"dwa_epoch_update: temperature must be > 0, got {temperature}")
    _k("vmtl_dwa_epoch_update", state=state, param=weights, T=T, temperature=float(temperature))


def argmax_channels(logits):
    """argmax over dim 1 of (B,C,H,W) logits -> int64 (B,H,W); reads NCHW or channels-last strides in place."""
    if not logits.is_cuda:
        raise RuntimeError("argmax_channels: tensor is not on the GPU (no CPU fallback on the hot path)")
    B, C, H, W = logits.shape
    z = logits.detach()
    if not (z.stride(3) * W == z.stride(2) and z.dtype == torch.float32):
        z = z.float().contiguous()
    out = torch.empty((B, H, W), dtype=torch.int64, device=z.device)
    _k("vmtl_argmax_channels", z=z, out=out, B=B, HW=H * W, C=C, sb=z.stride(0), sc=z.stride(1), sp=z.stride(3))
    return out


# ----------------------------------------------------------------------------- losses
NO_IGNORE = -(1 << 63)  # include/vmtl.h VMTL_NO_IGNORE: the ignore_index of "nothing to ignore"


def _ce_weight(weight, logits):
    """The class-weight operand of the weighted cross entropy: C fp32 floats on the logits' device (None: all ones)."""
    if weight is None:
        return None
    weight = _req(weight.detach(), "weight")
    if weight.dim() != 1 or weight.numel() != logits.shape[1]:
        raise ValueError(f"cross_entropy: weight must hold one float per class ({logits.shape[1]}), got shape "
                         f"{tuple(weight.shape)}")
    if weight.device != logits.device:
        raise RuntimeError(f"cross_entropy: weight is on {weight.device}, the logits on {logits.device}")
    return weight


def _ce_dims(logits):
    """The geometry operands of the loss kernels for NCHW-contiguous logits."""
    B, C, H, W = logits.shape
    return dict(B=B, HW=H * W, C=C, sb=C * H * W, sc=H * W, sp=1)


def _ce_front(who, logits, target, weight, want_argmax, max_classes=None):
    """What the segmentation criteria's nodes check and allocate before their forward kernel:
    (logits, target, weight, geometry operands, the (B,H,W) int64 prediction buffer or None)."""
    logits = _req(logits, "logits")
    if target.dtype != torch.int64:
        raise TypeError(f"{who}: target must be int64 class indices")
    target = target.contiguous()
    B, C, H, W = logits.shape
    if tuple(target.shape) != (B, H, W):
        raise ValueError(f"{who}: target shape {tuple(target.shape)} does not match logits {(B, H, W)}")
    if max_classes is not None and not 2 <= C <= max_classes:
        raise ValueError(f"{who}: the region term takes 2 to {max_classes} classes, got {C}")
    weight = _ce_weight(weight, logits)
    pred = torch.empty((B, H, W), dtype=torch.int64, device=logits.device) if want_argmax else None
    return logits, target, weight, _ce_dims(logits), pred


def _ce_result(ctx, loss, pred):
    """loss, or (loss, prediction) when the node was asked for the argmax."""
    if pred is None:
        return loss
    ctx.mark_non_differentiable(pred)
    return loss, pred


def _ce_grad_storage(logits):
    """Where a criterion's backward kernel writes dlogits, and the stride operands that say so.  The gradient is laid out
    NHWC with room for one more head ([B][H][W][ceil4(C+1)]) and returned as its (B,C,H,W) view (_ce_grad_view): a head
    conv that consumes it (ops.decoder_tail) takes the storage as its dY operand without the NCHW -> NHWC relayout of
    this 80 MB tensor; any other consumer sees an ordinary strided tensor."""
    B, C, H, W = logits.shape
    ld = ceil4(C + 1)
    return _empty((B, H, W, ld), logits), dict(dsb=H * W * ld, dsc=1, dsp=ld)


def _ce_grad_view(st, C):
    dl = st[..., :C].permute(0, 3, 1, 2)
    dl._vmtl_nhwc = st
    return dl


class _CrossEntropy(torch.autograd.Function):
    """mean_{b,h,w} -log_softmax(logits)[target]; logits (B,C,H,W) NCHW-contiguous.

    ignore_index None (and then no weight) is that plain mean.  An int (NO_IGNORE for none) selects torch's `weight` /
    `ignore_index` form (reduction "mean"): sum_valid w[t] nll / sum_valid w[t] with valid = (target != ignore_index).
    Its denominator depends on the targets: the forward leaves it in `stats` on the device and the backward reads it
    there, so the node never waits for the host.  weight gets no gradient."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, want_argmax):
        logits, target, weight, dims, pred = _ce_front("cross_entropy", logits, target, weight, want_argmax)
        P = target.numel()
        loss = _empty((), logits)
        ws_bytes = lib().raw("vmtl_ce_workspace_bytes" if ignore_index is None else "vmtl_ce_ex_workspace_bytes")(P)
        ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=logits.device)
        if ignore_index is not None:
            stats = _empty((2,), logits)
            _k("vmtl_ce_fwd_ex", logits=logits, target=target, weight=weight, ignore_index=ignore_index, loss=loss,
               stats=stats, workspace=ws, argmax=pred, **dims)
            ctx.save_for_backward(logits, target, stats, *(() if weight is None else (weight,)))
        else:
            if want_argmax:
                _k("vmtl_ce_fwd_argmax", logits=logits, target=target, loss=loss, workspace=ws, argmax=pred, **dims)
            else:
                _k("vmtl_ce_fwd", logits=logits, target=target, loss=loss, workspace=ws, **dims)
            ctx.save_for_backward(logits, target)
        ctx.ignore_index = ignore_index
        return _ce_result(ctx, loss, pred)

    @staticmethod
    def backward(ctx, g, _gpred=None):
        logits, target, *ex = ctx.saved_tensors  # ex: (stats[, weight]) of the weighted / ignoring form
        g = _req(g, "grad_output")
        st, dstrides = _ce_grad_storage(logits)
        if ctx.ignore_index is None:
            _k("vmtl_ce_bwd_strided", logits=logits, target=target, grad_out=g, dlogits=st, **_ce_dims(logits), **dstrides)
        else:
            _k("vmtl_ce_bwd_ex", logits=logits, target=target, weight=ex[1] if len(ex) > 1 else None,
               ignore_index=ctx.ignore_index, stats=ex[0], grad_out=g, dlogits=st, **_ce_dims(logits), **dstrides)
        return _ce_grad_view(st, logits.shape[1]), None, None, None, None


def _ce_ignore(weight, ignore_index):
    """The node's ignore_index: None for the plain mean (nothing given), else an int (NO_IGNORE: weights only)."""
    if ignore_index is None:
        return None if weight is None else NO_IGNORE
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise TypeError(f"cross_entropy: ignore_index must be an int or None, got {ignore_index!r}")
    return ignore_index


def cross_entropy(logits, target, weight=None, ignore_index=None):
    """torch.nn.functional.cross_entropy(logits, target) (mean); `weight` (C fp32 floats on the device) and
    `ignore_index` as torch's, except that the default ignores nothing: an unmapped label makes the loss NaN."""
    return _CrossEntropy.apply(logits, target, weight, _ce_ignore(weight, ignore_index), False)


def cross_entropy_with_argmax(logits, target, weight=None, ignore_index=None):
    """(loss, argmax over the class axis) from one pass over the logits (reference lit_module.py:123 + 137-138).  The
    prediction is written for every pixel, ignored or not."""
    return _CrossEntropy.apply(logits, target, weight, _ce_ignore(weight, ignore_index), True)


class _CrossEntropyOHEM(torch.autograd.Function):
    """The weighted / ignoring cross entropy over the hard pixels only (csrc/ce_ohem.hip): a valid pixel is kept when
    its unweighted nll is not below cut = min(tau, K-th largest nll), K = min(min_kept_total, valid pixels).  The
    selection runs on the device: K, the cut and the denominator never visit the host, so the node captures like
    _CrossEntropy.  The forward saves the per-pixel nll and stats = (den, num, cut, 0); the backward decides membership
    from those - never from a recomputed nll.  No gradient flows through the selection; weight gets none."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, tau, min_kept_total, want_argmax):
        logits, target, weight, dims, pred = _ce_front("cross_entropy_ohem", logits, target, weight, want_argmax)
        P = target.numel()
        loss, stats, nll = _empty((), logits), _empty((4,), logits), _empty(tuple(target.shape), logits)
        counts = torch.empty((2,), dtype=torch.int64, device=logits.device)
        ws = torch.empty((lib().raw("vmtl_ce_ohem_workspace_bytes")(P) // 8,), dtype=torch.float64, device=logits.device)
        _k("vmtl_ce_ohem_fwd", logits=logits, target=target, weight=weight, ignore_index=ignore_index, nll_thresh=tau,
           min_kept_total=min_kept_total, loss=loss, stats=stats, counts=counts, nll=nll, workspace=ws, argmax=pred,
           **dims)
        ctx.save_for_backward(logits, target, stats, nll, *(() if weight is None else (weight,)))
        ctx.ignore_index = ignore_index
        return _ce_result(ctx, loss, pred)

    @staticmethod
    def backward(ctx, g, _gpred=None):
        logits, target, stats, nll, *w = ctx.saved_tensors
        g = _req(g, "grad_output")
        st, dstrides = _ce_grad_storage(logits)
        _k("vmtl_ce_ohem_bwd", logits=logits, target=target, weight=w[0] if w else None, ignore_index=ctx.ignore_index,
           stats=stats, nll=nll, grad_out=g, dlogits=st, **_ce_dims(logits), **dstrides)
        return (_ce_grad_view(st, logits.shape[1]),) + (None,) * 6


def ohem_tau(thresh) -> float:
    """tau = -log(thresh), the nll above which a pixel counts as hard: thresh is a true-class probability in (0, 1];
    None is +inf (pure top-K).  Computed in double, +0.0 at thresh = 1."""
    if thresh is None:
        return float("inf")
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)):
        raise TypeError(f"cross_entropy_ohem: thresh must be a float in (0, 1] or None, got {thresh!r}")
    if not 0.0 < thresh <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"cross_entropy_ohem: thresh must be in (0, 1], got {thresh!r}")
    return -math.log(thresh) + 0.0


def _ohem_args(logits, min_kept, thresh, weight, ignore_index):
    if isinstance(min_kept, bool) or not isinstance(min_kept, int):
        raise TypeError(f"cross_entropy_ohem: min_kept must be an int, got {min_kept!r}")
    if min_kept < 1:
        raise ValueError(f"cross_entropy_ohem: min_kept must be at least 1 pixel per image, got {min_kept}")
    tau = ohem_tau(thresh)
    ign = _ce_ignore(weight, ignore_index)
    return NO_IGNORE if ign is None else ign, tau, min_kept * logits.shape[0]


def cross_entropy_ohem(logits, target, min_kept, thresh=None, weight=None, ignore_index=None):
    """Cross entropy with online hard example mining (bootstrapped cross entropy): the mean, weighted as
    ops.cross_entropy(weight=, ignore_index=) weights it, over the valid pixels whose true-class probability is below
    `thresh` - and never fewer than min_kept per image (min_kept * B hardest pixels of the batch; every tie at the cut is
    kept).  thresh None: pure top-K.  thresh = 1.0, or min_kept * B at least the number of valid pixels: every valid
    pixel, i.e. ops.cross_entropy."""
    ign, tau, total = _ohem_args(logits, min_kept, thresh, weight, ignore_index)
    return _CrossEntropyOHEM.apply(logits, target, weight, ign, tau, total, False)


def cross_entropy_ohem_with_argmax(logits, target, min_kept, thresh=None, weight=None, ignore_index=None):
    """(loss, argmax over the class axis) from the one pass over the logits; the prediction is written for every pixel."""
    ign, tau, total = _ohem_args(logits, min_kept, thresh, weight, ignore_index)
    return _CrossEntropyOHEM.apply(logits, target, weight, ign, tau, total, True)


CE_REGION_MAX_CLASSES = 32  # include/vmtl.h VMTL_CE_REGION_MAX_CLASSES: the register form of csrc/ce_region.hip


class _CrossEntropyRegion(torch.autograd.Function):
    """ce_weight * (weighted / ignoring cross entropy) + region_weight * the Dice / Jaccard / Tversky region term
    (csrc/ce_region.hip) from one pass over the logits per direction.  The forward leaves the
    cross entropy's denominator (stats) and the 2C coefficients of the term's gradient (coef) on the device; the backward
    reads them there, so the node never waits for the host and captures like _CrossEntropy.  The gradient is handed off
    in the same NHWC storage.  weight (cross entropy only) gets no gradient."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, alpha, beta, smooth, ce_weight, region_weight, want_argmax):
        logits, target, weight, dims, pred = _ce_front("segm_region_loss", logits, target, weight, want_argmax,
                                                       max_classes=CE_REGION_MAX_CLASSES)
        P, C = target.numel(), logits.shape[1]
        loss, terms, stats, coef = (_empty(s, logits) for s in ((), (2,), (2,), (2 * C,)))
        counts = torch.empty((C + 1,), dtype=torch.int64, device=logits.device)
        ws = torch.empty((lib().raw("vmtl_ce_region_workspace_bytes")(P, C) // 8,), dtype=torch.float64,
                         device=logits.device)
        _k("vmtl_ce_region_fwd", logits=logits, target=target, weight=weight, ignore_index=ignore_index, alpha=alpha,
           beta=beta, smooth=smooth, ce_weight=ce_weight, region_weight=region_weight, loss=loss, terms=terms,
           stats=stats, coef=coef, counts=counts, workspace=ws, argmax=pred, **dims)
        ctx.save_for_backward(logits, target, stats, coef, *(() if weight is None else (weight,)))
        ctx.ignore_index, ctx.ce_weight, ctx.region_weight = ignore_index, ce_weight, region_weight
        return _ce_result(ctx, loss, pred)

    @staticmethod
    def backward(ctx, g, _gpred=None):
        logits, target, stats, coef, *w = ctx.saved_tensors
        g = _req(g, "grad_output")
        st, dstrides = _ce_grad_storage(logits)
        _k("vmtl_ce_region_bwd", logits=logits, target=target, weight=w[0] if w else None, ignore_index=ctx.ignore_index,
           stats=stats, coef=coef, grad_out=g, ce_weight=ctx.ce_weight, region_weight=ctx.region_weight, dlogits=st,
           **_ce_dims(logits), **dstrides)
        return (_ce_grad_view(st, logits.shape[1]),) + (None,) * 9


def region_loss_number(v, name, who="segm_region_loss", positive=False) -> float:
    """A finite float >= 0 (> 0 with `positive`) among the region term's scalars; TypeError / ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{who}: {name} must be a float, got {v!r}")
    if not math.isfinite(v) or v < 0 or (positive and v == 0):
        raise ValueError(f"{who}: {name} must be finite and {'> 0' if positive else '>= 0'}, got {v!r}")
    return float(v)


def _region_args(logits, region_weight, alpha, beta, smooth, weight, ignore_index, ce_weight):
    """Everything that can be wrong with the call, before any launch."""
    args = (region_loss_number(alpha, "alpha", positive=True), region_loss_number(beta, "beta", positive=True),
            region_loss_number(smooth, "smooth"), region_loss_number(ce_weight, "ce_weight"),
            region_loss_number(region_weight, "region_weight", positive=True))
    ign = _ce_ignore(weight, ignore_index)
    if logits.dim() != 4:
        raise ValueError(f"segm_region_loss: logits must be (B,C,H,W), got shape {tuple(logits.shape)}")
    if not 2 <= logits.shape[1] <= CE_REGION_MAX_CLASSES:
        raise ValueError(f"segm_region_loss: the region term takes 2 to {CE_REGION_MAX_CLASSES} classes, got "
                         f"{logits.shape[1]}")
    return (NO_IGNORE if ign is None else ign,) + args


def segm_region_loss(logits, target, region_weight=1.0, alpha=0.5, beta=0.5, smooth=0.0, weight=None, ignore_index=None,
                     ce_weight=1.0):
    """ce_weight * ops.cross_entropy(logits, target, weight, ignore_index) + region_weight * the Tversky region term
    L = (1/C) sum_{c present} (1 - (TP_c + smooth) / (TP_c + alpha FP_c + beta FN_c + smooth)) on the softmax
    probabilities over the valid pixels of the batch (alpha = beta = 0.5: Dice, alpha = beta = 1: Jaccard; the
    multiclass form of segmentation_models_pytorch: a class absent from the labels adds 0).  `weight` applies to the
    cross entropy only; ce_weight = 0 is the term alone.  At most 32 classes."""
    return _CrossEntropyRegion.apply(logits, target, weight,
                                     *_region_args(logits, region_weight, alpha, beta, smooth, weight, ignore_index,
                                                   ce_weight), False)


def segm_region_loss_with_argmax(logits, target, region_weight=1.0, alpha=0.5, beta=0.5, smooth=0.0, weight=None,
                                 ignore_index=None, ce_weight=1.0):
    """(loss, argmax over the class axis) from the one pass over the logits; the prediction is written for every pixel."""
    return _CrossEntropyRegion.apply(logits, target, weight,
                                     *_region_args(logits, region_weight, alpha, beta, smooth, weight, ignore_index,
                                                   ce_weight), True)


class _SILog(torch.autograd.Function):
    """reference losses.py:29-36 on predictions in (0,1); pred and target hold the same number of elements.  The valid
    pixels are those with target > min_depth, or those of an explicit uint8 mask (losses.py:29-31 with `mask` given)."""

    @staticmethod
    def forward(ctx, pred, target, min_depth, mask):
        pred, target = _req(pred, "pred"), _req(target, "target")
        if pred.numel() != target.numel():
            raise ValueError("silog: pred and target must have the same number of elements")
        P = pred.numel()
        loss, stats = _empty((), pred), _empty((3,), pred)
        ws = torch.empty((lib().raw("vmtl_silog_workspace_bytes")(P) // 8,), dtype=torch.float64, device=pred.device)
        if mask is None:
            _k("vmtl_silog_fwd", pred=pred, target=target, min_depth=min_depth, loss=loss, stats=stats, workspace=ws, P=P)
            ctx.save_for_backward(pred, target, stats)
        else:
            _k("vmtl_silog_fwd_mask", pred=pred, target=target, mask=mask, loss=loss, stats=stats, workspace=ws, P=P)
            ctx.save_for_backward(pred, target, stats, mask)
        ctx.min_depth = min_depth
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, stats, *mask = ctx.saved_tensors
        g = _req(g, "grad_output")
        dp = _empty(pred.shape, pred)
        if mask:
            _k("vmtl_silog_bwd_mask", pred=pred, target=target, mask=mask[0], stats=stats, grad_out=g, dpred=dp,
               P=pred.numel())
        else:
            _k("vmtl_silog_bwd", pred=pred, target=target, stats=stats, grad_out=g, min_depth=ctx.min_depth, dpred=dp,
               P=pred.numel())
        return dp, None, None, None


def silog(pred, target, min_depth=1e-3, mask=None):
    """reference losses.py:14-36.  mask (bool or uint8, the shape of target): the valid pixels; min_depth is then not
    applied, as in the reference."""
    if mask is None:
        return _SILog.apply(pred, target, float(min_depth), None)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"silog: mask must be bool or uint8, got {mask.dtype}")
    if tuple(mask.shape) != tuple(target.shape):
        raise ValueError(f"silog: mask shape {tuple(mask.shape)} does not match target {tuple(target.shape)}")
    if not mask.is_cuda or mask.device != target.device:
        raise RuntimeError(f"silog: mask is on {mask.device}, the target on {target.device} (no CPU fallback)")
    mask = mask.contiguous()
    return _SILog.apply(pred, target, float(min_depth), mask.view(torch.uint8) if mask.dtype == torch.bool else mask)


DEPTH_GRAD_SCALES_MAX = 6  # csrc/depth_grad.hip


class _DepthLoss(torch.autograd.Function):
    """silog_weight * SILog + grad_weight * (multi-scale gradient matching on log depth), csrc/depth_grad.hip: one node,
    one dpred.  pred / target are [B][H][W] in memory; the residual image, SILog's statistics and the per-scale valid
    counts stay on the device between forward and backward."""

    @staticmethod
    def forward(ctx, pred, target, min_depth, mask, geom, scales, silog_weight, grad_weight):
        pred, target = _req(pred, "pred"), _req(target, "target")
        B, H, W = geom
        loss, terms, stats = _empty((), pred), _empty((2,), pred), _empty((3,), pred)
        resid = _empty((B, H, W), pred)
        counts = torch.empty((scales,), dtype=torch.int64, device=pred.device)
        ws = torch.empty((lib().raw("vmtl_depth_grad_workspace_bytes")(B, H, W, scales) // 8,), dtype=torch.float64,
                         device=pred.device)
        _k("vmtl_depth_grad_fwd", pred=pred, target=target, mask=mask, min_depth=min_depth, B=B, H=H, W=W, scales=scales,
           silog_weight=silog_weight, grad_weight=grad_weight, loss=loss, terms=terms, stats=stats, counts=counts,
           resid=resid, workspace=ws)
        if mask is None:
            ctx.save_for_backward(pred, target, resid, stats, counts)
        else:
            ctx.save_for_backward(pred, target, resid, stats, counts, mask)
        ctx.args = (min_depth, geom, scales, silog_weight, grad_weight)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, resid, stats, counts, *mask = ctx.saved_tensors
        min_depth, (B, H, W), scales, silog_weight, grad_weight = ctx.args
        g = _req(g, "grad_output")
        dp = _empty(pred.shape, pred)
        _k("vmtl_depth_grad_bwd", pred=pred, target=target, mask=mask[0] if mask else None, min_depth=min_depth,
           resid=resid, stats=stats, counts=counts, grad_out=g, B=B, H=H, W=W, scales=scales, silog_weight=silog_weight,
           grad_weight=grad_weight, dpred=dp)
        return dp, None, None, None, None, None, None, None


def depth_loss_weight(w, name):
    """A loss weight of the depth criterion as a float: finite and not negative."""
    if isinstance(w, bool) or not isinstance(w, (int, float)):
        raise TypeError(f"depth_loss: {name} must be a float, got {w!r}")
    w = float(w)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"depth_loss: {name} must be finite and not negative, got {w}")
    return w


def depth_loss_scales(scales):
    if isinstance(scales, bool) or not isinstance(scales, int):
        raise TypeError(f"depth_loss: scales must be an int, got {scales!r}")
    if not 1 <= scales <= DEPTH_GRAD_SCALES_MAX:
        raise ValueError(f"depth_loss: scales must be in 1..{DEPTH_GRAD_SCALES_MAX}, got {scales}")
    return scales


def depth_loss(pred, target, min_depth=1e-3, mask=None, grad_weight=0.5, scales=4, silog_weight=1.0):
    """silog_weight * SILog(pred, target) + grad_weight * L_grad, where L_grad is the scale-invariant gradient-matching
    term of MegaDepth / MiDaS on R = log(pred) - log(target): for s = 1, 2, .. 2^(scales-1), the sum of |R(y,x+s) - R(y,x)|
    and |R(y+s,x) - R(y,x)| over the pixels with y % s == x % s == 0 whose neighbour is inside the image, both valid,
    divided by the number of valid pixels of that grid (batch-based reduction; a scale with none contributes 0).
    pred: (B,H,W,1), (B,1,H,W) or (B,H,W); target: as many elements, in the same order.  Valid pixels and `mask` as
    ops.silog.  silog_weight = 0 gives the term alone (finite also with fewer than two valid pixels)."""
    scales = depth_loss_scales(scales)
    silog_weight, grad_weight = depth_loss_weight(silog_weight, "silog_weight"), depth_loss_weight(grad_weight, "grad_weight")
    if pred.dim() == 4 and pred.shape[3] == 1:
        geom = tuple(pred.shape[:3])
    elif pred.dim() == 4 and pred.shape[1] == 1:
        geom = (pred.shape[0], pred.shape[2], pred.shape[3])
    elif pred.dim() == 3:
        geom = tuple(pred.shape)
    else:
        raise ValueError(f"depth_loss: pred must be (B,H,W,1), (B,1,H,W) or (B,H,W), got {tuple(pred.shape)}")
    if pred.numel() != target.numel():
        raise ValueError("depth_loss: pred and target must have the same number of elements")
    if pred.numel() == 0:
        raise ValueError(f"depth_loss: empty pred {tuple(pred.shape)}")
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"depth_loss: mask must be bool or uint8, got {mask.dtype}")
        if tuple(mask.shape) != tuple(target.shape):
            raise ValueError(f"depth_loss: mask shape {tuple(mask.shape)} does not match target {tuple(target.shape)}")
        if not mask.is_cuda or mask.device != target.device:
            raise RuntimeError(f"depth_loss: mask is on {mask.device}, the target on {target.device} (no CPU fallback)")
        mask = mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    return _DepthLoss.apply(pred, target, float(min_depth), mask, tuple(int(v) for v in geom), scales, silog_weight,
                            grad_weight)


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        pred, target = _req(pred, "pred"), _req(target, "target")
        if pred.numel() != target.numel():
            raise ValueError("l1: pred and target must have the same number of elements")
        P = pred.numel()
        loss = _empty((), pred)
        ws = torch.empty((lib().raw("vmtl_silog_workspace_bytes")(P) // 8,), dtype=torch.float64, device=pred.device)
        _k("vmtl_l1_fwd", pred=pred, target=target, loss=loss, workspace=ws, P=P)
        ctx.save_for_backward(pred, target)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        g = _req(g, "grad_output")
        dp = _empty(pred.shape, pred)
        _k("vmtl_l1_bwd", pred=pred, target=target, grad_out=g, dpred=dp, P=pred.numel())
        return dp, None


def l1_loss(pred, target):
    return _L1.apply(pred, target)


# ----------------------------------------------------------------------------- optimizer
def adam_step(p, g, m, v, step_t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """Fused torch.optim.Adam update over flat fp32 buffers; step_t is a 1-element device
    tensor holding the (already incremented) step count."""
    _k("vmtl_adam_step", p=p, g=g, m=m, v=v, step_ptr=step_t, lr=lr, b1=betas[0], b2=betas[1], eps=eps,
       weight_decay=weight_decay, grad_scale=grad_scale, n=p.numel())


# Global-norm clipping and the extended Adam / AdamW update (csrc/optim.hip).  Plain launches, not autograd nodes: they
# run where torch.nn.utils.clip_grad_norm_ and optimizer.step() run, under no_grad, on flat fp32 buffers.
OPTIM_CTL_FLOATS = 16  # control block (include/vmtl.h): [0] norm [1] clip coefficient [2] non-finite [3] skipped [4] count
CTL_NORM, CTL_COEF, CTL_NONFINITE, CTL_SKIP, CTL_SKIPPED = 0, 1, 2, 3, 4


def _flat(t, name):
    """A flat fp32 device buffer exactly as given: these kernels write in place, so nothing may be copied."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the vmtl hot path only runs as HIP kernels on an MI355X "
                           "(there is deliberately no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous float32 buffer, got {t.dtype} with strides {t.stride()}")
    return t


def _max_norm(max_norm) -> float:
    """None / 0: no clipping (coefficient 1); a negative or NaN bound is an error, not a silent no-op."""
    if max_norm is None:
        return 0.0
    m = float(max_norm)
    if not m >= 0.0:
        raise ValueError(f"max_norm must be >= 0 or None, got {max_norm}")
    return m


@functools.lru_cache(maxsize=None)
def _hi_lo(x: float):
    """x as the fp32 pair the C ABI carries (hi + lo == x to double precision)."""
    hi = struct.unpack("f", struct.pack("f", x))[0]
    return hi, x - hi


def optim_workspace(n: int, like):
    """Workspace of grad_sumsq for n elements: one fp64 partial per workgroup."""
    return torch.empty((lib().raw("vmtl_grad_sumsq_workspace_bytes")(n) // 8,), dtype=torch.float64, device=like.device)


def optim_control_block(like):
    """A zeroed control block (the skipped-step count starts at 0)."""
    return torch.zeros(OPTIM_CTL_FLOATS, dtype=torch.float32, device=like.device)


def grad_sumsq(g, workspace=None, grad_scale=1.0):
    """Per-workgroup fp64 partial sums of (g * grad_scale)^2 into `workspace` (returned); deterministic."""
    g = _flat(g, "g")
    if workspace is None:
        workspace = optim_workspace(g.numel(), g)
    _k("vmtl_grad_sumsq", g=g, grad_scale=grad_scale, workspace=workspace, n=g.numel())
    return workspace


def optim_control(ctl, step_t, n, workspace=None, max_norm=None, skip_nonfinite=False, betas=(0.9, 0.999)):
    """Partials -> control block; step_t += 1 ON THE DEVICE unless the step is skipped.  n: the element count the
    partials cover, 0 when no norm was computed (then nothing is clipped and nothing can be skipped)."""
    (b1, b1_lo), (b2, b2_lo) = _hi_lo(betas[0]), _hi_lo(betas[1])
    _k("vmtl_optim_control", workspace=workspace if n else None, n=n, max_norm=_max_norm(max_norm),
       skip_nonfinite=int(bool(skip_nonfinite)), step_ptr=_flat(step_t, "step_t"), b1=b1, b1_lo=b1_lo, b2=b2,
       b2_lo=b2_lo, ctl=_flat(ctl, "ctl"))


def grad_norm(g, grad_scale=1.0, workspace=None, ctl=None):
    """Norm of g * grad_scale as a 0-dim device tensor (what clip_grad_norm_ returns); g is not written.  Two launches."""
    ws = grad_sumsq(g, workspace, grad_scale)
    ctl = optim_control_block(g) if ctl is None else ctl
    # the clip launch with nothing to clip: it sums the partials, records the norm and returns before touching g
    _k("vmtl_grad_clip_", g=g, workspace=ws, grad_scale=1.0, max_norm=0.0, ctl=_flat(ctl, "ctl"), n=g.numel())
    return ctl[CTL_NORM]


def scale_by_clip(g, max_norm, grad_scale=1.0, workspace=None, ctl=None):
    """torch.nn.utils.clip_grad_norm_ on the flat gradient g * grad_scale, in place, as two launches: g becomes
    g * grad_scale * min(1, max_norm / (norm + 1e-6)).  Returns the norm BEFORE clipping (0-dim device tensor)."""
    max_norm = _max_norm(max_norm)
    ws = grad_sumsq(g, workspace, grad_scale)
    ctl = optim_control_block(g) if ctl is None else ctl
    _k("vmtl_grad_clip_", g=g, workspace=ws, grad_scale=grad_scale, max_norm=max_norm, ctl=_flat(ctl, "ctl"),
       n=g.numel())
    return ctl[CTL_NORM]


def adam_step_ex(p, g, m, v, step_t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, *,
                 max_grad_norm=None, decoupled_weight_decay=False, skip_nonfinite=False, workspace=None, ctl=None):
    """torch.optim.Adam / AdamW over flat fp32 buffers with global-norm clipping folded in: the gradient the update sees
    is g * grad_scale * clip coefficient, g itself is only read.  step_t (1-element device tensor) holds the count of
    steps taken so far and is incremented by the control launch, not by the caller; with skip_nonfinite a step whose
    gradient norm is inf / NaN leaves p, m, v and step_t untouched and counts in ctl[CTL_SKIPPED].  lr: a float, or a
    0-dim / 1-element fp32 device tensor read at run time (a captured launch follows a scheduler).
    Launches: [sum of squares, when clipping or skipping] + control + update.  Returns the control block."""
    p, g, m, v = _flat(p, "p"), _flat(g, "g"), _flat(m, "m"), _flat(v, "v")
    n = p.numel()
    if not (g.numel() == m.numel() == v.numel() == n):
        raise ValueError("adam_step_ex: p, g, m and v must hold the same number of elements")
    max_norm = _max_norm(max_grad_norm)
    need_norm = max_norm > 0.0 or bool(skip_nonfinite)
    ctl = optim_control_block(p) if ctl is None else ctl
    if need_norm:
        workspace = grad_sumsq(g, workspace, grad_scale)
    optim_control(ctl, step_t, n if need_norm else 0, workspace, max_norm, skip_nonfinite, betas)
    lr_ptr = None
    if isinstance(lr, torch.Tensor):
        lr_ptr, lr = _flat(lr, "lr"), 0.0
    _k("vmtl_adam_step_ex", p=p, g=g, m=m, v=v, ctl=ctl, lr=lr, lr_ptr=lr_ptr, eps=eps, weight_decay=weight_decay,
       decoupled=int(bool(decoupled_weight_decay)), grad_scale=grad_scale, n=n)
    return ctl


# ----------------------------------------------------------------------------- averaged weights (csrc/weight_avg.hip)
# EMA / SWA of flat fp32 buffers.  Plain launches like the optimizer's: under no_grad, in place, no host sync.
WAVG_STATE_FLOATS = 8  # state block (include/vmtl.h): [0..1] n_averaged (int64) [2] weight [3] copy [4] skip [5] skipped count
WAVG_N, WAVG_WEIGHT, WAVG_COPY, WAVG_SKIP, WAVG_SKIPPED = 0, 2, 3, 4, 5
WAVG_MODES = {"ema": 0, "swa": 1}


def wavg_state(like):
    """A zeroed state block (n_averaged = 0: the first update copies)."""
    return _empty((WAVG_STATE_FLOATS,), like).zero_()


def wavg_n_averaged(state):
    """n_averaged as a 0-dim int64 view of the state block (what torch's AveragedModel keeps as a long)."""
    return state.view(torch.int64)[0]


def _wavg_mode(mode, decay):
    if mode not in WAVG_MODES:
        raise ValueError(f"weight averaging: mode must be one of {sorted(WAVG_MODES)}, got {mode!r}")
    d = float(decay)
    if mode == "ema" and not 0.0 <= d <= 1.0:
        raise ValueError(f"weight averaging: decay must lie in [0, 1], got {decay!r}")
    return WAVG_MODES[mode], _hi_lo(d)


def wavg_control(state, mode="ema", decay=0.999, warmup=False, ctl=None):
    """The weight of the next update into `state`, n_averaged += 1 ON THE DEVICE; with an optimizer control block `ctl`
    whose step was skipped, the update is skipped instead.  One launch of one workgroup."""
    code, (d, d_lo) = _wavg_mode(mode, decay)
    _k("vmtl_wavg_control", state=_flat(state, "state"), ctl=None if ctl is None else _flat(ctl, "ctl"), mode=code,
       decay=d, decay_lo=d_lo, warmup=int(bool(warmup)))


def wavg_update(e, p, state):
    """e += w * (p - e) (a copy on the first update, nothing on a skipped one) with w and the flags read from `state`;
    p is only read."""
    e, p = _flat(e, "e"), _flat(p, "p")
    if e.numel() != p.numel():
        raise ValueError("wavg_update: e and p must hold the same number of elements")
    _k("vmtl_wavg_update", e=e, p=p, state=_flat(state, "state"), n=e.numel())


def adam_step_wavg(p, g, m, v, e, state, step_t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, *,
                   mode="ema", decay=0.999, warmup=False, max_grad_norm=None, decoupled_weight_decay=False,
                   skip_nonfinite=False, workspace=None, ctl=None):
    """adam_step_ex with the averaged weights `e` updated in the same pass over the new p: the bits of adam_step_ex
    followed by wavg_control(ctl=ctl) + wavg_update, one launch and one read of p fewer.
    Launches: [sum of squares] + optimizer control + averaging control + update.  Returns the control block."""
    p, g, m, v, e = _flat(p, "p"), _flat(g, "g"), _flat(m, "m"), _flat(v, "v"), _flat(e, "e")
    n = p.numel()
    if not (g.numel() == m.numel() == v.numel() == e.numel() == n):
        raise ValueError("adam_step_wavg: p, g, m, v and e must hold the same number of elements")
    max_norm = _max_norm(max_grad_norm)
    need_norm = max_norm > 0.0 or bool(skip_nonfinite)
    ctl = optim_control_block(p) if ctl is None else ctl
    if need_norm:
        workspace = grad_sumsq(g, workspace, grad_scale)
    optim_control(ctl, step_t, n if need_norm else 0, workspace, max_norm, skip_nonfinite, betas)
    wavg_control(state, mode, decay, warmup, ctl=ctl)
    lr_ptr = None
    if isinstance(lr, torch.Tensor):
        lr_ptr, lr = _flat(lr, "lr"), 0.0
    _k("vmtl_adam_step_wavg", p=p, g=g, m=m, v=v, e=e, ctl=ctl, state=state, lr=lr, lr_ptr=lr_ptr, eps=eps,
       weight_decay=weight_decay, decoupled=int(bool(decoupled_weight_decay)), grad_scale=grad_scale, n=n)
    return ctl


def wavg_buffer_table(pairs):
    """Descriptor table of (live buffer, its average) pairs for wavg_buffers / swap_table_: built and uploaded once,
    never inside a graph capture (the idiom of _EvalBNTable).  The table holds addresses: the tensors must stay where
    they are, and the returned dict keeps them alive."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("wavg_buffer_table: the table must be built before the capture")
    pairs = [(_flat(s, "buffer"), _flat(a, "buffer average")) for s, a in pairs]
    if not pairs:
        raise ValueError("wavg_buffer_table: no buffers")
    for s, a in pairs:
        if s.numel() != a.numel() or s.numel() == 0:
            raise ValueError("wavg_buffer_table: a buffer and its average must hold the same, non-zero number of elements")
    size = lib().raw("vmtl_wavg_desc_bytes")()
    blob = b"".join(struct.pack("<QQq", s.data_ptr(), a.data_ptr(), s.numel()).ljust(size, b"\0") for s, a in pairs)
    return {"descs": torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(pairs[0][0].device), "n": len(pairs),
            "max_n": max(s.numel() for s, _ in pairs), "pairs": pairs}


def wavg_buffers(table, state):
    """wavg_update over every (buffer, average) pair of a wavg_buffer_table in ONE launch, same weight and flags."""
    _k("vmtl_wavg_buffers", descs=table["descs"], n=table["n"], max_n=table["max_n"], state=_flat(state, "state"))


def swap_(a, b):
    """Exchange two flat fp32 buffers in place, bit for bit (NaN payloads included); overlapping buffers are refused."""
    a, b = _flat(a, "a"), _flat(b, "b")
    if a.numel() != b.numel():
        raise ValueError("swap_: a and b must hold the same number of elements")
    _k("vmtl_swap_", a=a, b=b, n=a.numel())


def swap_table_(table):
    """swap_ over every (buffer, average) pair of a wavg_buffer_table in ONE launch."""
    _k("vmtl_swap_table_", descs=table["descs"], n=table["n"], max_n=table["max_n"])


# ----------------------------------------------------------------------------- gradient surgery (csrc/surgery.hip)
# The 2x2 Gram matrix of two per-task gradients, the coefficients a two-task method derives from it and their
# combination.  Plain launches like the optimizer's: no autograd, no host sync; surgery.GradSurgery owns the buffers.
SURGERY_STATE_FLOATS = 12  # state block (include/vmtl.h)
SURGERY_NA, SURGERY_D, SURGERY_NB, SURGERY_ALPHA, SURGERY_BETA, SURGERY_COSINE = range(6)
SURGERY_COUNTERS = 8  # first of the four words that hold the two int64 counters (steps, conflicts)
SURGERY_METHODS = {"sum": 0, "pcgrad": 1, "mgda": 2, "imtl_g": 3}


def surgery_method(method) -> int:
    if method not in SURGERY_METHODS:
        raise ValueError(f"gradient surgery: method must be one of {sorted(SURGERY_METHODS)}, got {method!r}")
    return SURGERY_METHODS[method]


def surgery_state(like):
    """A zeroed state block (both counters start at 0)."""
    return _empty((SURGERY_STATE_FLOATS,), like).zero_()


def surgery_counters(state):
    """(steps seen, steps with d < 0) as a 2-element int64 view of the state block."""
    return state[SURGERY_COUNTERS:SURGERY_COUNTERS + 4].view(torch.int64)


def surgery_workspace(rows: int, width: int, like):
    """Workspace of surgery_gram for `rows` rows of `width` floats: three fp64 partials per workgroup."""
    nbytes = lib().raw("vmtl_surgery_workspace_bytes")(rows, width)
    if nbytes <= 0:
        raise ValueError(f"gradient surgery: bad shape rows = {rows}, width = {width}")
    return _empty((nbytes // 4,), like).view(torch.float64)


def surgery_workspace_max(like):
    """A workspace large enough for surgery_gram at ANY shape (the grid is capped): what an owner allocates once when a
    captured launch will hold the address."""
    return surgery_workspace(1 << 40, 1, like)


def _surgery_operand(t, name):
    """An fp32 device operand exactly as given (a strided view of a map is fine: the launch takes its leading dimension)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the vmtl hot path only runs as HIP kernels on an MI355X "
                           "(there is deliberately no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t


def _surgery_pair(a, b, rows, width, lda, ldb):
    """(rows, width, lda, ldb) of a pair of operands: flat buffers of equal length unless the caller says otherwise."""
    _surgery_operand(a, "a"), _surgery_operand(b, "b")
    if rows is None:
        if a.numel() != b.numel():
            raise ValueError("gradient surgery: a and b must hold the same number of elements")
        rows, width = 1, a.numel()
    lda = width if lda is None else lda
    ldb = width if ldb is None else ldb
    return rows, width, lda, ldb


def surgery_gram(a, b, workspace=None, *, rows=None, width=None, lda=None, ldb=None):
    """Per-workgroup fp64 partial sums of a*a, a*b, b*b into `workspace` (returned); deterministic.  a, b: two flat
    buffers, or `rows` rows of `width` floats with leading dimensions lda / ldb (a and b may be views of one map)."""
    rows, width, lda, ldb = _surgery_pair(a, b, rows, width, lda, ldb)
    if workspace is None:
        workspace = surgery_workspace(rows, width, a)
    _k("vmtl_surgery_gram", a=a, lda=lda, b=b, ldb=ldb, rows=rows, width=width, workspace=workspace)
    return workspace


def surgery_control(workspace, state, method, rows, width):
    """Partials of surgery_gram(rows, width) -> Gram matrix, coefficients, cosine and counters in `state`.  One launch of
    one workgroup."""
    _k("vmtl_surgery_control", workspace=workspace, rows=rows, width=width, method=surgery_method(method),
       state=_flat(state, "state"))


def surgery_combine(a, b, state, out=None, *, rows=None, width=None, lda=None, ldb=None, ldo=None):
    """out = alpha * a + beta * b with the coefficients read from `state`; out may be a.  Lanes [width, ldo) of out are
    left alone."""
    rows, width, lda, ldb = _surgery_pair(a, b, rows, width, lda, ldb)
    if out is None:
        out = _empty((rows, width) if rows > 1 else (width,), a)
    ldo = width if ldo is None else ldo
    _k("vmtl_surgery_combine", a=a, lda=lda, b=b, ldb=ldb, state=_flat(state, "state"), out=_surgery_operand(out, "out"),
       ldo=ldo,
       rows=rows, width=width)
    return out
