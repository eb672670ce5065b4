"""csrc/weight_avg.hip against tests/weight_avg_oracle.py (fp64 on the CPU) and against csrc/optim.hip bit for bit.

Sizes: a lone element, fewer than one vector, one workgroup's edge (255 / 257), a vector-width edge (1023) and
4096 * 256 + 5, which needs a second trip of the grid-stride loop (the float4 body has 1024 workgroups of 256 threads; the
scalar fall-back has 4096 workgroups).  Each size runs on a 16-byte-aligned payload and on buf[1:] (3 head elements are
peeled); "mixed" puts every buffer at another offset inside its 16-byte line, which takes the scalar fall-back.

Every device buffer - parameters, average, gradient, moments, workspace, control block, state block, step counter - is the
payload of a guard-banded, NaN-poisoned allocation of tests/poison.py.  The average starts POISONED: the first update is a
copy that must not read it.

Tolerance of the update: the derived bound of weight_avg_oracle (2^-21 * max(|e|, |p|) per update, accumulated); a CPU
fp32 run of the same inputs stayed at 0.78 of 2^-22 per update.  Everything else is bit equality."""
import math

import pytest
import torch

from tests import poison
from tests import weight_avg_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 257, 1023, 4096 * 256 + 5]
OFFS = [0, 1, "mixed"]
MODES = [("ema", False), ("ema", True), ("swa", False)]
DECAY = 0.99
LR = 5e-3


def _ops():
    from vision_mtl_amd import ops

    return ops


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


_INPUTS = {}


def _inputs(n):
    """Three parameter vectors and three gradients (randn * 0.1, 10, 1), fp32 on the CPU; fixed per size."""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(7000 + n)
        ps = [torch.randn(n, generator=g) for _ in range(3)]
        grads = [torch.randn(n, generator=g) * s for s in (0.1, 10.0, 1.0)]
        _INPUTS[n] = (ps, grads)
    return _INPUTS[n]


_ORACLE = {}


def _oracle(n, mode, warmup):
    """The oracle's (e, bound) after each of the three updates; computed once per case."""
    key = (n, mode, warmup)
    if key not in _ORACLE:
        ps, _ = _inputs(n)
        o = O.AverageOracle(ps[0], mode, DECAY, warmup)
        snaps = []
        for p in ps:
            o.update(p)
            s = O.AverageOracle(p, mode, DECAY, warmup)
            s.e, s.bound, s.n = o.e.clone(), o.bound.clone(), o.n
            snaps.append(s)
        _ORACLE[key] = snaps
    return _ORACLE[key]


class _Bufs:
    """Guard-banded device buffers; close() checks the guards and the skipped elements in front of misaligned payloads."""

    def __init__(self, dev):
        self.P = poison.Poison("guard")
        self.like = torch.empty(0, device=dev)
        self.fronts = []

    def f32(self, n, off=0, src=None):
        base = self.P.empty(n + off, self.like)
        if off:
            self.fronts.append(base[:off])
        t = base[off:]
        if src is not None:
            t.copy_(src)
        return t

    def zeros(self, n, off=0):
        return self.f32(n, off, torch.zeros(n))

    def workspace(self, n):
        nbytes = _ops().lib().raw("vmtl_grad_sumsq_workspace_bytes")(n)
        return self.P.empty(nbytes // 4, self.like).view(torch.float64)

    def ctl(self):
        return self.zeros(_ops().OPTIM_CTL_FLOATS)

    def state(self):
        return self.zeros(_ops().WAVG_STATE_FLOATS)

    def close(self):
        for f in self.fronts:
            assert bool(poison.is_sentinel(f).all()), "an element in front of a misaligned payload was written"
        self.P.close()


def _offs(off):
    """Offsets of (p, g, m, v, e) inside their 16-byte lines."""
    return (0, 1, 2, 3, 1) if off == "mixed" else (off,) * 5


# ----------------------------------------------------------------------------- the stand-alone update
def _run_updates(dev, n, off, mode, warmup):
    ops = _ops()
    ps, _ = _inputs(n)
    offs = _offs(off)
    B = _Bufs(dev)
    state = B.state()
    e = B.f32(n, offs[4])  # poisoned: the first update copies and must not read it
    out = []
    for i in range(3):
        p = B.f32(n, offs[0], ps[i])
        ops.wavg_control(state, mode, DECAY, warmup)
        ops.wavg_update(e, p, state)
        assert _same_bits(p, ps[i]), "the update must not write p"
        out.append((e.clone(), state.clone()))
    B.close()
    return out


@pytest.mark.parametrize("mode,warmup", MODES)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_update_matches_oracle_and_is_deterministic(dev, n, off, mode, warmup):
    ops = _ops()
    ps, _ = _inputs(n)
    ref = _oracle(n, mode, warmup)
    a = _run_updates(dev, n, off, mode, warmup)
    b = _run_updates(dev, n, off, mode, warmup)
    for i, ((e, state), (e2, state2)) in enumerate(zip(a, b)):
        assert _same_bits(e, e2) and _same_bits(state, state2), f"two runs of update {i} differ"
        assert int(ops.wavg_n_averaged(state)) == i + 1
        assert float(state[ops.WAVG_WEIGHT]) == O.weight_fp32(i, mode, DECAY, warmup)
        assert float(state[ops.WAVG_COPY]) == (1.0 if i == 0 else 0.0) and float(state[ops.WAVG_SKIP]) == 0.0
        if i == 0:
            assert _same_bits(e, ps[0]), "the first update is an exact copy"
        O.assert_within(e, ref[i], what=f"n={n} off={off} {mode} warmup={warmup} update {i}")


@pytest.mark.parametrize("mode,warmup", MODES + [("swa", True)])
def test_weight_and_counter_match_the_oracle(dev, mode, warmup):
    """updates 0 to 3: the fp32 weight in the state block is the oracle's, exactly"""
    ops = _ops()
    B = _Bufs(dev)
    state = B.state()
    for n in range(4):
        ops.wavg_control(state, mode, DECAY, warmup)
        assert float(state[ops.WAVG_WEIGHT]) == O.weight_fp32(n, mode, DECAY, warmup and mode == "ema"), (mode, warmup, n)
        assert float(state[ops.WAVG_COPY]) == (1.0 if n == 0 else 0.0)
        got = ops.wavg_n_averaged(state)
        assert got.dim() == 0 and got.dtype == torch.int64 and got.is_cuda and int(got) == n + 1
    # the default decay needs its low half: 1 - 0.999 from the fp32 0.999 alone is off by 3e-5 of its value
    ops.wavg_control(state, "ema", 0.999, False)
    assert float(state[ops.WAVG_WEIGHT]) == O.weight_fp32(4, "ema", 0.999)
    B.close()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [3, 1023])
def test_optimizer_skip_flag_skips_the_update(dev, n, off):
    ops = _ops()
    ps, _ = _inputs(n)
    B = _Bufs(dev)
    state, ctl = B.state(), B.ctl()
    e = B.f32(n, off)
    p = B.f32(n, off, ps[0])
    ops.wavg_control(state, "ema", DECAY, False, ctl=ctl)
    ops.wavg_update(e, p, state)
    p.copy_(ps[1])
    before_e, before_n, before_w = e.clone(), ops.wavg_n_averaged(state).clone(), state[ops.WAVG_WEIGHT].clone()
    ctl[ops.CTL_SKIP] = 1.0
    ops.wavg_control(state, "ema", DECAY, False, ctl=ctl)
    ops.wavg_update(e, p, state)
    assert _same_bits(e, before_e), "a skipped update must leave the average bit for bit untouched"
    assert torch.equal(ops.wavg_n_averaged(state), before_n) and torch.equal(state[ops.WAVG_WEIGHT], before_w)
    assert float(state[ops.WAVG_SKIP]) == 1.0 and float(state[ops.WAVG_SKIPPED]) == 1.0
    ctl[ops.CTL_SKIP] = 0.0
    ops.wavg_control(state, "ema", DECAY, False, ctl=ctl)
    ops.wavg_update(e, p, state)
    assert int(ops.wavg_n_averaged(state)) == 2 and float(state[ops.WAVG_SKIP]) == 0.0
    o = O.AverageOracle(ps[0], "ema", DECAY).update(ps[0]).update(ps[1], skipped=True).update(ps[1])
    O.assert_within(e, o, what=f"n={n} off={off} after the skipped update")
    B.close()


# ----------------------------------------------------------------------------- the fused step
VARIANTS = {
    "plain": {},
    "clip": {"max_grad_norm": "sqrt_n"},
    "adamw": {"weight_decay": 0.1, "decoupled_weight_decay": True},
    "tensor_lr": {"tensor_lr": True},
}


def _run_steps(dev, n, off, variant, fused, grads=None, skip_nonfinite=False):
    """Three steps; returns the bits of (p, m, v, e, step, n_averaged) after each."""
    ops = _ops()
    ps, gs = _inputs(n)
    gs = gs if grads is None else grads
    kw = dict(VARIANTS[variant])
    if kw.get("max_grad_norm") == "sqrt_n":
        kw["max_grad_norm"] = math.sqrt(n)
    if skip_nonfinite:
        kw["skip_nonfinite"] = True
    offs = _offs(off)
    B = _Bufs(dev)
    lr = LR
    if kw.pop("tensor_lr", False):
        lr = B.f32(1, 0, torch.tensor([LR]))
    p, m, v, step = B.f32(n, offs[0], ps[0]), B.zeros(n, offs[2]), B.zeros(n, offs[3]), B.zeros(1)
    e = B.f32(n, offs[4])  # poisoned
    ws, ctl, state = B.workspace(n), B.ctl(), B.state()
    out = []
    for g_cpu in gs:
        g = B.f32(n, offs[1], g_cpu)
        if fused:
            ops.adam_step_wavg(p, g, m, v, e, state, step, lr, mode="ema", decay=DECAY, workspace=ws, ctl=ctl, **kw)
        else:
            ops.adam_step_ex(p, g, m, v, step, lr, workspace=ws, ctl=ctl, **kw)
            ops.wavg_control(state, "ema", DECAY, False, ctl=ctl)
            ops.wavg_update(e, p, state)
        assert _same_bits(g, g_cpu), "the gradient is read only"
        out.append([_bits(t) for t in (p, m, v, e, step)] + [int(ops.wavg_n_averaged(state))])
    B.close()
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_is_the_two_launches_bit_for_bit(dev, n, off, variant):
    two = _run_steps(dev, n, off, variant, fused=False)
    one = _run_steps(dev, n, off, variant, fused=True)
    again = _run_steps(dev, n, off, variant, fused=True)
    for i, (a, b, c) in enumerate(zip(two, one, again)):
        for name, x, y, z in zip(("p", "m", "v", "e", "step"), a, b, c):
            assert torch.equal(x, y), f"step {i}: {name} of the fused step differs from adam_step_ex + wavg_update"
            assert torch.equal(y, z), f"step {i}: two runs of the fused step differ in {name}"
        assert a[5] == b[5] == i + 1
        assert not bool(torch.isnan(b[3].view(torch.float32)).any())


@pytest.mark.parametrize("off", [0, 1, "mixed"])
@pytest.mark.parametrize("n", [3, 1023])
def test_fused_skipped_step_leaves_everything_untouched(dev, n, off):
    _, gs = _inputs(n)
    bad = gs[1].clone()
    bad[n // 2] = float("inf")
    for fused in (True, False):
        out = _run_steps(dev, n, off, "plain", fused=fused, grads=[gs[0], bad, gs[2]], skip_nonfinite=True)
        for name, x, y in zip(("p", "m", "v", "e", "step"), out[0], out[1]):
            assert torch.equal(x, y), f"fused={fused}: the skipped step changed {name}"
        assert [o[5] for o in out] == [1, 1, 2]
        assert not torch.equal(out[1][3], out[2][3]), "the step after the skipped one averages again"


# ----------------------------------------------------------------------------- swap
def _patterns(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    nans = torch.tensor([0x7FC12345, -0x3FFFFF, 0x7F800001, 0x7FFFFFFF], dtype=torch.int64).to(torch.int32)  # quiet,
    k = min(n, nans.numel())                                       # negative quiet, signalling, all-ones payloads
    x[:k] = nans[:k]
    return x


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bit_patterns(dev, n, off):
    ops = _ops()
    xa, xb = _patterns(n, 11), _patterns(n, 12)
    B = _Bufs(dev)
    oa, ob = (0, 1) if off == "mixed" else (off, off)
    a, b = B.f32(n, oa), B.f32(n, ob)
    a.view(torch.int32).copy_(xa)
    b.view(torch.int32).copy_(xb)
    ops.swap_(a, b)
    assert torch.equal(_bits(a), xb) and torch.equal(_bits(b), xa), "one swap exchanges the two buffers exactly"
    ops.swap_(a, b)
    assert torch.equal(_bits(a), xa) and torch.equal(_bits(b), xb), "two swaps restore them"
    B.close()


def test_swap_refuses_overlap(dev):
    ops = _ops()
    B = _Bufs(dev)
    buf = B.zeros(64)
    for a, b in ((buf[:32], buf[:32]), (buf[:32], buf[16:48]), (buf[31:63], buf[:32])):
        with pytest.raises(RuntimeError, match="bad argument"):
            ops.swap_(a, b)
    ops.swap_(buf[:32], buf[32:])  # adjacent, not overlapping
    assert float(buf.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        ops.swap_(buf[:8], buf[32:48])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.swap_(torch.zeros(4), torch.zeros(4))
    B.close()


# ----------------------------------------------------------------------------- buffers launch
_TABLE_SIZES = (1, 3, 64, 257, 1000)


def _run_table(dev, length, mode, warmup):
    ops = _ops()
    B = _Bufs(dev)
    g = torch.Generator().manual_seed(900 + length)
    sizes = [_TABLE_SIZES[i % len(_TABLE_SIZES)] for i in range(length)]
    srcs_cpu = [[torch.randn(s, generator=g) for s in sizes] for _ in range(3)]
    live = [B.f32(s, i % 2) for i, s in enumerate(sizes)]     # every other record misaligned
    avgs = [B.f32(s, (i // 2) % 2) for i, s in enumerate(sizes)]  # poisoned
    table = ops.wavg_buffer_table(list(zip(live, avgs)))
    state = B.state()
    out = []
    for k in range(3):
        for t, s in zip(live, srcs_cpu[k]):
            t.copy_(s)
        ops.wavg_control(state, mode, DECAY, warmup)
        ops.wavg_buffers(table, state)
        out.append([a.clone() for a in avgs])
    # the same table exchanges the pairs
    la, aa = [_bits(t) for t in live], [_bits(t) for t in avgs]
    ops.swap_table_(table)
    for t, a, x, y in zip(live, avgs, la, aa):
        assert torch.equal(_bits(t), y) and torch.equal(_bits(a), x), "swap_table_ exchanges every pair exactly"
    ops.swap_table_(table)
    for t, a, x, y in zip(live, avgs, la, aa):
        assert torch.equal(_bits(t), x) and torch.equal(_bits(a), y), "two table swaps restore every pair"
    B.close()
    return sizes, srcs_cpu, out


@pytest.mark.parametrize("mode,warmup", MODES)
@pytest.mark.parametrize("length", [1, 5, 64])
def test_buffers_table_matches_oracle(dev, length, mode, warmup):
    sizes, srcs, a = _run_table(dev, length, mode, warmup)
    _, _, b = _run_table(dev, length, mode, warmup)
    for r in range(length):
        o = O.AverageOracle(srcs[0][r], mode, DECAY, warmup)
        for k in range(3):
            o.update(srcs[k][r])
            assert _same_bits(a[k][r], b[k][r]), f"two runs differ in record {r}, update {k}"
            if k == 0:
                assert _same_bits(a[0][r], srcs[0][r]), "the first update is an exact copy"
            if r < 5 or k == 2:
                O.assert_within(a[k][r], o, what=f"table of {length}, record {r} ({sizes[r]} floats), update {k}")
            else:
                err = (a[k][r].double().cpu() - o.e).abs()
                assert bool((err <= o.bound).all())


def test_cpu_tensors_raise(dev):
    ops = _ops()
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wavg_control(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wavg_update(x, x.clone(), ops.wavg_state(torch.empty(0, device=dev)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wavg_buffer_table([(x, x.clone())])
    with pytest.raises(ValueError):
        ops.wavg_control(ops.wavg_state(torch.empty(0, device=dev)), "mean")
    with pytest.raises(ValueError):
        ops.wavg_control(ops.wavg_state(torch.empty(0, device=dev)), "ema", 1.5)
