"""The BatchNorm steps the autograd nodes of vision_mtl_amd.ops share (_bn_stats, _bn_apply, _resolve_rpb / stats_rpb,
_bn_bwd_tail): which entry point each one launches and with which row arguments.  No GPU: ops._k is replaced by a recorder
(as tests/test_pw_precision_cpu.py does) and the helpers only allocate and launch, so CPU tensors do."""
import pytest
import torch

C, CS, SHAPE = 6, 8, (1, 4, 8, 8)  # logical / stored channels, the activation (B, H, W, Cs)
M = SHAPE[0] * SHAPE[1] * SHAPE[2]
RPB = 7  # an explicit row block no fallback would produce


@pytest.fixture
def rec(monkeypatch):
    from vision_mtl_amd import ops

    calls = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: calls.append((name, kw)))
    return ops, calls


def _bn():
    return dict(rm=torch.zeros(C), rv=torch.ones(C), nbt=torch.zeros((), dtype=torch.int64), gamma=torch.ones(C),
                beta=torch.zeros(C))


def _table(monkeypatch, ops, b, eps=1e-5):
    """an eval table in force that describes the layer b: its four vectors"""
    e = tuple(torch.full((CS,), float(i)) for i in range(4))
    monkeypatch.setattr(ops.eval_bn, "active", {b["rm"].data_ptr(): e + (C, eps, b["gamma"].data_ptr(), b["beta"].data_ptr())})
    return e


def _stats(ops, x, b, stats, rpb, training, affine):
    return ops._bn_stats(x, stats, rpb, b["rm"], b["rv"], b["nbt"], C, training, 0.1, 1e-5,
                         (b["gamma"], b["beta"]) if affine else None)


def _row_cases(ops):
    return (1, ops._BN_FUSE_ROWS, ops._BN_FUSE_ROWS + 1)


@pytest.mark.parametrize("affine", [False, True])
def test_bn_stats_train(rec, affine):
    ops, calls = rec
    x, b = torch.zeros(SHAPE), _bn()
    name = "vmtl_bn_stats_coef" if affine else "vmtl_bn_stats"
    for nblk in _row_cases(ops):  # conv rows: finalized as they are, with the row block the caller resolved
        calls.clear()
        stats = torch.zeros(nblk, 2, CS)
        out = _stats(ops, x, b, stats, RPB, True, affine)
        (got, kw), = calls
        assert got == name and kw["partial"] is stats and tuple(kw["partial"].shape) == (nblk, 2, CS)
        assert (kw["nblk_from_conv"], kw["rows_per_blk_from_conv"]) == (nblk, RPB)
        assert len(out) == (4 if affine else 2) and all(tuple(t.shape) == (CS,) for t in out)
        assert kw["save_mean"] is out[0] and kw["save_invstd"] is out[1]
        assert ("coef_a" in kw) == affine and (not affine or (kw["coef_a"] is out[2] and kw["coef_c"] is out[3]))
    calls.clear()  # no rows: a sweep of x into scratch rows, whatever row block was passed
    _stats(ops, x, b, None, RPB, True, affine)
    (got, kw), = calls
    assert got == name and tuple(kw["partial"].shape) == (ops._reduce_rows(M), 2, CS)
    assert (kw["nblk_from_conv"], kw["rows_per_blk_from_conv"]) == (0, 0)


@pytest.mark.parametrize("affine", [False, True])
def test_bn_stats_eval(rec, monkeypatch, affine):
    ops, calls = rec
    x, b = torch.zeros(SHAPE), _bn()
    out = _stats(ops, x, b, torch.zeros(3, 2, CS), RPB, False, affine)  # without a table: one launch, rows ignored
    (got, kw), = calls
    assert got == ("vmtl_bn_eval_stats_coef" if affine else "vmtl_bn_eval_stats")
    assert "partial" not in kw and kw["running_mean"] is b["rm"] and kw["save_mean"] is out[0]
    assert len(out) == (4 if affine else 2)
    calls.clear()  # under a table: its vectors, no launch
    e = _table(monkeypatch, ops, b)
    out = _stats(ops, x, b, None, 0, False, affine)
    assert calls == [] and len(out) == (4 if affine else 2) and all(o is t for o, t in zip(out, e))


def test_bn_stats_hands_a_zero_row_block_through(rec):
    """the pre-activation nodes pass rpb as given: rows with rpb 0 reach the launch (and fail there), tag or no tag"""
    ops, calls = rec
    x, b = torch.zeros(SHAPE), _bn()
    stats = torch.zeros(4, 2, CS)
    stats._vmtl_rpb = 5
    _stats(ops, x, b, stats, 0, True, True)
    (got, kw), = calls
    assert got == "vmtl_bn_stats_coef" and (kw["nblk_from_conv"], kw["rows_per_blk_from_conv"]) == (4, 0)


def _apply(ops, x, b, stats, rpb, training):
    return ops._bn_apply(x, stats, rpb, b["gamma"], b["beta"], b["rm"], b["rv"], b["nbt"], C, training, 0.1, 1e-5,
                         ops.ACT_RELU)


def test_bn_apply_folds_the_finalize_for_few_rows(rec, monkeypatch):
    ops, calls = rec
    x, b = torch.zeros(SHAPE), _bn()
    for nblk in _row_cases(ops):
        calls.clear()
        stats = torch.zeros(nblk, 2, CS)
        y, mean, invstd = _apply(ops, x, b, stats, RPB, True)
        assert y.shape == x.shape and tuple(mean.shape) == tuple(invstd.shape) == (CS,)
        if nblk <= ops._BN_FUSE_ROWS:
            (got, kw), = calls
            assert got == "vmtl_bn_apply_fused" and kw["partial"] is stats and (kw["nblk"], kw["rows_per_blk"]) == (nblk, RPB)
            assert kw["y"] is y and kw["save_mean"] is mean and kw["save_invstd"] is invstd
        else:
            (n0, k0), (n1, k1) = calls
            assert (n0, n1) == ("vmtl_bn_stats", "vmtl_bn_apply") and k0["partial"] is stats
            assert (k0["nblk_from_conv"], k0["rows_per_blk_from_conv"]) == (nblk, RPB)
            assert k1["y"] is y and k1["mean"] is mean and k1["invstd"] is invstd
    calls.clear()  # the switch is read at call time
    monkeypatch.setattr(ops, "_BN_FUSE_ROWS", 0)
    _apply(ops, x, b, torch.zeros(1, 2, CS), RPB, True)
    assert [n for n, _ in calls] == ["vmtl_bn_stats", "vmtl_bn_apply"]


def test_bn_apply_without_rows_and_in_eval(rec, monkeypatch):
    ops, calls = rec
    x, b = torch.zeros(SHAPE), _bn()
    _apply(ops, x, b, None, RPB, True)
    (n0, k0), (n1, _) = calls
    assert (n0, n1) == ("vmtl_bn_stats", "vmtl_bn_apply") and tuple(k0["partial"].shape) == (ops._reduce_rows(M), 2, CS)
    assert (k0["nblk_from_conv"], k0["rows_per_blk_from_conv"]) == (0, 0)
    calls.clear()
    _apply(ops, x, b, torch.zeros(1, 2, CS), RPB, False)  # eval: rows or not, the running statistics
    assert [n for n, _ in calls] == ["vmtl_bn_eval_stats", "vmtl_bn_apply"]
    calls.clear()
    e = _table(monkeypatch, ops, b)
    _, mean, invstd = _apply(ops, x, b, None, 0, False)
    assert [n for n, _ in calls] == ["vmtl_bn_apply"] and mean is e[0] and invstd is e[1]


def test_row_block_resolver():
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    stats = torch.zeros(2, 2, CS)
    block = lib().raw("vmtl_conv2d_stats_block")(*SHAPE)
    assert block > 0 and block not in (RPB, 5)
    assert ops._resolve_rpb(stats, 0, SHAPE) == block and ops.stats_rpb(stats) == 0  # untagged: the implicit GEMM's block
    stats._vmtl_rpb = 5
    assert ops._resolve_rpb(stats, 0, SHAPE) == 5 and ops.stats_rpb(stats) == 5  # the tag wins over the shape
    assert ops._resolve_rpb(stats, RPB, SHAPE) == RPB  # the explicit argument wins over the tag
    assert ops._resolve_rpb(None, RPB, SHAPE) == 0 and ops.stats_rpb(None) == 0  # no rows


def test_bn_act_resolves_and_pass_through_wrappers_do_not(monkeypatch):
    """ops.bn_act hands its node the resolved row block; ops.bn_act_dwconv hands on the rpb it was given"""
    from vision_mtl_amd import ops

    seen = []

    class Stub:
        @staticmethod
        def apply(*args):
            seen.append(args)
            return (torch.zeros(SHAPE), None)

    monkeypatch.setattr(ops, "_BNAct", Stub)
    monkeypatch.setattr(ops, "_BNActDw", Stub)
    x, b = torch.zeros(SHAPE), _bn()
    stats = torch.zeros(2, 2, CS)
    stats._vmtl_rpb = 5
    ops.bn_act(x, b["gamma"], b["beta"], b["rm"], b["rv"], b["nbt"], C, True, stats=stats)
    assert seen[-1][-1] == 5
    bn = torch.nn.BatchNorm2d(C)
    ops.bn_act_dwconv(x, stats, 0, bn, C, ops.ACT_RELU, torch.zeros(C, 1, 3, 3), want_stats=False)
    assert seen[-1][1] is stats and seen[-1][2] == 0
    assert seen[-1][3:8] == (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    bn.momentum = None
    with pytest.raises(NotImplementedError):
        ops.bn_act_dwconv(x, stats, 0, bn, C, ops.ACT_RELU, torch.zeros(C, 1, 3, 3))


@pytest.mark.parametrize("want_dx", [False, True])
@pytest.mark.parametrize("slotted", [False, True])
def test_bn_bwd_tail(rec, want_dx, slotted):
    ops, calls = rec
    x, dz = torch.zeros(SHAPE), torch.zeros(SHAPE)
    mean, invstd, gamma = torch.zeros(CS), torch.ones(CS), torch.ones(C)
    rows = 3
    part = torch.zeros(rows, 2, CS)
    slots = (torch.zeros(C), torch.zeros(C)) if slotted else (None, None)  # tensors standing in for arena slots
    dx, dgamma, dbeta = ops._bn_bwd_tail(part, rows, x, dz, mean, invstd, gamma, C, True, slots, want_dx)
    assert [n for n, _ in calls] == ["vmtl_bn_bwd_finalize"] + (["vmtl_bn_bwd_apply"] if want_dx else [])
    fin = calls[0][1]
    assert fin["partial"] is part and (fin["nblk"], fin["M"], fin["C"], fin["Cs"], fin["training"]) == (rows, M, C, CS, 1)
    assert all(fin[k] is None for k in ("mean", "invstd", "gamma", "coef_a", "coef_b", "coef_c"))
    if slotted:  # the slots took the gradients: nothing for autograd to accumulate
        assert fin["sum_dzx"] is slots[0] and fin["sum_dz"] is slots[1] and dgamma is None and dbeta is None
    else:
        assert fin["sum_dzx"] is dgamma and fin["sum_dz"] is dbeta and tuple(dgamma.shape) == tuple(dbeta.shape) == (C,)
    if want_dx:
        ap = calls[1][1]
        assert ap["dx"] is dx and dx.shape == x.shape and ap["dz"] is dz and ap["x"] is x and ap["gamma"] is gamma
        assert ap["sum_dzx"] is fin["sum_dzx"] and ap["sum_dz"] is fin["sum_dz"] and ap["training"] == 1
    else:
        assert dx is None
