"""Host side of csrc/bn.hip (no GPU needed): every launcher refuses an argument set it cannot run with status -1 BEFORE
any launch and without trapping.  Pointers are dummy non-null values, so every call here is one the launcher must refuse
by its own checks; each runs in a forked child (tests/test_dwconv_host_cpu.in_child), so that a trap fails one test and
not the session.

BASE holds one acceptable argument set per launcher by parameter NAME (the order comes from include/vmtl.h through
lib().protos); a case overrides one or two of them.  The base sets themselves are never passed."""
import pytest

from tests.test_dwconv_host_cpu import in_child
from vision_mtl_amd._lib import lib

ERR_ARG = -1
P = 1  # a dummy non-null pointer

_DIMS = dict(M=8, C=6, Cs=8)
_STATS = dict(x=P, partial=P, nblk_from_conv=0, rows_per_blk_from_conv=0, eps=1e-5, momentum=0.1, running_mean=P,
              running_var=P, num_batches_tracked=P, save_mean=P, save_invstd=P, stream=None, **_DIMS)
_EVAL = dict(running_mean=P, running_var=P, C=6, Cs=8, eps=1e-5, save_mean=P, save_invstd=P, stream=None)
_POOL = dict(x=P, mean=P, invstd=P, gamma=P, beta=P, B=2, H=4, W=6, C=6, Cs=8, act=1, stream=None)
BASE = {
    "vmtl_bn_stats": _STATS,
    "vmtl_bn_stats_coef": dict(_STATS, gamma=P, beta=P, coef_a=P, coef_c=P),
    "vmtl_bn_eval_stats": _EVAL,
    "vmtl_bn_eval_stats_coef": dict(_EVAL, gamma=P, beta=P, coef_a=P, coef_c=P),
    "vmtl_bn_apply": dict(x=P, mean=P, invstd=P, gamma=P, beta=P, mul=P, res=P, y=P, act=1, stream=None, **_DIMS),
    "vmtl_bn_apply_fused": dict(x=P, partial=P, nblk=2, rows_per_blk=4, eps=1e-5, momentum=0.1, running_mean=P,
                                running_var=P, num_batches_tracked=P, save_mean=P, save_invstd=P, gamma=P, beta=P, mul=P,
                                res=P, y=P, act=1, stream=None, **_DIMS),
    "vmtl_bn_bwd": dict(x=P, dy=P, mean=P, invstd=P, gamma=P, beta=P, mul=P, dmul=P, partial=P, sum_dz=P, sum_dzx=P, dx=P,
                        act=1, training=1, stream=None, **_DIMS),
    "vmtl_bn_bwd_finalize": dict(partial=P, nblk=2, sum_dz=P, sum_dzx=P, mean=P, invstd=P, gamma=P, training=1, coef_a=P,
                                 coef_b=P, coef_c=P, stream=None, **_DIMS),
    "vmtl_bn_bwd_apply": dict(x=P, dz=P, mean=P, invstd=P, gamma=P, sum_dz=P, sum_dzx=P, dx=P, training=1, stream=None,
                              **_DIMS),
    "vmtl_bn_act_pool2_fwd": dict(_POOL, y=P),
    "vmtl_bn_act_pool2_bwd": dict(_POOL, dyp=P, partial=P, sum_dz=P, sum_dzx=P, dx=P, training=1),
    "vmtl_colsum": dict(a=P, b=P, mode=1, reduce_all=0, partial=P, out=P, stream=None, **_DIMS),
    "vmtl_stitch_bwd": dict(x=P, dy=P, w=P, dx=P, partial=P, dw=P, wstride=1, reduce_all=0, stream=None, **_DIMS),
}
LAUNCHERS = tuple(BASE)


def refused(name, **over):
    args = dict(BASE[name], **over)
    order = lib().protos[name][2]
    assert set(order) == set(args), f"{name}: the base set does not name the header's parameters: {sorted(set(order) ^ set(args))}"
    assert over, "a base set is never passed: it would launch"
    return in_child(name, *[args[n] for n in order])


def test_base_sets_cover_every_launcher_of_bn_hip():
    """every int-returning vmtl_bn_* / colsum / stitch_bwd entry point that takes a stream and lives in bn.hip"""
    in_bn_hip = {n for n, (_, _, names) in lib().protos.items()
                 if "stream" in names and (n.startswith("vmtl_bn_") or n in ("vmtl_colsum", "vmtl_stitch_bwd"))
                 and not n.startswith(("vmtl_bn_act_pool3s2", "vmtl_bn_add_act"))}  # csrc/resnet.hip
    assert in_bn_hip - {"vmtl_bn_eval_stats_batch"} == set(LAUNCHERS)


def _rows_name(name):
    return "B" if "pool2" in name else "M"


@pytest.mark.parametrize("name", LAUNCHERS)
def test_every_launcher_refuses_bad_dimensions(name):
    if "eval" not in name:
        for rows in (0, -1):
            assert refused(name, **{_rows_name(name): rows}) == ERR_ARG, f"{_rows_name(name)} = {rows}"
    for C in (0, -4):
        assert refused(name, C=C) == ERR_ARG, f"C = {C}"
    assert refused(name, C=9) == ERR_ARG, "C > Cs"
    assert refused(name, C=12, Cs=8) == ERR_ARG, "C > Cs"
    for Cs in (6, 7, 10):
        assert refused(name, Cs=Cs) == ERR_ARG, f"Cs = {Cs}"
    assert refused(name, C=1, Cs=0) == ERR_ARG and refused(name, C=0, Cs=0) == ERR_ARG


@pytest.mark.parametrize("name", ["vmtl_bn_apply", "vmtl_bn_bwd", "vmtl_bn_bwd_apply", "vmtl_bn_bwd_finalize",
                                  "vmtl_bn_act_pool2_fwd", "vmtl_bn_act_pool2_bwd"])
def test_one_of_mean_and_invstd_null(name):
    assert refused(name, mean=None) == ERR_ARG and refused(name, invstd=None) == ERR_ARG


def test_one_of_the_coefficient_outputs_null():
    for name in ("vmtl_bn_stats_coef", "vmtl_bn_eval_stats_coef"):
        assert refused(name, coef_a=None) == ERR_ARG and refused(name, coef_c=None) == ERR_ARG
    for missing in ("coef_a", "coef_b", "coef_c"):
        assert refused("vmtl_bn_bwd_finalize", **{missing: None}) == ERR_ARG, missing
    for name in ("vmtl_bn_stats", "vmtl_bn_stats_coef", "vmtl_bn_apply_fused"):  # the kernels test running_mean only
        assert refused(name, running_mean=None) == ERR_ARG and refused(name, running_var=None) == ERR_ARG


def test_rows_that_do_not_cover_m():
    for name in ("vmtl_bn_stats", "vmtl_bn_stats_coef"):
        assert refused(name, nblk_from_conv=2, rows_per_blk_from_conv=3) == ERR_ARG  # 6 < 8
        assert refused(name, nblk_from_conv=2, rows_per_blk_from_conv=0) == ERR_ARG
        assert refused(name, nblk_from_conv=3, rows_per_blk_from_conv=-4) == ERR_ARG
        assert refused(name, x=None) == ERR_ARG  # no rows given and nothing to sweep
    assert refused("vmtl_bn_apply_fused", nblk=2, rows_per_blk=3) == ERR_ARG
    assert refused("vmtl_bn_apply_fused", nblk=0) == ERR_ARG and refused("vmtl_bn_apply_fused", rows_per_blk=0) == ERR_ARG
    assert refused("vmtl_bn_apply_fused", nblk=1 << 16, rows_per_blk=1 << 16, M=(1 << 31) - 1) == ERR_ARG  # no int overflow
    # b * rows_per_blk is computed in int by the kernels: rows that would overflow it are refused, not miscounted
    assert refused("vmtl_bn_apply_fused", nblk=64, rows_per_blk=1 << 26) == ERR_ARG
    assert refused("vmtl_bn_apply_fused", nblk=2, rows_per_blk=1 << 30) == ERR_ARG
    for name in ("vmtl_bn_stats", "vmtl_bn_stats_coef"):
        assert refused(name, nblk_from_conv=64, rows_per_blk_from_conv=1 << 26) == ERR_ARG
        assert refused(name, nblk_from_conv=1 << 20, rows_per_blk_from_conv=1 << 11) == ERR_ARG


def test_fused_apply_refuses_more_rows_than_it_merges():
    most = lib().raw("vmtl_bn_fuse_max_rows")()
    assert most == 64
    assert refused("vmtl_bn_apply_fused", nblk=most + 1, rows_per_blk=1) == ERR_ARG
    assert refused("vmtl_bn_apply_fused", nblk=1000, rows_per_blk=8) == ERR_ARG


@pytest.mark.parametrize("name", ["vmtl_bn_act_pool2_fwd", "vmtl_bn_act_pool2_bwd"])
def test_pool_refuses_odd_and_sub_2_maps(name):
    for H, W in ((3, 6), (4, 5), (1, 6), (4, 1), (0, 6), (4, 0), (-2, 6), (5, 7)):
        assert refused(name, H=H, W=W) == ERR_ARG, (H, W)
    assert refused(name, B=1 << 20, H=1 << 10, W=1 << 10) == ERR_ARG  # B*H*W past int


@pytest.mark.parametrize("name", ["vmtl_bn_apply", "vmtl_bn_apply_fused", "vmtl_bn_bwd", "vmtl_bn_act_pool2_fwd",
                                  "vmtl_bn_act_pool2_bwd"])
def test_unknown_activation_code(name):
    for act in (5, -1, 99):
        assert refused(name, act=act) == ERR_ARG, act
    if name == "vmtl_bn_bwd":  # also on the route without sums and without dmul, which skips the first dispatch
        assert refused(name, act=5, mean=None, invstd=None, dmul=None) == ERR_ARG


def test_required_pointers():
    assert refused("vmtl_colsum", b=None) == ERR_ARG  # mode 1 reads b
    assert refused("vmtl_bn_bwd", partial=None) == ERR_ARG and refused("vmtl_bn_bwd", sum_dz=None) == ERR_ARG
    assert refused("vmtl_bn_bwd_apply", sum_dzx=None) == ERR_ARG  # training reads the sums
    assert refused("vmtl_bn_bwd_finalize", nblk=0) == ERR_ARG
    f = lib().raw("vmtl_bn_eval_stats_batch")
    assert f(None, 1, 8, None) == ERR_ARG and f(P, 0, 8, None) == ERR_ARG and f(P, 1, 6, None) == ERR_ARG
    assert f(P, 1, 0, None) == ERR_ARG and f(P, 65536, 8, None) == ERR_ARG


@pytest.mark.parametrize("M", [0, -1, -16, -(1 << 31)])
def test_reduce_rows_of_an_empty_map_is_one(M):
    assert in_child("vmtl_reduce_rows", M) >= 1
