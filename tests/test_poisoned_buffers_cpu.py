"""The poison / guard harness of tests/poison.py can fail: proven here on CPU tensors (no kernel is ever made to write
outside its allocation - the 'stray stores' below are in-bounds writes into the harness's own, larger buffer), plus the
collection guard of the sweep in tests/test_poisoned_buffers_gpu.py."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import poison
from tests.util import assert_close

LIKE = torch.zeros(1)


def _ops():
    from vision_mtl_amd import ops

    return ops


def test_sentinel_is_a_quiet_nan():
    v = torch.tensor([poison.SENTINEL], dtype=torch.int32).view(torch.float32)
    assert math.isnan(v.item())
    assert poison.SENTINEL >> 22 == 0x1FF  # sign 0, exponent all ones, quiet bit set
    assert (poison.GUARD * 4) % 256 == 0


def test_fully_written_buffer_closes_clean():
    ops = _ops()
    with poison.patched("guard") as p:
        t = ops._empty((3, 5, 8), LIKE)
        g = ops._grad_buf((7,), None, LIKE)  # parameter gradients come through the same allocator
        assert t.shape == (3, 5, 8) and t.dtype == torch.float32 and t.is_contiguous()
        assert poison.is_sentinel(t).all() and poison.is_sentinel(g).all()
        t.copy_(torch.arange(120.0).view(3, 5, 8))
        g.zero_()
        assert p.count == 2 and len(p.bases) == 2
    assert torch.equal(t, torch.arange(120.0).view(3, 5, 8))  # the payload outlives the harness


@pytest.mark.parametrize("side", ["before", "after"])
def test_store_next_to_the_payload_is_reported(side):
    ops = _ops()
    with pytest.raises(AssertionError) as e:
        with poison.patched("guard") as p:
            ops._empty((4,), LIKE).zero_()
            t = ops._empty((6, 4), LIKE)
            t.zero_()
            base = p.bases[1][0]
            assert base.numel() == 24 + 2 * poison.GUARD and t.data_ptr() == base.data_ptr() + 4 * poison.GUARD
            # one float through the BASE buffer, right next to the payload: in bounds of the harness's allocation
            base.view(torch.float32)[poison.GUARD - 1 if side == "before" else poison.GUARD + 24] = 1.0
    msg = str(e.value)
    lines = [l for l in msg.splitlines() if "buffer #" in l]
    assert len(lines) == 1, msg  # the clean buffer #0 and the clean side are not named
    assert "buffer #1 of shape (6, 4)" in lines[0] and f"{side} the payload" in lines[0]
    assert "1 guard word(s)" in lines[0]
    assert f"float offset {-1 if side == 'before' else 24} " in lines[0]


def test_all_violations_come_in_one_error():
    ops = _ops()
    with pytest.raises(AssertionError) as e:
        with poison.patched("guard") as p:
            for k in range(3):
                ops._empty((k + 1, 2), LIKE).zero_()
            p.bases[0][0][0] = 0
            p.bases[2][0][-3:] = 0
    msg = str(e.value)
    assert "buffer #0 of shape (1, 2): 1 guard word(s) before" in msg
    assert "buffer #2 of shape (3, 2): 3 guard word(s) after" in msg
    assert f"float offset {6 + poison.GUARD - 3} " in msg  # offsets count from the payload's first element
    assert "buffer #1" not in msg


@pytest.mark.parametrize("mode", poison.MODES)
def test_unwritten_last_row_is_nan_exactly_there(mode):
    ops = _ops()
    with poison.patched(mode):
        t = ops._empty((5, 12), LIKE)
        t[:4] = 1.0
    assert torch.equal(torch.isnan(t), torch.arange(5)[:, None].expand(5, 12) == 4)
    assert torch.equal(poison.is_sentinel(t), torch.isnan(t))


def test_empty_is_restored_also_after_an_exception():
    ops = _ops()
    orig = ops._empty
    with poison.patched("poison"):
        assert ops._empty is not orig
    assert ops._empty is orig
    with pytest.raises(KeyError):
        with poison.patched("guard"):
            assert ops._empty is not orig
            raise KeyError("from inside the block")
    assert ops._empty is orig
    with pytest.raises(AssertionError):
        with poison.patched("guard") as p:
            ops._empty((2,), LIKE)
            p.bases[0][0][0] = 0
    assert ops._empty is orig
    with pytest.raises(ValueError):
        poison.Poison("zero")


@pytest.mark.parametrize("mode", poison.MODES)
@pytest.mark.parametrize("shape", [(), (0,), (3, 0, 4), 5])
def test_zero_dim_and_empty_shapes(mode, shape):
    ops = _ops()
    with poison.patched(mode):
        t = ops._empty(shape, LIKE)
        want = torch.empty(shape)
        assert t.shape == want.shape and t.dtype == torch.float32
        assert torch.isnan(t).all()
        if t.numel():
            t.fill_(2.0)
    if t.dim() == 0:
        assert t.item() == 2.0


def test_poison_mode_keeps_the_storage_the_in_place_paths_test_for():
    ops = _ops()
    with poison.patched("poison"):
        for shape in ((2, 4, 32, 20), (), (7,)):
            t = ops._empty(shape, LIKE)
            assert t.storage_offset() == 0 and t.untyped_storage().nbytes() == 4 * t.numel()
            assert t.is_contiguous()
    with poison.patched("guard"):  # ... and guard mode does not: those nodes fall back to their relayout launch
        t = ops._empty((2, 4, 32, 20), LIKE)
        assert t.storage_offset() == poison.GUARD and t.is_contiguous()
        t.zero_()


def test_the_comparators_reject_the_sentinel():
    ops = _ops()
    with poison.patched("poison"):
        t = ops._empty((4, 8), LIKE)
    ref = torch.zeros(4, 8)
    with pytest.raises(AssertionError):
        assert_close(t, ref, atol=1.0)
    t.zero_()
    t.view(torch.int32)[3, 7] = poison.SENTINEL  # one element is enough
    with pytest.raises(AssertionError):
        assert_close(t, ref, atol=1.0)
    with pytest.raises(AssertionError):
        assert_close(ref, t, atol=1.0)
    assert not (t.abs().max().item() == 0.0)  # the pad-lane idiom
    assert not (t[..., 4:].abs().max().item() == 0.0)
    assert not torch.equal(t, ref)
    assert not torch.equal(t, t.clone())


# ------------------------------------------------------------------------------------------------ collection guard
def _collect(paths):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", *paths],
                       capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.strip() for l in r.stdout.splitlines() if re.match(r"^tests/\S+\.py::", l.strip())]


def test_sweep_covers_exactly_what_pytest_collects():
    """A renamed, added or newly parametrised test of a swept module must not drop out of a sweep silently: the ids
    pytest collects from the swept modules, and the ids of each sweep (test_guarded, test_launch_guarded) mapped back to
    their originals, are the same set (apart from that sweep's explicit exclusion list, which is bounded)."""
    from tests import test_poisoned_buffers_gpu as sweep

    mods = [f"tests/{m}.py" for m in sweep.SWEPT_MODULES]
    ids = _collect(mods + [f"tests/{m}.py" for m in sweep.SWEPT_FUNCTIONS] + ["tests/test_poisoned_buffers_gpu.py"])
    sweeps = {"test_guarded": (set(), sweep.EXCLUDED), "test_launch_guarded": (set(), sweep.EXCLUDED_LAUNCH)}
    originals, listed, others = set(), set(), []
    for i in ids:
        path, rest = i.split("::", 1)
        if path == "tests/test_poisoned_buffers_gpu.py":
            name = rest.split("[")[0]
            if name not in sweeps:
                others.append(rest)
                continue
            orig = sweep.original_id(rest, name)
            assert orig not in sweeps[name][0], f"{orig} is swept twice by {name}"
            sweeps[name][0].add(orig)
        elif path in mods:
            originals.add(i)
        elif rest.split("[")[0] in sweep.SWEPT_FUNCTIONS[path[len("tests/"):-len(".py")]]:
            listed.add(i)
    # the tally of the second sweep is collected, and after every case of it
    assert others == ["test_launch_guarded_leaves_few_pointers_in_place"] and ids[-1].endswith(others[0]), others
    for name, (swept, exclusions) in sweeps.items():
        excluded = {e for e, _ in exclusions}
        assert len(excluded) == len(exclusions), f"{name}: an id is excluded twice"
        assert excluded <= originals | listed, f"{name}: excluded ids that do not exist: {sorted(excluded - originals - listed)}"
        assert all(reason.strip() for _, reason in exclusions)
        assert len(excluded) <= 0.05 * len(originals | listed), name
        missing, extra = (originals | listed) - excluded - swept, swept - ((originals | listed) - excluded)
        assert not missing, f"{name}: collected but not swept: {sorted(missing)}"
        assert not extra, f"{name}: swept but not collected (or excluded): {sorted(extra)}"
    assert len(originals) >= 348  # the five modules at the commit that introduced the sweep
    assert len(listed) >= 219     # the listed functions at the commit that introduced the second sweep
    for m, names in sweep.SWEPT_FUNCTIONS.items():  # every listed function exists and contributed a case
        for n in names:
            assert any(i.startswith(f"tests/{m}.py::{n}") for i in listed), f"{m}.{n} is listed but not collected"
    assert sweep.LEFT_IN_PLACE_CAP == 0.05
