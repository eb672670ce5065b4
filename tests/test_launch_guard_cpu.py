"""tests/launch_guard.py proven without a GPU: a stand-in for _Lib whose callk is a Python function working on the CPU
tensors it is handed, with prototypes from a small header string.  No kernel is made to write outside an allocation:
the fake kernels' stray accesses go through as_strided over the harness's own, larger buffer, which is what a real
kernel's pointer arithmetic would reach."""
import pytest
import torch

from tests import launch_guard, poison

HEADER = """
/* a comment with a const float* in it */
int vmtl_fake_axpy(const float* x, float* y, float a, long long n, void* stream);
int vmtl_fake_scale(const float* x, float* y, const float* opt, int n, void* stream);  // y may alias x
int vmtl_fake_labels(const long long* t, const unsigned char* valid, float* out, int n, void* stream);
int vmtl_fake_table(const void* descs, int n, void* stream);
int vmtl_fake_count(int n);
"""


class FakeLib:
    """callk(name, **kw) as _Lib's: keyword arguments, tensors where the prototype has pointers."""

    def __init__(self, kernels):
        self.kernels = kernels
        self.seen = []

    def callk(self, name, **kw):
        self.seen.append((name, kw))
        self.kernels[name](**kw)


def _axpy(x, y, a, n, stream):
    y[:n] += a * x[:n]


def _scale(x, y, opt, n, stream):
    y[:n] = 2.0 * x[:n] if opt is None else opt[0] * x[:n]


def _elements(t, first, count):
    """`count` elements starting `first` elements from t's first one, wherever that lands in t's storage."""
    return t.as_strided((count,), (1,), t.storage_offset() + first)


def _guard(lib, **kw):
    return launch_guard.patched(lib=lib, header=HEADER, current_stream=kw.pop("current_stream", lambda: 0), **kw)


def test_honest_launch_is_identical_and_lands_in_the_callers_tensors():
    lib = FakeLib({"vmtl_fake_axpy": _axpy})
    x, y = torch.arange(7.0), torch.ones(7)
    want = y.clone()
    _axpy(x, want, 0.5, 7, 0)
    ptr = y.data_ptr()
    with _guard(lib) as g:
        lib.callk("vmtl_fake_axpy", x=x, y=y, a=0.5, n=7, stream=0)
        _, kw = lib.seen[-1]
        assert kw["x"].data_ptr() != x.data_ptr() and kw["y"].data_ptr() != ptr  # both moved
        assert kw["a"] == 0.5 and kw["n"] == 7 and kw["stream"] == 0 and isinstance(kw["n"], int)
        assert torch.equal(kw["x"], x) and kw["y"].shape == y.shape and kw["y"].dtype == y.dtype
    assert torch.equal(y, want) and y.data_ptr() == ptr
    assert torch.equal(x, torch.arange(7.0))
    assert (g.launches, g.pointers, g.relocated) == (1, 2, 2) and not any(g.left.values())
    assert "2 relocated" in g.counts()


def test_a_read_one_element_past_an_operand_is_nan():
    def kernel(x, y, a, n, stream):  # an unmasked tail: n + 1 elements of x are summed
        y[0] = _elements(x, 0, n + 1).sum()

    lib = FakeLib({"vmtl_fake_axpy": kernel})
    x, y = torch.ones(5), torch.zeros(1)
    kernel(x[:4], y, 0.0, 4, 0)
    assert y.item() == 5.0  # unguarded, the neighbour is live memory and the error is silent
    with _guard(lib):
        lib.callk("vmtl_fake_axpy", x=x, y=y, a=0.0, n=5, stream=0)
        seen = _elements(lib.seen[-1][1]["x"], -1, 7)
    assert torch.isnan(y).all()
    assert poison.is_sentinel(seen[[0, 6]]).all() and torch.equal(seen[1:6], x)  # NaN right before and right after


@pytest.mark.parametrize("side,first,offset", [("BEFORE", -1, -1), ("AFTER", 6, 6), ("AFTER", 9, 9)])
def test_a_store_next_to_an_output_is_reported_with_side_and_offset(side, first, offset):
    def kernel(x, y, a, n, stream):
        y[:n] = x[:n]
        _elements(y, first, 1).fill_(1.0)

    lib = FakeLib({"vmtl_fake_axpy": kernel, "vmtl_fake_scale": _scale})
    x, y = torch.arange(6.0), torch.zeros(6)
    with pytest.raises(AssertionError) as e:
        with _guard(lib):
            lib.callk("vmtl_fake_scale", x=x, y=torch.zeros(6), opt=None, n=6, stream=0)  # launch #1: honest
            lib.callk("vmtl_fake_axpy", x=x, y=y, a=0.0, n=6, stream=0)
    lines = [l for l in str(e.value).splitlines() if "launch #" in l]
    assert len(lines) == 1, str(e.value)  # the honest launch, the operand and the other side are not named
    assert "launch #2 vmtl_fake_axpy(y)" in lines[0] and f"store {side} the storage" in lines[0]
    assert f"byte offset {4 * offset} (float offset {offset})" in lines[0]
    assert torch.equal(y, x)  # the payload itself came back


def test_a_store_through_a_const_pointer_is_reported_by_parameter():
    def kernel(t, valid, out, n, stream):
        out[0] = t[:n].sum()
        valid[2] = 0  # `valid` is const in the header

    lib = FakeLib({"vmtl_fake_labels": kernel})
    t, valid, out = torch.arange(5), torch.ones(5, dtype=torch.uint8), torch.zeros(1)
    with pytest.raises(AssertionError) as e:
        with _guard(lib):
            lib.callk("vmtl_fake_labels", t=t, valid=valid, out=out, n=5, stream=0)
    msg = str(e.value)
    assert "vmtl_fake_labels: store through const parameter(s) valid," in msg and "byte offset 2 " in msg
    assert "parameter(s) t" not in msg and "the storage, the first" not in msg
    assert valid.tolist() == [1] * 5 and out.item() == 10.0  # a const group is not copied back


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.uint8, torch.bool, torch.uint16, torch.int32])
def test_every_dtype_moves_as_bytes(dtype):
    def kernel(descs, n, stream):
        assert descs.dtype == dtype and descs.shape == (3, 5)
        got.append(descs.clone())

    got = []
    lib = FakeLib({"vmtl_fake_table": kernel})
    src = (torch.arange(15).view(3, 5) % 2).to(dtype) if dtype == torch.bool else torch.arange(15).view(3, 5).to(dtype)
    with _guard(lib):
        lib.callk("vmtl_fake_table", descs=src, n=3, stream=0)
    assert torch.equal(got[0], src)


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_the_pointer_keeps_its_residue_modulo_256(offset):
    lib = FakeLib({"vmtl_fake_axpy": _axpy})
    base, y = torch.arange(40.0), torch.zeros(9)
    x = base[offset:offset + 9]
    with _guard(lib):
        for _ in range(3):  # fresh buffers every time
            lib.callk("vmtl_fake_axpy", x=x, y=y, a=1.0, n=9, stream=0)
            kw = lib.seen[-1][1]
            assert kw["x"].data_ptr() % 256 == x.data_ptr() % 256 and kw["x"].data_ptr() != x.data_ptr()
            assert kw["y"].data_ptr() % 256 == y.data_ptr() % 256
            assert kw["x"].data_ptr() % 16 == (base.data_ptr() + 4 * offset) % 16
    assert torch.equal(y, 3 * x)


def test_aliased_arguments_stay_aliased():
    lib = FakeLib({"vmtl_fake_scale": _scale})
    buf = torch.arange(8.0)
    with _guard(lib) as g:
        lib.callk("vmtl_fake_scale", x=buf, y=buf, opt=None, n=8, stream=0)  # in place
        kw = lib.seen[-1][1]
        assert kw["x"].data_ptr() == kw["y"].data_ptr() != buf.data_ptr()
        two = torch.arange(8.0)
        lib.callk("vmtl_fake_scale", x=two[:4], y=two, opt=None, n=4, stream=0)  # a const view of the output's storage
        kw = lib.seen[-1][1]
        assert kw["x"].data_ptr() == kw["y"].data_ptr() and kw["x"].shape == (4,)
    assert torch.equal(buf, 2 * torch.arange(8.0))
    assert two.tolist() == [0.0, 2.0, 4.0, 6.0, 4.0, 5.0, 6.0, 7.0]
    assert g.relocated == 4 and g.left["null"] == 2


def test_a_partial_writable_view_is_left_in_place_and_counted():
    """... once a second stream has been seen: it may be writing the rest of the storage."""
    lib = FakeLib({"vmtl_fake_scale": _scale})
    arena, x = torch.zeros(12), torch.arange(4.0)
    slot = arena[4:8]
    now = [5]
    with _guard(lib, current_stream=lambda: now[0]) as g:
        lib.callk("vmtl_fake_scale", x=x, y=torch.zeros(4), opt=None, n=4, stream=5)  # a launch under another stream
        now[0] = 0
        lib.callk("vmtl_fake_scale", x=x, y=slot, opt=arena[:1], n=4, stream=0)
        kw = lib.seen[-1][1]
        assert kw["y"].data_ptr() == slot.data_ptr() and kw["opt"].data_ptr() == arena.data_ptr()  # the whole storage stays
        assert kw["x"].data_ptr() != x.data_ptr()
    assert g.left == {"partial": 2, "stream": 0, "capturing": 0, "null": 1} and (g.pointers, g.relocated) == (6, 3)
    assert arena.tolist() == [0.0] * 12  # opt[0] == 0


def test_with_one_stream_a_partial_view_moves_and_only_its_own_bytes_come_back():
    def kernel(x, y, opt, n, stream):
        y[:n] = 2.0 * x[:n]
        if stray is not None:
            _elements(y, stray, 1).fill_(9.0)

    lib = FakeLib({"vmtl_fake_scale": kernel})
    x = torch.arange(4.0)
    stray = None
    arena = torch.full((12,), -1.0)
    with _guard(lib) as g:
        lib.callk("vmtl_fake_scale", x=x, y=arena[4:8], opt=arena[:1], n=4, stream=0)
        kw = lib.seen[-1][1]
        assert kw["y"].data_ptr() != arena[4:8].data_ptr() and kw["y"].data_ptr() - kw["opt"].data_ptr() == 16
        assert kw["y"].data_ptr() % 256 == arena[4:8].data_ptr() % 256
        arena[8:] = -2.0  # what another writer of the storage would do meanwhile: the copy-back must not undo it
    assert arena.tolist() == [-1.0] * 4 + [0.0, 2.0, 4.0, 6.0] + [-2.0] * 4
    assert g.relocated == 3 and not any(g.left.values())
    for stray, offset in ((-1, 3), (4, 8)):  # a store next to the slot, inside the arena
        arena = torch.full((12,), -1.0)
        with pytest.raises(AssertionError) as e:
            with _guard(lib):
                lib.callk("vmtl_fake_scale", x=x, y=arena[4:8], opt=None, n=4, stream=0)
        assert "vmtl_fake_scale: store outside the writable argument(s) y, inside their storage" in str(e.value)
        # 9.0 and -1.0 share their two low bytes: the first byte that differs is the third of the word
        assert f"byte offset {4 * offset + 2} (float offset {offset})" in str(e.value)
        assert arena[offset].item() == -1.0  # reported, not carried home


def test_foreign_stream_and_capture_leave_the_launch_alone():
    lib = FakeLib({"vmtl_fake_axpy": _axpy})
    x, y = torch.ones(3), torch.zeros(3)
    with _guard(lib, current_stream=lambda: 7) as g:
        lib.callk("vmtl_fake_axpy", x=x, y=y, a=1.0, n=3, stream=5)
        assert lib.seen[-1][1]["x"] is x and lib.seen[-1][1]["y"] is y
        lib.callk("vmtl_fake_axpy", x=x, y=y, a=1.0, n=3, stream=7)
        assert lib.seen[-1][1]["x"] is not x
    assert g.left["stream"] == 2 and g.relocated == 2
    with _guard(lib, capturing=lambda: True) as g:
        lib.callk("vmtl_fake_axpy", x=x, y=y, a=1.0, n=3, stream=0)
        assert lib.seen[-1][1]["y"] is y
    assert g.left["capturing"] == 2 and g.relocated == 0
    assert y.tolist() == [3.0] * 3


def test_none_ints_and_floats_pass_through_and_anything_else_raises():
    lib = FakeLib({"vmtl_fake_scale": _scale, "vmtl_fake_count": lambda n: None})
    x, y = torch.arange(3.0), torch.zeros(3)
    with _guard(lib) as g:
        lib.callk("vmtl_fake_scale", x=x, y=y, opt=None, n=3, stream=0)
        kw = lib.seen[-1][1]
        assert kw["opt"] is None and kw["n"] == 3 and kw["stream"] == 0
        lib.callk("vmtl_fake_count", n=4)
        assert lib.seen[-1][1] == {"n": 4}
        with pytest.raises(TypeError, match="does not declare as a pointer"):
            lib.callk("vmtl_fake_scale", x=x, y=y, opt=None, n=torch.tensor(3), stream=0)
        with pytest.raises(TypeError, match="neither a tensor"):
            lib.callk("vmtl_fake_scale", x=x, y=y, opt="weights", n=3, stream=0)
    assert g.left["null"] == 1 and y.tolist() == [0.0, 2.0, 4.0]


def test_empty_tensors_are_relocated_too():
    lib = FakeLib({"vmtl_fake_axpy": _axpy})
    with _guard(lib) as g:
        lib.callk("vmtl_fake_axpy", x=torch.empty(0), y=torch.empty(0), a=1.0, n=0, stream=0)
    assert g.relocated == 2


def test_the_wrapper_is_restored_also_after_an_exception():
    def failing(**kw):
        raise RuntimeError("vmtl_fake_axpy failed: bad argument (status -1)")

    lib = FakeLib({"vmtl_fake_axpy": failing})
    assert "callk" not in vars(lib)
    with _guard(lib):
        assert "callk" in vars(lib)
    assert "callk" not in vars(lib)
    y = torch.zeros(2)
    with pytest.raises(RuntimeError, match="status -1"):
        with _guard(lib):
            lib.callk("vmtl_fake_axpy", x=torch.ones(2), y=y, a=1.0, n=2, stream=0)
    assert "callk" not in vars(lib) and y.tolist() == [0.0, 0.0]
    with pytest.raises(AssertionError):  # ... and after a reported violation
        with _guard(FakeLib({"vmtl_fake_axpy": lambda x, y, a, n, stream: _elements(y, -1, 1).zero_()})) as g:
            g.lib.callk("vmtl_fake_axpy", x=torch.ones(2), y=y, a=1.0, n=2, stream=0)
    assert "callk" not in vars(g.lib)
    mine = lambda name, **kw: None
    lib.callk = mine  # an instance attribute that was there before comes back as it was
    with _guard(lib):
        assert lib.callk is not mine
    assert lib.callk is mine


def test_const_table_of_the_small_header():
    t = launch_guard.const_table(HEADER)
    assert t["vmtl_fake_axpy"] == {"x": True, "y": False, "stream": False}
    assert t["vmtl_fake_labels"] == {"t": True, "valid": True, "out": False, "stream": False}
    assert t["vmtl_fake_table"] == {"descs": True, "stream": False} and t["vmtl_fake_count"] == {}
    assert launch_guard.const_table("int vmtl_q(float* const p, float const* q, const float* const r);")["vmtl_q"] == {
        "p": False, "q": True, "r": True}


def test_const_table_of_the_real_header_names_every_pointer_parameter():
    import ctypes

    from vision_mtl_amd._lib import parse_header

    table, protos = launch_guard.const_table(), parse_header()
    assert set(table) == set(protos) and len(table) > 100
    pointers = 0
    for name, (_, argtypes, argnames) in protos.items():
        want = [n for n, ty in zip(argnames, argtypes) if ty is ctypes.c_void_p]
        assert list(table[name]) == want, name
        pointers += len(want)
        assert not table[name].get("stream", False), name  # the stream handle is never const
    assert pointers > 500
    up2 = table["vmtl_conv2d_up2_halo"]
    assert up2 == {"xl": True, "skip": True, "wp_eff": True, "y": False, "stats": False, "stream": False}
    assert table["vmtl_pack_weights_batch"]["descs"] and table["vmtl_bn_eval_stats_batch"]["descs"]
    assert table["vmtl_timestamp"] == {"out": False, "stream": False}
    assert (launch_guard.GUARD_BYTES, launch_guard.ALIGN) == (4 * poison.GUARD, 256)
