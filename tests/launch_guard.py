"""Test-only harness: every POINTER ARGUMENT of every launch sits between two NaN guard bands (tests/poison.py covers
only the buffers an autograd node allocates through ops._empty; this covers what a kernel is HANDED - operands built by
a test, outputs of the tests that call the C ABI directly, statistics rows, targets, descriptor tables).

All launches go through one function, _Lib.callk.  patched() wraps it on the loaded instance and restores it on exit,
also after an exception.  Per launch, before callk turns tensors into pointers:

  * the tensor arguments are grouped by underlying storage;
  * each group is moved into a fresh byte buffer [GUARD | copy of the whole storage | GUARD] whose guards hold
    poison.SENTINEL (poison.GUARD floats on each side), and each argument is rebuilt as a view at the same byte offset
    inside the copy - so a tensor that owns its storage sits tightly between two NaN bands, and arguments that alias
    (in-place launches, two views of one buffer) move together and keep aliasing;
  * the relocated pointer equals the original modulo 256 (ALIGN): kernels choose vector or scalar paths by alignment,
    and a relocation that changed data_ptr() % 16 would silently test another path;
  * bytes are copied, not floats: arguments are fp32, int64, uint8, bool, uint16, int32 and raw descriptor tables.
    A descriptor table (vmtl_pack_weights_batch, vmtl_bn_eval_stats_batch) is relocated as a byte blob; THE ADDRESSES
    STORED INSIDE IT ARE NOT FOLLOWED - the tensors they name stay where they are, unguarded.

After the launch, const-ness per parameter read from include/vmtl.h (const_table):

  * a group holding any non-const argument is copied back whole to the original storage;
  * a group of only const arguments is NOT copied back: it is compared with the original bit for bit, so a store
    through a pointer the header declares const is reported by entry point and parameter name;
  * all guards are compared with the sentinel.

Copies and checks are queued on the current stream - the stream ops._k passes to the launch, side streams included -
and every check writes one slot of a device-side record; there is no synchronisation per launch.  The relocated buffers
are released as soon as their checks are queued (the caching allocator reuses a block in stream order).  close()
synchronises once and raises ONE AssertionError naming every violated launch: entry point, parameter(s), side, and the
first offset relative to the payload (the copy of the storage).

Left in place, counted by reason (REASONS is closed; anything else raises):
  "partial"   while another stream is active: a group whose non-const argument does not span its whole storage (arena
              slots, out= slices, a test's own guard-banded buffers), together with the const arguments of that
              storage - another stream may be writing the rest of the storage.  "Active" is what the harness can see:
              since patched() began, a launch named, or ran under, a second stream handle.  Until then such a group is
              moved like any other, with two differences: only the byte ranges the non-const arguments address are
              copied back, and the rest of the copy is then compared with the original, so a store next to the
              argument inside its storage is reported instead of being carried home;
  "stream"    every pointer of a launch whose `stream` keyword is not the current torch stream;
  "capturing" every pointer of a launch while the current stream is capturing;
  "null"      a None argument: it stays NULL.

What the harness cannot see: an over-read whose value is discarded (a select after the load) leaves no trace; so does
any read that stays inside a storage larger than the tensor (a view into a bigger buffer is surrounded by that buffer,
not by NaN); so does anything reached through an address inside a descriptor table.  A store outside an argument that
spans its storage up to stride gaps is copied back like any other byte.  The harness only reports: it never zeroes or masks
anything, and every byte it lets a kernel touch is allocated memory."""
import contextlib
import re
from pathlib import Path

import torch

from tests import poison

ALIGN = 256
GUARD_BYTES = 4 * poison.GUARD
REASONS = ("partial", "stream", "capturing", "null")
HEADER = Path(__file__).resolve().parent.parent / "include" / "vmtl.h"

_CLEAN = 1 << 62     # what a check records when every byte compared equal
_CHUNK = 4096        # record slots per device tensor


def const_table(text=None):
    """{entry point: {pointer parameter: declared const?}} for every prototype of the header (include/vmtl.h unless
    `text` is given), in the header's parameter order.  Same grammar as vision_mtl_amd._lib.parse_header, which drops
    the qualifier."""
    if text is None:
        text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    table = {}
    for m in re.finditer(r"(const char\*|long long|int)\s+(vmtl_\w+)\s*\(([^)]*)\)\s*;", text):
        name, args = m.group(2), m.group(3).strip()
        ptrs = {}
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    pointee, param = a.rsplit("*", 1)
                    # `const T* p` / `T const* p`: the POINTEE is const; `T* const p` (a const pointer) is not
                    ptrs[param.replace("const", "").strip()] = bool(re.search(r"\bconst\b", pointee))
        table[name] = ptrs
    return table


def _sentinel_bytes(n, device):
    t = torch.empty((n + 3) // 4, dtype=torch.int32, device=device)
    t.fill_(poison.SENTINEL)
    return t.view(torch.uint8)


def _extent(t):
    """[lo, hi) in bytes, relative to the start of the storage, of the elements t addresses."""
    if t.numel() == 0:
        return None
    lo = t.storage_offset()
    hi = lo + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return lo * t.element_size(), hi * t.element_size()


class _Group:
    """The tensor arguments of one launch that share a storage."""

    def __init__(self, storage):
        self.storage = storage
        self.params = []  # [(parameter name, tensor, const?)]

    def names(self, const=None):
        return ", ".join(n for n, _, c in self.params if const is None or c == const)

    def writable_spans_storage(self):
        n = self.storage.nbytes()
        return all(c or _extent(t) in (None, (0, n)) or n == 0 for _, t, c in self.params)

    def writable_ranges(self):
        """The byte ranges of the storage that the non-const arguments address, merged."""
        out = []
        for lo, hi in sorted(_extent(t) for _, t, c in self.params if not c and _extent(t)):
            if out and lo <= out[-1][1]:
                out[-1][1] = max(out[-1][1], hi)
            else:
                out.append([lo, hi])
        return out


class LaunchGuard:
    def __init__(self, lib, consts, current_stream=None, capturing=None):
        self.lib = lib
        self.consts = consts
        self.current_stream = current_stream or (lambda: torch.cuda.current_stream().cuda_stream)
        self.capturing = capturing or (lambda: torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())
        self.launches = 0
        self.pointers = 0      # pointer arguments seen (tensors and None; the `stream` handle is not one)
        self.relocated = 0
        self.left = dict.fromkeys(REASONS, 0)
        self.streams = set()   # every stream handle a launch named or ran under: more than one = "another stream is active"
        self._recs = {}        # device -> [record tensors]
        self._what = {}        # device -> [description per record slot]
        self._pattern = {}     # device -> sentinel bytes, long enough for any guard

    # ------------------------------------------------------------------------------------------------- device record
    def _record(self, a, b, what):
        """Queue `first byte index at which a != b` (else _CLEAN) into the next record slot; `what(index)` words it."""
        dev = a.device
        recs, desc = self._recs.setdefault(dev, []), self._what.setdefault(dev, [])
        k = len(desc)
        if k == _CHUNK * len(recs):
            if dev.type == "cuda":  # a fresh block may still be in use on the stream that freed it: once per chunk
                torch.cuda.synchronize(dev)
            recs.append(torch.empty(_CHUNK, dtype=torch.int64, device=dev))
        if a.numel():
            differs, index = (a != b).view(torch.uint8).max(dim=0)  # of equal maxima, max(dim) returns the first
            first = torch.where(differs.bool(), index, _CLEAN)
        else:
            first = torch.tensor(_CLEAN, device=dev)
        recs[-1][k % _CHUNK].copy_(first)
        desc.append(what)

    # ------------------------------------------------------------------------------------------------------ one launch
    def callk(self, orig, name, kw):
        consts = self.consts[name]
        self.launches += 1
        groups, nulls = {}, 0
        for p, v in kw.items():
            if isinstance(v, torch.Tensor):
                if p not in consts:
                    raise TypeError(f"{name}: a tensor for `{p}`, which include/vmtl.h does not declare as a pointer")
                if v.device.type == "cpu" and torch.cuda.is_available() and v.is_pinned():
                    raise TypeError(f"{name}: `{p}` is pinned host memory, which a copy would not be")
                st = v.untyped_storage()
                key = (v.device, st.data_ptr(), st.nbytes()) if st.nbytes() else ("empty", id(v))
                groups.setdefault(key, _Group(st)).params.append((p, v, consts[p]))
            elif v is None:
                if p not in consts:
                    raise TypeError(f"{name}: None for `{p}`, which include/vmtl.h does not declare as a pointer")
                nulls += 1
            elif not isinstance(v, (int, float)):
                raise TypeError(f"{name}: `{p}` is a {type(v).__name__}: neither a tensor, None nor a number")
        ntens = sum(len(g.params) for g in groups.values())
        self.pointers += ntens + nulls
        self.left["null"] += nulls
        if not groups:
            return orig(name, **kw)
        if self.capturing():
            self.left["capturing"] += ntens
            return orig(name, **kw)
        self.streams.update({self.current_stream(), kw.get("stream", self.current_stream())})
        if "stream" in kw and kw["stream"] != self.current_stream():
            self.left["stream"] += ntens
            return orig(name, **kw)

        kw = dict(kw)
        moved = []  # (group, buffer, payload offset, payload bytes)
        for g in groups.values():
            g.partial = not g.writable_spans_storage()
            if g.partial and len(self.streams) > 1:
                self.left["partial"] += len(g.params)
                continue
            moved.append(self._relocate(g, kw))
            self.relocated += len(g.params)
        try:
            orig(name, **kw)
        finally:
            for g, buf, off, n in moved:
                home = self._bytes_of(g.storage, g.params[0][1])
                if g.partial:  # only what the arguments address goes back: the rest of the storage is not this launch's
                    for lo, hi in g.writable_ranges():
                        home[lo:hi].copy_(buf[off + lo:off + hi])
                elif any(not c for _, _, c in g.params):
                    home.copy_(buf[off:off + n])
        for g, buf, off, n in moved:
            self._check(name, g, buf, off, n)

    @staticmethod
    def _bytes_of(storage, like):
        return torch.empty(0, dtype=torch.uint8, device=like.device).set_(storage, 0, (storage.nbytes(),), (1,))

    def _relocate(self, g, kw):
        like = g.params[0][1]
        n = g.storage.nbytes()
        buf = _sentinel_bytes(2 * GUARD_BYTES + n + ALIGN, like.device)
        # the payload starts GUARD_BYTES + pad in, pad < ALIGN chosen so that every pointer keeps its residue mod ALIGN
        off = GUARD_BYTES + (g.storage.data_ptr() - buf.data_ptr() - GUARD_BYTES) % ALIGN
        assert off % 8 == 0, "storages are expected to be 8-byte aligned"
        if n:
            buf[off:off + n].copy_(self._bytes_of(g.storage, like))
        base = buf.storage_offset() + off
        for p, t, _ in g.params:
            es = t.element_size()
            view = torch.empty(0, dtype=t.dtype, device=t.device).set_(
                buf.untyped_storage(), base // es + t.storage_offset(), t.shape, t.stride())
            assert view.data_ptr() % ALIGN == t.data_ptr() % ALIGN or t.numel() == 0, (p, view.data_ptr(), t.data_ptr())
            kw[p] = view
        return g, buf, off, n

    def _check(self, name, g, buf, off, n):
        dev = buf.device
        pat = self._pattern.get(dev)
        if pat is None:
            pat = self._pattern[dev] = _sentinel_bytes(GUARD_BYTES + 2 * ALIGN, dev)
        launch = self.launches
        who = f"launch #{launch} {name}({g.names()})"
        self._record(buf[:off], pat[:off], lambda i: (
            f"{who}: store BEFORE the storage, the first at byte offset {i - off} (float offset {(i - off) // 4}) "
            f"of the payload"))
        tail = buf[off + n:]
        ph = (off + n) % 4
        self._record(tail, pat[ph:ph + tail.numel()], lambda i: (
            f"{who}: store AFTER the storage, the first at byte offset {n + i} (float offset {(n + i) // 4}) "
            f"of the payload of {n} bytes"))
        if n and all(c for _, _, c in g.params):
            def const_msg(i):
                hit = [p for p, t, _ in g.params if _extent(t) and _extent(t)[0] <= i < _extent(t)[1]]
                return (f"launch #{launch} {name}: store through const parameter(s) "
                        f"{', '.join(hit) if hit else g.names() + ' (outside the argument, inside its storage)'}"
                        f", the first at byte offset {i} (float offset {i // 4}) of the storage")
            self._record(buf[off:off + n], self._bytes_of(g.storage, g.params[0][1]), const_msg)
        elif g.partial:  # after the copy-back of the arguments' own bytes, any difference is a store next to them
            self._record(buf[off:off + n], self._bytes_of(g.storage, g.params[0][1]), lambda i: (
                f"launch #{launch} {name}: store outside the writable argument(s) {g.names(const=False)}, inside their "
                f"storage, the first at byte offset {i} (float offset {i // 4}) of the storage"))

    # ----------------------------------------------------------------------------------------------------------- end
    def violations(self):
        found = []
        for dev, desc in self._what.items():
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            vals = torch.cat([r for r in self._recs[dev]])[:len(desc)].tolist() if desc else []
            found += [what(v) for v, what in zip(vals, desc) if v != _CLEAN]
        return found

    def close(self):
        try:
            found = self.violations()
        finally:
            self._recs, self._what = {}, {}
        assert not found, "kernels wrote where they must not:\n  " + "\n  ".join(found)

    def counts(self):
        left = ", ".join(f"{r} {self.left[r]}" for r in REASONS)
        return (f"{self.launches} launches, {self.pointers} pointer arguments: {self.relocated} relocated between guards, "
                f"left in place: {left}")


@contextlib.contextmanager
def patched(lib=None, header=None, current_stream=None, capturing=None):
    """callk of the loaded _Lib instance (or of `lib`, a stand-in) wrapped for the duration of the block; guards and
    const operands are checked when the block ends normally (after an exception inside the block only the patch is
    undone: the first failure is the one reported)."""
    if lib is None:
        from vision_mtl_amd._lib import lib as loaded

        lib = loaded()
    g = LaunchGuard(lib, const_table(header), current_stream, capturing)
    had = "callk" in vars(lib)
    orig = lib.callk

    def callk(name, **kw):
        return g.callk(orig, name, kw)

    lib.callk = callk
    try:
        yield g
    except BaseException:
        g._recs, g._what = {}, {}
        raise
    else:
        g.close()
    finally:
        if had:
            lib.callk = orig
        else:
            del lib.callk
