"""Test-only harness: every fp32 buffer the autograd nodes of vision_mtl_amd/ops.py hand to a kernel comes from
ops._empty.  patched(mode) replaces it (a module attribute, so ops._grad_buf follows) and restores it on exit.

  "poison" : a tensor of exactly the requested shape with its own storage at offset 0 (the two nodes that inspect the
             storage of a gradient, _ToNCHW.backward and _DecoderTail.backward, still take it in place), every element
             set to the quiet-NaN bit pattern SENTINEL through an int32 view.
  "guard"  : the same poison, but the tensor is a view of [GUARD | payload | GUARD] inside a larger buffer whose guard
             words hold the sentinel too.  close() synchronises the device, compares both guards of every buffer
             bit-for-bit with the sentinel and raises ONE AssertionError naming every violated buffer.

Why a NaN: a read of an element no kernel wrote, or of a guard word, that reaches any result turns that result into
NaN, and the suite's comparators (tests.util.assert_close, torch.equal, `== 0.0` on a pad-lane maximum) all fail on
NaN.  The harness only reports: it never pre-zeroes a buffer and never masks a NaN in an output.

The fill is queued on the current stream at allocation, where torch.empty itself would be ordered.  Not for use under
graph capture (the guard buffers are freed on close, and the fill would become part of the graph)."""
import contextlib

import torch

SENTINEL = 0x7FC0BEEF  # a quiet NaN (exponent all ones, top mantissa bit set) that no kernel produces by itself
GUARD = 1024           # floats on each side of a guarded payload: a design choice, not a measurement - 4096 bytes, a
                       # multiple of 256, so the payload keeps the alignment the allocator gave the buffer

MODES = ("poison", "guard")


def _shape(shape):
    return (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Poison:
    """The replacement for ops._empty and the record of what it handed out.  Use patched() unless a test needs the
    object without touching ops."""

    def __init__(self, mode):
        if mode not in MODES:
            raise ValueError(f"poison mode {mode!r}: expected one of {MODES}")
        self.mode = mode
        self.bases = []  # guard mode: (int32 base buffer, payload shape, payload element count), alive until close()
        self.count = 0   # buffers handed out

    def empty(self, shape, like):
        """What ops._empty(shape, like) returns: fp32, on like's device, shape as requested."""
        shape = _shape(shape)
        n = _numel(shape)
        self.count += 1
        if self.mode == "poison":
            t = torch.empty(shape, dtype=torch.float32, device=like.device)
            t.view(torch.int32).fill_(SENTINEL)
            return t
        base = torch.empty((n + 2 * GUARD,), dtype=torch.int32, device=like.device)
        base.fill_(SENTINEL)
        self.bases.append((base, shape, n))
        return base[GUARD:GUARD + n].view(torch.float32).view(shape)

    def violations(self):
        """One line per guard that no longer holds the sentinel (synchronises the devices in use first)."""
        for dev in {b.device for b, _, _ in self.bases if b.is_cuda}:
            torch.cuda.synchronize(dev)
        found = []
        for k, (base, shape, n) in enumerate(self.bases):
            for side, words in (("before", base[:GUARD]), ("after", base[GUARD + n:])):
                bad = (words != SENTINEL).nonzero().flatten()
                if bad.numel():
                    # offsets count from the payload: -1 is the float just before it, numel the one just after it
                    first = int(bad[0]) - GUARD if side == "before" else n + int(bad[0])
                    found.append(f"buffer #{k} of shape {shape}: {bad.numel()} guard word(s) {side} the payload "
                                 f"overwritten, the first at float offset {first} of the payload")
        return found

    def close(self):
        try:
            found = self.violations()
        finally:
            self.bases = []
        assert not found, "stores outside a buffer handed out by ops._empty:\n  " + "\n  ".join(found)


@contextlib.contextmanager
def patched(mode="guard"):
    """ops._empty replaced for the duration of the block; in guard mode the guards are checked when the block ends
    normally (after an exception inside the block only the patch is undone: the first failure is the one reported)."""
    from vision_mtl_amd import ops

    p = Poison(mode)
    orig = ops._empty
    ops._empty = p.empty
    try:
        yield p
    except BaseException:
        p.bases = []
        raise
    else:
        p.close()
    finally:
        ops._empty = orig


def is_sentinel(t):
    """Boolean mask of the elements of an fp32 tensor that still hold the sentinel bit pattern."""
    return t.contiguous().view(torch.int32) == SENTINEL
