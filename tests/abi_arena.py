"""TEST INFRASTRUCTURE ONLY — guarded, poisoned output buffers for tests that
call the raw C ABI (include/g2k_hip.h states a write footprint per entry
point: "every element written", "others untouched", "columns >= n_active are
zero"; a torch.zeros / torch.empty output cannot tell a kernel that keeps such
a sentence from one that does not).

An ``Arena`` hands out every output as the payload view of ONE tensor
``[front guard | payload | back guard]`` filled with a fixed bit pattern:

* each guard is ``GUARD_BYTES`` = 256 bytes, so the payload keeps the 16-byte
  alignment of the allocation (the ABI's strictest requirement);
* float32: a quiet NaN with a recognisable payload (0x7FC0BEEF), compared
  bitwise through an int32 view since NaN != NaN; int32: 0x5EEDBEEF; uint8:
  0xA5 (no value any entry point writes: masks are 0 / 1);
* ``check_guards()`` asserts every guard word still holds the pattern (a store
  past either end of a buffer would otherwise land in allocator slack);
* ``untouched(view[, index])`` / ``all_written(view)`` compare the payload's
  bits with the pattern.

The tests build their inputs with the inactive parts (columns >= n_active,
frames >= n_frames) holding NaN: an output that stays finite proves the kernel
never read them, not even through a multiply by zero.  Works on CPU tensors
too (tests/test_abi_arena.py).
"""
import numpy as np
import torch

GUARD_BYTES = 256
PATTERNS = {torch.float32: 0x7FC0BEEF, torch.int32: 0x5EEDBEEF, torch.uint8: 0xA5}
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8}


def bits(t):
    """The tensor's bits as integers (same shape, no copy)."""
    return t.view(_BITS[t.dtype])


class Arena:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self._blocks = []          # (name, whole tensor, guard elements, payload elements)

    def alloc(self, shape, dtype=torch.float32, name=None):
        """A pattern-filled payload of ``shape`` between two guards."""
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64))
        g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        whole = torch.empty(g + n + g, dtype=dtype, device=self.device)
        bits(whole).fill_(PATTERNS[dtype])
        self._blocks.append((name or f"buf{len(self._blocks)}", whole, g, n))
        return whole[g:g + n].view(shape)

    def put(self, array, name=None):
        """A guarded in/out buffer holding ``array`` (h, params, ms, state)."""
        src = torch.from_numpy(np.ascontiguousarray(array))
        view = self.alloc(src.shape, src.dtype, name)
        view.copy_(src)
        return view

    def check_guards(self):
        for name, whole, g, n in self._blocks:
            pat = PATTERNS[whole.dtype]
            for side, part in (("front", whole[:g]), ("back", whole[g + n:])):
                bad = (bits(part) != pat).nonzero().flatten()
                assert bad.numel() == 0, (
                    f"{name}: {bad.numel()} {side} guard word(s) overwritten, first at guard "
                    f"element {int(bad[0])} (payload of {n} elements)")


def untouched(view, index=None):
    """Boolean tensor: True where ``view[index]`` still holds the pattern."""
    v = view if index is None else view[index]
    return bits(v) == PATTERNS[view.dtype]


def all_written(view):
    """No payload element holds the pattern any more."""
    return not bool(untouched(view).any())

