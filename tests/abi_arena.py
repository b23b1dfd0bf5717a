"""TEST INFRASTRUCTURE ONLY — guarded, poisoned output buffers for tests that
call the raw C ABI (include/g2k_hip.h states a write footprint per entry
point: "every element written", "others untouched", "columns >= n_active are
zero"; a torch.zeros / torch.empty output cannot tell a kernel that keeps such
a sentence from one that does not).

An ``Arena`` hands out every output as the payload view of ONE tensor
``[front guard | payload | back guard]`` filled with a fixed bit pattern:

* each guard is at least ``GUARD_BYTES`` = 256 bytes, and the payload starts
  on a 16-byte boundary (the ABI's strictest requirement) or, with
  ``offset=k`` (a multiple of the element size below 16), exactly ``k`` bytes
  past one: the weakest alignment an entry point accepts for an argument
  (tests/abi_alignment.py) is then what it is given — the front guard grows
  by the bytes that takes, and both guards are checked as before;
* float32: a quiet NaN with a recognisable payload (0x7FC0BEEF), compared
  bitwise through an int32 view since NaN != NaN; int32: 0x5EEDBEEF; uint8:
  0xA5 (no value any entry point writes: masks are 0 / 1); float64 / int64:
  a quiet NaN 0x7FF8BEEF0000BEEF / 0x5EEDBEEF5EEDBEEF, compared through int64;
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
PATTERNS = {torch.float32: 0x7FC0BEEF, torch.int32: 0x5EEDBEEF, torch.uint8: 0xA5,
            torch.float64: 0x7FF8BEEF0000BEEF, torch.int64: 0x5EEDBEEF5EEDBEEF}
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8,
         torch.float64: torch.int64, torch.int64: torch.int64}


def bits(t):
    """The tensor's bits as integers (same shape, no copy)."""
    return t.view(_BITS[t.dtype])


class Arena:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self._blocks = []          # (name, whole tensor, front guard elements, payload elements)

    def alloc(self, shape, dtype=torch.float32, name=None, offset=0):
        """A pattern-filled payload of ``shape`` between two guards, starting
        ``offset`` bytes past a 16-byte boundary."""
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64))
        es = torch.empty((), dtype=dtype).element_size()
        assert 0 <= offset < 16 and offset % es == 0, (offset, es)
        g = GUARD_BYTES // es
        whole = torch.empty(g + 16 // es + n + g, dtype=dtype, device=self.device)
        # whatever the allocator's own alignment: the bytes from the end of a
        # 256-byte front guard to the next address that is `offset` mod 16
        skip = (offset - (whole.data_ptr() + GUARD_BYTES)) % 16
        assert skip % es == 0, (whole.data_ptr(), es)
        lead = g + skip // es
        bits(whole).fill_(PATTERNS[dtype])
        self._blocks.append((name or f"buf{len(self._blocks)}", whole, lead, n))
        view = whole[lead:lead + n].view(shape)
        assert n == 0 or view.data_ptr() % 16 == offset
        return view

    def put(self, array, name=None, offset=0):
        """A guarded buffer holding ``array``: in/out state (h, params, ms) and,
        where a test places them, inputs."""
        src = torch.from_numpy(np.ascontiguousarray(array))
        view = self.alloc(src.shape, src.dtype, name, offset)
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

