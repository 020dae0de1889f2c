"""A guarded arena for calls through the C ABI: ONE allocation, carved into named buffers with a guard band before and behind
each, so that a kernel that writes outside what its prototype names -- or into an input -- is caught by a byte comparison (GPU
AddressSanitizer is not available for these kernels; tests/test_hip_abi_contract.py is the user, tests/test_abi_arena.py tests
the logic on CPU tensors, which work the same way).

    arena = Arena(device, guard_byte=1)
    arena.add("X", R * ldx, role="in", misalign=3)        # exactly R * ldx bytes, 3 bytes past a 256-byte boundary
    arena.add("H", R * S * 2, role="out", align=16)
    arena.build()
    arena.write("X", x_bytes); arena.fill("H", 0xFF)
    arena.snapshot()
    ... the call, with arena.ptr(name) ...
    arena.check()                                         # AssertionError naming the buffer, the side and the damaged offsets

Every buffer is sized exactly (the guard behind it starts at its last byte + 1).  A guard is GUARD bytes or more: larger than
any tile a kernel stages or stores at once, so that a store that misses its buffer by a row, a tile or a 16-byte vector lands
in a guard and not in the next buffer.  Guards are filled with `guard_byte`: not 0x00 or 0xFF (what stale or cleared memory
holds) and, as int8, a valid state of the case's model -- a stray READ of a guard as states then shows in the counts.
What a guard band cannot see: a read outside a buffer that changes no result."""
import ctypes as C

import numpy as np
import torch

GUARD = 64 * 1024
ROLES = ("in", "out", "ws")          # in: must be bit-identical after the call; out / ws: the call may write them


class Arena:
    def __init__(self, device, guard_byte=1, guard=GUARD):
        if guard < GUARD:
            raise ValueError("a guard band of at least %d bytes is a condition of the arena" % GUARD)
        if guard_byte in (0x00, 0xFF) or not 0 < guard_byte < 128:
            raise ValueError("the guard byte must not be 0x00 or 0xFF and must be a state as int8")
        self.device, self.guard_byte, self.guard = torch.device(device), guard_byte, guard
        self.specs, self.at, self.mem, self.snap, self.frozen = [], {}, None, None, ()

    # ---- layout
    def add(self, name, nbytes, role="out", align=256, misalign=0):
        """A buffer of exactly `nbytes` bytes whose address is `misalign` bytes past a multiple of `align`."""
        if self.mem is not None:
            raise RuntimeError("the arena is built")
        if role not in ROLES or name in [s[0] for s in self.specs] or nbytes < 0 or not 0 <= misalign < align:
            raise ValueError("bad buffer %r" % (name,))
        self.specs.append((name, int(nbytes), role, int(align), int(misalign)))

    def build(self):
        total = 2 * self.guard + sum(n + 2 * self.guard + 2 * a for _name, n, _r, a, _m in self.specs) + 256
        self.mem = torch.empty(total, dtype=torch.uint8, device=self.device)
        base = self.mem.data_ptr()
        cur = 0
        for name, n, role, align, mis in self.specs:
            start = (base + cur + 2 * self.guard + align - 1) // align * align + mis - base      # a guard of its own on either side
            self.at[name] = (start, start + n, role)
            cur = start + n
        assert cur + self.guard <= total
        self.order = sorted(self.at, key=lambda k: self.at[k][0])
        self.reset()
        return self

    def reset(self):
        """Every byte of the arena, buffers included, back to the guard byte."""
        self.mem.fill_(self.guard_byte)
        self.snap = None

    # ---- access
    def nbytes(self, name):
        return self.at[name][1] - self.at[name][0]

    def ptr(self, name):
        return C.c_void_p(self.mem.data_ptr() + self.at[name][0])

    def addr(self, name):
        return self.mem.data_ptr() + self.at[name][0]

    def bytes(self, name):
        """The buffer as a uint8 view of the arena."""
        a, b, _ = self.at[name]
        return self.mem[a:b]

    def write(self, name, array):
        """Host array (any dtype) -> the buffer, byte for byte; the sizes must agree exactly."""
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        if raw.size != self.nbytes(name):
            raise ValueError("%s holds %d bytes, got %d" % (name, self.nbytes(name), raw.size))
        self.bytes(name).copy_(torch.from_numpy(raw.copy()))

    def read(self, name, dtype=np.uint8):
        """The buffer as a host array of `dtype` (a copy)."""
        return self.bytes(name).cpu().numpy().copy().view(dtype)

    def fill(self, name, how, rng=None):
        """Prefill a buffer: an int = that byte, "random" = bytes of `rng`."""
        if how == "random":
            self.bytes(name).copy_(torch.from_numpy(rng.integers(0, 256, size=self.nbytes(name), dtype=np.uint8)))
        else:
            self.bytes(name).fill_(int(how))

    def guards(self, name):
        """(before, behind): the two guard bands of a buffer as uint8 views (GUARD bytes each, next to the buffer)."""
        a, b, _ = self.at[name]
        return self.mem[a - self.guard:a], self.mem[b:b + self.guard]

    def poison_guards(self, name, pattern):
        """Tile `pattern` (host uint8 array) through both guards of a buffer, in phase with the buffer's first byte -- a float32
        pattern is then a whole float wherever a kernel would read one next to the buffer."""
        a, b, _ = self.at[name]
        pattern = np.asarray(pattern, dtype=np.uint8)
        for lo, hi in ((a - self.guard, a), (b, b + self.guard)):
            idx = (np.arange(lo, hi) - a) % pattern.size
            self.mem[lo:hi].copy_(torch.from_numpy(pattern[idx]))

    # ---- the check
    def snapshot(self, frozen=()):
        """Remember every byte.  check() then wants everything outside the out / ws buffers unchanged; `frozen` names out / ws
        buffers that must stay unchanged too (an output the call was told not to produce)."""
        unknown = [f for f in frozen if f not in self.at]
        if unknown:
            raise ValueError("unknown buffers %r" % unknown)
        self.snap, self.frozen = self.mem.clone(), tuple(frozen)

    def _regions(self):
        """(lo, hi, buffer, side) covering the arena: a buffer itself ("input") and, around it, the bytes nearer to its edges
        than to any other buffer's ("before" / "behind")."""
        out, prev_end, prev = [], 0, None
        for name in self.order:
            a, b, _ = self.at[name]
            mid = prev_end if prev is None else (prev_end + a + 1) // 2
            if prev is not None:
                out.append((prev_end, mid, prev, "behind"))
            out.append((mid, a, name, "before"))
            out.append((a, b, name, "input"))
            prev_end, prev = b, name
        if prev is not None:
            out.append((prev_end, self.mem.numel(), prev, "behind"))
        return out

    def check(self):
        if self.snap is None:
            raise RuntimeError("check() without snapshot()")
        diff = self.mem != self.snap
        for name in self.order:
            a, b, role = self.at[name]
            if role != "in" and name not in self.frozen:
                diff[a:b] = False
        if not bool(diff.any()):
            return
        report = []
        for lo, hi, name, side in self._regions():
            if hi <= lo or not bool(diff[lo:hi].any()):
                continue
            where = torch.nonzero(diff[lo:hi]).reshape(-1)
            first, last, n = lo + int(where[0]), lo + int(where[-1]), int(where.numel())
            a, b, role = self.at[name]
            ref = b if side == "behind" else a
            what = ("input buffer %r changed" % name if side == "input" and role == "in" else
                    "buffer %r was written although the call was told not to produce it" % name if side == "input" else
                    "guard %s buffer %r damaged" % (side, name))
            report.append("%s: %d byte(s), first at offset %+d, last at offset %+d (relative to the buffer's %s)" % (
                what, n, first - ref, last - ref, "end" if side == "behind" else "start"))
        raise AssertionError("; ".join(report))
