"""A sentinel arena: output buffers carved out of one block of memory that is dirty everywhere, so that a store outside
the bytes a caller owns is seen instead of landing in a neighbour's allocation.

Every byte of the arena holds 0xA5.  As a double that pattern is a finite negative number of about 1e-129, which no
model produces; as a status byte it is 165, no PMX_PAIR_* code: one pattern serves every output type and leaves every
output dirty on entry.  ``carve`` hands out strided views with guard zones on both sides, ``assert_clean`` checks that
every byte outside the owned ranges ``[row * ld, row * ld + cols)`` still holds the pattern and says where it does not.

A plain helper: no fixture, no plugin.  Works on "cuda" and on "cpu" (the host-pointer entry points; tests/test_arena.py).
"""
from __future__ import annotations

FILL = 0xA5
ALIGN = 256
MIN_GUARD = 4096


class Region:
    """One carved matrix: ``rows x cols`` elements of ``itemsize`` bytes, rows ``ld`` elements apart, element [0, 0] at
    byte ``start`` of the arena."""

    def __init__(self, name, start, rows, cols, ld, itemsize, guard):
        self.name, self.start, self.rows, self.cols, self.ld, self.itemsize, self.guard = name, start, rows, cols, ld, itemsize, guard
        self.pitch = ld * itemsize
        self.end = start + ((rows - 1) * ld + cols) * itemsize  # one past the last owned byte: the last row owns cols, not ld

    def describe(self, off: int) -> str:
        """Where arena byte ``off`` lies relative to this region."""
        who = f"region '{self.name}' [{self.rows} x {self.cols}, ld {self.ld}, {self.itemsize}-byte elements]"
        if off < self.start:
            return f"{who}: before the first row, {self.start - off} byte(s) in front of element [0, 0]"
        if off >= self.end:
            return (f"{who}: after the last row, {off - self.end} byte(s) past the last column of row {self.rows - 1} "
                    f"(element [{self.rows - 1}, {self.cols - 1}] is the last one owned)")
        rel = off - self.start
        row, col, byte = rel // self.pitch, (rel % self.pitch) // self.itemsize, rel % self.itemsize
        kind = "padding" if col >= self.cols else "OWNED"
        return (f"{who}: row {row}, column {col}, byte {byte} of the element ({kind}: {col - self.cols + 1} element(s) "
                f"past the row's last column {self.cols - 1})")


class Arena:
    def __init__(self, device, n_bytes: int):
        import torch

        self.torch = torch
        self.n_bytes = int(n_bytes)
        raw = torch.empty(self.n_bytes + ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % ALIGN  # (a device allocation starts aligned; the CPU allocator promises 64 bytes only)
        self.buf = raw[skip:skip + self.n_bytes]
        assert self.buf.data_ptr() % ALIGN == 0
        self.owned = torch.zeros(self.n_bytes, dtype=torch.bool, device=device)
        self.regions = []
        self.cursor = 0
        self.buf.fill_(FILL)

    def reset(self) -> None:
        """Refill every byte and forget what was carved."""
        self.buf.fill_(FILL)
        self.owned.zero_()
        self.regions = []
        self.cursor = 0

    def carve(self, rows: int, cols: int, ld: int, dtype, offset_bytes: int = 0, name: str = None):
        """A ``[rows, cols]`` view with row stride ``ld`` whose element [0, 0] sits ``offset_bytes`` past a 256-byte
        boundary, with at least ``max(4096, ld * itemsize)`` untouched bytes on either side of what it owns."""
        torch = self.torch
        itemsize = torch.empty((), dtype=dtype).element_size()
        assert rows >= 1 and cols >= 1 and ld >= cols and 0 <= offset_bytes < ALIGN and offset_bytes % itemsize == 0
        guard = max(MIN_GUARD, ld * itemsize)
        gap = max(guard, self.regions[-1].guard if self.regions else 0)  # a row of either neighbour fits in between
        start = (self.cursor + gap + ALIGN - 1) // ALIGN * ALIGN + offset_bytes
        reg = Region(name or f"r{len(self.regions)}", start, rows, cols, ld, itemsize, guard)
        assert reg.end + guard <= self.n_bytes, f"arena of {self.n_bytes} bytes is too small for region '{reg.name}'"
        self.cursor = reg.end
        self.regions.append(reg)
        self.owned.as_strided((rows, cols * itemsize), (reg.pitch, 1), start).fill_(True)
        span = self.buf[start:reg.end].view(dtype)
        view = span.as_strided((rows, cols), (ld, 1))
        assert view.data_ptr() == self.buf.data_ptr() + start
        return view

    def _describe(self, off: int) -> str:
        inside = [r for r in self.regions if r.start - r.guard <= off < r.end + r.guard]
        pool = inside or self.regions
        if not pool:
            return f"arena byte {off} (nothing carved)"
        near = min(pool, key=lambda r: 0 if r.start <= off < r.end else min(abs(off - r.start), abs(off - (r.end - 1))))
        return f"arena byte {off}: " + near.describe(off)

    def assert_clean(self) -> None:
        """Every byte outside the owned ranges still holds the pattern."""
        stray = ((self.buf != FILL) & ~self.owned).nonzero().flatten()
        if stray.numel() == 0:
            return
        first, last = int(stray[0]), int(stray[-1])
        raise AssertionError(f"{stray.numel()} byte(s) outside the owned ranges were written\n"
                             f"  first: {self._describe(first)} (now 0x{int(self.buf[first]):02x})\n"
                             f"  last:  {self._describe(last)} (now 0x{int(self.buf[last]):02x})")
