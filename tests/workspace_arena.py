"""A stand-in for ops._workspace that hands every caller exactly the bytes it asked for, between two guard bands, with a
chosen byte pattern inside (tests/test_gpu_workspace.py; the CPU checks of the helper itself are in
tests/test_workspace_sizes_host.py).

Production keeps one grow-only buffer of at least 1 MiB per (device, stream) and passes its whole size as ws_bytes, so
an operator that writes past what its size query reported, reads scratch it never wrote, or expects bytes to survive
until a later call goes unnoticed there.  Under the arena

  * every call gets a fresh uint8 tensor of GUARD + nbytes + GUARD bytes; the caller sees the view [GUARD, GUARD + nbytes)
    -- 256-byte aligned like the production buffer, since the allocation is and GUARD is a multiple of 256 -- and so
    passes exactly nbytes as ws_bytes;
  * both guards hold 0xA5 and the interior holds `poison`: 0xFF reads as NaN in fp16 / f32 / f64 and as -1 in every
    integer width, 0x00 as zeros;
  * a request of 0 bytes gets the zero-length view (production hands out 1 MiB there);
  * verify() synchronizes, asserts that every guard byte of every call is still 0xA5 -- naming the caller, the
    requested size, the side and the first damaged offset otherwise -- and releases the records.

An overrun lands in allocated guard bytes, not in unmapped memory: it is detected without provoking a fault.
Install with  monkeypatch.setattr(ops, "_workspace", arena);  autograd.py calls ops._workspace through the module, so
the one patch covers it."""
import os
import sys

import torch

GUARD = 1 << 20          # larger than any single tile an operator stores (the cross-encoder's token tile: 128 KiB)
GUARD_BYTE = 0xA5
_THROUGH = ("_loss_ws",)  # helpers that only forward to _workspace: the site of interest is their caller as well


class Arena:
    def __init__(self, poison: int, guard: int = GUARD, verify_every: int = 0):
        """verify_every: verify() (and release) by itself once this many calls are on record -- whole-model cases."""
        assert 0 <= poison <= 255 and guard > 0 and guard % 256 == 0
        self.poison, self.guard, self.verify_every = int(poison), int(guard), int(verify_every)
        self.records = []        # (caller "file:function:line", nbytes, whole tensor)
        self.callers = set()     # (file name, line) of every frame that asked, through _THROUGH helpers as well
        self.calls = 0

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        assert nbytes >= 0, nbytes
        if self.verify_every and len(self.records) >= self.verify_every:
            self.verify()
        frame = sys._getframe(1)
        sites = [frame]
        if frame.f_code.co_name in _THROUGH and frame.f_back is not None:
            sites.append(frame.f_back)
        for f in sites:
            self.callers.add((os.path.basename(f.f_code.co_filename), f.f_lineno))
        f = sites[-1]
        caller = f"{os.path.basename(f.f_code.co_filename)}:{f.f_code.co_name}:{f.f_lineno}"
        g = self.guard
        buf = torch.empty(g + nbytes + g, dtype=torch.uint8, device=device)
        buf[:g].fill_(GUARD_BYTE)
        buf[g + nbytes:].fill_(GUARD_BYTE)
        if nbytes:
            buf[g:g + nbytes].fill_(self.poison)
        self.records.append((caller, nbytes, buf))
        self.calls += 1
        return buf[g:g + nbytes]

    def damage(self):
        """[(caller, nbytes, side, first damaged offset)] over the recorded calls; offsets count from the start of the
        guard concerned (so `after` + 0 is the first byte behind the view)."""
        out = []
        g = self.guard
        for caller, nbytes, buf in self.records:
            for side, band in (("before", buf[:g]), ("after", buf[g + nbytes:])):
                bad = band != GUARD_BYTE
                if bool(bad.any()):
                    out.append((caller, nbytes, side, int(torch.nonzero(bad)[0, 0])))
        return out

    def verify(self):
        if any(buf.is_cuda for _, _, buf in self.records):
            torch.cuda.synchronize()
        found = self.damage()
        self.records = []
        assert not found, "; ".join(f"{c} asked for {n} bytes and wrote {s} them (first at guard offset {o})"
                                    for c, n, s, o in found)
