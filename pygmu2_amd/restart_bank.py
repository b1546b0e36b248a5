"""
Restart bank: TriggerRestartPE and RandomSelectPE over candidates whose samples depend on the frame index alone.

The composed path (trigger_restart_pe.py) reads the whole trigger block back, then renders the source and copies the
piece once per event.  For a candidate that is a function of the frame index, every one of those short renders is a
prefix of ONE render from local time 0, so a block needs only
  (1) the trigger, scanned on the device (pgx_restart_plan): four integers come back -- how many events, the first, the
      last, the longest stretch -- 32 bytes, one read, counted in `d2h_reads`;
  (2) the owner's selections, one per event, in order (RandomSelectPE draws them from random.Random; TriggerRestartPE has
      one candidate);
  (3) "takes": the stretch that runs in from the previous block, [carry, carry + first) of the active candidate, and
      per DISTINCT candidate selected in this block one render over [0, longest).  Renders are counted in
      `take_renders`;
  (4) one gather (pgx_restart_gather): every frame reads its event's take at the local time since that event.
The samples are the composed path's to the bit: a take is the candidate's own render and the gather copies float32.

What may enter (eligible): read_ahead.eligible -- pure, allow-listed, inputs likewise -- without a PE whose fill rule
depends on where a block starts (IdentityPE beyond 2^24); and SlicePE over such a source: a crop, an integer shift and a
fixed envelope, though the DelayPE it is composed of is not on read-ahead's list.  The candidate's channel count must be
known and equal to the owner's.  One candidate that may not enter keeps its owner on the composed path.

Kept takes: a SlicePE candidate of at most wavetable_pe.KEPT_TABLE_MAX_BYTES (WavetablePE's rule and cap for its table)
is rendered once over its whole extent and stays in HBM until the owner's on_stop / on_start.  Other finite candidates
are not kept and not cut to their extent: a finite extent does not promise silence outside it (ArrayPE's hold modes).
PYGMU_RESTART_BANK=0 (or set_enabled(False)) switches the bank off: both PEs then take the composed path.
"""

from __future__ import annotations

import os

import numpy as np

from . import device as _dev
from . import read_ahead as _read_ahead
from . import wavetable_pe as _wavetable
from ._kernels import DeviceBuffer, check, lib, new_output
from .slice_pe import SlicePE
from .snippet import Snippet

_ENABLED = os.environ.get("PYGMU_RESTART_BANK", "1").strip().lower() not in ("0", "false", "no", "off")


def enabled() -> bool:
    return _ENABLED


def set_enabled(flag: bool) -> None:
    global _ENABLED
    _ENABLED = bool(flag)


def _start_sensitive(pe) -> bool:
    return bool(getattr(pe, "_READ_AHEAD_PERIOD_SENSITIVE", False)) or any(_start_sensitive(c) for c in pe.inputs())


def eligible(pe) -> bool:
    """May `pe` be a candidate of a bank?  (cached on the instance; graphs are static)"""
    cached = pe.__dict__.get("_rb_ok")
    if cached is None:
        core = pe._source if type(pe) is SlicePE else pe
        cached = bool(_read_ahead.eligible(core)) and not _start_sensitive(core)
        pe.__dict__["_rb_ok"] = cached
    return cached


def try_build(trigger, candidates, channels):
    """A RestartBank when the bank is on and every candidate may enter, else None."""
    if not _ENABLED or not candidates:
        return None
    for c in candidates:
        if c.channel_count() != channels or not eligible(c):
            return None
    return RestartBank(trigger, candidates, channels)


class RestartBank:
    def __init__(self, trigger, candidates, channels: int):
        self._trigger = trigger
        self._candidates = list(candidates)
        self._channels = int(channels)
        self.origin: int | None = None           # absolute frame of the latest event; None: nothing has started
        self.d2h_reads = 0                       # device-to-host copies issued (one 32-byte summary per block)
        self.take_renders = 0                    # candidate renders issued
        self._kept: dict[int, Snippet] = {}      # candidate index -> its whole extent, resident
        self._summary: DeviceBuffer | None = None
        self._workspace: DeviceBuffer | None = None
        self._staging = np.zeros(1024, dtype=np.uint8)

    def forget(self) -> None:
        """on_start / on_stop of the owner: nothing runs any more, the kept takes go."""
        self.origin = None
        self._kept.clear()

    # ------------------------------------------------------------------------------------------ takes
    def _keeps(self, index: int) -> bool:
        """Only a SlicePE: its ZERO-mode crop makes it silent outside its extent, which a PE with a finite extent need
        not be (ArrayPE / CropPE hold modes) -- and the gather plays silence outside a take."""
        pe = self._candidates[index]
        ext = pe.extent()
        if type(pe) is not SlicePE or not _wavetable.KEEP_TABLE or ext.start is None or ext.end is None:
            return False
        return 0 < (ext.end - ext.start) * self._channels * 4 <= _wavetable.KEPT_TABLE_MAX_BYTES

    def _take(self, index: int, lo: int, hi: int, keep: list):
        """(device address, first local frame, frames) of candidate `index` over [lo, hi) of its own time (a kept
        candidate: over its whole extent); None where that is empty."""
        pe = self._candidates[index]
        if self._keeps(index):
            ext = pe.extent()
            snip = self._kept.get(index)
            if snip is None:
                snip = self._kept[index] = pe.render(ext.start, ext.end - ext.start)
                self.take_renders += 1
            return snip.dev.ptr, ext.start, ext.end - ext.start
        if hi <= lo:
            return None
        snip = pe.render(lo, hi - lo)
        self.take_renders += 1
        if snip.channels != self._channels:
            raise ValueError(f"{type(pe).__name__} rendered {snip.channels} channels, expected {self._channels}")
        keep.append(snip)
        return snip.dev.ptr, lo, hi - lo

    # ------------------------------------------------------------------------------------------ render
    def render(self, start: int, duration: int, active, choose) -> Snippet:
        """One block.  active: index of the candidate that runs in from the previous block (None: none chosen yet);
        choose(count) -> the candidate index of each of the block's `count` events, in order.  Advances `origin`.
        None, with nothing done, for a block that begins before the running stretch's origin (a pull that goes back, as
        a PE that renders its source twice per block makes): its local times are negative, the composed path serves it."""
        if self.origin is not None and start < self.origin:
            return None
        L = lib()
        trig = self._trigger.render(start, duration)
        trig_dev, stride = trig.dev, trig.channels
        if self._summary is None:
            self._summary = DeviceBuffer((4,), np.int64)
            self._workspace = DeviceBuffer((_dev.RESTART_WORKSPACE_INT64,), np.int64)
        check(L.pgx_restart_plan(self._summary.ptr, self._workspace.ptr, trig_dev.ptr, stride, duration),
              "pgx_restart_plan")
        count, first, last, longest = (int(v) for v in self._summary.to_host())
        self.d2h_reads += 1
        running = self.origin is not None and active is not None and first > 0
        if count == 0 and not running:
            return Snippet.from_zeros(start, duration, self._channels)
        chosen = [int(c) for c in choose(count)] if count else []
        if len(chosen) != count:
            raise RuntimeError(f"restart bank: {len(chosen)} selections for {count} events")
        keep: list = [trig]
        takes, slot_of = [], {}
        sel = np.full(count + 1, -1, dtype=np.int32)
        carry_local = -1
        if running:
            carry_local = start - self.origin
            take = self._take(active, carry_local, carry_local + first, keep)
            if take is not None:
                sel[0] = len(takes)
                takes.append(take)
        for k, c in enumerate(chosen, start=1):
            slot = slot_of.get(c)
            if slot is None:
                take = self._take(c, 0, longest, keep)
                slot = slot_of[c] = -1 if take is None else len(takes)
                if take is not None:
                    takes.append(take)
            sel[k] = slot
        table = np.zeros(max(1, len(takes)), dtype=_dev.RESTART_TAKE)
        for i, take in enumerate(takes):
            table[i] = take
        block, (takes_at, sel_at) = self._upload([table, sel])
        out = new_output(duration, self._channels)
        check(L.pgx_restart_gather(out.ptr, duration, self._channels, trig_dev.ptr, stride, self._workspace.ptr,
                                   carry_local, block.ptr + sel_at, count + 1, block.ptr + takes_at, len(takes)),
              "pgx_restart_gather")
        if count:
            self.origin = start + last
        return Snippet(start, out)

    def _upload(self, parts):
        """The tables, packed 8-byte aligned into the reused staging array, in one copy: (device block, byte offsets)."""
        at, total = [], 0
        for p in parts:
            at.append(total)
            total += (p.nbytes + 7) & ~7
        if total > self._staging.nbytes:
            self._staging = np.zeros(max(total, 2 * self._staging.nbytes), dtype=np.uint8)
        for p, a in zip(parts, at):
            self._staging[a:a + p.nbytes] = p.view(np.uint8).reshape(-1)
        block = DeviceBuffer((total,), np.uint8)
        check(lib().pgx_memcpy_h2d(block.ptr, self._staging.ctypes.data, total), "pgx_memcpy_h2d")
        return block, at
