"""
Score bank: MixPE over notes -- inputs that each sound for a bounded stretch of the timeline (what SequencePE builds,
and what examples 19 and 29 build by hand as MixPE(DelayPE(CropPE(note, 0, len), start), ...)).

MixPE's generic path renders every input whose extent touches the block over the WHOLE block, zero-filled, and adds K
full-length rows.  The bank renders each sounding note over its overlap with the block only and adds the pieces where
they lie (pgx_score_mix): the work is the frames that sound plus the block, not K times the block.

What counts as a note (classify): peel from the outside any number of integer-delay DelayPE and ZERO-mode CropPE
layers; the accumulated window, in the input's own time, must be bounded on both sides and the extent of what is left
(the core) must contain it.  Inside its window each layer passes (start, duration) through, so rendering the input over
block x window pulls the core over exactly the range the generic path pulls it over -- which is what makes the two
paths agree for cores that carry state (KarplusStrongPE, NoisePE).  Every other input (an unbounded tail element, a
fractional or PE delay, a hold-mode crop, a filter whose ring-out leaves its extent) is rendered over the whole block
as before and enters the mix as a segment that covers the block.

Per render: (1) cull -- the notes that intersect the block come from arrays sorted by note start (a binary search for
the last start before the block's end, a running maximum of ends for the first candidate); (2) each sounding note is
rendered over its overlap: a general note through its own render(), the notes whose core is a KarplusStrongPE all in
ONE launch (pgx_karplus_score) from pointers to each string's own line and state, into one packed buffer; (3)
pgx_score_mix adds the segments in input order from per-tile lists.  Up to 16 segments / strings travel in the kernel
arguments; longer tables go up in one copy from a reused staging array.

Floating point: adding a float32 zero leaves a sample as it is (only the sign of a zero can differ), so the bank's sum
over the covering segments in input order equals the generic path's sum over zero-filled rows.
PYGMU_SCORE_BANK=0 (or set_enabled(False)) switches the bank off: MixPE then takes its generic path.
"""

from __future__ import annotations

import os

import numpy as np

from . import device as _dev
from . import diagnostics as _diag
from . import look_ahead as _look_ahead
from ._kernels import DeviceBuffer, check, lib
from .crop_pe import CropPE
from .delay_pe import DelayPE
from .extent import ExtendMode, Extent
from .karplus_strong_pe import KarplusStrongPE
from .snippet import Snippet

TILE = 1024                      # frames per tile of pgx_score_mix
INLINE = _dev.SCORE_INLINE       # tables up to this many entries travel in the kernel arguments
# Strings per workgroup of pgx_karplus_score.  Lanes of one wave that are at different places of their lines diverge (one
# wraps while the other does not: the wave runs both paths), and a lone lane issues as fast as 64, so a string gets a
# wave of its own for as long as the chip has room: 256 CUs x 8 waves of this kernel (its registers allow 2 per SIMD).
# Only a launch of more strings than that packs several into a wave.  A workgroup's lines then fit the 64 KiB of LDS up
# to N = 16 384 / group.  PYGMU_SCORE_KS_GROUP=<n> fixes the group (tools/score_probe.py times 16 and 64 against this).
WAVE_SLOTS = 256 * 8
KS_GROUP = int(os.environ.get("PYGMU_SCORE_KS_GROUP", "0"))


def ks_group(count: int) -> int:
    return KS_GROUP if KS_GROUP else min(64, max(1, -(-count // WAVE_SLOTS)))


_ENABLED = os.environ.get("PYGMU_SCORE_BANK", "1").strip().lower() not in ("0", "false", "no", "off")
STATS = {"renders": 0, "launches": 0, "uploads": 0}     # since the process started (tools/score_probe.py)


def enabled() -> bool:
    return _ENABLED


def set_enabled(flag: bool) -> None:
    global _ENABLED
    _ENABLED = bool(flag)


# ---------------------------------------------------------------------------------------------- what is a note
def classify(pe):
    """(core, shift, lo, hi, chain) when `pe` is a note: it sounds in [lo, hi) of its own time, where it is the core
    at time t - shift; chain = the peeled layers, outermost first.  None otherwise."""
    shift, lo, hi = 0, None, None
    node, chain = pe, []
    while True:
        if type(node) is DelayPE and node._mode == "int":
            shift += node._delay
        elif type(node) is CropPE and node._extend_mode is ExtendMode.ZERO:
            ws, we = node._extent.start, node._extent.end
            if ws is not None:
                lo = ws + shift if lo is None else max(lo, ws + shift)
            if we is not None:
                hi = we + shift if hi is None else min(hi, we + shift)
        else:
            break
        chain.append(node)
        node = node._source
    if lo is None or hi is None:
        return None
    hi = max(lo, hi)                                     # crops that miss each other: an empty note
    if not node.extent().spans(lo - shift, hi - lo):
        return None
    return node, shift, lo, hi, chain


def try_build_score(inputs):
    """A ScoreBank when at least two of `inputs` are notes, else None."""
    if not _ENABLED:
        return None
    notes = [classify(pe) for pe in inputs]
    if sum(n is not None for n in notes) < 2:
        return None
    return ScoreBank(inputs, notes)


# ---------------------------------------------------------------------------------------------- host tables
def cull(starts, ends, run_max, a: int, b: int):
    """Positions (into arrays sorted by start) of the notes [starts[i], ends[i]) that intersect [a, b);
    run_max = np.maximum.accumulate(ends).  One binary search for each end of the candidate range, then the candidates."""
    hi = int(np.searchsorted(starts, b, side="left"))            # starts[i] < b
    lo = int(np.searchsorted(run_max, a, side="right"))          # nothing before lo ends after a
    if lo >= hi:
        return np.zeros(0, dtype=np.int64)
    return lo + np.nonzero(ends[lo:hi] > a)[0]


def tile_lists(first, frames, n_frames: int, tile: int = TILE):
    """CSR over the tiles of a block of n_frames frames: (offsets int32 (tiles + 1), entries int32) with, per tile, the
    indices of the segments [first[i], first[i] + frames[i]) that touch it, ascending.  frames[i] >= 1."""
    first = np.asarray(first, dtype=np.int64)
    frames = np.asarray(frames, dtype=np.int64)
    n_tiles = -(-int(n_frames) // tile)
    t0 = first // tile
    cnt = (first + frames - 1) // tile - t0 + 1
    total = int(cnt.sum())
    seg = np.repeat(np.arange(len(first), dtype=np.int64), cnt)
    tiles = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(t0, cnt)
    order = np.argsort(tiles, kind="stable")                     # entries were made in segment order: it is kept
    offsets = np.zeros(n_tiles + 1, dtype=np.int32)
    np.cumsum(np.bincount(tiles, minlength=n_tiles), out=offsets[1:])
    return offsets, seg[order].astype(np.int32)


class ScoreBank:
    def __init__(self, inputs, notes):
        self._inputs = list(inputs)
        self._notes = notes                                      # per input: classify()'s tuple or None
        idx = [i for i, n in enumerate(notes) if n is not None and n[3] > n[2]]      # an empty note never sounds
        starts = np.array([notes[i][2] for i in idx], dtype=np.int64)
        ends = np.array([notes[i][3] for i in idx], dtype=np.int64)
        order = np.argsort(starts, kind="stable")
        self._starts, self._ends = starts[order], ends[order]
        self._run_max = np.maximum.accumulate(self._ends) if len(idx) else self._ends
        self._input_of = np.array(idx, dtype=np.int64)[order]
        self._whole = [i for i, n in enumerate(notes) if n is None]                  # rendered over the whole block
        self._pluck = [n is not None and type(n[0]) is KarplusStrongPE for n in notes]
        self._staging = np.zeros(4096, dtype=np.uint8)

    n_notes = property(lambda self: int(sum(n is not None for n in self._notes)))

    def active(self, start: int, duration: int):
        """Input indices, ascending, of the notes that sound in [start, start + duration)."""
        pos = cull(self._starts, self._ends, self._run_max, start, start + duration)
        return np.sort(self._input_of[pos])

    # ------------------------------------------------------------------------------------------ render
    def render_mix(self, mix, start: int, duration: int) -> Snippet:
        end = start + duration
        window = Extent(start, end)
        plucks_here = not _diag._ACTIVE          # with diagnostics on every note is pulled through its own render()
        segs = []                                # (input index, payload, first frame in the block, frames, channels)
        plucks = []                              # (its entry of segs, core, local start, frames, peeled layers)
        keep = []
        for i in self.active(start, duration).tolist():
            core, shift, n_lo, n_hi, chain = self._notes[i]
            lo, hi = max(start, n_lo), min(end, n_hi)
            if plucks_here and self._pluck[i]:
                segs.append([i, 0, lo - start, hi - lo, core._channels])
                plucks.append((segs[-1], core, lo - shift, hi - lo, chain))
            else:
                snip = self._inputs[i].render(lo, hi - lo)
                keep.append(snip)
                segs.append([i, snip.dev.ptr, lo - start, hi - lo, snip.channels])
        for i in self._whole:
            pe = self._inputs[i]
            if pe.extent().intersects(window):
                snip = pe.render(start, duration)
                keep.append(snip)
                segs.append([i, snip.dev.ptr, 0, duration, snip.channels])
        if not segs:
            return Snippet.from_zeros(start, duration, mix.channel_count() or 1)
        if self._whole:
            segs.sort(key=lambda s: s[0])                        # input order (the notes alone already are)
        ch = segs[0][4]
        for s in segs[1:]:
            if s[4] != ch:
                raise ValueError(f"operands could not be broadcast together with shapes "
                                 f"({duration},{ch}) ({duration},{s[4]})")
        STATS["renders"] += 1
        L = lib()
        S, P = len(segs), len(plucks)
        seg_tab = np.zeros(S, dtype=_dev.SCORE_SEG)
        note_tab = None
        if P:
            # strings that share a workgroup run until the longest is done: longest first, equal counts together
            plucks.sort(key=lambda p: -p[3])
            note_tab = np.zeros(P, dtype=_dev.KS_NOTE)
            total = 0
            max_line = 2
            for k, (_, core, local, n, chain) in enumerate(plucks):
                for node in chain:
                    if "_la_win" in node.__dict__ or "_la_owner" in node.__dict__:
                        _look_ahead.before_direct_access(node)
                if "_la_win" in core.__dict__ or "_la_owner" in core.__dict__:
                    _look_ahead.before_direct_access(core)
                if core._line is None:
                    core._excite()
                note_tab[k] = (core._params.ptr, core._line.ptr, core._state.ptr, local, n, total)
                total += n * ch
                max_line = max(max_line, core._delay_len)
            scratch = DeviceBuffer((total,), np.float32)
            keep.append(scratch)
            for k, p in enumerate(plucks):
                p[0][1] = scratch.ptr + 4 * int(note_tab["dst"][k])
        for k, s in enumerate(segs):
            seg_tab[k] = (s[1], s[2], s[3])

        inline_mix, inline_ks = S <= INLINE, P <= INLINE
        seg_ptr = note_ptr = off_ptr = list_ptr = None
        if not (inline_mix and inline_ks):
            parts = []
            if not inline_mix:
                offsets, entries = tile_lists(seg_tab["first"], seg_tab["frames"], duration)
                parts += [seg_tab, offsets, entries]
            if P and not inline_ks:
                parts.insert(0, note_tab)                        # 8-byte records first: everything stays aligned
            table, at = self._upload(parts)
            keep.append(table)
            where_at = {id(p): a for p, a in zip(parts, at)}
            if not inline_mix:
                seg_ptr = table.ptr + where_at[id(seg_tab)]
                off_ptr = table.ptr + where_at[id(offsets)]
                list_ptr = table.ptr + where_at[id(entries)]
            if P and not inline_ks:
                note_ptr = table.ptr + where_at[id(note_tab)]
        if P:
            check(L.pgx_karplus_score(scratch.ptr, ch, note_tab.ctypes.data if inline_ks else note_ptr, P,
                                      ks_group(P), max_line, int(inline_ks)), "pgx_karplus_score")
            STATS["launches"] += 1
        out = DeviceBuffer((duration, ch), np.float32)
        check(L.pgx_score_mix(out.ptr, duration, ch, seg_tab.ctypes.data if inline_mix else seg_ptr, S, off_ptr,
                              list_ptr, TILE), "pgx_score_mix")
        STATS["launches"] += 1
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
        table = DeviceBuffer((total,), np.uint8)
        check(lib().pgx_memcpy_h2d(table.ptr, self._staging.ctypes.data, total), "pgx_memcpy_h2d")
        STATS["uploads"] += 1
        return table, at
