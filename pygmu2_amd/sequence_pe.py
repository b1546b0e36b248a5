"""
SequencePE / SequenceMode: PEs placed on a timeline (sequence_pe.py:21-131).

Pure graph composition, as in the reference: every element becomes DelayPE(pe, start); in NON_OVERLAP mode every
element but the last is also cropped to end where the next one starts; one element is returned bare, more go into a
MixPE.  Rendering, extent, purity and channel count are that composed graph's -- so a score of bounded notes renders
through MixPE's score bank (score_bank.py): only the notes a block touches are rendered, each over its overlap, and one
kernel mixes them.
"""

from __future__ import annotations

from enum import Enum

from .crop_pe import CropPE
from .delay_pe import DelayPE
from .extent import Extent
from .mix_pe import MixPE
from .processing_element import ProcessingElement
from .snippet import Snippet


class SequenceMode(Enum):
    OVERLAP = "overlap"              # elements that overlap are mixed
    NON_OVERLAP = "non_overlap"      # an element ends where the next one starts


class SequencePE(ProcessingElement):
    _PASSES_BLOCKS = True              # look_ahead.py / read_ahead.py: (start, duration) go to the composed graph as
    _READ_AHEAD_SAFE = True            # they come; whether a window may open is decided by the PEs below

    def __init__(self, *input_start_pairs, mode: SequenceMode | str = SequenceMode.OVERLAP):
        args = input_start_pairs
        if len(args) == 2 and isinstance(args[0], ProcessingElement):
            pairs = [(args[0], args[1])]                       # SequencePE(pe, start)
        elif len(args) == 1 and isinstance(args[0], (list, tuple)):
            pairs = list(args[0])                              # SequencePE([(pe, start), ...])
        else:
            pairs = list(args)                                 # SequencePE((pe, start), (pe, start), ...)
        if not pairs:
            raise ValueError("SequencePE requires at least one (pe, start) pair")

        placed: list[tuple[ProcessingElement, int]] = []
        cursor: int | None = None                              # where the previous element ends; None: it never does
        for i, pair in enumerate(pairs):
            if not isinstance(pair, (list, tuple)) or len(pair) != 2:
                raise ValueError("Each input must be a (pe, start) pair")
            pe, start = pair
            if start is None:
                if i == 0:
                    start = 0
                elif cursor is None:
                    raise ValueError("Cannot auto-advance start time after an infinite extent")
                else:
                    start = cursor
            start = int(start)
            placed.append((pe, start))
            ext = pe.extent()
            cursor = None if ext.end is None else start + int(ext.end - (ext.start or 0))

        if isinstance(mode, str):
            mode = SequenceMode(mode.lower())
        self._mode = mode
        placed.sort(key=lambda p: p[1])                        # stable: equal starts keep the order given
        self._pairs = placed

        scheduled: list[ProcessingElement] = []
        for i, (pe, start) in enumerate(placed):
            node: ProcessingElement = DelayPE(pe, delay=start)
            if mode == SequenceMode.NON_OVERLAP and i + 1 < len(placed):
                node = CropPE(node, start, placed[i + 1][1] - start)
            scheduled.append(node)
        self._out = scheduled[0] if len(scheduled) == 1 else MixPE(*scheduled)

    @property
    def mode(self) -> SequenceMode:
        return self._mode

    def inputs(self) -> list[ProcessingElement]:
        return [self._out]

    def is_pure(self) -> bool:
        return self._out.is_pure()

    def channel_count(self) -> int | None:
        return self._out.channel_count()

    def _compute_extent(self) -> Extent:
        return self._out.extent()

    def _render(self, start: int, duration: int) -> Snippet:
        return self._out.render(start, duration)

    def __repr__(self) -> str:
        return f"SequencePE(pairs={len(self._pairs)}, mode={self._mode.value})"
