"""
RandomSelectPE: every trigger event picks one of N sources at random and plays it from its own time 0
(random_select_pe.py:22-172).

The reference composes it as TriggerRestartPE(trigger, selector), where the selector rerolls whenever it is reset and
renders whatever it holds.  That composition is kept here as the composed path: it serves candidates that carry state,
and it is what the gather path is measured against.

The gather path (restart_bank.py) is taken when every candidate's samples depend on the frame index alone: the trigger is
scanned on the device, the block's draws are made on the host from the same random.Random in the same order, each distinct
candidate drawn is rendered once, and one launch gathers the block.

Draws, as the reference consumes them: one at every on_start, one at every positive trigger sample, one at reset_state()
(which also forgets the running stretch: silence until the next event).  on_stop forgets the selection but not the
generator, so a stop / start continues the sequence.  The candidates are never reset.
"""

from __future__ import annotations

import random
from typing import Sequence

from . import restart_bank as _bank
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet
from .trigger_restart_pe import TriggerRestartPE
from .trigger_signal import TriggerSignal


class _RandomSelectSourcePE(ProcessingElement):
    """Holds one of the inputs and renders it; a reset picks again.  Under TriggerRestartPE every event is a reset."""

    def __init__(self, inputs: Sequence[ProcessingElement], weights: Sequence[float] | None = None,
                 seed: int | None = None):
        if not inputs:
            raise ValueError("_RandomSelectSourcePE requires at least one input")
        if weights is not None and len(weights) != len(inputs):
            raise ValueError("weights must have the same length as inputs")
        self._inputs = list(inputs)
        self._weights = list(weights) if weights is not None else None
        self._rng = random.Random(seed)
        self._indices = list(range(len(self._inputs)))
        self._active_index: int | None = None

    def inputs(self) -> list[ProcessingElement]:
        return list(self._inputs)

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int | None:
        return self._inputs[0].channel_count()

    def resolve_channel_count(self, input_channel_counts: list[int]) -> int:
        if not input_channel_counts:
            raise ValueError("_RandomSelectSourcePE has no inputs")
        cc0 = input_channel_counts[0]
        for i, cc in enumerate(input_channel_counts[1:], start=1):
            if cc != cc0:
                raise ValueError(f"_RandomSelectSourcePE channel mismatch: input 0 has {cc0}, input {i} has {cc}")
        return cc0

    def _compute_extent(self) -> Extent:
        return Extent(None, None)

    def draw(self, count: int) -> list[int]:
        """`count` picks in a row; the last one stays selected.  random.choices takes one random() per pick, so one
        call for k picks leaves the generator where k calls for one pick each leave it."""
        if count <= 0:
            return []
        picks = self._rng.choices(self._indices, weights=self._weights, k=count)
        self._active_index = picks[-1]
        return picks

    def _reset_state(self) -> None:
        self.draw(1)

    _on_start = _reset_state

    def _on_stop(self) -> None:
        self._active_index = None

    def _render(self, start: int, duration: int) -> Snippet:
        if self._active_index is None:
            self.draw(1)
        return self._inputs[self._active_index].render(start, duration)


class RandomSelectPE(ProcessingElement):
    def __init__(self, trigger: TriggerSignal, inputs: Sequence[ProcessingElement],
                 weights: Sequence[float] | None = None, seed: int | None = None):
        if not inputs:
            raise ValueError("RandomSelectPE requires at least one input")
        self._trigger = trigger
        self._sources = list(inputs)
        self._selector = _RandomSelectSourcePE(self._sources, weights=weights, seed=seed)
        self._impl = TriggerRestartPE(self._trigger, self._selector)        # the composed path
        self._bank = None                                                   # False: looked, not to be had

    def inputs(self) -> list[ProcessingElement]:
        return [self._trigger] + self._sources

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int | None:
        return self._selector.channel_count()

    def resolve_channel_count(self, input_channel_counts: list[int]) -> int:
        if len(input_channel_counts) < 2:
            raise ValueError("RandomSelectPE has no audio inputs")
        audio = input_channel_counts[1:]
        cc0 = audio[0]
        for i, cc in enumerate(audio[1:], start=2):
            if cc != cc0:
                raise ValueError(f"RandomSelectPE channel mismatch: input 1 has {cc0}, input {i} has {cc}")
        return cc0

    def _compute_extent(self) -> Extent:
        return self._trigger.extent()

    # the two layers of the composed path keep the state (the running stretch's origin, the selection, the generator);
    # the bank borrows it block by block, so the two paths can be switched between blocks
    def _reset_state(self) -> None:
        self._selector.reset_state()
        self._impl.reset_state()

    def _on_start(self) -> None:
        self._selector.on_start()
        self._impl.on_start()
        if self._bank:
            self._bank.forget()

    def _on_stop(self) -> None:
        self._impl.on_stop()
        self._selector.on_stop()
        if self._bank:
            self._bank.forget()

    take_renders = property(lambda self: self._bank.take_renders if self._bank else 0)
    d2h_reads = property(lambda self: self._bank.d2h_reads if self._bank else 0)

    def _gather_bank(self):
        if not _bank.enabled():
            return None
        if self._bank is None:
            self._bank = _bank.try_build(self._trigger, self._sources, self.channel_count() or 1) or False
        return self._bank or None

    def _render(self, start: int, duration: int) -> Snippet:
        bank = self._gather_bank()
        if bank is None:
            return self._impl.render(start, duration)
        bank.origin = self._impl._origin
        out = bank.render(start, duration, self._selector._active_index, self._selector.draw)
        if out is None:
            return self._impl.render(start, duration)
        self._impl._origin = bank.origin
        return out

    def __repr__(self) -> str:
        return f"RandomSelectPE(trigger={type(self._trigger).__name__}, inputs={len(self._sources)})"
