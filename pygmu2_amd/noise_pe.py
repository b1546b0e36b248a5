"""
NoisePE: white, pink (Paul Kellet's filter) or brown (clamped random walk) noise, scaled to [min_value, max_value]
(noise_pe.py:20-171).

The reference draws np.random.default_rng(seed).uniform(-1, 1, duration).astype(float32) per render and walks the block
in Python for PINK and BROWN.  Here the draws are made on the device (pgx_noise_*, csrc/pgx_noise.hip): numpy's PCG64 is
a 128-bit LCG, so draw number k of a stream is a function of the seeded (state, inc) and k alone.  The host asks numpy
for the seeded state once per start and from then on keeps only the count of draws consumed; the seven pink taps and the
brown level live in HBM.  Samples are the reference's to the bit in all three modes, however the stream is cut.

Like the reference, `start` is ignored: every render consumes the next `duration` draws wherever it is asked to be.  A
seek does not rewind the stream; only on_start / reset_state() does (generator back to the seed, taps and level zero;
seed=None draws fresh OS entropy, as default_rng(None) does).

A MixPE of many NoisePEs of one mode renders them as a bank (voice_bank._NoiseNode: the same kernels with batch = K); the
node then holds the voices' records, and advance() / reset_state() on a voice are passed on to it (`_bank_slot`).
"""

from __future__ import annotations

from enum import Enum

import numpy as np

from . import device as _dev
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .snippet import Snippet
from .source_pe import SourcePE

_MASK64 = (1 << 64) - 1


class NoiseMode(Enum):
    """Which of the three spectra NoisePE renders (noise_pe.py:20-25)."""

    WHITE = "white"
    PINK = "pink"
    BROWN = "brown"


class NoisePE(SourcePE):
    _LOOK_AHEAD_SAFE = True            # draws and filter state do not depend on how the stream is cut (look_ahead.py)
    _STATE_FIELDS = ("_consumed", "_filter")

    def __init__(self, min_value: float = -1.0, max_value: float = 1.0, seed: int | None = None,
                 mode: NoiseMode = NoiseMode.WHITE):
        if max_value < min_value:
            raise ValueError("NoisePE requires max_value >= min_value")
        self._min_value = float(min_value)
        self._max_value = float(max_value)
        self._seed = seed
        self._mode = mode
        self._params: DeviceBuffer | None = None      # one pgx_noise_params; None until the first render after a start
        self._filter: DeviceBuffer | None = None      # one pgx_noise_state; None: all zero
        self._consumed = 0                            # draws taken since the generator was seeded
        self._bank_slot = None                        # (weakref to the voice bank node that renders this PE, its voice)

    min_value = property(lambda self: self._min_value)
    max_value = property(lambda self: self._max_value)
    seed = property(lambda self: self._seed)
    mode = property(lambda self: self._mode)

    def inputs(self) -> list:
        return []

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int:
        return 1

    def _compute_extent(self) -> Extent:
        return Extent(None, None)

    def _reset_state(self) -> None:
        self._params = None             # the next render seeds the generator again
        self._filter = None
        self._consumed = 0
        node = self._bank_node()
        if node is not None:
            node.reset_voice(self._bank_slot[1])

    def _bank_node(self):
        """The voice bank node that renders this PE (voice_bank._NoiseNode; this PE is its voice _bank_slot[1]), or None."""
        slot = self._bank_slot
        return slot[0]() if slot is not None else None

    _on_start = _reset_state
    _on_stop = _reset_state

    def advance(self, draws: int) -> None:
        """Skip `draws` draws of the stream without rendering them (numpy's PCG64.advance): O(1) on the host, the next
        render skips ahead on the device.  The pink taps and the brown level stay as they are."""
        if draws < 0:
            raise ValueError("draws must be >= 0")
        self._consumed += int(draws)
        node = self._bank_node()
        if node is not None:                # a voice of a bank: its record there skips ahead
            node.advance(self._bank_slot[1], int(draws))

    def _seed_record(self) -> np.ndarray:
        """One pgx_noise_params for the seeded generator (seed=None: fresh OS entropy at every call)."""
        s = np.random.PCG64(self._seed).state["state"]
        state, inc = int(s["state"]), int(s["inc"])
        rec = np.zeros(1, dtype=_dev.NOISE_PARAMS)
        rec["state_hi"], rec["state_lo"] = state >> 64, state & _MASK64
        rec["inc_hi"], rec["inc_lo"] = inc >> 64, inc & _MASK64
        rec["scaled"] = int(not (self._min_value == -1.0 and self._max_value == 1.0))     # noise_pe.py:104
        with np.errstate(over="ignore"):
            rec["span"] = np.float32(self._max_value - self._min_value)
            rec["min_value"] = np.float32(self._min_value)
        return rec

    def _seed_generator(self) -> None:
        self._params = _dev.upload_structs(self._seed_record())

    def _render(self, start: int, duration: int) -> Snippet:
        if duration <= 0:
            return Snippet.from_zeros(start, 0, 1)
        mode = self._mode
        if mode is not NoiseMode.WHITE and mode is not NoiseMode.PINK and mode is not NoiseMode.BROWN:
            raise ValueError(f"Unknown NoiseMode: {self._mode}")
        if self._params is None:
            self._seed_generator()
        out = new_output(duration, 1)
        draws = self._consumed & _MASK64
        if mode is NoiseMode.WHITE:
            check(lib().pgx_noise_white(out.ptr, duration, 1, duration, draws, self._params.ptr), "pgx_noise_white")
        else:
            if self._filter is None:
                self._filter = DeviceBuffer((1,), _dev.NOISE_STATE, zero=True)
            entry = lib().pgx_noise_pink if mode is NoiseMode.PINK else lib().pgx_noise_brown
            check(entry(out.ptr, duration, 1, duration, draws, self._params.ptr, self._filter.ptr), "pgx_noise")
        self._consumed += duration
        return Snippet(start, out)

    def __repr__(self) -> str:
        return f"NoisePE(mode={self._mode.value}, range=[{self._min_value}, {self._max_value}])"
