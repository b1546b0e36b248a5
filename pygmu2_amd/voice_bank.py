"""
Voice bank: batched rendering of structurally identical voice sub-graphs under a MixPE.

The reference renders a MixPE of K voices by pulling K separate sub-graphs, one numpy
call chain each (mix_pe.py:69-96).  On MI355X K x (PEs per voice) small launches would
leave the chip idle, so when every input of a MixPE is the same tree of supported PEs
with scalar parameters, the trees are walked in lock-step and each level is rendered by
ONE batched launch: per-voice parameter blocks and state blobs are stacked [K] in HBM,
intermediate signals are [K][frames][channels], and the final pgx_mix_batch adds the
K voices in input order in float32 -- the same additions, in the same order, as MixPE.
The batched kernels are the very same kernels the single PEs use (batch = 1 there), so a
bank produces the same samples as rendering the voices one by one.

Supported nodes: SinePE (scalar, or frequency / amplitude / phase driven by single-channel PEs of batchable classes),
FunctionGenPE (scalar), NoisePE, BlitSawPE (scalar), SuperSawPE (scalar),
AnalogOscPE (scalar parameters, or
single-channel PEs of batchable classes), BiquadPE (constant coefficients, or cutoff and / or Q driven by single-channel
PEs of batchable classes), LadderPE (scalar controls), CombPE (scalar controls), GainPE (constant or PE gain), TransformPE
(a chain lowered to pgx_transform), AdsrGatedPE, PeriodicGate, SVFilterPE (scalar frequency and Q), AdsrTriggeredPE,
PeriodicTrigger, SpatialPE (SpatialLinear / SpatialConstantPower with a scalar azimuth or a single-channel PE of a batchable
class; SpatialAdapter).
Anything else -> `try_build_bank` returns None and MixPE falls back to per-input rendering.

Panned voices (_PanNode): a voice that ends in SpatialPE(voice, method=SpatialConstantPower(azimuth=a_i)) -- each voice at its
place in the stereo field -- is a kind of its own, key ("pan", method class, azimuth is a PE, source[, azimuth]); the scalar
azimuths are per-voice data, turned into {lg, rg}[K] ONCE when the node is built (pgx_pan_gains: the device function pgx_pan
evaluates, so no transcendental per frame afterwards); a PE azimuth is a batched level of (n, 1) streams rendered first.  The
node carries nothing.  As the root it is ONE launch per block, pgx_pan_mix_batch: every voice's mono sample is read once,
multiplied by its two gains (each product rounded to float32) and added in voice order into the mix's (n, 2) block -- the
additions of pgx_pan per voice followed by the mix, bit for bit, without the [K][n][2] layer.  Under another PE -- GainPE(
SpatialPE(...), 0.5) -- it is a level like any other: pgx_pan_bank, pgx_pan with the voice in the grid.  SpatialAdapter
(_AdaptNode) is one pgx_channel_adapt over the stacked K * n frames.  SpatialHRTF carries a convolution tail and is not
batched; voices whose methods differ in class, that mix scalar and PE azimuths, or that share an azimuth PE are not one bank.
Banked from MIN_VOICES voices on (measured: tools/pan_bank_probe.py -- the bank wins from 4 voices at both block lengths).

Percussive voices: a constant SVFilterPE is a level of its own (pgx_svf_bank, _SvfNode: pgx_svf's plan with the voice in
the grid, the host's nine constants per voice; an SVFilterPE with a PE parameter stays per voice), and
AdsrTriggeredPE(PeriodicTrigger) -- as a gain or under a TransformPE as a cutoff -- is two: K trigger rows in one launch
(pgx_periodic_trigger_bank, _TriggerNode), then pgx_adsr_triggered with batch = K (_AdsrTriggeredNode, a plain node: the
gated envelope's walk ahead of the stream is not for it; the on-chip mix takes its rows as any gain rows).  Banked from
SVF_MIN_VOICES / ADSR_TRIGGERED_MIN_VOICES voices on, the walk from SVF_WALK_MIN_ROWS rows on (all three measured:
tools/percussive_bank_probe.py).

Noise voices (_NoiseNode): pgx_noise_white / _pink / _brown have taken a batch since they were written -- an instance per grid
row or workgroup, params[i], state[i] -- so K NoisePEs of one mode are ONE call, and K pink or brown recurrences stepped side by
side last as long as one.  Seed and range are per-voice data, the draws consumed are one host number (every voice takes n per
render); NoisePE.advance / reset_state on one voice move that voice's record alone.  A hi-hat voice -- GainPE(SVFilterPE(NoisePE),
gain=AdsrTriggeredPE(PeriodicTrigger)) -- is batched on every level.  Banked from NOISE_MIN_VOICES voices on (measured:
tools/noise_bank_probe.py).  A pure FunctionGenPE (_FunctionGenNode: pgx_function_gen_bank, the PE's sample function with the
voice in the grid, bit for bit) is a source or a modulator like SinePE; one with a PE parameter carries a phase and stays per voice.

Swept-filter voices (pgx_biquad_varying_bank, _BiquadVarNode): a BiquadPE whose cutoff or Q is a PE -- an oscillator into a
low-pass that follows an envelope or an LFO -- is a kind of its own, key ("biquad_var", freq_is_pe, q_is_pe, source, ...);
mode, gain_db and the scalar of the other parameter are per-voice data.  The modulators are batched levels rendered first,
then ONE call runs pgx_biquad_varying's plan with the voice in the grid: each voice's samples and {x1, x2, y1, y2} are the
PE's, bit for bit.  From BIQUAD_VAR_WALK_MIN_ROWS rows (voices x channels) on the node passes no workspace: every row is
walked by one workgroup in one launch, the same recurrence in another association (within a float32 rounding).  Banked
from BIQUAD_VAR_MIN_VOICES voices on (both measured: tools/swept_bank_probe.py).

Modulated-sine voices (pgx_sine_stateful_bank, _SineModNode): a SinePE whose frequency, amplitude or phase is a PE -- FM,
tremolo, phase modulation -- is a kind of its own, key ("sine_mod", channels, freq_is_pe, amp_is_pe, phase_is_pe, ...); the
scalars of the other parameters are per-voice data.  The modulators are batched levels rendered first (one that is itself
a modulated sine has the same kind: nested FM), then ONE call runs the PE's kernel with the voice in the grid, {phase,
initialised} carried per voice: samples and state are the PE's, bit for bit, on either plan -- a workgroup per tile and
voice in two launches (the tiles' totals, then their left fold in tile order and the frames), or from
SINE_MOD_WALK_MIN_ROWS voices on one workgroup per voice walking its row.  Like the PE the node carries the phase through a
seek and clears it on start and stop; a phase in play (SinePE._look_ahead_condition) forbids windows.  Banked from
SINE_MOD_MIN_VOICES voices on (both measured: tools/fm_bank_probe.py).

AnalogOscPE voices (pgx_analog_osc_bank): the voice is a grid dimension of the PE's own scan kernels, so a bank of K
takes the launches of one PE -- 1 (pure rectangle), 3 (pure sawtooth, stateful rectangle), 5 (stateful sawtooth) -- and
gives each voice the PE's samples bit for bit.  Frequency and duty may be PEs (the reference's PWM voice: duty =
TransformPE(SinePE, Affine)): they are batched levels of their own, rendered first; phase and saw value are carried
per voice in a [K][2] state blob under the PE's restart rule.  The pure sawtooth restarts its integration at every
request (analog_osc_pe.py), so a bank that holds one renders exactly the requests it is given: no windows
(_Node._REQUEST_DEPENDENT).  A voice tree that holds an AnalogOscPE is banked from ANALOG_OSC_MIN_VOICES voices on: below,
over a long stream, the per-voice path's look-ahead windows are faster than a bank rendered block by block (measured).
"""

from __future__ import annotations

import functools
import math
import os
import weakref
from typing import NamedTuple

import numpy as np

from . import device as _dev
from ._kernels import DeviceBuffer, blitsaw_workspace, check, lib, ptr
from . import transforms as _tf
from .adsr_pe import AdsrGatedPE, AdsrTriggeredPE
from .analog_osc_pe import AnalogOscPE
from .biquad_pe import _MODE_INDEX, BiquadPE, rbj_coefficients, settle_frames, settle_frames_fine
from .blit_saw_pe import BlitSawPE, wide_oscillators_ok
from .comb_pe import CombPE
from .extent import Extent
from .function_gen_pe import FunctionGenPE
from .gain_pe import GainPE
from .ladder_pe import LadderPE
from .noise_pe import _MASK64, NoiseMode, NoisePE
from .periodic_gate import PeriodicGate
from .periodic_trigger import PeriodicTrigger
from .processing_element import ProcessingElement
from .sine_pe import SinePE
from .snippet import Snippet
from .spatial_pe import SpatialAdapter, SpatialConstantPower, SpatialLinear, SpatialPE
from .super_saw_pe import SuperSawPE
from .svfilter_pe import _SVF_MODE_INDEX, SVFilterPE, svf_coefficients
from .transform_pe import TransformPE

MIN_VOICES = 4
ANALOG_OSC_MIN_VOICES = 64    # ... and for voices that hold an AnalogOscPE.  The per-voice path streams through look-ahead's
                              # windows of up to 256 blocks, a bank block by block: tools/analog_bank_probe.py, PWM voice under
                              # an envelope, us per block bank / per voice over a long stream -- 4 096-frame blocks: 4 voices
                              # 55 / 8, 8: 48 / 14, 64: 50 / 120, 512: 94 / 1 728; 48 000-frame blocks: 52 / 46, 43 / 85, 80 / 767,
                              # 377 / 11 733 (streams of 8 blocks: the bank from 4 voices on, 62 / 96 ... 451 / 49 040).  The
                              # smallest K measured from which the bank wins every row, and every row of a larger K
BIQUAD_VAR_MIN_VOICES = 16    # ... and for voices that hold a BiquadPE with a PE-driven cutoff or Q (_BiquadVarNode), for the same
                              # reason: tools/swept_bank_probe.py, sawtooth -> swept low-pass under an envelope, us per block bank /
                              # per voice over a stream of 248 blocks -- 4 096-frame blocks: 4 voices 57 / 26, 8: 48 / 46, 16: 49 / 90,
                              # 64: 66 / 362, 512: 132 / 2 990; 48 000-frame blocks: 63 / 56, 72 / 107, 84 / 219, 166 / 851,
                              # 727 / 7 231 (streams of 8 blocks: the bank from 4 voices on, 70 / 137 ... 807 / 40 556).  The smallest
                              # K measured from which the bank wins every row, and every row of a larger K
BIQUAD_VAR_WALK_MIN_ROWS = 512   # rows (voices x channels) from which _BiquadVarNode passes no workspace: one workgroup per row walks
                              # the block in one launch instead of the segmented plan's two.  The same probe, us per block walk /
                              # segmented, streams of 8 and of 248 blocks -- 4 096 frames: 256 rows 102 / 90 and 78 / 88, 512 rows
                              # 120 / 141 and 112 / 132; 48 000 frames: 16 rows 231 / 91, 64: 271 / 179, 256: 344 / 435 and 308 / 392,
                              # 512: 521 / 807 and 470 / 727.  The smallest row count measured from which the walk is not slower in
                              # any row, and in no row of a larger count (256 loses one of its four: short streams of 4 096 frames)
SVF_MIN_VOICES = 256          # ... and for voices that hold an SVFilterPE (_SvfNode): tools/percussive_bank_probe.py, SVFilterPE(BlitSawPE),
                              # us per block bank / per voice over streams of 2 040 (248) blocks, look-ahead on -- 512-frame blocks:
                              # 4 voices 17 / 1, 16: 21 / 4, 64: 20 / 14, 256: 21 / 59; 4 096: 20 / 1, 21 / 5, 26 / 19, 37 / 78; 48 000:
                              # 21 / 9, 34 / 34, 91 / 138, 306 / 548 (profiles/percussive_bank_probe.md; the spread of three passes is
                              # below 1 us in these rows).  Two PEs per voice in windows of up to 256 blocks cost the per-voice path
                              # 0.25 us per voice and block; the bank pays its ~20 us every block.  The smallest K measured from which
                              # the bank wins every row (64 loses at 512 and at 4 096 frames; between 64 and 256: not measured)
SVF_WALK_MIN_ROWS = 256       # rows (voices x channels) from which _SvfNode passes no workspace: one workgroup per row walks the block in
                              # one launch instead of the segmented plan's two.  The same probe, us per block walk / segmented -- 4 096
                              # frames: 4 rows 18 / 20, 64: 21 / 26, 256: 25 / 37; 48 000 frames: 4 rows 109 / 21, 64: 123 / 91, 256: 150 /
                              # 306 (blocks of up to two tiles are walked either way).  The smallest row count measured from which the
                              # walk is not slower in any row
ADSR_TRIGGERED_MIN_VOICES = 64   # ... and for voices that hold an AdsrTriggeredPE (_AdsrTriggeredNode): the same probe, GainPE(BiquadPE(
                              # BlitSawPE), gain=AdsrTriggeredPE(PeriodicTrigger)), us per block bank / per voice -- 512-frame blocks: 4
                              # voices 54 / 3, 16: 59 / 13, 32: 59 / 27, 64: 51 / 57, 256: 58 / 292; 4 096: 57 / 18, 8 voices 59 / 37, 16
                              # (the on-chip mix from here on): 11 / 76, 64: 13 / 332, 256: 21 / 1 790; 48 000: 97 / 209, 16: 66 / 854,
                              # 256: 195 / 20 490.  The smallest K measured from which the bank wins every row (32 loses at 512 frames)
NOISE_MIN_VOICES = 64         # ... and for voices that hold a NoisePE (_NoiseNode): tools/noise_bank_probe.py, MixPE of K NoisePE(seed=i), us
                              # per block bank / per voice, look-ahead on, streams of 248 blocks of 1 024 frames and of 8 of 48 000
                              # (profiles/noise_bank_probe.md; the spread of three passes is below 3 us in the rows that decide).  White,
                              # the mode that decides -- 1 024 frames: 4 voices 12 / 2, 8: 11 / 3, 16: 12 / 5.5, 64: 11 / 20, 256: 13 / 78,
                              # 512: 19 / 177; 48 000: 14 / 27, 18 / 58, 15 / 89, 24 / 330, 59 / 1 293, 104 / 2 580.  Pink and brown win
                              # from 4 voices on (pink 1 024 frames: 25 / 70 ... 41 / 9 089; 48 000: 846 / 3 659 ... 1 041 / 472 907: K
                              # recurrences side by side last as long as one), the hi-hat voice from 64 (16 voices, 1 024 frames: 61 / 50).
                              # The smallest K measured at which the bank is not slower at either block length in ANY mode, nor at a
                              # larger K (between 16 and 64: not measured).  One number for the three modes: a minimum per mode is open
SINE_MOD_MIN_VOICES = 16      # ... and for voices that hold a SinePE with a PE parameter (_SineModNode): tools/fm_bank_probe.py, MixPE of K
                              # SinePE(frequency=TransformPE(SinePE, Affine)), us per block bank / per voice, look-ahead on, streams of
                              # 248 blocks of 1 024 frames and of 8 of 48 000 (profiles/fm_bank_probe.md; the spread of three passes
                              # is below 1 us in the rows that decide) -- 1 024 frames: 4 voices 22 / 8.5, 8: 22 / 16.5, 16: 22 / 32,
                              # 64: 22 / 131, 512: 26 / 1 054; 48 000: 31 / 367, 31 / 731, 31 / 1 457, 56 / 5 819, 235 / 46 523 (a voice
                              # alone is one workgroup walking its block: 92 us).  The smallest K measured from which the bank wins
                              # every row, and every row of a larger K (between 8 and 16: not measured).  The same voice under an
                              # AdsrTriggeredPE envelope wins from 64 on (16 voices, 1 024 frames: 57 / 52) -- the minimum that class
                              # already asks for
SINE_MOD_WALK_MIN_ROWS = 512  # voices from which _SineModNode passes no workspace: one workgroup per voice walks the block in one
                              # launch instead of the time-parallel form's two (blocks of up to two tiles of 2 048 frames are walked
                              # either way).  The same probe, 48 000-frame blocks, us per block walk / time-parallel -- fm: 4 voices
                              # 90 / 31, 16: 98 / 31, 64: 123 / 56, 256: 164 / 138, 512: 235 / 249; under the envelope: 111 / 79,
                              # 115 / 89, 135 / 117, 209 / 207, 362 / 349 (within the spread).  The smallest K measured from which the
                              # walk is not slower in any row (256 -- a workgroup per CU, the value before the probe -- loses the fm
                              # row; between 256 and 512: not measured)
BANK_WINDOWS = True           # a small bank streamed in equal blocks: 2, 4, 8 blocks per render, handed out as rows (VoiceBank)
BANK_WINDOWS_ANY_ROOT = os.environ.get("PGX_BANK_WINDOWS_ANY_ROOT", "0") == "1"     # experiments (C5: measured slower)
BANK_WINDOW_FIRST = 2
BANK_WINDOW_MAX = int(os.environ.get("PGX_BANK_WINDOW_MAX", "8"))
BANK_WINDOW_FRAMES = 1 << 20
BANK_WINDOW_MAX_VOICES = int(os.environ.get("PGX_BANK_WINDOW_MAX_VOICES", "256"))  # (a bank that fills the chip gains nothing: its launches are long)
LADDER_WINDOWS = True         # a ladder bank directly under the mix, streamed in equal blocks: several blocks per launch
LADDER_WINDOW_FIRST = 2       # ... 2, then 4, 8, 16, 32 blocks (a lane of k_ladder_segments pays its 1024-sample warm-up once per
                              # launch: C4 over a stream 0.0675 ms per block with windows up to 8, 0.0591 up to 16, 0.0497 up to 32
                              # -- tools/c4_windows_probe.py; the same ladders at resonance 0.6, whose warm-up is 2048: 0.226 /
                              # 0.134 / 0.088; like look-ahead's windows a stream that stops after k blocks has rendered < 2k + 2)
LADDER_WINDOW_MAX = int(os.environ.get("PGX_LADDER_WINDOW_MAX", "32"))
LADDER_WINDOW_FRAMES = int(os.environ.get("PGX_LADDER_WINDOW_FRAMES", str(1 << 21)))   # ... and at most this many frames
PREFETCH_LADDER_INPUT = True
PREFETCH_SUPERSAW_VOICES = True   # small SuperSaw banks under the mix: oscillators one block ahead (_SuperSawNode.mix)  # _LadderNode: next block's oscillators beside this block's ladder
FUSED_PAN_MIX = True          # a _PanNode root: pan and mix in ONE launch (pgx_pan_mix_batch), no [K][n][2] layer (False: pgx_pan_bank
                              # + pgx_mix_batch, the same samples -- what tools/pan_bank_probe.py compares it with)
FUSED_VOICE_MIN = 128        # voices (one workgroup each) from which BlitSaw -> Biquad runs as one launch
SEGMENTED_CHAIN_MAX = int(os.environ.get("PGX_BBW_MAX_BATCH", "256"))
SEGMENTED_CHAIN = True       # ... and smaller banks (4 .. 256 voices: a rank's share of C5) as one launch in concurrent time
                             # segments (pgx_blitsaw_biquad_wide_seg: closed-form oscillator carries, the filters warm up)
PIPELINE_FULL_SUPERSAW_BANK = True    # ... and for a bank that fills the chip (512 instances: the 17 us mix beside the next block's bank)
VOICE_TILES = os.environ.get("PGX_VOICE_TILES", "1") != "0"   # BlitSaw -> Biquad [-> x envelope] voices mixed on chip (pgx_voice_tiles)
VOICE_TILES_MIN_FRAMES = 4096
VOICE_TILES_MAX_WARM = 2048  # pgx_voice_tiles_max_warm(): a filter has to settle (every entry of A^warm below 2^-90) within this many frames
VOICE_TILE_WINDOWS = os.environ.get("PGX_VOICE_TILE_WINDOWS", "1") != "0"    # ... in windows of 2, 4, 8 blocks: the stream synchronisations,
                             # the edge searches and the small launches of a block are per window then, and the envelopes of the NEXT
                             # window are walked beside this one's voices (C5: 94 -> 83 us per block)
VOICE_TILES_MIN_VOICES = int(os.environ.get("PGX_VOICE_TILES_MIN_VOICES", "16"))   # (192 while the mix ran block by block: the
                             # envelope walk, which the on-chip mix waits for BEFORE the voices, was then the block's critical chain for
                             # smaller banks -- 64 voices 56 us per block against 52.  In windows: 8 voices 33 against 45, 64 voices 40
                             # against 49, 128: 48 against 56, 256: 63 against 72, 512: 83 against 106.  Smaller banks keep the kernels
                             # that are bit-identical to the per-voice path)
EARLY_WALK_MAX_VOICES = int(os.environ.get("PGX_EARLY_WALK_MAX", "256"))  # ... started at once (not behind the block's oscillators) for banks up to this size
ENVELOPE_AHEAD = True        # a bank's AdsrGatedPE(PeriodicGate) envelopes one block ahead on the side stream (render_mix)
WIDE_SUPERSAW = True         # the bank kernel with 16 frames per thread (pgx_supersaw_wide) where its conditions hold
SEGMENTED_SUPERSAW = True    # below FUSED_SUPERSAW_MIN: the fused bank in concurrent time segments (closed-form carries)
FUSED_SUPERSAW_MIN = 257     # SuperSaw instances from which the bank is rendered in one segment per instance, one block ahead (256 -- a rank's
                             # share at two ranks -- is better off in two time segments and windows: 97 -> 84 us per block)


def _is_pe(x) -> bool:
    return isinstance(x, ProcessingElement)


class _Rows:
    """Frames [offset, offset + n) of every voice of a [K][total][channels] buffer: what a node that renders several
    blocks at once hands out per block (`.ptr` at the first voice's first frame, `.stride` elements from voice to voice)."""
    __slots__ = ("buf", "ptr", "shape", "stride")

    def __init__(self, buf, offset: int, n: int):
        k, total, ch = buf.shape
        self.buf = buf
        self.ptr = buf.offset_ptr(offset * ch)
        self.shape = (k, n, ch)
        self.stride = total * ch


def _rows(x, dense: int):
    """(pointer, elements from voice to voice) of a [K][n][channels] DeviceBuffer -- `dense`: its rows lie back to back --
    or of a _Rows; (None, dense) of None, a stream the kernel does not read."""
    return ptr(x), getattr(x, "stride", dense)


def _param_records(dtype, pes, fields) -> np.ndarray:
    """One record of `dtype` per PE, filled from the dict that `fields(pe)` returns."""
    rec = np.zeros(len(pes), dtype=dtype)
    for i, pe in enumerate(pes):
        for key, v in fields(pe).items():
            rec[i][key] = v
    return rec


def closed_form_ok(rec) -> bool:
    """BLITSAW_PARAMS records whose integrator carries have a closed form -- the automatic (odd) M, a leak below 1: what
    the kernels that cut an oscillator into concurrent time segments need."""
    return bool(np.all(rec["m"] < 0.0) and np.all(rec["leak"] > 0.0) and np.all(rec["leak"] <= 0.9999)
                and np.all(rec["freq"] >= 1.0))


def _ensure_alt(*nodes) -> None:
    """Double-buffered states: a kernel that runs in concurrent segments reads `state` and writes `state_alt` ..."""
    for node in nodes:
        if node.state_alt is None:
            node.state_alt = DeviceBuffer(node.state.shape, node.state.dtype)


def _swap_states(*nodes) -> None:
    """... and the two change places behind it."""
    for node in nodes:
        node.state, node.state_alt = node.state_alt, node.state


def _copy_state(dst, src) -> None:
    check(lib().pgx_memcpy_d2d(dst.ptr, src.ptr, src.nbytes), "pgx_memcpy_d2d")


class _Ahead:
    """What a node rendered ahead of the stream: `data` for the frames (start, n); `undo()` puts back what that moved."""
    __slots__ = ("start", "n", "data", "undo")

    def __init__(self, start, n, data, undo=None):
        self.start, self.n, self.data, self.undo = start, n, data, undo

    def forget(self) -> None:
        if self.undo is not None:
            self.undo()

    def take(self, start, n):
        """`data` if it was rendered for these frames, else None: undone.  (The owner empties the slot either way.)"""
        if self.start == start and self.n == n:
            return self.data
        self.forget()
        return None


class _StateBefore:
    """The undo of oscillators that ran ahead: `node`'s states (a copy) and last_end from before."""
    __slots__ = ("node", "state", "last_end")

    def __init__(self, node, state=None):
        self.node, self.last_end = node, node.last_end
        self.state = state
        if state is None:
            self.state = DeviceBuffer(node.state.shape, node.state.dtype)
            _copy_state(self.state, node.state)

    def __call__(self) -> None:
        _copy_state(self.node.state, self.state)
        self.node.last_end = self.last_end


class _Window:
    """Several blocks of a stream rendered at once, handed out block by block: frames [first, end) in `buf`, blocks of
    `block` frames, consumed up to `served`; `undo`: what the owner needs to go back to `first`."""
    __slots__ = ("first", "end", "block", "buf", "served", "undo")

    def __init__(self, first, blocks, block, buf, undo):
        self.first, self.end, self.block, self.buf, self.undo = first, first + blocks * block, block, buf, undo
        self.served = first + block


class _Windowed:
    """The 'stream of equal blocks -> windows of 2, 4, 8 ... blocks' machine of VoiceBank and _LadderNode.  The owner
    decides whether a window may open, what to snapshot, how to restore and re-render; this keeps `win` (None: no window
    is open), `last` -- (start, n) of the last block handed out --, `grow` and look-ahead's counters (bench.py: frames
    rendered vs frames counted)."""

    def _reset_windows(self, first_blocks: int) -> None:
        self.win = None
        self.last = None
        self.grow = first_blocks

    def _next_row(self, start, n):
        """Offset of (start, n) in the open window's buffer if it is the window's next block, else None."""
        win = self.win
        if win is not None and start == win.served and n == win.block and start + n <= win.end:
            win.served = start + n
            self.last = (start, n)
            return start - win.first
        return None

    def _continues(self, start, n) -> bool:
        """Is (start, n) the block after the last one, same length?  It is the last one from here on."""
        streaming = self.last == (start - n, n)
        self.last = (start, n)
        return streaming

    def _window_blocks(self, n, max_blocks, max_frames) -> int:
        """How many blocks of n frames to render at once (1: no window); the next window is twice as long."""
        blocks = max(1, min(self.grow, max_frames // n))
        if blocks > 1:
            self.grow = min(self.grow * 2, max_blocks)
        return blocks

    def _open_window(self, start, blocks, n, buf, undo) -> None:
        """(the first block is handed out by the caller)"""
        from . import look_ahead as _look_ahead
        _look_ahead.STATS["window_frames"] += n * blocks
        _look_ahead.STATS["windows"] += 1
        self.win = _Window(start, blocks, n, buf, undo)

    def _close_window(self):
        """No window is open afterwards.  -> (first, served, undo) if one was left half consumed -- the owner goes back to
        `first` and renders [first, served) again, quietly (exact: the same kernels over the same frames) --, else None
        (consumed to the last frame: the states are already there)."""
        win, self.win = self.win, None
        if win is None or win.served >= win.end:
            return None
        return win.first, win.served, win.undo


class _Node:
    """One level of the voice tree: K PE instances of the same class and static config."""

    def __init__(self, pes, children):
        self.pes = pes
        self.k = len(pes)
        self.children = children
        self.sr = float(pes[0].sample_rate)

    def reset(self):
        for c in self.children.values():
            c.reset()

    # ---- what VoiceBank's windows need of a node: its carried state by name, and a way to come to rest
    _STATE = ()                  # attributes (DeviceBuffers, numbers, None) that make up the carried state
    _REQUEST_DEPENDENT = False   # the samples depend on how the stream is cut into requests: VoiceBank opens no window

    def quiesce(self, keep=None) -> None:
        """Anything rendered ahead of the stream is dropped: the states are where the last block handed out left them."""

    def _forget_ahead(self, slot: str) -> None:
        """What a node rendered ahead of the stream lives in a slot -- an attribute that holds an _Ahead, or None: empties
        the slot and undoes what was ahead."""
        ahead = getattr(self, slot)
        if ahead is not None:
            setattr(self, slot, None)
            ahead.forget()

    def snapshot(self) -> dict:
        snap = {}
        for name in self._STATE:
            value = getattr(self, name)
            if isinstance(value, DeviceBuffer):
                twin = DeviceBuffer(value.shape, value.dtype)
                _copy_state(twin, value)
                value = twin
            snap[name] = value
        return snap

    def restore(self, snap: dict) -> None:
        for name, value in snap.items():
            mine = getattr(self, name)
            if isinstance(value, DeviceBuffer) and isinstance(mine, DeviceBuffer) and mine.shape == value.shape:
                _copy_state(mine, value)
            else:
                setattr(self, name, value)

    def channels(self) -> int:
        raise NotImplementedError

    def render(self, start: int, n: int) -> DeviceBuffer:
        """-> DeviceBuffer [K][n][channels] float32."""
        raise NotImplementedError

    # ---- as the root of a VoiceBank: the node under the mix decides how its voices are added
    def mixes_on_chip(self, n: int) -> bool:
        """`mix` adds the voices of blocks of n frames on chip (pgx_voice_tiles): no [voices][frames] layer."""
        return False

    def mix(self, bank, start: int, n: int) -> DeviceBuffer:
        """-> the MixPE's block (n, channels) for `bank`, the VoiceBank this node is the root of: the voices rendered, then
        added in input order (pgx_mix_batch).  A node that can do better overrides this."""
        stacked = self.render(start, n)                          # [K][n][C], or rows of a window (_Rows)
        ch = stacked.shape[2]
        out = DeviceBuffer((n, ch), np.float32)
        check(lib().pgx_mix_batch(out.ptr, *_rows(stacked, n * ch), self.k, n * ch), "pgx_mix_batch")
        return out

    ws = None                    # a kernel's scratch: uint8, grown when a render needs more, never shrunk

    def _scratch_of(self, need: int) -> DeviceBuffer:
        if self.ws is None or self.ws.nbytes < need:
            self.ws = DeviceBuffer((need,), np.uint8)
        return self.ws


class _SineNode(_Node):
    def __init__(self, pes):
        super().__init__(pes, {})
        rec = np.zeros(self.k, dtype=_dev.SINE_PARAMS)
        for i, pe in enumerate(pes):
            rec[i] = (2.0 * np.pi * float(pe._frequency), float(pe._amplitude), float(pe._phase))
        self.params = _dev.upload_structs(rec)
        self.ch = pes[0]._channels

    def channels(self):
        return self.ch

    def render(self, start, n):
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        check(lib().pgx_sine_render(out.ptr, n * self.ch, self.k, start, n, self.ch, self.sr,
                                    self.params.ptr), "pgx_sine_render")
        return out


class _SineModNode(_Node):
    """Bank of SinePEs with PE-valued parameters -- FM, AM, PM voices: pgx_sine_stateful_bank, the PE's kernel with the
    voice in the grid.  The children's [K][n][1] streams first, then one call; the scalars of the other parameters are
    per-voice data (`params`, the record SinePE._render fills), {accumulated phase, initialised} is carried per voice in
    `state`, zeroed by reset() as SinePE._clear_phase does on start and stop.  Like the PE the node carries the phase
    whatever `start` is.  Below SINE_MOD_WALK_MIN_ROWS voices the entry gets a workspace: a workgroup per tile and
    voice, two launches; from there on a workgroup per voice walks its row.  Each voice's samples and state are the
    PE's either way, bit for bit.  A phase in play (a PE, or a scalar that is not 0) makes the carried phase depend on
    where the blocks are cut (SinePE._look_ahead_condition): no windows then."""

    _STATE = ("state",)
    _STREAMS = ("frequency", "amplitude", "phase")
    TILE = 2048                  # frames per tile of the entry (pgx_phase.hip: kSinTile)

    @classmethod
    def scratch_bytes(cls, n: int, k: int) -> int:
        """What the time-parallel form needs (pygmu_hip.h): per voice {phase, initialised} as they were on entry and one
        total per tile, float64.  The library exports the same number; the node restates it because the guard-band
        sweep (tests/test_gpu_guard_bands.py) counts the sizing exports this package calls against its own guarded runs,
        and this node's guarded runs are tests/test_gpu_fm_voices.py's.  tests/test_fm_bank_host.py holds the two equal."""
        return k * (-(-n // cls.TILE) + 2) * 8

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.params = _dev.upload_structs(_param_records(_dev.SINE_STATEFUL_PARAMS, pes, lambda pe: dict(
            freq=0.0 if _is_pe(pe._frequency) else float(pe._frequency),
            amp=0.0 if _is_pe(pe._amplitude) else float(pe._amplitude),
            phase=0.0 if _is_pe(pe._phase) else float(pe._phase), phase_is_stream=int(_is_pe(pe._phase)))))
        self.ch = pes[0]._channels
        self.state = DeviceBuffer((self.k, 2), np.float64, zero=True)
        self._REQUEST_DEPENDENT = any(_is_pe(pe._phase) or float(pe._phase) != 0.0 for pe in pes)

    def reset(self):
        super().reset()
        self.state.zero_()

    def channels(self):
        return self.ch

    def render(self, start, n):
        L = lib()
        streams = [self.children[name].render(start, n) if name in self.children else None for name in self._STREAMS]
        ws = None if self.k >= SINE_MOD_WALK_MIN_ROWS else self._scratch_of(self.scratch_bytes(n, self.k))
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        check(L.pgx_sine_stateful_bank(out.ptr, n * self.ch, self.k, n, self.ch, self.sr, self.params.ptr,
                                       *_rows(streams[0], n), *_rows(streams[1], n), *_rows(streams[2], n),
                                       self.state.ptr, ptr(ws)), "pgx_sine_stateful_bank")
        return out


class _FunctionGenNode(_Node):
    """Bank of pure FunctionGenPEs of one waveform and channel count: pgx_function_gen_bank, pgx_function_gen_pure's
    sample function with the voice in the grid.  Stateless, like _SineNode: dt, phase and duty are the PE's expressions."""

    def __init__(self, pes):
        super().__init__(pes, {})
        rec = np.zeros(self.k, dtype=_dev.FUNCTION_GEN_PARAMS)
        for i, pe in enumerate(pes):
            rec[i] = (float(np.float64(pe._frequency) / self.sr), float(pe._phase_in), float(pe._duty_cycle))
        self.params = _dev.upload_structs(rec)
        self.saw = int(pes[0]._waveform == FunctionGenPE.WAVE_SAWTOOTH)
        self.ch = pes[0]._channels

    def channels(self):
        return self.ch

    def render(self, start, n):
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        check(lib().pgx_function_gen_bank(out.ptr, n * self.ch, self.k, start, n, self.ch, self.saw, self.params.ptr),
              "pgx_function_gen_bank")
        return out


def _wrap_i64(value: int) -> int:
    """`value` modulo 2^64 as the int64 of pgx_noise_params.consumed (the kernel adds it to `draws` as uint64)."""
    value &= _MASK64
    return value - (1 << 64) if value >> 63 else value


class _NoiseNode(_Node):
    """Bank of NoisePEs of one mode: the PE's kernel with batch = K (pgx_noise_white / _pink / _brown: an instance per
    grid row / workgroup, params[i], state[i]) -- K pink or brown recurrences stepped side by side last as long as one.
    `rec` / `params`: one record per voice, filled as NoisePE._seed_generator fills its one; `state`: the voices' taps
    and levels (pink, brown); `draws`: what every voice has consumed since the seed -- all of them n per render, so one
    number.  Like the PE, `start` is ignored and nothing depends on how the stream is cut.  NoisePE.advance(d) and
    reset_state() on one voice reach `advance` and `reset_voice` (NoisePE._bank_slot): that voice's record alone moves,
    by its `consumed` field -- draws + consumed, modulo 2^64, is where the voice stands."""

    _STATE = ("state", "draws", "params")

    def __init__(self, pes):
        super().__init__(pes, {})
        mode = pes[0]._mode
        self.entry = {NoiseMode.WHITE: "pgx_noise_white", NoiseMode.PINK: "pgx_noise_pink",
                      NoiseMode.BROWN: "pgx_noise_brown"}[mode]
        self.state = None if mode is NoiseMode.WHITE else DeviceBuffer((self.k,), _dev.NOISE_STATE, zero=True)
        self.bank = None             # weakref to the VoiceBank that renders this node (VoiceBank.__init__)
        self._seed()
        for i, pe in enumerate(pes):
            pe._bank_slot = (weakref.ref(self), i)

    def _seed(self) -> None:
        """Every generator back to its seed (seed=None: fresh entropy, per voice, every time), no draw consumed."""
        self.rec = np.concatenate([pe._seed_record() for pe in self.pes])
        self.params = _dev.upload_structs(self.rec)
        self.draws = 0
        self.pending = set()         # voices whose own reset_state() waits for the next render (reset_voice)

    def reset(self):
        """NoisePE._reset_state and what the render after it does: reseed, taps and level zero."""
        self._seed()
        if self.state is not None:
            self.state.zero_()

    def _settle_bank(self) -> None:
        """A window the bank has run ahead by holds samples of the streams as they were: the states go back to the last
        block handed out before a voice's stream is moved."""
        bank = self.bank() if self.bank is not None else None
        if bank is not None:
            bank._settle_window()

    def reset_voice(self, voice: int) -> None:
        """NoisePE.reset_state() (on_start, on_stop) on one voice: that voice alone starts over with the next render."""
        self._settle_bank()
        self.pending.add(voice)

    def quiesce(self, keep=None) -> None:
        """VoiceBank calls this on every node in front of the snapshot a new window goes back to: resets that wait are
        applied first, so that the snapshot holds the records and taps the window is rendered from.  (Nothing waits while
        a window is open: reset_voice and advance settle it before they touch anything.)"""
        if self.pending:
            self._apply_pending()

    def _apply_pending(self) -> None:
        if len(self.pending) == self.k:
            return self.reset()
        for i in sorted(self.pending):
            self.rec[i] = self.pes[i]._seed_record()[0]
            self.rec["consumed"][i] = _wrap_i64(-self.draws)               # consumed + draws = 0: the seed's first draw is next
            if self.state is not None:
                check(lib().pgx_memset(self.state.offset_ptr(i), 0, self.state.dtype.itemsize), "pgx_memset")
        self.params = _dev.upload_structs(self.rec)
        self.pending = set()

    def advance(self, voice: int, draws: int) -> None:
        """NoisePE.advance on one voice: its record alone skips `draws` draws, taps and level stay."""
        self._settle_bank()
        if self.pending:
            self._apply_pending()
        self.rec["consumed"][voice] = _wrap_i64(int(self.rec["consumed"][voice]) + int(draws))
        self.params = _dev.upload_structs(self.rec)

    def channels(self):
        return 1

    def render(self, start, n):
        if self.pending:
            self._apply_pending()
        out = DeviceBuffer((self.k, n, 1), np.float32)
        entry = getattr(lib(), self.entry)
        args = (out.ptr, n, self.k, n, self.draws & _MASK64, self.params.ptr)
        check(entry(*args) if self.state is None else entry(*args, self.state.ptr), self.entry)
        self.draws += n
        return out


class _SawNode(_Node):
    """What the banks of BlitSawPEs (nv = 1) and of SuperSawPEs (nv oscillators per instance) share: `params`, `state`
    and `init_state` are per oscillator; the reset rule; the fused bank kernels with their tables and double-buffered
    states."""

    _STATE = ("state", "last_end")

    def __init__(self, pes, nv, rec, init_state):
        super().__init__(pes, {})
        self.nv = nv
        self.params = _dev.upload_structs(rec)
        self.init_state = init_state
        self.state = DeviceBuffer((self.k * nv, 2), np.float64)
        self.state_alt = None        # the segmented bank reads one state buffer and writes the other
        self.ch = pes[0]._channels
        self.last_end = None
        # a few instances in concurrent time segments (segmented): needs the integrator's closed-form carries
        self.closed_form_ok = closed_form_ok(rec)
        # pgx_supersaw_wide (16 frames per thread): the rotation / recurrence form of the Dirichlet kernel only -- scalar
        # frequency, the automatic M -- and the closed-form carries of the time segments (blit_saw_pe.wide_oscillators_ok)
        self.wide_ok = wide_oscillators_ok(rec, self.sr)
        self.tables = {}             # what depends on the parameters only (pgx_supersaw_*_tables), made on first use

    def channels(self):
        return self.ch

    def prepare(self, start):
        """The reset rule of blit_saw_pe.py: a render that does not continue the previous one starts over."""
        if self.last_end is None or start != self.last_end:
            self.state.upload(self.init_state)

    def wide(self) -> bool:
        return WIDE_SUPERSAW and self.wide_ok and self.nv <= 16

    SEGMENTED_MIN = 0            # instances from which the bank is cut into time segments

    def segmented(self, n: int) -> bool:
        """Fewer instances than fill the chip (a rank's share of a sharded mix; a few BlitSawPEs -- the SuperSaw bank
        kernel with one voice per instance): the fused bank in concurrent time segments (pgx_supersaw_wide /
        pgx_supersaw_bank_seg), carries from the integrator's closed form -- automatic (odd) M, leak < 1."""
        L = lib()
        segments = (L.pgx_supersaw_wide_segments(self.k, self.nv, n) if self.wide()
                    else L.pgx_supersaw_bank_segments(self.k, n))
        return (SEGMENTED_SUPERSAW and self.SEGMENTED_MIN <= self.k < FUSED_SUPERSAW_MIN and self.nv <= 16
                and self.closed_form_ok and segments > 1)

    def saw_tables(self, kind: str) -> DeviceBuffer:
        """The per-oscillator tables of pgx_supersaw_wide ("wide") or pgx_supersaw_bank_seg ("bank")."""
        tables = self.tables.get(kind)
        if tables is None:
            L = lib()
            size, make = ((L.pgx_supersaw_wide_table_bytes, L.pgx_supersaw_wide_tables) if kind == "wide"
                          else (L.pgx_supersaw_bank_table_bytes, L.pgx_supersaw_bank_tables))
            tables = self.tables[kind] = DeviceBuffer((size(self.k, self.nv),), np.uint8)
            check(make(tables.ptr, self.k, self.nv, self.sr, self.params.ptr), f"pgx_supersaw_{kind}_tables")
        return tables

    def _render_bank(self, start, n, amp):
        """[instances][n][channels], the oscillators of an instance summed on chip and scaled by `amp`, on the current
        stream; the states move from `state` to `state_alt` and swap.  The caller has prepared the states."""
        L = lib()
        if self.state_alt is None:
            _ensure_alt(self)
        kind = "wide" if self.wide() else "bank"
        tables = self.saw_tables(kind)
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        if kind == "wide":
            check(L.pgx_supersaw_wide(out.ptr, n * self.ch, self.k, self.nv, n, self.ch, self.state.ptr,
                                      self.state_alt.ptr, amp.ptr, tables.ptr), "pgx_supersaw_wide")
        else:
            check(L.pgx_supersaw_bank_seg(out.ptr, n * self.ch, self.k, self.nv, n, self.ch, self.sr,
                                          self.params.ptr, self.state.ptr, self.state_alt.ptr, amp.ptr,
                                          tables.ptr), "pgx_supersaw_bank_seg")
        _swap_states(self)
        self.last_end = start + n
        return out


class _BlitSawNode(_SawNode):
    SEGMENTED_MIN = 4

    def __init__(self, pes):
        rec = _param_records(_dev.BLITSAW_PARAMS, pes, lambda pe: pe._scalar_params())
        super().__init__(pes, 1, rec, np.stack([pe._initial_state() for pe in pes]))
        self.unit_amp = None

    def reset(self):
        self.last_end = None

    def _render_segments(self, start, n):
        """The SuperSaw bank kernels with one voice per instance and unit instance amplitude: float32(y * 2 amp * 1.0)
        is the oscillator's own sample (pgx_supersaw_wide; pgx_supersaw_bank_seg rounds to float32 twice, the same)."""
        self.prepare(start)
        if self.unit_amp is None:
            self.unit_amp = DeviceBuffer.from_host(np.ones(self.k, dtype=np.float64))
        return self._render_bank(start, n, self.unit_amp)

    def render(self, start, n):
        if self.segmented(n):
            return self._render_segments(start, n)
        self.prepare(start)
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        ws = blitsaw_workspace(self, self.k, n, False)
        check(lib().pgx_blitsaw(out.ptr, n * self.ch, self.k, n, self.ch, self.sr, self.params.ptr,
                                None, 0, None, 0, None, 0, self.state.ptr, ptr(ws), None), "pgx_blitsaw")
        self.last_end = start + n
        return out


class _SuperSawNode(_SawNode):
    """Bank of SuperSawPEs.  From FUSED_SUPERSAW_MIN instances on: one launch, voices summed on chip.  Below
    (a rank's share of a sharded mix): the oscillators of all instances in one launch (`_voices`), then the
    ordered voice sum.  When the node feeds the bank's mix directly the two are pipelined (see
    `mix`): `ahead` then holds the oscillator samples of the block after the last one,
    or `ahead_bank` the bank's output for it."""

    def __init__(self, pes):
        rec = np.concatenate([pe._voice_param_records() for pe in pes])
        super().__init__(pes, len(pes[0]._oscillators), rec, np.concatenate([pe._voice_initial_state() for pe in pes]))
        self.amp = DeviceBuffer.from_host(np.array([float(pe._amplitude) for pe in pes], dtype=np.float64))
        self.ahead = None            # _Ahead(voices buffer; undo: the states and last_end from before)
        self.ahead_bank = None       # _Ahead(bank output; undo: the states swapped back, last_end from before)

    def quiesce(self, keep=None):
        self._forget_ahead("ahead")
        self._forget_ahead("ahead_bank")

    def reset(self):
        self.ahead = self.ahead_bank = None
        self.last_end = None

    def fused(self) -> bool:
        return self.k >= FUSED_SUPERSAW_MIN and self.nv <= 16

    def banked(self, n: int) -> bool:
        """The voices-summed-on-chip kernel with per-voice tables and double-buffered states (pgx_supersaw_bank_seg):
        in time segments for a few instances, one segment each from FUSED_SUPERSAW_MIN instances on."""
        return self.segmented(n) or (self.fused() and self.closed_form_ok)

    def _voices(self, start, n, backup=None):
        """[instances * voices][n] float32 oscillator samples, on the current stream.  backup: a buffer that
        receives the states on entry (written by the oscillator kernel itself: no extra launch)."""
        if self.ahead_bank is not None:
            self._forget_ahead("ahead_bank")
        self.prepare(start)
        voices = DeviceBuffer((self.k * self.nv, n), np.float32)
        ws = blitsaw_workspace(self, self.k * self.nv, n, False)
        check(lib().pgx_blitsaw(voices.ptr, n, self.k * self.nv, n, 1, self.sr, self.params.ptr,
                                None, 0, None, 0, None, 0, self.state.ptr, ptr(ws), ptr(backup)), "pgx_blitsaw")
        self.last_end = start + n
        return voices

    def take_voices(self, start, n):
        """The oscillator samples of (start, n): the ones rendered ahead if they are these, else rendered now
        (after the states went back to where the caller's last block left them)."""
        voices = self.ahead.take(start, n) if self.ahead is not None else None
        self.ahead = None
        return voices if voices is not None else self._voices(start, n)

    def render_ahead(self, start, n) -> None:
        undo = _StateBefore(self, state=DeviceBuffer(self.state.shape, self.state.dtype))
        self.ahead = _Ahead(start, n, self._voices(start, n, backup=undo.state), undo)

    def sum_voices(self, voices, n):
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        check(lib().pgx_supersaw_sum(out.ptr, n * self.ch, self.k, self.nv, n, self.ch, voices.ptr,
                                     self.amp.ptr, None, 0), "pgx_supersaw_sum")
        return out

    def _bank(self, start, n):
        """[instances][n][channels] on the current stream; the states move from `state` to `state_alt` and swap."""
        if self.ahead is not None:
            self._forget_ahead("ahead")
        self.prepare(start)
        return self._render_bank(start, n, self.amp)

    def _bank_undo(self, last_end) -> None:
        _swap_states(self)           # one render happened since: the states it started from are the other buffer
        self.last_end = last_end

    def take_bank(self, start, n):
        """The bank's output for (start, n): the block rendered ahead if it is this one, else rendered now (after the
        states went back to where the caller's last block left them)."""
        out = self.ahead_bank.take(start, n) if self.ahead_bank is not None else None
        self.ahead_bank = None
        return out if out is not None else self._bank(start, n)

    def render_bank_ahead(self, start, n) -> None:
        undo = functools.partial(self._bank_undo, self.last_end)
        self.ahead_bank = _Ahead(start, n, self._bank(start, n), undo)

    def render(self, start, n):
        if self.banked(n):
            return self.take_bank(start, n)
        if self.ahead_bank is not None:
            self._forget_ahead("ahead_bank")
        if self.fused():
            # enough instances to fill the chip with one wave per oscillator: voices summed on chip
            self.prepare(start)
            out = DeviceBuffer((self.k, n, self.ch), np.float32)
            check(lib().pgx_supersaw_bank(out.ptr, n * self.ch, self.k, self.nv, n, self.ch, self.sr,
                                          self.params.ptr, self.state.ptr, self.amp.ptr), "pgx_supersaw_bank")
            self.last_end = start + n
            return out
        return self.sum_voices(self.take_voices(start, n), n)

    def mix(self, bank, start, n):
        """A bank of SuperSawPEs under the mix (a rank's share of a sharded mix: 64 instances at G = 8 -- or all 512).
        The oscillators are the long pole and depend on nothing but time and two carried numbers each, so they
        own the main stream, one block ahead: block k's mix (and, on the oscillator-by-oscillator path, its voice
        sum) runs on the side stream beside block k+1's oscillators.  Nothing on the main stream ever waits for the side stream to catch up (the join at the end is
        enqueued behind the oscillators, which outlast sum + mix): a cross-stream wait that has to wake a stalled
        queue costs ~16 us on this part, a whole launch.  A pull that is not the next block copies the oscillator
        states back (take_voices).  What follows on the library stream -- the all-reduce of this block, a read-back --
        runs behind the next block's oscillators: one block of latency, no throughput."""
        L = lib()
        # (the voices-summed-on-chip bank + mix stay on one stream: with the bank one block ahead and the mix on the
        # side stream a rank's share went from 60.5 to 64.3 us -- the fork / join packets cost more than the 5 us mix)
        if not (PREFETCH_SUPERSAW_VOICES and n >= 4096
                and (PIPELINE_FULL_SUPERSAW_BANK if self.fused() else not self.banked(n))
                and not L.pgx_stream_is_forked()):
            return super().mix(bank, start, n)
        banked = self.banked(n)
        # main stream: this block's oscillators (already there when the previous call rendered them ahead)
        first = self.take_bank(start, n) if banked else self.take_voices(start, n)
        check(L.pgx_stream_fork(), "pgx_stream_fork")                  # side stream: behind this block's oscillators
        try:
            stacked = first if banked else self.sum_voices(first, n)
            ch = stacked.shape[2]
            out = DeviceBuffer((n, ch), np.float32)
            check(L.pgx_mix_batch(out.ptr, stacked.ptr, n * ch, self.k, n * ch), "pgx_mix_batch")
            check(L.pgx_stream_select(0), "pgx_stream_select")
            if banked:
                self.render_bank_ahead(start + n, n)                   # main stream
            else:
                self.render_ahead(start + n, n)
        finally:
            check(L.pgx_stream_join(), "pgx_stream_join")
        return out


class _AnalogOscNode(_Node):
    """Bank of AnalogOscPEs of one waveform: pgx_analog_osc_bank, the PE's kernels with the voice in the grid.  Scalar
    parameters only: the pure form, a function of the frame index (and, for the sawtooth, of where the request begins).
    A PE-valued frequency or duty cycle: the stateful form -- the children's [K][n][1] streams first, then the bank,
    phase and saw value carried per voice in `state`."""

    _STATE = ("state", "last_end")

    def __init__(self, pes, children):
        super().__init__(pes, children)
        rec = np.zeros(self.k, dtype=_dev.OSC_PARAMS)
        for i, pe in enumerate(pes):          # (the scalar of a PE-valued parameter is never read: 0.0 as in the PE's render)
            rec[i] = (0.0 if _is_pe(pe._frequency) else float(pe._frequency),
                      0.0 if _is_pe(pe._duty_cycle) else float(pe._duty_cycle))
        self.params = _dev.upload_structs(rec)
        self.wave = 0 if pes[0]._waveform == AnalogOscPE.WAVE_RECTANGLE else 1
        self.ch = pes[0]._channels
        self.stateful = bool(children)
        self.state = DeviceBuffer((self.k, 2), np.float64, zero=True) if self.stateful else None
        self.last_end = None
        self._REQUEST_DEPENDENT = not self.stateful and self.wave == 1

    def reset(self):
        super().reset()
        self.last_end = None          # the next render restarts at phase 0 / saw -1 (AnalogOscPE._reset_state)

    def channels(self):
        return self.ch

    def render(self, start, n):
        L = lib()
        freq = self.children["frequency"].render(start, n) if "frequency" in self.children else None
        duty = self.children["duty"].render(start, n) if "duty" in self.children else None
        if self.stateful or self.wave:
            self._scratch_of(L.pgx_analog_osc_bank_workspace_bytes(n, self.k))
        out = DeviceBuffer((self.k, n, self.ch), np.float32)
        # the PE's own rule (AnalogOscPE._render): a render that does not continue the previous one starts over
        restart = self.stateful and (self.last_end is None or start != self.last_end)
        check(L.pgx_analog_osc_bank(out.ptr, n * self.ch, self.k, start, n, self.ch, self.sr, self.wave,
                                    self.params.ptr, ptr(freq), n, ptr(duty), n, int(self.stateful), int(restart),
                                    ptr(self.state), ptr(self.ws)), "pgx_analog_osc_bank")
        if self.stateful:
            self.last_end = start + n
        return out


class _FedNode(_Node):
    """A node fed by children["source"]: as many channels as the source has.  The filters among them carry `state`, float64
    [K][channels][STATE_WIDTH], made (zeroed) by the first render -- which is where the channel count is known -- and zeroed
    by reset()."""

    STATE_WIDTH = 0              # numbers carried per voice and channel
    state = None

    def channels(self):
        return self.children["source"].channels()

    def _ensure_state(self, ch: int) -> None:
        if self.state is None:
            self.state = DeviceBuffer((self.k, ch, self.STATE_WIDTH), np.float64, zero=True)

    def reset(self):
        super().reset()
        if self.state is not None:
            self.state.zero_()


class _TransformNode(_FedNode):
    """Bank of TransformPEs whose chains hold the same steps.  The same parameters in every voice (the PWM voice's
    Affine(0.4, 0.5)): one pgx_transform over the stacked K * n * channels elements.  Per-voice parameters (a pitch
    envelope's Affine(300, f_i)): pgx_transform_bank, one launch as well, each voice under its own ops."""

    def __init__(self, pes, children):
        super().__init__(pes, children)
        programs = [pe._lowered.ops() for pe in pes]
        self.nops = len(programs[0])
        self.uniform = all(program == programs[0] for program in programs)
        table = np.zeros((1 if self.uniform else self.k, max(self.nops, 1)), dtype=_dev.TRANSFORM_OP)
        for i, program in enumerate(programs[:table.shape[0]]):
            for j, (code, p0, p1) in enumerate(program):
                table[i, j] = (code, 0, p0, p1)
        self.ops = DeviceBuffer.from_host(table.view(np.uint8))

    def render(self, start, n):
        x = self.children["source"].render(start, n)
        k, _, ch = x.shape
        out = DeviceBuffer((k, n, ch), np.float32)
        if self.uniform:
            check(lib().pgx_transform(out.ptr, x.ptr, k * n * ch, self.ops.ptr, self.nops), "pgx_transform")
        else:
            check(lib().pgx_transform_bank(out.ptr, x.ptr, n * ch, k, self.ops.ptr, self.nops), "pgx_transform_bank")
        return out


class _BiquadNode(_FedNode):
    _STATE = ("state",)
    STATE_WIDTH = 2

    def __init__(self, pes, children):
        super().__init__(pes, children)
        coef = np.array([rbj_coefficients(pe._mode, pe._frequency, pe._q, pe._gain_db, self.sr)
                         for pe in pes], dtype=np.float64)
        self.coef = DeviceBuffer.from_host(coef)
        # one warm-up horizon for the batch (0 = some voice decays too slowly: exact path).  It only matters
        # for small banks, where the library cuts each voice into time segments to fill the machine; a
        # 512-voice bank is one workgroup per voice either way.
        settles = [settle_frames(c[3], c[4]) for c in coef]
        self.settle = 0 if min(settles) == 0 else max(settles)
        fine = [settle_frames_fine(c[3], c[4]) for c in coef] if self.settle else [0]
        self.settle_fine = 0 if min(fine) == 0 else max(fine)      # (a multiple of 16: the on-chip mix's warm-up)
        self.rot_tables = None
        self.tiles_ws = None
        self.entries_ahead = {}      # start -> (n, set): what the tiles of that block enter with, made behind the block before it
        self.tables = None           # per-voice powers of A (pgx_biquad_tables), made on first render
        self.state_alt = None        # (the time-segmented chain reads one buffer and writes the other)

    def _chain_segments(self, n: int) -> int:
        """Time segments of the fused oscillator -> filter launch for a small bank, or 0: not that path."""
        src = self.children["source"]
        if not (SEGMENTED_CHAIN and isinstance(src, _BlitSawNode) and src.ch == 1 and 4 <= self.k <= SEGMENTED_CHAIN_MAX
                and src.wide() and src.closed_form_ok and self.settle > 0):
            return 0
        segs = lib().pgx_blitsaw_biquad_wide_segments(self.k, n, self.settle)
        return segs if segs > 1 else 0

    def mixes_on_chip(self, n: int) -> bool:
        """render_mix(start, n[, gain]) returns the MixPE's block: pgx_voice_tiles, no [voices][frames] layer."""
        src = self.children["source"]
        return (VOICE_TILES and isinstance(src, _BlitSawNode) and src.ch == 1 and self.k >= VOICE_TILES_MIN_VOICES and src.wide()
                and src.closed_form_ok and n >= VOICE_TILES_MIN_FRAMES
                and 0 < self.settle_fine <= VOICE_TILES_MAX_WARM)

    def quiesce(self, keep=None):
        mine = self.entries_ahead.get(keep[0]) if keep is not None else None
        self.entries_ahead = {keep[0]: mine} if mine is not None and mine[0] == keep[1] else {}

    def _power_tables(self) -> DeviceBuffer:
        """Per-voice powers of A (pgx_biquad_tables), made on first use."""
        if self.tables is None:
            L = lib()
            self.tables = DeviceBuffer((self.k, L.pgx_biquad_table_doubles()), np.float64)
            check(L.pgx_biquad_tables(self.tables.ptr, self.coef.ptr, self.k), "pgx_biquad_tables")
        return self.tables

    def _mix_tables(self) -> DeviceBuffer:
        if self.rot_tables is None:
            L = lib()
            saw_tables, tables = self.children["source"].saw_tables("wide"), self._power_tables()
            assert L.pgx_voice_tiles_max_warm() == VOICE_TILES_MAX_WARM
            self.rot_tables = DeviceBuffer((L.pgx_voice_tiles_table_bytes(self.k),), np.uint8)
            check(L.pgx_voice_tiles_tables(self.rot_tables.ptr, saw_tables.ptr, self.coef.ptr, tables.ptr, self.k),
                  "pgx_voice_tiles_tables")
        return self.rot_tables

    def render_mix(self, start, n, gain=None, streaming=False):
        """The voices' mix (times `gain`, [K][n] float32, voice by voice) as one (n, 1) block.  streaming: (start + n, n)
        is expected next -- what its tiles enter with (the oscillators' phases decide it: pgx_voice_tiles_entries) is made
        in the launch that adds this block's rows, off the next block's critical chain."""
        L = lib()
        src = self.children["source"]
        self._ensure_state(1)
        _ensure_alt(self, src)
        slot = -1
        mine = self.entries_ahead.pop(start, None)
        if mine is not None and mine[0] == n and src.last_end == start:
            slot = mine[1]
        stale = [s0 for s0, (n0, _) in self.entries_ahead.items() if s0 != start + n or n0 != n]
        if stale:
            self.entries_ahead = {}
        src.prepare(start)
        rot_tables = self._mix_tables()
        need = L.pgx_voice_tiles_workspace_bytes(self.k, n, self.settle_fine)
        if self.tiles_ws is None or self.tiles_ws.nbytes < need:
            self.tiles_ws = DeviceBuffer((need,), np.uint8)
            slot = -1
        out = DeviceBuffer((n, 1), np.float32)
        nxt = ((slot if slot >= 0 else 0) ^ 1) if streaming else -1
        check(L.pgx_voice_tiles(out.ptr, self.k, n, rot_tables.ptr, src.state.ptr, src.state_alt.ptr,
                                self.state.ptr, self.state_alt.ptr, ptr(gain), n, self.settle_fine, self.tiles_ws.ptr,
                                slot, nxt), "pgx_voice_tiles")
        if streaming:
            self.entries_ahead[start + n] = (n, nxt)
        _swap_states(src, self)
        src.last_end = start + n
        return out

    def mix(self, bank, start, n):
        if self.mixes_on_chip(n):
            return self.render_mix(start, n, streaming=bank.streaming)
        return super().mix(bank, start, n)

    def _render_chain_segments(self, start, n):
        """A small bank (a rank's share of C5): oscillator -> filter as ONE launch in concurrent time segments instead of
        the segmented oscillator bank followed by the batched settled biquad (two kernels and the dispatch gap between
        them on the block's critical chain).  States are read from one buffer and written to another."""
        L = lib()
        src = self.children["source"]
        self._ensure_state(1)
        _ensure_alt(self, src)
        src.prepare(start)
        saw_tables, tables = src.saw_tables("wide"), self._power_tables()
        out = DeviceBuffer((self.k, n, 1), np.float32)
        check(L.pgx_blitsaw_biquad_wide_seg(out.ptr, n, self.k, n, saw_tables.ptr, src.state.ptr, src.state_alt.ptr,
                                            self.coef.ptr, tables.ptr, self.state.ptr, self.state_alt.ptr,
                                            None, n, self.settle), "pgx_blitsaw_biquad_wide_seg")
        _swap_states(src, self)
        src.last_end = start + n
        return out

    def render(self, start, n):
        L = lib()
        src = self.children["source"]
        if self._chain_segments(n):
            return self._render_chain_segments(start, n)
        if isinstance(src, _BlitSawNode) and src.ch == 1 and self.k >= FUSED_VOICE_MIN:
            # oscillator -> filter without the [K][frames] oscillator buffer (pgx_blitsaw_biquad_bank)
            self._ensure_state(1)
            src.prepare(start)
            out = DeviceBuffer((self.k, n, 1), np.float32)
            if src.wide():
                # sixteen frames per thread (pgx_blitsaw_biquad_wide): the oscillator's and the filter's per-voice tables
                saw_tables, tables = src.saw_tables("wide"), self._power_tables()
                check(L.pgx_blitsaw_biquad_wide(out.ptr, n, self.k, n, saw_tables.ptr, src.state.ptr, self.coef.ptr,
                                                tables.ptr, self.state.ptr, None, n), "pgx_blitsaw_biquad_wide")
            else:
                check(L.pgx_blitsaw_biquad_bank(out.ptr, n, self.k, n, self.sr, src.params.ptr, src.state.ptr,
                                                self.coef.ptr, self.state.ptr), "pgx_blitsaw_biquad_bank")
            src.last_end = start + n
            return out
        x = src.render(start, n)
        ch = x.shape[2]
        self._ensure_state(ch)
        tables = self._power_tables()
        need = L.pgx_biquad_workspace_bytes(self.k, n, ch, self.settle)
        ws = self._scratch_of(need) if need else None
        out = DeviceBuffer((self.k, n, ch), np.float32)
        check(L.pgx_biquad_const(out.ptr, n * ch, x.ptr, n * ch, self.k, n, ch, self.coef.ptr,
                                 tables.ptr, self.settle, self.state.ptr, ptr(ws)), "pgx_biquad_const")
        return out


class _RowFilterNode(_FedNode):
    """What _BiquadVarNode and _SvfNode share -- banks of a PE whose kernel takes the voice in the grid: `params`, one
    BIQUAD_VAR_PARAMS record per voice as the PE's _render fills it (MODES: the PE's mode -> index table); `gains`, what
    `_voice_gains` makes of each voice's 10^(gain_db / 40); the rule of the rows; the call, `_filter`."""

    _STATE = ("state",)
    MODES = None

    def __init__(self, pes, children):
        super().__init__(pes, children)
        rec = np.zeros(self.k, dtype=_dev.BIQUAD_VAR_PARAMS)
        for i, pe in enumerate(pes):          # (0.0 for a PE-valued parameter, never read)
            rec[i]["freq"] = 0.0 if pe._freq_is_pe else float(pe._frequency)
            rec[i]["q"] = 0.0 if pe._q_is_pe else float(pe._q)
            rec[i]["gain_db"] = float(pe._gain_db)
            rec[i]["mode"] = self.MODES[pe._mode]
        self.params = _dev.upload_structs(rec)
        self.gains = DeviceBuffer.from_host(np.array([self._voice_gains(10.0 ** (pe._gain_db / 40.0)) for pe in pes],
                                                     dtype=np.float64))

    def _filter(self, entry: str, x, n, *between):
        """-> out [K][n][ch] of lib().<entry>(out, out_stride, x, x_stride, K, n, ch, sr, params, gains, *between, state,
        workspace).  From _walk_min_rows() rows (voices x channels) on no workspace is passed -- enough rows to give every
        CU a workgroup: each row walked by one workgroup, one launch, the coefficients evaluated once, instead of the
        segmented plan's reduce and apply."""
        L = lib()
        ch = x.shape[2]
        self._ensure_state(ch)
        walk = self.k * ch >= self._walk_min_rows()
        need = 0 if walk else self.k * L.pgx_scan2_workspace_bytes(n, ch)
        ws = self._scratch_of(need) if need else None
        out = DeviceBuffer((self.k, n, ch), np.float32)
        check(getattr(L, entry)(out.ptr, n * ch, *_rows(x, n * ch), self.k, n, ch, self.sr, self.params.ptr, self.gains.ptr,
                                *between, self.state.ptr, ptr(ws)), entry)
        return out


class _BiquadVarNode(_RowFilterNode):
    """Bank of BiquadPEs whose cutoff and / or Q is a PE (the swept filter of a subtractive voice):
    pgx_biquad_varying_bank, the PE's kernel with the voice in the grid.  The children's [K][n][ch] and [K][n][1] streams
    first, then one call; mode, gain_db and the scalar of a parameter that is no PE are per voice (`params`, `gains`),
    {x1, x2, y1, y2} is carried per voice and channel in `state`.  (No subclass of _BiquadNode: it takes none of the
    on-chip mixes that class makes as the root.)"""

    STATE_WIDTH = 4
    MODES = _MODE_INDEX

    @staticmethod
    def _voice_gains(gain_a):
        return gain_a, math.sqrt(gain_a)

    def _walk_min_rows(self) -> int:
        return BIQUAD_VAR_WALK_MIN_ROWS

    def render(self, start, n):
        x = self.children["source"].render(start, n)
        freq = self.children["frequency"].render(start, n) if "frequency" in self.children else None
        q = self.children["q"].render(start, n) if "q" in self.children else None
        return self._filter("pgx_biquad_varying_bank", x, n, *_rows(freq, n), *_rows(q, n))


class _SvfNode(_RowFilterNode):
    """Bank of SVFilterPEs with scalar frequency and Q: pgx_svf_bank, the PE's kernel with the voice in the grid.  Per voice:
    `params` and `gains` as SVFilterPE._render fills them (mode and gain_db are data, not part of the key) and `coef`, the
    nine numbers of svfilter_pe.svf_coefficients the PE uploads -- so each voice's samples and {s0, s1} are the PE's, bit for
    bit, while the node passes the workspace (the PE's segmented plan)."""

    STATE_WIDTH = 2
    MODES = _SVF_MODE_INDEX

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.coef = DeviceBuffer.from_host(np.array([svf_coefficients(pe._mode, pe._frequency, pe._q, pe._gain_db, self.sr)
                                                     for pe in pes], dtype=np.float64))

    @staticmethod
    def _voice_gains(gain_a):
        return gain_a

    def _walk_min_rows(self) -> int:
        return SVF_WALK_MIN_ROWS

    def render(self, start, n):
        return self._filter("pgx_svf_bank", self.children["source"].render(start, n), n, None, 0, None, 0, self.coef.ptr)


class _LadderNode(_Windowed, _FedNode):
    """Bank of LadderPEs.  The ladder kernel is latency-bound (two waves per CU, most of the chip idle) and its
    input, a bank of scalar oscillators, is a pure function of time plus a few carried numbers -- so while block k
    goes through the ladder on the main stream, the oscillators of block k+1 are rendered on the side stream.
    The speculation is undone exactly if the next pull is not the next block: the oscillator states are
    snapshot before it and copied back."""

    _STATE = ("state",)
    STATE_WIDTH = 9

    def quiesce(self, keep=None):
        self._settle_window()
        self._forget_ahead("ahead")

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.params = _dev.upload_structs(_param_records(_dev.LADDER_PARAMS, pes, lambda pe: pe._scalar_params()))
        settles = [pe._settle_frames() for pe in pes]
        self.settle = 0 if min(settles) == 0 else max(settles)     # one warm-up length for the batch
        self.accurate = max(pe._accurate_frames() for pe in pes) if self.settle else 0
        # a voice without an estimate (at or above self-oscillation, a very slow decay): warm-up lengths by trial, the
        # device check decides (ladder_pe.SettleOptimist) -- an oscillator bank locks a saturating ladder to itself
        from .ladder_pe import SettleOptimist
        self.optimist = SettleOptimist() if self.settle == 0 else None
        self.ahead = None          # _Ahead(the input rendered ahead of the caller; undo: the oscillators' _StateBefore)
        self.is_root = False       # directly under the bank's mix: may hand out rows of a window (VoiceBank.__init__)
        self._reset_windows(LADDER_WINDOW_FIRST)     # win.undo: (ladder state, the oscillators' _StateBefore)

    # ---- windows (root node only).  A lane of k_ladder_segments integrates 1024 warm-up samples to emit its share of the
    # block -- 94 frames of a 48 000-frame block of 64 instances: 92 % of the work is warm-up.  A stream of equal blocks
    # is therefore rendered several blocks at a time (2, 4, 8: the share per lane grows, the warm-up does not) and handed
    # out block by block as rows of that window.  A pull that is not the next block puts the states back to the
    # window's start and renders the consumed part again, quietly (exact: the same kernels over the same frames).
    def _settle_window(self) -> None:
        left = self._close_window()
        if left is None:
            return
        first, served, (ladder_state, oscillators_before) = left
        self.ahead = None                                # (the oscillators go back further than that)
        _copy_state(self.state, ladder_state)
        oscillators_before()
        if served > first:
            self._render_now(first, served - first)

    def render(self, start, n):
        offset = self._next_row(start, n)
        if offset is not None:
            return _Rows(self.win.buf, offset, n)
        closed = self.win          # (held to the end of this pull: its buffers return to the pool behind what is enqueued here)
        if closed is not None:
            self._settle_window()
        streaming = self._continues(start, n)
        src = self.children["source"]
        if (LADDER_WINDOWS and self.is_root and streaming and n >= 4096 and self.state is not None
                and isinstance(src, _SawNode) and not lib().pgx_stream_is_forked()):
            blocks = self._window_blocks(n, LADDER_WINDOW_MAX, LADDER_WINDOW_FRAMES)
            if blocks > 1:
                ahead = self.ahead
                if ahead is not None and not (ahead.start == start and ahead.n == n * blocks):
                    self._forget_ahead("ahead")
                    ahead = None
                ladder_state = DeviceBuffer(self.state.shape, self.state.dtype)
                _copy_state(ladder_state, self.state)
                if ahead is not None:                    # the oscillators already ran on: their states before that
                    before = _StateBefore(src, state=DeviceBuffer(src.state.shape, src.state.dtype))
                    _copy_state(before.state, ahead.undo.state)
                    before.last_end = ahead.undo.last_end
                else:
                    before = _StateBefore(src)
                big = self._render_now(start, n * blocks)
                self._open_window(start, blocks, n, big, (ladder_state, before))
                return _Rows(big, 0, n)
        else:
            self.grow = LADDER_WINDOW_FIRST
        return self._render_now(start, n)

    def reset(self):
        self._reset_windows(LADDER_WINDOW_FIRST)
        self.ahead = None                            # (nothing to undo: the oscillators start over anyway)
        super().reset()

    def _render_now(self, start, n):
        L = lib()
        src = self.children["source"]
        x = self.ahead.take(start, n) if self.ahead is not None else None
        self.ahead = None
        if x is None:
            x = src.render(start, n)
        ch = x.shape[2]
        self._ensure_state(ch)
        out = DeviceBuffer((self.k, n, ch), np.float32)
        settle, accurate = self.settle, self.accurate
        if self.optimist is not None and n >= 8192:
            settle, accurate = self.optimist.settle(n)
        need = L.pgx_ladder_workspace_bytes(self.k, n, ch, settle)
        if need and (self.ws is None or self.ws.nbytes < need):
            counters = None if self.ws is None else self.ws.rows(0, 16)
            self.ws = DeviceBuffer((need,), np.uint8, zero=True)
            if counters is not None:                     # cumulative counters at the head of the workspace
                check(L.pgx_memcpy_d2d(self.ws.ptr, counters.ptr, 16), "pgx_memcpy_d2d")

        def ladder():
            check(L.pgx_ladder(out.ptr, n * ch, x.ptr, n * ch, self.k, n, ch, self.sr, self.params.ptr,
                               None, None, None, self.state.ptr, settle, accurate,
                               ptr(self.ws) if need else None), "pgx_ladder")
            if self.optimist is not None and need and settle:
                self.optimist.launched(self.ws, settle, n, self.k * ch)

        speculate = (PREFETCH_LADDER_INPUT and isinstance(src, _SawNode) and n >= 4096
                     and not L.pgx_stream_is_forked())
        if not speculate:
            ladder()
            return out
        # The ladder stays on the main stream, in front of everything else of this block: no cross-stream wait on
        # the chain ladder -> finish -> mix -> next ladder, and its waves are placed before the oscillators' are.
        check(L.pgx_stream_fork(), "pgx_stream_fork")              # side stream: behind x
        try:
            check(L.pgx_stream_select(0), "pgx_stream_select")
            ladder()
            check(L.pgx_stream_select(1), "pgx_stream_select")
            before = _StateBefore(src)
            nxt = src.render(start + n, n)                         # side stream, next to the ladder
        finally:
            check(L.pgx_stream_join(), "pgx_stream_join")          # what follows the ladder also follows the oscillators
        self.ahead = _Ahead(start + n, n, nxt, before)
        return out


class _CombNode(_FedNode):
    """Bank of CombPEs with scalar frequency and feedback: every voice's D * C polyphase chains in one launch
    (two when the block is long enough to be cut into time segments), per-voice delay / feedback / ring."""

    _STATE = ("ring", "total", "parity")

    def __init__(self, pes, children):
        super().__init__(pes, children)
        rec = np.concatenate([pe._param_record() for pe in pes])
        self.params = _dev.upload_structs(rec)
        self.d_min, self.d_max = int(rec["delay"].min()), int(rec["delay"].max())
        self.rows = int(rec["buffer_len"].max())
        self.ring = None
        self.total = 0
        self.parity = 0

    def reset(self):
        super().reset()
        # CombPE has no _reset_state hook (comb_pe.py): only start / stop clear the ring -- VoiceBank.reset is
        # called from those
        self.ring = None

    def render(self, start, n):
        L = lib()
        x = self.children["source"].render(start, n)
        ch = x.shape[2]
        if self.ring is None:
            self.ring = DeviceBuffer((self.k, 2, self.rows, ch), np.float64, zero=True)
            self.total, self.parity = 0, 0
        need = L.pgx_comb_workspace_bytes(self.k, n, ch, self.d_max, 0)
        ws = self._scratch_of(need) if need else None
        out = DeviceBuffer((self.k, n, ch), np.float32)
        check(L.pgx_comb(out.ptr, n * ch, x.ptr, n * ch, self.k, n, ch, self.sr, self.params.ptr, self.d_min,
                         self.d_max, None, None, 1.0, 1, self.ring.ptr, self.rows, self.total, self.parity, None,
                         ptr(ws)), "pgx_comb")
        self.total += n
        self.parity ^= 1
        return out


class _GateNode(_Node):
    def __init__(self, pes):
        super().__init__(pes, {})
        self.params = _dev.upload_structs(_param_records(_dev.GATE_PARAMS, pes, lambda pe: pe._gate_params()))

    def channels(self):
        return 1

    def render(self, start, n):
        out = DeviceBuffer((self.k, n, 1), np.float32)
        check(lib().pgx_periodic_gate(out.ptr, n, self.k, start, n, self.params.ptr), "pgx_periodic_gate")
        return out


class _TriggerNode(_Node):
    """Bank of PeriodicTriggers: K rows of impulses in one launch (pgx_periodic_trigger_bank), integer arithmetic."""

    def __init__(self, pes):
        super().__init__(pes, {})
        self.periods = DeviceBuffer.from_host(np.array([pe._period for pe in pes], dtype=np.int64))
        self.phases = DeviceBuffer.from_host(np.array([pe._phase_samples for pe in pes], dtype=np.int64))
        self.amplitudes = DeviceBuffer.from_host(np.array([float(pe._amp) for pe in pes], dtype=np.float32))

    def channels(self):
        return 1

    def render(self, start, n):
        out = DeviceBuffer((self.k, n, 1), np.float32)
        check(lib().pgx_periodic_trigger_bank(out.ptr, n, self.k, start, n, self.periods.ptr, self.phases.ptr,
                                              self.amplitudes.ptr), "pgx_periodic_trigger_bank")
        return out


class _AdsrTriggeredNode(_Node):
    """Bank of AdsrTriggeredPEs: one pgx_adsr_triggered call with batch = K over the trigger rows, {state, env,
    sustain_ends_at} carried per voice.  A plain node: nothing of it runs ahead of the stream (_AdsrGatedNode's side-stream
    walk is for the fused PeriodicGate)."""

    _STATE = ("state",)

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.params = _dev.upload_structs(_param_records(_dev.ADSR_PARAMS, pes, lambda pe: pe._adsr_params()))
        self.state = DeviceBuffer((self.k, 3), np.float64, zero=True)

    def reset(self):
        super().reset()
        self.state.zero_()

    def channels(self):
        return 1

    def render(self, start, n):
        L = lib()
        trig = self.children["trigger"].render(start, n)
        ws = self._scratch_of(L.pgx_adsr_workspace_bytes(self.k, n))
        out = DeviceBuffer((self.k, n, 1), np.float32)
        check(L.pgx_adsr_triggered(out.ptr, n, *_rows(trig, n), self.k, start, n, self.params.ptr,
                                   self.state.ptr, ws.ptr), "pgx_adsr_triggered")
        return out


class _AdsrGatedNode(_Node):
    _STATE = ("state", "last")

    def quiesce(self, keep=None):
        """keep = (start, n): the render that follows -- envelopes walked ahead for exactly that render stay (they were
        made from `state`, which they leave alone: a snapshot taken now is the state before them)."""
        if keep is not None and self.ahead is not None and (self.ahead.start, self.ahead.n) == tuple(keep):
            return
        self.forget_ahead()

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.params = _dev.upload_structs(_param_records(_dev.ADSR_PARAMS, pes, lambda pe: pe._adsr_params()))
        self.state = DeviceBuffer((self.k, 3), np.float64, zero=True)
        self.ahead = None            # _Ahead(envelopes; nothing to undo): render_ahead
        self.state_next = None       # ... which reads `state` and leaves the states after the block here
        self.ring = []               # ... into one of three envelope buffers of its own, used in turn: [buffer, event]
        self.ring_at = 0             #     (event: recorded behind the mix that read the buffer last; None: never used)
        self.last = None             # (start, n) of the last block handed out

    def _scratch(self, n):
        need = lib().pgx_adsr_workspace_bytes(self.k, n)
        if self.ahead is not None and (self.ws is None or self.ws.nbytes < need):
            check(lib().pgx_stream_wait_detached(), "pgx_stream_wait_detached")     # (the side stream may still be using the old one)
        return self._scratch_of(need)

    def reset(self):
        self.forget_ahead()
        self.last = None
        super().reset()
        self.state.zero_()

    # ---- one block ahead (VoiceBank.render_mix): the envelopes depend on nothing but time and three carried numbers
    # each, and their walk is a latency chain that leaves the machine to everybody else -- so block k+1's are walked
    # on the side stream while block k is mixed and block k+1's oscillators run; nobody waits for them until block
    # k+1's mix.  A pull that is not the next block puts the states back.
    def forget_ahead(self) -> None:
        """(nothing to put back: a block rendered ahead reads `state` and writes `state_next`)"""
        ahead, self.ahead = self.ahead, None
        if ahead is not None:
            check(lib().pgx_stream_wait_detached(), "pgx_stream_wait_detached")

    def take_ahead(self, start, n):
        """The envelopes of (start, n) if they were rendered ahead (the main stream then waits for them, which by now is
        no wait) -- their end states become the carried ones; else None, nothing having moved."""
        ahead = self.ahead
        if ahead is None:
            return None
        self.forget_ahead()
        env = ahead.take(start, n)
        if env is not None:
            self.state, self.state_next = self.state_next, self.state
            self.last = (start, n)
        return env

    def render_ahead(self, start, n, also=None, edges_here=False, behind_main=False) -> None:
        """Fused PeriodicGate only.  Edge search and walk go to the side stream, which starts behind what the main
        stream holds so far and is left running (pgx_stream_detach).  also: called on the side stream, in front of the
        walk (the on-chip mix's entries of the same block)."""
        L = lib()
        gate_node = self.children["gate"]
        if self.state_next is None:
            self.state_next = DeviceBuffer(self.state.shape, self.state.dtype)
        scratch = self._scratch(n)
        # The walk depends on nothing the main stream is doing: it only must not overwrite an envelope buffer a mix is
        # still reading.  With three buffers of the node's own used in turn, the last reader of the one to be written is
        # the mix of three blocks ago, long finished: the side stream waits for THAT (an event recorded behind it,
        # mark_consumed) instead of for the main stream's tail -- no queue to be woken (~17 us), and the walk starts as
        # soon as the one before it has ended.  A buffer's first use starts behind the main stream's tail (it comes
        # from the pool: its previous owner's kernels are somewhere on the main stream).
        # (A full bank's walk -- 512 envelopes x 8 waves -- is better started behind the block's oscillators, whose SIMDs it
        # would share from their first tile otherwise, and written to the pool's most recently freed buffer: three
        # 98 MB buffers in turn are more than the memory-side cache holds.  137 us per block against 144.)
        if self.k > EARLY_WALK_MAX_VOICES:
            out, seen = DeviceBuffer((self.k, n, 1), np.float32), None
            if edges_here and also is None:
                # (the caller enqueues the block's voices right behind this call: an edge search that starts beside them --
                # short, parallel -- finds no free SIMD for 20 us, and the walk waits for it.  It goes in front of them, on
                # the main stream; the library forks behind it)
                try:
                    check(L.pgx_adsr_gated_periodic_to(out.ptr, n, self.k, start, n, gate_node.params.ptr, self.params.ptr,
                                                       self.state.ptr, self.state_next.ptr, scratch.ptr, 1),
                          "pgx_adsr_gated_periodic_to")
                finally:
                    if L.pgx_stream_is_forked():
                        check(L.pgx_stream_detach(), "pgx_stream_detach")
                self.ahead = _Ahead(start, n, out)
                return
        else:
            if not self.ring or self.ring[0][0].shape != (self.k, n, 1):
                self.ring = [[DeviceBuffer((self.k, n, 1), np.float32), None] for _ in range(3)]
            self.ring_at = (self.ring_at + 1) % 3
            out, seen = self.ring[self.ring_at]
        if seen is None or behind_main:       # (behind_main: the states this walk starts from were written on the main stream)
            check(L.pgx_stream_fork(), "pgx_stream_fork")
        else:
            check(L.pgx_stream_fork_after(seen.ptr), "pgx_stream_fork_after")
        try:
            if also is not None:                 # (first: short, and nothing behind it on this stream depends on it)
                also()
            check(L.pgx_adsr_gated_periodic_to(out.ptr, n, self.k, start, n, gate_node.params.ptr, self.params.ptr,
                                               self.state.ptr, self.state_next.ptr, scratch.ptr, 0),
                  "pgx_adsr_gated_periodic_to")
        finally:
            check(L.pgx_stream_detach(), "pgx_stream_detach")
        self.ahead = _Ahead(start, n, out)

    def mark_consumed(self, env) -> None:
        """Called behind the launch that read `env` (a buffer take_ahead handed out): from here on the main stream is done
        with it."""
        for slot in self.ring:
            if slot[0] is env:
                if slot[1] is None:
                    slot[1] = _dev.Event()
                slot[1].record()

    def channels(self):
        return 1

    def fused_gate(self) -> bool:
        return isinstance(self.children["gate"], _GateNode)

    def render(self, start, n, detach=False):
        """detach=True (fused gate only): the envelope walk is left running on the side stream;
        the caller joins (pgx_stream_join) before using the result."""
        if self.ahead is not None:
            self.forget_ahead()
        self.last = (start, n)
        out = DeviceBuffer((self.k, n, 1), np.float32)
        gate_node = self.children["gate"]
        if isinstance(gate_node, _GateNode):
            # PeriodicGate feeding the envelope: evaluate the gate inside the envelope kernel
            check(lib().pgx_adsr_gated_periodic(out.ptr, n, self.k, start, n, gate_node.params.ptr,
                                                self.params.ptr, self.state.ptr, self._scratch(n).ptr,
                                                1 if detach else 0), "pgx_adsr_gated_periodic")
            return out
        gate = gate_node.render(start, n)
        check(lib().pgx_adsr_gated(out.ptr, n, gate.ptr, n, self.k, n, self.params.ptr, self.state.ptr,
                                   self._scratch(n).ptr), "pgx_adsr_gated")
        return out


class _GainNode(_FedNode):
    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.gains = None
        if "gain" not in children:
            self.gains = [float(np.float32(pe._gain)) for pe in pes]

    def mixes_on_chip(self, n):
        """(a PE gain over the chain that mixes on chip -- `mix` also wants the gain to be one channel)"""
        source = self.children["source"]
        return self.gains is None and isinstance(source, _BiquadNode) and source.mixes_on_chip(n)

    def mix(self, bank, start, n):
        """Voices that end in GainPE(x, gain=<PE>): the per-voice multiply goes into the launch that adds the voices --
        pgx_voice_tiles where the chain under the gain mixes on chip, else pgx_gain_mix_batch.  AdsrGatedPE(PeriodicGate)
        envelopes (a fused gate) run one block ahead on the side stream from a stream's second block on."""
        if self.gains is not None:
            return super().mix(bank, start, n)
        L = lib()
        gain, source = self.children["gain"], self.children["source"]
        gated = isinstance(gain, _AdsrGatedNode)
        fused = gated and gain.fused_gate()
        ahead = fused and ENVELOPE_AHEAD and n >= 1024 and not L.pgx_stream_is_forked()
        walk_ahead = ahead and gain.last == (start - n, n)         # equal blocks, one after the other: the next one is walked ahead

        def envelopes():
            """-> (this block's gain rows, were they walked here?): the ones walked ahead while the last block was mixed (the
            wait for the side stream is no wait by now), else -- a stream's first block, a seek, another kind of gain --
            rendered now."""
            g = gain.take_ahead(start, n) if ahead and gain.ahead is not None else None
            return (g, False) if g is not None else (gain.render(start, n), True)

        if self.mixes_on_chip(n) and gain.channels() == 1:
            # GainPE(BiquadPE(BlitSawPE), gain=<PE>) voices: oscillator -> filter -> x gain -> mix in one kernel
            # (pgx_voice_tiles).  The gains come first -- the kernel reads them -- so envelopes with a fused gate are
            # walked one block ahead on the side stream, the next block's walk enqueued in front of this block's voices.
            g, walked_here = envelopes()
            if walk_ahead:
                # (walked_here: this block's walk ran on the MAIN stream and left the states the next one starts from there --
                # the side stream, which otherwise only waits for its envelope buffer's last reader, has to start behind it)
                gain.render_ahead(start + n, n, edges_here=True, behind_main=walked_here)
            out = source.render_mix(start, n, gain=g, streaming=walk_ahead)
        else:
            # fuse the per-voice multiply into the mix.  The gain sub-graph (envelopes: few, latency-bound waves) and the
            # signal sub-graph (oscillators and filters: VALU-bound) share nothing, so they are enqueued on two streams
            # and overlap.
            if not fused:
                check(L.pgx_stream_fork(), "pgx_stream_fork")
                try:
                    g = gain.render(start, n)
                    check(L.pgx_stream_select(0), "pgx_stream_select")
                    x = source.render(start, n)
                finally:
                    check(L.pgx_stream_join(), "pgx_stream_join")
            elif ahead and gain.ahead is not None:
                # this block's envelopes were walked while the last block was mixed.  (Multiplying by them in the chain's
                # own kernel -- the mix then reads one [voices][frames] layer, not two: 35 -> 17 us -- made the oscillators
                # depend on the envelopes; the next walk had to start in front of them and shared their SIMDs from the first
                # tile: 512 voices 139 us per block against 137, 256 voices 91 against 90.  Removed.)
                x = source.render(start, n)
                g, _ = envelopes()                      # (a seek: walked now, behind the oscillators)
            else:
                # nothing was walked ahead: edge search first (parallel, short), then the walk detached on the side stream
                try:
                    g = gain.render(start, n, detach=True)
                    x = source.render(start, n)
                finally:
                    if L.pgx_stream_is_forked():        # the fork happens inside the detached render
                        check(L.pgx_stream_join(), "pgx_stream_join")
            if walk_ahead:
                # from a stream's second block on.  Between this block's oscillators and its mix: the side stream starts
                # behind what the main stream holds at the fork.  Behind the mix the walk -- edge search, walk, a
                # cross-stream wake-up: longer than the next block's oscillators -- became the critical path (a rank's 64
                # voices: 66 -> 89 us per block); in front of the oscillators it shares the SIMDs with them from their
                # first tile (66 -> 74 us; 512 voices 133 -> 143 us)
                gain.render_ahead(start + n, n)
            ch, gch = x.shape[2], g.shape[2]
            out = DeviceBuffer((n, ch), np.float32)
            check(L.pgx_gain_mix_batch(out.ptr, x.ptr, n * ch, g.ptr, n * gch, self.k, n, ch, gch), "pgx_gain_mix_batch")
        if gated:
            gain.mark_consumed(g)                       # (behind the launch that read them)
        return out

    def render(self, start, n):
        L = lib()
        x = self.children["source"].render(start, n)
        ch = x.shape[2]
        out = DeviceBuffer((self.k, n, ch), np.float32)
        if self.gains is None:
            g = self.children["gain"].render(start, n)
            # elementwise over the stacked [K*n] frames: one launch for all voices
            check(L.pgx_gain_vec(out.ptr, x.ptr, g.ptr, self.k * n, ch, g.shape[2]), "pgx_gain_vec")
        elif len(set(self.gains)) == 1:
            check(L.pgx_gain_const(out.ptr, x.ptr, self.k * n * ch, self.gains[0]), "pgx_gain_const")
        else:
            for i, gval in enumerate(self.gains):
                check(L.pgx_gain_const(out.offset_ptr(i * n * ch), x.offset_ptr(i * n * ch), n * ch, gval),
                      "pgx_gain_const")
        return out


class _PanNode(_Node):
    """Bank of SpatialPEs under SpatialLinear or SpatialConstantPower (one class per bank): pgx_pan with the voice in the
    grid.  Scalar azimuths: uploaded once and turned into `gains` [K][2] by pgx_pan_gains when the node is built -- the
    device function pgx_pan evaluates, so no transcendental per frame afterwards.  PE azimuths: a child level of (n, 1)
    streams, the gains evaluated per frame.  Nothing is carried.  As a level: `render`, one pgx_pan_bank.  As the root:
    `render_mix`, one pgx_pan_mix_batch straight into the mix's (n, 2) block."""

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.mode = int(pes[0]._method._constant_power)
        self.gains = None
        if "azimuth" not in children:
            self.azimuths = DeviceBuffer.from_host(np.array([float(pe._azimuth) for pe in pes], dtype=np.float32))
            self.gains = DeviceBuffer((self.k, 2), np.float32)
            check(lib().pgx_pan_gains(self.gains.ptr, self.azimuths.ptr, self.k, self.mode), "pgx_pan_gains")

    def channels(self):
        return 2

    def _render(self, start, n, mix: bool):
        x = self.children["source"].render(start, n)
        az = self.children["azimuth"].render(start, n) if self.gains is None else None
        ch = x.shape[2]
        # what both entries take behind `out`: the source rows, then the gains or the azimuth rows
        rows = (*_rows(x, n * ch), self.k, n, ch, ptr(self.gains), *_rows(az, n), self.mode)
        if mix:
            out = DeviceBuffer((n, 2), np.float32)
            check(lib().pgx_pan_mix_batch(out.ptr, *rows), "pgx_pan_mix_batch")
        else:
            out = DeviceBuffer((self.k, n, 2), np.float32)
            check(lib().pgx_pan_bank(out.ptr, n * 2, *rows), "pgx_pan_bank")
        return out

    def render(self, start, n):
        return self._render(start, n, mix=False)

    def render_mix(self, start, n):
        """The voices' mix as one (n, 2) block: what `render` followed by pgx_mix_batch gives, bit for bit."""
        return self._render(start, n, mix=True)

    def mix(self, bank, start, n):
        if FUSED_PAN_MIX:
            # voices end in SpatialPE(x, <panner>): the pan fused into the mix, each voice's mono sample read once
            return self.render_mix(start, n)
        return super().mix(bank, start, n)


class _AdaptNode(_Node):
    """Bank of SpatialPEs under SpatialAdapter(channels): one pgx_channel_adapt over the stacked K * n frames (frame by
    frame: the voice does not matter).  As many channels as the source has: the source's buffer, as the method returns it."""

    def __init__(self, pes, children):
        super().__init__(pes, children)
        self.out_ch = int(pes[0]._method.output_channels)

    def channels(self):
        return self.out_ch

    def render(self, start, n):
        x = self.children["source"].render(start, n)
        ch = x.shape[2]
        if ch == self.out_ch:
            return x
        out = DeviceBuffer((self.k, n, self.out_ch), np.float32)
        check(lib().pgx_channel_adapt(out.ptr, x.ptr, self.k * n, ch, self.out_ch), "pgx_channel_adapt")
        return out


# ------------------------------------------------------------------------------------ builder
def on_chip_mix_rule(pes) -> bool:
    """Host-only (no device, no bank): would a bank of these voices -- or of any subset of at least VOICE_TILES_MIN_VOICES of
    them -- mix its voices on chip (_BiquadNode.mixes_on_chip, block length permitting)?  ShardedMixPE asks this of ALL the
    inputs of a sharded mix on every rank: the conditions are per voice, so what holds for all holds for every rank's share."""
    if not (VOICE_TILES and WIDE_SUPERSAW and pes):
        return False
    chains = []
    for pe in pes:
        if isinstance(pe, GainPE):
            if not pe._gain_is_pe or pe._gain.channel_count() != 1:
                return False
            pe = pe._source
        if not isinstance(pe, BiquadPE) or pe._freq_is_pe or pe._q_is_pe:
            return False
        saw = pe._source
        if not isinstance(saw, BlitSawPE) or saw.inputs() or saw._channels != 1:
            return False
        chains.append((saw, pe))
    sr = float(pes[0].sample_rate)
    rec = _param_records(_dev.BLITSAW_PARAMS, [saw for saw, _ in chains], lambda saw: saw._scalar_params())
    if not (closed_form_ok(rec) and wide_oscillators_ok(rec, sr)):        # (what _BlitSawNode asks of its oscillators)
        return False
    for _, bq in chains:
        c = rbj_coefficients(bq._mode, bq._frequency, bq._q, bq._gain_db, sr)
        if not settle_frames(c[3], c[4]) or not 0 < settle_frames_fine(c[3], c[4]) <= VOICE_TILES_MAX_WARM:
            return False
    return True


class _Kind(NamedTuple):
    """How one PE class is batched.  A voice tree is batchable when every PE of it is, and two trees are batched
    together when their keys -- (tag, *extras, *children's keys) -- are equal."""
    pe_class: type
    tag: object                  # of the key: a string, or a function of the PE
    batchable: object            # (pe) -> bool
    extras: object               # (pe) -> what else goes into the key, or None
    children: tuple              # ((name the node knows the child by, attribute of the PE that holds it, present(pe)), ...)
    node: object                 # node(pes, children); node(pes) for a class without children
    min_voices: object = None    # (pe) -> voices below which a tree that holds this PE is not banked (None: MIN_VOICES)


_ALWAYS = lambda pe: True
_SOURCE = ("source", "_source", _ALWAYS)


def _osc_batchable(pe) -> bool:
    """Parameter PEs as (n, 1) streams only (what the kernel reads; the PE itself takes channel 0 of anything)."""
    return all(p.channel_count() == 1 for p in pe.inputs())


def _biquad_swept(pe) -> bool:
    """A BiquadPE whose cutoff or Q is a PE: per-sample coefficients (_BiquadVarNode)."""
    return bool(pe._freq_is_pe or pe._q_is_pe)


def _biquad_batchable(pe) -> bool:
    """Constant coefficients, or parameter PEs that are (n, 1) streams: the rule of _osc_batchable."""
    return all(p.channel_count() == 1 for p, is_pe in ((pe._frequency, pe._freq_is_pe), (pe._q, pe._q_is_pe)) if is_pe)


_PAN_METHODS = (SpatialLinear, SpatialConstantPower)


def _spatial_panned(pe) -> bool:
    return type(pe._method) in _PAN_METHODS


def _spatial_batchable(pe) -> bool:
    """SpatialAdapter; SpatialLinear / SpatialConstantPower with a scalar azimuth or an (n, 1) azimuth stream (the rule of
    _osc_batchable: the PE itself takes channel 0 of anything).  Not SpatialHRTF: it carries a convolution tail."""
    if type(pe._method) is SpatialAdapter:
        return True
    return _spatial_panned(pe) and (not _is_pe(pe._azimuth) or pe._azimuth.channel_count() == 1)


def _transform_codes(pe):
    """The op codes of a TransformPE's device program -- what two voices must share to be one launch (their
    parameters may differ: _TransformNode) --, or None: a host callable, a chain that follows temperament.py's
    globals (resolved when a block is rendered), a tuning step (pgx_tuning's program, not pgx_transform's)."""
    if pe._lowered is None or pe._follows_globals:
        return None
    try:
        codes = tuple(op[0] for op in pe._lowered.ops())
    except LookupError:
        return None
    return None if any(code in _tf.TUNING_CODES for code in codes) else codes


_KINDS = (
    # (all scalars: _SineNode, key ("sine", channels); a PE-driven frequency, amplitude or phase -- FM, AM, PM: _SineModNode --
    # the scalars of the other parameters are per-voice data there, which parameters are PEs is part of the key)
    _Kind(SinePE, lambda pe: "sine_mod" if pe._has_pe_inputs() else "sine", _osc_batchable,
          lambda pe: ((pe._channels, _is_pe(pe._frequency), _is_pe(pe._amplitude), _is_pe(pe._phase))
                      if pe._has_pe_inputs() else (pe._channels,)),
          (("frequency", "_frequency", lambda pe: _is_pe(pe._frequency)),
           ("amplitude", "_amplitude", lambda pe: _is_pe(pe._amplitude)),
           ("phase", "_phase", lambda pe: _is_pe(pe._phase))),
          lambda pes, children: _SineModNode(pes, children) if children else _SineNode(pes),
          lambda pe: SINE_MOD_MIN_VOICES if pe._has_pe_inputs() else MIN_VOICES),
    # (a FunctionGenPE with a PE parameter carries a phase and restarts on a seek: not batched -- PeriodicGate's rule)
    _Kind(FunctionGenPE, "function_gen", lambda pe: pe.is_pure(), lambda pe: (pe._waveform, pe._channels), (),
          _FunctionGenNode),
    # (one kernel per mode: part of the key; range and seed are per-voice data)
    _Kind(NoisePE, "noise", _ALWAYS, lambda pe: (pe._mode.value,), (), _NoiseNode, lambda pe: NOISE_MIN_VOICES),
    _Kind(BlitSawPE, "blitsaw", lambda pe: not pe.inputs(), lambda pe: (pe._channels,), (), _BlitSawNode),
    _Kind(SuperSawPE, "supersaw", lambda pe: not pe.inputs(), lambda pe: (pe._channels, len(pe._oscillators)), (),
          _SuperSawNode),
    # (which parameters are PEs is part of the key: a frequency child and a duty child may have the same key)
    _Kind(AnalogOscPE, "analog_osc", _osc_batchable,
          lambda pe: (pe._waveform, pe._channels, _is_pe(pe._frequency), _is_pe(pe._duty_cycle)),
          (("frequency", "_frequency", lambda pe: _is_pe(pe._frequency)),
           ("duty", "_duty_cycle", lambda pe: _is_pe(pe._duty_cycle))), _AnalogOscNode, lambda pe: ANALOG_OSC_MIN_VOICES),
    _Kind(TransformPE, "transform", lambda pe: _transform_codes(pe) is not None, lambda pe: (_transform_codes(pe),),
          (_SOURCE,), _TransformNode),
    # (constant coefficients: _BiquadNode; a PE-driven cutoff or Q: _BiquadVarNode -- mode, gain_db and the scalar of the
    # other parameter are per-voice data there, which parameters are PEs is part of the key)
    _Kind(BiquadPE, lambda pe: "biquad_var" if _biquad_swept(pe) else "biquad", _biquad_batchable,
          lambda pe: (pe._freq_is_pe, pe._q_is_pe) if _biquad_swept(pe) else (),
          (_SOURCE, ("frequency", "_frequency", lambda pe: pe._freq_is_pe), ("q", "_q", lambda pe: pe._q_is_pe)),
          lambda pes, children: (_BiquadVarNode if _biquad_swept(pes[0]) else _BiquadNode)(pes, children),
          lambda pe: BIQUAD_VAR_MIN_VOICES if _biquad_swept(pe) else MIN_VOICES),
    # (scalar frequency and Q only -- a PE-driven SVFilterPE stays per voice; mode, gain_db and the scalars are per-voice data)
    _Kind(SVFilterPE, "svf", lambda pe: not (pe._freq_is_pe or pe._q_is_pe), None, (_SOURCE,), _SvfNode,
          lambda pe: SVF_MIN_VOICES),
    _Kind(LadderPE, "ladder", lambda pe: not (pe._freq_is_pe or pe._res_is_pe or pe._drive_is_pe), None, (_SOURCE,),
          _LadderNode),
    _Kind(CombPE, "comb", lambda pe: not (pe._freq_is_pe or pe._fb_is_pe), None, (_SOURCE,), _CombNode),
    _Kind(PeriodicGate, "gate", lambda pe: pe.is_pure(), None, (), _GateNode),       # PE-driven gates carry a phase: not batched
    _Kind(AdsrGatedPE, "adsr_gated", _ALWAYS, None, (("gate", "_gate", _ALWAYS),), _AdsrGatedNode),
    _Kind(PeriodicTrigger, "trigger", _ALWAYS, None, (), _TriggerNode),
    _Kind(AdsrTriggeredPE, "adsr_trig", _ALWAYS, None, (("trigger", "_trigger", _ALWAYS),), _AdsrTriggeredNode,
          lambda pe: ADSR_TRIGGERED_MIN_VOICES),
    _Kind(GainPE, lambda pe: "gain_pe" if pe._gain_is_pe else "gain", _ALWAYS, None,
          (_SOURCE, ("gain", "_gain", lambda pe: pe._gain_is_pe)), _GainNode),
    # (the method object decides: panners by class and by whether the azimuth is a PE -- the scalar azimuths are per-voice
    # data --, the adapter by its channel count)
    _Kind(SpatialPE, lambda pe: "pan" if _spatial_panned(pe) else "adapt", _spatial_batchable,
          lambda pe: (type(pe._method).__name__, _is_pe(pe._azimuth)) if _spatial_panned(pe)
          else (pe._method.output_channels,),
          (_SOURCE, ("azimuth", "_azimuth", lambda pe: _spatial_panned(pe) and _is_pe(pe._azimuth))),
          lambda pes, children: (_PanNode if _spatial_panned(pes[0]) else _AdaptNode)(pes, children)),
)


def _kind(pe):
    for kind in _KINDS:
        if isinstance(pe, kind.pe_class):
            return kind
    return None


def _signature(pe):
    """Structural key of a voice tree, or None when the tree cannot be batched."""
    if pe.extent() != Extent(None, None):
        return None          # MixPE's extent-skip rule is per input; banks need always-on voices
    kind = _kind(pe)
    if kind is None or not kind.batchable(pe):
        return None
    key = (kind.tag(pe) if callable(kind.tag) else kind.tag,) + (kind.extras(pe) if kind.extras else ())
    for _, attribute, present in kind.children:
        if present(pe):
            sub = _signature(getattr(pe, attribute))
            if sub is None:
                return None
            key += (sub,)
    return key


def _min_voices(pe) -> int:
    """Voices from which trees like `pe` (batchable: _signature) are banked: the largest minimum of a class in the tree."""
    kind = _kind(pe)
    need = kind.min_voices(pe) if kind.min_voices is not None else MIN_VOICES
    for _, attribute, present in kind.children:
        if present(pe):
            need = max(need, _min_voices(getattr(pe, attribute)))
    return need


def _collect_ids(pe, seen):
    if id(pe) in seen:
        return False
    seen.add(id(pe))
    return all(_collect_ids(c, seen) for c in pe.inputs())


def _build(pes):
    kind = _kind(pes[0])
    if kind is None:
        raise TypeError(type(pes[0]).__name__)
    if not kind.children:
        return kind.node(pes)
    return kind.node(pes, {name: _build([getattr(p, attribute) for p in pes])
                           for name, attribute, present in kind.children if present(pes[0])})


class VoiceBank(_Windowed):
    def __init__(self, inputs):
        self.k = len(inputs)
        self.root = _build(list(inputs))
        if isinstance(self.root, _LadderNode):
            self.root.is_root = True
        for node in self._nodes():
            if isinstance(node, _NoiseNode):
                node.bank = weakref.ref(self)        # (NoisePE.advance settles an open window through it)
        self.mix_windows = False     # windows at the level of the mix whatever the root (set_mix_windows)
        self.request_dependent = any(node._REQUEST_DEPENDENT for node in self._nodes())     # (a pure sawtooth: no windows)
        self._reset_windows(BANK_WINDOW_FIRST)       # win.buf: the mixed window (Snippet), win.undo: [(node, snapshot)]
        self.streaming = False       # the block being rendered continues the one before it, same length

    def reset(self) -> None:
        self._reset_windows(BANK_WINDOW_FIRST)
        self.root.reset()

    def set_mix_windows(self) -> None:
        """A rank's share of a sharded mix (sharding.ShardedMixPE): the windows are made at the level of the MIX, so that
        a window is one collective.  A ladder root then leaves its own windows (rows of the ladders' outputs, mixed block
        by block) alone: 8 instances 39.9 -> 41.2 us per block without the collective, but one collective per 8 blocks."""
        self.mix_windows = True
        if isinstance(self.root, _LadderNode):
            self.root.is_root = False

    # ---- windows.  A small bank's block (a rank's share of a sharded mix: 64 voices) is a handful of launches whose
    # fixed parts -- launch, per-workgroup tables and carries, the first tile's anchor sines, the gaps between dependent
    # kernels -- are as long as the work itself.  A stream of equal blocks is therefore rendered 2, 4, 8 blocks at a
    # time and handed out block by block as rows of the mixed window (look_ahead.py does the same for PE graphs; a bank
    # keeps its states in its nodes, so the snapshot is taken there).  A pull that is not the next block puts every
    # node's state back to the window's start and renders the consumed part again, quietly.
    def _nodes(self):
        found, stack = [], [self.root]
        while stack:
            node = stack.pop()
            found.append(node)
            stack.extend(node.children.values())
        return found

    def _settle_window(self) -> None:
        left = self._close_window()
        if left is None:
            return
        first, served, snaps = left
        for node in self._nodes():
            node.quiesce()
        for node, snap in snaps:
            node.restore(snap)
        if served > first:
            self._render_mix_now(first, served - first)

    def render_mix(self, start: int, duration: int) -> Snippet:
        offset = self._next_row(start, duration)
        if offset is not None:
            row = Snippet.window_rows(start, self.win.buf.dev, offset, duration)
            row._bank_window = True
            return row
        closed = self.win          # (held to the end of this pull: its buffers return to the pool behind what is enqueued here)
        if closed is not None:
            self._settle_window()
        streaming = self.streaming = self._continues(start, duration)
        # (SuperSaw banks below the size that fills the chip: measured 44 -> 23 us per block for a rank's 64 instances,
        # 62 -> 42 for 128.  Not 256 and more -- rendered one block ahead already, a window ahead is too much thrown away
        # when the stream ends: 97 -> 155 us; not the C5 graph -- its envelope walk and mixes do not shrink with the
        # block, 56 -> 93 us for 64 voices.  A ladder root has windows of its own.)
        on_chip = VOICE_TILE_WINDOWS and self._mixes_on_chip(duration)
        if (BANK_WINDOWS and streaming and not self.request_dependent
                and (self.k <= BANK_WINDOW_MAX_VOICES or on_chip) and duration >= 4096
                and (isinstance(self.root, _SuperSawNode) and not self.root.fused() or BANK_WINDOWS_ANY_ROOT
                     or self.mix_windows or on_chip)
                and not lib().pgx_stream_is_forked()):
            # (a ladder root -- a rank's share of C4 -- takes the ladder bank's longer windows: its lanes' warm-up does
            # not shrink with the share, so the fewer instances a rank owns the more of a short window is warm-up)
            ladder_root = isinstance(self.root, _LadderNode)
            blocks = self._window_blocks(duration, LADDER_WINDOW_MAX if ladder_root else BANK_WINDOW_MAX,
                                         LADDER_WINDOW_FRAMES if ladder_root else BANK_WINDOW_FRAMES)
            if blocks > 1:
                nodes = self._nodes()
                for node in nodes:
                    node.quiesce(keep=(start, duration * blocks))
                snaps = [(node, node.snapshot()) for node in nodes if node._STATE]
                big = self._render_mix_now(start, duration * blocks)
                self._open_window(start, blocks, duration, big, snaps)
                row = Snippet.window_rows(start, big.dev, 0, duration)
                row._bank_window = True
                return row
        elif not streaming:
            self.grow = BANK_WINDOW_FIRST
        return self._render_mix_now(start, duration)

    def _mixes_on_chip(self, n: int) -> bool:
        """The voices of this bank are added on chip (pgx_voice_tiles) for blocks of n frames."""
        return self.root.mixes_on_chip(n)

    def _render_mix_now(self, start: int, duration: int) -> Snippet:
        return Snippet(start, self.root.mix(self, start, duration))


def try_build_bank(inputs):
    """VoiceBank for `inputs` if they are >= MIN_VOICES (_min_voices: some classes ask for more) identical, private,
    batchable trees."""
    if len(inputs) < MIN_VOICES:
        return None
    sig0 = _signature(inputs[0])
    if sig0 is None or len(inputs) < _min_voices(inputs[0]):
        return None
    seen = set()
    for pe in inputs:
        if _signature(pe) != sig0 or not _collect_ids(pe, seen):
            return None          # different structure, or a node shared between voices
    return VoiceBank(inputs)
