"""
The control plane of the SoundFont synthesizer: MIDI channels, voice allocation and the per-block state machine of a
voice (two envelopes, two LFOs, pitch, filter coefficients, gains), after the reference's meltysynth port
(meltysynth/synth/).  It never reads a sample.  `Synthesizer.advance(n_blocks)` runs it for n_blocks blocks and emits
the render table that pgx_soundfont_render (csrc/pgx_soundfont.hip) plays: one row per (block, audible voice), in block
order and within a block in the reference's mix order.

Every double is computed with Python's `math` functions in the reference's expression order, so under the same libm
the table is the reference's to the bit.

Columns of a row (include/pygmu_hip.h names the counts PGX_SOUNDFONT_ICOLS / PGX_SOUNDFONT_DCOLS):
  int32   I_VOICE       id of the voice object (0 .. polyphony - 1): it owns the filter state
          I_FLAGS       F_CLEAR: zero that state first (first block after a start); F_LOOP: looping oscillator;
                        F_FILTER: the low-pass is active
          I_END, I_START_LOOP, I_END_LOOP     sample frames
          I_MIX_L, I_MIX_R                    MIX_SKIP / MIX_CONST / MIX_SLOPE
          (one pad column)
  float64 D_POSITION, D_RATIO                 position at block start, pitch ratio
          D_A0 .. D_A0 + 4                    the normalised coefficients (0 when the filter is inactive)
          D_MIX_L, D_MIX_L + 1                MIX_CONST: gain, 0; MIX_SLOPE: gain at frame 0, step; MIX_SKIP: 0, 0
          D_MIX_R, D_MIX_R + 1                the same for the right side
"""

from __future__ import annotations

import math
import threading

import numpy as np

from . import sf2 as G

ICOLS, DCOLS = 8, 11
I_VOICE, I_FLAGS, I_END, I_START_LOOP, I_END_LOOP, I_MIX_L, I_MIX_R = range(7)
D_POSITION, D_RATIO, D_A0, D_MIX_L, D_MIX_R = 0, 1, 2, 7, 9
F_CLEAR, F_LOOP, F_FILTER = 1, 2, 4
MIX_SKIP, MIX_CONST, MIX_SLOPE = 0, 1, 2

NON_AUDIBLE = 1.0e-3
_LOG_NON_AUDIBLE = math.log(NON_AUDIBLE)
_HALF_PI = math.pi / 2
_PEAK_OFFSET = 1.0 - 1.0 / math.sqrt(2.0)
_PLAYING, _RELEASE_REQUESTED, _RELEASED = 0, 1, 2
_DELAY, _ATTACK, _HOLD, _DECAY, _RELEASE = range(5)


def _pow2_cents(x):                     # timecents -> seconds, cents -> factor
    return math.pow(2.0, (1.0 / 1200.0) * x)


def _hertz(x):
    return 8.176 * math.pow(2.0, (1.0 / 1200.0) * x)


def _linear(db):
    return math.pow(10.0, 0.05 * db)


def _key_factor(cents, key):
    return _pow2_cents(cents * (60 - key))


def _exp_cutoff(x):
    return 0.0 if x < _LOG_NON_AUDIBLE else math.exp(x)


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def mix_mode(previous_gain, current_gain, inverse_block_size):
    """What the reference's _write_block does with one side of one voice: (mode, a, b)."""
    if max(previous_gain, current_gain) < NON_AUDIBLE:
        return MIX_SKIP, 0.0, 0.0
    if abs(current_gain - previous_gain) < 1.0e-3:
        return MIX_CONST, float(current_gain), 0.0
    return MIX_SLOPE, float(previous_gain), inverse_block_size * (current_gain - previous_gain)


class Channel:
    """One MIDI channel: 14-bit controllers, RPN 0 / 1 / 2; the percussion channel lives on bank 128."""

    def __init__(self, is_percussion: bool):
        self.is_percussion_channel = is_percussion
        self.reset()

    def reset(self):
        self.bank_number = 128 if self.is_percussion_channel else 0
        self.patch_number = 0
        self._modulation = 0
        self._volume = 100 << 7
        self._pan = 64 << 7
        self._expression = 127 << 7
        self.hold_pedal = False
        self._reverb_send = 40
        self._chorus_send = 0
        self._rpn = -1
        self._pitch_bend_range = 2 << 7
        self._coarse_tune = 0
        self._fine_tune = 8192
        self._pitch_bend = 0

    def reset_all_controllers(self):
        self._modulation = 0
        self._expression = 127 << 7
        self.hold_pedal = False
        self._rpn = -1
        self._pitch_bend = 0

    def set_bank(self, value):
        self.bank_number = value + (128 if self.is_percussion_channel else 0)

    def set_patch(self, value):
        self.patch_number = value

    def _coarse(self, name, value):
        setattr(self, name, (getattr(self, name) & 0x7F) | (value << 7))

    def _fine(self, name, value):
        setattr(self, name, (getattr(self, name) & 0xFF80) | value)

    def set_hold_pedal(self, value):
        self.hold_pedal = value >= 64

    def data_entry_coarse(self, value):
        if self._rpn == 0:
            self._coarse("_pitch_bend_range", value)
        elif self._rpn == 1:
            self._coarse("_fine_tune", value)
        elif self._rpn == 2:
            self._coarse_tune = value - 64

    def data_entry_fine(self, value):
        if self._rpn == 0:
            self._fine("_pitch_bend_range", value)
        elif self._rpn == 1:
            self._fine("_fine_tune", value)

    def set_pitch_bend(self, value1, value2):
        self._pitch_bend = (1.0 / 8192.0) * ((value1 | (value2 << 7)) - 8192)

    @property
    def modulation(self):
        return (50.0 / 16383.0) * self._modulation

    @property
    def volume(self):
        return (1.0 / 16383.0) * self._volume

    @property
    def pan(self):
        return (100.0 / 16383.0) * self._pan - 50.0

    @property
    def expression(self):
        return (1.0 / 16383.0) * self._expression

    @property
    def reverb_send(self):
        return (1.0 / 127.0) * self._reverb_send

    @property
    def chorus_send(self):
        return (1.0 / 127.0) * self._chorus_send

    @property
    def pitch_bend_range(self):
        return (self._pitch_bend_range >> 7) + 0.01 * (self._pitch_bend_range & 0x7F)

    @property
    def tune(self):
        return self._coarse_tune + (1.0 / 8192.0) * (self._fine_tune - 8192)

    @property
    def pitch_bend(self):
        return self.pitch_bend_range * self._pitch_bend


class _Envelope:
    """Both envelopes share the stage walk; `volume` picks the exponential decay / release and the priority."""

    def __init__(self, sample_rate, volume: bool):
        self.sample_rate, self.volume = sample_rate, volume
        self.value = 0
        self.priority = 0

    def start(self, delay, attack, hold, decay, sustain, release):
        self.attack_slope = 1 / attack
        if self.volume:
            self.decay_slope = -9.226 / decay
            self.release_slope = -9.226 / release
        else:
            self.decay_slope = 1 / decay
            self.release_slope = 1 / release
        self.attack_start = delay
        self.hold_start = self.attack_start + attack
        self.decay_start = self.hold_start + hold
        if self.volume:
            self.release_start = 0
        else:
            self.decay_end = self.decay_start + decay
            self.release_end = release
        self.sustain_level = _clamp(sustain, 0, 1)
        self.release_level = 0
        self.count = 0
        self.stage = _DELAY
        self.value = 0
        self.process(0)

    def release(self):
        self.stage = _RELEASE
        now = float(self.count) / self.sample_rate
        if self.volume:
            self.release_start = now
        else:
            self.release_end += now
        self.release_level = self.value

    def process(self, sample_count) -> bool:
        self.count += sample_count
        now = float(self.count) / self.sample_rate
        while self.stage <= _HOLD:
            end = (self.attack_start, self.hold_start, self.decay_start)[self.stage]
            if now < end:
                break
            self.stage += 1
        stage = self.stage
        if stage == _DELAY:
            self.value = 0
            self.priority = 4 + self.value
            return True
        if stage == _ATTACK:
            self.value = self.attack_slope * (now - self.attack_start)
            self.priority = 3 + self.value
            return True
        if stage == _HOLD:
            self.value = 1
            self.priority = 2 + self.value
            return True
        if self.volume:
            if stage == _DECAY:
                self.value = max(_exp_cutoff(self.decay_slope * (now - self.decay_start)), self.sustain_level)
                self.priority = 1 + self.value
            else:
                self.value = self.release_level * _exp_cutoff(self.release_slope * (now - self.release_start))
                self.priority = self.value
        elif stage == _DECAY:
            self.value = max(self.decay_slope * (self.decay_end - now), self.sustain_level)
        else:
            self.value = max(self.release_level * self.release_slope * (self.release_end - now), 0)
        return self.value > NON_AUDIBLE


class _Lfo:
    def __init__(self, sample_rate, block_size):
        self.sample_rate, self.block_size = sample_rate, block_size
        self.active, self.value = False, 0

    def start(self, delay, frequency):
        self.value = 0
        self.active = frequency > 1.0e-3
        if self.active:
            self.delay = delay
            self.period = 1.0 / frequency
            self.count = 0

    def process(self):
        if not self.active:
            return
        self.count += self.block_size
        now = float(self.count) / self.sample_rate
        if now < self.delay:
            self.value = 0
            return
        phase = ((now - self.delay) % self.period) / self.period
        if phase < 0.25:
            self.value = 4 * phase
        elif phase < 0.75:
            self.value = 4 * (0.5 - phase)
        else:
            self.value = 4 * (phase - 1.0)


class Voice:
    def __init__(self, synth: "Synthesizer", index: int):
        self.synth, self.id = synth, index
        sr, bs = synth.sample_rate, synth.block_size
        self.vol_env, self.mod_env = _Envelope(sr, True), _Envelope(sr, False)
        self.vib_lfo, self.mod_lfo = _Lfo(sr, bs), _Lfo(sr, bs)
        self.previous_left = self.previous_right = self.current_left = self.current_right = 0
        self.note_gain = 0
        self.exclusive_class = self.channel = self.key = self.velocity = 0
        self.voice_length = 0
        self.filter_active = False
        self.coefficients = (0.0,) * 5
        self.row = None

    # ------------------------------------------------------------------ note start
    def start(self, preset_region, instrument_region, channel, key, velocity):
        pg, ig, sample = preset_region.gs, instrument_region.gs, instrument_region.sample

        def g(kind):
            return pg[kind] + ig[kind]

        sr = self.synth.sample_rate
        self.exclusive_class = ig[G.G_EXCLUSIVE_CLASS]
        self.channel, self.key, self.velocity = channel, key, velocity
        if velocity > 0:
            sample_attenuation = 0.4 * (0.1 * g(G.G_ATTENUATION))
            filter_attenuation = 0.5 * (0.1 * g(G.G_Q))
            decibels = 2 * (20.0 * math.log10(velocity / 127.0)) - sample_attenuation - filter_attenuation
            self.note_gain = _linear(decibels)
        else:
            self.note_gain = 0
        self.cutoff = _hertz(g(G.G_CUTOFF))
        self.resonance = _linear(0.1 * g(G.G_Q))
        self.vib_lfo_to_pitch = 0.01 * g(G.G_VIBLFO_PITCH)
        self.mod_lfo_to_pitch = 0.01 * g(G.G_MODLFO_PITCH)
        self.mod_env_to_pitch = 0.01 * g(G.G_MODENV_PITCH)
        self.mod_lfo_to_cutoff = g(G.G_MODLFO_CUTOFF)
        self.mod_env_to_cutoff = g(G.G_MODENV_CUTOFF)
        self.dynamic_cutoff = self.mod_lfo_to_cutoff != 0 or self.mod_env_to_cutoff != 0
        self.mod_lfo_to_volume = 0.1 * g(G.G_MODLFO_VOLUME)
        self.dynamic_volume = self.mod_lfo_to_volume > 0.05
        self.instrument_pan = _clamp(0.1 * g(G.G_PAN), -50, 50)

        self.vol_env.start(
            _pow2_cents(g(G.G_VOLENV_DELAY)), _pow2_cents(g(G.G_VOLENV_ATTACK)),
            _pow2_cents(g(G.G_VOLENV_HOLD)) * _key_factor(g(G.G_VOLENV_KEY_HOLD), key),
            _pow2_cents(g(G.G_VOLENV_DECAY)) * _key_factor(g(G.G_VOLENV_KEY_DECAY), key),
            _linear(-(0.1 * g(G.G_VOLENV_SUSTAIN))), max(_pow2_cents(g(G.G_VOLENV_RELEASE)), 0.01))
        self.mod_env.start(
            _pow2_cents(g(G.G_MODENV_DELAY)), _pow2_cents(g(G.G_MODENV_ATTACK)) * ((145 - velocity) / 144.0),
            _pow2_cents(g(G.G_MODENV_HOLD)) * _key_factor(g(G.G_MODENV_KEY_HOLD), key),
            _pow2_cents(g(G.G_MODENV_DECAY)) * _key_factor(g(G.G_MODENV_KEY_DECAY), key),
            1.0 - (0.1 * g(G.G_MODENV_SUSTAIN)) / 100.0, _pow2_cents(g(G.G_MODENV_RELEASE)))
        self.vib_lfo.start(_pow2_cents(g(G.G_VIBLFO_DELAY)), _hertz(g(G.G_VIBLFO_FREQ)))
        self.mod_lfo.start(_pow2_cents(g(G.G_MODLFO_DELAY)), _hertz(g(G.G_MODLFO_FREQ)))

        # oscillator: the addresses, the loop mode and the root key are the instrument's alone
        modes = ig[G.G_SAMPLE_MODES]
        if modes not in (0, 1, 2, 3):
            raise ValueError(f"{modes} is not a valid LoopMode")
        self.loop_mode = 0 if modes == 2 else modes
        self.looping = self.loop_mode != 0
        self.end = sample.end + 32768 * ig[G.G_END_COARSE] + ig[G.G_END_OFS]
        self.start_loop = sample.start_loop + 32768 * ig[G.G_STARTLOOP_COARSE] + ig[G.G_STARTLOOP_OFS]
        self.end_loop = sample.end_loop + 32768 * ig[G.G_ENDLOOP_COARSE] + ig[G.G_ENDLOOP_OFS]
        self.root_key = ig[G.G_ROOT_KEY] if ig[G.G_ROOT_KEY] != -1 else sample.original_pitch
        self.tune = g(G.G_COARSE_TUNE) + 0.01 * (g(G.G_FINE_TUNE) + sample.pitch_correction)
        self.pitch_change_scale = 0.01 * g(G.G_SCALE_TUNING)
        self.sample_rate_ratio = sample.sample_rate / sr
        self.position = sample.start + 32768 * ig[G.G_START_COARSE] + ig[G.G_START_OFS]

        self.clear_filter = True
        self._set_low_pass(self.cutoff, self.resonance)
        self.smoothed_cutoff = self.cutoff
        self.state = _PLAYING
        self.voice_length = 0

    def _set_low_pass(self, cutoff, resonance):
        sr = self.synth.sample_rate
        self.filter_active = cutoff < 0.499 * sr
        if not self.filter_active:
            return
        q = resonance - _PEAK_OFFSET / (1 + 6 * (resonance - 1))
        w = 2 * math.pi * cutoff / sr
        cosw = math.cos(w)
        alpha = math.sin(w) / (2 * q)
        b0 = (1 - cosw) / 2
        b1 = 1 - cosw
        b2 = (1 - cosw) / 2
        a0 = 1 + alpha
        a1 = -2 * cosw
        a2 = 1 - alpha
        self.coefficients = (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)

    def end_note(self):
        if self.state == _PLAYING:
            self.state = _RELEASE_REQUESTED

    def kill(self):
        self.note_gain = 0

    @property
    def priority(self):
        return 0 if self.note_gain < NON_AUDIBLE else self.vol_env.priority

    # ------------------------------------------------------------------ one block
    def _oscillate(self, pitch) -> bool:
        """Pitch ratio and position update of the reference's numpy fill paths; False when a no-loop sample has run out."""
        n = self.synth.block_size
        pitch_change = self.pitch_change_scale * (pitch - self.root_key) + self.tune
        ratio = self.sample_rate_ratio * math.pow(2.0, pitch_change / 12.0)
        position = self.position
        last = position + float(n - 1) * ratio
        if self.looping:
            new = last + ratio
            if new >= float(self.end_loop):
                new -= float(self.end_loop - self.start_loop)
        else:
            if last < self.end:
                new = last + ratio
            else:
                positions = position + np.arange(n, dtype=np.float64) * ratio
                past = int(np.searchsorted(positions, self.end))
                if past == 0:
                    return False
                new = float(positions[past - 1]) + ratio
        self.block_position, self.block_ratio, self.block_looping = float(position), ratio, self.looping
        self.position = new
        return True

    def process(self) -> bool:
        if self.note_gain < NON_AUDIBLE:
            return False
        synth = self.synth
        ch = synth.channels[self.channel]
        if (self.voice_length >= synth.minimum_voice_duration and self.state == _RELEASE_REQUESTED
                and not ch.hold_pedal):
            self.vol_env.release()
            self.mod_env.release()
            if self.loop_mode == 3:
                self.looping = False
            self.state = _RELEASED
        if not self.vol_env.process(synth.block_size):
            return False
        self.mod_env.process(synth.block_size)
        self.vib_lfo.process()
        self.mod_lfo.process()

        vib_pitch_change = (0.01 * ch.modulation + self.vib_lfo_to_pitch) * self.vib_lfo.value
        mod_pitch_change = self.mod_lfo_to_pitch * self.mod_lfo.value + self.mod_env_to_pitch * self.mod_env.value
        channel_pitch_change = ch.tune + ch.pitch_bend
        pitch = self.key + vib_pitch_change + mod_pitch_change + channel_pitch_change
        if not self._oscillate(pitch):
            return False

        if self.dynamic_cutoff:
            cents = self.mod_lfo_to_cutoff * self.mod_lfo.value + self.mod_env_to_cutoff * self.mod_env.value
            new_cutoff = _pow2_cents(cents) * self.cutoff
            lower, upper = 0.5 * self.smoothed_cutoff, 2.0 * self.smoothed_cutoff
            self.smoothed_cutoff = lower if new_cutoff < lower else upper if new_cutoff > upper else new_cutoff
            self._set_low_pass(self.smoothed_cutoff, self.resonance)

        self.previous_left, self.previous_right = self.current_left, self.current_right
        ve = ch.volume * ch.expression
        channel_gain = ve * ve
        mix_gain = self.note_gain * channel_gain * self.vol_env.value
        if self.dynamic_volume:
            mix_gain *= _linear(self.mod_lfo_to_volume * self.mod_lfo.value)
        angle = (math.pi / 200.0) * (ch.pan + self.instrument_pan + 50.0)
        if angle <= 0:
            self.current_left, self.current_right = mix_gain, 0
        elif angle >= _HALF_PI:
            self.current_left, self.current_right = 0, mix_gain
        else:
            self.current_left, self.current_right = mix_gain * math.cos(angle), mix_gain * math.sin(angle)
        if self.voice_length == 0:
            self.previous_left, self.previous_right = self.current_left, self.current_right
        self.voice_length += synth.block_size
        return True

    def emit(self, irows, drows):
        synth = self.synth
        flags = (F_CLEAR if self.clear_filter else 0) | (F_LOOP if self.block_looping else 0) \
            | (F_FILTER if self.filter_active else 0)
        self.clear_filter = False
        mv, inv = synth.master_volume, synth.inverse_block_size
        ml, la, lb = mix_mode(mv * self.previous_left, mv * self.current_left, inv)
        mr, ra, rb = mix_mode(mv * self.previous_right, mv * self.current_right, inv)
        irows.append((self.id, flags, self.end, self.start_loop, self.end_loop, ml, mr, 0))
        coefficients = self.coefficients if self.filter_active else (0.0,) * 5
        drows.append((self.block_position, self.block_ratio) + coefficients + (la, lb, ra, rb))


class Synthesizer:
    """What `MeltysynthPE.synthesizer` returns: the reference Synthesizer's event interface.  A lock guards the event
    methods and advance(): events arrive from a MIDI thread."""

    CHANNEL_COUNT = 16
    PERCUSSION_CHANNEL = 9

    def __init__(self, sound_font, sample_rate: int, block_size: int = 64, maximum_polyphony: int = 64):
        if not 16000 <= sample_rate <= 192000:
            raise ValueError("The sample rate must be between 16000 and 192000.")
        if not 8 <= block_size <= 1024:
            raise ValueError("The block size must be between 8 and 1024.")
        if not 8 <= maximum_polyphony <= 256:
            raise ValueError("The maximum number of polyphony must be between 8 and 256.")
        self._lock = threading.RLock()
        self._sound_font = sound_font
        self._sample_rate, self._block_size, self._maximum_polyphony = sample_rate, block_size, maximum_polyphony
        self.minimum_voice_duration = sample_rate // 500
        self.inverse_block_size = 1.0 / block_size
        self.master_volume = 0.5
        self._preset_lookup = {}
        lowest = None
        for preset in sound_font.presets:
            preset_id = (preset.bank_number << 16) | preset.patch_number
            self._preset_lookup[preset_id] = preset
            if lowest is None or preset_id < lowest:
                self._default_preset, lowest = preset, preset_id
        self.channels = [Channel(i == self.PERCUSSION_CHANNEL) for i in range(self.CHANNEL_COUNT)]
        self.voices = [Voice(self, i) for i in range(maximum_polyphony)]
        self._active = 0

    # ------------------------------------------------------------------ properties
    block_size = property(lambda self: self._block_size)
    maximum_polyphony = property(lambda self: self._maximum_polyphony)
    channel_count = property(lambda self: self.CHANNEL_COUNT)
    percussion_channel = property(lambda self: self.PERCUSSION_CHANNEL)
    sample_rate = property(lambda self: self._sample_rate)
    sound_font = property(lambda self: self._sound_font)
    active_voice_count = property(lambda self: self._active)

    # ------------------------------------------------------------------ events
    def process_midi_message(self, channel: int, command: int, data1: int, data2: int) -> None:
        with self._lock:
            if not 0 <= channel < len(self.channels):
                return
            ch = self.channels[channel]
            if command == 0x80:
                self.note_off(channel, data1)
            elif command == 0x90:
                self.note_on(channel, data1, data2)
            elif command == 0xC0:
                ch.set_patch(data1)
            elif command == 0xE0:
                ch.set_pitch_bend(data1, data2)
            elif command == 0xB0:
                pairs = {0x01: "_modulation", 0x07: "_volume", 0x0A: "_pan", 0x0B: "_expression", 0x65: "_rpn"}
                fine = {0x21: "_modulation", 0x27: "_volume", 0x2A: "_pan", 0x2B: "_expression", 0x64: "_rpn"}
                if data1 in pairs:
                    ch._coarse(pairs[data1], data2)
                elif data1 in fine:
                    ch._fine(fine[data1], data2)
                elif data1 == 0x00:
                    ch.set_bank(data2)
                elif data1 == 0x06:
                    ch.data_entry_coarse(data2)
                elif data1 == 0x26:
                    ch.data_entry_fine(data2)
                elif data1 == 0x40:
                    ch.set_hold_pedal(data2)
                elif data1 == 0x5B:
                    ch._reverb_send = data2
                elif data1 == 0x5D:
                    ch._chorus_send = data2
                elif data1 == 0x78:
                    self.note_off_all_channel(channel, True)
                elif data1 == 0x79:
                    self.reset_all_controllers_channel(channel)
                elif data1 == 0x7B:
                    self.note_off_all_channel(channel, False)

    def note_off(self, channel: int, key: int) -> None:
        with self._lock:
            if not 0 <= channel < len(self.channels):
                return
            for voice in self.voices[:self._active]:
                if voice.channel == channel and voice.key == key:
                    voice.end_note()

    def note_on(self, channel: int, key: int, velocity: int) -> None:
        with self._lock:
            if velocity == 0:
                self.note_off(channel, key)
                return
            if not 0 <= channel < len(self.channels):
                return
            ch = self.channels[channel]
            preset = self._preset_lookup.get((ch.bank_number << 16) | ch.patch_number)
            if preset is None:
                gm = ch.patch_number if ch.bank_number < 128 else (128 << 16)
                preset = self._preset_lookup.get(gm, self._default_preset)
            for preset_region in preset.regions:
                if preset_region.contains(key, velocity):
                    for instrument_region in preset_region.instrument.regions:
                        if instrument_region.contains(key, velocity):
                            voice = self._request_voice(instrument_region.gs[G.G_EXCLUSIVE_CLASS], channel)
                            voice.start(preset_region, instrument_region, channel, key, velocity)

    def _request_voice(self, exclusive_class: int, channel: int) -> Voice:
        active = self.voices[:self._active]
        if exclusive_class != 0:
            for voice in active:
                if voice.exclusive_class == exclusive_class and voice.channel == channel:
                    return voice
        if self._active < len(self.voices):
            self._active += 1
            return self.voices[self._active - 1]
        candidate, lowest = self.voices[0], 1000000.0
        for voice in active:
            priority = voice.priority
            if priority < lowest:
                lowest, candidate = priority, voice
            elif priority == lowest and voice.voice_length > candidate.voice_length:
                candidate = voice
        return candidate

    def note_off_all(self, immediate: bool) -> None:
        with self._lock:
            if immediate:
                self._active = 0
            else:
                for voice in self.voices[:self._active]:
                    voice.end_note()

    def note_off_all_channel(self, channel: int, immediate: bool) -> None:
        with self._lock:
            for voice in self.voices[:self._active]:
                if voice.channel == channel:
                    voice.kill() if immediate else voice.end_note()

    def reset_all_controllers(self) -> None:
        with self._lock:
            for ch in self.channels:
                ch.reset_all_controllers()

    def reset_all_controllers_channel(self, channel: int) -> None:
        with self._lock:
            if 0 <= channel < len(self.channels):
                self.channels[channel].reset_all_controllers()

    def reset(self) -> None:
        with self._lock:
            self._active = 0
            for ch in self.channels:
                ch.reset()
            self.pending_reset = True

    pending_reset = False          # reset() drops what is left of the block being served

    def take_reset(self) -> bool:
        """Has reset() been called since the last call of this?  (MeltysynthPE then drops its carry.)"""
        with self._lock:
            flag, self.pending_reset = self.pending_reset, False
            return flag

    # ------------------------------------------------------------------ the render table
    def advance(self, n_blocks: int):
        """Run the state machine for n_blocks blocks: (block_rows int32[n_blocks + 1], int32[rows, ICOLS],
        float64[rows, DCOLS]); the rows of block b are block_rows[b] .. block_rows[b + 1]."""
        with self._lock:
            voices = self.voices
            offsets, irows, drows = [0], [], []
            for _ in range(int(n_blocks)):
                i = 0
                while i != self._active:
                    if voices[i].process():
                        i += 1
                    else:                      # swap the finished voice with the last active one
                        self._active -= 1
                        voices[i], voices[self._active] = voices[self._active], voices[i]
                for voice in voices[:self._active]:
                    voice.emit(irows, drows)
                offsets.append(len(irows))
        return (np.asarray(offsets, dtype=np.int32), np.asarray(irows, dtype=np.int32).reshape(-1, ICOLS),
                np.asarray(drows, dtype=np.float64).reshape(-1, DCOLS))
