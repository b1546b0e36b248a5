"""
oracle/sources_oracle.py -- TEST INFRASTRUCTURE ONLY.

CPU restatement of KarplusStrongPE and AnalogOscPE (the reference's karplus_strong_pe.py / analog_osc_pe.py
arithmetic, written out), used by oracle/graph_eval.py and re-exported by tests/sources_oracle.py.

KarplusStrongPE: the reference's float32 loop.  AnalogOscPE: numpy float64 with u**4 as (u*u)*(u*u), which is the
rounding the reference's vectorised power gives for these arguments.
"""

from __future__ import annotations

import numpy as np


# ---------------------------------------------------------------------------------------------- KarplusStrongPE
def ks_geometry(sr, frequency):
    delay_float = sr / float(frequency)
    n = max(2, int(np.floor(delay_float)))
    frac = max(0.0, min(1.0, delay_float - n))
    return n, (1.0 - frac) / (1.0 + frac)


class KarplusStrong:
    """One string, streamed: render(start, duration) -> (duration, channels) float32, as KarplusStrongPE."""

    def __init__(self, sr, frequency, rho=0.996, duration=None, rho_damping=None, amplitude=0.3, seed=None,
                 channels=1):
        self.n, self.c = ks_geometry(sr, frequency)
        self.rho = float(rho)
        two = duration is not None and rho_damping is not None
        self.switch_at = duration if two else None
        self.rho_damping = float(rho_damping) if two else None
        self.amplitude, self.seed, self.channels = float(amplitude), seed, channels
        self.buf = None

    def excitation(self):
        rng = np.random.default_rng(self.seed)
        noise = rng.standard_normal(self.n).astype(np.float32)
        noise *= self.amplitude / (np.max(np.abs(noise)) + 1e-9)
        return noise

    def render(self, start, duration):
        data = np.zeros((duration, self.channels), dtype=np.float32)
        ks_start, ks_end = max(0, start), max(0, start + duration)
        need = ks_end - ks_start
        if need <= 0:
            return data
        if self.buf is None:
            self.buf = self.excitation().copy()
            self.r, self.ap_in, self.ap_out = 0, np.float32(0.0), np.float32(0.0)
        f32 = np.float32
        buf, r, ap_in, ap_out, n = self.buf, self.r, self.ap_in, self.ap_out, self.n
        c = f32(self.c)
        rho0 = f32(self.rho)
        rho1 = f32(self.rho_damping) if self.rho_damping is not None else rho0
        half = f32(0.5)
        out = np.empty(need, dtype=np.float32)
        for i in range(need):
            rho = rho1 if (self.switch_at is not None and ks_start + i >= self.switch_at) else rho0
            r1 = r + 1 if r + 1 < n else 0
            ov = (rho * (buf[r] + buf[r1])) * half
            ao = ((c * ov) + ap_in) - (c * ap_out)
            ap_in, ap_out = ov, ao
            buf[r] = ao
            out[i] = ao
            r = r1
        self.r, self.ap_in, self.ap_out = r, ap_in, ap_out
        off = ks_start - start
        data[off:off + need] = out[:, None]
        return data


# ---------------------------------------------------------------------------------------------- AnalogOscPE
def _blep(t, dt):
    y = np.zeros_like(t, dtype=np.float64)
    m = t < 2.0 * dt
    x = np.zeros_like(t)
    x[m] = t[m] / dt[m]
    u = 2.0 - x
    y[m] += (u[m] * u[m]) * (u[m] * u[m])
    m2 = t < dt
    v = 1.0 - x
    y[m2] -= 4.0 * ((v[m2] * v[m2]) * (v[m2] * v[m2]))
    return y / 12.0


def _residual(t, dt):
    t = np.mod(t, 1.0)
    return _blep(t, dt) - _blep(1.0 - t, dt)


def _piecewise(phase0, a):
    if phase0 < a:
        return -1.0 + 2.0 * (phase0 / a)
    return 1.0 - 2.0 * ((phase0 - a) / (1.0 - a))


class AnalogOsc:
    """render(start, freq, duty) with float64 per-frame parameter arrays (the PE's parameter streams, widened) ->
    float64 mono samples; `pure` selects the index-phase form.  `phases` keeps the last render's phases."""

    def __init__(self, sr, waveform, pure):
        self.sr, self.saw, self.pure = float(sr), waveform == "sawtooth", pure
        self.phase, self.saw_value, self.last_end = 0.0, -1.0, None

    def render(self, start, freq, duty):
        freq = np.asarray(freq, dtype=np.float64)
        duty = np.asarray(duty, dtype=np.float64)
        n = len(freq)
        dt = freq / self.sr
        dtb = np.clip(np.abs(dt), 1e-12, 0.5)
        edge = np.maximum(1e-5, 2.0 * dtb)
        duty = np.clip(duty, edge, 1.0 - edge)
        if self.pure:
            phase = np.mod(np.arange(start, start + n, dtype=np.float64) * float(dt[0]), 1.0)
        else:
            if self.last_end is None or start != self.last_end:
                self.phase, self.saw_value = 0.0, -1.0
            inc = np.concatenate(([0.0], np.cumsum(dt[:-1], dtype=np.float64)))
            phase = np.mod(self.phase + inc, 1.0)
            self.phase = float(np.mod(self.phase + float(np.sum(dt)), 1.0))
            self.last_end = start + n
        self.phases, self.duties = phase, duty
        if not self.saw:
            base = np.where(phase < duty, 1.0, -1.0)
            return base + _residual(phase, dtb) - _residual(phase - duty, dtb)
        a = 1.0 - duty
        u1, u2 = 2.0 / a, -2.0 / (1.0 - a)
        u = np.where(phase < a, u1, u2)
        delta = u2 - u1
        uc = u + (-0.5 * delta) * _residual(phase, dtb) + (0.5 * delta) * _residual(phase - a, dtb)
        dy = uc * dt
        y0 = _piecewise(float(phase[0]), float(a[0])) if self.pure else self.saw_value
        y = y0 + np.concatenate(([0.0], np.cumsum(dy[:-1], dtype=np.float64)))
        if not self.pure:
            self.saw_value = float(y0 + float(np.sum(dy)))
        return y

    def edge_distance(self):
        """Smallest distance of the last render's phases (but its first, which every form computes alike) from a
        discontinuity of the waveform: 0 / 1, the duty (rectangle) or a = 1 - duty (sawtooth)."""
        p, d = self.phases[1:], self.duties[1:]
        if len(p) == 0:
            return np.inf
        e = (1.0 - d) if self.saw else d
        return float(min(np.min(np.abs(p - e)), np.min(p), np.min(1.0 - p)))
