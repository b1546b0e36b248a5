"""GPU: pgx_sine_stateful_bank -- pgx_sine_stateful with the voice in the grid -- against pgx_sine_stateful itself, bit for
bit in samples and in the final {phase, initialised}, on both plans: the walk (no workspace: a workgroup per voice) and the
time-parallel form (a workspace: a workgroup per tile of 2 048 frames and voice, two launches; blocks of one or two tiles
are walked either way).  Block lengths: one frame, part of a tile, a tile less one / exactly / plus one, two tiles exactly
and plus one (the first length that takes the two launches), three tiles and a ragged fourth.  1, 5 and 33 voices, 1, 2 and
3 channels, a frequency stream, an amplitude stream, a phase stream, all three.  Half the voices enter with a carried
phase, half with a zeroed state (the first-render rule: the scalar phase is where a voice starts when the phase is no
stream).  Rows longer than their data keep the NaN pattern the gaps were filled with; every device buffer lies between
guard bands (tests/guarded_alloc.py).  Then two contiguous calls and one after the state was zeroed, and the argument
checks."""

import functools

import numpy as np
import pytest

from fixture_harness import assert_bits
from guarded_alloc import guarded
from pygmu2_amd import device
from pygmu2_amd._kernels import DeviceBuffer, lib

pytestmark = pytest.mark.gpu

SR = 48000.0
PGX_OK, PGX_ERR_INVALID = 0, -1
LENGTHS = (1, 7, 2047, 2048, 2049, 4096, 4097, 6149)
BATCHES = (1, 5, 33)
FORMS = {"freq": (True, False, False), "amp": (False, True, False), "phase": (False, False, True),
         "all": (True, True, True)}
PADS = (5, 3, 7, 2)            # elements past the data of a row: out, freq, amp, phase


def _pattern(count, first=0):
    """float32 NaNs, no two alike (the guard bands' words)."""
    words = (np.arange(count, dtype=np.uint32) + np.uint32(first)) & np.uint32(0xFFFFF)
    return (np.uint32(0xFFF00000) | words).view(np.float32)


def _same64(name, got, want):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{name}: {got} != {want}"


def _voices(batch, n, form, seed):
    """Per voice: a frequency stream a few hundred Hz around its carrier, an amplitude stream in 0.1 .. 0.5, a phase
    stream of +-1.5 rad (those the form uses, else None), the record SinePE._render fills, and the state on entry."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    use_f, use_a, use_p = FORMS[form]
    carrier = np.array([200.0 + 37.0 * v for v in range(batch)])
    freq = np.stack([carrier[v] + (150.0 + 20.0 * (v % 7)) * np.sin(0.01 * (v + 1) * t + v) + rng.uniform(-5, 5, n)
                     for v in range(batch)]).astype(np.float32) if use_f else None
    amp = np.stack([0.3 + 0.2 * np.cos(0.003 * (v + 2) * t) for v in range(batch)]).astype(np.float32) if use_a else None
    phase = np.stack([1.5 * np.sin(0.002 * (v + 3) * t + 0.5 * v) for v in range(batch)]).astype(np.float32) if use_p else None
    rec = np.zeros(batch, dtype=device.SINE_STATEFUL_PARAMS)
    for v in range(batch):
        rec[v]["freq"] = 0.0 if use_f else carrier[v]
        rec[v]["amp"] = 0.0 if use_a else 0.1 + 0.02 * v
        rec[v]["phase"] = 0.0 if use_p else 0.1 * v - 0.7
        rec[v]["phase_is_stream"] = int(use_p)
    state = np.zeros((batch, 2), dtype=np.float64)
    state[1::2, 0] = rng.uniform(-3.0, 40.0, len(state[1::2]))          # odd voices carry a phase, even ones start fresh
    state[1::2, 1] = 1.0
    return freq, amp, phase, rec, state


def _singles(n, channels, freq, amp, phase, rec, state):
    """pgx_sine_stateful voice by voice over copies of the inputs -> (samples [batch][n][channels], final states)."""
    L = lib()
    batch = len(rec)
    out = DeviceBuffer((batch, n, channels), np.float32)
    f, a, p = (DeviceBuffer.from_host(x) if x is not None else None for x in (freq, amp, phase))
    params, st = device.upload_structs(rec), DeviceBuffer.from_host(state)
    for v in range(batch):
        rc = L.pgx_sine_stateful(out.offset_ptr(v * n * channels), n, channels, SR, params.offset_ptr(v),
                                 f.offset_ptr(v * n) if f else None, a.offset_ptr(v * n) if a else None,
                                 p.offset_ptr(v * n) if p else None, st.offset_ptr(2 * v))
        assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host(), st.to_host()


def _padded(rows, pad, first):
    """[batch][n + pad] float32: the rows' data, then the NaN pattern up to the stride; None of None."""
    if rows is None:
        return None
    batch, width = rows.shape
    buf = _pattern(batch * (width + pad), first).reshape(batch, width + pad).copy()
    buf[:, :width] = rows
    return buf


def _bank(n, channels, freq, amp, phase, rec, state, use_ws, pads=(0, 0, 0, 0)):
    """pgx_sine_stateful_bank over the voices, rows `pads` elements longer than their data
    -> (the whole padded output [batch][out_stride], final states)."""
    L = lib()
    batch = len(rec)
    out_stride = n * channels + pads[0]
    filled = _pattern(batch * out_stride, 77).reshape(batch, out_stride)
    out = DeviceBuffer.from_host(filled)
    f, a, p = (DeviceBuffer.from_host(_padded(x, pad, 11 * (i + 1))) if x is not None else None
               for i, (x, pad) in enumerate(zip((freq, amp, phase), pads[1:])))
    params, st = device.upload_structs(rec), DeviceBuffer.from_host(state)
    need = L.pgx_sine_stateful_bank_workspace_bytes(n, batch) if use_ws else 0
    ws = DeviceBuffer((need,), np.uint8) if need else None
    rc = L.pgx_sine_stateful_bank(out.ptr, out_stride, batch, n, channels, SR, params.ptr,
                                  f.ptr if f else None, n + pads[1], a.ptr if a else None, n + pads[2],
                                  p.ptr if p else None, n + pads[3], st.ptr, ws.ptr if ws else None)
    assert rc == PGX_OK, L.pgx_last_error()
    got = out.to_host()
    width = n * channels
    assert np.array_equal(got[:, width:].view(np.uint32), filled[:, width:].view(np.uint32)), "the gaps between the rows"
    return got[:, :width].reshape(batch, n, channels), st.to_host()


@functools.lru_cache(None)
def _reference(form, channels, n):
    """The inputs of the largest batch and what pgx_sine_stateful makes of them, once; the smaller batches are its first
    voices.  Nobody changes it."""
    inputs = _voices(max(BATCHES), n, form, seed=1000 * channels + n)
    want, want_state = _singles(n, channels, *inputs)
    assert np.all(np.isfinite(want)) and np.any(want) and np.all(want_state[:, 1] == 1.0)
    for x in (*inputs, want, want_state):
        if x is not None:
            x.setflags(write=False)
    return inputs, want, want_state


def _first(x, batch):
    return None if x is None else x[:batch].copy()


# ------------------------------------------------------------------------------------------ 1. both plans, every shape
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_bank_equals_the_single_entry(form, channels):
    with guarded():
        for n in LENGTHS:
            (freq, amp, phase, rec, state), want, want_state = _reference(form, channels, n)
            for batch in BATCHES:
                for use_ws in (False, True):
                    for pads in ((0, 0, 0, 0), PADS):
                        what = f"{form} ch={channels} n={n} batch={batch} workspace={use_ws} pads={pads}"
                        got, got_state = _bank(n, channels, _first(freq, batch), _first(amp, batch), _first(phase, batch),
                                               rec[:batch].copy(), state[:batch].copy(), use_ws, pads)
                        assert_bits(what, got, want[:batch])
                        _same64(what, got_state, want_state[:batch])


# ------------------------------------------------------------------------------------------ 2. carried and zeroed state
@pytest.mark.parametrize("use_ws", [False, True], ids=["walk", "time-parallel"])
@pytest.mark.parametrize("form", ["freq", "all"])
def test_contiguous_calls_and_a_call_after_the_state_is_zeroed(form, use_ws):
    batch, channels = 5, 2
    with guarded():
        state = want_state = np.zeros((batch, 2), dtype=np.float64)
        for call, n in enumerate((6149, 4097, 2049)):
            freq, amp, phase, rec, _ = _voices(batch, n, form, seed=31 + call)
            if call == 2:                                            # SinePE._clear_phase: the voices start over
                state = want_state = np.zeros((batch, 2), dtype=np.float64)
            before = state.copy()
            want, want_state = _singles(n, channels, freq, amp, phase, rec, want_state)
            got, state = _bank(n, channels, freq, amp, phase, rec, state, use_ws, PADS)
            what = f"{form} call {call} workspace={use_ws}"
            assert np.all(np.isfinite(want)) and np.any(want), what
            assert_bits(what, got, want)
            _same64(what, state, want_state)
            assert np.all(state[:, 1] == 1.0) and not np.any(state[:, 0] == before[:, 0]), what
            if call in (0, 2) and form == "freq":
                # the first-render rule: the scalar phase is the initial phase AND the per-sample term -- frame 0 is
                # amp * sin((inc0 + phase) + phase)
                inc0 = (2.0 * np.pi * freq[:, 0].astype(np.float64)) / SR
                first = rec["amp"] * np.sin((inc0 + rec["phase"]) + rec["phase"])
                assert np.allclose(got[:, 0, 0], first, rtol=0, atol=1e-6), what


# ------------------------------------------------------------------------------------------ 3. the argument checks
def test_nothing_to_do_and_bad_arguments():
    L = lib()
    n, channels, batch = 4097, 2, 3
    freq, amp, phase, rec, state = _voices(batch, n, "all", seed=5)
    width = n * channels
    with guarded():
        filled = _pattern(batch * width, 77).reshape(batch, width)
        out = DeviceBuffer.from_host(filled)
        f, a, p = DeviceBuffer.from_host(freq), DeviceBuffer.from_host(amp), DeviceBuffer.from_host(phase)
        params, st = device.upload_structs(rec), DeviceBuffer.from_host(state)
        ws = DeviceBuffer((L.pgx_sine_stateful_bank_workspace_bytes(n, batch),), np.uint8)
        here = dict(out_ptr=out.ptr, out_stride=width, batch=batch, n=n, channels=channels, sr=SR, params_ptr=params.ptr,
                    f_ptr=f.ptr, f_stride=n, a_ptr=a.ptr, a_stride=n, p_ptr=p.ptr, p_stride=n, state_ptr=st.ptr, ws_ptr=ws.ptr)

        def call(**changed):
            x = dict(here, **changed)
            return L.pgx_sine_stateful_bank(x["out_ptr"], x["out_stride"], x["batch"], x["n"], x["channels"], x["sr"],
                                            x["params_ptr"], x["f_ptr"], x["f_stride"], x["a_ptr"], x["a_stride"], x["p_ptr"],
                                            x["p_stride"], x["state_ptr"], x["ws_ptr"])

        def untouched(why):
            assert np.array_equal(out.to_host().view(np.uint32), filled.view(np.uint32)), why    # nothing was launched
            assert np.array_equal(st.to_host(), state), why

        for nothing in (dict(n=0), dict(batch=0), dict(n=-4), dict(batch=-1)):
            assert call(**nothing) == PGX_OK, nothing
            untouched(nothing)
        refused = [dict(out_ptr=None), dict(params_ptr=None), dict(state_ptr=None), dict(channels=0), dict(sr=0.0),
                   dict(sr=-48000.0), dict(out_stride=width - 1), dict(f_stride=n - 1), dict(a_stride=n - 1),
                   dict(p_stride=n - 1), dict(batch=65_536)]
        for changed in refused:
            for ws_ptr in (ws.ptr, None):
                assert call(**changed, ws_ptr=ws_ptr) == PGX_ERR_INVALID, changed
                assert b"pgx_sine_stateful_bank" in L.pgx_last_error()
                untouched(changed)
        assert call(f_ptr=None, f_stride=0, a_ptr=None, a_stride=0, p_ptr=None, p_stride=0) == PGX_OK    # (no stream: its stride is not looked at)
        assert call() == PGX_OK                                    # (the same arguments, valid: it does run)
        assert np.all(np.isfinite(out.to_host()))
        assert np.all(st.to_host()[:, 1] == 1.0)
