"""
GPU: BiquadPE(SinePE) in closed form (pgx_biquad_tone, csrc/pgx_tone.hip: the settled tone scaled by |H| and shifted by
arg H) called directly at small sizes -- against the oracle (np.sin + scipy.signal.lfilter on the float32 sine) and
against pgx_biquad_sine on the same call; what it writes (guard bands, unaligned outputs, partial pieces); the carried
state, the snapshot and the seam into an exact block; the gate (pgx_biquad_tone_supported).

One case of the grid is declined by the gate itself and is asserted as such: the peaking section settles in 2048
frames, so n = 3 * 1024 + 5 is below 2 * settle_frames.
"""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
CHAINS = [dict(freq=440.0, amp=1.0, phase=0.0, cutoff=1000.0, q=0.707, mode="lowpass", gain_db=0.0),
          dict(freq=3000.3, amp=0.3, phase=1.1, cutoff=2500.0, q=2.0, mode="bandpass", gain_db=0.0),
          dict(freq=5500.0, amp=1.0, phase=0.0, cutoff=3000.0, q=0.707, mode="highpass", gain_db=0.0),
          dict(freq=700.0, amp=1.0, phase=0.0, cutoff=1000.0, q=1.0, mode="peaking", gain_db=6.0)]
DECLINED = dict(freq=55.0, amp=1.0, phase=0.0, cutoff=8000.0, q=0.707, mode="highpass", gain_db=0.0)
SIZES = [3 * 1024 + 5, 200_001]
STARTS = [0, 10_000, 10 ** 9]
BEFORE = 10_000                      # frames rendered exactly in front of `start` for the non-zero carried state


class _Chain:
    """The device-side constants of one chain, made once per test session."""

    def __init__(self, p):
        import pygmu2_amd as pg
        from pygmu2_amd import device
        from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
        self.p = p
        self.lib = device.ensure_init()
        self.c = rbj_coefficients(pg.BiquadMode(p["mode"]), p["cutoff"], p["q"], p["gain_db"], float(SR))
        self.settle = settle_frames(self.c[3], self.c[4])
        self.w = 2.0 * np.pi * p["freq"]
        self.coef = device.DeviceBuffer.from_host(np.asarray(self.c, dtype=np.float64))
        self.tables = device.DeviceBuffer((self.lib.pgx_biquad_table_doubles(),), np.float64)
        device.check(self.lib.pgx_biquad_tables(self.tables.ptr, self.coef.ptr, 1))

    def supported(self, n, settle=None):
        return self.lib.pgx_biquad_tone_supported(n, self.settle if settle is None else settle, self.w, float(SR), *self.c)

    def tone_into(self, out_ptr, start, n, state, backup):
        p = self.p
        return self.lib.pgx_biquad_tone(out_ptr, start, n, float(SR), self.w, p["amp"], p["phase"], *self.c,
                                        self.tables.ptr, self.settle, state.ptr, backup.ptr if backup else None)

    def tone(self, start, n, state0):
        from pygmu2_amd import device
        state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
        backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
        out = device.DeviceBuffer((n, 1), np.float32)
        device.check(self.tone_into(out.ptr, start, n, state, backup))
        return out.to_host()[:, 0], state.to_host().reshape(-1), backup.to_host().reshape(-1)

    def exact(self, start, n, state0):
        """pgx_biquad_sine (the recurrence) on the same call."""
        from pygmu2_amd import device
        p = self.p
        state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
        out = device.DeviceBuffer((n, 1), np.float32)
        device.check(self.lib.pgx_biquad_sine(out.ptr, start, n, float(SR), self.w, p["amp"], p["phase"], self.coef.ptr,
                                              self.tables.ptr, self.settle, state.ptr, None))
        return out.to_host()[:, 0], state.to_host().reshape(-1)


@functools.lru_cache(maxsize=None)
def _chain(k):
    return _Chain(CHAINS[k] if k >= 0 else DECLINED)


@functools.lru_cache(maxsize=None)
def _carried(k, start):
    """The filter state after an exact render of the BEFORE frames in front of `start`, from rest."""
    return tuple(_chain(k).exact(start - BEFORE, BEFORE, [0.0, 0.0])[1])


@functools.lru_cache(maxsize=None)
def _oracle(k, start, n, carried):
    """lfilter over the float32 sine: from rest at `start`, or from rest BEFORE frames in front of it."""
    from oracle import pe_oracle as O
    p = CHAINS[k]
    lead = BEFORE if carried else 0
    x = O.sine_pure(start - lead, n + lead, p["freq"], p["amp"], p["phase"], sr=SR)
    y = O.biquad_const(O.biquad_state(1), x, p["cutoff"], p["q"], p["mode"], p["gain_db"], SR)
    y = np.asarray(y, dtype=np.float64).reshape(-1)[lead:]
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _exact(k, start, n, carried):
    y, st = _chain(k).exact(start, n, _carried(k, start) if carried else (0.0, 0.0))
    y.setflags(write=False)
    return y, st


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("carried", [False, True], ids=["rest", "carried"])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", range(len(CHAINS)), ids=[c["mode"] for c in CHAINS])
def test_tone_against_the_oracle_and_the_recurrence(k, n, start, carried):
    ch = _chain(k)
    state0 = _carried(k, start) if carried else (0.0, 0.0)
    if n < 2 * ch.settle:                                   # (peaking, 3077): the gate's own condition declines it
        assert ch.supported(n) == 0
        from pygmu2_amd import device
        state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
        out = device.DeviceBuffer((n, 1), np.float32)
        assert ch.tone_into(out.ptr, start, n, state, None) == device.ERR_INVALID
        assert b"not supported" in ch.lib.pgx_last_error()
        return
    assert ch.supported(n) == 1
    got, _, backup = ch.tone(start, n, state0)
    assert np.array_equal(backup, np.asarray(state0))
    want = _oracle(k, start, n, carried)
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    cur = _exact(k, start, n, carried)[0]
    err_cur = float(np.max(np.abs(got.astype(np.float64) - cur)))
    print(f"chain {k} n {n} start {start} carried {carried}: vs lfilter {err / peak:.3e}, vs pgx_biquad_sine "
          f"{err_cur / peak:.3e} of peak {peak:.4f}; {np.count_nonzero(got != cur) / n:.3f} of the samples differ")
    assert err <= 1e-6 * peak + 1e-9, (err, peak)
    assert err_cur <= 5e-7 * peak, (err_cur, peak)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("n", [3 * 1024 + 5, 2 * 4096 + 1022, 4096 + 1])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_tone_writes_its_frames_and_nothing_else(offset, n):
    """Outputs 0 - 3 floats past a 16-byte boundary, block lengths that are no multiple of 4 or of the 4096-frame piece:
    the same samples bit for bit as the aligned call's, the floats around [out, out + n) and the guard bands untouched."""
    from guarded_alloc import guarded
    from pygmu2_amd import device
    ch = _chain(0)
    start, pad = 12_345, 64
    ref = ch.tone(start, n, [0.25, -0.125])[0]
    with guarded():
        buf = device.DeviceBuffer((n + 2 * pad,), np.float32)          # poisoned: every float 0xFFFFFFFF
        state = device.DeviceBuffer.from_host(np.asarray([[0.25, -0.125]], dtype=np.float64))
        first = pad + offset
        device.check(ch.tone_into(buf.ptr + 4 * first, start, n, state, None))
        host = buf.to_host().reshape(-1)
    bits = host.view(np.uint32)
    assert np.all(bits[:first] == 0xFFFFFFFF) and np.all(bits[first + n:] == 0xFFFFFFFF)
    assert np.array_equal(host[first:first + n].view(np.uint32), ref.view(np.uint32))


# ------------------------------------------------------------------------------------------------ state
@pytest.mark.parametrize("k", range(len(CHAINS)), ids=[c["mode"] for c in CHAINS])
def test_tone_state_snapshot_and_seam(k):
    ch = _chain(k)
    start, n, tail = 10_000, 200_001, 8192
    state0 = _carried(k, start)
    y, st, backup = ch.tone(start, n, state0)
    assert np.array_equal(backup, np.asarray(state0))                  # the snapshot: the incoming state bit for bit
    st_cur = _exact(k, start, n, True)[1]
    assert float(np.max(np.abs(st - st_cur))) <= 1e-6, (st, st_cur)
    # the same call twice: the same bits, samples and state
    y2, st2, _ = ch.tone(start, n, state0)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(st, st2)
    # a tone window, then an exact block from the state it left: no seam against the oracle's one stream
    nxt = ch.exact(start + n, tail, st)[0]
    want = _oracle(k, start, n, True)
    from oracle import pe_oracle as O
    p = CHAINS[k]
    x = O.sine_pure(start - BEFORE, BEFORE + n + tail, p["freq"], p["amp"], p["phase"], sr=SR)
    full = np.asarray(O.biquad_const(O.biquad_state(1), x, p["cutoff"], p["q"], p["mode"], p["gain_db"], SR),
                      dtype=np.float64).reshape(-1)[BEFORE:]
    peak = float(np.max(np.abs(want)))
    seam = float(np.max(np.abs(nxt.astype(np.float64) - full[n:])))
    print(f"chain {k}: state {st} against {st_cur}, seam {seam / peak:.3e} of peak")
    assert seam <= 1e-6 * peak, (seam, peak)


# ------------------------------------------------------------------------------------------------ gate
def test_gate():
    ch = _chain(0)
    assert ch.supported(200_001) == 1
    assert ch.supported(200_001, settle=0) == 0                        # a section that does not forget
    assert ch.supported(2 * ch.settle - 1) == 0 and ch.supported(2 * ch.settle) == 1
    low = _chain(-1)                                                   # 55 Hz -> highpass 8 kHz: the output is rounding noise
    assert low.settle > 0 and low.supported(200_001) == 0 and low.supported(134_000_000) == 0


def _render_window(pg, p, tone, blocks):
    from pygmu2_amd import biquad_pe, look_ahead
    pg.set_sample_rate(SR)
    keep = biquad_pe.TONE_WINDOWS
    biquad_pe.TONE_WINDOWS = tone
    look_ahead.set_enabled(False)
    try:
        pe = pg.BiquadPE(pg.SinePE(frequency=p["freq"], amplitude=p["amp"], phase=p["phase"]), frequency=p["cutoff"],
                         q=p["q"], mode=pg.BiquadMode(p["mode"]), gain_db=p["gain_db"])
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(pe)
        r.start()
        outs = [pe.render(s, n).data.reshape(-1).copy() for s, n in blocks]
        taken = dict(pe._tone_supported)
        r.stop()
        return outs, taken
    finally:
        biquad_pe.TONE_WINDOWS = keep
        look_ahead.set_enabled(True)


WINDOW = 17_000_000                 # window-sized: pgx_biquad_sine hands it to its wave-run kernel


def test_declined_chain_is_still_the_two_launch_chain_through_the_pe():
    import pygmu2_amd as pg
    from pygmu2_amd import biquad_pe
    blocks = [(10 ** 9, WINDOW)]
    (a,), _ = _render_window(pg, DECLINED, True, blocks)
    keep = biquad_pe.FUSE_SINE_SOURCE
    biquad_pe.FUSE_SINE_SOURCE = False
    try:
        (b,), _ = _render_window(pg, DECLINED, True, blocks)
    finally:
        biquad_pe.FUSE_SINE_SOURCE = keep
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_pe_takes_the_tone_window_and_it_continues_into_blocks():
    """Through the PE: a window-sized render takes the closed form (switch on) and equals the wave-run kernel's (switch
    off) to a few float32 roundings; so do the 1 M-frame blocks rendered exactly from the state each left."""
    import pygmu2_amd as pg
    blocks = [(10 ** 9, WINDOW), (10 ** 9 + WINDOW, 1_000_000), (10 ** 9 + WINDOW + 1_000_000, 3000)]
    new, taken = _render_window(pg, CHAINS[0], True, blocks)
    cur, off = _render_window(pg, CHAINS[0], False, blocks)
    assert taken == {WINDOW: True, 1_000_000: False, 3000: False} and off == {}
    peak = max(float(np.max(np.abs(b))) for b in cur)
    for a, b in zip(new, cur):
        err = float(np.max(np.abs(a.astype(np.float64) - b)))
        print(f"{a.size} frames: {err / peak:.3e} of peak, {np.count_nonzero(a != b) / a.size:.3f} of the samples differ")
        assert err <= 5e-7 * peak, (err, peak)
