"""
GPU: every channel-aware kernel at 3, 4, 5 and 8 channels (tests/channel_cases.py), HIP path against

* the reference's own renders (tests/golden/channels_cases.json + channels.npz, tools/gen_golden_channels.py) on the
  blocks the fixture stores, and
* the oracle on every block (tests/test_oracle_channels.py pins the oracle to the same fixture first).

A graph built only from bit-exact kinds (fuzz_graphs_all.bit_exact) must match exactly; every other graph is held to
tests/test_gpu_parity.py's bar, 1e-5 of the block's peak + its floor, three times that on the stream patterns and from a
case's long block on (channel_cases.compare_block, which tests/test_oracle_channels.py turns against swapped and late
columns).  Then what the PE layer cannot set up: MixPEs of 24 voices at C = 3 through the voice bank, and the entry
points pgx_score_mix, pgx_karplus_score, pgx_gain_vec, pgx_gain_mix_batch, pgx_extract_channel, pgx_mono_mean and the
PCM16 pair through the C ABI, against numpy in float32 in the reference's order of operations.

The families with oracles of their own (playback, control, spectral, score) keep their `ch<C>_*` cases in their own
fixtures and GPU modules: see the end of channel_cases.py's docstring.

Each check prints `CHANNELS_RATIO <case> <against> <largest err / (rel * peak + floor)>` before it asserts.
"""

import json
import os
import wave

import numpy as np
import pytest

import channel_cases
from channel_cases import compare_block

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "channels_cases.json")) as _f:
    CASES = json.load(_f)
STREAMS = [c for c in CASES if c["pattern"] == "stream"]
BLOCKS = [c for c in CASES if c["pattern"] != "stream"]
PURE_STREAMS = {"WindowPE", "DelayPE"}        # stateless over an ArrayPE: nothing for look-ahead to run ahead of


@pytest.fixture(scope="module")
def npz():
    return np.load(os.path.join(GOLDEN, "channels.npz"))


def _judge(case, against, got, want, indices):
    worst, failures = 0.0, []
    for i, g, w in zip(indices, got, want):
        ok, ratio, msg = compare_block(case, i, g, w)
        worst = max(worst, ratio)
        if not ok:
            failures.append(msg)
    print(f"CHANNELS_RATIO {case['name']} {against} {worst:.3f}")
    assert not failures, (against, failures[:4], case["graph"])


def _check(case, npz):
    from oracle.graph_eval import run_case as oracle_run
    from spec_build import run_case as hip_run
    got = hip_run(case)
    stored = [npz[f"{case['name']}/{i}"] for i in case["keep"]]
    channels = stored[0].shape[1]                       # what the reference gave: C, bar SpatialPE's own widths
    if case["kind"] != "SpatialPE":
        assert channels == case["C"]
    for (_, n), g in zip(case["blocks"], got):
        assert g.shape == (n, channels), (case["name"], g.shape, (n, channels))
    _judge(case, "reference", [got[i] for i in case["keep"]], stored, case["keep"])
    _judge(case, "oracle", got, oracle_run(case), range(len(got)))


@pytest.mark.parametrize("case", BLOCKS, ids=lambda c: c["name"])
def test_hip_matches_reference_and_oracle(case, npz):
    _check(case, npz)


@pytest.mark.parametrize("ahead", [True, False], ids=["look_ahead", "no_look_ahead"])
@pytest.mark.parametrize("case", STREAMS, ids=lambda c: c["name"])
def test_streams_with_and_without_look_ahead(case, ahead, npz):
    """Look-ahead and read-ahead windows hand out row views at frame offsets times C * 4 bytes: with three channels
    16-byte aligned at every fourth offset only, so every consumer's aligned16 test takes both branches in one stream."""
    from pygmu2_amd import look_ahead
    was = look_ahead.enabled()
    look_ahead.set_enabled(ahead)
    try:
        before = look_ahead.STATS["windows"]
        _check(case, npz)
        opened = look_ahead.STATS["windows"] - before
    finally:
        look_ahead.set_enabled(was)
    print(f"CHANNELS_WINDOWS {case['name']} look_ahead={ahead} windows={opened}")
    if not ahead:
        assert opened == 0
    elif case["kind"] not in PURE_STREAMS:
        assert opened > 0, "the stream was not served from look-ahead windows"


# ---------------------------------------------------------------------------------------------- voice banks, C = 3
@pytest.mark.parametrize("case", channel_cases.bank_cases(), ids=lambda c: c["name"])
def test_voice_bank_of_three_channel_voices(case):
    import pygmu2_amd as pg
    import spec_build
    from oracle.graph_eval import run_case as oracle_run
    pg.set_sample_rate(case["sr"])
    mix = spec_build.build(case["graph"])
    r = pg.NullRenderer(sample_rate=case["sr"])
    r.set_source(mix)
    r.start()
    assert mix._voice_bank(), "24 voices of one signature did not make a voice bank"
    got = [mix.render(int(s), int(n)).data.copy() for s, n in case["blocks"]]
    r.stop()
    for (_, n), g in zip(case["blocks"], got):
        assert g.shape == (n, 3)
    _judge(case, "oracle", got, oracle_run(case), range(len(got)))          # a MixPE of 24: the float bar


# ---------------------------------------------------------------------------------------------- through the C ABI
@pytest.mark.parametrize("ch", [3, 5])
def test_score_mix_kernel_at_odd_channel_counts(ch):
    from test_gpu_score import check_score_mix_kernel
    check_score_mix_kernel(ch, frames=3000, count=40, edges=(1, 2), crowd=10)


@pytest.mark.parametrize("ch,group", [(3, 16), (5, 7), (3, 64)])
def test_karplus_score_kernel_at_odd_channel_counts(ch, group):
    from test_gpu_score import check_karplus_score_kernel
    check_karplus_score_kernel(ch, group, count=24)


def _device():
    from pygmu2_amd import device
    return device.ensure_init(), device.DeviceBuffer


N_ABI = 4099          # frames: odd, several workgroups, n * C a multiple of 4 only at C = 4 and 8


@pytest.mark.parametrize("ch", [3, 4, 5, 8])
@pytest.mark.parametrize("wide", [False, True], ids=["mono_gain", "wide_gain"])
def test_gain_vec_broadcast(ch, wide):
    lib, Buf = _device()
    rng = np.random.default_rng(100 + ch)
    x = rng.standard_normal((N_ABI, ch)).astype(np.float32)
    g = rng.standard_normal((N_ABI, ch if wide else 1)).astype(np.float32)
    out = Buf((N_ABI, ch), np.float32)
    out.upload(np.full((N_ABI, ch), np.nan, dtype=np.float32))
    xd, gd = Buf.from_host(x), Buf.from_host(g)
    assert lib.pgx_gain_vec(out.ptr, xd.ptr, gd.ptr, N_ABI, ch, g.shape[1]) == 0
    assert np.array_equal(out.to_host(), x * g)                       # one float32 multiply (gain_pe.py:104-119)


@pytest.mark.parametrize("ch", [3, 5, 8])
@pytest.mark.parametrize("wide", [False, True], ids=["mono_gain", "wide_gain"])
def test_gain_mix_batch_broadcast(ch, wide):
    lib, Buf = _device()
    rng = np.random.default_rng(200 + ch)
    k, n, gch = 7, 1237, ch if wide else 1
    x = rng.standard_normal((k, n, ch)).astype(np.float32)
    g = rng.standard_normal((k, n, gch)).astype(np.float32)
    out = Buf((n, ch), np.float32)
    out.upload(np.full((n, ch), np.nan, dtype=np.float32))
    xd, gd = Buf.from_host(x), Buf.from_host(g)
    rc = lib.pgx_gain_mix_batch(out.ptr, xd.ptr, n * ch, gd.ptr, n * gch, k, n, ch, gch)
    assert rc == 0, lib.pgx_last_error()
    want = x[0] * g[0]                                                # products rounded to float32, added in voice order
    for b in range(1, k):
        want = want + x[b] * g[b]
    assert np.array_equal(out.to_host(), want)


@pytest.mark.parametrize("ch", [3, 4, 5, 8])
def test_extract_channel_every_channel(ch):
    lib, Buf = _device()
    x = np.random.default_rng(300 + ch).standard_normal((N_ABI, ch)).astype(np.float32)
    xd = Buf.from_host(x)
    for c in range(ch):
        out = Buf((N_ABI, 1), np.float32)
        out.upload(np.full((N_ABI, 1), np.nan, dtype=np.float32))
        assert lib.pgx_extract_channel(out.ptr, xd.ptr, N_ABI, ch, c) == 0
        assert np.array_equal(out.to_host()[:, 0], x[:, c]), c


@pytest.mark.parametrize("ch", [3, 5, 8, 9, 16, 21, 128])
def test_mono_mean_is_numpys_float32_mean(ch):
    lib, Buf = _device()
    x = np.random.default_rng(400 + ch).standard_normal((N_ABI, ch)).astype(np.float32)
    out = Buf((N_ABI, 1), np.float32)
    out.upload(np.full((N_ABI, 1), np.nan, dtype=np.float32))
    xd = Buf.from_host(x)
    assert lib.pgx_mono_mean(out.ptr, xd.ptr, N_ABI, ch) == 0
    want = np.mean(x, axis=1)                           # spatial_pe.py:483: float32 adds in numpy's order, one division
    assert want.dtype == np.float32 and np.array_equal(out.to_host()[:, 0], want)


@pytest.mark.parametrize("src_ch,out_ch", [(3, 3), (8, 3), (3, 8), (8, 1), (12, 1), (16, 3), (21, 2)])
def test_channel_adapt_is_the_oracles_adapter(src_ch, out_ch):
    """Bit for bit (tests/test_gpu_parity.py holds the adapter cases so): from 8 averaged channels on numpy adds a
    float32 row on eight running sums, not one after the other."""
    from oracle import pe_oracle as O
    lib, Buf = _device()
    x = np.random.default_rng(500 + src_ch).standard_normal((N_ABI, src_ch)).astype(np.float32)
    xd, out = Buf.from_host(x), Buf((N_ABI, out_ch), np.float32)
    out.upload(np.full((N_ABI, out_ch), np.nan, dtype=np.float32))
    assert lib.pgx_channel_adapt(out.ptr, xd.ptr, N_ABI, src_ch, out_ch) == 0
    assert np.array_equal(out.to_host(), O.spatial_adapter(x, out_ch))


def test_more_than_128_source_channels_are_refused():
    """numpy halves a row of more than 128 terms before it adds: not restated on the device, so an error, not a result
    that is off in the last bit."""
    lib, Buf = _device()
    x = Buf.from_host(np.zeros((4, 129), dtype=np.float32))
    out = Buf((4, 2), np.float32)
    assert lib.pgx_mono_mean(out.ptr, x.ptr, 4, 129) != 0
    assert lib.pgx_channel_adapt(out.ptr, x.ptr, 4, 129, 2) != 0
    assert lib.pgx_pan(out.ptr, x.ptr, 4, 129, 0.0, None, 0) != 0
    assert lib.pgx_mono_mean(out.ptr, x.ptr, 4, 128) == 0


# ---------------------------------------------------------------------------------------------- WAV, three channels
def test_render_to_file_and_read_back_three_channels(tmp_path):
    """render_to_file (k_f32_to_pcm16) and WavReaderPE (pgx_pcm16_to_f32) over 3 interleaved channels, by the rule
    tests/test_gpu_wav.py asserts: the file holds float_to_pcm16 of the render, the reader gives pcm16_to_float of it."""
    import pygmu2_amd as pg
    from oracle import pe_oracle as O
    from oracle.golden_cases import materialize_array
    pg.set_sample_rate(44100)
    frames = 6041
    data = materialize_array({"rng": 77, "n": frames, "ch": 3, "scale": 0.6})        # beyond +-1 here and there: saturates
    assert np.max(np.abs(data)) > 1.0
    path = str(tmp_path / "three.wav")
    pg.render_to_file(pg.ArrayPE(data), path)
    with wave.open(path, "rb") as f:
        assert (f.getnchannels(), f.getframerate(), f.getnframes(), f.getsampwidth()) == (3, 44100, frames, 2)
        raw = np.frombuffer(f.readframes(frames), dtype="<i2").reshape(-1, 3)
    assert np.array_equal(raw, O.float_to_pcm16(data))
    reader = pg.WavReaderPE(path)
    assert reader.channel_count() == 3 and (reader.extent().start, reader.extent().end) == (0, frames)
    got = reader.render(-10, frames + 59).data
    assert got.shape == (frames + 59, 3) and not np.any(got[:10]) and not np.any(got[10 + frames:])
    assert np.array_equal(got[10:10 + frames], O.pcm16_to_float(raw))
