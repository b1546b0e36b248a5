"""CPU: ReversePitchEchoPE without a device.  The class's host side -- repr, extent, purity, channel count, input order
-- is the reference's as tests/golden/reverse_echo_cases.json recorded it; the sizes it derives from the sample rate
and the echo-block length of a scalar block_seconds are the reference's; the constants of include/pygmu_hip.h, of
pygmu2_amd/device.py and of the class agree; pgx_reverse_echo refuses bad arguments before it looks for a device."""

import numpy as np
import pytest

import pygmu2_amd as pg
import reverse_echo_common as RC
from fixture_harness import load_cases, split_blocks
from pygmu2_amd import device
from pygmu2_amd.build import build

CASES, NPZ = load_cases(RC.FAMILY)
ALL = CASES["cases"]
BY_NAME = {c["name"]: c for c in ALL}
INVALID = -1                      # PGX_ERR_INVALID


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_host_side_matches_reference(case):
    pe, made = RC.build_case(case)
    ext = pe.extent()
    assert [ext.start, ext.end] == case["extent"]
    assert len(made) == len(case["new_pes"]) == len(case["sizes"]) > 0
    for m, ref, sizes in zip(made, case["new_pes"], case["sizes"]):
        assert type(m) is pg.ReversePitchEchoPE
        assert repr(m) == ref["repr"]
        assert [m.extent().start, m.extent().end] == ref["extent"]
        assert m.is_pure() is ref["pure"] is False
        assert m.channel_count() == ref["channels"]
        assert [type(i).__name__ for i in m.inputs()] == ref["inputs"]
        assert m.inputs()[0] is m.source
        assert (m._buffer_rows(), m._pitch_len(), m._initial_smoothed()) == \
            (sizes["rows"], sizes["pitch_len"], sizes["initial_smoothed"])
        if not m._block_is_pe:
            # a scalar block_seconds: the one-pole rests on it, every echo block has the clamped, rounded size
            assert set(case["echo_blocks"]) == {m._initial_smoothed()}


def test_sizes_at_both_sample_rates():
    seen = {c["sr"]: c["sizes"][0] for c in ALL}
    assert (seen[8000]["rows"], seen[8000]["pitch_len"]) == (80000, 133)
    assert (seen[48000]["rows"], seen[48000]["pitch_len"]) == (480000, 800)
    assert BY_NAME["defaults_like"]["sizes"][0]["initial_smoothed"] == 160
    assert BY_NAME["block_below_minimum"]["sizes"][0]["initial_smoothed"] == 64
    assert BY_NAME["block_stream"]["sizes"][0]["initial_smoothed"] == 2000          # 0.25 s under a stream parameter
    assert BY_NAME["sr48k_block_stream"]["sizes"][0]["initial_smoothed"] == 12000
    pg.set_sample_rate(8000)
    src = pg.ConstantPE(0.0)
    assert pg.ReversePitchEchoPE(src, float("inf"))._initial_smoothed() == 64       # not finite: the minimum
    assert pg.ReversePitchEchoPE(src, 100.0)._initial_smoothed() == 79999           # rows - 1


def test_fixture_covers_what_it_must():
    for c in ALL:
        assert c["compare"] == "fuzz" and len(c["echo_blocks"]) >= 6, c["name"]
        assert float(np.max(np.abs(NPZ[c["name"]]))) > 0.05, c["name"]
        # the first echo block of a stream is exactly silent
        assert not np.any(NPZ[c["name"]][:min(c["echo_blocks"][0], c["blocks"][0][1])]) or c["name"] == "dry_wet_mix"
    assert {c["new_pes"][0]["channels"] for c in ALL} >= {1, 2, 3}
    assert set(BY_NAME["block_below_minimum"]["echo_blocks"]) == {64}
    for name in ("block_stream", "sr48k_block_stream", "all_four_streams_2ch"):
        d = np.diff(BY_NAME[name]["echo_blocks"])
        assert np.any(d > 0) and np.any(d < 0), name
    assert not np.array_equal(NPZ["alternate_0"], NPZ["alternate_1"])
    assert len(BY_NAME["ratio_stream_2ch_uses_channel_0"]["new_pes"][0]["inputs"]) == 2
    assert BY_NAME["all_four_streams_2ch"]["new_pes"][0]["inputs"] == ["ArrayPE", "TransformPE", "TransformPE",
                                                                        "TransformPE", "ArrayPE"]
    blocks = BY_NAME["gap_and_seek"]["blocks"]
    steps = [blocks[i][0] - (blocks[i - 1][0] + blocks[i - 1][1]) for i in range(1, len(blocks))]
    assert any(s > 0 for s in steps) and any(s < 0 for s in steps)
    case = BY_NAME["reset_and_restart"]
    assert case["ops"] == {"2": "reset", "4": "restart"}
    stored = split_blocks(case, NPZ[case["name"]])
    assert np.any(stored[2][:160]) and not np.any(stored[4][:160]) and np.any(stored[4][160:])
    for c in ALL:
        if c["patterns"]:
            n = c["blocks"][0][1]
            assert set(c["patterns"]) == {"edges", "around", "b64", "ones"}
            for blocks in c["patterns"].values():
                assert blocks[0][0] == 0 and sum(b[1] for b in blocks) == n
                assert all(blocks[i][0] == blocks[i - 1][0] + blocks[i - 1][1] for i in range(1, len(blocks)))


def test_constructor_and_export():
    assert pg.ReversePitchEchoPE.__name__ == "ReversePitchEchoPE"
    # bound in the namespace, not in __all__: entering the fuzz census of exported PEs is a later change
    assert "ReversePitchEchoPE" not in pg.__all__
    pg.set_sample_rate(8000)
    src = pg.SinePE(3.0)
    pe = pg.ReversePitchEchoPE(src)
    assert (pe._block_seconds, pe._pitch_ratio, pe._feedback, pe._alternate_direction, pe._smoothing_samples) == \
        (0.25, 1.0, 0.85, 0.0, 2400)
    assert pe.source is src and pe.inputs() == [src] and not pe.is_pure() and pe.channel_count() == 1
    for given, kept in ((0, 1), (-5, 1), (2.9, 2), (1, 1), (50, 50)):
        assert pg.ReversePitchEchoPE(src, smoothing_samples=given)._smoothing_samples == kept
    block, ratio, fb, alt = pg.ConstantPE(0.02), pg.ConstantPE(1.5), pg.ConstantPE(0.5), pg.ConstantPE(1.0)
    assert pg.ReversePitchEchoPE(src, block, ratio, fb, alt).inputs() == [src, block, ratio, fb, alt]
    assert pg.ReversePitchEchoPE(src, 0.02, ratio, 0.5, alt).inputs() == [src, ratio, alt]
    crop = pg.CropPE(src, 10, 90)
    assert pg.ReversePitchEchoPE(src, pitch_ratio=crop).extent() == crop.extent()
    assert not getattr(pe, "_LOOK_AHEAD_SAFE", False)                    # renders block by block
    assert not hasattr(pe, "_reset_state")                               # reset_state() changes nothing
    with pytest.raises(ValueError, match="duration must be >= 0"):
        pe.render(0, -1)
    empty = pe.render(7, 0)                                               # no kernel, no device needed
    assert empty.start == 7 and empty.duration == 0 and empty.channels == 1


def test_constants_shared_with_the_header():
    defines = {k: v for k, v in device._ABI.constants.items() if k.startswith("PGX_REVERSE_ECHO_")}
    assert defines == {
        "PGX_REVERSE_ECHO_MIN_BLOCK": device.REVERSE_ECHO_MIN_BLOCK,
        "PGX_REVERSE_ECHO_MAX_FEEDBACK": device.REVERSE_ECHO_MAX_FEEDBACK,
        "PGX_REVERSE_ECHO_MIN_RATIO": device.REVERSE_ECHO_MIN_RATIO,
        "PGX_REVERSE_ECHO_UNITY_BAND": device.REVERSE_ECHO_UNITY_BAND}
    assert (device.REVERSE_ECHO_MIN_BLOCK, device.REVERSE_ECHO_MAX_FEEDBACK, device.REVERSE_ECHO_MIN_RATIO,
            device.REVERSE_ECHO_UNITY_BAND) == (64, 0.995, 0.001, 1e-4)
    assert type(device.REVERSE_ECHO_MIN_BLOCK) is int
    cls = pg.ReversePitchEchoPE
    assert (cls._MAX_DELAY_SECONDS, cls._MIN_BLOCK_SAMPLES, cls._MAX_FEEDBACK) == (10.0, 64, 0.995)
    # the record of the header, field by field
    assert device.REVERSE_ECHO_STATE is device._ABI.struct("pgx_reverse_echo_state")
    assert [(name, device.REVERSE_ECHO_STATE.fields[name][0].str) for name in device.REVERSE_ECHO_STATE.names] == \
        [("smoothed", "<f8"), ("read_pos", "<f8"), ("write_idx", "<i8"), ("read_idx", "<i8"), ("current_block", "<i8"),
         ("prev_len", "<i8"), ("pitch_write_pos", "<i8"), ("reverse", "<i4"), ("current_is_a", "<i4"),
         ("pitch_parity", "<i4"), ("pad", "<i4")]
    assert device.REVERSE_ECHO_STATE.itemsize == 72


def test_entry_point_refuses_bad_arguments():
    """Every call here is invalid, or has n == 0: none reaches a launch, with or without a device."""
    build()
    L = device.load_library()
    assert L.pgx_reverse_echo_workspace_bytes(0, 2) == 0 and L.pgx_reverse_echo_workspace_bytes(100, 0) == 0
    assert L.pgx_reverse_echo_workspace_bytes(1000, 2) >= 1000 * (2 + 2) * 8
    p = 4096                                                             # a non-null address that is never read

    def call(out=p, src=p, n=16, channels=1, sr=8000.0, smoothing=2400, state=p, a=p, b=p, rows=80000, hist=p, plen=133,
             ws=p):
        return L.pgx_reverse_echo(out, src, n, channels, sr, 0.02, None, 1.0, None, 0.85, None, 0.0, None, smoothing,
                                  state, a, b, rows, hist, plen, ws)

    for bad in (dict(state=None), dict(a=None), dict(b=None), dict(hist=None), dict(out=None), dict(src=None),
                dict(ws=None), dict(channels=0), dict(n=-1), dict(rows=64), dict(rows=0), dict(plen=1),
                dict(smoothing=0), dict(sr=0.0), dict(sr=float("nan"))):
        assert call(**bad) == INVALID, bad
        assert b"pgx_reverse_echo" in L.pgx_last_error()
    # n == 0: nothing to do, nothing launched -- success on a device, "not initialised" without one
    assert call(n=0, out=None, src=None, ws=None) in (0, -3)
