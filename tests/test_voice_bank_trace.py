"""
CPU: what a voice bank launches, in which order, on which stream, with which buffers -- pinned against a recorded trace
(tests/bank_trace.py: the stand-ins for the library and the buffers, the canonical form, what must match).

Cases: SuperSaw banks of every size class, the C4 (ladder) and C5 (BlitSaw -> Biquad x envelope) voices, comb, constant
biquad, sine and constant-gain banks, each under the switches that change its path, over a script of windows, seeks,
another block length and a reset.

    python tests/test_voice_bank_trace.py --record        writes tests/golden/voice_bank_trace.json
"""

import os

import pytest

from bank_trace import assert_matches, launches, record_main, recorded, recorded_names, run

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voice_bank_trace.json")
SWITCHES = ("BANK_WINDOWS", "LADDER_WINDOWS", "ENVELOPE_AHEAD", "PREFETCH_SUPERSAW_VOICES", "PREFETCH_LADDER_INPUT")
ALL_OFF = {name: False for name in SWITCHES}


# ------------------------------------------------------------------------------------------------------------ cases
def voices(pg, kind, count):
    from pygmu2_amd.sharding import c4_voice, c5_voice
    if kind == "supersaw":
        nv = {8: 3, 64: 7, 130: 1, 260: 7}[count]
        return [pg.SuperSawPE(55.0 * 2 ** (i / 24.0), voices=nv, detune_cents=20.0, seed=i) for i in range(count)]
    if kind == "c4":
        return [c4_voice(pg, i) for i in range(count)]
    if kind == "c5":
        return [c5_voice(pg, i) for i in range(count)]
    if kind == "comb":
        return [pg.CombPE(pg.BlitSawPE(55.0 * 2 ** (i / 12.0)), frequency=110.0 * 2 ** (i / 24.0), feedback=0.7)
                for i in range(count)]
    if kind == "biquad":
        return [pg.BiquadPE(pg.BlitSawPE(27.5 * 2 ** (i / 48.0)), frequency=2000.0, q=0.707) for i in range(count)]
    if kind == "sine":
        return [pg.SinePE(220.0 + 3.0 * i, amplitude=0.1) for i in range(count)]
    if kind == "gain":                      # constant gains, one per voice: a launch per voice
        return [pg.GainPE(pg.BlitSawPE(55.0 * 2 ** (i / 12.0)), gain=0.25 + 0.125 * (i % 3)) for i in range(count)]
    if kind == "gain_equal":                # ... all the same: one launch
        return [pg.GainPE(pg.BlitSawPE(55.0 * 2 ** (i / 12.0)), gain=0.5) for i in range(count)]
    raise KeyError(kind)


def script(block, odd):
    """Nine equal blocks (windows of 2 and 4 open, the window of 8 is left after two of its blocks), two blocks after a
    seek of +100 frames, two blocks of another length, two blocks from frame 0 again, reset() and one more block."""
    pulls, pos = [], 0
    for _ in range(9):
        pulls.append((pos, block))
        pos += block
    pos += 100
    for size in (block, block, odd, odd):
        pulls.append((pos, size))
        pos += size
    pulls += [(0, block), (block, block), "reset", (2 * block, block)]
    return pulls


LONG, SHORT = script(6000, 5000), script(1024, 1000)        # (SHORT: below every 4096 threshold)

# (kind, instances, switches, mix-level windows, script, [(kernel, stream)] that must occur)
CASES = {}


def _case(kind, count, expect, switches=None, mix_windows=False, pulls="LONG", tag=None):
    name = f"{kind}-{count}" + (f"-{tag}" if tag else "")
    assert name not in CASES
    CASES[name] = (kind, count, switches or {}, mix_windows, pulls, expect)


_case("supersaw", 8, [("pgx_supersaw_wide", 0)])
_case("supersaw", 64, [("pgx_supersaw_wide", 0)])
_case("supersaw", 130, [("pgx_blitsaw", 0), ("pgx_supersaw_sum", 1), ("pgx_mix_batch", 1)])
_case("supersaw", 260, [("pgx_supersaw_bank_seg", 0), ("pgx_mix_batch", 1)])
_case("c4", 8, [("pgx_ladder", 0), ("pgx_supersaw_wide", 1)])
_case("c5", 6, [("pgx_blitsaw_biquad_wide_seg", 0), ("pgx_adsr_gated_periodic_to", 1), ("pgx_gain_mix_batch", 0)])
_case("c5", 64, [("pgx_voice_tiles", 0), ("pgx_adsr_gated_periodic_to", 1)])
_case("c5", 200, [("pgx_voice_tiles", 0), ("pgx_adsr_gated_periodic_to", 1)])
_case("comb", 8, [("pgx_comb", 0), ("pgx_supersaw_wide", 0)])
_case("biquad", 16, [("pgx_voice_tiles", 0)])
_case("biquad", 128, [("pgx_voice_tiles", 0)])
_case("sine", 8, [("pgx_sine_render", 0)])
_case("gain", 8, [("pgx_gain_const", 0)])
_case("gain_equal", 8, [("pgx_gain_const", 0)])
_case("supersaw", 8, [("pgx_supersaw_bank_seg", 0)], {"WIDE_SUPERSAW": False}, tag="narrow")
_case("supersaw", 260, [("pgx_supersaw_bank_seg", 0)], {"WIDE_SUPERSAW": False}, tag="narrow")
_case("c5", 64, [("pgx_supersaw_bank_seg", 0), ("pgx_biquad_const", 0)], {"WIDE_SUPERSAW": False}, tag="narrow")
_case("biquad", 128, [("pgx_blitsaw_biquad_bank", 0)], {"WIDE_SUPERSAW": False}, tag="narrow")
_case("supersaw", 8, [("pgx_blitsaw", 0), ("pgx_supersaw_sum", 1)], {"SEGMENTED_SUPERSAW": False}, tag="unsegmented")
_case("supersaw", 64, [("pgx_blitsaw", 0), ("pgx_supersaw_sum", 1)], {"SEGMENTED_SUPERSAW": False}, tag="unsegmented")
_case("comb", 8, [("pgx_comb", 0), ("pgx_blitsaw", 0)], {"SEGMENTED_SUPERSAW": False}, tag="unsegmented")
_case("c5", 6, [("pgx_supersaw_wide", 0), ("pgx_biquad_const", 0)], {"SEGMENTED_CHAIN": False}, tag="nochain")
_case("biquad", 16, [("pgx_supersaw_wide", 0), ("pgx_biquad_const", 0)],
      {"SEGMENTED_CHAIN": False, "VOICE_TILES": False}, tag="nochain")
_case("c5", 64, [("pgx_blitsaw_biquad_wide_seg", 0), ("pgx_gain_mix_batch", 0)], {"VOICE_TILES": False}, tag="notiles")
_case("c5", 200, [("pgx_blitsaw_biquad_wide", 0), ("pgx_gain_mix_batch", 0)], {"VOICE_TILES": False}, tag="notiles")
_case("biquad", 128, [("pgx_blitsaw_biquad_wide", 0), ("pgx_mix_batch", 0)], {"VOICE_TILES": False}, tag="notiles")
_case("c5", 6, [("pgx_voice_tiles", 0)], {"VOICE_TILES_MIN_VOICES": 4}, tag="tiles4")
_case("supersaw", 8, [("pgx_supersaw_wide", 0)], ALL_OFF, tag="off")
_case("supersaw", 130, [("pgx_blitsaw", 0), ("pgx_supersaw_sum", 0)], ALL_OFF, tag="off")
_case("supersaw", 260, [("pgx_supersaw_bank_seg", 0)], ALL_OFF, tag="off")
_case("c4", 8, [("pgx_ladder", 0), ("pgx_supersaw_wide", 0)], ALL_OFF, tag="off")
_case("c5", 64, [("pgx_voice_tiles", 0), ("pgx_adsr_gated_periodic", 0)], ALL_OFF, tag="off")
_case("comb", 8, [("pgx_comb", 0)], ALL_OFF, tag="off")
_case("supersaw", 8, [("pgx_supersaw_wide", 0)], mix_windows=True, tag="mixwin")
_case("c4", 8, [("pgx_ladder", 0), ("pgx_supersaw_wide", 1)], mix_windows=True, tag="mixwin")
_case("c5", 6, [("pgx_blitsaw_biquad_wide_seg", 0), ("pgx_gain_mix_batch", 0)], pulls="SHORT", tag="short")
_case("c5", 64, [("pgx_blitsaw_biquad_wide_seg", 0), ("pgx_adsr_gated_periodic_to", 1)], pulls="SHORT", tag="short")
_case("c5", 200, [("pgx_blitsaw_biquad_wide", 0), ("pgx_adsr_gated_periodic_to", 1)], pulls="SHORT", tag="short")
_case("supersaw", 8, [("pgx_supersaw_wide", 0)], pulls="SHORT", tag="short")
_case("supersaw", 130, [("pgx_blitsaw", 0), ("pgx_supersaw_sum", 0)], pulls="SHORT", tag="short")
_case("supersaw", 260, [("pgx_supersaw_bank_seg", 0)], pulls="SHORT", tag="short")


def run_case(monkeypatch, name):
    """-> the canonical trace of case `name`."""
    import pygmu2_amd as pg
    kind, count, switches, mix_windows, pulls, _ = CASES[name]
    return run(monkeypatch, lambda: voices(pg, kind, count), {"LONG": LONG, "SHORT": SHORT}[pulls],
               switches=switches, mix_windows=mix_windows)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_trace(monkeypatch, name):
    got = run_case(monkeypatch, name)
    calls = {(entry[0], entry[1]) for entry in launches(got)}
    for expected in CASES[name][5]:
        assert tuple(expected) in calls, f"{name}: {expected[0]} on stream {expected[1]} does not occur"
    assert_matches(name, got, recorded(FIXTURE)[name])


def test_fixture_has_every_case_once():
    assert recorded_names(FIXTURE) == list(CASES)


if __name__ == "__main__":
    record_main(FIXTURE, CASES, run_case)
