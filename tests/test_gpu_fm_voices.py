"""GPU: a MixPE of modulated-sine voices -- SinePE with a PE-valued frequency, amplitude or phase: FM, AM, PM -- is rendered
as a voice bank (voice_bank._SineModNode: the modulators as batched levels, then ONE pgx_sine_stateful_bank) and gives, bit
for bit, what a twin graph rendered voice by voice (`mix._bank = False`) gives.  Graphs: tests/fm_cases.py, five voices
each -- `fm`, `am_pm` (a phase in play), `nested` (the modulator is itself an FM voice), `bell` (the bank under GainPE with
an AdsrTriggeredPE envelope).  Pull script (tests/test_gpu_panned_voices.py's): contiguous blocks of 1 024 and of 3 077
frames, a seek back -- which continues the phase, in the PE and in the bank --, renderer stop + start -- which clears it.
Look-ahead is off on both sides of a bit-for-bit comparison: a window is another cut of the stream, and the phase of a frame
is ((carry + offset) + local) + initial, another association per cut.  With everything at its defaults the two paths are
held to fixture_harness.PEAK_BOUND.  Both plans of the entry are reached through the node at blocks of 6 149 frames (three
tiles and a ragged fourth) by moving SINE_MOD_WALK_MIN_ROWS.  Windows at the level of the mix hand out the bank's own
block-by-block samples within PEAK_BOUND; a bank with a phase in play opens none.  The banked render of the fixture cases
is held to the reference's samples (tests/golden/fm_voices*, tools/gen_golden_fm_voices.py) by the per-block rule of graphs
with oscillators.  The measured minimums are set to MIN_VOICES."""

import numpy as np
import pytest

import fm_cases
import pygmu2_amd as pg
import spec_build
from fixture_harness import PEAK_BOUND, assert_bits, assert_peak, check_case, load_cases
from guarded_alloc import guarded
from pygmu2_amd import look_ahead, voice_bank

pytestmark = pytest.mark.gpu

SR = fm_cases.SR
# contiguous blocks of 1 024 and of 3 077 frames, a seek back, (stop + start in front of block 6,) two more
PULLS = [(0, 1024), (1024, 1024), (2048, 3077), (5125, 3077), (1024, 1024), (2048, 1024), (0, 3077), (3077, 1024)]
RESTART_AT = 6
LONG_PULLS = [(0, 6149), (6149, 6149), (12298, 6149), (6149, 6149)]
DOC, NPZ = load_cases("fm_voices")


@pytest.fixture
def small_banks(monkeypatch):
    for name in ("SINE_MOD_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES"):
        monkeypatch.setattr(voice_bank, name, voice_bank.MIN_VOICES)


@pytest.fixture
def block_by_block():
    """No look-ahead windows on either path."""
    was = look_ahead.enabled()
    look_ahead.set_enabled(False)
    yield
    look_ahead.set_enabled(was)


def _render(spec, bank, pulls=PULLS, restart_at=RESTART_AT):
    """-> (the blocks of the pull script, the MixPE)."""
    pg.set_sample_rate(SR)
    mix = spec_build.build(spec)
    if not bank:
        mix._bank = False
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(mix)
    r.start()
    out = []
    for k, (start, n) in enumerate(pulls):
        if k == restart_at:
            r.stop()
            r.start()
        out.append(np.array(mix.render(start, n).data, dtype=np.float32))
    r.stop()
    return out, mix


def _sine_mod_nodes(bank):
    return [node for node in bank._nodes() if type(node) is voice_bank._SineModNode]


def _twins(kind, pulls=PULLS, restart_at=RESTART_AT):
    """-> (the bank's blocks, the twin's blocks), the bank and its root asserted."""
    spec = fm_cases.mix(kind)
    with guarded():
        got, mix = _render(spec, True, pulls, restart_at)
        bank = mix._bank
        assert isinstance(bank, voice_bank.VoiceBank) and bank.k == fm_cases.K
        assert type(bank.root).__name__ == fm_cases.ROOTS[kind]
        assert len(_sine_mod_nodes(bank)) == (2 if kind == "nested" else 1)
        want, plain = _render(spec, False, pulls, restart_at)
        assert plain._bank is False
    for k, b in enumerate(want):
        assert b.shape == (pulls[k][1], 1) and np.all(np.isfinite(b)) and np.any(b), f"{kind} block {k}"
    return got, want


@pytest.mark.usefixtures("small_banks", "block_by_block")
@pytest.mark.parametrize("kind", fm_cases.KINDS)
def test_bank_equals_the_voices_one_by_one(kind):
    got, want = _twins(kind)
    for k, (a, b) in enumerate(zip(got, want)):
        assert_bits(f"{kind} block {k}", a, b)
    # the seek back continued the phase: block 4 covers the frames of block 1 and is not block 1 again
    assert not np.array_equal(want[4], want[1])
    # stop + start cleared it: block 6 starts at frame 0 as block 0 did
    assert np.array_equal(want[6][:1024], want[0])


@pytest.mark.usefixtures("small_banks", "block_by_block")
@pytest.mark.parametrize("walk_min_rows", [1, 1 << 30], ids=["walk", "time-parallel"])
@pytest.mark.parametrize("kind", ["fm", "am_pm"])
def test_both_plans_through_the_node(monkeypatch, kind, walk_min_rows):
    monkeypatch.setattr(voice_bank, "SINE_MOD_WALK_MIN_ROWS", walk_min_rows)
    got, want = _twins(kind, LONG_PULLS, restart_at=None)
    for k, (a, b) in enumerate(zip(got, want)):
        assert_bits(f"{kind} block {k}", a, b)


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("kind", fm_cases.KINDS)
def test_bank_at_the_defaults(kind):
    got, want = _twins(kind)
    assert_peak(f"{kind}, defaults", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "FM_DEFAULT")


@pytest.mark.usefixtures("small_banks")
def test_windows_of_the_mix_hand_out_the_block_by_block_samples():
    """The existing window rule of a rank's share of a sharded mix (VoiceBank.set_mix_windows) over an fm bank: a stream of
    4 096-frame blocks is rendered 2, then 4 blocks at a time, a seek leaves the window of 4 half consumed -- the states go
    back to the window's start (the node's `state`, by _STATE) and the consumed part is rendered again -- and the stream
    continues from the carried phase.  A window is another cut: held to PEAK_BOUND, not to the bit."""
    pulls = [(4096 * i, 4096) for i in range(5)] + [(4096, 4096), (8192, 4096)]
    spec = fm_cases.mix("fm")
    windows = []

    def pull(mix_windows):
        pg.set_sample_rate(SR)
        mix = spec_build.build(spec)
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(mix)
        r.start()
        assert mix._voice_bank()
        if mix_windows:
            mix._bank.set_mix_windows()
        out = []
        for start, n in pulls:
            out.append(np.array(mix.render(start, n).data, dtype=np.float32))
            if mix_windows:
                windows.append(mix._bank.win is not None)
        r.stop()
        assert not mix._bank.request_dependent
        return out

    with guarded():
        got = pull(True)
        want = pull(False)
    assert windows == [False, True, True, True, True, False, True], windows         # 2, 4, the seek, 2 again
    for k, (a, b) in enumerate(zip(got, want)):
        assert b.shape == (4096, 1) and np.any(b)
        assert_peak(f"fm block {k}", a, b, PEAK_BOUND, "FM_WINDOWS")
    assert not np.array_equal(want[5], want[1])                   # (the phase went on through the seek)


@pytest.mark.usefixtures("small_banks")
def test_a_bank_with_a_phase_in_play_opens_no_window():
    pulls = [(4096 * i, 4096) for i in range(5)] + [(4096, 4096), (8192, 4096)]
    with guarded():
        pg.set_sample_rate(SR)
        mix = spec_build.build(fm_cases.mix("am_pm"))
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(mix)
        r.start()
        assert mix._voice_bank()
        bank = mix._bank
        bank.set_mix_windows()
        assert bank.request_dependent
        for start, n in pulls:
            block = np.array(mix.render(start, n).data, dtype=np.float32)
            assert block.shape == (4096, 1) and np.any(block)
            assert mix._bank is bank and bank.win is None
        r.stop()


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("case", DOC["cases"], ids=[c["name"] for c in DOC["cases"]])
def test_bank_matches_the_reference(case):
    assert case["compare"] == "fuzz"
    built = []

    def build(case):
        pe, made = spec_build.build_case(case, ())
        built.append(pe)
        return pe, made

    with guarded():
        check_case(case, NPZ, build, tag="FM_VOICES_ERR")
    bank = built[0]._bank
    assert isinstance(bank, voice_bank.VoiceBank) and bank.k == fm_cases.K and _sine_mod_nodes(bank)
