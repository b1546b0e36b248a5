"""
CPU: what a bank of NoisePE voices, of hi-hat voices and of voices swept by a FunctionGenPE launches -- pinned against a
recorded trace, with the stand-ins of tests/bank_trace.py (its Recorder, Library and buffers: no device).

Graphs, five voices each, the measured minimums set to 4:
    pink    NoisePE(seed=i, mode=PINK)
    hihat   GainPE(SVFilterPE(NoisePE(seed=i), f_i, 2, HIGHPASS), gain=AdsrTriggeredPE(PeriodicTrigger))
    swept   BiquadPE(BlitSawPE(f_i), frequency=TransformPE(FunctionGenPE(0.5, 0.5, sawtooth), Affine(2000, 2500)), q=2)
Pull scripts: BLOCKS -- four contiguous pulls of 1 024 frames, then a seek back to frame 1 024; WINDOWS -- the same with
4 096 frames and windows at the level of the mix (a window of 2 blocks used up, a window of 4 left after its first block).

Pinned beside the recorded launches: every rendered block or window is exactly ONE pgx_noise_* / pgx_function_gen_bank
call with batch = 5 and a row stride of its frames; `draws` of each noise call is the frames rendered so far -- and after
the seek the frames CONSUMED so far (the window's unconsumed half is drawn again) --; nothing is uploaded after the bank
was built.

    python tests/test_noise_bank_trace.py --record        writes tests/golden/noise_bank_trace.json
"""

import os

import pytest

from bank_trace import assert_matches, install, record_main, recorded, recorded_names, run

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_bank_trace.json")
K = 5
MINIMUMS = ("NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES", "BIQUAD_VAR_MIN_VOICES")


def script(block):
    return [(i * block, block) for i in range(4)] + [(block, block)]


SCRIPTS = {"blocks": (script(1024), False), "windows": (script(4096), True)}
CASES = [f"{kind}-{pulls}" for kind in ("pink", "hihat", "swept") for pulls in SCRIPTS]


def voices(pg, kind):
    from pygmu2_amd.biquad_pe import BiquadMode
    from pygmu2_amd.transforms import Affine
    if kind == "pink":
        return [pg.NoisePE(seed=i, mode=pg.NoiseMode.PINK) for i in range(K)]
    if kind == "hihat":
        return [pg.GainPE(pg.SVFilterPE(pg.NoisePE(seed=i), 6000.0 + 100.0 * i, 2.0, BiquadMode.HIGHPASS),
                          gain=pg.AdsrTriggeredPE(pg.PeriodicTrigger(4.0 + 0.25 * i), 0.001, 0.02, 0.03, 0.3, 0.05))
                for i in range(K)]
    if kind == "swept":
        return [pg.BiquadPE(pg.BlitSawPE(110.0 * 2 ** (i / 12.0)),
                            frequency=pg.TransformPE(pg.FunctionGenPE(0.5 + 0.1 * i, 0.5, waveform="sawtooth"),
                                                     func=Affine(2000.0, 2500.0)), q=2.0) for i in range(K)]
    raise KeyError(kind)


def run_case(monkeypatch, name):
    """-> the canonical trace of case `name`."""
    import pygmu2_amd as pg
    kind, pulls = name.split("-")
    pulls, mix_windows = SCRIPTS[pulls]
    return run(monkeypatch, lambda: voices(pg, kind), pulls, switches={minimum: 4 for minimum in MINIMUMS},
               mix_windows=mix_windows)


def _renders(trace, entry_names):
    """[(frames asked for by the pull in front, the call)] of every call of `entry_names`."""
    found, pull = [], None
    for entry in trace:
        if entry[0] == "pull":
            pull = entry
        elif entry[0] in entry_names:
            found.append((pull, entry))
    return found


@pytest.mark.parametrize("name", CASES)
def test_launch_trace(monkeypatch, name):
    assert_matches(name, run_case(monkeypatch, name), recorded(FIXTURE)[name])


@pytest.mark.parametrize("pulls", list(SCRIPTS))
@pytest.mark.parametrize("kind", ["pink", "hihat"])
def test_one_noise_call_per_rendered_block_or_window(monkeypatch, kind, pulls):
    """[name, stream, out, out_stride, batch, n, draws, params(, state)]"""
    trace = run_case(monkeypatch, f"{kind}-{pulls}")
    entry = "pgx_noise_pink" if kind == "pink" else "pgx_noise_white"
    calls = _renders(trace, ("pgx_noise_white", "pgx_noise_pink", "pgx_noise_brown"))
    assert calls and all(call[0] == entry for _, call in calls)
    block = SCRIPTS[pulls][0][0][1]
    if pulls == "blocks":
        # five pulls, five renders; `start` is ignored: the seek back continues the stream
        want = [(block, 0), (block, block), (block, 2 * block), (block, 3 * block), (block, 4 * block)]
    else:
        # window of 2 at the second pull (the first streaming one), window of 4 at the fourth; the seek back finds that
        # window half consumed: the states go back to its start (3 blocks in) and the consumed block is drawn again,
        # then the block asked for
        want = [(block, 0), (2 * block, block), (4 * block, 3 * block), (block, 3 * block), (block, 4 * block)]
    assert [(call[5], call[6]) for _, call in calls] == want
    for _, call in calls:
        assert call[4] == K and call[3] == call[5]             # batch, out_stride = n
    pulls_seen = [e for e in trace if e[0] == "pull"]
    assert len(pulls_seen) == 5
    # draws after the last render: the frames consumed (five blocks), whatever was rendered ahead in between
    assert calls[-1][1][6] + calls[-1][1][5] == 5 * block


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_one_function_gen_call_per_rendered_block_or_window(monkeypatch, pulls):
    """[name, stream, out, out_stride, batch, start, n, channels, sawtooth, params]"""
    trace = run_case(monkeypatch, f"swept-{pulls}")
    calls = _renders(trace, ("pgx_function_gen_bank",))
    assert not _renders(trace, ("pgx_function_gen_pure", "pgx_function_gen_stateful"))
    block = SCRIPTS[pulls][0][0][1]
    if pulls == "blocks":
        want = [(0, block), (block, block), (2 * block, block), (3 * block, block), (block, block)]
    else:
        want = [(0, block), (block, 2 * block), (3 * block, 4 * block), (3 * block, block), (block, block)]
    assert [(call[5], call[6]) for _, call in calls] == want
    for _, call in calls:
        assert call[4] == K and call[3] == call[6] and call[7] == 1 and call[8] == 1
    params = {call[9] for _, call in calls}
    assert len(params) == 1                                    # one upload, made when the bank was built


@pytest.mark.parametrize("name", CASES)
def test_nothing_is_uploaded_per_block(monkeypatch, name):
    """The parameter records go up when the bank is built.  (A BlitSawPE bank uploads its initial states where a render does
    not continue the last one -- the first pull and the seek of `swept` --: blit_saw_pe.py's reset rule, not a block's.)"""
    trace = run_case(monkeypatch, name)
    at = [i for i, e in enumerate(trace) if e[0] == "pull"]
    assert any(e[0] == "h2d" for e in trace[:at[0]])
    streamed = trace[at[1]:at[4]] if name.startswith("swept") else trace[at[0]:]
    assert not [e for e in streamed if e[0] == "h2d"]


def test_advance_and_reset_state_of_one_voice_reach_its_record(monkeypatch):
    """NoisePE.advance(d) on voice 2: one upload, no launch; the next render draws with the same `draws` (the skip is in
    the voice's `consumed`).  reset_state() on voice 3: applied by the next render -- one record upload, one 32-byte
    memset of its taps."""
    import pygmu2_amd as pg
    from pygmu2_amd import config, voice_bank
    rec = install(monkeypatch)
    monkeypatch.setattr(voice_bank, "NOISE_MIN_VOICES", 4)
    monkeypatch.setattr(config, "_sample_rate", 48000)
    pes = voices(pg, "pink")
    bank = voice_bank.try_build_bank(pes)
    node = bank.root
    assert [pe._bank_node() for pe in pes] == [node] * K and [pe._bank_slot[1] for pe in pes] == list(range(K))
    bank.render_mix(0, 1024)
    before = len(rec.entries)
    pes[2].advance(1000)
    assert [e[0] for e in rec.entries[before:] if e[0] != "free"] == ["h2d"]
    assert [int(c) for c in node.rec["consumed"]] == [0, 0, 1000, 0, 0] and node.draws == 1024
    pes[3].reset_state()
    assert node.pending == {3}
    before = len(rec.entries)
    bank.render_mix(1024, 1024)
    names = [e[0] for e in rec.entries[before:] if e[0] != "free"]
    assert names == ["pgx_memset", "h2d", "pgx_noise_pink", "pgx_mix_batch"]
    assert [int(c) for c in node.rec["consumed"]] == [0, 0, 1000, -1024, 0] and not node.pending
    call = next(e for e in rec.entries[before:] if e[0] == "pgx_noise_pink")
    assert call[6] == 1024 and node.draws == 2048
    # every voice reset: the whole bank starts over (what renderer stop / start does)
    for pe in pes:
        pe.reset_state()
    bank.render_mix(2048, 1024)
    assert node.draws == 1024 and not np_any(node.rec["consumed"])


def test_a_reset_of_one_voice_goes_into_the_snapshot_of_the_window_it_opens(monkeypatch):
    """reset_state() on voice 3, then the pull that applies it opens a window, then a seek inside that window: the states go
    back to the window's start -- AFTER the reset.  So the reset (a memset of the voice's taps, the upload of the records)
    comes in front of the snapshot's copies, the copy of the records reads the uploaded buffer, and the part rendered again
    is drawn from records that are the host's."""
    import pygmu2_amd as pg
    from pygmu2_amd import config, voice_bank
    rec = install(monkeypatch)
    monkeypatch.setattr(voice_bank, "NOISE_MIN_VOICES", 4)
    monkeypatch.setattr(config, "_sample_rate", 48000)
    pes = voices(pg, "pink")
    bank = voice_bank.try_build_bank(pes)
    bank.set_mix_windows()
    node = bank.root
    for i in range(3):                                   # a block, then a window of 2 used up
        bank.render_mix(4096 * i, 4096)
    pes[3].reset_state()
    assert node.pending == {3} and node.draws == 3 * 4096
    before = len(rec.entries)
    bank.render_mix(3 * 4096, 4096)                      # applies the reset, opens a window of 4
    assert bank.win is not None and not node.pending
    opened = [e for e in rec.entries[before:] if e[0] != "free"]
    names = [e[0] for e in opened]
    assert names == ["pgx_memset", "h2d", "pgx_memcpy_d2d", "pgx_memcpy_d2d", "pgx_noise_pink", "pgx_mix_batch"]
    uploaded = opened[1][2]
    assert uploaded in [e[3] for e in opened[2:4]]       # [name, stream, dst, src, bytes]: the snapshot copies the NEW records
    call = opened[4]
    assert call[7] == uploaded and (call[5], call[6]) == (4 * 4096, 3 * 4096)
    assert [int(c) for c in node.rec["consumed"]] == [0, 0, 0, -3 * 4096, 0]
    bank.render_mix(4 * 4096, 4096)
    before = len(rec.entries)
    bank.render_mix(4096, 4096)                          # a seek: two of the window's four blocks were consumed
    again = [e for e in rec.entries[before:] if e[0] in ("pgx_noise_pink", "h2d", "pgx_memset")]
    assert [(e[0], e[5], e[6]) for e in again] == [("pgx_noise_pink", 2 * 4096, 3 * 4096), ("pgx_noise_pink", 4096, 5 * 4096)]
    assert all(e[7] == uploaded for e in again)          # the buffer the restored (post-reset) records were copied into
    assert node.draws == 6 * 4096 and [int(c) for c in node.rec["consumed"]] == [0, 0, 0, -3 * 4096, 0]


def np_any(values):
    return any(int(v) for v in values)


def test_fixture_has_every_case_once():
    assert recorded_names(FIXTURE) == CASES


if __name__ == "__main__":
    record_main(FIXTURE, CASES, run_case)
