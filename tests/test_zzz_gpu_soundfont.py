"""
GPU: MeltysynthPE and pgx_soundfont_render (csrc/pgx_soundfont.hip) against fixtures of the reference
(tools/gen_golden_soundfont.py), every comparison bit for bit.

Independent of the host's libm: the render table RECORDED from the reference goes to the entry and the result is
compared with the reference's samples; hand-made tables at the smallest shapes at which the kernel can go wrong are
compared with the numpy restatement tests/soundfont_oracle.AudioPlane, which the generator holds to the reference.
Every device buffer of those calls is made inside guarded_alloc.guarded(): guard bands around each, outputs poisoned,
inputs read back unchanged.

Then the PE: every session through pg.MeltysynthPE.  When such a comparison fails the assertion first says whether the
PE's own table differs from the recorded one: a differing table points at the host's libm (pow, exp, sin, cos, log10
round as they did where the fixtures were made: DESIGN.md section 6), not at the kernel.
"""

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device as dev
from pygmu2_amd import meltysynth_pe

import soundfont_oracle as SO
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

CASES = SO.load_cases()
SESSIONS = CASES["sessions"]
INVALID = dev.ERR_INVALID


@pytest.fixture(scope="module")
def data():
    return SO.load_data()


@pytest.fixture(scope="module")
def font_wave():
    return pg.soundfont.SoundFont.from_file(SO.SF2_PATH).wave


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def call_entry(samples, table, bs, polyphony, n_frames=None, state=None, expect=0, **override):
    """One pgx_soundfont_render under guards -> (out float32 (n_frames, 2), carry (bs, 2), filter state).  Outputs
    start as 0xFF bytes; every input is read back and must be unchanged."""
    block_rows, rows_i, rows_d = (np.ascontiguousarray(t) for t in table)
    n_blocks, n_rows = len(block_rows) - 1, len(rows_i)
    if n_frames is None:
        n_frames = n_blocks * bs
    if state is None:
        state = np.zeros((polyphony, 4))
    L = dev.ensure_init()
    with guarded():
        inputs = {"wave": np.ascontiguousarray(samples, dtype=np.int16), "block_rows": block_rows.astype(np.int32),
                  "rows_i": rows_i.astype(np.int32).reshape(-1, SO.ICOLS), "rows_d": rows_d.astype(np.float64)}
        bufs = {k: dev.DeviceBuffer.from_host(v) for k, v in inputs.items()}
        out = dev.DeviceBuffer((max(n_frames, 1), 2), np.float32)
        carry = dev.DeviceBuffer((max(bs, 1), 2), np.float32)
        filter_state = dev.DeviceBuffer.from_host(np.ascontiguousarray(state, dtype=np.float64))
        scratch = dev.DeviceBuffer((max(n_rows, 1) * max(bs, 1),), np.float64)
        args = {"out": out.ptr, "n_frames": n_frames, "carry": carry.ptr, "wave": bufs["wave"].ptr,
                "wave_len": len(samples), "block_rows": bufs["block_rows"].ptr, "rows_i": bufs["rows_i"].ptr,
                "rows_d": bufs["rows_d"].ptr, "n_rows": n_rows, "n_blocks": n_blocks, "block_size": bs,
                "filter_state": filter_state.ptr, "polyphony": polyphony, "scratch": scratch.ptr}
        args.update(override)
        rc = L.pgx_soundfont_render(*args.values())
        assert rc == expect, (rc, L.pgx_last_error())
        dev.synchronize()
        for k, v in inputs.items():
            assert _same(bufs[k].to_host().reshape(v.shape), v), f"the call wrote its input {k!r}"
        return out.to_host()[:n_frames], carry.to_host(), filter_state.to_host()


def check_table(wave, table, bs, polyphony, n_frames=None, state=None):
    """The entry against the restated audio plane: output, carry (the rest poisoned) and filter state, bit for bit."""
    plane = SO.AudioPlane(wave, bs, polyphony)
    if state is not None:
        plane.state[:] = state
    want = plane.render(*table).astype(np.float32)
    total = len(want)
    n = total if n_frames is None else n_frames
    out, carry, got_state = call_entry(wave, table, bs, polyphony, n, state)
    assert _same(out, want[:n]), f"{int(np.sum(_bits(out) != _bits(want[:n])))} samples differ"
    assert _same(carry[:total - n], want[n:])
    assert np.all(_bits(carry[total - n:]) == 0xFFFFFFFF), "the carry was written past the block's remainder"
    assert _same(got_state, plane.state)
    return out, got_state


# ---------------------------------------------------------------------------------------------- hand-made tables
RNG = np.random.default_rng(7)
WAVE = RNG.integers(-32768, 32767, 200).astype(np.int16)
LOWPASS = (0.02008336556421123, 0.04016673112842246, 0.02008336556421123, -1.5610180758007182, 0.6413515380575631)
RESONANT = (0.0036, 0.0072, 0.0036, -1.95, 0.9644)


def row(voice, position, ratio, *, end=150, loop=None, coefficients=None, clear=False, left=(SO.MIX_CONST, 0.4, 0.0),
        right=(SO.MIX_CONST, 0.3, 0.0)):
    flags = (SO.F_CLEAR if clear else 0) | (SO.F_LOOP if loop else 0) | (SO.F_FILTER if coefficients else 0)
    start_loop, end_loop = loop or (0, 0)
    return ([voice, flags, end, start_loop, end_loop, left[0], right[0], 0],
            [position, ratio] + list(coefficients or (0.0,) * 5) + list(left[1:]) + list(right[1:]))


def table_of(blocks):
    """[[row, ...] per block] -> (block_rows, rows_i, rows_d)."""
    offsets, ri, rd = [0], [], []
    for rows in blocks:
        for i, d in rows:
            ri.append(i)
            rd.append(d)
        offsets.append(len(ri))
    return (np.asarray(offsets, dtype=np.int32), np.asarray(ri, dtype=np.int32).reshape(-1, SO.ICOLS),
            np.asarray(rd, dtype=np.float64).reshape(-1, SO.DCOLS))


def slope(a, b, bs):
    return (SO.MIX_SLOPE, a, (b - a) / bs)


SKIP = (SO.MIX_SKIP, 0.0, 0.0)


def shapes(bs):
    loop = (40, 90)
    step = 0.731
    after = lambda k: 10.25 + k * bs * step                      # noqa: E731  (positions keep running, wrapped by the loop)
    return {
        "one_voice_one_block": [[row(0, 3.5, 0.37, coefficients=LOWPASS, clear=True)]],
        "one_voice_two_blocks": [[row(0, 3.5, 0.37, coefficients=LOWPASS, clear=True)],
                                 [row(0, 3.5 + bs * 0.37, 0.41, coefficients=RESONANT)]],
        "two_voices": [[row(0, after(0), step, loop=loop, coefficients=RESONANT, clear=True),
                        row(1, 5.0, 0.11, clear=True, left=slope(0.1, 0.6, bs), right=slope(0.5, 0.0, bs))],
                       [row(0, after(1), step, loop=loop, coefficients=LOWPASS),
                        row(1, 5.0 + bs * 0.11, 0.11, coefficients=LOWPASS)]],
        "nine_rows": [[row(v, 1.0 + v, 0.05 + 0.01 * v, loop=(20 + v, 60 + 2 * v), coefficients=LOWPASS if v % 2 else None,
                           clear=True, left=(SO.MIX_CONST, 0.05 * v, 0.0), right=slope(0.3, 0.02 * v, bs))
                       for v in (8, 0, 3, 5, 1, 7, 2, 6, 4)]] * 2,
        # voice 2 moves from row 2 to row 0 (a swap removal), voice 1 stays, voice 0 is gone; filter states follow the id
        "voice_changes_rows": [[row(0, 0.0, 0.5, coefficients=LOWPASS, clear=True),
                                row(1, 7.0, 0.25, loop=loop, coefficients=RESONANT, clear=True),
                                row(2, 9.0, 0.125, loop=loop, coefficients=LOWPASS, clear=True)],
                               [row(2, 9.0 + bs * 0.125, 0.125, loop=loop, coefficients=LOWPASS),
                                row(1, 7.0 + bs * 0.25, 0.25, loop=loop, coefficients=RESONANT)]],
        "clear_on_a_reused_voice": [[row(0, after(0), step, loop=loop, coefficients=RESONANT, clear=True)],
                                    [row(0, 12.0, 0.2, coefficients=RESONANT, clear=True)],
                                    [row(0, 12.0 + bs * 0.2, 0.2, coefficients=RESONANT)]],
        "inactive_then_active": [[row(0, after(0), step, loop=loop, clear=True)],
                                 [row(0, after(1), step, loop=loop, coefficients=RESONANT)]],
        # a no-loop voice whose sample runs out at frame 0, 1 and block_size - 1 of the block
        "ends_at_0": [[row(0, 150.0, 1.0, end=150, coefficients=LOWPASS)]],
        "ends_at_1": [[row(0, 149.5, 1.0, end=150, coefficients=LOWPASS)]],
        "ends_at_last": [[row(0, 150.0 - (bs - 1) * 0.125, 0.125, end=150, coefficients=LOWPASS)]],
        "loop_of_length_1_from_below": [[row(0, 10.25, 1.5, loop=(50, 51), coefficients=LOWPASS)]],
        "position_below_start_loop": [[row(0, 3.25, 0.2, loop=(60, 75))]],
        "hi_at_end_loop": [[row(0, 58.5, 0.5, loop=(50, 60))]],
        "last_wave_frame": [[row(0, 197.0, 0.25, end=260), row(1, 190.5, 1.0, loop=(180, 230)),
                             row(2, 195.0, 1.0, end=100000, left=slope(0.0, 1.0, bs))]],
        "mix_modes": [[row(0, 1.0, 0.3, left=SKIP, right=(SO.MIX_CONST, 0.7, 0.0)),
                       row(1, 2.0, 0.2, left=(SO.MIX_CONST, 0.2, 0.0), right=slope(0.0, 0.9, bs)),
                       row(2, 3.0, 0.1, left=slope(0.8, 0.1, bs), right=SKIP)]],
        "all_skipped": [[row(0, 1.0, 0.3, left=SKIP, right=SKIP), row(1, 2.0, 0.3, left=SKIP, right=SKIP)], []],
    }


BLOCK_SIZES = (8, 64, 1024)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("shape", sorted(shapes(64)))
def test_hand_made_tables(shape, bs):
    table = table_of(shapes(bs)[shape])
    out, _ = check_table(WAVE, table, bs, polyphony=16)
    if shape == "all_skipped" or shape == "ends_at_0":
        assert not np.any(_bits(out)), "exactly +0.0 is expected"
    else:
        assert np.any(out != 0.0)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_fewer_frames_than_the_last_block_holds(bs):
    table = table_of(shapes(bs)["two_voices"])
    for n_frames in (2 * bs, 2 * bs - 1, bs + 1, bs):
        check_table(WAVE, table, bs, polyphony=8, n_frames=n_frames)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_filter_state_is_carried_across_calls(bs):
    blocks = shapes(bs)["voice_changes_rows"]
    whole, state_whole = check_table(WAVE, table_of(blocks), bs, polyphony=8)
    first, state = check_table(WAVE, table_of(blocks[:1]), bs, polyphony=8)
    assert np.any(state[:3] != 0.0)
    second, state_two = check_table(WAVE, table_of(blocks[1:]), bs, polyphony=8, state=state)
    assert _same(np.concatenate([first, second]), whole) and _same(state_two, state_whole)


def test_no_blocks_is_ok_and_writes_nothing():
    out, carry, state = call_entry(WAVE, table_of([]), 64, 8, n_frames=0)
    assert np.all(_bits(carry) == 0xFFFFFFFF) and not np.any(state)


def test_bad_arguments_are_refused_and_nothing_is_written():
    good = table_of(shapes(64)["two_voices"])

    def refused(table=good, bs=64, polyphony=8, n_frames=None, **override):
        n = 128 if n_frames is None else n_frames
        state = np.full((max(polyphony, 1), 4), 0.5)
        out, carry, got = call_entry(WAVE, table, bs, polyphony, n, state, expect=INVALID, **override)
        assert np.all(_bits(out) == 0xFFFFFFFF) and np.all(_bits(carry) == 0xFFFFFFFF) and _same(got, state)

    for name in ("out", "carry", "wave", "block_rows", "rows_i", "rows_d", "filter_state", "scratch"):
        refused(**{name: None})
    refused(block_size=7)
    refused(block_size=1025)
    refused(n_rows=-1)
    refused(n_blocks=-1)
    refused(wave_len=-1)
    refused(n_frames=129)
    refused(n_frames=63)
    refused(polyphony=0)
    refused(polyphony=257)
    block_rows, rows_i, rows_d = good
    for column, value in ((SO.I_VOICE, 8), (SO.I_VOICE, -1), (SO.I_VOICE, 1), (SO.I_MIX_L, 3), (SO.I_MIX_R, -1)):
        bad = rows_i.copy()
        bad[0, column] = value                         # voice 1 in row 0: twice in block 0
        refused((block_rows, bad, rows_d))
    refused((np.array([0, 3, 4], dtype=np.int32), rows_i, rows_d))          # 3 rows, then 1
    refused((np.array([0, 2, 3], dtype=np.int32), rows_i, rows_d))          # does not span the rows
    refused((np.array([1, 2, 4], dtype=np.int32), rows_i, rows_d))
    refused((np.array([0, 3, 2], dtype=np.int32), rows_i, rows_d), n_rows=2)


# ---------------------------------------------------------------------------------------------- the reference's tables
@pytest.mark.parametrize("session", SESSIONS, ids=lambda s: s["name"])
def test_recorded_table_renders_the_reference_s_samples(session, data, font_wave):
    table = SO.session_table(data, session["name"])
    blocks, _, _ = call_entry(font_wave, table, session["block_size"], session["polyphony"])
    got = SO.requests_over_blocks(session, blocks)
    want = data[f"{session['name']}/samples"]
    assert _same(got, want), f"{int(np.sum(_bits(got) != _bits(want)))} of {want.size} samples differ"


# ---------------------------------------------------------------------------------------------- the PE
class Stream:
    def __init__(self, session, pull=None):
        pg.set_sample_rate(session["sr"])
        self.pe = pg.MeltysynthPE(SO.SF2_PATH, block_size=session["block_size"], program=session["program"])
        self.pe.maximum_polyphony = session["polyphony"]
        self.pe.table_log = []
        self.pe.on_start()
        self.at, self.pull, self.requests = 0, pull, 0

    def render(self, frames):
        """`frames` frames, in one request or cut by the `pull` sizes in turn."""
        got, left = [np.zeros((0, 2), np.float32)], frames
        while left:
            n = left if self.pull is None else min(left, self.pull[self.requests % len(self.pull)])
            self.requests += 1
            snippet = self.pe.render(self.at, n)
            assert snippet.start == self.at and snippet.data.shape == (n, 2)
            got.append(np.array(snippet.data))
            self.at, left = self.at + n, left - n
        return np.concatenate(got)

    def play(self, session):
        pieces, active = SO.replay(session, self.pe.synthesizer, self.render)
        self.pe.on_stop()
        assert self.pe.synthesizer is None
        return np.concatenate(pieces), active


def assert_stream(session, data, got, tables):
    want = data[f"{session['name']}/samples"]
    if not _same(got, want):
        difference = SO.table_difference(SO.join_tables(tables), SO.session_table(data, session["name"]))
        where = "the PE's table is the recorded one: the kernel differs" if difference is None else \
            f"the PE's own table differs from the recorded one (the host's libm?): {difference}"
        raise AssertionError(f"{session['name']}: {int(np.sum(_bits(got) != _bits(want)))} of {want.size} samples "
                             f"differ; {where}")


@pytest.mark.parametrize("session", SESSIONS, ids=lambda s: s["name"])
def test_pe_renders_the_reference_s_samples(session, data):
    stream = Stream(session)
    got, active = stream.play(session)
    assert_stream(session, data, got, stream.pe.table_log)
    assert active == session["active"]


@pytest.mark.parametrize("name", ["held_released", "controllers", "block8", "block1024"])
def test_request_sizes_do_not_change_the_stream(name, data):
    session = next(s for s in SESSIONS if s["name"] == name)
    stream = Stream(session, pull=(1, 63, 64, 65, 1000))
    got, _ = stream.play(session)
    assert_stream(session, data, got, stream.pe.table_log)


def test_small_chunks_do_not_change_the_stream(data, monkeypatch):
    session = next(s for s in SESSIONS if s["name"] == "stolen")
    monkeypatch.setattr(meltysynth_pe, "MAX_CHUNK_ROWS", 5)
    L = dev.ensure_init()
    entry, calls = L.pgx_soundfont_render, []
    monkeypatch.setattr(L, "pgx_soundfont_render", lambda *a: calls.append(a) or entry(*a))
    stream = Stream(session)
    got, _ = stream.play(session)
    assert_stream(session, data, got, stream.pe.table_log)
    expected = sum(len(meltysynth_pe.chunk_blocks(t[0], 5)) for t in stream.pe.table_log)
    assert len(calls) == expected > len(stream.pe.table_log)
    assert max(a[8] for a in calls) <= 8                   # rows per call: a single block may exceed the limit, not two


def test_graph_hears_an_event_from_the_next_block_on(data):
    """GainPE(MeltysynthPE, 0.5) under a NullRenderer in 64-frame blocks, a note_on between blocks: neither read-ahead
    nor look-ahead may have rendered past the event."""
    session = next(s for s in SESSIONS if s["name"] == "graph")
    pg.set_sample_rate(session["sr"])
    synth_pe = pg.MeltysynthPE(SO.SF2_PATH)
    renderer = pg.NullRenderer(sample_rate=session["sr"])
    renderer.set_source(pg.GainPE(synth_pe, 0.5))
    renderer.start()
    state = {"at": 0}

    def block(frames):
        renderer.render(state["at"], frames)
        state["at"] += frames
        return np.array(renderer.last_snippet.data)

    pieces, _ = SO.replay(session, synth_pe.synthesizer, block)
    renderer.stop()
    want = data["graph/samples"] * np.float32(0.5)
    assert _same(np.concatenate(pieces), want)
    assert np.any(want[:192] != 0)
