"""CPU: the host side of MeltysynthPE against fixtures of the reference (tools/gen_golden_soundfont.py): the SF2 reader
against what the reference parsed, the control plane's render table against the one recorded from the reference for
every session -- every integer equal, every double bit for bit -- the block accounting of MeltysynthPE._render with the
device calls replaced, and the PE's surface."""

import struct

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, meltysynth_pe
from pygmu2_amd.soundfont import SoundFont, SoundFontError, Synthesizer, sf2

import soundfont_oracle as SO

CASES = SO.load_cases()
SESSIONS = CASES["sessions"]


@pytest.fixture(scope="module")
def data():
    return SO.load_data()


@pytest.fixture(scope="module")
def font():
    return SoundFont.from_file(SO.SF2_PATH)


@pytest.fixture(scope="module")
def blob():
    with open(SO.SF2_PATH, "rb") as f:
        return f.read()


# ---------------------------------------------------------------------------------------------- the reader
def test_reader_matches_what_the_reference_parsed(font):
    want = CASES["font"]
    assert len(font.wave) == want["wave_length"] and font.wave.dtype == np.int16
    assert list(font.info["version"]) == want["info"]["version"]
    assert font.info["bank_name"] == want["info"]["bank_name"]
    assert font.info["target_sound_engine"] == want["info"]["target_sound_engine"]
    assert len(font.sample_headers) == len(want["sample_headers"])
    for h, w in zip(font.sample_headers, want["sample_headers"]):
        assert {k: getattr(h, k) for k in w} == w
    assert [i.name for i in font.instruments] == [i["name"] for i in want["instruments"]]
    for inst, w in zip(font.instruments, want["instruments"]):
        assert len(inst.regions) == len(w["regions"])
        for region, wr in zip(inst.regions, w["regions"]):
            assert region.gs == wr["gs"] and region.sample is font.sample_headers[wr["sample"]]
    assert [(p.name, p.patch_number, p.bank_number) for p in font.presets] \
        == [(p["name"], p["patch_number"], p["bank_number"]) for p in want["presets"]]
    for preset, w in zip(font.presets, want["presets"]):
        assert len(preset.regions) == len(w["regions"])
        for region, wr in zip(preset.regions, w["regions"]):
            assert region.gs == wr["gs"] and region.instrument is font.instruments[wr["instrument"]]
    # the reference's float32 -> float64 sample values are s / 32768 exactly
    assert np.array_equal(font.wave_data, font.wave.astype(np.float32).astype(np.float64) / 32768.0)


def _patched(blob, old, new, count=1):
    assert blob.count(old) >= 1
    return blob.replace(old, new, count)


def test_malformed_files_raise(blob, tmp_path):
    bad = {
        "not riff": b"RIFX" + blob[4:],
        "not sfbk": blob[:8] + b"sfbx" + blob[12:],
        "truncated": blob[:len(blob) // 2],
        "truncated header": blob[:10],
        "unknown info id": _patched(blob, b"isng", b"isnx"),
        "no INFO list": _patched(blob, b"INFO", b"INFX"),
        "no sdta list": _patched(blob, b"sdta", b"sdtx"),
        "no smpl": _patched(blob, b"smpl", b"sm24"),
        "unknown pdta id": _patched(blob, b"ibag", b"ibax"),
        "missing shdr": _patched(blob, b"shdr", b"imod"),
        "empty": b"",
    }
    # a generator list whose size is no multiple of four, a sample id outside the headers
    at = blob.index(b"igen")
    size = struct.unpack("<I", blob[at + 4:at + 8])[0]
    gens = bytearray(blob)
    last_sample_id = at + 8 + size - 8                    # the last generator before the terminator: sampleID
    assert struct.unpack("<H", blob[last_sample_id:last_sample_id + 2])[0] == sf2.G_SAMPLE_ID
    gens[last_sample_id + 2:last_sample_id + 4] = struct.pack("<h", 7)
    bad["sample id"] = bytes(gens)
    kinds = bytearray(blob)
    kinds[last_sample_id:last_sample_id + 2] = struct.pack("<H", 61)
    bad["generator number"] = bytes(kinds)
    for name, raw in bad.items():
        with pytest.raises(SoundFontError):
            SoundFont(raw)
        assert issubclass(SoundFontError, ValueError), name
    path = tmp_path / "bad.sf2"
    path.write_bytes(bad["truncated"])
    with pytest.raises(SoundFontError):
        SoundFont.from_file(str(path))


# ---------------------------------------------------------------------------------------------- the control plane
class _Buffer:
    """Stands in for DeviceBuffer: an address and a shape, nothing behind them."""

    def __init__(self, shape, dtype=np.float32, zero=False):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.dtype, self.ptr = np.dtype(dtype), 1 << 20

    @classmethod
    def from_host(cls, array):
        return cls(np.asarray(array).shape, np.asarray(array).dtype)

    def offset_ptr(self, n):
        return self.ptr + int(n) * self.dtype.itemsize


class _Lib:
    def __init__(self):
        self.copies = []

    def pgx_memcpy_d2d(self, dst, src, nbytes):
        self.copies.append((dst, src, nbytes))
        return 0


class _Host:
    """MeltysynthPE with the device taken away: _render's block accounting runs as it is, _play records its table."""

    def __init__(self, monkeypatch, session, max_rows=None):
        pg.set_sample_rate(session["sr"])
        self.lib = _Lib()
        monkeypatch.setattr(meltysynth_pe, "DeviceBuffer", _Buffer)
        monkeypatch.setattr(meltysynth_pe, "new_output", lambda frames, ch: _Buffer((frames, ch)))
        monkeypatch.setattr(meltysynth_pe, "lib", lambda: self.lib)
        monkeypatch.setattr(meltysynth_pe, "Snippet", lambda start, out: (start, out))
        if max_rows is not None:
            monkeypatch.setattr(meltysynth_pe, "MAX_CHUNK_ROWS", max_rows)
        self.pe = pg.MeltysynthPE(SO.SF2_PATH, block_size=session["block_size"], program=session["program"])
        self.pe.maximum_polyphony = session["polyphony"]
        self.calls = []                                    # (frames, table) per entry call
        self.pe._play = lambda L, out_ptr, frames, block_rows, rows_i, rows_d, bs: \
            self.calls.append((out_ptr, frames, (np.array(block_rows), np.array(rows_i), np.array(rows_d))))
        self.pe.on_start()
        self.at = 0

    def render(self, frames):
        start, out = self.pe.render(self.at, frames)
        assert start == self.at and out.shape == (frames, 2)
        self.at += frames
        return out


@pytest.mark.parametrize("session", SESSIONS, ids=lambda s: s["name"])
def test_advance_emits_the_reference_s_table(session, data, monkeypatch):
    host = _Host(monkeypatch, session)
    _, active = SO.replay(session, host.pe.synthesizer, host.render)
    assert active == session["active"]
    got = SO.join_tables([table for _, _, table in host.calls])
    assert SO.table_difference(got, SO.session_table(data, session["name"])) is None
    assert got[1].dtype == np.int32 and got[2].dtype == np.float64 and got[1].shape[1] == device._ABI.constant(
        "PGX_SOUNDFONT_ICOLS") and got[2].shape[1] == device._ABI.constant("PGX_SOUNDFONT_DCOLS")


@pytest.mark.parametrize("name", ["odd_requests", "block8", "all_off"])
def test_block_accounting_serves_the_carry_first(name, monkeypatch):
    """Each request takes what the last block left over, then ceil(rest / block_size) new blocks; frames asked of the
    entry plus frames copied from the carry are the request; an event between two renders starts no block."""
    session = next(s for s in SESSIONS if s["name"] == name)
    host = _Host(monkeypatch, session)
    bs, carry, carry_at, blocks = session["block_size"], 0, 0, 0
    for step in session["steps"]:
        if step[0] != "render":
            before = len(host.calls)
            SO.replay({"steps": [step]}, host.pe.synthesizer, None)
            assert len(host.calls) == before                  # nothing is rendered by an event
            if step[1] == "reset":
                carry = 0
            continue
        calls, copies = len(host.calls), len(host.lib.copies)
        out = host.render(step[1])
        served = min(carry, step[1])
        new_blocks = -(-(step[1] - served) // bs)
        copied = host.lib.copies[copies:]
        assert [c[2] for c in copied] == ([served * 8] if served else [])
        if served:
            assert copied[0][0] == out.ptr and copied[0][1] == host.pe._carry.ptr + carry_at * 8
        asked = host.calls[calls:]
        assert sum(len(t[0]) - 1 for _, _, t in asked) == new_blocks
        assert sum(frames for _, frames, _ in asked) == step[1] - served
        if asked:
            assert asked[0][0] == out.ptr + served * 8
        carry_at = 0 if new_blocks else carry_at + served       # the entry leaves the new remainder at the carry's start
        carry = carry - served + new_blocks * bs - (step[1] - served)
        blocks += new_blocks
    assert blocks == session["blocks"]


def test_chunks_are_whole_blocks_within_the_row_limit(data, monkeypatch):
    session = next(s for s in SESSIONS if s["name"] == "stolen")
    whole = _Host(monkeypatch, session)
    SO.replay(session, whole.pe.synthesizer, whole.render)
    cut = _Host(monkeypatch, session, max_rows=12)
    SO.replay(session, cut.pe.synthesizer, cut.render)
    assert len(cut.calls) > len(whole.calls)
    for _, frames, (block_rows, rows_i, _) in cut.calls:
        assert block_rows[0] == 0 and block_rows[-1] == len(rows_i)
        assert len(rows_i) <= 12 or len(block_rows) == 2
    assert SO.table_difference(SO.join_tables([t for _, _, t in cut.calls]),
                               SO.session_table(data, "stolen")) is None
    assert meltysynth_pe.chunk_blocks(np.array([0, 5, 10, 30, 31]), 12) == [(0, 2), (2, 3), (3, 4)]


def test_synthesizer_facade(font):
    synth = Synthesizer(font, 44100)
    assert (synth.block_size, synth.maximum_polyphony, synth.channel_count, synth.percussion_channel,
            synth.sample_rate, synth.master_volume, synth.active_voice_count) == (64, 64, 16, 9, 44100, 0.5, 0)
    assert synth.sound_font is font
    synth.master_volume = 0.25
    assert synth.master_volume == 0.25
    synth.note_on(0, 45, 100)
    synth.note_on(16, 45, 100)                                 # no such channel: ignored
    synth.process_midi_message(-1, 0x90, 45, 100)
    assert synth.active_voice_count == 1
    synth.note_on(0, 45, 0)                                    # velocity 0 is a note off: the voice stays until it fades
    assert synth.active_voice_count == 1
    synth.note_off_all(True)
    assert synth.active_voice_count == 0
    block_rows, rows_i, rows_d = synth.advance(3)
    assert list(block_rows) == [0, 0, 0, 0] and rows_i.shape == (0, 8) and rows_d.shape == (0, 11)
    for bad in ({"sample_rate": 8000}, {"sample_rate": 44100, "block_size": 4},
                {"sample_rate": 44100, "block_size": 2048}, {"sample_rate": 44100, "maximum_polyphony": 4}):
        with pytest.raises(ValueError):
            Synthesizer(font, **bad)
    channel = synth.channels[9]
    assert channel.bank_number == 128 and synth.channels[0].bank_number == 0
    synth.process_midi_message(9, 0xB0, 0x00, 2)
    assert channel.bank_number == 130
    synth.process_midi_message(0, 0xB0, 0x65, 0)
    synth.process_midi_message(0, 0xB0, 0x64, 0)
    synth.process_midi_message(0, 0xB0, 0x06, 12)
    assert synth.channels[0].pitch_bend_range == 12.0
    synth.reset_all_controllers()
    synth.reset()
    assert synth.channels[0].pitch_bend_range == 2.0 and channel.bank_number == 128


# ---------------------------------------------------------------------------------------------- the PE's surface
def test_pe_surface(tmp_path):
    import os
    pe = pg.MeltysynthPE(SO.SF2_PATH)
    path = os.path.realpath(SO.SF2_PATH)
    assert repr(pe) == f"MeltysynthPE(soundfont_path={path!r}, block_size=64)"
    assert repr(pg.MeltysynthPE(SO.SF2_PATH, block_size=128, program=5)) \
        == f"MeltysynthPE(soundfont_path={path!r}, block_size=128, program=5)"
    assert pe.channel_count() == 2 and pe.is_pure() is False and pe.inputs() == []
    assert pe.extent().start is None and pe.extent().end is None
    assert pe.synthesizer is None
    assert not getattr(pe, "_READ_AHEAD_SAFE", False) and not getattr(pe, "_LOOK_AHEAD_SAFE", False)
    assert "MeltysynthPE" not in pg.__all__ and "soundfont" not in pg.__all__
    assert isinstance(pe, pg.SourcePE)
    assert "pgx_soundfont_render" in device.EXPORTED_SYMBOLS
    silence = pe.render(100, 16)
    assert silence.start == 100 and silence.data.shape == (16, 2) and not np.any(silence.data)
    with pytest.raises(FileNotFoundError):
        pg.MeltysynthPE(str(tmp_path / "missing.sf2")).on_start()
