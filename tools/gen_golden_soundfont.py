"""
Fixtures for MeltysynthPE: write a tiny SoundFont with this file's own writer (tests/golden/soundfont_tiny.sf2), load
it in the reference's meltysynth port, play the scripted sessions below through the reference's Synthesizer and write
tests/golden/soundfont_cases.json + tests/golden/soundfont.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_soundfont.py
The json holds what the reference parsed (presets, instruments, every generator of every region, sample headers, wave
length) and the sessions: sample rate, block size, polyphony, and "steps" -- ["ev", method, args], ["set", attribute,
value] or ["render", frames] -- with the active voice count after every render.  The npz holds data only: per session
"<name>/samples" (the float32 of the reference's stereo output, the requests end to end) and the reference's render
table "<name>/block_rows", "<name>/rows_i", "<name>/rows_d" (include/pygmu_hip.h lays it out), recorded by wrapping
Oscillator.fill_block, BiQuadFilter.process / clear_buffer and Synthesizer._write_block / _render_block in this process.

Checked while generating, on the reference alone (the tool stops at the first that fails):
  * tests/soundfont_oracle.AudioPlane, fed with the recorded table, reproduces every session's samples bit for bit;
  * every session has a block with two or more audible voices;
  * every instrument zone and every preset zone of the file is struck by some session;
  * all three mix modes, an inactive filter, a clear flag on a reused voice, a swap removal and a stolen voice occur.
"""

from __future__ import annotations

import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
import soundfont_oracle as SO                                     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# generator numbers used by the writer
(START_LOOP_OFS, VIB_PITCH, MODENV_PITCH, CUTOFF, Q, MODLFO_CUTOFF, MODENV_CUTOFF, MODLFO_VOLUME, PAN, MODLFO_FREQ,
 VIBLFO_FREQ, MODENV_ATTACK, MODENV_DECAY, MODENV_SUSTAIN, VOL_ATTACK, VOL_DECAY, VOL_SUSTAIN, VOL_RELEASE, INSTRUMENT,
 KEY_RANGE, ATTENUATION, COARSE_TUNE, FINE_TUNE, SAMPLE_ID, SAMPLE_MODES, EXCLUSIVE_CLASS, ROOT_KEY) = (
    2, 6, 7, 8, 9, 10, 11, 13, 17, 22, 24, 26, 28, 29, 34, 36, 37, 38, 41, 43, 48, 51, 52, 53, 54, 57, 58)


def key_range(lo, hi):
    return (KEY_RANGE, lo | (hi << 8))


# ---------------------------------------------------------------------------------------------- the SF2 writer
def chunk(tag, body):
    return tag.encode() + struct.pack("<I", len(body)) + body + (b"\0" if len(body) % 2 else b"")


def name20(text):
    return text.encode("ascii")[:19].ljust(20, b"\0")


def bags_and_generators(zone_lists):
    """[[zone, ...] per owner], a zone a list of (generator, value) -> (first bag index per owner + terminal, bag bytes,
    generator bytes)."""
    firsts, bags, gens, n_gens = [], [], b"", 0
    for zones in zone_lists:
        firsts.append(len(bags))
        for zone in zones:
            bags.append(n_gens)
            for kind, value in zone:
                gens += struct.pack("<Hh", kind, value if value < 32768 else value - 65536)
                n_gens += 1
    firsts.append(len(bags))
    bags.append(n_gens)
    gens += struct.pack("<Hh", 0, 0)
    return firsts, b"".join(struct.pack("<HH", b, 0) for b in bags), gens


def build_sf2():
    rng = np.random.default_rng(20261021)
    t = np.arange(600)
    tone = np.round(26000 * np.sin(2 * np.pi * t / 50.0) * np.exp(-t / 900.0)).astype("<i2")    # 12 periods, loopable
    burst = np.round(20000 * rng.uniform(-1, 1, 300) * np.exp(-np.arange(300) / 120.0)).astype("<i2")
    pad = np.zeros(46, dtype="<i2")
    smpl = np.concatenate([tone, pad, burst, pad])
    tone_at, burst_at = 0, 646
    # name, start, end, start_loop, end_loop, rate, pitch, correction, link, type
    headers = [("tone", tone_at, tone_at + 600, tone_at + 300, tone_at + 500, 22050, 60, 0, 0, 1),
               ("burst", burst_at, burst_at + 300, burst_at + 8, burst_at + 292, 44100, 48, -7, 0, 1),
               ("EOS", 0, 0, 0, 0, 0, 0, 0, 0, 0)]
    shdr = b"".join(name20(h[0]) + struct.pack("<iiiiiBbHH", *h[1:]) for h in headers)

    instruments = [
        ("Tone", [
            [(PAN, -200), (VOL_RELEASE, -6000)],                                                # global zone
            [key_range(0, 59), (SAMPLE_MODES, 1), (CUTOFF, 8000), (Q, 60), (SAMPLE_ID, 0)],     # loop, static low-pass
            [key_range(60, 71), (SAMPLE_MODES, 3), (CUTOFF, 7000), (MODENV_CUTOFF, 3600), (MODLFO_CUTOFF, 1200),
             (MODLFO_FREQ, 1200), (MODENV_ATTACK, -4000), (MODENV_DECAY, -3000), (MODENV_SUSTAIN, 600),
             (VIB_PITCH, 50), (VIBLFO_FREQ, 600), (START_LOOP_OFS, 50), (SAMPLE_ID, 0)],        # swept cutoff, vibrato
            [key_range(72, 127), (SAMPLE_MODES, 0), (CUTOFF, 14000), (MODLFO_VOLUME, 30), (MODLFO_FREQ, 2400),
             (PAN, 350), (VOL_ATTACK, -5000), (SAMPLE_ID, 0)],                                  # no loop, filter inactive
        ]),
        ("Kit", [
            [key_range(0, 60), (EXCLUSIVE_CLASS, 1), (ROOT_KEY, 50), (SAMPLE_ID, 1)],
            [key_range(61, 127), (EXCLUSIVE_CLASS, 1), (PAN, 300), (FINE_TUNE, 25), (VOL_DECAY, -4000),
             (VOL_SUSTAIN, 400), (SAMPLE_ID, 1)],
        ]),
    ]
    presets = [
        ("Lead", 0, 0, [[(ATTENUATION, 30)], [(INSTRUMENT, 0)]]),                               # global zone
        ("Octave", 5, 0, [[key_range(0, 100), (COARSE_TUNE, 12), (MODENV_PITCH, 100), (INSTRUMENT, 0)],
                          [key_range(101, 127), (INSTRUMENT, 1)]]),
        ("Drums", 0, 128, [[(INSTRUMENT, 1)]]),
    ]
    ifirst, ibag, igen = bags_and_generators([z for _, z in instruments])
    inst = b"".join(name20(n) + struct.pack("<H", f) for n, f in zip([i[0] for i in instruments] + ["EOI"], ifirst))
    pfirst, pbag, pgen = bags_and_generators([p[3] for p in presets])
    heads = [(p[0], p[1], p[2]) for p in presets] + [("EOP", 0, 0)]
    phdr = b"".join(name20(n) + struct.pack("<HHHiii", patch, bank, f, 0, 0, 0) for (n, patch, bank), f in zip(heads, pfirst))
    mod_end = b"\0" * 10
    info = b"INFO" + chunk("ifil", struct.pack("<HH", 2, 1)) + chunk("isng", b"EMU8000\0") + chunk("INAM", b"tiny test bank\0\0")
    sdta = b"sdta" + chunk("smpl", smpl.tobytes())
    pdta = b"pdta" + chunk("phdr", phdr) + chunk("pbag", pbag) + chunk("pmod", mod_end) + chunk("pgen", pgen) \
        + chunk("inst", inst) + chunk("ibag", ibag) + chunk("imod", mod_end) + chunk("igen", igen) + chunk("shdr", shdr)
    body = b"sfbk" + chunk("LIST", info) + chunk("LIST", sdta) + chunk("LIST", pdta)
    return b"RIFF" + struct.pack("<I", len(body)) + body


# ---------------------------------------------------------------------------------------------- the sessions
def ev(method, *args):
    return ["ev", method, list(args)]


def render(*frames):
    return [["render", n] for n in frames]


def sessions():
    s = []

    def add(name, steps, sr=44100, block_size=64, polyphony=64, program=None):
        s.append({"name": name, "sr": sr, "block_size": block_size, "polyphony": polyphony, "program": program,
                  "steps": steps})

    two = [ev("note_on", 0, 45, 100), ev("note_on", 0, 64, 90)]
    add("held_released", two + render(1500) + [ev("note_off", 0, 45)] + render(700) + [ev("note_off", 0, 64)]
        + render(2600))
    add("chord", [ev("note_on", 0, 40, 110), ev("note_on", 0, 62, 80), ev("note_on", 0, 50, 120), ev("note_on", 1, 66, 70)]
        + render(900) + [ev("note_off", 0, 40)] + render(1300) + [ev("note_off", 0, 62), ev("note_off", 1, 66)]
        + render(640) + [ev("note_off", 0, 50)] + render(1500))
    add("ends_itself", [ev("note_on", 0, 72, 100), ev("note_on", 0, 79, 100), ev("note_on", 0, 50, 60)] + render(1000)
        + [ev("note_off", 0, 50)] + render(1200))
    add("controllers", two + render(300) + [ev("process_midi_message", 0, 0xE0, 0, 96)] + render(300)
        + [ev("process_midi_message", 0, 0xB0, 0x01, 100), ev("process_midi_message", 0, 0xB0, 0x21, 5)] + render(300)
        + [ev("process_midi_message", 0, 0xB0, 0x07, 60), ev("process_midi_message", 0, 0xB0, 0x27, 3)] + render(200)
        + [ev("process_midi_message", 0, 0xB0, 0x0B, 90)] + render(200)
        + [ev("process_midi_message", 0, 0xB0, 0x0A, 127), ev("process_midi_message", 0, 0xB0, 0x2A, 127)] + render(200)
        + [ev("process_midi_message", 0, 0xB0, 0x0A, 0), ev("process_midi_message", 0, 0xB0, 0x2A, 0)] + render(200)
        + [ev("process_midi_message", 0, 0xB0, 0x40, 127), ev("note_off", 0, 45), ev("note_off", 0, 64)] + render(500)
        + [ev("process_midi_message", 0, 0xB0, 0x65, 0), ev("process_midi_message", 0, 0xB0, 0x64, 0),
           ev("process_midi_message", 0, 0xB0, 0x06, 12), ev("process_midi_message", 0, 0xB0, 0x26, 50),
           ev("process_midi_message", 0, 0xB0, 0x64, 1), ev("process_midi_message", 0, 0xB0, 0x06, 70),
           ev("process_midi_message", 0, 0xB0, 0x64, 2), ev("process_midi_message", 0, 0xB0, 0x06, 66),
           ev("process_midi_message", 0, 0xE0, 0, 32)] + render(300)
        + [ev("process_midi_message", 0, 0xB0, 0x40, 0)] + render(400)
        + [ev("process_midi_message", 0, 0xB0, 0x79, 0), ["set", "master_volume", 0.8], ev("note_on", 0, 45, 90),
           ev("note_on", 0, 30, 90)] + render(500))
    add("program_change", [ev("note_on", 0, 64, 100), ev("process_midi_message", 0, 0xC0, 5, 0), ev("note_on", 0, 52, 100),
                           ev("note_on", 0, 110, 100)] + render(1200)
        + [ev("process_midi_message", 0, 0xC0, 77, 0), ev("note_on", 0, 47, 100),
           ev("process_midi_message", 0, 0xB0, 0x00, 3), ev("process_midi_message", 0, 0xC0, 5, 0),
           ev("note_on", 0, 74, 64)] + render(900))
    add("program_at_start", [ev("note_on", 0, 57, 100), ev("note_on", 0, 60, 100)] + render(1100), program=5)
    add("percussion", [ev("note_on", 9, 50, 100), ev("note_on", 0, 45, 80)] + render(200) + [ev("note_on", 9, 70, 127)]
        + render(300) + [ev("process_midi_message", 9, 0xB0, 0x00, 1), ev("note_on", 9, 40, 90)] + render(800))
    add("exclusive_class", [ev("note_on", 9, 50, 100), ev("note_on", 1, 45, 80)] + render(256) + [ev("note_on", 9, 62, 110)]
        + render(256) + [ev("note_on", 9, 48, 127), ev("note_on", 10, 48, 127)] + render(700))
    add("all_off", [ev("note_on", 0, 45, 100), ev("note_on", 1, 47, 100), ev("note_on", 1, 64, 100), ev("note_on", 2, 50, 90)]
        + render(400) + [ev("note_off_all_channel", 1, True)] + render(300) + [ev("note_off_all_channel", 0, False)]
        + render(500) + [ev("note_on", 3, 45, 100), ev("note_on", 3, 47, 100)] + render(200)
        + [ev("note_off_all", False)] + render(300) + [ev("note_on", 3, 40, 100), ev("note_on", 3, 41, 100)] + render(128)
        + [ev("note_off_all", True)] + render(128) + [ev("note_on", 4, 33, 100), ev("note_on", 4, 36, 100)] + render(192)
        + [ev("reset")] + render(64))
    steal = []
    for i in range(8):
        steal += [ev("note_on", 0, 36 + 2 * i, 60 + 8 * i)] + render(96)
    steal += [ev("note_off", 0, 38), ev("note_off", 0, 44)] + render(320) + [ev("note_on", 0, 55, 100)] + render(64) \
        + [ev("note_on", 0, 57, 100)] + render(1200)
    add("stolen", steal, polyphony=8)
    add("block8", two + render(300) + [ev("note_off", 0, 45)] + render(301) + [ev("note_on", 0, 77, 100)] + render(299),
        block_size=8)
    add("block1024", two + [ev("note_on", 0, 72, 100)] + render(1024) + [ev("note_off", 0, 45)] + render(3072),
        block_size=1024)
    add("sr48000", two + [ev("note_on", 0, 84, 100), ev("note_on", 9, 65, 100)] + render(1000)
        + [ev("note_off", 0, 64), ev("note_off", 0, 45)] + render(2000), sr=48000)
    add("odd_requests", two + render(1, 63, 64, 65, 1000) + [ev("note_off", 0, 45), ev("note_on", 0, 74, 100)]
        + render(1, 63, 64, 65, 1000))
    # the stream the graph test pulls in 64-frame blocks: a note_on between blocks
    add("graph", [ev("note_on", 0, 45, 100)] + render(64, 64, 64) + [ev("note_on", 0, 66, 100)] + render(*[64] * 9)
        + [ev("note_off", 0, 45)] + render(*[64] * 12))
    return s


# ---------------------------------------------------------------------------------------------- recording the reference
class Recorder:
    """Wraps the reference's audio-plane methods for the lifetime of one Synthesizer and builds its render table."""

    def __init__(self, synth_mod, osc_mod, filter_mod):
        self.classes = (synth_mod.Synthesizer, osc_mod.Oscillator, filter_mod.BiQuadFilter)
        self.block_rows, self.rows_i, self.rows_d = [0], [], []
        self.voice_of = {}
        self.pending = {}
        self.struck = set()

    def attach(self, synth):
        self.synth = synth
        self.voice_of = {id(v._block): i for i, v in enumerate(synth._voices._voices)}
        Synthesizer, Oscillator, BiQuadFilter = self.classes
        rec = self
        self.saved = (Oscillator.fill_block, BiQuadFilter.process, BiQuadFilter.clear_buffer, Synthesizer._write_block,
                      Synthesizer._render_block)
        fill, process, clear, write, render_block = self.saved

        def fill_block(osc, block, ratio):
            before = (float(osc._position), bool(osc._looping))
            ok = fill(osc, block, ratio)
            if ok:
                rec.pending[id(block)] = {"position": before[0], "ratio": float(ratio), "loop": before[1],
                                          "end": osc._end, "start_loop": osc._start_loop, "end_loop": osc._end_loop}
            return ok

        def clear_buffer(flt):
            flt._recorder_clear = True
            clear(flt)

        def filter_process(flt, block):
            row = rec.pending[id(block)]
            row["clear"] = getattr(flt, "_recorder_clear", False)
            flt._recorder_clear = False
            row["active"] = bool(flt._active)
            row["coefficients"] = [float(c) for c in (flt._a0, flt._a1, flt._a2, flt._a3, flt._a4)] if flt._active \
                else [0.0] * 5
            process(flt, block)

        def write_block(synth_, previous, current, source, destination):
            row = rec.pending[id(source)]
            side = "left" if destination is synth_._block_left else "right"
            row[side] = SO.mix_mode(previous, current, synth_._inverse_block_size)
            # the rule itself is checked against what the reference does with the destination
            before = destination.copy()
            write(synth_, previous, current, source, destination)
            changed = not np.array_equal(before, destination)
            assert changed <= (row[side][0] != SO.MIX_SKIP), "a skipped side was written"
            if side == "right":
                flags = (SO.F_CLEAR if row["clear"] else 0) | (SO.F_LOOP if row["loop"] else 0) \
                    | (SO.F_FILTER if row["active"] else 0)
                rec.rows_i.append([rec.voice_of[id(source)], flags, row["end"], row["start_loop"], row["end_loop"],
                                   row["left"][0], row["right"][0], 0])
                rec.rows_d.append([row["position"], row["ratio"]] + row["coefficients"] + list(row["left"][1:])
                                  + list(row["right"][1:]))

        def render_block_(synth_):
            rec.pending = {}
            render_block(synth_)
            rec.block_rows.append(len(rec.rows_i))

        Oscillator.fill_block, BiQuadFilter.process, BiQuadFilter.clear_buffer = fill_block, filter_process, clear_buffer
        Synthesizer._write_block, Synthesizer._render_block = write_block, render_block_

    def detach(self):
        Synthesizer, Oscillator, BiQuadFilter = self.classes
        (Oscillator.fill_block, BiQuadFilter.process, BiQuadFilter.clear_buffer, Synthesizer._write_block,
         Synthesizer._render_block) = self.saved

    def table(self):
        return (np.asarray(self.block_rows, dtype=np.int32), np.asarray(self.rows_i, dtype=np.int32).reshape(-1, SO.ICOLS),
                np.asarray(self.rows_d, dtype=np.float64).reshape(-1, SO.DCOLS))


def describe_font(font):
    def region(r, owner_list, owner_attr):
        d = {"gs": [int(v) for v in r._gs]}
        d[owner_attr] = owner_list.index(getattr(r, "_" + owner_attr))
        return d
    return {
        "wave_length": int(len(font.wave_data)),
        "info": {"version": [font.info.version.major, font.info.version.minor], "bank_name": font.info.bank_name,
                 "target_sound_engine": font.info.target_sound_engine},
        "sample_headers": [{"name": h.name, "start": h.start, "end": h.end, "start_loop": h.start_loop,
                            "end_loop": h.end_loop, "sample_rate": h.sample_rate, "original_pitch": h.original_pitch,
                            "pitch_correction": h.pitch_correction} for h in font.sample_headers],
        "instruments": [{"name": i.name, "regions": [region(r, list(font.sample_headers), "sample") for r in i.regions]}
                        for i in font.instruments],
        "presets": [{"name": p.name, "patch_number": p.patch_number, "bank_number": p.bank_number,
                     "regions": [region(r, list(font.instruments), "instrument") for r in p.regions]}
                    for p in font.presets],
    }


def main():
    gen_golden.load_reference()
    import importlib
    melty = importlib.import_module("pygmu2.meltysynth")
    synth_mod = importlib.import_module("pygmu2.meltysynth.synth.synthesizer")
    osc_mod = importlib.import_module("pygmu2.meltysynth.synth.oscillator")
    filter_mod = importlib.import_module("pygmu2.meltysynth.synth.filter_")
    pair_mod = importlib.import_module("pygmu2.meltysynth.synth.region_pair")

    sf2_path = os.path.join(GOLDEN, "soundfont_tiny.sf2")
    blob = build_sf2()
    with open(sf2_path, "wb") as f:
        f.write(blob)
    font = melty.SoundFont.from_file(sf2_path)
    wave_i16 = np.round(np.asarray(font.wave_data) * 32768.0).astype(np.int16)
    assert np.array_equal(wave_i16.astype(np.float64) * (1.0 / 32768.0), np.asarray(font.wave_data))

    struck = set()
    pair_init = pair_mod.RegionPair.__init__

    def pair_spy(self, preset, instrument):
        struck.add(("preset", id(preset)))
        struck.add(("instrument", id(instrument)))
        pair_init(self, preset, instrument)
    pair_mod.RegionPair.__init__ = pair_spy

    arrays, out_sessions, seen = {}, [], {"modes": set(), "inactive": False, "reclear": False, "swap": False, "stolen": False}
    for session in sessions():
        settings = melty.SynthesizerSettings(session["sr"])
        settings.block_size = session["block_size"]
        settings.maximum_polyphony = session["polyphony"]
        synth = melty.Synthesizer(font, settings)
        rec = Recorder(synth_mod, osc_mod, filter_mod)
        rec.attach(synth)
        try:
            if session["program"] is not None:
                synth.process_midi_message(0, 0xC0, session["program"], 0)
            pieces, active = [], []
            for step in session["steps"]:
                if step[0] == "ev":
                    if step[1] == "note_on" and synth.active_voice_count == session["polyphony"]:
                        seen["stolen"] = True
                    getattr(synth, step[1])(*step[2])
                elif step[0] == "set":
                    setattr(synth, step[1], step[2])
                else:
                    left, right = np.zeros(step[1]), np.zeros(step[1])
                    synth.render(left, right, 0, step[1])
                    pieces.append(np.column_stack([left, right]))
                    active.append(int(synth.active_voice_count))
        finally:
            rec.detach()
        block_rows, rows_i, rows_d = rec.table()
        want = np.concatenate(pieces)
        name, bs = session["name"], session["block_size"]

        # the restated audio plane over the recorded table is the reference's output, bit for bit
        plane = SO.AudioPlane(wave_i16, bs, session["polyphony"])
        blocks = plane.render(block_rows, rows_i, rows_d)
        got = SO.requests_over_blocks(session, blocks)
        if not (got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))):
            raise SystemExit(f"{name}: the restated audio plane differs from the reference "
                             f"(max {np.max(np.abs(got - want)) if got.shape == want.shape else 'shape'})")
        per_block = np.diff(block_rows)
        audible = [sum(1 for r in range(block_rows[k], block_rows[k + 1]) if rows_i[r, 5] or rows_i[r, 6])
                   for k in range(len(per_block))]
        if max(audible) < 2:
            raise SystemExit(f"{name}: no block with two audible voices")
        seen["modes"] |= set(rows_i[:, 5]) | set(rows_i[:, 6])
        seen["inactive"] |= bool(np.any(rows_i[:, 1] & SO.F_FILTER == 0))
        first_seen = set()
        for k in range(len(per_block)):
            ids = [int(v) for v in rows_i[block_rows[k]:block_rows[k + 1], 0]]
            for r in range(block_rows[k], block_rows[k + 1]):
                v = int(rows_i[r, 0])
                if rows_i[r, 1] & SO.F_CLEAR and v in first_seen:
                    seen["reclear"] = True
                first_seen.add(v)
            if k and len(ids) >= 1:
                prev = [int(v) for v in rows_i[block_rows[k - 1]:block_rows[k], 0]]
                common = [v for v in ids if v in prev]
                if common != [v for v in prev if v in ids]:
                    seen["swap"] = True
        arrays[f"{name}/samples"] = want.astype(np.float32)
        arrays[f"{name}/block_rows"], arrays[f"{name}/rows_i"], arrays[f"{name}/rows_d"] = block_rows, rows_i, rows_d
        out_sessions.append(dict(session, active=active, frames=int(len(want)), blocks=int(len(per_block)),
                                 rows=int(len(rows_i)), max_rows_in_block=int(per_block.max())))
        print(f"{name}: {len(want)} frames, {len(per_block)} blocks, {len(rows_i)} rows, <= {per_block.max()} per block")
    pair_mod.RegionPair.__init__ = pair_init

    for preset in font.presets:
        for region in preset.regions:
            if ("preset", id(region)) not in struck:
                raise SystemExit(f"a zone of preset {preset.name} is never struck")
    for instrument in font.instruments:
        for k, region in enumerate(instrument.regions):
            if ("instrument", id(region)) not in struck:
                raise SystemExit(f"zone {k} of instrument {instrument.name} is never struck")
    if seen["modes"] != {0, 1, 2} or not all(seen[k] for k in ("inactive", "reclear", "swap", "stolen")):
        raise SystemExit(f"the sessions miss a path: {seen}")

    np.savez_compressed(os.path.join(GOLDEN, "soundfont.npz"), **arrays)
    with open(os.path.join(GOLDEN, "soundfont_cases.json"), "w") as f:
        json.dump({"font": describe_font(font), "sessions": out_sessions}, f, indent=1)
        f.write("\n")
    for fn in ("soundfont.npz", "soundfont_cases.json", "soundfont_tiny.sf2"):
        print(fn, os.path.getsize(os.path.join(GOLDEN, fn)), "bytes")


if __name__ == "__main__":
    main()
