"""
Where a MeltysynthPE render spends its time: the host control plane (Python, per voice-block), the upload of the render
table, and the device entry (the read-back of the integer columns plus the two launches), for 1, 8 and 64 sustained
looping voices with swept filters (keys 60 .. 71 of tests/golden/soundfont_tiny.sf2 on channels 0 .. 5), one second at
44 100 Hz rendered as one request and as 64-frame blocks.

    python tools/soundfont_probe.py                 on the GPU: writes profiles/soundfont_probe.jsonl and .md
    python tools/soundfont_probe.py --reference     on a CPU with the reference package: the reference's
                                                    Synthesizer.render over the same notes, timed by the same loop,
                                                    into profiles/soundfont_probe_reference_cpu.jsonl
    --out DIR writes there instead of profiles/.

Every figure is the median of three timed repetitions after one warm-up repetition of the same shape; a repetition
starts a fresh synthesizer.  control: time.perf_counter around Synthesizer.advance.  upload: perf_counter around packing
and the synchronous copy.  entry: device events around pgx_soundfont_render (so the gap while the host checks the
integer columns is inside).  render: perf_counter around MeltysynthPE.render of the whole second, ending in a device
synchronise -- the end-to-end figure, measured apart from the three parts.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SF2 = os.path.join(ROOT, "tests", "golden", "soundfont_tiny.sf2")
SR, BLOCK, SECONDS = 44100, 64, 1.0
VOICES = (1, 8, 64)
REPEATS = 3


def notes(count):
    return [(i // 12, 60 + i % 12, 100) for i in range(count)]          # (channel, key, velocity); channels 0 .. 5


def requests(mode):
    frames = int(SR * SECONDS)
    return [frames] if mode == "one_request" else [BLOCK] * (frames // BLOCK) + ([frames % BLOCK] if frames % BLOCK else [])


def median_of(run):
    run()
    samples = [run() for _ in range(REPEATS)]
    return {k: statistics.median(s[k] for s in samples) for k in samples[0]}


# ---------------------------------------------------------------------------------------------- this package, on the GPU
def probe_device(voices, mode):
    import pygmu2_amd as pg
    from pygmu2_amd import device as dev
    from pygmu2_amd import meltysynth_pe as M

    pg.set_sample_rate(SR)

    def parts():
        pe = pg.MeltysynthPE(SF2, block_size=BLOCK)
        pe.on_start()
        synth, L = pe.synthesizer, dev.ensure_init()
        for channel, key, velocity in notes(voices):
            synth.note_on(channel, key, velocity)
        control = upload = entry = 0.0
        rows = blocks = 0
        out = dev.DeviceBuffer((max(requests(mode)), 2), np.float32)
        start, stop = dev.Event(), dev.Event()
        for frames in requests(mode):                # requests are whole blocks here but the last: no carry to serve
            n_blocks = -(-frames // BLOCK)
            t0 = time.perf_counter()
            block_rows, rows_i, rows_d = synth.advance(n_blocks)
            t1 = time.perf_counter()
            d_bytes, i_bytes = rows_d.nbytes, rows_i.nbytes
            packed = np.concatenate([rows_d.view(np.uint8).reshape(-1), rows_i.view(np.uint8).reshape(-1),
                                     block_rows.view(np.uint8)])
            table = dev.DeviceBuffer.from_host(packed)
            scratch = dev.DeviceBuffer((max(len(rows_i), 1) * BLOCK,), np.float64)
            t2 = time.perf_counter()
            start.record()
            dev.check(L.pgx_soundfont_render(out.ptr, frames, pe._carry.ptr, pe._wave.ptr, pe._wave_len,
                                             table.ptr + d_bytes + i_bytes, table.ptr + d_bytes, table.ptr, len(rows_i),
                                             n_blocks, BLOCK, pe._filter_state.ptr, synth.maximum_polyphony, scratch.ptr),
                      "pgx_soundfont_render")
            stop.record()
            dev.synchronize()
            control += t1 - t0
            upload += t2 - t1
            entry += stop.elapsed_ms_since(start) * 1e-3
            rows += len(rows_i)
            blocks += n_blocks
        pe.on_stop()
        return {"control_s": control, "upload_s": upload, "entry_s": entry, "voice_blocks": rows, "blocks": blocks}

    def whole():
        pe = pg.MeltysynthPE(SF2, block_size=BLOCK)
        pe.on_start()
        for channel, key, velocity in notes(voices):
            pe.synthesizer.note_on(channel, key, velocity)
        dev.synchronize()
        at, t0 = 0, time.perf_counter()
        for frames in requests(mode):
            pe.render(at, frames)
            at += frames
        dev.synchronize()
        elapsed = time.perf_counter() - t0
        pe.on_stop()
        return {"render_s": elapsed}

    rec = {"probe": "soundfont", "voices": voices, "mode": mode, "sr": SR, "block_size": BLOCK, "seconds": SECONDS,
           "device": dev.device_name(), "chunk_rows": M.MAX_CHUNK_ROWS}
    rec.update(median_of(parts))
    rec.update(median_of(whole))
    rec["control_us_per_voice_block"] = 1e6 * rec["control_s"] / max(rec["voice_blocks"], 1)
    shares = {k: rec[k] for k in ("control_s", "upload_s", "entry_s")}
    rec["bound_by"] = max(shares, key=shares.get)[:-2]
    return rec


# ---------------------------------------------------------------------------------------------- the reference, on a CPU
def probe_reference(voices, mode, melty):
    font = melty.SoundFont.from_file(SF2)

    def run():
        settings = melty.SynthesizerSettings(SR)
        settings.block_size = BLOCK
        synth = melty.Synthesizer(font, settings)
        for channel, key, velocity in notes(voices):
            synth.note_on(channel, key, velocity)
        t0 = time.perf_counter()
        for frames in requests(mode):
            left, right = np.zeros(frames), np.zeros(frames)
            synth.render(left, right, 0, frames)
        return {"render_s": time.perf_counter() - t0}

    rec = {"probe": "soundfont_reference_cpu", "voices": voices, "mode": mode, "sr": SR, "block_size": BLOCK,
           "seconds": SECONDS}
    rec.update(median_of(run))
    return rec


def write_markdown(path, records, reference):
    ref = {(r["voices"], r["mode"]): r["render_s"] for r in reference}
    lines = ["# MeltysynthPE: where one second of audio goes", "",
             f"`tools/soundfont_probe.py` on {records[0]['device']}: sustained looping voices with swept filters, "
             f"{SECONDS:g} s at {SR} Hz, block size {BLOCK}; medians of {REPEATS} after a warm-up.  control = "
             "Synthesizer.advance (Python), upload = packing and the synchronous copy of the table, entry = device events "
             "around pgx_soundfont_render (read-back of the integer columns, then the two launches), render = the whole "
             "second through MeltysynthPE.render, measured apart.  reference = the reference's Synthesizer.render on a "
             "CPU (`profiles/soundfont_probe_reference_cpu.jsonl`).", "",
             "| voices | requests | control ms | us / voice-block | upload ms | entry ms | bound by | render ms | reference CPU ms | reference / render |",
             "|---:|---|---:|---:|---:|---:|---|---:|---:|---:|"]
    for r in records:
        cpu = ref.get((r["voices"], r["mode"]))
        lines.append(f"| {r['voices']} | {r['mode']} | {1e3 * r['control_s']:.2f} | {r['control_us_per_voice_block']:.2f} | "
                     f"{1e3 * r['upload_s']:.2f} | {1e3 * r['entry_s']:.2f} | {r['bound_by']} | {1e3 * r['render_s']:.2f} | "
                     + (f"{1e3 * cpu:.1f} | {cpu / r['render_s']:.2f} |" if cpu else "not measured | - |"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ref_path = os.path.join(ROOT, "profiles", "soundfont_probe_reference_cpu.jsonl")
    if args.reference:
        from oracle import gen_golden
        import importlib
        gen_golden.load_reference()
        melty = importlib.import_module("pygmu2.meltysynth")
        records = [probe_reference(v, m, melty) for v in VOICES for m in ("one_request", "blocks_of_64")]
        path = os.path.join(args.out, "soundfont_probe_reference_cpu.jsonl")
    else:
        records = [probe_device(v, m) for v in VOICES for m in ("one_request", "blocks_of_64")]
        path = os.path.join(args.out, "soundfont_probe.jsonl")
    with open(path, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)
    if not args.reference:
        reference = [json.loads(line) for line in open(ref_path)] if os.path.exists(ref_path) else []
        write_markdown(os.path.join(args.out, "soundfont_probe.md"), records, reference)


if __name__ == "__main__":
    main()
