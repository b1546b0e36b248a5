"""
Fixtures for KarplusStrongPE / AnalogOscPE: render the cases below through the reference implementation (a started
NullRenderer graph, the caller's blocks) and write tests/golden/sources_cases.json + tests/golden/sources.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_sources.py
The npz holds data only: per case the float32 samples of its stored blocks ("<name>"), the float32 parameter streams
of stateful AnalogOscPE cases ("<name>/freq", "<name>/duty"), and the rho_for_decay_db grid ("rho/...").
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_golden import load_reference, write_fixture          # noqa: E402
from fixture_harness import render_blocks, stored_blocks      # noqa: E402
from sources_oracle import build_graph                        # noqa: E402


def contig(start, sizes):
    out, s = [], start
    for n in sizes:
        out.append([s, n])
        s += n
    return out


def S(t, *args, **kwargs):
    return {"type": t, "args": list(args), "kwargs": kwargs}


def affine(src, scale, offset):
    return {"type": "Affine", "source": src, "scale": scale, "offset": offset}


def cases():
    c = []
    B = [1024] * 8
    ks = lambda **kw: S("KarplusStrongPE", **kw)            # noqa: E731
    c += [
        {"name": "ks_440_seed42", "kind": "ks", "sr": 44100, "graph": ks(frequency=440.0, rho=0.996, seed=42),
         "blocks": contig(0, B)},
        {"name": "ks_neg_start", "kind": "ks", "sr": 44100, "graph": ks(frequency=440.0, rho=0.996, seed=7),
         "blocks": contig(-300, [1024] * 5)},
        {"name": "ks_gap_seek", "kind": "ks", "sr": 44100, "graph": ks(frequency=330.0, rho=0.995, seed=11),
         "blocks": [[0, 1024], [1024, 1024], [5000, 1024], [3000, 512], [-700, 1024]]},
        {"name": "ks_two_phase", "kind": "ks", "sr": 44100,
         "graph": ks(frequency=97.3, rho=0.999, duration=3000, rho_damping=0.93, seed=5), "blocks": contig(-50, B)},
        {"name": "ks_27_5", "kind": "ks", "sr": 44100, "graph": ks(frequency=27.5, rho=0.998, seed=3),
         "blocks": contig(0, B)},
        {"name": "ks_8k", "kind": "ks", "sr": 44100, "graph": ks(frequency=8000.0, rho=0.99, seed=9),
         "blocks": contig(0, [1024] * 4)},
        {"name": "ks_rho1", "kind": "ks", "sr": 44100, "graph": ks(frequency=220.0, rho=1.0, seed=13),
         "blocks": contig(0, B)},
        {"name": "ks_stereo", "kind": "ks", "sr": 44100,
         "graph": ks(frequency=523.25, rho=0.997, seed=17, amplitude=0.5, channels=2), "blocks": contig(0, [1024] * 4)},
        {"name": "ks_sr48k", "kind": "ks", "sr": 48000, "graph": ks(frequency=261.6, rho=0.996, seed=19),
         "blocks": contig(0, [1000, 2048, 777, 4096])},
    ]
    osc = lambda **kw: S("AnalogOscPE", **kw)               # noqa: E731
    for wave in ("rectangle", "sawtooth"):
        for f, d in ((110.0, 0.3), (3520.7, 0.5), (12000.0, 0.1), (440.0, 0.0), (440.0, 1.0), (0.45 * 44100, 0.5),
                     (-220.0, 0.4)):
            for start in (0, 10 ** 6, -5000):
                c.append({"name": f"osc_pure_{wave}_{f:g}_{d:g}_{start}", "kind": "osc", "sr": 44100,
                          "graph": osc(frequency=f, duty_cycle=d, waveform=wave), "blocks": contig(start, [1024] * 2)})
    sine_duty = affine(S("SinePE", frequency=0.25, amplitude=1.0), 0.45, 0.5)
    c += [
        {"name": "osc_st_rect_sine_duty", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=110.3, duty_cycle=sine_duty, waveform="rectangle"), "blocks": contig(0, B)},
        {"name": "osc_st_saw_sine_duty", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=110.3, duty_cycle=affine(S("SinePE", frequency=3.0, amplitude=1.0), 0.4, 0.5),
                      waveform="sawtooth"), "blocks": contig(0, B)},
        {"name": "osc_st_saw_piecewise_duty", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=220.7, duty_cycle=S("PiecewisePE", [[0, 0.05], [8192, 0.95]]), waveform="sawtooth"),
         "blocks": contig(0, B)},
        {"name": "osc_st_rect_freq_sweep", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, 100.0], [8192, 2000.0]]), duty_cycle=0.5, waveform="rectangle"),
         "blocks": contig(0, B)},
        {"name": "osc_st_saw_freq_sweep", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, 100.0], [8192, 2000.0]]), duty_cycle=0.3, waveform="sawtooth"),
         "blocks": contig(0, B)},
        {"name": "osc_st_saw_negative_freq", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, -300.0], [8192, -50.0]]), duty_cycle=0.5, waveform="sawtooth"),
         "blocks": contig(0, B)},
        {"name": "osc_st_rect_restart", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, 200.0], [8192, 400.0]]), duty_cycle=0.25, waveform="rectangle"),
         "blocks": [[0, 1024], [1024, 1024], [4096, 1024], [5120, 1024]]},
        {"name": "osc_st_saw_restart", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, 200.0], [8192, 400.0]]), duty_cycle=0.6, waveform="sawtooth"),
         "blocks": [[0, 1024], [1024, 1024], [4096, 1024], [5120, 1024]]},
        {"name": "osc_st_saw_stereo", "kind": "osc", "sr": 44100,
         "graph": osc(frequency=S("PiecewisePE", [[0, 150.0], [8192, 600.0]]), duty_cycle=sine_duty,
                      waveform="sawtooth", channels=2), "blocks": contig(0, [1024] * 4)},
    ]
    # the examples' graphs (examples/21_analog_osc.py, examples/29_karplus_strong.py), 1024-frame blocks
    sr = 44100
    d6, d8 = 6 * sr, 8 * sr
    ex = []
    ex.append(("ex21_pwm", S("CropPE", S("GainPE", osc(frequency=110.0, duty_cycle=sine_duty, waveform="rectangle"),
                                         gain=0.25), 0, d6)))
    ex.append(("ex21_morph", S("CropPE", S("GainPE", osc(frequency=220.0, duty_cycle=S("PiecewisePE", [[0, 0.05], [d8, 0.95]]),
                                                         waveform="sawtooth"), gain=0.35), 0, d8)))
    ladder = S("LadderPE", osc(frequency=110.0, duty_cycle=affine(S("SinePE", frequency=0.15, amplitude=1.0), 0.40, 0.5),
                               waveform="rectangle"),
               mode="LP24", frequency=S("PiecewisePE", [[0, 400.0], [d8, 3200.0]]), resonance=0.4, drive=1.2)
    ex.append(("ex21_subtractive", S("CropPE", S("GainPE", ladder, gain=0.25), 0, d8)))

    def rho_for(seconds, f):
        return rho_for_decay_db_ref(seconds, f, sr, db=-30)

    ex.append(("ex29_single", S("CropPE", S("CropPE", ks(frequency=440.0, rho=rho_for(1.0, 440.0), amplitude=0.35, seed=1),
                                             0, sr), 0, sr)))
    ex.append(("ex29_two_phase", S("CropPE", ks(frequency=440.0, rho=0.999, duration=sr, rho_damping=0.93,
                                                amplitude=0.35, seed=42), 0, int(2.5 * sr))))
    notes, t = [], 0.0
    for midi in (60, 64, 67, 72):
        f = 440.0 * 2.0 ** ((midi - 69) / 12.0)
        note = S("CropPE", ks(frequency=f, rho=rho_for(0.8, f), amplitude=0.5, seed=1), 0, int(round(0.8 * sr)))
        notes.append(S("DelayPE", note, int(round(t * sr))))
        t += 0.8
    ex.append(("ex29_arpeggio", S("CropPE", S("MixPE", *notes), 0, int(round(t * sr)))))
    for name, g in ex:
        c.append({"name": name, "kind": "example", "sr": sr, "graph": g, "blocks": contig(0, [1024] * 120),
                  "keep_every": 8})
    return c


rho_for_decay_db_ref = None


def main():
    global rho_for_decay_db_ref
    mods = load_reference()
    mods["config"].set_sample_rate(44100)
    ks_mod = mods["karplus_strong_pe"]
    rho_for_decay_db_ref = ks_mod.rho_for_decay_db
    M = mods["K"]
    M.affine = lambda scale, offset: (lambda x: offset + scale * x)
    arrays = {}
    all_cases = cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        pe = build_graph(M, case["graph"])
        r = mods["null_renderer"].NullRenderer(sample_rate=case["sr"])
        outs = render_blocks(pe, case["sr"], case["blocks"], renderer=r)
        keep = stored_blocks(case)
        arrays[case["name"]] = np.concatenate([outs[i] for i in keep])
        if case["kind"] == "osc" and case["graph"]["kwargs"] and not pe.is_pure():
            for key, param in (("freq", pe.frequency), ("duty", pe.duty_cycle)):
                if not isinstance(param, (int, float)):
                    r.start()
                    vals = [param.render(int(s), int(n)).data[:, 0].astype(np.float32) for s, n in case["blocks"]]
                    r.stop()
                    arrays[f"{case['name']}/{key}"] = np.concatenate(vals)
        print(f"{case['name']}: {arrays[case['name']].shape}", flush=True)
    grid, errors = [], []
    for seconds in (0.1, 1.0, 2.5):
        for f in (27.5, 440.0, 4000.0, 22050.0):
            for sr in (44100, 48000):
                for db in (-60.0, -30.0, -90.0):
                    grid.append([seconds, f, sr, db, ks_mod.rho_for_decay_db(seconds, f, sr, db=db)])
    for seconds, f, sr in ((0.0, 440.0, 44100), (-1.0, 440.0, 44100), (1.0, -440.0, 44100)):
        try:
            ks_mod.rho_for_decay_db(seconds, f, sr)
        except ValueError as e:
            errors.append([seconds, f, sr, str(e)])
    arrays["rho/grid"] = np.array(grid, dtype=np.float64)
    write_fixture("sources", {"cases": all_cases, "rho_errors": errors}, arrays)


if __name__ == "__main__":
    main()
