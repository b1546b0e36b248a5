"""
Fixtures for NoisePE: render the cases below through the reference implementation (a started NullRenderer graph, the
caller's blocks) and write tests/golden/noise_cases.json + tests/golden/noise.npz.

Needs the reference package (oracle.gen_golden.load_reference) and numpy >= 2: the float32 arithmetic of PINK and BROWN
is what numpy >= 2 (NEP 50) makes of the reference's source; the version used is recorded in the json.  Run from the
repository root:
    python tools/gen_golden_noise.py
The npz holds data only: per case the float32 samples of its stored blocks ("<name>").  The json holds the graph SPECs,
the blocks, the reference's extent of the root, repr / extent / purity / channel count / inputs of every NoisePE in the
graph (in construction order), the lifecycle calls between blocks ("ops": reset_state() of the NoisePEs / stop + start
of the renderer before block i) and, per case, how it is compared:
    "bits"  nothing above the NoisePE re-associates: NoisePE alone, under MixPE, CropPE, integer DelayPE, constant GainPE,
            the holds;
    "peak"  a SlewLimiterPE in the graph: max abs error <= 1e-6 * peak of the case (fixture_harness.PEAK_BOUND);
    "fuzz"  a filter, an oscillator or an envelope in the graph: per block max abs error <= 1e-5 * peak + 1e-6
            (tests/test_gpu_fuzz.py).

A NoisePE's samples depend on how often and for how long it was pulled, not on where, so these cases also pin the pull
pattern of every PE above one.

Checked while generating, against the reference alone: the numpy restatement (tests/noise_oracle.py) gives every block
of every "bits" case bit for bit and every other case within its bound; the BROWN rail case holds an exact 1.0 and an
exact -1.0.
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import affine, describe, render_reference, write_fixture      # noqa: E402
from oracle.golden_cases import S, blocks_contig                  # noqa: E402
from fixture_harness import stored_blocks, within                 # noqa: E402
import noise_oracle as P                                           # noqa: E402

SR = 48000
SEEDS = (0, 1, 12345, 2 ** 63 + 5, 2 ** 100 + 7)
RANGES = {"unit": (0.0, 1.0), "cutoff": (100.0, 2000.0), "huge": (-1e6, 1e6), "point": (-0.3, -0.3)}
BITS_KINDS = {"NoisePE", "MixPE", "CropPE", "DelayPE", "GainPE", "SampleHoldPE", "TrackHoldPE", "PeriodicTrigger",
              "PeriodicGate", "ConstantPE"}


def N(seed, mode="white", lo=-1.0, hi=1.0):
    return S("NoisePE", seed=seed, mode=mode, min_value=lo, max_value=hi)


def compare_rule(graph):
    kinds = P.kinds_of(graph)
    if "SlewLimiterPE" in kinds:
        return "peak"
    if kinds <= BITS_KINDS and not _gain_is_pe(graph):
        return "bits"
    return "fuzz"


def _gain_is_pe(spec):
    if isinstance(spec, dict):
        if spec.get("pe") == "GainPE" and P.is_spec(spec.get("gain")):
            return True
        return any(_gain_is_pe(v) for v in spec.values())
    if isinstance(spec, list):
        return any(_gain_is_pe(v) for v in spec)
    return False


def patch(seed, mode="white"):
    """noise -> sample-and-hold -> slew -> filter cutoff."""
    steps = S("SampleHoldPE", source=N(seed, mode), trigger=S("PeriodicTrigger", hz=12.0), initial_value=0.0)
    glide = S("SlewLimiterPE", source=steps, rise_rate=30.0, fall_rate=10.0, mode="linear")
    return S("BiquadPE", source=S("BlitSawPE", frequency=110.0), frequency=affine(glide, 1000.0, 3000.0), q=2.0)


def percussion(seed, mode="white"):
    return S("GainPE", source=N(seed, mode),
             gain=S("AdsrGatedPE", gate=S("PeriodicGate", frequency=40.0, duty_cycle=0.4), attack_time=0.002,
                    decay_time=0.004, sustain_level=0.6, release_time=0.005))


def cases():
    c = []

    def add(name, graph, blocks, **extra):
        c.append(dict({"name": name, "sr": SR, "graph": graph, "blocks": blocks}, **extra))

    for mode in P.MODES:
        for seed in SEEDS:
            add(f"{mode}_seed_{seed}", N(seed, mode), blocks_contig(0, [1, 63, 64, 3968]))
        # non-contiguous and negative starts: one continuing stream
        add(f"{mode}_starts_ignored", N(3, mode), [[0, 128], [1000, 128], [-500, 128], [0, 128]])
        add(f"{mode}_reset_restart", N(4, mode), blocks_contig(0, [96] * 6), ops={"2": "reset", "4": "restart"})
        add(f"{mode}_stream_64", N(5, mode), blocks_contig(0, [64] * 16))
        for rname, (lo, hi) in RANGES.items():
            add(f"{mode}_range_{rname}", N(6, mode, lo, hi), blocks_contig(0, [64, 448]))
    # reaches +1 at frame 3941 and -1 at frame 7511
    add("brown_rails", N(27, "brown"), blocks_contig(0, [4096, 4096]))

    # ---- a NoisePE under existing PEs
    add("patch_noise_sh_slew_biquad", patch(21), blocks_contig(0, [1024] * 8), keep_every=2)
    for mode in ("white", "pink"):
        add(f"graph_biquad_{mode}", S("BiquadPE", source=N(31, mode), frequency=1200.0, q=1.5), blocks_contig(0, [64, 448, 512]))
    add("graph_gain_adsr", percussion(32), blocks_contig(0, [64, 448, 1024]))
    add("graph_comb", S("CombPE", source=N(33), frequency=440.0, feedback=0.7), blocks_contig(0, [64, 448, 512]))
    add("graph_mix_two_seeds", S("MixPE", inputs=[N(34, "white"), N(35, "brown", -0.5, 0.5)]), blocks_contig(0, [64, 448]))
    add("graph_mix_noise_and_sine", S("MixPE", inputs=[S("SinePE", frequency=440.0, amplitude=0.25), N(36, "pink")]),
        blocks_contig(0, [64, 448]))
    # CropPE: a block before the window (no pull), one across its start, one inside, one across its end, one after it
    add("graph_crop", S("CropPE", source=N(37), start=100, duration=400), [[0, 64], [64, 128], [192, 128], [320, 256], [576, 64]])
    add("graph_delay", S("DelayPE", source=N(38, "pink"), delay=17), blocks_contig(0, [64, 448]))
    add("graph_gain_const", S("GainPE", source=N(39, "brown"), gain=0.37), blocks_contig(0, [64, 448]))
    c += fuzz_cases()
    for case in c:
        case["compare"] = compare_rule(case["graph"])
    return c


def fuzz_cases(count=30, seed=41):
    rng = np.random.default_rng(seed)
    out = []

    def pick(*options):
        return options[int(rng.integers(len(options)))]

    def r(lo, hi, digits=2):
        return float(np.round(rng.uniform(lo, hi), digits))

    def noise():
        lo, hi = pick((-1.0, 1.0), (-1.0, 1.0), (0.0, 1.0), (-0.5, 0.25), (200.0, 900.0))
        return N(int(rng.integers(0, 2 ** 62)), pick(*P.MODES), lo, hi)

    def unit_noise():
        return N(int(rng.integers(0, 2 ** 62)), pick(*P.MODES))

    for i in range(count):
        shape = pick("alone", "patch", "biquad", "percussion", "comb", "mix", "crop", "delay", "hold")
        if shape == "alone":
            g = noise()
        elif shape == "patch":
            g = patch(int(rng.integers(0, 10 ** 6)), pick(*P.MODES))
        elif shape == "biquad":
            g = S("BiquadPE", source=unit_noise(), frequency=r(200, 5000, 1), q=r(0.7, 3.0),
                  mode=pick("lowpass", "highpass", "bandpass"))
        elif shape == "percussion":
            g = percussion(int(rng.integers(0, 10 ** 6)), pick(*P.MODES))
        elif shape == "comb":
            g = S("CombPE", source=unit_noise(), frequency=r(100, 900, 1), feedback=r(0.2, 0.9))
        elif shape == "mix":
            g = S("MixPE", inputs=[noise() for _ in range(int(rng.integers(2, 4)))])
        elif shape == "crop":
            g = S("CropPE", source=noise(), start=int(rng.integers(0, 100)), duration=int(rng.integers(200, 500)))
        elif shape == "delay":
            g = S("DelayPE", source=noise(), delay=int(rng.integers(1, 50)))
        else:
            g = S("SampleHoldPE", source=noise(), trigger=S("PeriodicTrigger", hz=pick(375.0, 750.0, 1000.0)),
                  initial_value=pick(0.0, 0.1))
        out.append({"name": f"fuzz_{i:02d}_{shape}", "sr": SR, "graph": g, "blocks": blocks_contig(0, [64, 448]),
                    "fuzz": True})
    return out


def main():
    assert int(np.__version__.split(".")[0]) >= 2, \
        f"numpy {np.__version__}: the float32 arithmetic of PINK / BROWN needs numpy >= 2 (NEP 50)"
    mods = gen_golden.load_reference()
    arrays, all_cases = {}, cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe, made = render_reference(case, mods, (P.KIND,))
        restated, _ = P.run_case(case)
        peak = max(float(np.max(np.abs(o))) for o in outs)
        for i, (a, b) in enumerate(zip(outs, restated)):
            assert within(case["compare"], b, a, peak), \
                f"{case['name']}: the restatement differs from the reference in block {i}"
        if case["compare"] != "bits":
            assert peak > 0.0, f"{case['name']}: a silent case has no peak to compare against"
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        case["new_pes"] = [dict(describe(m), min_value=m.min_value, max_value=m.max_value, mode=m.mode.value)
                           for m in made]
        keep = stored_blocks(case)
        arrays[case["name"]] = np.concatenate([outs[i] for i in keep])
        print(f"{case['name']}: {arrays[case['name']].shape} {case['compare']}", flush=True)
    rails = arrays["brown_rails"]
    assert np.any(rails == np.float32(1.0)) and np.any(rails == np.float32(-1.0)), "brown_rails misses a rail"
    write_fixture("noise", {"numpy": np.__version__, "cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
