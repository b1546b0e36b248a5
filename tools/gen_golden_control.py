"""
Fixtures for SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE: render the cases below through the reference
implementation (a started NullRenderer graph, the caller's blocks) and write tests/golden/control_cases.json +
tests/golden/control.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_control.py
The npz holds data only: per case the float32 samples of its stored blocks ("<name>").  The json holds the graph SPECs,
the blocks, the reference's extent of the root and repr / extent / purity / channel count / input types of every new PE
in the graph (in construction order), the lifecycle calls between blocks ("ops": reset_state() of the new PEs / stop +
start of the renderer before block i) and, per case, how it is compared: "compare": "bits", or "peak" -- max abs error
<= 1e-6 * peak of the case -- for graphs that hold a SlewLimiterPE (its time-parallel solution carries ~1e-13 in the
entry levels) or a stateful sawtooth FunctionGenPE whose phase sums are not exact in float64.

Checked while generating, against the reference alone:
  * the numpy restatement (tests/control_oracle.py) gives every block bit for bit;
  * FunctionGenPE with inexact phase sums: no sample's phase lies within 1e-6 cycle of a discontinuity of its waveform
    (the wrap for a sawtooth with duty at an end; the duty threshold and the wrap for a rectangle).  A rectangle that
    satisfies this is compared "bits" after all: a +-1 output has no "close";
  * SlewLimiterPE: the reference, rendered again in 16-frame blocks with the carried value of every SlewLimiterPE
    perturbed by +-1e-13 (relative) before each of them, stays within the bound.
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import affine, describe, render_reference, sums_exact, write_fixture      # noqa: E402
from oracle.golden_cases import S, blocks_contig                  # noqa: E402
from fixture_harness import PEAK_BOUND, stored_blocks             # noqa: E402
import control_oracle as P                                         # noqa: E402

SR = 48000
EDGE_CLEARANCE = 1e-6
PERTURB = 1e-13
PERTURB_EVERY = 16


def SH(source, trigger, initial_value=0.0):
    return S("SampleHoldPE", source=source, trigger=trigger, initial_value=initial_value)


def TH(source, gate, initial_value=0.0):
    return S("TrackHoldPE", source=source, gate=gate, initial_value=initial_value)


def SL(source, rise, fall=None, mode="linear"):
    return S("SlewLimiterPE", source=source, rise_rate=rise, fall_rate=fall, mode=mode)


def FG(frequency=1.0, duty_cycle=0.5, phase=0.0, waveform="rectangle", channels=1):
    return S("FunctionGenPE", frequency=frequency, duty_cycle=duty_cycle, phase=phase, waveform=waveform,
             channels=channels)


def noise(seed, n=2048, ch=1):
    return S("ArrayPE", data={"rng": seed, "n": n, "ch": ch, "scale": 0.5})


def values(v):
    return S("ArrayPE", data={"values": [float(x) for x in v]})


def events(n, at, level=1.0):
    v = np.zeros(n)
    v[list(at)] = level
    return values(v)


def staircase(seed=11):
    """A step every 128 frames: the classic noise -> sample-and-hold."""
    return SH(noise(seed), S("PeriodicTrigger", hz=375.0))


SLEW_SOURCES = {"staircase": staircase(), "noise": noise(12), "sine": S("SinePE", frequency=20.0, amplitude=0.5)}
SLEW_RATES = {"symmetric": (50.0, None), "fastrise": (2000.0, 5.0), "never": (1e6, 1e6), "always": (0.01, 0.01)}


def cases():
    c = []

    def add(name, graph, blocks, **extra):
        c.append(dict({"name": name, "sr": SR, "graph": graph, "blocks": blocks}, **extra))

    three = blocks_contig(0, [64, 192, 256])
    gaps = [[0, 128], [128, 128], [1000, 128], [300, 128]]
    for p, H, thr, periodic in (("sh", SH, 0.0, S("PeriodicTrigger", hz=375.0)),
                                ("th", TH, 0.5, S("PeriodicGate", frequency=200.0, duty_cycle=0.3))):
        # an initial value that float32 does not hold, and nothing passes in the first block
        add(f"{p}_initial_no_latch", H(noise(1), events(512, [100, 101, 300]), 0.1), three)
        # a latch on the first and on the last sample of a block
        add(f"{p}_latch_first_last", H(noise(2), events(512, [0, 63, 64, 255, 256, 511]), -0.3), three)
        add(f"{p}_stereo_source", H(noise(3, ch=2), periodic, 0.25), three)
        # a source that ends at 200: a latch beyond it takes the 0 the source renders there
        add(f"{p}_bounded_source", H(S("CropPE", source=S("SinePE", frequency=500.0), start=0, duration=200),
                                     events(512, [50, 150, 199, 250, 400]), 0.1), three)
        # control samples exactly at the threshold do not pass; the float32 neighbours on either side do / do not
        up, down = np.nextafter(np.float32(thr), np.float32(1)), np.nextafter(np.float32(thr), np.float32(-1))
        pattern = np.tile(np.array([thr, down, thr, up, thr, thr, -1.0, 1.0], dtype=np.float32), 64)
        add(f"{p}_threshold_exact", H(noise(4), values(pattern), 0.1), three)
        add(f"{p}_gap_state_carried", H(noise(5), periodic, 0.1), gaps)
        add(f"{p}_reset_restart", H(noise(6), periodic, 0.1), blocks_contig(0, [96] * 6), ops={"2": "reset", "4": "restart"})
        add(f"{p}_stream_64", H(S("SinePE", frequency=300.0), periodic, 0.1), blocks_contig(0, [64] * 16))
    # a gate that opens and closes within blocks of one frame
    add("th_single_frames", TH(noise(7), S("PeriodicGate", frequency=6000.0, duty_cycle=0.5), 0.1), blocks_contig(0, [1] * 24))

    # ---- SlewLimiterPE: modes x rate pairs x sources
    slew_blocks = blocks_contig(0, [1, 511, 1024])
    for mode in ("linear", "exponential"):
        for rname, (rise, fall) in SLEW_RATES.items():
            for sname, src in SLEW_SOURCES.items():
                add(f"slew_{mode}_{rname}_{sname}", SL(src, rise, fall, mode), slew_blocks)
    # rise_rate / sr > 1: the exponential coefficient is clamped to 1, the falling one is not
    add("slew_exponential_rise_k_clamped", SL(noise(13), 96000.0, 4800.0, "exponential"), slew_blocks)
    add("slew_gap_state_carried", SL(noise(14), 300.0, 100.0), gaps)
    add("slew_reset_restart", SL(staircase(15), 100.0, None, "exponential"), blocks_contig(0, [96] * 6),
        ops={"2": "reset", "4": "restart"})
    add("slew_stereo_source", SL(noise(16, ch=2), 500.0), blocks_contig(0, [64, 448]))
    add("slew_stream_64", SL(staircase(17), 200.0, 50.0), blocks_contig(0, [64] * 16))

    # ---- FunctionGenPE, all scalars: waveforms x duties, a negative start, 2 channels
    pure_blocks = [[-300, 200], [-100, 312]]
    for wf in ("rectangle", "sawtooth"):
        for duty in (0.0, 1e-13, 0.25, 0.5, 1.0):
            add(f"fg_pure_{wf}_duty_{duty:g}", FG(441.0, duty, 0.0, wf, 2), pure_blocks)
        add(f"fg_pure_{wf}_phase", FG(1000.0, 0.3, 0.37, wf, 1), blocks_contig(0, [1, 64, 447]))
        add(f"fg_pure_{wf}_duty_near_1", FG(333.0, 1.0 - 1e-13, 0.1, wf, 1), pure_blocks)
    # ---- FunctionGenPE with PE parameters
    st_blocks = blocks_contig(0, [1, 511, 1024])
    vib = affine(S("SinePE", frequency=5.0), 20.0, 440.0)                 # 440 Hz +- vibrato: inexact sums
    duty_pe = affine(S("SinePE", frequency=3.0), 0.3, 0.5)
    phase_pe = affine(S("SinePE", frequency=2.0), 0.25, 0.25)
    for wf in ("rectangle", "sawtooth"):
        add(f"fg_stateful_{wf}_frequency", FG(vib, 0.3, 0.0, wf), st_blocks)
        add(f"fg_stateful_{wf}_duty", FG(441.0, duty_pe, 0.0, wf), st_blocks)
        add(f"fg_stateful_{wf}_phase", FG(441.0, 0.3, phase_pe, wf), st_blocks)
        add(f"fg_stateful_{wf}_all", FG(vib, duty_pe, phase_pe, wf, 2), st_blocks)
        # 750 Hz at 48 kHz: dt = 1/64, every sum exact
        add(f"fg_stateful_{wf}_exact", FG(S("ConstantPE", value=750.0), 0.25, 0.0, wf), st_blocks)
        add(f"fg_stateful_{wf}_seek", FG(vib, 0.4, 0.0, wf), [[0, 256], [256, 256], [4096, 256], [4352, 256], [100, 256]])
        add(f"fg_stateful_{wf}_stop_start", FG(vib, 0.4, 0.0, wf), blocks_contig(0, [128] * 6),
            ops={"2": "reset", "4": "restart"})
    add("fg_stateful_sawtooth_duty_ends", FG(vib, 0.0, 0.0, "sawtooth"), st_blocks)
    add("fg_stateful_bounded_parameter", FG(S("PiecewisePE", points=[[100, 200.0], [900, 800.0]]), 0.5, 0.0, "sawtooth"),
        blocks_contig(0, [512, 512]))
    add("fg_stateful_stream_64", FG(S("ConstantPE", value=375.0), duty_pe, 0.0, "sawtooth"), blocks_contig(0, [64] * 16))

    # ---- the classic patch: noise -> sample-and-hold -> slew -> filter cutoff
    cutoff = affine(SL(SH(noise(21, 8192), S("PeriodicTrigger", hz=12.0)), 30.0, 10.0), 1000.0, 3000.0)
    add("patch_sh_slew_biquad", S("BiquadPE", source=S("BlitSawPE", frequency=110.0), frequency=cutoff, q=2.0),
        blocks_contig(0, [1024] * 8), keep_every=2)
    c += fuzz_cases()
    c += channel_cases()
    return c


# ---------------------------------------------------------------------------------------------- 3, 4, 5, 8 channels
def channel_cases():
    """Sources of 3, 4, 5 and 8 different columns under SampleHoldPE / TrackHoldPE (a mono control: pgx_hold's vector
    path; a control as wide as the source) and SlewLimiterPE (both modes) -- these PEs read channel 0 of a wider source
    or control and give one channel, so it is the strides of the reads that change; FunctionGenPE with `channels` of as
    many, pure and stateful.  Blocks of odd lengths from a negative start, state carried."""
    c = []
    odd = blocks_contig(-37, [1, 17, 257, 1000])
    vib = affine(S("SinePE", frequency=5.0), 20.0, 440.0)
    for ch in (3, 4, 5, 8):
        def add(name, graph, blocks=odd):
            c.append({"name": f"ch{ch}_{name}", "sr": SR, "graph": graph, "blocks": blocks})
        add("sh_mono_control", SH(noise(200 + ch, 1300, ch), S("PeriodicTrigger", hz=375.0), 0.1))
        add("sh_wide_control", SH(noise(210 + ch, 1300, ch), affine(noise(220 + ch, 1300, ch), 1.0, -0.6), 0.1))
        add("th_mono_control", TH(noise(230 + ch, 1300, ch), S("PeriodicGate", frequency=200.0, duty_cycle=0.3), 0.1))
        add("th_wide_control", TH(noise(240 + ch, 1300, ch), affine(noise(250 + ch, 1300, ch), 1.0, 0.5), 0.1))
        add("slew_linear", SL(noise(260 + ch, 1300, ch), 2000.0, 500.0, "linear"))
        add("slew_exponential", SL(noise(270 + ch, 1300, ch), 3000.0, 800.0, "exponential"))
        add("fg_pure_sawtooth", FG(441.0, 0.25, 0.1, "sawtooth", ch))
        add("fg_pure_rectangle", FG(441.0, 0.3, 0.37, "rectangle", ch))
        add("fg_stateful_sawtooth", FG(vib, 0.3, 0.0, "sawtooth", ch), blocks_contig(0, [1, 17, 257, 1000]))
        add("fg_stateful_rectangle", FG(S("ConstantPE", value=750.0), 0.25, 0.0, "rectangle", ch),
            blocks_contig(0, [1, 17, 257, 1000]))
    return c


# ---------------------------------------------------------------------------------------------- random graphs
def fuzz_cases(count=40, seed=31):
    rng = np.random.default_rng(seed)
    out = []

    def pick(*options):
        return options[int(rng.integers(len(options)))]

    def r(lo, hi, digits=2):
        return float(np.round(rng.uniform(lo, hi), digits))

    def signal():
        kind = pick("noise", "sine", "saw", "stereo")
        if kind == "noise":
            return noise(int(rng.integers(100, 10 ** 6)), 1024)
        if kind == "stereo":
            return noise(int(rng.integers(100, 10 ** 6)), 1024, 2)
        if kind == "sine":
            return S("SinePE", frequency=r(20, 900, 1), amplitude=r(0.2, 1.0))
        return FG(pick(375.0, 750.0, 1500.0), pick(0.0, 0.25, 0.5, 1.0), 0.0, "sawtooth")

    def trigger():
        return S("PeriodicTrigger", hz=pick(375.0, 750.0, 1000.0, 3000.0), phase=pick(0.0, 0.25, 0.5))

    def gate():
        if rng.random() < 0.5:
            return S("PeriodicGate", frequency=pick(100.0, 375.0, 1000.0), duty_cycle=pick(0.1, 0.5, 0.9))
        # a +-1 rectangle as the gate: +1 passes, -1 does not
        return FG(pick(375.0, 750.0), pick(0.25, 0.5), 0.0, "rectangle")

    def hold():
        iv = pick(0.0, 0.1, -0.7)
        return SH(signal(), trigger(), iv) if rng.random() < 0.5 else TH(signal(), gate(), iv)

    def slew(src):
        return SL(src, pick(20.0, 300.0, 5000.0, 1e6), pick(None, 10.0, 1000.0), pick("linear", "exponential"))

    def fg_exact():
        return FG(S("ConstantPE", value=pick(375.0, 750.0, 1500.0)), pick(0.25, 0.5, S("ConstantPE", value=0.375)),
                  pick(0.0, 0.125), pick("rectangle", "sawtooth"), pick(1, 2))

    for i in range(count):
        shape = pick("hold", "slew_hold", "gain_slew", "fg", "hold_fg", "crop_hold", "delay_slew", "biquad_slew")
        if shape == "hold":
            g = hold()
        elif shape == "slew_hold":
            g = slew(hold())
        elif shape == "gain_slew":
            g = S("GainPE", source=S("SinePE", frequency=r(100, 800, 1)), gain=slew(hold()))
        elif shape == "fg":
            g = fg_exact()
        elif shape == "hold_fg":
            g = SH(fg_exact(), trigger(), 0.1)
        elif shape == "crop_hold":
            g = S("CropPE", source=hold(), start=int(rng.integers(0, 100)), duration=int(rng.integers(200, 500)))
        elif shape == "delay_slew":
            g = S("DelayPE", source=slew(signal()), delay=int(rng.integers(1, 50)))
        else:
            g = S("BiquadPE", source=S("BlitSawPE", frequency=r(60, 400, 1)),
                  frequency=affine(slew(hold()), 500.0, 1200.0), q=r(0.7, 3.0))
        out.append({"name": f"fuzz_{i:02d}_{shape}", "sr": SR, "graph": g, "blocks": blocks_contig(0, [64, 448]),
                    "fuzz": True})
    return out


# ---------------------------------------------------------------------------------------------- checks
def fg_verdict(node, name):
    """"exact" (phase sums exact: bits), "rectangle" (inexact, clear of every edge: bits), "sawtooth" (peak)."""
    if not node.sub or not node.log:
        return "exact"                                     # pure: correctly rounded operations on the frame index
    if sums_exact(np.concatenate([b["dt"] for b in node.log])):
        return "exact"
    rect = str(node.kw.get("waveform", "rectangle")).lower() == "rectangle"
    for b in node.log:
        phase, duty = b["phase"], b["duty"]
        summed = np.ones(len(phase), dtype=bool)
        if b["restart"]:
            summed[0] = False                              # phase0 = 0 and no increment yet: no sum in this sample
        wrap = np.minimum(phase, 1.0 - phase)
        if rect:
            gap = np.minimum(wrap, np.abs(phase - duty))
        else:
            at_end = (duty <= 1e-12) | (duty >= 1.0 - 1e-12)
            gap = np.where(at_end, wrap, np.inf)
        gap = gap[summed]
        if gap.size:
            assert float(np.min(gap)) > EDGE_CLEARANCE, \
                f"{name}: a phase lies {float(np.min(gap)):g} cycle from a discontinuity: choose other parameters"
    return "rectangle" if rect else "sawtooth"


def perturbed(slew_type):
    """A way to pull one block for gen_golden.render_reference: in PERTURB_EVERY-frame parts, the carried value of every
    SlewLimiterPE moved by +-PERTURB (relative) before each of them."""
    sign = [1.0]

    def render(pe, made, s, n):
        parts = []
        for at in range(0, n, PERTURB_EVERY):
            for m in made:
                if isinstance(m, slew_type):
                    m._current *= 1.0 + sign[0] * PERTURB
            sign[0] = -sign[0]
            parts.append(pe.render(s + at, min(PERTURB_EVERY, n - at)).data.astype(np.float32))
        return np.concatenate(parts)
    return render


def main():
    mods = gen_golden.load_reference()
    arrays, all_cases = {}, cases()
    worst_perturbed = 0.0
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe, made = render_reference(case, mods, P.NEW_KINDS)
        restated, root = P.run_case(case)
        for i, (a, b) in enumerate(zip(outs, restated)):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f"{case['name']}: the restatement differs from the reference in block {i}"
        verdicts = {fg_verdict(node, case["name"]) for node in P.find_nodes(root, ("FunctionGenPE",))}
        has_slew = bool(P.find_nodes(root, ("SlewLimiterPE",)))
        case["compare"] = "peak" if (has_slew or "sawtooth" in verdicts) else "bits"
        peak = max(float(np.max(np.abs(o))) for o in outs)
        if has_slew:
            again, _, _ = render_reference(case, mods, P.NEW_KINDS, render=perturbed(mods["K"].SlewLimiterPE))
            err = max(float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) for a, b in zip(outs, again))
            assert err <= PEAK_BOUND * peak, \
                f"{case['name']}: a 1e-13 perturbation of the carried value moves the output by {err / peak:.3g} of peak"
            worst_perturbed = max(worst_perturbed, err / peak)
        if case["compare"] == "peak":
            assert peak > 0.0, f"{case['name']}: a silent case has no peak to compare against"
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        case["new_pes"] = [describe(m) for m in made]
        keep = stored_blocks(case)
        arrays[case["name"]] = np.concatenate([outs[i] for i in keep])
        print(f"{case['name']}: {arrays[case['name']].shape} {case['compare']}", flush=True)
    print(f"worst output change under the 1e-13 perturbation: {worst_perturbed:.3g} of peak")
    write_fixture("control", {"cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
