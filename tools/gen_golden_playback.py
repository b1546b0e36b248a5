"""
Fixtures for WavetablePE / TimeWarpPE: render the cases below through the reference implementation (a started
NullRenderer graph, the caller's blocks) and write tests/golden/playback_cases.json + tests/golden/playback.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_playback.py
The npz holds data only: per case the float32 samples of its stored blocks ("<name>").  The json holds the graph SPECs,
the blocks, the reference's extent of the root and repr / extent / purity / channel count / input types of every new PE
in the graph (in construction order: inputs before the PE that reads them), the lifecycle calls between blocks ("ops": reset_state() of the TimeWarpPEs / stop + start of the renderer
before block i) and, per case, how it is compared: "compare": "bits", or "peak" -- max abs error <= 1e-6 * peak of the
case -- for graphs that hold a TimeWarpPE whose rate sums are not exact in float64 (a parallel scan re-associates them).

Checked while generating: the numpy restatement (tests/playback_oracle.py) gives every block bit for bit; for every
"peak" case no head position lies within 1e-6 frame of a finite edge of its source's extent (there the mask switches
a sample to 0, and no tolerance on the positions covers that).
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
from fixture_harness import reset_all, stored_blocks              # noqa: E402
import playback_oracle as P                                        # noqa: E402

SR = 48000
EDGE_CLEARANCE = 1e-6


def WT(table, indexer, interpolation="linear", out_of_bounds="zero"):
    return S("WavetablePE", wavetable=table, indexer=indexer, interpolation=interpolation, out_of_bounds=out_of_bounds)


def TW(source, rate, interpolation="linear"):
    return S("TimeWarpPE", source=source, rate=rate, interpolation=interpolation)


def noise(seed, n, ch=1):
    return S("ArrayPE", data={"rng": seed, "n": n, "ch": ch, "scale": 0.5})


def sine_table(length, start=0):
    """One cycle of a sine over `length` frames, as a table whose extent is [start, start + length)."""
    return S("CropPE", source=S("SinePE", frequency=SR / length), start=start, duration=length)


def cases():
    c = []

    def add(name, graph, blocks, **extra):
        c.append(dict({"name": name, "sr": SR, "graph": graph, "blocks": blocks}, **extra))

    mixed = blocks_contig(0, [1, 64, 1024])
    short = blocks_contig(0, [64, 512])
    # ---- WavetablePE: every mode x interpolation; indices below, inside and beyond the table
    swing = affine(S("SinePE", frequency=97.0), 200.0, 128.0)               # [-72, 328] over a table on [0, 256)
    for mode in ("zero", "clamp", "wrap"):
        for interp in ("linear", "cubic"):
            add(f"wt_{mode}_{interp}", WT(noise(1, 256), swing, interp, mode), mixed)
            # a table whose extent is [100, 400): indices [0, 500]
            add(f"wt_offset_{mode}_{interp}",
                WT(sine_table(300, 100), affine(S("SinePE", frequency=61.0), 250.0, 250.0), interp, mode), short)
        # an unbounded table: the index stays raw in every mode
        add(f"wt_unbounded_{mode}", WT(S("SinePE", frequency=100.0), affine(S("SinePE", frequency=31.0), 3000.0, 0.0),
                                        "cubic", mode), short)
    add("wt_stereo_wrap_cubic", WT(noise(2, 200, 2), affine(S("SinePE", frequency=53.0), 400.0, 50.0), "cubic", "wrap"), short)
    add("wt_stereo_zero_linear", WT(noise(2, 200, 2), affine(S("SinePE", frequency=53.0), 400.0, 50.0), "linear", "zero"), short)
    # the indexer's extent [100, 900) is the output's
    add("wt_bounded_indexer", WT(noise(3, 256), S("PiecewisePE", points=[[100, 0.0], [900, 255.0]]), "linear", "zero"),
        blocks_contig(0, [512, 512]))
    # integer-valued indices: the last one sits on the window's edge with a weight-0 neighbour beyond it
    ramp = S("PiecewisePE", points=[[0, 0.0], [512, 512.0]])
    for interp in ("linear", "cubic"):
        add(f"wt_integer_zero_{interp}", WT(noise(4, 256), ramp, interp, "zero"), blocks_contig(0, [256, 256]))
        add(f"wt_integer_wrap_{interp}", WT(noise(4, 256), ramp, interp, "wrap"), blocks_contig(0, [256, 256]))
    # a 2048-frame table oscillator, one large block
    saw = S("LoopPE", source=S("PiecewisePE", points=[[0, 0.0], [109, 2048.0]]), loop_start=0, loop_end=109)
    add("wt_osc_48000", WT(sine_table(2048), saw, "cubic", "wrap"), [[0, 48000]])
    add("wt_osc_stream", WT(sine_table(2048), saw, "cubic", "wrap"), blocks_contig(0, [64] * 16))

    # ---- TimeWarpPE: scalar rates over a source on [-1500, 1500) that the head leaves
    tape = S("DelayPE", source=noise(5, 3000), delay=-1500)
    steps = blocks_contig(0, [1, 64, 1024, 1, 1024])
    for rate in (1.0, 1.5, 0.25, -1.0, 0.0, 1.1):
        add(f"tw_rate_{rate:g}_linear", TW(tape, rate), steps)
    for rate in (1.5, -1.0, 1.1):
        add(f"tw_rate_{rate:g}_cubic", TW(tape, rate, "cubic"), steps)
    # a source on [500, 2500) that the head enters and leaves
    add("tw_enter_leave", TW(S("DelayPE", source=noise(6, 2000), delay=500), 1.0, "cubic"), blocks_contig(0, [1024] * 3))
    # sources open on one side or both
    add("tw_unbounded_1.1", TW(S("SinePE", frequency=220.0), 1.1), blocks_contig(0, [1, 64, 1024]))
    add("tw_unbounded_0.25_cubic", TW(S("SinePE", frequency=220.0), 0.25, "cubic"), blocks_contig(0, [1, 64, 1024]))
    add("tw_open_end", TW(S("CropPE", source=S("SinePE", frequency=220.0), start=-100, duration=None), -0.75), blocks_contig(0, [64, 512]))
    # PE rates: a ramp through zero in steps of 1/512 (every partial sum exact), a general ramp, a constant, a slow sine
    add("tw_ramp_through_zero", TW(tape, S("PiecewisePE", points=[[0, 2.0], [2048, -2.0]], extend_mode="hold_both"), "cubic"),
        blocks_contig(0, [1, 64, 1024, 1024, 512]))
    add("tw_ramp_general", TW(tape, S("PiecewisePE", points=[[0, 0.3], [3000, 1.7]], extend_mode="hold_both")),
        blocks_contig(0, [1, 64, 1024, 1024]))
    add("tw_constant_pe_rate", TW(tape, S("ConstantPE", value=1.5), "cubic"), blocks_contig(0, [64, 1024]))
    add("tw_sine_rate", TW(S("SinePE", frequency=330.0), affine(S("SinePE", frequency=3.0), 1.5, 0.5), "cubic"),
        blocks_contig(0, [64, 1024, 1024]))
    add("tw_bounded_rate", TW(tape, S("PiecewisePE", points=[[100, 1.0], [900, 2.0]])), blocks_contig(0, [512, 512]))
    # renders that are not contiguous: whatever the reference does with them (it does not look at `start`)
    gaps = [[0, 512], [512, 512], [4096, 512], [2000, 256]]
    add("tw_gap_scalar", TW(tape, 0.5, "cubic"), gaps)
    add("tw_gap_pe_rate", TW(tape, S("PiecewisePE", points=[[0, 0.5], [4096, 1.0]], extend_mode="hold_both")), gaps)
    # reset_state() before block 2, stop + start before block 4: the head is back at 0 each time
    add("tw_reset_scalar", TW(tape, 1.5), blocks_contig(0, [256] * 6), ops={"2": "reset", "4": "restart"})
    add("tw_reset_pe_rate", TW(tape, S("ConstantPE", value=0.75), "cubic"), blocks_contig(0, [256] * 6),
        ops={"2": "reset", "4": "restart"})
    add("tw_stream_64", TW(tape, S("PiecewisePE", points=[[0, 2.0], [1024, -2.0]], extend_mode="hold_both")),
        blocks_contig(0, [64] * 24))
    # the reference's example 20 over a synthetic buffer (N frames): a speed ramp, and the jog-shuttle ramp
    N = 24000
    loop = S("LoopPE", source=noise(7, 6000), crossfade_seconds=0.01)
    speed = TW(loop, S("PiecewisePE", points=[[0, 0.25], [N, 5.0]]))
    add("ex20_speed_ramp", S("CropPE", source=S("GainPE", source=speed, gain=0.8), start=0, duration=N),
        blocks_contig(0, [1024] * 24), keep_every=4)
    jog = TW(loop, S("PiecewisePE", points=[[0, 2.0], [48000, -2.0]]))
    add("ex20_jog_shuttle_48000", S("CropPE", source=S("GainPE", source=jog, gain=0.8), start=0, duration=48000),
        [[0, 48000]])
    c += fuzz_cases()
    c += channel_cases()
    return c


# ---------------------------------------------------------------------------------------------- 3, 4, 5, 8 channels
def channel_cases():
    """Tables and tapes of 3, 4, 5 and 8 different columns (a float4 straddles frames at 3, lies inside one at 5; a
    frame is one or two float4s at 4 and 8): every out-of-bounds mode x interpolation of WavetablePE, TimeWarpPE at a
    scalar and at a PE rate, in blocks of odd lengths that carry the head from one to the next."""
    c = []
    swing = affine(S("SinePE", frequency=97.0), 200.0, 128.0)               # [-72, 328] over a table on [0, 256)
    for ch in (3, 4, 5, 8):
        for mode in ("zero", "clamp", "wrap"):
            for interp in ("linear", "cubic"):
                c.append({"name": f"ch{ch}_wt_{mode}_{interp}", "sr": SR, "blocks": blocks_contig(-37, [1, 17, 257]),
                          "graph": WT(noise(100 + ch, 256, ch), swing, interp, mode)})
        tape = S("DelayPE", source=noise(110 + ch, 3000, ch), delay=-1500)
        ramp = S("PiecewisePE", points=[[0, 0.3], [3000, 1.7]], extend_mode="hold_both")
        c.append({"name": f"ch{ch}_tw_rate_1.5_cubic", "sr": SR, "blocks": blocks_contig(0, [1, 17, 257]),
                  "graph": TW(tape, 1.5, "cubic")})
        c.append({"name": f"ch{ch}_tw_pe_rate", "sr": SR, "blocks": blocks_contig(0, [1, 17, 257]),
                  "graph": TW(tape, ramp)})
    return c


# ---------------------------------------------------------------------------------------------- random graphs
def fuzz_cases(count=40, seed=20):
    rng = np.random.default_rng(seed)
    out = []

    def pick(*options):
        return options[int(rng.integers(len(options)))]

    def table():
        if rng.random() < 0.5:
            return noise(int(rng.integers(100, 10 ** 6)), int(rng.integers(32, 400)), pick(1, 1, 2))
        return sine_table(int(rng.integers(64, 512)), int(rng.integers(-50, 200)))

    def indexer():
        kind = pick("sine", "ramp", "delay")
        if kind == "ramp":
            a, b = (float(np.round(rng.uniform(-100, 500), 2)) for _ in range(2))
            return S("PiecewisePE", points=[[0, a], [int(rng.integers(200, 600)), b]], extend_mode="hold_both")
        sine = affine(S("SinePE", frequency=float(np.round(rng.uniform(20, 300), 1))),
                      float(np.round(rng.uniform(50, 400), 1)), float(np.round(rng.uniform(-50, 300), 1)))
        if kind == "delay":
            return S("DelayPE", source=sine, delay=float(np.round(rng.uniform(0.5, 20), 2)),
                     interpolation=pick("linear", "cubic"))
        return sine

    def rate():
        kind = pick("ramp", "steps", "constant", "sine")
        if kind == "ramp":
            a, b = (float(np.round(rng.uniform(-2, 3), 3)) for _ in range(2))
            return S("PiecewisePE", points=[[0, a], [int(rng.integers(200, 600)), b]], extend_mode="hold_both")
        if kind == "steps":                        # steps of a power of two: every partial sum is exact
            return S("PiecewisePE", points=[[0, pick(-1.0, 0.5, 2.0)], [512, pick(-2.0, 1.0, 3.0)]],
                     extend_mode="hold_both")
        if kind == "constant":
            return S("ConstantPE", value=pick(0.5, 1.0, 1.25, -0.75, 1.1))
        return affine(S("SinePE", frequency=float(np.round(rng.uniform(0.5, 5), 2))), 2.0, pick(0.0, 0.5, 1.0))

    def wavetable():
        return WT(table(), indexer(), pick("linear", "cubic"), pick("zero", "clamp", "wrap"))

    def source():
        kind = pick("tape", "sine", "wavetable")
        if kind == "tape":
            return S("DelayPE", source=noise(int(rng.integers(100, 10 ** 6)), int(rng.integers(300, 2000)), pick(1, 1, 2)),
                     delay=int(rng.integers(-600, 100)))
        if kind == "sine":
            return S("SinePE", frequency=float(np.round(rng.uniform(50, 2000), 1)))
        return wavetable()

    def timewarp():
        return TW(source(), pick(rate(), rate(), pick(1.0, 1.5, 0.25, -1.0, 1.1)), pick("linear", "cubic"))

    for i in range(count):
        shape = pick("wt", "tw", "gain_wt", "crop_tw", "wt_of_tw", "gain_tw")
        if shape == "wt":
            g = wavetable()
        elif shape == "tw":
            g = timewarp()
        elif shape == "gain_wt":
            g = S("GainPE", source=wavetable(), gain=float(np.round(rng.uniform(0.1, 2), 2)))
        elif shape == "crop_tw":
            g = S("CropPE", source=timewarp(), start=int(rng.integers(0, 100)), duration=int(rng.integers(200, 500)))
        elif shape == "wt_of_tw":                  # a time-warped ramp as the index stream
            ramp = S("PiecewisePE", points=[[0, 0.0], [2000, float(np.round(rng.uniform(200, 900), 1))]],
                     extend_mode="hold_both")
            g = WT(table(), TW(ramp, pick(rate(), 1.5, 0.5)), pick("linear", "cubic"), pick("zero", "clamp", "wrap"))
        else:
            g = S("GainPE", source=timewarp(), gain=S("PiecewisePE", points=[[0, 0.0], [256, 1.0]], extend_mode="hold_both"))
        out.append({"name": f"fuzz_{i:02d}_{shape}", "sr": SR, "graph": g, "blocks": blocks_contig(0, [64, 448]),
                    "fuzz": True})
    return out


def main():
    mods = gen_golden.load_reference()
    arrays, all_cases = {}, cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe, made = render_reference(case, mods, P.NEW_KINDS, reset=lambda made: reset_all(
            m for m in made if isinstance(m, mods["K"].TimeWarpPE)))
        restated, root = P.run_case(case)
        for i, (a, b) in enumerate(zip(outs, restated)):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f"{case['name']}: the restatement differs from the reference in block {i}"
        exact = True
        for node in P.find_nodes(root, "TimeWarpPE"):
            if not node.positions:
                continue
            pos = np.concatenate(node.positions)
            rates = np.concatenate(node.rates)
            if sums_exact(rates):
                continue
            exact = False
            for edge in node.sub["source"].extent():
                if edge is not None:
                    gap = float(np.min(np.abs(pos - float(edge))))
                    assert gap > EDGE_CLEARANCE, \
                        f"{case['name']}: a head position lies {gap:g} frames from the extent edge {edge}"
        case["compare"] = "bits" if exact else "peak"
        # what the reference says about the graph's root and about every new PE in it, for the host-side tests
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        case["new_pes"] = [describe(m) for m in made]
        keep = stored_blocks(case)
        arrays[case["name"]] = np.concatenate([outs[i] for i in keep])
        print(f"{case['name']}: {arrays[case['name']].shape} {case['compare']}", flush=True)
    write_fixture("playback", {"cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
