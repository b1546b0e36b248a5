"""
Fixtures for ReversePitchEchoPE: render the cases below through the reference implementation (a started NullRenderer
graph, the caller's blocks) and write tests/golden/reverse_echo_cases.json + tests/golden/reverse_echo.npz.

Needs the reference package (oracle.gen_golden.load_reference: its numba stand-in makes the class take
_reverse_pitch_echo_numba, the arithmetic the device reproduces); run from the repository root:
    python tools/gen_golden_reverse_echo.py
The npz holds data only: per case the float32 samples of its "blocks" ("<name>").  The json holds the graph SPECs
(tests/reverse_echo_common.py names the new kind), the blocks, the other block "patterns" of the same stretch, the
lifecycle "ops" (tests/fixture_harness.render_blocks), the reference's extent of the root, repr / extent / purity /
channel count / input types of every ReversePitchEchoPE, the sizes it derives from the sample rate, and the echo-block
lengths it locked in.  Every case is compared "fuzz": per block REL_TOL * peak + ABS_FLOOR (tests/fixture_harness.py).

Checked while generating, on the reference alone (the tool stops at the first that fails), with CLEAR = 1e-6:
  * at every echo-block start the smoothed size is at least CLEAR away from a half-integer;
  * no pitch ratio lies within CLEAR of 1 +- 1e-4, unless it is exactly 1.0;
  * no block_seconds * sr lies within CLEAR of a half-integer or of a clamp (64, rows - 1);
  * no feedback sample lies within CLEAR of +-0.995, no alternate sample within CLEAR of 0.5;
  * every pattern of a case, and its render in one-frame blocks, equals its one-block render to the bit; a case with
    gaps or ops equals itself with every block cut in two;
  * every case spans at least 6 echo blocks and is not silent;
  * where a case says so ("needs"), block lengths grow and shrink / both direction branches follow a forward block.
"""

from __future__ import annotations

import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import affine, describe, write_fixture     # noqa: E402
from oracle.golden_cases import S, blocks_contig                  # noqa: E402
import fixture_harness as H                                       # noqa: E402
from fixture_harness import bits_equal                            # noqa: E402
import reverse_echo_common as RC                                  # noqa: E402

SR = 8000                  # pitch buffer 133 frames (odd: half of it is 66.5), a 64-frame echo block is 0.008 s
SR_HIGH = 48000            # pitch buffer 800 frames
CLEAR = 1e-6


def RPE(source, block=0.02, ratio=1.0, fb=0.85, alt=0.0, smoothing=2400):
    return S(RC.KIND, source=source, block_seconds=block, pitch_ratio=ratio, feedback=fb, alternate_direction=alt,
             smoothing_samples=smoothing)


def noise(seed, n, ch=1):
    return S("ArrayPE", data={"rng": seed, "n": n, "ch": ch, "scale": 0.5})


def values(v):
    return S("ArrayPE", data={"values": [float(x) for x in v]})


def sine(hz, scale, offset):
    return affine(S("SinePE", frequency=hz), scale, offset)


def runs(levels, length):
    return values(np.repeat(np.asarray(levels, dtype=np.float64), length))


def patterns(n):
    """Contiguous cuts of [0, n).  With 160-frame echo blocks "edges" has a block edge on an echo-block edge (160, 320)
    and one frame after one (1); "around" one frame before (159), one after (161) and on one (320)."""
    def rest(sizes):
        return blocks_contig(0, sizes + [n - sum(sizes)])
    return {"edges": rest([1, 159, 160, 777]),
            "around": rest([159, 2, 159]),
            "b64": blocks_contig(0, [64] * (n // 64) + ([n % 64] if n % 64 else [])),
            "ones": rest([1] * 7 + [313] + [1] * 5 + [64, 63, 65])}


def cases():
    c = []

    def add(name, graph, n, sr=SR, blocks=None, **extra):
        case = {"name": name, "sr": sr, "graph": graph, "compare": "fuzz",
                "blocks": blocks or [[0, n]], "patterns": {} if blocks else patterns(n)}
        c.append(dict(case, **extra))

    # ---- scalar parameters
    add("defaults_like", RPE(noise(1, 3000)), 3000)
    add("example_settings", RPE(noise(2, 3000, 2), 0.02, 0.75, 0.6, 1.0), 3000)
    add("unity_no_feedback", RPE(noise(3, 2000), 0.02, 1.0, 0.0), 2000)
    add("ratio_2", RPE(noise(4, 2500), 0.02, 2.0, 0.7), 2500)
    add("ratio_half_3ch", RPE(noise(5, 2500, 3), 0.02, 0.5, 0.7), 2500)
    add("ratio_below_minimum", RPE(noise(6, 2000), 0.02, 0.0005, 0.7), 2000)
    add("feedback_above_maximum", RPE(noise(7, 2500), 0.02, 1.5, 2.0), 2500)
    add("feedback_below_minimum", RPE(noise(8, 2500), 0.02, 1.5, -2.0), 2500)
    add("block_below_minimum", RPE(noise(9, 2000), 0.001, 1.25, 0.8), 2000)
    add("alternate_0", RPE(noise(10, 2500), 0.02, 1.5, 0.8, 0.0), 2500)
    add("alternate_1", RPE(noise(10, 2500), 0.02, 1.5, 0.8, 1.0), 2500)
    add("sine_source", RPE(S("SinePE", frequency=440.0, amplitude=0.5), 0.02, 1.5, 0.7, 1.0), 2500)
    add("sr48k_scalars_2ch", RPE(noise(11, 4000, 2), 0.005, 0.75, 0.6, 1.0), 4000, sr=SR_HIGH)
    # ---- stream parameters
    # 64 .. 256 frames around 160, a 3 Hz swing (2667 frames) followed closely: lengths grow and shrink
    add("block_stream", RPE(noise(12, 4000), sine(3.0, 0.012, 0.02), 1.5, 0.7, smoothing=50), 4000, needs="grow_shrink")
    add("ratio_stream_crosses_unity", RPE(noise(13, 3000), 0.02, sine(2.0, 0.3, 1.0), 0.7), 3000)
    add("feedback_stream_crosses_clamps", RPE(noise(14, 3000), 0.02, 1.5, sine(5.0, 1.2, 0.0)), 3000)
    add("alternate_stream_runs", RPE(noise(15, 3200), 0.02, 1.5, 0.8, runs([1, 1, 0, 1, 0, 0, 1, 1], 400)), 3200,
        needs="both_after_forward")
    add("all_four_streams_2ch",
        RPE(noise(16, 4000, 2), sine(3.0, 0.01, 0.02), sine(2.0, 0.4, 1.1), sine(5.0, 1.1, 0.0),
            runs([1, 0, 1, 1, 0, 1, 1, 1, 0, 1], 400), smoothing=50), 4000)
    add("ratio_stream_2ch_uses_channel_0", RPE(noise(17, 2500), 0.02, affine(noise(18, 2500, 2), 0.4, 1.4), 0.7), 2500)
    # smoothing_samples=1: the size follows its target at once (from the 0.25 s a stream parameter starts at)
    add("sr48k_block_stream", RPE(noise(19, 4000), sine(20.0, 0.002, 0.004), 1.5, 0.7, smoothing=1), 4000, sr=SR_HIGH,
        needs="grow_shrink")
    # ---- state: a gap and a backward seek change nothing, reset_state() changes nothing, a restart starts silent
    add("gap_and_seek", RPE(noise(20, 3000), 0.02, 1.5, 0.8, 1.0), 0,
        blocks=[[0, 700], [1000, 600], [300, 900], [1200, 500]])
    add("reset_and_restart", RPE(noise(21, 3000, 2), 0.02, 0.75, 0.8), 0, blocks=blocks_contig(0, [500] * 6),
        ops={"2": "reset", "4": "restart"})
    # ---- the example's dry/wet mix, one source instance on both paths
    src = dict(noise(22, 3000, 2), share="src")
    add("dry_wet_mix", S("MixPE", inputs=[S("GainPE", source=src, gain=0.5),
                                           S("GainPE", source=RPE(src, 0.02, 0.75, 0.6, 1.0), gain=0.5)]), 3000)
    return c


# ---------------------------------------------------------------------------------------------- checks
def near(v, x):
    return np.abs(np.asarray(v, dtype=np.float64) - x) < CLEAR


class Recorder:
    """A thin wrapper around the module's kernel function: checks the control values of every call, and in calls of one
    frame notes what the frame locked in and decided."""

    def __init__(self, mod):
        self.inner = mod._reverse_pitch_echo_numba
        self.name = ""
        self.clear()

    def clear(self):
        self.locked, self.boundaries = [], []        # echo-block lengths; (was reverse, alternate) per boundary

    def __call__(self, x, block, pitch, fb, alt, a, b, is_a, pbuf, pwp, prp, w, r, smoothed, cur, prev, rev, sr, lo, rows,
                 *rest):
        target = np.asarray(block, dtype=np.float64) * sr
        assert not np.any(near(target - np.floor(target), 0.5)), f"{self.name}: block * sr near a half-integer"
        assert not np.any(near(target, lo) | near(target, rows - 1)), f"{self.name}: block * sr near a clamp"
        ratio = np.asarray(pitch, dtype=np.float64)
        assert not np.any(near(np.abs(ratio - 1.0), 1e-4) & (ratio != 1.0)), f"{self.name}: a ratio near 1 +- 1e-4"
        assert not np.any(near(np.abs(fb), 0.995)), f"{self.name}: a feedback near +-0.995"
        assert not np.any(near(alt, 0.5)), f"{self.name}: an alternate near 0.5"
        out = self.inner(x, block, pitch, fb, alt, a, b, is_a, pbuf, pwp, prp, w, r, smoothed, cur, prev, rev, sr, lo, rows,
                         *rest)
        if x.shape[0] == 1:
            if w == 0:
                s = out[6]
                assert abs(s - np.floor(s) - 0.5) >= CLEAR, f"{self.name}: smoothed size {s} near a half-integer"
                self.locked.append(int(out[7]))
            if out[4] == 0:
                self.boundaries.append((int(rev), bool(alt[0] >= 0.5)))
        return out


def split_in_two(case):
    blocks, ops = [], {}
    for i, (s, n) in enumerate(case["blocks"]):
        if str(i) in case.get("ops", {}):
            ops[str(len(blocks))] = case["ops"][str(i)]
        blocks += [[s, n // 2], [s + n // 2, n - n // 2]]
    return dict(case, blocks=blocks, ops=ops)


def one_frame_blocks(case):
    blocks, ops = [], {}
    for i, (s, n) in enumerate(case["blocks"]):
        if str(i) in case.get("ops", {}):
            ops[str(len(blocks))] = case["ops"][str(i)]
        blocks += [[s + k, 1] for k in range(n)]
    return dict(case, blocks=blocks, ops=ops)


def render_reference(case, mods, kinds, render=None):
    """oracle.gen_golden.render_reference with the new kind: a case with its "ops" through the reference's classes
    -> (blocks, root PE, its PEs of `kinds` in construction order)."""
    made = []
    pe = RC.build(case["graph"], mods["K"], on_make=lambda kind, node: made.append(node) if kind in kinds else None)
    outs = H.render_blocks(pe, case["sr"], case["blocks"], case.get("ops"), lambda: H.reset_all(made),
                           renderer=mods["null_renderer"].NullRenderer(sample_rate=case["sr"]),
                           render=render and (lambda s, n: render(pe, made, s, n)))
    return outs, pe, made


def main():
    mods = gen_golden.load_reference()
    mod = importlib.import_module("pygmu2.reverse_pitch_echo_pe")
    assert mod.NUMBA_AVAILABLE
    setattr(mods["K"], RC.KIND, mod.ReversePitchEchoPE)
    rec = Recorder(mod)
    mod._reverse_pitch_echo_numba = rec
    arrays, all_cases = {}, cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        rec.name = case["name"]
        outs, pe, made = render_reference(case, mods, RC.NEW_KINDS)
        flat = np.concatenate(outs)
        assert flat.dtype == np.float32 and np.all(np.isfinite(flat))
        peak = float(np.max(np.abs(flat)))
        assert peak > 0.05, f"{case['name']}: peak {peak}: a silent case has no bar"
        others = dict(case["patterns"], split=split_in_two(case)["blocks"])
        for pname, blocks in others.items():
            again = split_in_two(case) if pname == "split" else dict(case, blocks=blocks)
            got = np.concatenate(render_reference(again, mods, RC.NEW_KINDS)[0])
            assert bits_equal(got, flat), f"{case['name']}/{pname}: the reference differs from its one-block render"
        rec.clear()
        got = np.concatenate(render_reference(one_frame_blocks(case), mods, RC.NEW_KINDS)[0])
        assert bits_equal(got, flat), f"{case['name']}: the reference differs in one-frame blocks"
        locked, boundaries = list(rec.locked), list(rec.boundaries)
        assert len(locked) >= 6, f"{case['name']}: {len(locked)} echo blocks"
        if case.get("needs") == "grow_shrink":
            d = np.diff(locked)
            assert np.any(d > 0) and np.any(d < 0), f"{case['name']}: lengths {locked}"
        if case.get("needs") == "both_after_forward":
            after_forward = {alternate for was_reverse, alternate in boundaries if not was_reverse}
            assert after_forward == {True, False}, f"{case['name']}: after a forward block only {after_forward}"
        case["echo_blocks"] = locked
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        case["new_pes"] = [describe(m) for m in made]
        # the sizes a started instance derives from the sample rate
        fresh, _, _ = render_reference(dict(case, blocks=[[0, 1]], ops={}), mods, RC.NEW_KINDS,
                                             render=lambda pe, made, s, n: sizes(case, made))
        case["sizes"] = fresh[0]
        arrays[case["name"]] = flat
        print(f"{case['name']}: {flat.shape} peak {peak:.4g} echo blocks {locked[:8]}{'...' if len(locked) > 8 else ''}",
              flush=True)
    write_fixture(RC.FAMILY, {"cases": all_cases}, arrays)


def sizes(case, made):
    """Read before the first frame of a started graph."""
    return [{"rows": int(m._buffer_a.shape[0]), "pitch_len": int(m._pitch_buffer.shape[0]),
             "initial_smoothed": int(m._smoothed_block_samples)} for m in made]


if __name__ == "__main__":
    main()
