"""
Random graphs over EVERY exported PE kind, in the spec language of oracle/golden_cases.py -- the second generator of
the differential fuzz, shared by tests/test_gpu_fuzz_all.py and oracle/gen_golden_fuzz.py.

tests/test_gpu_fuzz.py's `_graph` stays as it is (its seeds keep their graphs); this module reuses its helpers and adds
what it never draws: KarplusStrongPE, AnalogOscPE (pure rectangle, pure sawtooth, stateful forms driven by other PEs,
negative frequencies included), CachePE referenced twice from one graph (and under TriggerRestartPE), and IdentityPE
(behind a ~1e-4 GainPE: its ramp would swamp the tolerance of what follows).  The new sources also go under the
processors that re-address pulls (DelayPE, LoopPE, WindowPE, TriggerRestartPE, SpatialPE) and under MixPEs of cropped
inputs, and the effects lean on what the old generator rarely reaches on long blocks and in streams: TriggerRestartPE,
AdsrTriggeredPE and the compressor family.

Three pull patterns, as in test_gpu_fuzz.py: `short_case` (blocks of 1 .. 5000 frames, negative starts), `long_case`
(4096 .. 65 537 frames) and `stream_case` (dozens of equal blocks with seeks and steps back).

`bit_exact(graph)` says whether every node of a graph is a kind DESIGN section 6 holds bit-exact to the reference.
"""

from __future__ import annotations

import numpy as np

from test_gpu_fuzz import _control, _effect, _source


# ------------------------------------------------------------------------------------------------ bit-exact kinds
def _node_bit_exact(g) -> bool:
    """DESIGN section 6 ("bit-exact"): Constant / Identity / Dirac / Array / Crop, GainPE with a constant gain, the
    gates and triggers with scalar parameters, both ADSRs, DelayPE by a whole number of frames, PiecewisePE step /
    linear, LoopPE (crossfade included), MixPE off the voice-bank paths (a MixPE of two different trees), CachePE,
    TriggerRestartPE (it only re-addresses its source's pulls), KarplusStrongPE, the pure AnalogOscPE rectangle."""
    k = g["pe"]
    if k in ("ConstantPE", "IdentityPE", "DiracPE", "ArrayPE", "CropPE", "CachePE", "LoopPE", "PeriodicTrigger",
             "AdsrGatedPE", "AdsrTriggeredPE", "TriggerRestartPE", "KarplusStrongPE"):
        return True
    if k == "GainPE":
        return not isinstance(g.get("gain", 1.0), dict)
    if k == "PeriodicGate":
        return not any(isinstance(g.get(p), dict) for p in ("frequency", "duty_cycle", "phase"))
    if k == "DelayPE":
        return not isinstance(g["delay"], dict) and float(g["delay"]).is_integer()
    if k == "PiecewisePE":
        return g.get("transition_type", "linear") in ("step", "linear")
    if k == "MixPE":
        return len(g["inputs"]) <= 2 and not (len(g["inputs"]) == 2 and g["inputs"][0] == g["inputs"][1])
    if k == "AnalogOscPE":
        return (str(g.get("waveform", "rectangle")) == "rectangle"
                and not any(isinstance(g.get(p), dict) for p in ("frequency", "duty_cycle")))
    return False


def bit_exact(g) -> bool:
    """True if every node of the spec `g` is of a bit-exact kind (`_node_bit_exact`): the HIP output must then equal
    the reference's (and the oracle's) float32 samples exactly."""
    if isinstance(g, list):
        return all(bit_exact(x) for x in g)
    if not isinstance(g, dict):
        return True
    if "pe" in g and not _node_bit_exact(g):
        return False
    return all(bit_exact(v) for k, v in g.items() if isinstance(v, (dict, list)) and k != "data")


def kinds(g, out=None) -> set:
    """Every PE kind named in a spec."""
    out = set() if out is None else out
    if isinstance(g, list):
        for x in g:
            kinds(x, out)
    elif isinstance(g, dict):
        if "pe" in g:
            out.add(g["pe"])
        for v in g.values():
            kinds(v, out)
    return out


# ------------------------------------------------------------------------------------------------ new sources
def _karplus_strong(rng, ch):
    sr_lines = rng.random() < 0.1            # a line of 17 640 .. 88 200 floats: beyond LDS, the global-memory path
    f = float(rng.uniform(0.5, 2.5)) if sr_lines else float(np.exp(rng.uniform(np.log(27.5), np.log(8000.0))))
    g = {"pe": "KarplusStrongPE", "frequency": f, "rho": 1.0 if rng.random() < 0.25 else float(rng.uniform(0.97, 0.9995)),
         "amplitude": float(rng.uniform(0.1, 0.8)), "seed": int(rng.integers(1 << 16)), "channels": ch}
    what = rng.random()
    if what < 0.4:                                   # two-phase decay, the switch anywhere in the first blocks
        g["duration"] = int(rng.integers(0, 6000))
        g["rho_damping"] = float(rng.uniform(0.8, 0.995))
    elif what < 0.55:                                # duration without rho_damping: one rho throughout
        g["duration"] = int(rng.integers(0, 6000))
    return g


def _osc_control(rng, lo, hi):
    """A PE-valued oscillator parameter spanning [lo, hi]: PiecewisePE, TransformPE(SinePE) or a MixPE control."""
    kind = rng.choice(["piecewise", "transform_sine", "mix"])
    if kind == "piecewise":
        pts = sorted({int(t) for t in rng.integers(-300, 20000, size=int(rng.integers(2, 6)))})
        return {"pe": "PiecewisePE", "points": [[t, float(rng.uniform(lo, hi))] for t in pts],
                "transition_type": str(rng.choice(["step", "linear"])), "extend_mode": "hold_both"}
    if kind == "transform_sine":
        mid, span = (lo + hi) / 2.0, (hi - lo) / 2.0 * 0.9
        return {"pe": "TransformPE", "source": {"pe": "SinePE", "frequency": float(rng.uniform(0.5, 20.0))},
                "ops": [["affine", span, mid]]}
    return _control(rng, lo, hi)


def _analog_osc(rng, ch):
    wave = str(rng.choice(["rectangle", "sawtooth"]))
    if rng.random() < 0.45:                          # pure: the index-phase form
        return {"pe": "AnalogOscPE", "frequency": float(rng.uniform(30.0, 5000.0)),
                "duty_cycle": float(rng.uniform(0.05, 0.95)), "waveform": wave, "channels": ch}
    what = rng.random()
    if what < 0.15:                                  # negative frequency: the phase runs backwards
        freq = _osc_control(rng, -900.0, -60.0)
    elif what < 0.8:
        freq = _osc_control(rng, 40.0, 2500.0)
    else:
        freq = float(rng.uniform(40.0, 2500.0))
    duty = _osc_control(rng, 0.1, 0.9) if (not isinstance(freq, dict) or rng.random() < 0.5) \
        else float(rng.uniform(0.05, 0.95))
    return {"pe": "AnalogOscPE", "frequency": freq, "duty_cycle": duty, "waveform": wave, "channels": ch}


def _identity(rng, ch):
    return {"pe": "GainPE", "source": {"pe": "IdentityPE", "channels": ch}, "gain": float(rng.uniform(5e-5, 2e-4))}


def _adsr_triggered(rng):
    return {"pe": "AdsrTriggeredPE", "trigger": {"pe": "PeriodicTrigger", "hz": float(rng.uniform(5.0, 50.0))},
            "attack_time": float(rng.uniform(0.001, 0.01)), "decay_time": float(rng.uniform(0.002, 0.02)),
            "sustain_time": float(rng.uniform(0.0, 0.02)), "sustain_level": float(rng.uniform(0.2, 0.9)),
            "release_time": float(rng.uniform(0.002, 0.03))}


def _new_source(rng, ch):
    what = rng.random()
    if ch <= 2 and what < 0.3:
        return _karplus_strong(rng, ch)
    if what < 0.6:
        return _analog_osc(rng, ch)
    if what < 0.68:
        return _identity(rng, ch)
    if ch == 1 and what < 0.74:
        return _adsr_triggered(rng)
    if ch == 1 and what < 0.78:
        return {"pe": "AdsrGatedPE", "gate": {"pe": "PeriodicGate", "frequency": float(rng.uniform(3.0, 40.0)),
                                              "duty_cycle": float(rng.uniform(0.2, 0.8))},
                "attack_time": float(rng.uniform(0.001, 0.02)), "decay_time": float(rng.uniform(0.002, 0.03)),
                "sustain_level": float(rng.uniform(0.2, 0.9)), "release_time": float(rng.uniform(0.002, 0.05))}
    return _source(rng, ch)


def _stateful_subtree(rng, ch):
    """Something whose output depends on the order of its pulls: a string, a stateful oscillator, a filter."""
    what = rng.random()
    if ch <= 2 and what < 0.35:
        return _karplus_strong(rng, ch)
    if what < 0.6:
        osc = _analog_osc(rng, ch)
        if not isinstance(osc["frequency"], dict):
            osc["frequency"] = _osc_control(rng, 60.0, 1500.0)
        return osc
    src = _new_source(rng, ch)
    return {"pe": "BiquadPE", "source": src, "frequency": float(rng.uniform(200, 6000)), "q": float(rng.uniform(0.5, 4.0)),
            "mode": str(rng.choice(["lowpass", "bandpass", "highpass"]))}


# ------------------------------------------------------------------------------------------------ effects
def _cached_twice(rng, ch, tag):
    """One CachePE instance pulled from two places (a `share` name: one instance wherever it appears)."""
    c = {"pe": "CachePE", "source": _stateful_subtree(rng, ch), "share": f"cache{tag}"}
    what = rng.random()
    if what < 0.4:
        return {"pe": "MixPE", "inputs": [c, {"pe": "GainPE", "source": c, "gain": float(rng.uniform(-1.0, 1.0))}]}
    if what < 0.8:
        return {"pe": "MixPE", "inputs": [{"pe": "DelayPE", "source": c, "delay": int(rng.integers(1, 700))}, c]}
    return {"pe": "TriggerRestartPE", "trigger": {"pe": "PeriodicTrigger", "hz": float(rng.uniform(8.0, 90.0))},
            "src": {"pe": "MixPE", "inputs": [c, {"pe": "GainPE", "source": c, "gain": 0.5}]}}


def _effect_all(rng, src, ch, tag):
    what = rng.random()
    if what < 0.4:
        return _effect(rng, src, ch)
    if what < 0.55:
        return {"pe": "TriggerRestartPE", "trigger": {"pe": "PeriodicTrigger", "hz": float(rng.uniform(8.0, 90.0))},
                "src": src}, ch
    if what < 0.68:
        which = str(rng.choice(["CompressorPE", "LimiterPE", "ExpanderPE"]))
        if which == "CompressorPE":
            return {"pe": which, "source": src, "threshold": float(rng.uniform(-30.0, -6.0)),
                    "ratio": float(rng.uniform(2.0, 8.0)), "detection": str(rng.choice(["peak", "rms"])),
                    "lookahead": float(rng.choice([0.0, 0.002]))}, ch
        if which == "LimiterPE":
            return {"pe": which, "source": src, "ceiling": float(rng.uniform(-12.0, -0.5))}, ch
        return {"pe": which, "source": src, "threshold": float(rng.uniform(-40.0, -10.0)),
                "knee": float(rng.uniform(3.0, 10.0)), "gate_range": float(rng.uniform(-60.0, -20.0))}, ch
    if what < 0.74:
        return {"pe": "DelayPE", "source": src, "delay": int(rng.integers(-300, 2000))}, ch
    if what < 0.79:
        return {"pe": "DelayPE", "source": src, "delay": float(rng.uniform(0.1, 300.0)) + 0.37,
                "interpolation": str(rng.choice(["linear", "cubic"]))}, ch
    if what < 0.84:
        a = int(rng.integers(-100, 900))
        return {"pe": "LoopPE", "source": src, "loop_start": a, "loop_end": a + int(rng.integers(30, 4000)),
                "count": None if rng.random() < 0.5 else int(rng.integers(1, 5)),
                "crossfade_seconds": None if rng.random() < 0.4 else float(rng.uniform(0.0, 0.02))}, ch
    if what < 0.88:
        return {"pe": "WindowPE", "source": src, "window": float(rng.choice([0.0, 0.0007, 0.004])),
                "mode": str(rng.choice(["max", "min", "mean", "rms"])), "rectify": bool(rng.random() < 0.8)}, ch
    if what < 0.92:
        if rng.random() < 0.5:
            out = int(rng.integers(1, 3))
            return {"pe": "SpatialPE", "source": src, "method": "adapter", "channels": out}, out
        return {"pe": "SpatialPE", "source": src, "method": str(rng.choice(["linear", "constant_power"])),
                "azimuth": float(rng.uniform(-120, 120))}, 2
    if what < 0.96:
        return {"pe": "CropPE", "source": src, "start": int(rng.integers(-200, 800)),
                "duration": int(rng.integers(500, 9000)), "extend_mode": "zero"}, ch
    return {"pe": "MixPE", "inputs": [src, _cached_twice(rng, ch, tag)]}, ch


def _cropped(rng, g):
    return {"pe": "CropPE", "source": g, "start": int(rng.integers(-400, 3000)), "duration": int(rng.integers(200, 6000)),
            "extend_mode": "zero"}


def _draw_graph(rng):
    ch = int(rng.choice([1, 1, 2]))
    tags = iter(range(100))
    g = _cached_twice(rng, ch, next(tags)) if rng.random() < 0.1 else _new_source(rng, ch)
    for _ in range(int(rng.integers(1, 4))):
        g, ch = _effect_all(rng, g, ch, next(tags))
    if rng.random() < 0.35:
        other = _new_source(rng, ch)
        if rng.random() < 0.7:                       # bounded extents: the mix skips what misses the window
            g, other = _cropped(rng, g), _cropped(rng, other)
        g = {"pe": "MixPE", "inputs": [g, other]}
    return g, ch


# ------------------------------------------------------------------------------------------------ pull patterns
def _short_blocks(rng):
    sizes = [int(v) for v in rng.choice([1, 17, 64, 257, 1024, 3000, 5000], size=int(rng.integers(2, 5)))]
    return _contiguous(int(rng.integers(-600, 400)), sizes)


def _long_blocks(rng):
    sizes = [int(v) for v in rng.choice([4096, 12_289, 20_000, 48_000, 65_537], size=int(rng.integers(2, 4)))]
    return _contiguous(int(rng.integers(-600, 400)), sizes)


def _stream_blocks(rng):
    n = int(rng.choice([64, 256, 1024, 1024, 4096]))
    pos, blocks = int(rng.integers(-600, 400)), []
    for _ in range(int(rng.integers(20, 60))):
        what = rng.random()
        if what < 0.04:
            pos += int(rng.integers(1, 5000))                    # a seek forward
        elif what < 0.07:
            pos -= int(rng.integers(1, 3 * n))                   # a step back (overlapping pull)
        size = n if rng.random() < 0.95 else int(rng.choice([1, 17, 3 * n]))
        blocks.append([pos, size])
        pos += size
    return blocks


def _contiguous(pos, sizes):
    blocks = []
    for n in sizes:
        blocks.append([pos, n])
        pos += n
    return blocks


_PATTERNS = {"short": (1, _short_blocks), "long": (2, _long_blocks), "stream": (3, _stream_blocks)}


def make_case(pattern, seed):
    """The case `seed` of a pull pattern ("short", "long", "stream").  A draw whose stateful AnalogOscPE comes within
    1e-9 of a discontinuity of its waveform on these pulls is drawn again (the reference is undefined within rounding
    of a wrap: tests/test_sources_host.py)."""
    tag, blocks_of = _PATTERNS[pattern]
    for attempt in range(100):
        rng = np.random.default_rng([tag, seed, attempt])
        g, _ = _draw_graph(rng)
        case = {"name": f"all_{pattern}_{seed}", "sr": int(rng.choice([22050, 44100, 48000])), "graph": g,
                "blocks": blocks_of(rng)}
        case["keep"] = list(range(len(case["blocks"])))
        if osc_edge_distance(case) > 1e-9:
            return case
    raise RuntimeError(f"no draw for {pattern} seed {seed} keeps its oscillators away from their edges")


def short_case(seed):
    return make_case("short", seed)


def long_case(seed):
    return make_case("long", seed)


def stream_case(seed):
    return make_case("stream", seed)


def _has_stateful_osc(g) -> bool:
    if isinstance(g, list):
        return any(_has_stateful_osc(x) for x in g)
    if not isinstance(g, dict):
        return False
    if g.get("pe") == "AnalogOscPE" and any(isinstance(g.get(p), dict) for p in ("frequency", "duty_cycle")):
        return True
    return any(_has_stateful_osc(v) for v in g.values())


def osc_edge_distance(case) -> float:
    """Smallest distance from a waveform edge of any restated phase of a stateful AnalogOscPE in the case, over all its
    blocks (inf when there is none): the oracle renders the case and its oscillators record their phases."""
    if not _has_stateful_osc(case["graph"]):
        return np.inf
    from oracle.graph_eval import make_node
    root = make_node(case["graph"], case["sr"])
    for s, n in case["blocks"]:
        root.render(int(s), int(n))
    return _min_edge(root, set())


def _min_edge(node, seen) -> float:
    if id(node) in seen:
        return np.inf
    seen.add(id(node))
    d = getattr(node, "osc_edge", np.inf)
    for s in node.sub.values():
        for x in (s if isinstance(s, list) else [s]):
            d = min(d, _min_edge(x, seen))
    return d
