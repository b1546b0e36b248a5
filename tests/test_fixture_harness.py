"""CPU: the SPEC builder's table (oracle/spec_builder.py) over a namespace of recording stubs, and the comparison rules,
block bookkeeping and render lifecycle of tests/fixture_harness.py."""

import json
import os

import numpy as np
import pytest

import fixture_harness as H
from oracle import spec_builder as B

SPEC_FIXTURES = ("cases.json", "fuzz_cases.json", "channels_cases.json", "playback_cases.json", "control_cases.json",
                 "noise_cases.json")


class Stubs:
    """A namespace whose every class records (kind, args, kwargs) in `calls` and returns that triple; an enum gives
    (enum name, string), transform_func ("func", ops)."""

    def __init__(self):
        self.calls = []

    def transform_func(self, ops):
        return ("func", ops)

    def __getattr__(self, name):
        if name.endswith("Mode"):
            return lambda value: (name, value)

        def make(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return self.calls[-1]
        return make


LEAF = {"pe": "ConstantPE", "value": 1.0}
MADE = ("ConstantPE", (), {"value": 1.0})

# kind -> (the SPEC's keywords, the positional arguments expected, the keyword arguments expected)
EXPECT = {
    "MixPE": ({"inputs": [LEAF, LEAF]}, (MADE, MADE), {}),
    "PiecewisePE": ({"points": [[0, 1], [10.0, 2]], "extend_mode": "hold_both"}, (),
                    {"points": [(0, 1.0), (10, 2.0)], "extend_mode": ("ExtendMode", "hold_both")}),
    "TransformPE": ({"source": LEAF, "ops": [["abs"]]}, (MADE,), {"func": ("func", [["abs"]]), "name": "ops"}),
    "BiquadPE": ({"source": LEAF, "mode": "lowpass", "q": 2.0}, (), {"source": MADE, "mode": ("BiquadMode", "lowpass"),
                                                                      "q": 2.0}),
    "SVFilterPE": ({"source": LEAF, "mode": "highpass"}, (), {"source": MADE, "mode": ("BiquadMode", "highpass")}),
    "LadderPE": ({"source": LEAF, "mode": "LP24"}, (), {"source": MADE, "mode": ("LadderMode", "LP24")}),
    "EnvelopePE": ({"source": LEAF, "mode": "rms"}, (), {"source": MADE, "mode": ("DetectionMode", "rms")}),
    "WindowPE": ({"source": LEAF, "mode": "max"}, (), {"source": MADE, "mode": ("WindowMode", "max")}),
    "DynamicsPE": ({"source": LEAF, "envelope": LEAF, "mode": "gate"}, (),
                   {"source": MADE, "envelope": MADE, "mode": ("DynamicsMode", "gate")}),
    "NoisePE": ({"seed": 3, "mode": "pink"}, (), {"seed": 3, "mode": ("NoiseMode", "pink")}),
    "DelayPE": ({"source": LEAF, "delay": 1.5, "interpolation": "cubic"}, (),
                {"source": MADE, "delay": 1.5, "interpolation": ("InterpolationMode", "cubic")}),
    "ConvolvePE": ({"fir": LEAF, "src": LEAF, "fft_threshold": 8}, (MADE, MADE), {"fft_threshold": 8}),
    "ReverbPE": ({"source": LEAF, "ir": LEAF, "normalize": True}, (MADE, MADE, 0.5), {"normalize": True}),
    "LoopPE": ({"source": LEAF, "count": 3}, (MADE,), {"count": 3}),
    "CachePE": ({"source": LEAF}, (MADE,), {}),
    "TriggerRestartPE": ({"src": LEAF, "trigger": LEAF}, (MADE, MADE), {}),
    "CompressorPE": ({"source": LEAF, "detection": "peak", "ratio": 4.0}, (MADE,),
                     {"detection": ("DetectionMode", "peak"), "ratio": 4.0}),
    "LimiterPE": ({"source": LEAF, "detection": "rms"}, (MADE,), {"detection": ("DetectionMode", "rms")}),
    "ExpanderPE": ({"source": LEAF, "detection": "rms"}, (MADE,), {"detection": ("DetectionMode", "rms")}),
    "WavetablePE": ({"indexer": LEAF, "wavetable": LEAF, "interpolation": "linear", "out_of_bounds": "wrap"},
                    (MADE, MADE), {"interpolation": ("InterpolationMode", "linear"),
                                   "out_of_bounds": ("OutOfBoundsMode", "wrap")}),
    "TimeWarpPE": ({"source": LEAF, "rate": 1.5, "interpolation": "cubic"}, (MADE,),
                   {"rate": 1.5, "interpolation": ("InterpolationMode", "cubic")}),
    "SampleHoldPE": ({"trigger": LEAF, "source": LEAF, "initial_value": 0.1}, (MADE, MADE), {"initial_value": 0.1}),
    "TrackHoldPE": ({"gate": LEAF, "source": LEAF}, (MADE, MADE), {}),
    "SlewLimiterPE": ({"source": LEAF, "rise_rate": 5.0, "mode": "linear"}, (MADE,),
                      {"rise_rate": 5.0, "mode": ("SlewMode", "linear")}),
}
PLAIN = sorted(k for k, row in B.TABLE.items() if row is B.PLAIN)
SPATIAL = {"adapter": ({"channels": 2}, ("SpatialAdapter", (2,), {})),
           "linear": ({"azimuth": 30.0}, ("SpatialLinear", (30.0,), {})),
           "constant_power": ({"azimuth": -45.0}, ("SpatialConstantPower", (-45.0,), {})),
           "hrtf": ({"azimuth": 30.0, "elevation": 10.0}, ("hrtf", (30.0, 10.0), {}))}


def committed_specs():
    for name in SPEC_FIXTURES:
        with open(os.path.join(H.GOLDEN_DIR, name)) as f:
            doc = json.load(f)
        for case in (doc["cases"] if isinstance(doc, dict) else doc):
            yield case["graph"]


# ---------------------------------------------------------------------------------------------- the table
def test_every_kind_of_the_committed_fixtures_has_a_row():
    kinds = B.kinds_of(list(committed_specs()))
    assert len(kinds) > 40 and kinds <= set(B.TABLE), sorted(kinds - set(B.TABLE))
    assert set(EXPECT) | set(PLAIN) | {"SpatialPE"} == set(B.TABLE)


@pytest.mark.parametrize("kind", sorted(EXPECT))
def test_row_gives_the_expected_constructor_call(kind):
    keywords, args, kwargs = EXPECT[kind]
    K = Stubs()
    pe = B.build(dict({"pe": kind}, **keywords), K)
    assert pe == (kind, args, kwargs) and K.calls[-1] == pe


@pytest.mark.parametrize("kind", PLAIN)
def test_plain_row_passes_keywords_through(kind):
    K = Stubs()
    spec = {"pe": kind, "source": LEAF, "data": {"values": [1.0, 2.0]}, "x": 2, "extend_mode": "zero"}
    name, args, kwargs = B.build(spec, K)
    assert (name, args) == (kind, ()) and sorted(kwargs) == ["data", "extend_mode", "source", "x"]
    assert kwargs["source"] == MADE and kwargs["x"] == 2 and kwargs["extend_mode"] == ("ExtendMode", "zero")
    assert kwargs["data"].dtype == np.float32 and kwargs["data"].tolist() == [1.0, 2.0]


@pytest.mark.parametrize("method", sorted(SPATIAL))
def test_spatial_row_builds_its_method_object(method):
    keywords, made_method = SPATIAL[method]
    K = Stubs()
    pe = B.build(dict({"pe": "SpatialPE", "source": LEAF, "method": method}, **keywords), K)
    assert pe == ("SpatialPE", (MADE,), {"method": made_method})
    assert K.calls == [MADE, made_method, pe]


def test_reverb_mix_is_positional_when_the_spec_has_it():
    pe = B.build({"pe": "ReverbPE", "mix": 0.25, "ir": LEAF, "source": LEAF}, Stubs())
    assert pe == ("ReverbPE", (MADE, MADE, 0.25), {})


def test_shared_nodes_are_built_once_and_on_make_sees_construction_order():
    shared_leaf = dict(LEAF, share="c")
    spec = {"pe": "MixPE", "inputs": [{"pe": "GainPE", "gain": shared_leaf, "source": {"pe": "SinePE", "frequency": 2.0}},
                                      shared_leaf, {"pe": "NoisePE", "seed": 1}]}
    K, seen = Stubs(), []
    root = B.build(spec, K, on_make=lambda kind, pe: seen.append((kind, pe)))
    assert [k for k, _ in seen] == ["ConstantPE", "SinePE", "GainPE", "NoisePE", "MixPE"]
    assert [pe for _, pe in seen] == K.calls and seen[-1][1] is root
    assert root[1][1] is root[1][0][2]["gain"]                 # the one shared instance, twice
    store = {}
    first = B.build(shared_leaf, K, store)
    assert B.build(shared_leaf, K, store) is first and len(K.calls) == 6


@pytest.mark.parametrize("kind", ["WavetablePE", "TimeWarpPE", "SampleHoldPE", "TrackHoldPE", "SlewLimiterPE",
                                  "FunctionGenPE", "NoisePE"])
def test_newer_kind_builds_as_a_mix_input(kind):
    keywords = EXPECT[kind][0] if kind in EXPECT else {"frequency": LEAF}
    K = Stubs()
    root = B.build({"pe": "MixPE", "inputs": [LEAF, dict({"pe": kind}, **keywords)]}, K)
    assert root[0] == "MixPE" and root[1][1][0] == kind and K.calls[-2][0] == kind


def test_unknown_kind_is_an_error():
    with pytest.raises(KeyError, match="NoSuchPE"):
        B.build({"pe": "NoSuchPE"}, Stubs())


# ---------------------------------------------------------------------------------------------- comparisons
def test_assert_bits_sees_one_ulp_and_a_shape_mismatch():
    a = np.linspace(-1.0, 1.0, 64, dtype=np.float32).reshape(-1, 1)
    H.assert_bits("same", a, a.copy())
    b = a.copy()
    b[17, 0] = np.nextafter(b[17, 0], np.float32(2.0))
    with pytest.raises(AssertionError, match=r"differs in 1 of 64 samples, max .*, first at 17"):
        H.assert_bits("ulp", b, a)
    with pytest.raises(AssertionError, match="shape"):
        H.assert_bits("shape", a[:-1], a)
    with pytest.raises(AssertionError, match="differs in 1 of 2"):
        H.assert_bits("signed zero", np.array([0.0, -0.0], np.float32), np.zeros(2, np.float32))
    assert H.bits_equal(a, a.astype(np.float64)) and not H.bits_equal(a, b) and not H.bits_equal(a, a[:, 0])


def test_assert_peak_holds_the_bound_on_either_side(capsys):
    want = np.zeros((100, 1), np.float64)
    want[3, 0] = -0.5                                          # the peak
    for factor, passes in ((0.99, True), (1.01, False)):
        got = want.copy()
        got[50, 0] = factor * 1e-6 * 0.5
        if passes:
            H.assert_peak("near", got, want, 1e-6, "TAG_ERR")
        else:
            with pytest.raises(AssertionError, match="max abs error"):
                H.assert_peak("near", got, want, 1e-6, "TAG_ERR")
    assert capsys.readouterr().out.startswith("TAG_ERR near max_abs_err=4.950e-07 peak=5.000e-01 ratio=9.900e-07\n")
    with pytest.raises(AssertionError, match="shape"):
        H.assert_peak("shape", want[:-1], want, 1e-6, "TAG_ERR")
    H.assert_peak("given peak", want + 1.5e-6, want, 1e-6, "TAG_ERR", peak=2.0)       # the fixture's own peak


def test_assert_peak_and_a_silent_expectation():
    silent = np.zeros((10, 2), np.float32)
    one = silent.copy()
    one[4, 1] = 1e-30
    with pytest.raises(AssertionError, match="silent"):
        H.assert_peak("control rule", silent, silent, H.PEAK_BOUND, "TAG_ERR")
    H.assert_peak("tralfam rule", silent, silent, H.PEAK_BOUND, "TAG_ERR", silent="zero")
    with pytest.raises(AssertionError, match="exactly zero"):
        H.assert_peak("tralfam rule", one, silent, H.PEAK_BOUND, "TAG_ERR", silent="zero")


def test_assert_per_block_judges_each_block_by_its_own_peak(capsys):
    loud, quiet = np.full((8, 1), 100.0, np.float32), np.full((8, 1), 0.01, np.float32)
    stored = {0: loud, 2: quiet}
    outs = [loud, None, quiet + np.float32(2e-6)]              # 2e-6 > 1e-5 * 0.01 + 1e-6, but < 1e-5 * 100
    assert H.max_err(np.concatenate([outs[0], outs[2]]), np.concatenate([loud, quiet])) < H.REL_TOL * 100.0
    with pytest.raises(AssertionError, match="block 2"):
        H.assert_per_block("case", outs, stored, H.REL_TOL, H.ABS_FLOOR, "TAG_ERR")
    H.assert_per_block("case", [loud, None, quiet + np.float32(1e-6)], stored, H.REL_TOL, H.ABS_FLOOR, "TAG_ERR")
    assert "TAG_ERR case block 0 max_abs_err=0.000e+00 peak=1.000e+02\n" in capsys.readouterr().out
    with pytest.raises(AssertionError, match="shape"):
        H.assert_per_block("case", [loud[:-1], None, quiet], stored, H.REL_TOL, H.ABS_FLOOR, "TAG_ERR")


def test_within_is_the_same_three_rules():
    want = np.array([[0.5], [0.001]], np.float32)
    assert H.within("bits", want.copy(), want, 0.5) and not H.within("bits", want + np.float32(1e-7), want, 0.5)
    assert H.within("peak", want + np.float32(4e-7), want, 0.5) and not H.within("peak", want + np.float32(6e-7), want, 0.5)
    assert H.within("fuzz", want + np.float32(5e-6), want, 0.5) and not H.within("fuzz", want + np.float32(7e-6), want, 0.5)
    assert not H.within("fuzz", want[:1], want, 0.5)
    silent = np.zeros((2, 1), np.float32)
    assert H.within("peak", silent, silent, 0.0, silent="zero") and not H.within("peak", silent + 1e-30, silent, 0.0, silent="zero")


# ---------------------------------------------------------------------------------------------- blocks and lifecycle
def test_split_blocks_honours_keep_every_and_the_length():
    case = {"name": "c", "blocks": [[0, 3], [3, 5], [8, 2], [10, 4]], "keep_every": 2}
    assert H.stored_blocks(case) == [0, 2] and H.stored_blocks({"blocks": case["blocks"]}) == [0, 1, 2, 3]
    flat = np.arange(5, dtype=np.float32).reshape(-1, 1)
    split = H.split_blocks(case, flat)
    assert sorted(split) == [0, 2] and split[0][:, 0].tolist() == [0.0, 1.0, 2.0] and split[2][:, 0].tolist() == [3.0, 4.0]
    with pytest.raises(AssertionError):
        H.split_blocks(case, flat[:-1])
    with pytest.raises(AssertionError):
        H.split_blocks(dict(case, keep_every=1), flat)


class Log:
    """A stub PE and renderer in one: every call goes into `events`."""

    def __init__(self):
        self.events = []

    def set_source(self, pe):
        self.events.append(("set_source", pe))

    def start(self):
        self.events.append("start")

    def stop(self):
        self.events.append("stop")

    def render(self, start, n):
        self.events.append(("render", start, n))
        return type("Snippet", (), {"data": np.full((n, 1), start, np.float64)})()


def test_render_blocks_places_the_lifecycle_calls_before_the_blocks_the_ops_name():
    log = Log()
    outs = H.render_blocks(log, 48000, [[0, 4], [4, 4], [100, 2], [8, 1]], ops={"1": "reset", "3": "restart"},
                           reset=lambda: log.events.append("reset"), renderer=log)
    assert log.events == [("set_source", log), "start", ("render", 0, 4), "reset", ("render", 4, 4), ("render", 100, 2),
                          "stop", "start", ("render", 8, 1), "stop"]
    assert [o.shape for o in outs] == [(4, 1), (4, 1), (2, 1), (1, 1)] and all(o.dtype == np.float32 for o in outs)
    assert outs[2][0, 0] == 100.0
    log = Log()
    H.render_blocks(log, 48000, [[0, 1], [1, 1]], renderer=log, render=lambda s, n: log.events.append(("pull", s, n)))
    assert log.events == [("set_source", log), "start", ("pull", 0, 1), ("pull", 1, 1), "stop"]


def test_check_case_dispatches_on_the_rule_of_the_case():
    flat = np.array([[0.5], [0.25], [0.125]], np.float32)
    case = {"name": "c", "sr": 48000, "blocks": [[0, 2], [2, 1]], "ops": {"1": "reset"}, "compare": "bits"}
    resets = []

    def check(rule, off):
        pe = Log()
        pe.render = lambda s, n: type("Snippet", (), {"data": flat[s:s + n] + np.float32(off)})()
        H.check_case(dict(case, compare=rule), {"c": flat}, lambda c: (pe, ["made"]), reset=resets.append, tag="TAG_ERR",
                     renderer=pe)

    check("bits", 0.0)
    assert resets == [["made"]]
    with pytest.raises(AssertionError, match="c block 0: differs in 2 of 2"):
        check("bits", 1e-7)
    check("peak", 4e-7)
    with pytest.raises(AssertionError, match="max abs error"):
        check("peak", 6e-7)
    check("fuzz", 2e-6)
    with pytest.raises(AssertionError, match="block 1"):
        check("fuzz", 3e-6)
    with pytest.raises(AssertionError):
        check("other", 0.0)
