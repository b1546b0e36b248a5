"""GPU: every golden family and every bank test once more, with a guard band round each device allocation the PE layer
makes and the payload poisoned (tests/guarded_alloc.py).  The other GPU modules compare the n * channels samples a
kernel was asked to write; this one asks what else was written -- past an output, a workspace or a state record -- and
whether scratch is read before it is written.  Neither shows in pool memory: pgx_malloc rounds every request up to a
power of two, so an overrun lands in slack the buffer owns, and a recycled block hands a stale but plausible value to a
kernel that reads what it never wrote.

* Positive controls: three floats written past a buffer, four bytes written before one, a buffer read unwritten.  All
  three stay inside the test's own allocation.
* Every case of every golden family (cases.json, channels, fuzz corpus, control, playback, noise, sources, tralfam,
  tuning, score, random_select, reverse_echo), built, rendered and compared by its own GPU module's function, inside
  `with guarded():` -- with look-ahead / read-ahead windows on (the default) and then off.  With windows on a
  contiguous pull is rendered a window at a time and the ragged block lengths (1, 17, 257, 1000, 4099) never reach a
  kernel as a launch of their own; with windows off they do.  One pytest id per (family, case); a failure names the
  windows setting it happened under.
* The bank modules' functions (their rule is "equals the unbanked render"), called as they stand.
* The coverage condition: every sizing function of include/pygmu_hip.h that the PE layer calls was asked for a size
  inside a guarded block, so its formula was held against its kernels' indexing at least once.

Each sweep prints `GUARD_BANDS <family> cases=<n> allocations=<n> exact_fit=<n>` at the end (pytest -s shows it)."""

import collections
import glob
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import guarded_alloc
from guarded_alloc import G, GuardViolation, guarded

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOTALS = collections.defaultdict(lambda: {"cases": 0, "allocations": 0, "exact_fit": 0})
SIZING = collections.Counter()
RAN = set()


def _tally(family, test_id, g):
    t = TOTALS[family]
    t["cases"] += 1
    t["allocations"] += g.allocations
    t["exact_fit"] += g.exact_fit
    SIZING.update(g.sizing_calls)
    RAN.add(test_id)


# ---------------------------------------------------------------------------------------------- positive controls
def _device():
    from pygmu2_amd import device
    return device.ensure_init(), device


@pytest.mark.parametrize("n", [1024, 1000], ids=["exact_fit", "with_slack"])
def test_three_floats_past_the_end_are_reported(n):
    lib, device = _device()
    with pytest.raises(GuardViolation) as e:
        with guarded() as g:
            buf = device.DeviceBuffer((n,), np.float32)
            device.check(lib.pgx_fill(buf.ptr, n + 3, 1.1), "pgx_fill")        # three floats into its own back guard
    (v,) = e.value.violations
    assert (v.bytes, v.side, v.first, v.last) == (4 * n, "back", 0, 11)
    assert [w.split("/")[0] for w in v.words] == ["3f8ccccd"] * 3
    assert v.stack and v.stack[0][0].endswith("device.py")
    assert (g.allocations, g.exact_fit) == (1, 1 if n == 1024 else 0)


def test_four_bytes_before_the_start_are_reported():
    lib, device = _device()
    word = np.array([0x12345678], dtype="<u4")
    with pytest.raises(GuardViolation) as e:
        with guarded():
            buf = device.DeviceBuffer((256,), np.float32)
            device.check(lib.pgx_memcpy_h2d(buf.ptr - 4, word.ctypes.data, 4), "pgx_memcpy_h2d")   # its own front guard
    (v,) = e.value.violations
    assert (v.bytes, v.side, v.first, v.last) == (1024, "front", -4, -1)
    assert v.words == [f"12345678/{0xFFF00000 | (G // 4 - 1):08x}"]


def test_a_buffer_that_is_only_read_delivers_nan():
    _, device = _device()
    with guarded() as g:
        assert np.all(np.isnan(device.DeviceBuffer((1000,), np.float32).to_host()))
        assert np.all(np.isnan(device.DeviceBuffer((333,), np.float64).to_host()))
        assert np.all(device.DeviceBuffer((7,), np.int32).to_host() == -1)
        assert not np.any(device.DeviceBuffer((1000,), np.float32, zero=True).to_host())
    assert g.allocations == 4 and not g.violations
    with guarded(poison=False):
        device.DeviceBuffer((1000,), np.float32).to_host()                      # whatever the pool held: no claim


def test_a_write_of_exactly_the_payload_reports_nothing_and_the_buffer_outlives_the_block():
    lib, device = _device()
    with guarded() as g:
        buf = device.DeviceBuffer((1024,), np.float32)
        assert buf.ptr % 256 == 0
        device.check(lib.pgx_fill(buf.ptr, 1024, 0.5), "pgx_fill")
    assert (g.allocations, g.exact_fit, g.violations) == (1, 1, [])
    assert np.all(buf.to_host() == 0.5)
    del buf                                             # freed after the block: by its raw pointer, through the wrapper
    assert device.DeviceBuffer((16,), np.float32).ptr   # and the pool goes on working


# ---------------------------------------------------------------------------------------------- the golden families
class _Windows:
    """Look-ahead and read-ahead windows switched for the length of a `with`."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from pygmu2_amd import look_ahead, read_ahead
        self.was = (look_ahead.enabled(), read_ahead.enabled())
        if not self.on:
            look_ahead.set_enabled(False)
            read_ahead.set_enabled(False)

    def __exit__(self, *exc):
        from pygmu2_amd import look_ahead, read_ahead
        look_ahead.set_enabled(self.was[0])
        read_ahead.set_enabled(self.was[1])
        return False


_npz = {}


def _load(name):
    if name not in _npz:
        _npz[name] = np.load(os.path.join(GOLDEN, name))
    return _npz[name]


def _parity():
    import test_gpu_parity as m
    return [(c["name"], lambda fx, c=c: m.test_hip_matches_reference_golden(c, fx["golden_data"])) for c in m.CASES]


def _channels():
    import test_gpu_channels as m
    return [(c["name"], lambda fx, c=c: m._check(c, _load("channels.npz"))) for c in m.CASES]      # "long" and stream too


def _fuzz():
    import test_gpu_fuzz_all as m
    return [(c["name"], lambda fx, c=c: m.test_hip_matches_reference_corpus(c, _load("fuzz.npz"))) for c in m.CORPUS]


def _harness_family(common, family):
    def cases():
        import importlib
        from fixture_harness import load_cases
        check = importlib.import_module(common).check_case
        data, npz = load_cases(family)
        return [(c["name"], lambda fx, c=c: check(c, npz)) for c in data["cases"]]      # the family's fuzz cases too
    return cases


def _sources():
    import test_gpu_analog_osc as osc
    import test_gpu_examples_sources as ex
    import test_gpu_karplus_strong as ks
    run = {"osc": osc.test_goldens, "ks": ks.test_goldens_bit_exact, "example": ex.test_example_graph}
    return [(c["name"], lambda fx, c=c: run[c["kind"]](c)) for c in ex.DATA["cases"]]


def _tuning():
    import pygmu2_amd as pg
    import test_gpu_tuning as m
    import tuning_oracle as T

    def run(c):
        T.default_tuning(pg)                            # the module's autouse fixture
        try:
            m.check_case(c)
        finally:
            T.default_tuning(pg)
    return [(c["name"], lambda fx, c=c: run(c)) for c in m.CASES]


def _score():
    import test_gpu_score as m

    def run(fx, c):
        fx["monkeypatch"].setattr(m, "_RENDERS", {})    # the module shares renders between its tests: render here
        m.test_fixture_cases_match_the_reference(c)
    return [(c["name"], lambda fx, c=c: run(fx, c)) for c in m.CASES]


def _random_select():
    import pygmu2_amd as pg
    import test_gpu_random_select as m
    from pygmu2_amd import restart_bank

    def run(c, p):
        pg.set_sample_rate(m.DATA["sr"])                # the module's autouse fixture
        was = restart_bank.enabled()
        restart_bank.set_enabled(True)
        try:
            m.test_cases_match_the_reference(c, p)
        finally:
            restart_bank.set_enabled(was)
    return [(i, lambda fx, c=c, p=p: run(c, p)) for (c, p), i in zip(m.RUNS, m.RUN_IDS)]


def _reverse_echo():
    import fixture_harness as H
    import reverse_echo_common as RC
    import test_gpu_reverse_echo as m
    return [(i, lambda fx, c=c: H.check_case(c, m.NPZ, RC.build_case, tag=RC.TAG)) for i, c in m.EVERY]


FAMILIES = [
    ("cases", _parity), ("channels", _channels), ("fuzz", _fuzz),
    ("control", _harness_family("control_gpu_common", "control")),
    ("playback", _harness_family("playback_gpu_common", "playback")),
    ("noise", _harness_family("noise_gpu_common", "noise")),
    ("sources", _sources),
    ("tralfam", _harness_family("tralfam_gpu_common", "tralfam")),
    ("tuning", _tuning), ("score", _score), ("random_select", _random_select), ("reverse_echo", _reverse_echo),
]
SWEEP = [(family, name, run) for family, cases in FAMILIES for name, run in cases()]
SWEEP_IDS = [f"{family}-{name}" for family, name, _ in SWEEP]
assert len(set(SWEEP_IDS)) == len(SWEEP_IDS)


@pytest.mark.parametrize("entry", SWEEP, ids=SWEEP_IDS)
def test_golden_case_under_guards(entry, golden_data, monkeypatch):
    """One id per (family, case): the case is rendered and compared twice, with windows on and with windows off, and a
    failure says under which (both are always run).  One id per setting as well would take the GPU suite past 5 000 ids."""
    family, name, run = entry
    fx = {"golden_data": golden_data, "monkeypatch": monkeypatch}
    failures = []
    for windows in (True, False):
        setting = "windows on" if windows else "windows off"
        try:
            with _Windows(windows):
                with guarded() as g:
                    try:
                        run(fx)
                    finally:
                        _tally(family if windows else family + "/windows_off", f"{family}-{name}-{windows}", g)
        except Exception as e:                          # (a skip of the family's own is no Exception: it stands)
            failures.append((setting, e))
    if failures:
        text = "\n".join(f"{family}-{name}, {setting}: {type(e).__name__}: {e}" for setting, e in failures)
        raise AssertionError(text) from failures[0][1]


# ---------------------------------------------------------------------------------------------- no family reaches these
# pgx_dft_workspace_bytes: TralfamPE sizes its own workspace (pgx_tralfam_workspace_bytes); the plain transform is
# reached through spectral.dft alone, which is no PE and has no golden family.  tests/test_gpu_dft.py's own function and
# bound against numpy.fft, at the lengths where pgx_dft_c2c changes its path: one point, Bluestein over an LDS
# transform (3, 7, 1000), the LDS Stockham FFT (128, 2048), its four-step form (4096) and Bluestein over that (4097).
DFT_LENGTHS = (1, 3, 7, 128, 1000, 2048, 4096, 4097)


@pytest.mark.parametrize("n", DFT_LENGTHS)
def test_dft_under_guards(n):
    import test_gpu_dft as m
    from pygmu2_amd import spectral
    spectral.plan_for.cache_clear()                     # a plan made earlier has no guards: make this length's here
    with guarded() as g:
        try:
            m.test_dft_matches_numpy(n)
        finally:
            _tally("dft", f"dft-{n}", g)


# ---------------------------------------------------------------------------------------------- the banks
BANK_MODULES = ("test_gpu_voice_bank", "test_gpu_voice_tiles", "test_gpu_analog_bank", "test_gpu_supersaw_segments")
BANK_SKIPPED = {
    # "<module>::<function>": why it is not run a second time here.  Empty: the slowest of the functions taken runs
    # for 0.4 s under guards (profiles/guard_bands.md).
}


def _parameter_sets(fn):
    """A test function's own parametrize marks -> [(id, kwargs)], or None if it needs a fixture besides monkeypatch."""
    marks = list(getattr(fn, "pytestmark", []))
    if any(m.name == "usefixtures" for m in marks):
        return None
    axes = []
    for m in marks:
        if m.name != "parametrize":
            continue
        names = [s.strip() for s in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        rows = []
        for v in m.args[1]:
            if hasattr(v, "values") and hasattr(v, "marks"):        # pytest.param(...)
                values = tuple(v.values)
            else:
                values = tuple(v) if len(names) > 1 else (v,)
            rows.append(dict(zip(names, values)))
        axes.append(rows)
    given = {k for rows in axes for k in rows[0]}
    needs = set(inspect.signature(fn).parameters) - given
    if needs - {"monkeypatch"}:
        return None
    out = []
    for combo in itertools.product(*axes):
        kw = {}
        for row in combo:
            kw.update(row)
        label = "-".join(re.sub(r"[^A-Za-z0-9_.]+", "_", v if isinstance(v, str) else getattr(v, "__name__", None) or repr(v))
                         for v in kw.values())
        out.append((label, kw, "monkeypatch" in needs))
    return out


def _bank_entries():
    import importlib
    out = []
    for mod in BANK_MODULES:
        m = importlib.import_module(mod)
        for name, fn in sorted(vars(m).items()):
            if not name.startswith("test_") or not inspect.isfunction(fn) or fn.__module__ != mod:
                continue
            if f"{mod}::{name}" in BANK_SKIPPED:
                continue
            sets = _parameter_sets(fn)
            for label, kw, wants_mp in sets or []:
                out.append((f"{mod[9:]}-{name[5:]}" + (f"-{label}" if label else ""), fn, kw, wants_mp))
    return out


BANKS = _bank_entries()


@pytest.mark.parametrize("entry", BANKS, ids=[e[0] for e in BANKS])
def test_bank_function_under_guards(entry, monkeypatch):
    test_id, fn, kw, wants_monkeypatch = entry
    if wants_monkeypatch:
        kw = dict(kw, monkeypatch=monkeypatch)
    with guarded() as g:
        try:
            fn(**kw)
        finally:
            _tally("banks", test_id, g)


# ---------------------------------------------------------------------------------------------- the coverage condition
def sizing_functions_the_pe_layer_calls():
    from pygmu2_amd import device
    text = ""
    for path in glob.glob(os.path.join(ROOT, "pygmu2_amd", "*.py")):
        if os.path.basename(path) != "device.py":
            with open(path) as f:
                text += f.read()
    return sorted(n for n in device.EXPORTED_SYMBOLS if guarded_alloc.is_sizing_name(n) and re.search(rf"\b{n}\b", text))


def test_every_sizing_function_was_asked_under_guards():
    """Last in the module: sums what the sweeps above saw."""
    expected = ({f"{f}-{n}-{w}" for f, n, _ in SWEEP for w in (True, False)} | {e[0] for e in BANKS}
                | {f"dft-{n}" for n in DFT_LENGTHS})
    for family in sorted(TOTALS):
        print(f"GUARD_BANDS {family} " + " ".join(f"{k}={v}" for k, v in TOTALS[family].items()))
    for name in sorted(SIZING):
        print(f"GUARD_BANDS_SIZING {name} calls={SIZING[name]}")
    if not expected <= RAN:
        pytest.skip(f"{len(expected - RAN)} of {len(expected)} guarded runs were not part of this session")
    allocations = sum(t["allocations"] for t in TOTALS.values())
    exact_fit = sum(t["exact_fit"] for t in TOTALS.values())
    print(f"GUARD_BANDS total allocations={allocations} exact_fit={exact_fit}")
    assert allocations > 0 and exact_fit > 0
    wanted = sizing_functions_the_pe_layer_calls()
    for prefix in guarded_alloc.SIZING_PREFIXES:
        assert any(n.startswith(prefix) for n in wanted), f"no sizing function {prefix}* is called by the PE layer"
    missing = [n for n in wanted if not SIZING[n]]
    assert not missing, f"never asked for a size inside a guarded block: {missing}"
