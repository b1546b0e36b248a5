"""What every family of golden-case tests does with its fixture, once: load tests/golden/<family>_cases.json and
<family>.npz, split the stored samples into blocks, render a graph block by block in a started NullRenderer with the
case's lifecycle calls, and hold the result to the rule the fixture names -- to the bit, within a bound of the case's
peak, or per block within a relative tolerance of the block's peak plus a floor.

Where two families' rules differ the difference is an argument (`silent`, `reset`, `floor`, `tag`), never the laxer
rule.  The fixture generators (tools/gen_golden_*.py, oracle/gen_golden.py) use the same loader, lifecycle and rules
over the reference's classes."""

import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

PEAK_BOUND = 1e-6          # re-associated float64 sums rounded to float32: max abs error <= 1e-6 * peak of the case
REL_TOL = 1e-5             # a filter, an oscillator or an envelope in the graph, per block: REL_TOL * peak + a floor
ABS_FLOOR = 1e-6           # the floor of tests/test_gpu_fuzz.py
SCORE_ABS_FLOOR = 1e-7     # the floor of tests/test_gpu_parity.py, where the score family's float sources are tested


# ---------------------------------------------------------------------------------------------- fixtures
def paths(family):
    """-> (path of the json, path of the npz) of a family's fixture."""
    return os.path.join(GOLDEN_DIR, f"{family}_cases.json"), os.path.join(GOLDEN_DIR, f"{family}.npz")


def load_cases(family):
    """-> (the json document, the opened npz)."""
    cases_path, npz_path = paths(family)
    with open(cases_path) as f:
        return json.load(f), np.load(npz_path)


def stored_blocks(case):
    """Indices of the blocks whose samples the fixture keeps (every `keep_every`-th; all by default)."""
    k = int(case.get("keep_every", 1))
    return [i for i in range(len(case["blocks"])) if i % k == 0]


def split_blocks(case, flat):
    """The fixture's concatenated samples -> {block index: samples} for the stored blocks."""
    out, at = {}, 0
    for i in stored_blocks(case):
        n = int(case["blocks"][i][1])
        out[i] = flat[at:at + n]
        at += n
    assert at == len(flat), f"{case.get('name')}: the stored blocks hold {at} frames, the fixture {len(flat)}"
    return out


# ---------------------------------------------------------------------------------------------- rendering
def render_blocks(pe, sr, blocks, ops=None, reset=None, renderer=None, render=None):
    """Every block, in order, of `pe` in a started NullRenderer -> list of float32 arrays.  ops: {block index: "restart"
    (stop + start of the renderer) | "reset" (the `reset` callable)}, applied before that block.  renderer: pygmu2_amd's
    NullRenderer by default; render(start, n): another way to pull one block (the default is pe.render(start, n).data)."""
    if renderer is None:
        import pygmu2_amd as pg
        renderer = pg.NullRenderer(sample_rate=sr)
    if render is None:
        def render(start, n):
            return np.array(pe.render(start, n).data, dtype=np.float32)
    ops = {int(k): v for k, v in (ops or {}).items()}
    renderer.set_source(pe)
    renderer.start()
    outs = []
    for i, (s, n) in enumerate(blocks):
        if ops.get(i) == "restart":
            renderer.stop()
            renderer.start()
        elif ops.get(i) == "reset":
            reset()
        outs.append(render(int(s), int(n)))
    renderer.stop()
    return outs


def reset_all(made):
    for m in made:
        m.reset_state()


# ---------------------------------------------------------------------------------------------- comparisons
def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def max_err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def within(rule, got, want, peak, silent="fail"):
    """The three rules as a predicate (the generators hold the restatements to them): "bits"; "peak" -- of the case's
    `peak`; anything else -- of `want`'s own peak.  silent="zero": a silent case must be equal whatever its rule."""
    if got.shape != want.shape:
        return False
    if rule == "bits" or (silent == "zero" and peak == 0.0):
        return bits_equal(got, want) if rule == "bits" else bool(np.array_equal(got, want))
    if rule == "peak":
        return max_err(got, want) <= PEAK_BOUND * peak
    return max_err(got, want) <= REL_TOL * float(np.max(np.abs(want))) + ABS_FLOOR


def report(tag, name, err, peak, ratio=None):
    """The one line a measured comparison prints before it asserts."""
    print(f"{tag} {name} max_abs_err={err:.3e} peak={peak:.3e}" + ("" if ratio is None else f" ratio={ratio:.3e}"))


def assert_bits(name, got, want):
    if not bits_equal(got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        differ = (np.ascontiguousarray(got, np.float32).view(np.uint32)
                  != np.ascontiguousarray(want, np.float32).view(np.uint32)).reshape(-1)
        raise AssertionError(f"{name}: differs in {int(np.sum(differ))} of {d.size} samples, max {float(d.max()):.3g}, "
                             f"first at {int(np.argmax(differ))}")


def assert_peak(name, got, want, bound, tag, silent="fail", peak=None):
    """max abs error <= bound * peak, printed first.  peak: of `want` unless the fixture recorded the case's own.
    A silent expectation (peak 0) fails under silent="fail"; under silent="zero" `got` must then be exactly zero."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    peak = (float(np.max(np.abs(want))) if want.size else 0.0) if peak is None else float(peak)
    err = max_err(got, want)
    report(tag, name, err, peak, err / peak if peak else (0.0 if silent == "zero" else float("nan")))
    if peak == 0.0 and silent == "zero":
        assert not np.any(got), f"{name}: a silent case must be exactly zero"
        return
    assert peak > 0.0, f"{name}: a silent case has no peak to compare against"
    assert err <= bound * peak, f"{name}: max abs error {err:.3e} > {bound:g} * peak {peak:.3e}"


def assert_per_block(name, outs, stored, rel, floor, tag, numbered=True):
    """Each stored block by its own peak: max abs error <= rel * peak of the block + floor, printed first.
    outs: the rendered blocks by index; stored: {block index: expected samples}."""
    for i, want in stored.items():
        got = np.asarray(outs[i])
        label = f"{name} block {i}" if numbered else f"{name} block"
        assert got.shape == want.shape, f"{label}: shape {got.shape} != {want.shape}"
        peak = float(np.max(np.abs(want))) if want.size else 0.0
        err = max_err(got, want)
        report(tag, label, err, peak)
        assert err <= rel * peak + floor, f"{name} block {i}: {err:.3e} > {rel:g} * peak {peak:.3e} + {floor:g}"


def check_case(case, npz, build, reset=reset_all, tag="ERR", peak_tag=None, renderer=None):
    """Device render of every stored block against the fixture, in full, by the case's rule: "bits"; "peak" -- max abs
    error <= PEAK_BOUND * peak of the case, which may not be silent; "fuzz" / "gain" -- per block REL_TOL * peak of the
    block + ABS_FLOOR.  build(case) -> (root PE, the PEs that `reset` gets on a "reset" op).  A case that is not held
    to the bit prints its measured error before it asserts."""
    pe, made = build(case)
    outs = render_blocks(pe, case["sr"], case["blocks"], case.get("ops"), lambda: reset(made), renderer)
    flat = npz[case["name"]]
    stored = split_blocks(case, flat)
    assert stored
    if case["compare"] == "bits":
        for i, want in stored.items():
            assert_bits(f"{case['name']} block {i}", outs[i], want)
    elif case["compare"] == "peak":
        assert_peak(case["name"], np.concatenate([outs[i] for i in stored]), flat, PEAK_BOUND, peak_tag or tag)
    else:
        assert case["compare"] in ("fuzz", "gain"), case["compare"]
        assert_per_block(case["name"], outs, stored, REL_TOL, ABS_FLOOR, tag)
