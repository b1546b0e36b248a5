"""
GPU: the interpolation family of csrc/pgx_lookup.hip through the C ABI -- pgx_index_range, pgx_wavetable_range,
pgx_stream_range, pgx_timewarp_scan, pgx_wavetable, pgx_interp_lookup, pgx_timewarp -- at every switch of their
dispatchers and at the edges the PE layer never reaches: a NaN anywhere in a range reduction, the tile loop and the
carry of the time-warp scan (more than 524 288 frames), either side of the staging switch of pgx_wavetable
(pgx_wavetable_plan says which branch a case took, and every case asserts it), neighbours clipped to a window that is
shorter than the indices reach, indices exactly on an extent and one ulp either side of it.

Every device buffer is a DeviceBuffer made inside guarded_alloc.guarded(): guard bands around each, outputs, the range
pair and the scan's workspace start as 0xFF bytes (NaN), inputs are read back and must be unchanged.

The references are the numpy restatements of tests/playback_oracle.py (linear_interp, cubic_interp, wavetable_indices,
timewarp_step: float64, the reference's expression order).  Everything but one layer is compared bit for bit:
  B1 ranges     np.min / np.max of the same float64 indices; NaN where numpy's are, +-inf where numpy's are.
  B2 scan       rates k / 2^20, |k| <= 2^22, exact in float32; with |pos0| <= 2^24 every partial sum of up to 1 050 625
                of them is a multiple of 2^-20 below 2^25 -- 45 bits, exact in float64 in any association order.
  B2 float      rates in [0.5, 2] against an np.longdouble cumsum.  Any order of summing m float64 terms errs by at
                most (m - 1) 2^-53 sum|x|; position i has i + 1 terms, the limit used is (i + 2) 2^-53 (|pos0| + sum|rate|).
  B3, B4        float32 outputs, the bits of the restatement's.
"""

import contextlib
import itertools
import types

import numpy as np
import pytest

from guarded_alloc import guarded
from lookup_plan import ENV, ENV_CASES, SWITCH_CASES, export
from playback_oracle import cubic_interp, linear_interp, timewarp_step, wavetable_indices

gpu = pytest.mark.gpu

BLOCK = 256                     # kBlock: the thread stride of the one-workgroup range kernels
MODES = ["zero", "clamp", "wrap"]
NAN, INF = float("nan"), float("inf")
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    from pygmu2_amd import device
    device.ensure_init()
    return device


@pytest.fixture(autouse=True)
def _default_staging_limit(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)


# ------------------------------------------------------------------------------------------------- harness
@contextlib.contextmanager
def _buffers(dev, **spec):
    """Guarded device buffers: an array is uploaded (and must come back unchanged), a (shape, dtype) pair stays 0xFF."""
    with guarded() as g:
        bufs = {k: dev.DeviceBuffer.from_host(v) if isinstance(v, np.ndarray) else dev.DeviceBuffer(*v)
                for k, v in spec.items()}
        ns = types.SimpleNamespace(**bufs)
        try:
            yield ns
            assert g.allocations == len(spec)
            for k, v in spec.items():
                if isinstance(v, np.ndarray) and k not in getattr(ns, "rewritten", ()):
                    assert _same_bits(bufs[k].to_host(), np.ascontiguousarray(v)), f"the call wrote its input {k!r}"
        finally:
            ns.__dict__.clear()
            bufs.clear()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _first_miss(got, want):
    bad = np.argwhere(_bits(got) != _bits(want))
    at = tuple(bad[0])
    return f"{bad.shape[0]} cells differ, first at {list(at)}: got {got[at]!r} want {want[at]!r}"


def _assert_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert _same_bits(got, want), f"{what}: {_first_miss(got, want)}"


@contextlib.contextmanager
def _collect(misses, what):
    """One combination of a test that walks several: a failed assertion (a damaged guard band is one) is noted under
    `what` and the walk goes on, so that the test's last line reports every combination that failed, not the first."""
    try:
        yield
    except AssertionError as e:
        misses.append(f"[{what}] {e}")


def _none(misses):
    assert not misses, f"{len(misses)} combination(s) failed:\n" + "\n".join(misses)


def _assert_range(got, lo, hi, what=""):
    """(min, max) as numpy has them: NaN where numpy's is, otherwise the same bits (+-inf included)."""
    want = np.array([lo, hi], dtype=F64)
    assert got.dtype == F64 and got.shape == (2,)
    for g, w, side in zip(got, want, ("min", "max")):
        if np.isnan(w):
            assert np.isnan(g), f"{what}: {side} is {g!r}, numpy's is NaN"
        else:
            assert _bits(np.array([g]))[0] == _bits(np.array([w]))[0], f"{what}: {side} is {g!r}, numpy's is {w!r}"


# ------------------------------------------------------------------------------------------------- B1: the ranges
RANGE_SIZES = [1, 255, 256, 257, 600, 4099]
RANGE_STARTS = [-37, 0, 1 << 40]
STREAM_PARTS = [1, 3, 1024]
WT_EXTENT = (5, 205)


def _special_frames(n):
    """Frame 0, frame n - 1, the last frame thread 0 visits, and frames that another frame of the same thread follows
    (f + 256 < n: what a per-thread fold that keeps a NaN only until the next element loses)."""
    frames = {0, n - 1, (n - 1) // BLOCK * BLOCK}
    frames |= {f for f in (3, 1000) if f + BLOCK < n}
    return sorted(frames)


NONFINITE = [("nan", NAN), ("pinf", INF), ("ninf", -INF)]
assert _special_frames(600) == [0, 3, 512, 599] and _special_frames(256) == [0, 255] and 1000 in _special_frames(4099)


def _control(rng, n):
    """A float32 control stream with fractions, both signs, neither extreme a zero."""
    x = rng.uniform(-300.0, 500.0, n).astype(F32)
    x[x == 0] = 1.0
    return x


def _index_range(dev, delay, start):
    lib = dev.ensure_init()
    with _buffers(dev, delay=delay, result=((2,), F64)) as b:
        dev.check(lib.pgx_index_range(b.result.ptr, b.delay.ptr, start, delay.shape[0]))
        return b.result.to_host()


def _indices_of(delay, start):
    n = delay.shape[0]
    return np.arange(start, start + n, dtype=np.int64).astype(F64) - delay.astype(F64)


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_index_range_is_numpy_s_min_and_max(dev, n):
    delay = _control(np.random.default_rng([n, 1]), n)
    misses = []
    for start in RANGE_STARTS:
        idx = _indices_of(delay, start)
        with _collect(misses, f"start={start}"):
            _assert_range(_index_range(dev, delay, start), np.min(idx), np.max(idx))
    _none(misses)


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_index_range_keeps_a_non_finite_delay(dev, n):
    misses = []
    for frame in _special_frames(n):
        for name, value in NONFINITE:
            delay = _control(np.random.default_rng([n, 2]), n)
            delay[frame] = value
            idx = _indices_of(delay, -37)
            assert not np.isfinite(idx[frame])
            with _collect(misses, f"n{n}-f{frame}-{name}"):
                _assert_range(_index_range(dev, delay, -37), np.min(idx), np.max(idx))
    _none(misses)


def _wavetable_range(dev, raw, mode, finite):
    lib = dev.ensure_init()
    with _buffers(dev, indexer=raw, result=((2,), F64)) as b:
        dev.check(lib.pgx_wavetable_range(b.result.ptr, b.indexer.ptr, raw.shape[0], MODES.index(mode), finite,
                                          float(WT_EXTENT[0]), float(WT_EXTENT[1])))
        return b.result.to_host()


def _processed(raw, mode, finite, extent=WT_EXTENT):
    with np.errstate(invalid="ignore"):                        # inf % length is NaN, as in the reference
        return wavetable_indices(raw.astype(F64), mode, extent if finite else (None, None))


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_wavetable_range_is_numpy_s_min_and_max(dev, n):
    raw = _control(np.random.default_rng([n, 3]), n)
    edges = np.array([WT_EXTENT[0], WT_EXTENT[1] - 1, WT_EXTENT[1], WT_EXTENT[0] - 200, WT_EXTENT[1] - 0.5], dtype=F32)
    if n >= 255:
        raw[7:7 + edges.size] = edges
    misses = []
    for mode in MODES:
        for finite in (0, 1):
            idx, _ = _processed(raw, mode, finite)
            with _collect(misses, f"{mode} finite={finite}"):
                _assert_range(_wavetable_range(dev, raw, mode, finite), np.min(idx), np.max(idx))
    _none(misses)


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_wavetable_range_keeps_a_non_finite_index(dev, n):
    misses = []
    for frame in _special_frames(n):
        for name, value in NONFINITE:
            raw = _control(np.random.default_rng([n, 4]), n)
            raw[frame] = value
            for mode in MODES:
                for finite in (0, 1):
                    idx, _ = _processed(raw, mode, finite)
                    if np.isnan(value):
                        assert np.isnan(idx[frame])
                    with _collect(misses, f"n{n}-f{frame}-{name} {mode} finite={finite}"):
                        _assert_range(_wavetable_range(dev, raw, mode, finite), np.min(idx), np.max(idx))
    _none(misses)


def _stream_range(dev, x, parts):
    """-> the (parts, 2) pairs; workgroups without a frame must answer (+inf, -inf)."""
    lib = dev.ensure_init()
    n = x.shape[0]
    with _buffers(dev, x=x, partials=((parts, 2), F64)) as b:
        dev.check(lib.pgx_stream_range(b.partials.ptr, parts, b.x.ptr, n))
        pairs = b.partials.to_host()
    idle = pairs[-(-n // BLOCK):]
    assert np.all(idle[:, 0] == INF) and np.all(idle[:, 1] == -INF), "a workgroup without a frame"
    return pairs


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_stream_range_folds_to_numpy_s_min_and_max(dev, n):
    x = _control(np.random.default_rng([n, 5]), n)
    misses = []
    for parts in STREAM_PARTS:
        with _collect(misses, f"parts={parts}"):
            pairs = _stream_range(dev, x, parts)
            _assert_range(np.array([np.min(pairs[:, 0]), np.max(pairs[:, 1])]), np.min(x.astype(F64)),
                          np.max(x.astype(F64)))
    _none(misses)


@gpu
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_stream_range_keeps_a_non_finite_value(dev, n):
    misses = []
    for frame in _special_frames(n):
        for name, value in NONFINITE:
            x = _control(np.random.default_rng([n, 6]), n)
            x[frame] = value
            for parts in STREAM_PARTS:
                with _collect(misses, f"n{n}-f{frame}-{name} parts={parts}"):
                    pairs = _stream_range(dev, x, parts)
                    _assert_range(np.array([np.min(pairs[:, 0]), np.max(pairs[:, 1])]), np.min(x.astype(F64)),
                                  np.max(x.astype(F64)))
    _none(misses)


# ------------------------------------------------------------------------------------------------- B2: the scan
TW_TILE = 2048                  # kTwTile
TW_MAX_SEG = 256                # kTwMaxSeg
# n -> (tiles per segment, segments, frames of the last segment)
SCAN_SIZES = {1: (1, 1, 1), 7: (1, 1, 7), 2048: (1, 1, 2048), 2049: (1, 2, 1), 4099: (1, 3, 3), 524288: (1, 256, 2048),
              524289: (2, 129, 1), 1050625: (3, 172, 1)}
POS0 = 12345.0 + 3 * 2.0 ** -20
FLOAT_FRAMES = 524289


def _scan_plan(n):
    """pgx_timewarp_scan's segmentation, restated."""
    tiles = -(-n // TW_TILE)
    per_seg = -(-tiles // TW_MAX_SEG)
    nseg = -(-tiles // per_seg)
    return per_seg, nseg, n - (nseg - 1) * per_seg * TW_TILE


def _exact_rates(n):
    """k / 2^20 with |k| <= 2^22: up over the first quarter, down over the middle half, up again -- the highest position
    lies near n / 4 and the lowest near 3 n / 4, inside the block and in different segments."""
    k = np.random.default_rng([n, 7]).integers(-2 ** 21, 2 ** 21 + 1, n)
    i = np.arange(n)
    k += np.where((i < n // 4) | (i >= 3 * n // 4), 2 ** 21, -2 ** 21)
    rate = (k / 2.0 ** 20).astype(F32)
    assert np.max(np.abs(k)) <= 2 ** 22 and np.array_equal(rate.astype(F64) * 2.0 ** 20, k)
    return rate


def _scan_buffers(dev, rate, pos0):
    from pygmu2_amd.device import TIMEWARP_WORKSPACE_DOUBLES
    assert TIMEWARP_WORKSPACE_DOUBLES == 768
    n = rate.shape[0]
    return _buffers(dev, rate=rate, state=np.array([pos0], dtype=F64), positions=((n,), F64), range=((2,), F64),
                    workspace=((TIMEWARP_WORKSPACE_DOUBLES,), F64))


def _scan(dev, b, n):
    """One pgx_timewarp_scan over the buffers -> (positions, range, head)."""
    b.rewritten = ("state",)
    dev.check(dev.ensure_init().pgx_timewarp_scan(b.positions.ptr, b.range.ptr, b.state.ptr, b.workspace.ptr,
                                                  b.rate.ptr, n))
    return b.positions.to_host(), b.range.to_host(), float(b.state.to_host()[0])


@gpu
@pytest.mark.parametrize("n", sorted(SCAN_SIZES))
def test_timewarp_scan_is_exact_on_dyadic_rates(dev, n):
    assert _scan_plan(n) == SCAN_SIZES[n]
    per_seg, nseg, _ = SCAN_SIZES[n]
    rate = _exact_rates(n)
    rate64 = rate.astype(F64)
    heads, wants = [POS0], []
    for _ in range(2):
        want, _, head = timewarp_step(heads[-1], rate64, (None, None))
        wants.append(want)
        heads.append(head)
    assert np.max(np.abs(wants[1])) < 2.0 ** 25 and np.all(wants[1] * 2.0 ** 20 == np.rint(wants[1] * 2.0 ** 20))
    if n >= TW_TILE:
        hi_at, lo_at = int(np.argmax(wants[0])), int(np.argmin(wants[0]))
        assert 0 < hi_at < n - 1 and 0 < lo_at < n - 1
        if nseg > 2:
            assert hi_at // (per_seg * TW_TILE) != lo_at // (per_seg * TW_TILE)
    want_zero, _, head_zero = timewarp_step(0.0, rate64, (None, None))

    def check(got, want, head, what):
        _assert_bits(got[0], want, f"{what}: positions")
        _assert_range(got[1], np.min(want), np.max(want), f"{what}: range")
        assert got[2] == head, f"{what}: head {got[2]!r}, want {head!r}"

    with _scan_buffers(dev, rate, POS0) as b:
        check(_scan(dev, b, n), wants[0], heads[1], "first scan")
        check(_scan(dev, b, n), wants[1], heads[2], "second scan, from the first one's head")
        b.state.zero_()
        check(_scan(dev, b, n), want_zero, head_zero, "from a zeroed state")
        b.state.upload(np.array([POS0]))
        check(_scan(dev, b, n), wants[0], heads[1], "the first scan again")


@gpu
def test_timewarp_scan_float_rates_within_the_summation_bound(dev):
    """Rates in [0.5, 2]: a dropped or doubled frame moves every later position by at least 0.5, the limit at the last
    frame is 524 290 x 2^-53 x 6.6e5 = 3.8e-5."""
    n = FLOAT_FRAMES
    assert _scan_plan(n) == (2, 129, 1)
    pos0 = 1000.25
    rate = np.random.default_rng([n, 8]).uniform(0.5, 2.0, n).astype(F32)
    sums = np.concatenate(([0.0], np.cumsum(rate.astype(np.longdouble))))            # sums[i] = sum(rate[:i])
    ref = np.longdouble(pos0) + sums
    limit = (np.arange(n + 1) + 2) * 2.0 ** -53 * (abs(pos0) + sums)                  # the rates are positive
    with _scan_buffers(dev, rate, pos0) as b:
        got, rng_, head = _scan(dev, b, n)
    assert np.all(np.isfinite(got))
    ratio = np.abs(got.astype(np.longdouble) - ref[:n]) / limit[:n]
    worst = int(np.argmax(ratio))
    print(f"LOOKUP_DIRECT scan float n={n}: max(err/limit)={float(ratio[worst]):.4f} at frame {worst}, "
          f"head err/limit={float(abs(np.longdouble(head) - ref[n]) / limit[n]):.4f}")
    assert float(ratio[worst]) <= 1.0, (worst, got[worst], ref[worst])
    assert abs(np.longdouble(head) - ref[n]) <= limit[n]
    _assert_range(rng_, np.min(got), np.max(got), "range of the positions written")
    assert rng_[0] == got[0] == pos0 and rng_[1] == got[-1]


# ------------------------------------------------------------------------------------------------- B3: pgx_wavetable
WT_WINDOW_START = -1            # the window is [wt_start - 1, wt_end + 2), as WavetablePE keeps it


def _interp_want(indices, window, window_start, cubic, oob=None):
    res = (cubic_interp if cubic else linear_interp)(indices, window, window_start)
    if oob is not None and np.any(oob):
        res = res.copy()
        res[oob] = 0.0
    return res.astype(F32)


def _table_indices(rng, n, wt_start, wt_end):
    """The edges first (a short case keeps the first ones), then fractional indices inside the table and exact integers."""
    length = wt_end - wt_start
    edges = [wt_end - 0.5, wt_start - 0.25, wt_start, wt_end - 1, wt_end, wt_end - 0.25, wt_end - 0.75,
             wt_start - 0.5, wt_start - 1.75, -0.0, 0.0, wt_start - length, wt_start - 3 * length, wt_start - 7 * length,
             wt_start + 2 * length, wt_start + length + 0.5, -1e-20, 1e6, -1e6, wt_start + 0.5]
    inside = rng.uniform(wt_start, wt_end - 1, n)
    inside[::3] = rng.integers(wt_start, wt_end, n)[::3]
    raw = np.concatenate((edges, inside))[:n].astype(F32)
    if n > len(edges):
        assert np.any(raw == wt_start - 3 * length) and np.any((raw > wt_end - 1) & (raw < wt_end))
        assert np.any((raw < 0) & (raw != np.floor(raw))) and np.any(np.signbit(raw) & (raw == 0))
    return raw


def _wavetable_case(window_len, channels, n, seed):
    rng = np.random.default_rng([window_len, channels, n, seed])
    window = rng.standard_normal((window_len, channels)).astype(F32)
    wt_start, wt_end = WT_WINDOW_START + 1, WT_WINDOW_START + window_len - 2
    assert wt_end > wt_start
    return window, _table_indices(rng, n, wt_start, wt_end), wt_start, wt_end


def _wavetable(dev, raw, window, cubic, mode, finite, wt_start, wt_end):
    lib = dev.ensure_init()
    n, (window_len, channels) = raw.shape[0], window.shape
    with _buffers(dev, indexer=raw, window=window, out=((n, channels), F32)) as b:
        dev.check(lib.pgx_wavetable(b.out.ptr, b.indexer.ptr, n, b.window.ptr, WT_WINDOW_START, window_len, channels,
                                    cubic, MODES.index(mode), finite, float(wt_start), float(wt_end)))
        return b.out.to_host()


def _check_wavetable(dev, monkeypatch, env, window_len, channels, cubic, n, staged, grid):
    """One row under every oob_mode x finite: the plan's answer, the restatement, the run gathered from global memory."""
    lib = dev.ensure_init()
    window, raw, wt_start, wt_end = _wavetable_case(window_len, channels, n, 9)
    misses = []
    for mode in MODES:
        for finite in (0, 1):
            idx, oob = _processed(raw, mode, finite, (wt_start, wt_end))
            want = _interp_want(idx, window, WT_WINDOW_START, cubic, oob)
            with _collect(misses, f"{mode} finite={finite}"):
                if env is None:
                    monkeypatch.delenv(ENV, raising=False)
                else:
                    monkeypatch.setenv(ENV, env)
                rc, got_staged, got_grid = export(lib, n, window_len, channels, cubic)
                assert (rc, got_staged) == (0, staged) and grid in (None, got_grid), (rc, got_staged, got_grid)
                got = _wavetable(dev, raw, window, cubic, mode, finite, wt_start, wt_end)
                monkeypatch.setenv(ENV, "0")
                assert export(lib, n, window_len, channels, cubic)[:2] == (0, 0)
                gathered = _wavetable(dev, raw, window, cubic, mode, finite, wt_start, wt_end)
                _assert_bits(got, want, "against the restatement")
                _assert_bits(got, gathered, "against the run gathered from global memory")
    _none(misses)


@gpu
@pytest.mark.parametrize("window_len,channels,cubic,n,staged,grid", SWITCH_CASES,
                         ids=[f"{c[0]}x{c[1]}-{'cubic' if c[2] else 'linear'}-n{c[3]}" for c in SWITCH_CASES])
def test_wavetable_either_side_of_the_staging_switch(dev, monkeypatch, window_len, channels, cubic, n, staged, grid):
    _check_wavetable(dev, monkeypatch, None, window_len, channels, cubic, n, staged, grid)


@gpu
@pytest.mark.parametrize("env,window_len,channels,cubic,n,staged", ENV_CASES,
                         ids=[f"env{c[0]}-{c[1]}x{c[2]}-{'cubic' if c[3] else 'linear'}-n{c[4]}" for c in ENV_CASES])
def test_wavetable_follows_the_staging_limit_of_the_environment(dev, monkeypatch, env, window_len, channels, cubic, n,
                                                                staged):
    _check_wavetable(dev, monkeypatch, env, window_len, channels, cubic, n, staged, None)


@gpu
def test_wavetable_and_its_plan_answer_bad_arguments_alike(dev):
    lib = dev.ensure_init()
    window, raw, wt_start, wt_end = _wavetable_case(4, 1, 4, 10)
    with _buffers(dev, indexer=raw, window=window, out=((4, 1), F32)) as b:
        seen = set()
        for n, window_len, channels in ((0, 4, 1), (-3, 4, 1), (0, 0, 0), (4, 0, 1), (4, -1, 1), (4, 4, 0), (4, 4, -2)):
            rc = lib.pgx_wavetable(b.out.ptr, b.indexer.ptr, n, b.window.ptr, WT_WINDOW_START, window_len, channels, 0, 0,
                                   1, float(wt_start), float(wt_end))
            assert rc == export(lib, n, window_len, channels, 0)[0], (n, window_len, channels, rc)
            seen.add(rc)
        assert seen == {0, dev.ERR_INVALID}
        assert np.all(_bits(b.out.to_host()) == 0xFFFFFFFF)        # nothing was launched


# ------------------------------------------------------------------------------------------------- B4: the edges
CHANNELS = [1, 2, 3, 5]
LENGTHS = [1, 257, 4099]
STARTS = [-37, 1 << 40]


def _interp_lookup(dev, window, window_start, start, n, delay, cubic, bounded=0, extent=(0.0, 0.0), delay_scalar=0.0):
    lib = dev.ensure_init()
    spec = dict(window=window, out=((n, window.shape[1]), F32))
    if delay is not None:
        spec["delay"] = delay
    with _buffers(dev, **spec) as b:
        dev.check(lib.pgx_interp_lookup(b.out.ptr, b.window.ptr, window_start, window.shape[0], window.shape[1], start, n,
                                        delay_scalar, None if delay is None else b.delay.ptr, cubic, bounded,
                                        extent[0], extent[1]))
        return b.out.to_host()


def _timewarp(dev, window, window_start, n, positions, cubic, has_start=0, extent_start=0.0, has_end=0, extent_end=0.0,
              pos0=0.0, rate=0.0):
    lib = dev.ensure_init()
    spec = dict(window=window, out=((n, window.shape[1]), F32))
    if positions is not None:
        spec["positions"] = positions
    with _buffers(dev, **spec) as b:
        dev.check(lib.pgx_timewarp(b.out.ptr, n, None if positions is None else b.positions.ptr, pos0, rate,
                                   b.window.ptr, window_start, window.shape[0], window.shape[1], cubic, has_start,
                                   extent_start, has_end, extent_end))
        return b.out.to_host()


def _window(rng, length, channels):
    w = rng.standard_normal((length, channels)).astype(F32)
    w[w == 0] = 1.0
    return w


def _walk(case, dev, cubic, **axes):
    """case(dev, cubic=cubic, ...) at every combination of the axes; every combination that failed is reported."""
    misses = []
    for combo in itertools.product(*axes.values()):
        kw = dict(zip(axes, combo))
        with _collect(misses, " ".join(f"{k}={v}" for k, v in kw.items())):
            case(dev, cubic=cubic, **kw)
    _none(misses)


def _reach(idx, window_start, window_len):
    """The indices go at least 3 frames past either end of the window."""
    return np.min(idx) <= window_start - 3 and np.max(idx) >= window_start + window_len - 1 + 3


def _clip_lookup(dev, channels, n, start, cubic):
    rng = np.random.default_rng([channels, n, cubic, 11])
    window_start, window_len = start + 5, max(n - 10, 1)
    window = _window(rng, window_len, channels)
    delay = (rng.integers(-256, 257, n) / 64.0).astype(F32)
    delay[0], delay[-1] = (3.75, -3.25) if n > 1 else (3.25, 3.25)
    idx = _indices_of(delay, start)
    assert n == 1 or _reach(idx, window_start, window_len)
    got = _interp_lookup(dev, window, window_start, start, n, delay, cubic)
    _assert_bits(got, _interp_want(idx, window, window_start, cubic))


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_interp_lookup_clips_its_neighbours_like_np_clip(dev, cubic):
    """A window 5 frames short of the block at either end, no extents: every clipped neighbour shapes a frame that is
    kept.  Delays are multiples of 1/64 in [-4, 4]: start + i - delay is exact at 2^40 too."""
    _walk(_clip_lookup, dev, cubic, channels=CHANNELS, n=LENGTHS, start=STARTS)


def _clip_timewarp(dev, channels, n, window_start, cubic):
    rng = np.random.default_rng([channels, n, cubic, 12])
    window_len = 64
    window = _window(rng, window_len, channels)
    positions = window_start - 4.0 + rng.uniform(0.0, window_len + 8.0, n)
    positions[0] = window_start - 3.5
    positions[-1] = window_start + window_len + 2.5 if n > 1 else positions[0]
    assert n == 1 or _reach(positions, window_start, window_len)
    got = _timewarp(dev, window, window_start, n, positions, cubic)
    _assert_bits(got, _interp_want(positions, window, window_start, cubic))


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_timewarp_clips_its_neighbours_like_np_clip(dev, cubic):
    """Positions over [window - 4, window + 4) of a 64-frame window, both sides open."""
    _walk(_clip_timewarp, dev, cubic, channels=CHANNELS, n=LENGTHS, window_start=STARTS)


def _ulp_either_side(v):
    return [np.nextafter(v, -INF), v, np.nextafter(v, INF)]


def _extent_lookup(dev, channels, start, cubic):
    n, a, z = 257, 10, 200
    rng = np.random.default_rng([channels, cubic, 13])
    window_start, window_len = start - 3, n + 8
    window = _window(rng, window_len, channels)
    delay = (rng.integers(0, 33, n) / 64.0).astype(F32)                 # in [0, 0.5]: the indices rise
    idx = _indices_of(delay, start)
    assert np.all(np.diff(idx) > 0)
    for k, extent_start in enumerate(_ulp_either_side(idx[a])):
        for m, extent_end in enumerate(_ulp_either_side(idx[z])):
            oob = (idx < extent_start) | (idx >= extent_end)
            assert oob[a] == (k == 2) and oob[z] == (m != 2) and not oob[a + 1] and oob[z + 1] and oob[a - 1]
            got = _interp_lookup(dev, window, window_start, start, n, delay, cubic, 1, (extent_start, extent_end))
            _assert_bits(got, _interp_want(idx, window, window_start, cubic, oob), f"extent {k} {m}")
            assert np.all(_bits(got)[oob] == 0) and np.all(got[~oob] != 0)   # true +0.0, and only there


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_interp_lookup_extent_edges(dev, cubic):
    """An index equal to extent_start is kept, one equal to extent_end is zeroed; an ulp either side of each."""
    _walk(_extent_lookup, dev, cubic, channels=[1, 3], start=STARTS)


def _extent_timewarp(dev, window_start, cubic, has_start, has_end):
    n, channels, window_len = 257, 2, 80
    rng = np.random.default_rng([cubic, has_start, has_end, 14])
    window = _window(rng, window_len, channels)
    extent_start, extent_end = window_start + 10.25, window_start + 60.5
    positions = window_start + rng.uniform(3.0, window_len - 4.0, n)
    edges = _ulp_either_side(extent_start) + _ulp_either_side(extent_end)
    positions[5:5 + len(edges)] = edges
    oob = np.zeros(n, dtype=bool)
    if has_start:
        oob |= positions < extent_start
    if has_end:
        oob |= positions >= extent_end
    assert list(oob[5:11]) == [bool(has_start), False, False, False, bool(has_end), bool(has_end)]
    got = _timewarp(dev, window, window_start, n, positions, cubic, has_start, extent_start, has_end, extent_end)
    _assert_bits(got, _interp_want(positions, window, window_start, cubic, oob))
    assert np.all(_bits(got)[oob] == 0) and np.all(got[~oob] != 0)


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_timewarp_extent_edges(dev, cubic):
    _walk(_extent_timewarp, dev, cubic, window_start=STARTS, has_start=[0, 1], has_end=[0, 1])


def _scalar_delay(dev, channels, n, start, cubic):
    rng = np.random.default_rng([channels, n, cubic, 15])
    window_start, window_len = start - 6, n + 8
    window = _window(rng, window_len, channels)
    delay = np.full(n, 3.25, dtype=F32)
    idx = _indices_of(delay, start)
    extent = (float(start), float(start + n) + 0.5)
    oob = (idx < extent[0]) | (idx >= extent[1])
    assert np.all(oob[:4]) and not np.any(oob[4:])
    want = _interp_want(idx, window, window_start, cubic, oob)
    scalar = _interp_lookup(dev, window, window_start, start, n, None, cubic, 1, extent, delay_scalar=3.25)
    stream = _interp_lookup(dev, window, window_start, start, n, delay, cubic, 1, extent)
    _assert_bits(scalar, want, "scalar delay")
    _assert_bits(stream, scalar, "stream against scalar")


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_interp_lookup_scalar_delay_is_the_constant_stream(dev, cubic):
    """delay = NULL with delay_scalar 3.25 (exact in float32) against a stream of 3.25; the first four frames lie below
    the extent."""
    _walk(_scalar_delay, dev, cubic, channels=CHANNELS, n=LENGTHS, start=STARTS)


def _scalar_rate(dev, channels, n, window_start, cubic, rate):
    rng = np.random.default_rng([channels, n, cubic, 16])
    span = (n - 1) * abs(rate)
    window_len = int(np.ceil(span)) + 8
    window = _window(rng, window_len, channels)
    pos0 = window_start + 3.5 + (span if rate < 0 else 0.0)
    positions = pos0 + np.arange(n, dtype=F64) * rate
    assert window_start + 3 <= np.min(positions) and np.max(positions) <= window_start + window_len - 4
    extent_start, extent_end = float(np.min(positions)) + 2.0, float(np.max(positions)) - 2.0
    oob = (positions < extent_start) | (positions >= extent_end)
    want = _interp_want(positions, window, window_start, cubic, oob)
    scalar = _timewarp(dev, window, window_start, n, None, cubic, 1, extent_start, 1, extent_end, pos0=pos0, rate=rate)
    stream = _timewarp(dev, window, window_start, n, positions, cubic, 1, extent_start, 1, extent_end)
    _assert_bits(scalar, want, "scalar rate")
    _assert_bits(stream, scalar, "stream against scalar")


@gpu
@pytest.mark.parametrize("cubic", [0, 1])
def test_timewarp_scalar_rate_is_the_position_stream(dev, cubic):
    """positions = NULL with pos0 + i * rate (multiples of 1/8: exact in float64, at 2^40 too) against the same positions
    handed over; the extent cuts two frames' worth off either end."""
    _walk(_scalar_rate, dev, cubic, channels=CHANNELS, n=LENGTHS, window_start=STARTS, rate=[0.375, -1.25])
