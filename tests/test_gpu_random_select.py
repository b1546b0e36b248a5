"""GPU: RandomSelectPE and the restart bank.  Every fixture case of the reference (tests/golden/random_select_cases.json,
random_select.npz) in its three block patterns with the bank on; the bank on against the bank off (the composed path:
one render and one copy per event) to the bit; pgx_restart_plan / pgx_restart_gather through the C ABI against numpy
restatements (tests/random_select_oracle.py); and what the bank promises to count: one 32-byte read per block, one render
per distinct candidate."""


import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, restart_bank
import fixture_harness as H
import random_select_oracle as R

pytestmark = pytest.mark.gpu

DATA, NPZ = H.load_cases("random_select")
CASES = DATA["cases"]
RUNS = [(c, p) for c in CASES for p in c["patterns"]]
RUN_IDS = [f"{c['name']}-{p}" for c, p in RUNS]
T, S = device.RESTART_TILE, device.RESTART_MAX_SEGMENTS


@pytest.fixture(autouse=True)
def _bank_on():
    pg.set_sample_rate(DATA["sr"])
    was = restart_bank.enabled()
    restart_bank.set_enabled(True)
    yield
    restart_bank.set_enabled(was)


def render(case, pattern, graph=None):
    made = []
    pe = R.build(pg, graph or case["graph"], made)
    outs = H.render_blocks(pe, case["sr"], case["patterns"][pattern], case.get("ops"), lambda: H.reset_all(made))
    return outs, made


_off = {}


def bank_off(case, pattern):
    """The composed path's render of a run, once per session."""
    key = (case["name"], pattern)
    if key not in _off:
        restart_bank.set_enabled(False)
        try:
            _off[key] = render(case, pattern)[0]
        finally:
            restart_bank.set_enabled(True)
    return _off[key]


# ---------------------------------------------------------------------------------------------- fixtures of the reference
@pytest.mark.parametrize("case,pattern", RUNS, ids=RUN_IDS)
def test_cases_match_the_reference(case, pattern):
    outs, made = render(case, pattern)
    eligible = all(restart_bank.eligible(s) for m in made for s in m._sources)
    assert eligible == (case["name"] != "stateful_saws")
    assert all(bool(m._bank) == eligible for m in made)          # the path each case is meant to take
    blocks = case["patterns"][pattern]
    want = R.expected(case, pattern, NPZ)
    stored = H.split_blocks({"blocks": blocks, "name": case["name"]}, want)
    if case["compare"] == "bits":
        for i, w in stored.items():
            H.assert_bits(f"{case['name']}/{pattern} block {i}", outs[i], w)
    else:
        assert case["compare"] == "float"
        H.assert_per_block(f"{case['name']}/{pattern}", outs, stored, H.REL_TOL, H.SCORE_ABS_FLOOR, "RSEL")


@pytest.mark.parametrize("case,pattern", RUNS, ids=RUN_IDS)
def test_bank_on_equals_bank_off(case, pattern):
    on, off = render(case, pattern)[0], bank_off(case, pattern)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{case['name']}/{pattern} block {i}"


def test_stop_start_and_reset_state():
    """The fixture's ops case: a stop / start goes on in the sequence of draws and forgets the running stretch; a
    reset_state() takes one draw and is silent until the next event."""
    case = next(c for c in CASES if "ops" in c)
    (pattern, blocks), = case["patterns"].items()
    outs, _ = render(case, pattern)
    stored = H.split_blocks({"blocks": blocks, "name": case["name"]}, R.expected(case, pattern, NPZ))
    for i, w in stored.items():
        H.assert_bits(f"{case['name']} block {i}", outs[i], w)
    for at, op in case["ops"].items():
        block = outs[int(at)]
        fired = pg.PeriodicTrigger(hz=case["graph"]["trigger"]["hz"]).render(*blocks[int(at)]).data[:, 0] > 0
        lead = int(np.argmax(fired)) if fired.any() else len(block)
        assert lead > 0 and not block[:lead].any(), f"{op}: silence until the block's first event"
        assert block[lead:].any()


# ---------------------------------------------------------------------------------------------- TriggerRestartPE
SOURCES = {"sine": {"t": "sine", "f": 300.0, "amp": 0.5}, "const2": {"t": "const", "v": 0.5, "ch": 2},
           "slice3": {"t": "slice", "src": {"t": "array", "n": 700, "ch": 3, "key": 9}, "start": 20, "dur": 120}}


def _triggers():
    seen = {}
    for c in CASES:
        g = c["graph"]["f"] if c["graph"]["t"] == "sine" else c["graph"]
        seen.setdefault(str(g["trigger"]), (c, g["trigger"]))
    return list(seen.values())


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_trigger_restart_over_an_eligible_source_is_unchanged(source):
    """Each case's trigger over one eligible source: the bank (one candidate, no draws) against today's path."""
    for case, trigger in _triggers():
        graph = {"t": "restart", "trigger": trigger, "src": SOURCES[source]}
        for pattern in [p for p in case["patterns"] if p != "equal"] or list(case["patterns"]):
            pe = R.build(pg, graph)
            on = H.render_blocks(pe, case["sr"], case["patterns"][pattern])
            assert pe._bank and pe._bank.take_renders > 0
            restart_bank.set_enabled(False)
            try:
                pe_off = R.build(pg, graph)
                off = H.render_blocks(pe_off, case["sr"], case["patterns"][pattern])
                assert not pe_off._bank
            finally:
                restart_bank.set_enabled(True)
            assert np.concatenate(on).any()
            for i, (a, b) in enumerate(zip(on, off)):
                assert a.shape == b.shape and np.array_equal(a, b), f"{source} {case['name']}/{pattern} block {i}"


# ---------------------------------------------------------------------------------------------- the C ABI
def _trigger(kind, n, seg_frames):
    trig = np.zeros(n, dtype=np.float32)
    if kind == "all":
        trig[:] = 1.0
    elif kind == "first":
        trig[0] = 1.0
    elif kind == "last":
        trig[n - 1] = 1.0
    elif kind == "edges":                     # adjacent pairs across a tile edge and a segment edge; a NaN, a negative, a +2
        for at in (T - 1, T, seg_frames - 1, seg_frames, 2 * seg_frames - 1, 2 * seg_frames, n - 1):
            if 0 <= at < n:
                trig[at] = 1.0
        for at, v in ((3, np.nan), (5, -1.0), (T + 7, np.nan), (T + 9, -2.0), (7, 2.0), (n // 2, 2.0)):
            if 0 <= at < n and trig[at] == 0.0:
                trig[at] = v
    elif kind == "sparse":
        rng = np.random.default_rng(n)
        at = rng.integers(0, n, size=max(1, n // 300))
        trig[at] = rng.choice(np.array([1.0, 2.0, 0.5], dtype=np.float32), size=len(at))
        quiet = rng.integers(0, n, size=max(1, n // 500))
        trig[quiet] = np.where(trig[quiet] > 0, trig[quiet], rng.choice(np.array([np.nan, -1.0], np.float32),
                                                                          size=len(quiet)))
    else:
        assert kind == "none"
    return trig


def _dev_offset(array, offset):
    """`array` on the device, `offset` floats into a 16-byte aligned block: (keep-alive, device address)."""
    flat = np.ascontiguousarray(array, dtype=np.float32).reshape(-1)
    buf = device.DeviceBuffer((flat.size + offset,), np.float32)
    assert buf.ptr % 16 == 0
    if flat.size:
        device.check(device.ensure_init().pgx_memcpy_h2d(buf.ptr + 4 * offset, flat.ctypes.data, flat.nbytes), "h2d")
    return buf, buf.ptr + 4 * offset


def _abi_run(lib, scratch, n, channels, kind, carry_local, offset=0, stride=1):
    summary, workspace = scratch
    seg_frames = -(-(-(-n // T)) // S) * T
    column = _trigger(kind, n, seg_frames)
    trig = column if stride == 1 else np.stack([column] + [np.ones(n, np.float32)] * (stride - 1), axis=1)
    want_plan = R.plan(column)
    count = want_plan[0]
    # the running take begins one frame late and is three frames long; event takes: five frames from local 0, and a long
    # one that begins at local 2 -- zeros fall before, between and behind them
    base = max(carry_local, 0)
    data = [R.array_data(3, channels, 1), R.array_data(5, channels, 2), R.array_data(min(n, 5000), channels, 3)]
    firsts = [base + 1, 0, 2]
    k = np.arange(count + 1)
    sel = np.where(k % 7 == 3, -1, 1 + (k + 1) % 2).astype(np.int32)
    sel[0] = 0
    want = R.gather(column, channels, carry_local, sel, list(zip(data, firsts)))

    keep_t, trig_ptr = _dev_offset(trig, offset)
    device.check(lib.pgx_restart_plan(summary.ptr, workspace.ptr, trig_ptr, stride, n), "pgx_restart_plan")
    got_plan = [int(v) for v in summary.to_host()]
    tag = f"n={n} ch={channels} {kind} carry={carry_local} offset={offset} stride={stride}"
    assert got_plan == want_plan, tag
    held = [device.DeviceBuffer.from_host(d) for d in data]
    table = np.zeros(len(data), dtype=device.RESTART_TAKE)
    for i, (h, d, f) in enumerate(zip(held, data, firsts)):
        table[i] = (h.ptr, f, len(d))
    table_dev = device.DeviceBuffer.from_host(table.view(np.uint8))
    sel_dev = device.DeviceBuffer.from_host(sel)
    keep_o, out_ptr = _dev_offset(np.full((n, channels), 7.0, np.float32), offset)
    device.check(lib.pgx_restart_gather(out_ptr, n, channels, trig_ptr, stride, workspace.ptr, carry_local, sel_dev.ptr,
                                        len(sel), table_dev.ptr, len(data)), "pgx_restart_gather")
    got = np.empty((n, channels), dtype=np.float32)
    device.check(lib.pgx_memcpy_d2h(got.ctypes.data, out_ptr, got.nbytes), "d2h")
    H.assert_bits(tag, got, want)
    return count, want


SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17, T * S + T + 3]
KINDS = ["none", "all", "first", "last", "edges", "sparse"]
CARRIES = [-1, 0, 5, 1 << 40]


@pytest.fixture(scope="module")
def abi():
    lib = device.ensure_init()
    return lib, (device.DeviceBuffer((4,), np.int64), device.DeviceBuffer((device.RESTART_WORKSPACE_INT64,), np.int64))


@pytest.mark.parametrize("n", SIZES)
def test_plan_and_gather_against_numpy(n, abi):
    """Up to 2 T + 17 frames: every trigger x channels x carry.  T S + T + 3 frames (two tiles per segment): every
    trigger, with channels and carries taking turns -- the per-frame arithmetic is the small sizes', what is new at that
    size is the carry between tiles and segments, which every trigger kind exercises."""
    lib, scratch = abi
    small = n <= 2 * T + 17
    events = sounding = 0
    for i, kind in enumerate(KINDS):
        for ch in ((1, 2, 3) if small else (1 + i % 3,)):
            for carry in (CARRIES if small else (CARRIES[(i + 1) % 4],)):
                count, want = _abi_run(lib, scratch, n, ch, kind, carry)
                events += count
                sounding += int(np.count_nonzero(want))
    assert events > 0 and sounding > 0


@pytest.mark.parametrize("n", [65, T + 1, 2 * T + 17])
def test_misaligned_pointers_and_wide_triggers(n, abi):
    """`out` and `trigger` one float off 16-byte alignment, and a trigger of two channels: the paths without vector
    loads and stores."""
    lib, scratch = abi
    for kind in KINDS:
        for ch in (1, 3):
            _abi_run(lib, scratch, n, ch, kind, 5, offset=1)
        _abi_run(lib, scratch, n, 1, kind, 0, offset=0, stride=2)
        _abi_run(lib, scratch, n, 2, kind, -1, offset=1, stride=2)


def test_bad_arguments_are_refused(abi):
    lib, (summary, workspace) = abi
    trig = device.DeviceBuffer.from_host(np.zeros(8, np.float32))
    assert lib.pgx_restart_plan(None, workspace.ptr, trig.ptr, 1, 8) == -1
    assert lib.pgx_restart_plan(summary.ptr, workspace.ptr, trig.ptr, 0, 8) == -1
    assert lib.pgx_restart_gather(None, 8, 1, trig.ptr, 1, workspace.ptr, 0, trig.ptr, 1, None, 0) == -1
    assert lib.pgx_restart_gather(trig.ptr, 8, 1, trig.ptr, 1, workspace.ptr, 0, trig.ptr, 1, None, 1) == -1


# ---------------------------------------------------------------------------------------------- counters
def _started(pe, sr):
    r = pg.NullRenderer(sample_rate=sr)
    r.set_source(pe)
    r.start()
    return r


def test_fifty_events_cost_a_render_per_distinct_candidate():
    sr = DATA["sr"]
    pe = pg.RandomSelectPE(pg.PeriodicTrigger(hz=100.0, phase=0.5), [pg.SinePE(f, amplitude=0.5) for f in (200.0, 300.0, 450.0)],
                           seed=3)
    r = _started(pe, sr)
    n = 50 * (sr // 100)
    for block in range(3):                                # from the second block on a stretch runs in as well
        renders, reads = pe.take_renders, pe.d2h_reads
        data = pe.render(block * n, n).data
        assert pe.d2h_reads - reads == 1
        assert 1 <= pe.take_renders - renders <= 4
        assert int(np.count_nonzero(pg.PeriodicTrigger(hz=100.0, phase=0.5).render(block * n, n).data > 0)) == 50
        assert data.any()
    r.stop()


def test_finite_candidates_are_rendered_once_for_a_stream():
    sr = DATA["sr"]
    arr = pg.ArrayPE(R.array_data(900, 2, 4))
    slices = [pg.SlicePE(arr, 10, 40), pg.SlicePE(arr, 100, 150), pg.SlicePE(arr, 300, 500)]
    pe = pg.RandomSelectPE(pg.PeriodicTrigger(hz=40.0), slices, seed=8)
    r = _started(pe, sr)
    outs = [pe.render(i * 512, 512).data for i in range(20)]
    assert pe._bank and 1 <= pe.take_renders <= len(slices)
    assert pe.d2h_reads == 20
    r.stop()
    restart_bank.set_enabled(False)
    off = pg.RandomSelectPE(pg.PeriodicTrigger(hz=40.0), slices, seed=8)
    r = _started(off, sr)
    for i, a in enumerate(outs):
        assert np.array_equal(a, off.render(i * 512, 512).data), f"block {i}"
    assert off.take_renders == 0 and off.d2h_reads == 0
    r.stop()


def test_a_block_pulled_twice_goes_back_in_time_like_the_composed_path():
    """The second pull of a block begins before the origin its first pull left: negative local times, which the
    composed path renders.  The bank hands such a block over."""
    sr = DATA["sr"]
    outs = {}
    for bank in (True, False):
        restart_bank.set_enabled(bank)
        pe = pg.RandomSelectPE(pg.PeriodicTrigger(hz=30.0), [pg.SinePE(f, amplitude=0.5) for f in (200.0, 310.0)], seed=2)
        r = _started(pe, sr)
        outs[bank] = [pe.render(s, n).data for s, n in ((0, 1000), (0, 1000), (1000, 700), (900, 300), (1200, 64))]
        r.stop()
    restart_bank.set_enabled(True)
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert np.array_equal(a, b), f"pull {i}"
    assert outs[True][1].any()
