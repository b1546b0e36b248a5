"""GPU: SequencePE scores and the score bank (pgx_karplus_score, pgx_score_mix).

Every fixture case against what the reference rendered, in the class its note source already has in this suite: pluck,
noise and array scores bit for bit (np.array_equal: the sign of a zero is not pinned), SinePE / BlitSawPE scores within
the float-path bar of tests/test_gpu_parity.py (1e-5 of the block's peak + 1e-7).  Every case with the bank on against
the bank off in the same process: equal, the bank adds no rounding of its own.  The two kernels through the C ABI
against numpy / against pgx_karplus_strong one string at a time, and a 300-note pluck score whole, in blocks and after
reset_state against the float32 restatement of tests/sources_oracle.py."""

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, score_bank
from pygmu2_amd.device import DeviceBuffer
from fixture_harness import REL_TOL, SCORE_ABS_FLOOR as ABS_FLOOR, bits_equal, load_cases, render_blocks
from score_oracle import SR, build_case, expected, ordered_sum
from spec_build import PG
from sources_oracle import KarplusStrong, ks_geometry

pytestmark = pytest.mark.gpu

DATA, NPZ = load_cases("score")
CASES = DATA["cases"]
_RENDERS = {}


def _mix_of(pe):
    return pe if isinstance(pe, pg.MixPE) else pe.inputs()[0]


def _render(case, pattern, bank):
    """Blocks of (case, pattern) on a fresh graph, rendered once per bank setting and shared by the tests."""
    key = (case["name"], pattern, bank)
    if key not in _RENDERS:
        pg.set_sample_rate(SR)
        score_bank.set_enabled(bank)
        try:
            pe = build_case(PG, case)
            outs = render_blocks(pe, SR, case["patterns"][pattern])
            mix = _mix_of(pe)
            if isinstance(mix, pg.MixPE):
                assert bool(mix._score) == bank, "the score bank was not what rendered this case"
        finally:
            score_bank.set_enabled(True)
        _RENDERS[key] = outs
    return _RENDERS[key]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_cases_match_the_reference(case):
    for pattern, blocks in case["patterns"].items():
        got = _render(case, pattern, True)
        want = expected(case, pattern, NPZ)
        at = 0
        for i, ((_, n), g) in enumerate(zip(blocks, got)):
            w = want[at:at + n]
            at += n
            assert g.dtype == np.float32 and g.shape == w.shape, (pattern, i, g.shape, w.shape)
            if case["compare"] == "bits":
                assert np.array_equal(g, w), f"{pattern} block {i}: {int(np.sum(g != w))} of {w.size} samples differ"
            else:
                peak = float(np.max(np.abs(w))) if w.size else 0.0
                err = float(np.max(np.abs(g.astype(np.float64) - w.astype(np.float64)))) if w.size else 0.0
                print(f"{case['name']} {pattern} block {i}: max|d| = {err:.3e}, peak {peak:.3e}")
                assert err <= REL_TOL * peak + ABS_FLOOR, f"{pattern} block {i}: {err:.3e} > 1e-5 * {peak:.3e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_bank_on_equals_bank_off(case):
    for pattern in case["patterns"]:
        on, off = _render(case, pattern, True), _render(case, pattern, False)
        assert len(on) == len(off)
        for i, (a, b) in enumerate(zip(on, off)):
            assert np.array_equal(a, b), f"{pattern} block {i}: {int(np.sum(a != b))} samples differ"


# ---------------------------------------------------------------------------------------------- pgx_score_mix
def _score_mix(lib, segments, frames, ch, inline):
    """segments: [(first, data (n, ch))] -> the kernel's (frames, ch) through the C ABI."""
    k = len(segments)
    out = DeviceBuffer((frames, ch), np.float32)
    out.upload(np.full((frames, ch), np.nan, dtype=np.float32))
    if k == 0:
        assert lib.pgx_score_mix(out.ptr, frames, ch, None, 0, None, None, score_bank.TILE) == 0
        return out.to_host()
    packed = DeviceBuffer.from_host(np.concatenate([d.reshape(-1) for _, d in segments]))
    tab = np.zeros(k, dtype=device.SCORE_SEG)
    at = 0
    for i, (first, d) in enumerate(segments):
        tab[i] = (packed.ptr + 4 * at, first, len(d))
        at += d.size
    if inline:
        rc = lib.pgx_score_mix(out.ptr, frames, ch, tab.ctypes.data, k, None, None, score_bank.TILE)
    else:
        offsets, entries = score_bank.tile_lists(tab["first"], tab["frames"], frames)
        d_tab, d_off, d_list = (DeviceBuffer.from_host(a) for a in (tab, offsets, entries))
        rc = lib.pgx_score_mix(out.ptr, frames, ch, d_tab.ptr, k, d_off.ptr, d_list.ptr, score_bank.TILE)
    assert rc == 0, lib.pgx_last_error()
    return out.to_host()


@pytest.mark.parametrize("ch", [1, 2])
def test_score_mix_kernel_is_the_ordered_sum(ch):
    check_score_mix_kernel(ch)


def check_score_mix_kernel(ch, frames=10_000, count=300, edges=(1, 3, 9), crowd=40):
    """pgx_score_mix against the ordered float32 sum: `count` segments over `frames` frames, some a frame either side
    of the tile edges `edges`, `crowd` of them over the middle frame (tests/test_gpu_channels.py runs it at 3 and 5
    channels with smaller counts)."""
    lib = device.ensure_init()
    tile, mid = score_bank.TILE, frames // 2
    rng = np.random.default_rng(7 + ch)

    def seg(first, n):
        return int(first), rng.uniform(-1, 1, (int(n), ch)).astype(np.float32)

    assert not np.any(_score_mix(lib, [], frames, ch, False))                         # k = 0
    one = [seg(123, min(4567, frames - 123))]
    for inline in (True, False):                                                      # k = 1, both table routes
        assert np.array_equal(_score_mix(lib, one, frames, ch, inline), ordered_sum(one, frames, ch))
    segs = [seg(0, 1), seg(frames - 1, 1), seg(0, 700), seg(frames - 333, 333), seg(0, frames)]
    for t in edges:                                                                   # one frame either side of a tile edge
        segs += [seg(t * tile - 500, 499), seg(t * tile - 500, 500), seg(t * tile - 500, 501), seg(t * tile, 1),
                 seg(t * tile - 1, 1), seg(t * tile - 1, 2)]
    segs += [seg(mid - j, 1 + j + (j * 7) % 90) for j in range(crowd)]                # `crowd` segments cover frame `mid`
    while len(segs) < count:
        first = int(rng.integers(0, frames))
        segs.append(seg(first, rng.integers(1, min(2500, frames - first) + 1)))
    order = rng.permutation(len(segs))
    segs = [segs[i] for i in order]
    assert len(segs) == count and sum(f <= mid < f + len(d) for f, d in segs) >= crowd
    assert np.array_equal(_score_mix(lib, segs, frames, ch, False), ordered_sum(segs, frames, ch))
    few = segs[:device.SCORE_INLINE]
    assert np.array_equal(_score_mix(lib, few, frames, ch, True), ordered_sum(few, frames, ch))


# ---------------------------------------------------------------------------------------------- pgx_karplus_score
@pytest.mark.parametrize("ch,group", [(1, 1), (1, 16), (2, 16), (1, 64), (2, 7)])
def test_karplus_score_kernel_matches_one_string_at_a_time(ch, group):
    check_karplus_score_kernel(ch, group)


def check_karplus_score_kernel(ch, group, count=130):
    """pgx_karplus_score against pgx_karplus_strong one string at a time, `count` strings (tests/test_gpu_channels.py
    runs it at 3 and 5 channels with fewer strings)."""
    lib = device.ensure_init()
    sr, far = 20_000, min(77, count - 1)
    rng = np.random.default_rng(3)
    freqs = np.exp(rng.uniform(np.log(25.0), np.log(6000.0), count))
    freqs[5], freqs[far] = 10_000.0, 1.0                    # N = 2 and N = 20 000 (80 KB: past the LDS path)
    geo = [ks_geometry(sr, f) for f in freqs]
    assert geo[5][0] == 2 and geo[far][0] == 20_000
    fixed = [1, 63, 64, 65, 129]
    calls = [np.array(fixed + list(rng.integers(1, 3001, count - len(fixed)))),
             np.array(list(rng.integers(1, 3001, count - len(fixed))) + fixed)]
    starts = rng.integers(1, 50_000, count)
    params = np.zeros(count, dtype=device.KS_PARAMS)
    lines0 = []
    for i, (N, c) in enumerate(geo):
        two = i % 3 == 0
        switch = int(starts[i] + rng.integers(1, calls[0][i] + calls[1][i])) if two else 0
        params[i] = (0, N, int(two), switch, np.float32(0.99 + 0.00005 * i), np.float32(0.9), np.float32(c), 0.0)
        lines0.append(KarplusStrong(sr, freqs[i], seed=i).excitation())

    def fresh():
        p = [DeviceBuffer.from_host(params[i:i + 1]) for i in range(count)]
        ln = [DeviceBuffer.from_host(x) for x in lines0]
        st = [DeviceBuffer((1,), device.KS_STATE, zero=True) for _ in range(count)]
        return p, ln, st

    # one string at a time
    p, ln, st = fresh()
    want = [[], []]
    pos = starts.copy()
    for c_i, frames in enumerate(calls):
        for i in range(count):
            n = int(frames[i])
            out = DeviceBuffer((n, ch), np.float32)
            rc = lib.pgx_karplus_strong(out.ptr, n * ch, 1, int(pos[i]), n, ch, p[i].ptr, ln[i].ptr, st[i].ptr, geo[i][0])
            assert rc == 0
            want[c_i].append(out.to_host())
        pos = pos + frames
    want_lines = [b.to_host() for b in ln]
    want_states = [b.to_host() for b in st]

    # the score launch: every string its own buffers, destinations packed in a shuffled order
    p, ln, st = fresh()
    pos = starts.copy()
    max_line = max(g[0] for g in geo)
    for c_i, frames in enumerate(calls):
        order = rng.permutation(count)
        dst = np.zeros(count, dtype=np.int64)
        dst[order] = np.concatenate(([0], np.cumsum(frames[order] * ch)[:-1]))
        notes = np.zeros(count, dtype=device.KS_NOTE)
        for i in range(count):
            notes[i] = (p[i].ptr, ln[i].ptr, st[i].ptr, pos[i], frames[i], dst[i])
        by_count = np.argsort(-frames, kind="stable")       # as the bank orders them
        total = int(np.sum(frames)) * ch
        out = DeviceBuffer((total,), np.float32)
        if c_i == 0:
            d_notes = DeviceBuffer.from_host(notes[by_count])
            rc = lib.pgx_karplus_score(out.ptr, ch, d_notes.ptr, count, group, max_line, 0)
            assert rc == 0, lib.pgx_last_error()
        else:                                               # the second call in slices that travel as kernel arguments
            for a in range(0, count, device.SCORE_INLINE):
                part = np.ascontiguousarray(notes[by_count][a:a + device.SCORE_INLINE])
                rc = lib.pgx_karplus_score(out.ptr, ch, part.ctypes.data, len(part), group, max_line, 1)
                assert rc == 0, lib.pgx_last_error()
        got = out.to_host()
        for i in range(count):
            n = int(frames[i]) * ch
            assert bits_equal(got[dst[i]:dst[i] + n].reshape(-1, ch), want[c_i][i]), (c_i, i)
        pos = pos + frames
    for i in range(count):
        assert bits_equal(ln[i].to_host(), want_lines[i]), i
        assert st[i].to_host().tobytes() == want_states[i].tobytes(), i


# ---------------------------------------------------------------------------------------------- a long pluck score
def test_300_note_pluck_score_whole_blocks_and_reset():
    rng = np.random.default_rng(11)
    count = 300
    lens = rng.integers(200, 1001, count)
    starts = np.cumsum(rng.integers(20, 260, count))
    freqs = np.exp(rng.uniform(np.log(60.0), np.log(2000.0), count))
    two = [(int(n * 0.4), 0.8) if i % 3 == 0 else (None, None) for i, n in enumerate(lens)]
    total = int(np.max(starts + lens)) + 100
    want = np.zeros((total, 1), dtype=np.float32)
    for i in range(count):
        alone = KarplusStrong(SR, freqs[i], rho=0.995, seed=i, duration=two[i][0], rho_damping=two[i][1])
        s, n = int(starts[i]), int(lens[i])
        want[s:s + n] = want[s:s + n] + alone.render(0, n)

    def make():
        pg.set_sample_rate(SR)
        return pg.SequencePE([(pg.CropPE(pg.KarplusStrongPE(float(freqs[i]), rho=0.995, seed=i, duration=two[i][0],
                                                            rho_damping=two[i][1]), 0, int(lens[i])), int(starts[i]))
                              for i in range(count)])

    pe = make()
    whole = render_blocks(pe, SR, [[0, total]])[0]
    assert pe.inputs()[0]._score and np.array_equal(whole, want)
    pe = make()
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    blocks = [[s, min(1024, total - s)] for s in range(0, total, 1024)]
    first = np.concatenate([pe.render(s, n).data for s, n in blocks])
    assert np.array_equal(first, want)
    for node in (pe.inputs()[0].inputs()):                   # every pluck back to its excitation
        node.inputs()[0].inputs()[0].reset_state()
    second = np.concatenate([pe.render(s, n).data for s, n in blocks])
    r.stop()
    assert np.array_equal(second, first)
