"""GPU: KarplusStrongPE (pgx_karplus_strong) is bit-exact -- against the reference's fixtures, against the float32
restatement over 10 s, with a line too long for LDS, in a batch of 256 strings through the C ABI, and under
look-ahead windows (samples and the carried line identical to block-by-block rendering)."""

import numpy as np
import pytest

import pygmu2_amd as pg
from fixture_harness import load_cases
from pygmu2_amd import device, look_ahead
from pygmu2_amd.device import DeviceBuffer
from sources_gpu_common import bits_equal, render_case, stream
from sources_oracle import KarplusStrong, ks_geometry

pytestmark = pytest.mark.gpu

DATA, NPZ = load_cases("sources")
KS_CASES = [c for c in DATA["cases"] if c["kind"] == "ks"]


@pytest.mark.parametrize("case", KS_CASES, ids=lambda c: c["name"])
def test_goldens_bit_exact(case):
    assert bits_equal(render_case(case), NPZ[case["name"]])


def _contig(start, n, block):
    return [(s, min(block, start + n - s)) for s in range(start, start + n, block)]


def test_ten_seconds_one_render_and_blocks():
    sr, n = 44100, 441_000
    want = KarplusStrong(sr, 440.0, rho=0.996, seed=42).render(0, n)
    pg.set_sample_rate(sr)
    _, one = stream(pg.KarplusStrongPE(440.0, rho=0.996, seed=42), sr, [(0, n)])
    assert bits_equal(one[0], want)
    _, blocks = stream(pg.KarplusStrongPE(440.0, rho=0.996, seed=42), sr, _contig(0, n, 1024))
    assert bits_equal(np.concatenate(blocks), want)


def test_line_beyond_lds():
    sr = 192_000                       # 1 Hz: N = 192 000 floats, the global-memory path
    n = 420_000
    oracle = KarplusStrong(sr, 1.0, rho=0.999, seed=4, duration=300_000, rho_damping=0.9)
    want = np.concatenate([oracle.render(s, d) for s, d in _contig(-1000, n, 65_536)])
    pg.set_sample_rate(sr)
    pe = pg.KarplusStrongPE(1.0, rho=0.999, seed=4, duration=300_000, rho_damping=0.9)
    _, got = stream(pe, sr, _contig(-1000, n, 65_536))
    assert bits_equal(np.concatenate(got), want)


def test_batch_of_256_matches_one_by_one():
    sr, n, batch = 44100, 20_000, 256
    rng = np.random.default_rng(1)
    freqs = np.exp(rng.uniform(np.log(20.0), np.log(9000.0), batch))
    lib = pg.device.ensure_init()
    geo = [ks_geometry(sr, f) for f in freqs]
    offsets = np.concatenate(([0], np.cumsum([g[0] for g in geo])))
    params = np.zeros(batch, dtype=device.KS_PARAMS)
    lines = np.zeros(int(offsets[-1]), dtype=np.float32)
    for i, (N, c) in enumerate(geo):
        two = i % 3 == 0
        params[i] = (offsets[i], N, int(two), 5000 + 37 * i, np.float32(0.99 + 0.00003 * i), np.float32(0.95),
                     np.float32(c), 0.0)
        lines[offsets[i]:offsets[i + 1]] = KarplusStrong(sr, freqs[i], seed=i).excitation()
    max_line = int(max(g[0] for g in geo))

    def run(idx, start, frames, state_buf, line_buf, p_buf, out_buf):
        rc = lib.pgx_karplus_strong(out_buf.ptr, frames, len(idx), start, frames, 1, p_buf.ptr, line_buf.ptr,
                                    state_buf.ptr, max_line)
        assert rc == 0

    # the whole bank, two renders
    p_all, l_all = DeviceBuffer.from_host(params), DeviceBuffer.from_host(lines)
    s_all = DeviceBuffer((batch,), device.KS_STATE, zero=True)
    bank = []
    for start, frames in ((0, 7_000), (7_000, n - 7_000)):
        out = DeviceBuffer((batch, frames), np.float32)
        run(range(batch), start, frames, s_all, l_all, p_all, out)
        bank.append(out.to_host())
    bank = np.concatenate(bank, axis=1)
    # each string on its own (line offset 0 in its own buffer)
    for i in range(0, batch, 1):
        p1 = params[i:i + 1].copy()
        p1["line_offset"] = 0
        pb, lb = DeviceBuffer.from_host(p1), DeviceBuffer.from_host(lines[offsets[i]:offsets[i + 1]])
        sb = DeviceBuffer((1,), device.KS_STATE, zero=True)
        outs = []
        for start, frames in ((0, 7_000), (7_000, n - 7_000)):
            out = DeviceBuffer((1, frames), np.float32)
            rc = lib.pgx_karplus_strong(out.ptr, frames, 1, start, frames, 1, pb.ptr, lb.ptr, sb.ptr, int(p1["n"][0]))
            assert rc == 0
            outs.append(out.to_host()[0])
        assert bits_equal(np.concatenate(outs), bank[i]), i
    # the carried lines agree with the serial restatement for a few strings
    got_lines = l_all.to_host()
    for i in (0, 1, 97, 255):
        ks = KarplusStrong(sr, freqs[i], rho=float(params["rho"][i]), seed=i,
                           duration=int(params["switch_at"][i]) if i % 3 == 0 else None,
                           rho_damping=0.95 if i % 3 == 0 else None)
        want = ks.render(0, n)[:, 0]
        assert bits_equal(want, bank[i]), i
        assert bits_equal(ks.buf, got_lines[offsets[i]:offsets[i + 1]]), i


def _la_run(enabled):
    look_ahead.set_enabled(enabled)
    try:
        pg.set_sample_rate(44100)
        pe = pg.KarplusStrongPE(196.0, rho=0.998, duration=30_000, rho_damping=0.95, seed=8)
        root = pg.GainPE(pe, gain=0.5)
        if enabled:
            assert look_ahead.capable(root)
        r, out = stream(root, 44100, _contig(0, 60 * 1024, 1024))
        look_ahead.before_direct_access(pe)
        lines = [pe._line.to_host().copy()]
        out += [root.render(s, n).data.copy() for s, n in [(200_000, 1024), (201_024, 1024)]]     # seek: continues
        out += [root.render(s, 1024).data.copy() for s in range(202_048, 202_048 + 40 * 1024, 1024)]
        look_ahead.before_direct_access(pe)
        lines.append(pe._line.to_host().copy())
        pe.reset_state()
        out += [root.render(s, 1024).data.copy() for s in range(0, 30 * 1024, 1024)]
        look_ahead.before_direct_access(pe)
        lines.append(pe._line.to_host().copy())
        r.stop()
        return out, lines
    finally:
        look_ahead.set_enabled(True)


def test_look_ahead_matches_block_by_block():
    a, la = _la_run(True)
    b, lb = _la_run(False)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert bits_equal(x, y)
    for x, y in zip(la, lb):
        assert bits_equal(x, y)
