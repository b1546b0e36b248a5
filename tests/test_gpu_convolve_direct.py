"""
GPU: the direct MFMA form of ConvolvePE (pgx_convolve, csrc/pgx_convolve.hip) through the C ABI, at every geometry
cv_plan() can choose: both k_conv_mfma instantiations, one and several K-chunks, one and several K-splits, the
in-kernel chunk loop, the clipped last split, one and several tile groups, blocks shorter and longer than the filter,
a one-tap filter, every channel rule.

`_plan` restates cv_plan().  test_plan_mirror_matches_the_library pins its byte count to pgx_convolve_workspace_bytes
for every case of this file, and every case asserts the plan fields it was chosen for, so a retune of cv_plan that
moves a case off its branch fails here instead of silently thinning the coverage.

Every device allocation of the harness is made inside guarded_alloc.guarded(): guard bands around out, hist and the
workspace, and a workspace that starts as 0xFF bytes, so a cell the kernels read before they write it is a NaN.

Layer A / A' / PE level: integers in [-7, 7] held as float32.  A product is at most 49, a float32 run of at most
1100 taps at most 53 900, the whole sum over 135 168 taps at most 6.7e6 -- all below 2^24, so every intermediate of
the documented arithmetic (float32 runs, float64 folds and partials, one float32 rounding) is exact in any order and
the result must equal the integer convolution bit for bit.  No tolerance anywhere in these.
Layer A'': larger positive integers, chosen so that a float32 run is exact up to the documented fold and not beyond it.
Layer B: float data against float64, pointwise, with a limit derived from the documented arithmetic (_float_reference).
Layer B': the float64 fold every 1024 taps is really there (the GPU against two CPU emulations of the arithmetic).
Layer C: the direct and the FFT path on the same inputs (what tests/test_gpu_fftconv.py's header points to).
"""

import types

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided
from scipy.signal import fftconvolve

from guarded_alloc import guarded

gpu = pytest.mark.gpu

RULES = [(1, 1), (2, 1), (2, 2), (1, 2)]
TILE_OUT = 4096                 # kCvOut: outputs per workgroup
FOLD_TAPS = 1024                # 4 * kCvFlush
RUN_TAPS = 1100                 # the header's 1024 + 16, rounded up as in the task's bound


@pytest.fixture(scope="module")
def dev():
    from pygmu2_amd import device
    device.ensure_init()
    return device


# ------------------------------------------------------------------------------------------------- the plan mirror
def _ceil_div(a, b):
    return -(-a // b)


def _up256(v):
    return (v + 255) & ~255


def _plan(n, L, C):
    """cv_plan() of csrc/pgx_convolve.hip, restated."""
    p = types.SimpleNamespace()
    p.kc = 512 if L <= 1024 else 4096
    p.n_chunks = _ceil_div(L, p.kc)
    p.tile_groups = _ceil_div(n, TILE_OUT)
    p.npad = p.tile_groups * TILE_OUT
    p.workgroups = p.tile_groups * C
    want = min(max(_ceil_div(3072, p.workgroups), 1), p.n_chunks)
    p.chunks_per_split = _ceil_div(p.n_chunks, want)
    p.n_split = _ceil_div(p.n_chunks, p.chunks_per_split)
    p.last_split_chunks = p.n_chunks - (p.n_split - 1) * p.chunks_per_split
    ktot = p.n_chunks * p.kc
    p.fp = (ktot + 64 + 15) // 16 * 16
    p.ql = (p.fp + (L - 1) + p.npad + 64) // 16 + 2 + 1100
    p.lp = ktot + 64
    p.total = _up256(C * 16 * p.ql * 4) + _up256(C * p.lp * 4) + _up256(p.n_split * C * p.npad * 8)
    return p


def _case(L, n, src_ch, fir_ch, **expect):
    return pytest.param(L, n, src_ch, fir_ch, expect, id=f"L{L}-n{n}-{src_ch}x{fir_ch}")


def _cases():
    out = []
    one = dict(kc=512, n_chunks=1, n_split=1, chunks_per_split=1)
    # a one-tap filter: Lm1 = 0, the history is neither read nor written
    for n in (1, 4096):
        for rule in ((1, 1), (2, 1)):
            out.append(_case(1, n, *rule, tile_groups=1, **one))
    # the 16-row / 16-residue edges (L = 17, n = 1: a block shorter than the history)
    for L in (2, 15, 16, 17):
        for n in (1, 255, 256, 257):
            for rule in RULES:
                out.append(_case(L, n, *rule, tile_groups=1, **one))
    # tile groups, the ragged last one; n = 100: the history shifts
    for n, tg in ((100, 1), (4095, 1), (4096, 1), (4097, 2), (12289, 4)):
        out.append(_case(300, n, 2, 2, tile_groups=tg, **one))
    for L in (511, 512):
        for n in (100, 5000):
            for rule in ((1, 1), (1, 2)):
                out.append(_case(L, n, *rule, **one))
    for L in (513, 1023, 1024):
        for n in (100, 5000):
            for rule in ((2, 1), (2, 2)):
                out.append(_case(L, n, *rule, kc=512, n_chunks=2, n_split=2, chunks_per_split=1))
    # 3072 workgroups before any K-split: the only way into the chunk loop of k_conv_mfma<512>
    out.append(_case(1024, 20481, 512, 1, kc=512, n_chunks=2, tile_groups=6, workgroups=3072, n_split=1,
                     chunks_per_split=2))
    out.append(_case(1024, 700, 512, 1, kc=512, n_chunks=2, tile_groups=1, workgroups=512))   # its n < L-1 twin
    for L in (1025, 2047):
        for n, tg in ((1, 1), (700, 1), (4097, 2)):
            for rule in ((1, 1), (2, 2)):
                out.append(_case(L, n, *rule, kc=4096, n_chunks=1, n_split=1, chunks_per_split=1, tile_groups=tg))
    for L, chunks in ((4096, 1), (4097, 2), (8193, 3)):
        for n in (3000, 9000):                                  # shorter and longer than every one of the filters
            out.append(_case(L, n, 2, 1, kc=4096, n_chunks=chunks, n_split=chunks, chunks_per_split=1))
    # beyond the FFT path's longest filter: a clipped last split
    out.append(_case(131073, 61441, 8, 1, kc=4096, n_chunks=33, tile_groups=16, workgroups=128, chunks_per_split=2,
                     n_split=17, last_split_chunks=1))
    out.append(_case(131073, 131072, 1, 1, kc=4096, n_chunks=33, tile_groups=32, chunks_per_split=1, n_split=33))
    return out


CASES = _cases()


def _assert_plan(n, L, C, expect):
    p = _plan(n, L, C)
    for field, value in expect.items():
        assert getattr(p, field) == value, (field, getattr(p, field), value, (n, L, C))
    return p


def test_plan_fields_of_every_case():
    """Host only: every case sits on the branch it was chosen for."""
    for case in CASES:
        L, n, src_ch, fir_ch, expect = case.values
        assert expect
        _assert_plan(n, L, max(src_ch, fir_ch), expect)


@gpu
def test_plan_mirror_matches_the_library(dev):
    lib = dev.ensure_init()
    seen = set()
    for case in CASES:
        L, n, src_ch, fir_ch, _ = case.values
        seen.add((n, L, max(src_ch, fir_ch)))
    seen |= {(n, L, 2) for L in STREAM_TAPS for n in STREAM_BLOCKS}
    seen |= {(RUN_EDGE_FRAMES, L, 2) for L in RUN_EDGE_TAPS}
    seen |= {(n, L, max(r)) for L in FLOAT_TAPS for n in FLOAT_FRAMES for r in RULES}
    seen |= {(9000, L, 2) for L in CROSS_TAPS} | {(FOLD_FRAMES, FOLD_FILTER, 1)}
    seen |= {(n, L, 2) for L in PE_TAPS for n in PE_BLOCKS + [PE_GAP[1], 700]}
    seen |= {(n, FOLD_FILTER, 2) for n in LONG_BLOCKS + [LONG_TAIL]}
    for n, L, C in sorted(seen):
        assert _plan(n, L, C).total == lib.pgx_convolve_workspace_bytes(n, L, C), (n, L, C)
    assert lib.pgx_convolve_workspace_bytes(0, 5, 1) == 0


# ------------------------------------------------------------------------------------------------- harness + references
def _direct_conv(dev, x, h, hist):
    """pgx_convolve over guarded, poisoned device buffers -> (out, the rewritten history)."""
    lib = dev.ensure_init()
    n, src_ch = x.shape
    L, fir_ch = h.shape
    out_ch = max(src_ch, fir_ch)
    assert hist.shape == (max(L - 1, 1), out_ch)
    assert x.dtype == h.dtype == hist.dtype == np.float32
    with guarded() as g:
        need = lib.pgx_convolve_workspace_bytes(n, L, out_ch)
        assert need == _plan(n, L, out_ch).total
        xd = dev.DeviceBuffer.from_host(x)
        hd = dev.DeviceBuffer.from_host(h)
        histd = dev.DeviceBuffer.from_host(hist)
        ws = dev.DeviceBuffer((need,), np.uint8)                # 0xFF poison
        out = dev.DeviceBuffer((n, out_ch), np.float32)         # 0xFF poison
        dev.check(lib.pgx_convolve(out.ptr, xd.ptr, n, src_ch, hd.ptr, L, fir_ch, out_ch, histd.ptr, ws.ptr))
        got, got_hist = out.to_host(), histd.to_host()
        assert g.allocations == 5
        del xd, hd, histd, ws, out
    return got, got_hist                                        # (leaving the block raised if a guard was damaged)


def _extended(x, h, hist):
    """[hist | x] and h, both widened to out_ch columns, float64."""
    n, src_ch = x.shape
    L, fir_ch = h.shape
    out_ch = max(src_ch, fir_ch)
    ext = np.empty((L - 1 + n, out_ch))
    ext[:L - 1] = hist[:L - 1]
    ext[L - 1:] = x                                             # broadcasts a mono source
    return ext, np.broadcast_to(h.astype(np.float64), (L, out_ch))


def _conv64(ext, hh, L, n):
    if L * n <= 1 << 16:
        return np.stack([np.convolve(ext[:, c], hh[:, c])[L - 1:L - 1 + n] for c in range(ext.shape[1])], axis=1)
    return fftconvolve(ext, hh, axes=0)[L - 1:L - 1 + n]


def _integer_conv(x, h, hist, below=2 ** 24):
    """The exact convolution over [hist | x] of integer-valued inputs, and the history it leaves, as float32 (exactly,
    as long as the sums stay below 2^24; rounded once, to nearest even, beyond)."""
    n, L = x.shape[0], h.shape[0]
    ext, hh = _extended(x, h, hist)
    y = _conv64(ext, hh, L, n)
    want = np.rint(y)
    assert float(np.max(np.abs(y - want))) < 1e-3               # the float64 FFT landed on the integers
    assert float(np.max(np.abs(want))) < below
    new_hist = hist.copy()
    new_hist[:L - 1] = ext[n:n + L - 1]
    return want.astype(np.float32), new_hist


def _integers(rng, shape):
    return rng.integers(-7, 8, size=shape).astype(np.float32)   # not decaying: the last tap weighs as much as the first


def _taps(rng, shape):
    """An integer filter whose first and last taps are not zero, so that dropping either end always shows."""
    h = _integers(rng, shape)
    for row in (0, -1):
        h[row][h[row] == 0] = 7.0
    return h


def _bit_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if not (got.dtype == want.dtype == np.float32 and got.shape == want.shape):
        return False
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _first_miss(got, want):
    bad = np.argwhere(~(got == want))
    at = tuple(bad[0])
    return f"{bad.shape[0]} cells differ, first at {list(at)}: got {got[at]!r} want {want[at]!r}"


# ------------------------------------------------------------------------------------------------- layer A
@gpu
@pytest.mark.parametrize("L,n,src_ch,fir_ch,expect", CASES)
def test_integer_convolution_is_bit_exact(dev, L, n, src_ch, fir_ch, expect):
    out_ch = max(src_ch, fir_ch)
    _assert_plan(n, L, out_ch, expect)
    rng = np.random.default_rng([L, n, src_ch, fir_ch])
    x, h = _integers(rng, (n, src_ch)), _taps(rng, (L, fir_ch))
    hist = _integers(rng, (max(L - 1, 1), out_ch))
    got, got_hist = _direct_conv(dev, x, h, hist)
    want, want_hist = _integer_conv(x, h, hist)
    if L == 1:
        assert np.array_equal(want_hist, hist)                  # nothing to carry: the buffer is left as it was
    assert np.array_equal(got, want), _first_miss(got, want)
    assert np.array_equal(got_hist, want_hist), _first_miss(got_hist, want_hist)
    assert _bit_equal(got_hist, want_hist)


# ------------------------------------------------------------------------------------------------- layer A'
STREAM_TAPS = [17, 513, 1025, 2047]
STREAM_BLOCKS = [4097, 1, 17, 5000, 4096, 1789]


@gpu
@pytest.mark.parametrize("L", STREAM_TAPS)
def test_streamed_blocks_equal_the_one_shot_convolution(dev, L):
    total = sum(STREAM_BLOCKS)
    assert total == 15000
    rng = np.random.default_rng([L, total])
    x, h = _integers(rng, (total, 2)), _taps(rng, (L, 2))
    zeros = np.zeros((L - 1, 2), dtype=np.float32)
    want, _ = _integer_conv(x, h, zeros)
    hist, pos, parts = zeros, 0, []
    for n in STREAM_BLOCKS:
        y, hist = _direct_conv(dev, x[pos:pos + n], h, hist)
        parts.append(y)
        pos += n
    got = np.concatenate(parts)
    assert np.array_equal(got, want), _first_miss(got, want)
    assert np.array_equal(hist, x[total - (L - 1):])


# ------------------------------------------------------------------------------------------------- layer A'': the fold
RUN_EDGE_TAPS = [2047, 4096, 8193]
RUN_EDGE_FRAMES = 5000


@gpu
@pytest.mark.parametrize("L", RUN_EDGE_TAPS)
def test_float32_runs_end_at_the_fold(dev, L):
    """Integers in [100, 123], all positive.  A float32 run of the documented length, at most 1024 + 16 taps, reaches
    at most 1040 * 123^2 = 15 734 160 < 2^24 and is exact; the float64 folds and partials are exact; the one float32
    rounding of the total (up to 1.3e8) is to nearest even -- so the result is float32(exact integer sum), bit for bit.
    A run that goes on past the fold is not exact: after 2047 taps it holds at least 2047 * 100^2 > 2^24, where odd
    sums are lost one by one, far more of them than the last rounding can hide.  (Layer B' cannot see this: 4096-tap
    runs are only twice as far from float64 as 1024-tap runs, inside its factor of four.)"""
    n = RUN_EDGE_FRAMES
    p = _plan(n, L, 2)
    assert p.kc == 4096 and p.n_chunks == _ceil_div(L, 4096) and p.tile_groups == 2
    assert (FOLD_TAPS + 16) * 123 ** 2 < 2 ** 24 < 2047 * 100 ** 2
    rng = np.random.default_rng([L, n, 5])
    x, h, hist = (rng.integers(100, 124, size=s).astype(np.float32) for s in ((n, 2), (L, 2), (L - 1, 2)))
    got, got_hist = _direct_conv(dev, x, h, hist)
    want, want_hist = _integer_conv(x, h, hist, below=L * 123 ** 2 + 1)
    assert float(np.max(want)) > 2 ** 24
    assert np.array_equal(got, want), _first_miss(got, want)
    assert _bit_equal(got_hist, want_hist)


# ------------------------------------------------------------------------------------------------- layer B
FLOAT_TAPS = [129, 1024, 2047, 8193]
FLOAT_FRAMES = [1000, 9000]
U32 = 2.0 ** -24                # unit roundoff of float32


def _float_inputs(rng, L, n, src_ch, fir_ch):
    out_ch = max(src_ch, fir_ch)
    x = (rng.standard_normal((n, src_ch)) * 0.1).astype(np.float32)
    h = (rng.standard_normal((L, fir_ch)) * np.exp(-np.arange(L) / (L / 8.0))[:, None]).astype(np.float32)
    hist = (rng.standard_normal((L - 1, out_ch)) * 0.1).astype(np.float32)
    return x, h, hist


def _float_reference(x, h, hist):
    """-> (the float64 convolution of the float32 inputs, its pointwise limit, the history it leaves).

    The limit, from the header of csrc/pgx_convolve.hip: float32 accumulation runs of at most 1024 + 16 taps (1100
    here), each add allowed twice the unit roundoff because the order inside one MFMA is not specified; the runs are
    folded and summed in float64 (nothing next to 2^-24); one final rounding to float32:
        |got - want| <= 2 * 1100 * 2^-24 * (|x| * |h|) + 2^-24 * |want| + 1e-30."""
    n, L = x.shape[0], h.shape[0]
    ext, hh = _extended(x, h, hist)
    want = _conv64(ext, hh, L, n)
    mass = _conv64(np.abs(ext), np.abs(hh), L, n)
    bound = 2 * RUN_TAPS * U32 * mass + U32 * np.abs(want) + 1e-30
    return want, bound, ext[n:n + L - 1].astype(np.float32)


def _worst(got, want, bound):
    assert np.all(np.isfinite(got)), f"{int(np.sum(~np.isfinite(got)))} non-finite outputs"
    return float(np.max(np.abs(got.astype(np.float64) - want) / bound))


@gpu
@pytest.mark.parametrize("src_ch,fir_ch", RULES)
@pytest.mark.parametrize("n", FLOAT_FRAMES)
@pytest.mark.parametrize("L", FLOAT_TAPS)
def test_float_convolution_against_float64(dev, L, n, src_ch, fir_ch):
    x, h, hist = _float_inputs(np.random.default_rng([L, n, src_ch, fir_ch, 1]), L, n, src_ch, fir_ch)
    got, got_hist = _direct_conv(dev, x, h, hist)
    want, bound, want_hist = _float_reference(x, h, hist)
    ratio = _worst(got, want, bound)
    print(f"CONV_DIRECT float L={L} n={n} {src_ch}x{fir_ch} max(err/bound)={ratio:.4f}")
    assert ratio <= 1.0, f"max(err / bound) = {ratio:.4f}"
    assert _bit_equal(got_hist, want_hist)


# ------------------------------------------------------------------------------------------------- layer B'
FOLD_FILTER = 131073
FOLD_FRAMES = 4096
FOLD_SEED = 20261
FOLD_FACTOR = 4.0               # accumulation-order differences between the emulation and the matrix pipe


def _emulate(e, h, n, run):
    """y[i] = sum_k h[k] e[L-1+i-k], i < n, in the documented arithmetic, on the CPU: exact-product fused
    multiply-adds into a float32 accumulator in tap order for `run` taps, the runs summed in float64, one rounding to
    float32.  (The product of two float32 is exact in float64; adding it there and rounding to float32 is the fma.)"""
    L = h.size
    S = _ceil_div(L, run)
    h64 = np.zeros(S * run)
    h64[:L] = h
    e64 = np.concatenate([np.zeros(S * run - (L - 1)), e.astype(np.float64)])
    taps = h64.reshape(S, run)
    st = e64.strides[0]
    acc = np.zeros((S, n), dtype=np.float32)
    for t in range(run):                                        # row s, column i: e[L-1 + i - (s*run + t)]
        v = as_strided(e64[S * run - t:], shape=(S, n), strides=(-run * st, st), writeable=False)
        acc = (acc + taps[:, t:t + 1] * v).astype(np.float32)
    return acc.astype(np.float64).sum(axis=0).astype(np.float32)


def _fold_inputs():
    rng = np.random.default_rng(FOLD_SEED)
    x = (rng.standard_normal(FOLD_FRAMES) * 0.1).astype(np.float32)
    h = rng.standard_normal(FOLD_FILTER).astype(np.float32)      # not decaying
    hist = (rng.standard_normal(FOLD_FILTER - 1) * 0.1).astype(np.float32)
    e = np.concatenate([hist, x])
    want = fftconvolve(e.astype(np.float64), h.astype(np.float64))[FOLD_FILTER - 1:FOLD_FILTER - 1 + FOLD_FRAMES]
    return x, h, hist, e, want


def _rms(y, want):
    return float(np.sqrt(np.mean((y.astype(np.float64) - want[:y.shape[0]]) ** 2)))


def test_fold_emulations_are_far_enough_apart():
    """Host only, on the first 1024 outputs of the B' inputs: one float32 run over all 131 073 taps misses float64 by
    more than FOLD_FACTOR times what 1024-tap runs folded in float64 miss it by -- so the limit of the GPU test below
    cannot be met by a kernel that has lost its fold.  Over all 4096 outputs, seed 20261, RMS of the outputs 35.8:
    (a) folded 2.091e-05, (b) one run 2.352e-04, (b) / (a) = 11.25."""
    _, h, _, e, want = _fold_inputs()
    n = 1024
    folded = _rms(_emulate(e, h, n, FOLD_TAPS), want)
    one_run = _rms(_emulate(e, h, n, 1 << 18), want)
    print(f"CONV_DIRECT fold emulation n={n}: folded {folded:.4e} one-run {one_run:.4e}")
    assert one_run > FOLD_FACTOR * folded, (one_run, folded)


@gpu
def test_the_float64_fold_is_there(dev):
    """A 131 073-tap white filter, mono, 4096 frames, seed 20261: the RMS error against float64 is at most 4 x that of
    the CPU emulation of the documented design (float32 runs of 1024 taps folded in float64: 2.091e-05 over these
    outputs; one float32 run over all taps: 2.352e-04, eleven times that and far outside the limit).  The measured
    figure is in profiles/conv_direct_accuracy.md."""
    p = _plan(FOLD_FRAMES, FOLD_FILTER, 1)
    assert (p.kc, p.n_chunks, p.n_split, p.tile_groups) == (4096, 33, 33, 1)
    x, h, hist, e, want = _fold_inputs()
    got, got_hist = _direct_conv(dev, x[:, None], h[:, None], hist[:, None])
    assert np.all(np.isfinite(got))
    folded = _rms(_emulate(e, h, FOLD_FRAMES, FOLD_TAPS), want)
    measured = _rms(got[:, 0], want)
    print(f"CONV_DIRECT fold rms: gpu {measured:.4e} folded-emulation {folded:.4e} ratio {measured / folded:.3f}")
    assert measured <= FOLD_FACTOR * folded, (measured, folded, measured / folded)
    assert _bit_equal(got_hist[:, 0], e[FOLD_FRAMES:])


# ------------------------------------------------------------------------------------------------- layer C
CROSS_TAPS = [2047, 2048, 2049]


def _fft_conv(dev, x, h, hist, fft_size):
    lib = dev.ensure_init()
    n, src_ch = x.shape
    L, fir_ch = h.shape
    out_ch = max(src_ch, fir_ch)
    with guarded():
        hd = dev.DeviceBuffer.from_host(h)
        spec = dev.DeviceBuffer((lib.pgx_convolve_fft_spectrum_bytes(fft_size, fir_ch),), np.uint8)
        dev.check(lib.pgx_convolve_fft_prepare(spec.ptr, hd.ptr, L, fir_ch, fft_size))
        xd = dev.DeviceBuffer.from_host(x)
        histd = dev.DeviceBuffer.from_host(hist)
        ws = dev.DeviceBuffer((lib.pgx_convolve_fft_workspace_bytes(n, L, out_ch, fft_size),), np.uint8)
        out = dev.DeviceBuffer((n, out_ch), np.float32)
        dev.check(lib.pgx_convolve_fft(out.ptr, xd.ptr, n, src_ch, spec.ptr, L, fir_ch, out_ch, fft_size, histd.ptr,
                                       ws.ptr, 0))
        got, got_hist = out.to_host(), histd.to_host()
        del hd, spec, xd, histd, ws, out
    return got, got_hist


@gpu
@pytest.mark.parametrize("src_ch,fir_ch", [(2, 1), (2, 2)])
@pytest.mark.parametrize("L", CROSS_TAPS)
def test_direct_and_fft_paths_agree(dev, L, src_ch, fir_ch):
    """Either side of convolve_pe.FFT_MIN_TAPS, both ABIs on the same x, h and carried history: the outputs differ by
    no more than the two paths' own limits against float64 together (layer B's for the direct form, 1e-6 of the peak
    for the FFT form, the limit of tests/test_gpu_fftconv.py); the histories are the same bits."""
    n = 9000
    lib = dev.ensure_init()
    x, h, hist = _float_inputs(np.random.default_rng([L, n, src_ch, fir_ch, 2]), L, n, src_ch, fir_ch)
    fft_size = int(lib.pgx_convolve_fft_size(L))
    assert fft_size == (4096 if L <= 2048 else 8192)
    direct, direct_hist = _direct_conv(dev, x, h, hist)
    fft, fft_hist = _fft_conv(dev, x, h, hist, fft_size)
    want, bound, want_hist = _float_reference(x, h, hist)
    limit = bound + 1e-6 * float(np.max(np.abs(want)))
    assert np.all(np.isfinite(direct)) and np.all(np.isfinite(fft))
    ratio = float(np.max(np.abs(direct.astype(np.float64) - fft.astype(np.float64)) / limit))
    print(f"CONV_DIRECT direct-vs-fft L={L} {src_ch}x{fir_ch} max(diff/limit)={ratio:.4f} "
          f"direct-vs-f64 {_worst(direct, want, bound):.4f}")
    assert ratio <= 1.0, f"max(|direct - fft| / limit) = {ratio:.4f}"
    assert _bit_equal(direct_hist, fft_hist) and _bit_equal(direct_hist, want_hist)


# ------------------------------------------------------------------------------------------------- PE level
PE_TAPS = [513, 1025, 2047]
PE_BLOCKS = [4800, 17, 1, 9000, 4096]
PE_GAP = (2000, 3000)           # a render that does not continue the previous one: (start, frames)
LONG_BLOCKS = [4097, 4095]
LONG_TAIL = 131072             # frames rendered past the end of the source


def _one_shot(x, h):
    """The integer convolution of the whole signal from cleared history."""
    want, _ = _integer_conv(x, h, np.zeros((max(h.shape[0] - 1, 1), max(x.shape[1], h.shape[1])), dtype=np.float32))
    return want


def _render_blocks(pe, blocks, start=0):
    pos, parts = start, []
    for n in blocks:
        parts.append(np.array(pe.render(pos, n).data))
        pos += n
    return np.concatenate(parts)


@gpu
@pytest.mark.parametrize("L", PE_TAPS)
def test_convolve_pe_streams_through_the_direct_path(dev, L):
    import pygmu2_amd as pg
    from pygmu2_amd import convolve_pe
    assert L < convolve_pe.FFT_MIN_TAPS
    total = sum(PE_BLOCKS)
    rng = np.random.default_rng([L, total, 3])
    x, h = _integers(rng, (total, 2)), _taps(rng, (L, 2))
    want = _one_shot(x, h)
    with guarded():
        pe = pg.ConvolvePE(pg.ArrayPE(x), pg.ArrayPE(h))
        r = pg.NullRenderer(sample_rate=48000)
        r.set_source(pe)
        r.start()
        got = _render_blocks(pe, PE_BLOCKS)
        assert pe._device_fft == 0
        assert got.dtype == np.float32
        assert np.array_equal(got, want), _first_miss(got, want)
        # not contiguous with the last render: the history counts as cleared (the conv_gap_clears_history golden's
        # semantics; at 513 taps with two K-chunks)
        start, n = PE_GAP
        if L == 513:
            assert _plan(n, L, 2).n_chunks == 2
        gap = np.array(pe.render(start, n).data)
        gap_want = _one_shot(x[start:start + n], h)
        assert np.array_equal(gap, gap_want), _first_miss(gap, gap_want)
        # ... and the stream goes on from there
        more = np.array(pe.render(start + n, 700).data)
        more_want = _one_shot(x[start:start + n + 700], h)[n:]
        assert np.array_equal(more, more_want), _first_miss(more, more_want)
        r.stop()
        del pe, r


@gpu
def test_convolve_pe_renders_a_filter_the_fft_path_declines(dev):
    """131 073 taps: pgx_convolve_fft_size answers 0 and ConvolvePE stays on the direct product.  The 8192 source frames
    meet only the first 8192 taps while they are rendered (the history starts as zeros), so the render goes on through
    the tail, one block of 131 072 frames of silence in which every tap, the last one too, meets every source frame."""
    import pygmu2_amd as pg
    L, total = FOLD_FILTER, sum(LONG_BLOCKS)
    assert total == 8192 and dev.ensure_init().pgx_convolve_fft_size(L) == 0
    p = _plan(LONG_BLOCKS[0], L, 2)
    assert (p.kc, p.n_chunks, p.tile_groups, p.n_split) == (4096, 33, 2, 33)
    rng = np.random.default_rng([L, total, 4])
    x, h = _integers(rng, (total, 2)), _taps(rng, (L, 1))
    want = _one_shot(np.concatenate([x, np.zeros((LONG_TAIL, 2), dtype=np.float32)]), h)
    assert np.any(want[L - 1:] != 0)                            # the last tap over the first source frames
    with guarded():
        pe = pg.ConvolvePE(pg.ArrayPE(x), pg.ArrayPE(h))
        r = pg.NullRenderer(sample_rate=48000)
        r.set_source(pe)
        r.start()
        got = _render_blocks(pe, LONG_BLOCKS)
        assert pe._device_fft == 0
        assert np.array_equal(got, want[:total]), _first_miss(got, want[:total])
        tail = np.array(pe.render(total, LONG_TAIL).data)
        assert np.array_equal(tail, want[total:]), _first_miss(tail, want[total:])
        r.stop()
        del pe, r
