"""TralfamPE, SlicePE and SetExtentPE on the CPU, plus the case plumbing shared by the fixture generator
(tools/gen_golden_tralfam.py, over the reference's classes) and the tests (over pygmu2_amd's); tests/fixture_harness.py
loads the fixture and holds the bounds.

(a) The numpy restatement: `mogrify` is the reference's _mogrify (tralfam_pe.py:70-105) with every transform in float64,
    `Sig` / `restate_case` restate the graphs of the cases (finite signals with an extent; integer delay, crop, slice
    with its float32 envelope, set-extent with its extend modes, a counted loop) and TralfamPE._render's slicing.
(b) A numpy model of the DEVICE algorithm: `bluestein_dft` (chirp-z over np.fft of size M = 2^ceil(log2(2N-1)) with the
    chirp phase k^2 mod 2N reduced in integers) and `model_random` (rng.random from the PCG64 skip-ahead of
    tests/noise_oracle.py: u = (raw >> 11) * 2^-53).
(c) Inputs that are bit-reproducible from the json alone: `make_signal` builds the long ones by integer arithmetic -- a
    32-bit hash of the frame index scaled by 2^-23, times an envelope of powers of two; short ones come from the npz.

A case is a dict: "graph" names the shape ("plain", "delay", "loop", "example", "noise_crop", "slice", "set_extent"),
"source" the input signal, "blocks" the renders in order, "store" whether the fixture keeps every sample ("full") or the
sampled frames of one whole-extent render ("sampled": `sample_index`)."""

from __future__ import annotations

import os

import numpy as np

import noise_oracle as P
from fixture_harness import GOLDEN_DIR

F = np.float32
DFT_FACTOR = 8.0             # pgx_dft_c2c: max |X_dev - X_numpy| <= DFT_FACTOR * 2^-52 * max(1, log2 M) * max |X_numpy|
EPS = 2.0 ** -52
SEEDS = (0, 1, 12345, 2 ** 63 + 5, 2 ** 100 + 7)
FULL_STORE_LIMIT = 8192
WINDOW = 1024


# ------------------------------------------------------------------------------------------------- (c) the inputs
def hash32(index: np.ndarray, salt: int) -> np.ndarray:
    """murmur3's 32-bit finaliser of (index * 2654435761 + salt), in uint64 arithmetic masked to 32 bits."""
    m = np.uint64(0xFFFFFFFF)
    h = (index.astype(np.uint64) * np.uint64(2654435761) + np.uint64(salt)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def hashed_noise(n: int, salt: int) -> np.ndarray:
    """Uniform-looking float32 in [-1, 1): the top 24 bits of the hash as a signed integer times 2^-23 (exact)."""
    h = hash32(np.arange(n, dtype=np.uint64), salt)
    return ((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(F) * F(2.0 ** -23)


def decay(n: int) -> np.ndarray:
    """2^-floor(16 i / n): sixteen steps down to 2^-15, every value a power of two."""
    i = np.arange(n, dtype=np.int64)
    return np.ldexp(F(1.0), -((16 * i) // n).astype(np.int32)).astype(F)


def wav_path(name: str) -> str:
    return os.path.join(GOLDEN_DIR, "kemar", name)


def read_wav(name: str) -> np.ndarray:
    """A PCM_16 fixture file as float32 (frames, channels), libsndfile's 1/32768."""
    from pygmu2_amd import wav_io
    path = wav_path(name)
    info = wav_io.read_info(path)
    raw = wav_io.read_frames(path, info, 0, info.frames)
    assert raw.dtype == np.int16, raw.dtype
    return (raw.astype(F) * F(1.0 / 32768.0)).reshape(info.frames, info.channels)


def make_signal(spec: dict, arrays) -> np.ndarray:
    """(frames, channels) float32 of a case's "source"."""
    kind = spec["kind"]
    if kind == "array":
        a = np.asarray(arrays[spec["name"]], dtype=F)
        return a.reshape(-1, 1) if a.ndim == 1 else a
    if kind == "wav":
        return read_wav(spec["file"])
    n, ch = int(spec["n"]), int(spec.get("channels", 1))
    if kind == "noise_decay":
        cols = [hashed_noise(n, 0x9E3779B9 * (c + 1) & 0xFFFFFFFF) * decay(n) for c in range(ch)]
    elif kind == "stereo60":       # the second channel 2^-10 (60.2 dB) below the first
        cols = [hashed_noise(n, 11) * decay(n), hashed_noise(n, 12) * F(2.0 ** -10)]
    elif kind == "dirac":
        cols = [np.zeros(n, dtype=F) for _ in range(ch)]
        for c in range(ch):
            cols[c][(n // 3 + c) % n] = F(1.0)
    elif kind == "dc":
        cols = [np.full(n, F(0.25) / F(c + 1), dtype=F) for c in range(ch)]
    elif kind == "ramp":
        i = np.arange(n, dtype=np.int64)
        cols = [(((i * (c + 1)) % 4096).astype(F) * F(2.0 ** -12) - F(0.5)) for c in range(ch)]
    elif kind == "silence":
        cols = [np.zeros(n, dtype=F) for _ in range(ch)]
    else:
        raise ValueError(f"unknown signal kind {kind!r}")
    return np.stack(cols, axis=1).astype(F)


# ------------------------------------------------------------------------------------------------- (a) the restatement
def mogrify(frames: np.ndarray, seed, normalize_peak) -> np.ndarray:
    """tralfam_pe.py:88-105 with the forward transform in float64 too."""
    x = np.asarray(frames, dtype=np.float64)
    magnitudes = np.abs(np.fft.fft(x, axis=0))
    rng = np.random.default_rng(seed)
    phases = rng.random(x.shape) * 2.0 * np.pi
    out = np.real(np.fft.ifft(magnitudes * np.exp(1j * phases), axis=0)).astype(F)
    if normalize_peak is not None:
        peak = np.max(np.abs(out))
        if peak > 0:
            out *= (F(normalize_peak) / peak)             # a float32 quotient (NEP 50), a float32 product
    return out


class Sig:
    """A finite signal: `data` (frames, channels) at [start, start + frames), zeros elsewhere.  start None: no extent
    on either side is modelled by the subclasses that need it."""

    def __init__(self, start: int, data: np.ndarray):
        self.start, self.data = int(start), np.asarray(data, dtype=F)

    @property
    def end(self):
        return self.start + self.data.shape[0]

    @property
    def channels(self):
        return self.data.shape[1]

    def render(self, start: int, n: int) -> np.ndarray:
        out = np.zeros((n, self.channels), dtype=F)
        lo, hi = max(start, self.start), min(start + n, self.end)
        if hi > lo:
            out[lo - start:hi - start] = self.data[lo - self.start:hi - self.start]
        return out


def slice_envelope(duration: int, fade_in: int, fade_out: int) -> np.ndarray | None:
    """slice_pe.py:69-81, the same float32 expressions."""
    if not (duration > 0 and (fade_in > 0 or fade_out > 0)):
        return None
    env = np.ones((duration,), dtype=F)
    fi, fo = min(fade_in, duration), min(fade_out, duration)
    if fi > 0:
        ramp = (np.arange(fi, dtype=F) + 1.0) / float(fi)
        env[:fi] = np.minimum(env[:fi], ramp)
    if fo > 0:
        ramp = 1.0 - (np.arange(fo, dtype=F) + 1.0) / float(fo)
        env[-fo:] = np.minimum(env[-fo:], ramp)
    return env


def restate_slice(src: Sig, start: int, duration: int, sr: int, fade_in_seconds, fade_out_seconds) -> Sig:
    """SlicePE as a Sig at [0, duration) (zero frames: an empty Sig of the source's width)."""
    body = src.render(start, duration)
    fi = int(round(fade_in_seconds * sr)) if fade_in_seconds is not None else 0
    fo = int(round(fade_out_seconds * sr)) if fade_out_seconds is not None else 0
    env = slice_envelope(duration, fi, fo)
    if env is not None:
        body = body * env[:, None]
    return Sig(0, body)


def restate_set_extent(src: Sig, start, duration, mode: str, at: int, n: int) -> np.ndarray:
    """extent_window_pe.py:88-157 over a Sig."""
    ws = start
    we = None if duration is None else (duration if start is None else start + duration)
    out = src.render(at, n)
    idx = np.arange(at, at + n)
    first = src.render(ws, 1)[0] if ws is not None else None
    last = src.render(we - 1, 1)[0] if we is not None and we > 0 else None
    if ws is not None:
        before = idx < ws
        out[before] = first if mode in ("hold_first", "hold_both") else 0.0
    if we is not None:
        after = idx >= we
        out[after] = last if (mode in ("hold_last", "hold_both") and last is not None) else 0.0
    return out


def restate_case(case: dict, arrays) -> list:
    """Every block of a case -> list of (frames, channels) float32 arrays; a "noise_crop" case ends with the block of
    the second pull of its NoisePE."""
    sr, graph = case["sr"], case["graph"]
    seed, norm = case.get("seed"), case.get("normalize_peak")
    blocks = [(int(s), int(n)) for s, n in case["blocks"]]
    if graph == "noise_crop":
        rng = np.random.default_rng(case["noise_seed"])
        n = case["source"]["n"]
        src = Sig(0, rng.uniform(-1.0, 1.0, size=n).astype(F).reshape(-1, 1))
        t = Sig(0, mogrify(src.data, seed, norm))
        outs = [t.render(s, k) for s, k in blocks]
        outs.append(rng.uniform(-1.0, 1.0, size=case["after"]).astype(F).reshape(-1, 1))
        return outs
    src = Sig(0, make_signal(case["source"], arrays))
    if graph == "slice":
        sl = restate_slice(src, case["start"], case["duration"], sr, case.get("fade_in_seconds"),
                           case.get("fade_out_seconds"))
        return [sl.render(s, k) for s, k in blocks]
    if graph == "set_extent":
        return [restate_set_extent(src, case["start"], case["duration"], case["extend_mode"], s, k) for s, k in blocks]
    if graph == "delay":
        src = Sig(case["delay"], src.data)
    elif graph == "example":
        d = case["duration"]
        sl = restate_slice(src, case["start"], d, sr, case.get("fade_in_seconds"), case.get("fade_out_seconds"))
        src = Sig(0, sl.render(0, d + 2 * sr))
    t = Sig(src.start, mogrify(src.data, seed, norm))
    if graph == "loop":
        length, count = t.data.shape[0], case["count"]
        outs = []
        for s, k in blocks:
            i = np.arange(s, s + k)
            inside = (i >= 0) & (i < length * count)
            out = np.zeros((k, t.channels), dtype=F)
            out[inside] = t.data[i[inside] % length]
            outs.append(out)
        return outs
    return [t.render(s, k) for s, k in blocks]


# ------------------------------------------------------------------------------------------------- storage
def sample_index(n: int, peak_at: int) -> np.ndarray:
    """The frames a "sampled" case keeps of its one whole-extent render: the first and the last WINDOW, WINDOW around
    n/2 and around the peak, and every ceil(n / 8192)-th frame of the whole span."""
    half = WINDOW // 2
    step = -(-n // FULL_STORE_LIMIT)
    parts = [np.arange(0, WINDOW), np.arange(n - WINDOW, n), np.arange(n // 2 - half, n // 2 + half),
             np.arange(peak_at - half, peak_at + half), np.arange(0, n, step)]
    idx = np.unique(np.concatenate(parts))
    return idx[(idx >= 0) & (idx < n)]


def stored_of(case: dict, outs: list) -> np.ndarray:
    """What the fixture keeps of a case's blocks (channels kept: a (k, C) array)."""
    if case["store"] == "full":
        return np.concatenate(outs)
    assert len(outs) == 1
    return outs[0][sample_index(outs[0].shape[0], case["peak_at"])]


# ------------------------------------------------------------------------------------------------- (b) the device model
def fft_points(n: int) -> int:
    """The power-of-two transform behind length n: n itself, or Bluestein's M >= 2n - 1."""
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def dft_bound(n: int, ref: np.ndarray) -> float:
    return DFT_FACTOR * EPS * max(1.0, float(np.log2(fft_points(n)))) * float(np.max(np.abs(ref)))


def chirp(n: int) -> np.ndarray:
    """b_k = exp(i pi k^2 / n), k < n, with k^2 mod 2n taken in integers first."""
    k = np.arange(n, dtype=np.int64)
    r = (k * k) % (2 * n)
    return np.exp(1j * np.pi * (r.astype(np.float64) / n))


def bluestein_dft(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """The device's route for a 1-D complex x: a power of two goes to the FFT, any other length through the chirp-z."""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[0]
    m = fft_points(n)
    if m == n:
        return np.fft.ifft(x) if inverse else np.fft.fft(x)
    if inverse:
        return np.conj(bluestein_dft(np.conj(x))) / n
    b = chirp(n)
    a = np.zeros(m, dtype=np.complex128)
    a[:n] = x * np.conj(b)
    wrapped = np.zeros(m, dtype=np.complex128)
    wrapped[:n] = b
    wrapped[m - n + 1:] = b[1:][::-1]
    conv = np.fft.ifft(np.fft.fft(a) * np.fft.fft(wrapped))
    return np.conj(b) * conv[:n]


def model_random(seed, offset: int, n: int) -> np.ndarray:
    """Draws offset .. offset + n - 1 of default_rng(seed).random(...), the device's way: the LCG reached by the table
    skip-ahead, XSL-RR, u = (raw >> 11) * 2^-53."""
    state, inc = P.seeded(seed)
    state = P.pcg_skip(state, inc, offset)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        state = (state * P.PCG_MULT + inc) & P.MASK128
        hi, lo = state >> 64, state & P.MASK64
        x, rot = hi ^ lo, hi >> 58
        raw = ((x >> rot) | (x << ((64 - rot) & 63))) & P.MASK64
        out[i] = (raw >> 11) * 2.0 ** -53
    return out


def numpy_random(seed, offset: int, n: int) -> np.ndarray:
    bit_gen = np.random.PCG64(seed)
    if offset:
        bit_gen.advance(offset)
    return np.random.Generator(bit_gen).random(n)


# ------------------------------------------------------------------------------------------------- graphs over classes
def build_case(case: dict, K, arrays):
    """The case's graph over the classes of namespace K (ArrayPE, DelayPE, LoopPE, CropPE, NoisePE, TralfamPE, SlicePE,
    SetExtentPE, ExtendMode, and wav(file name) -> a PE reading tests/golden/kemar/<file>).
    -> (root PE, the TralfamPE or SlicePE / SetExtentPE under test, the NoisePE of a "noise_crop" case or None)."""
    graph = case["graph"]
    seed, norm = case.get("seed"), case.get("normalize_peak")
    if graph == "noise_crop":
        noise = K.NoisePE(seed=case["noise_seed"])
        t = K.TralfamPE(K.CropPE(noise, 0, case["source"]["n"]), seed=seed, normalize_peak=norm)
        return t, t, noise
    spec = case["source"]
    src = K.wav(spec["file"]) if spec["kind"] == "wav" else K.ArrayPE(make_signal(spec, arrays))
    if graph == "slice":
        pe = K.SlicePE(src, case["start"], case["duration"], fade_in_seconds=case.get("fade_in_seconds"),
                       fade_out_seconds=case.get("fade_out_seconds"))
        return pe, pe, None
    if graph == "set_extent":
        pe = K.SetExtentPE(src, case["start"], case["duration"], K.ExtendMode(case["extend_mode"]))
        return pe, pe, None
    if graph == "delay":
        src = K.DelayPE(src, case["delay"])
    elif graph == "example":
        d = case["duration"]
        sl = K.SlicePE(src, case["start"], d, fade_in_seconds=case.get("fade_in_seconds"),
                       fade_out_seconds=case.get("fade_out_seconds"))
        src = K.SetExtentPE(sl, 0, d + 2 * case["sr"])
    t = K.TralfamPE(src, seed=seed, normalize_peak=norm)
    if graph == "loop":
        return K.LoopPE(t, count=case["count"]), t, None
    assert graph in ("plain", "delay", "example"), graph
    return t, t, None


def render_case(case: dict, K, arrays) -> tuple:
    """Every block of the case through K's classes -> (list of arrays, the PE under test)."""
    root, pe, noise = build_case(case, K, arrays)
    if noise is not None:
        noise.on_start()                       # the reference seeds its generator there
    outs = [np.array(root.render(int(s), int(n)).data, dtype=F) for s, n in case["blocks"]]
    if noise is not None:
        outs.append(np.array(noise.render(0, case["after"]).data, dtype=F))
    return outs, pe
