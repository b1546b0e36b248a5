#!/usr/bin/env python3
"""`bench.py --dump-outputs DIR` of the C2 workload against the steady tone evaluated in extended precision on the host:
the last timed step's 1 000 000 frames are amp |H| sin(phase0 + arg H + w m / sr) at the frames m bench.py rendered them
at (H from the float64 coefficients BiquadPE uses, everything else in numpy's longdouble: the phase there is 1.4e9 rad,
a float64's ulp of it 2.4e-7, a longdouble's 1e-10).  Two builds that place their anchors differently are each checked
against this, not against each other.  No GPU needed.

    python tools/c2_dump_check.py DIR/c2.npy [--steps 20000] [--warmup 2000] [--tolerance 5e-7]
"""
import os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def steady_tone(first, frames, sr=44100, tone=440.0, cutoff=1000.0, q=0.707):
    sys.path.insert(0, ROOT)
    from pygmu2_amd.biquad_pe import BiquadMode, rbj_coefficients
    L = np.longdouble
    b0, b1, b2, a1, a2 = (L(c) for c in rbj_coefficients(BiquadMode.LOWPASS, cutoff, q, 0.0, float(sr)))
    w = L(2.0 * np.pi * tone)                              # SinePE's float64 (2 pi) f
    d = w / L(sr)
    zr, zi = L(np.cos(d)), L(-np.sin(d))
    z2r, z2i = zr * zr - zi * zi, 2 * zr * zi
    nr, ni = b0 + b1 * zr + b2 * z2r, b1 * zi + b2 * z2i
    dr, di = 1 + a1 * zr + a2 * z2r, a1 * zi + a2 * z2i
    den = dr * dr + di * di
    hr, hi = (nr * dr + ni * di) / den, (ni * dr - nr * di) / den
    m = np.arange(first, first + frames, dtype=np.int64).astype(L)
    phase = w * m / L(sr)                                  # (sinl / cosl reduce the argument themselves)
    return hr * np.sin(phase) + hi * np.cos(phase)


def main(argv):
    path = argv[0]
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 20000
    warmup = int(argv[argv.index("--warmup") + 1]) if "--warmup" in argv else 2000
    tolerance = float(argv[argv.index("--tolerance") + 1]) if "--tolerance" in argv else 5e-7
    got = np.load(path).reshape(-1)
    frames = got.size
    first = (warmup + 1000) * frames + (steps - 1) * frames          # bench.py bench_c2: origin + (steps - 1) frames
    want = steady_tone(first, frames)
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got.astype(np.longdouble) - want)))
    print(f"{path}: frames {first} .. {first + frames - 1}, peak {peak:.4f}, max |got - steady tone| / peak {err / peak:.3e} "
          f"(tolerance {tolerance:.1e})")
    return 0 if err <= tolerance * peak else 1


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1:]))
