"""
Arbitrary-length float64 DFT on the device (pgx_dft_*, csrc/pgx_spectral.hip).

A power-of-two length is a Stockham FFT held in LDS (up to 2048 points: one launch) or its four-step decomposition; every
other length is Bluestein's chirp-z over the next power of two M >= 2n - 1.  What depends on the length alone -- the
chirp and its spectrum -- is a DftPlan, made once per length and shared by everything that transforms that length
(TralfamPE instances over sources of equal duration).  Lengths up to max_length() = 2^21; a longer one is a ValueError.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from ._kernels import DeviceBuffer, check, lib
from .device import load_library


def max_length() -> int:
    """The longest supported transform (needs no device)."""
    return int(load_library().pgx_dft_max_length())


def check_length(n: int, what: str = "DFT") -> None:
    limit = max_length()
    if n > limit:
        raise ValueError(f"{what}: {n} frames exceed the longest supported transform of {limit} (2^21) frames")


class DftPlan:
    """The part of a transform of `n` points that depends on n alone, resident in HBM."""

    def __init__(self, n: int):
        n = int(n)
        if n < 1:
            raise ValueError(f"DFT length must be >= 1, got {n}")
        check_length(n)
        self.n = n
        self.buf = DeviceBuffer((lib().pgx_dft_plan_bytes(n),), np.uint8)
        check(lib().pgx_dft_plan(self.buf.ptr, n), "pgx_dft_plan")


@lru_cache(maxsize=2)
def plan_for(n: int) -> DftPlan:
    """The plan of length n; the two most recent lengths stay resident (a plan of 2^21 - 1 points is 160 MB)."""
    return DftPlan(n)


def dft(x, inverse: bool = False) -> np.ndarray:
    """numpy.fft.fft / ifft along the last axis of a complex (batch, n) or (n,) host array, computed on the device in
    float64.  A convenience for tests and tools: it uploads, transforms and downloads."""
    a = np.ascontiguousarray(x, dtype=np.complex128)
    flat = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
    batch, n = flat.shape
    if n == 0 or batch == 0:
        return a.copy()
    plan = plan_for(n)
    need = lib().pgx_dft_workspace_bytes(n, batch)
    if not need:
        raise ValueError(f"DFT: unsupported shape (batch {batch}, length {n})")
    work = DeviceBuffer((need,), np.uint8)
    dev = DeviceBuffer.from_host(flat.view(np.float64))
    check(lib().pgx_dft_c2c(dev.ptr, dev.ptr, n, batch, int(bool(inverse)), plan.buf.ptr, work.ptr), "pgx_dft_c2c")
    return dev.to_host().view(np.complex128).reshape(a.shape)
