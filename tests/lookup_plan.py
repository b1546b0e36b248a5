"""The launch rule of pgx_wavetable (csrc/pgx_lookup.hip wavetable_plan), restated, and the table of cases either side of
each of its switches -- shared by tests/test_lookup_plan_host.py (the export against the restatement, no device) and
tests/test_gpu_lookup_direct.py (every case rendered on the branch it was chosen for)."""

import ctypes as C

BLOCK = 256                     # kBlock
GRID_CAP = 256 * 128            # pgx::grid_for: kNumCU workgroups x 128
LDS_FLOATS = 2560               # kWtLdsFloats
LDS_MAX_FLOATS = 16384          # kWtLdsMaxFloats
ENV = "PGX_WT_LDS_FLOATS"


def restated(n, window_len, channels, cubic, env=None):
    """-> (staged, grid) for valid arguments; env: the text of PGX_WT_LDS_FLOATS, or None when it is not set."""
    floats = window_len * channels
    taps = 4 if cubic else 2
    grid = min(max(-(-n // BLOCK), 1), GRID_CAP)
    limit = min(LDS_FLOATS if env is None else int(env), LDS_MAX_FLOATS)
    if not (floats <= limit and n * taps * channels >= floats):
        return 0, grid
    per_group = -(-floats // (taps * channels))
    groups = n // max(per_group, BLOCK)
    return 1, min(grid, max(groups, 1))


def export(lib, n, window_len, channels, cubic):
    """pgx_wavetable_plan -> (status, staged, grid)."""
    out = (C.c_int * 2)(-7, -7)
    rc = lib.pgx_wavetable_plan(n, window_len, channels, int(cubic), out)
    return rc, out[0], out[1]


# (window_len, channels, cubic, n, staged, grid or None) with PGX_WT_LDS_FLOATS not set
SWITCH_CASES = [
    (2560, 1, 0, 4096, 1, 3),
    (2561, 1, 0, 4096, 0, None),
    (1280, 2, 1, 4096, 1, None),
    (853, 3, 0, 5000, 1, None),             # 2559 floats
    (853, 3, 1, 5000, 1, None),
    (854, 3, 0, 5000, 0, None),             # 2562 floats
    (854, 3, 1, 5000, 0, None),
    (2560, 1, 0, 1280, 1, 1),               # exactly as many gathers as floats
    (2560, 1, 0, 1279, 0, None),
    (2560, 1, 1, 640, 1, None),
    (2560, 1, 1, 639, 0, None),
    (2560, 1, 0, 3000, 1, 2),               # every workgroup walks its stride past a ragged tail
    (4, 1, 0, 1, 0, None),
    (4, 1, 0, 2, 1, 1),
]

# (the text of PGX_WT_LDS_FLOATS, window_len, channels, cubic, n, staged)
ENV_CASES = [
    ("0", 4, 1, 0, 2, 0),
    ("0", 2560, 1, 0, 4096, 0),
    ("0", 1280, 2, 1, 4096, 0),
    ("100000", 16384, 1, 0, 40000, 1),      # clamped to 16 384 floats: a 64 KiB launch
    ("100000", 16385, 1, 0, 40000, 0),
]
