"""CPU: pgx_wavetable_plan -- the staged-or-gathered decision and the grid of pgx_wavetable, exported -- against the
restatement of the rule in tests/lookup_plan.py.  It is host arithmetic and needs neither a device nor pgx_init.
pgx_wavetable calls the same function (csrc/pgx_lookup.hip wavetable_plan); that the two answer bad arguments alike
needs pgx_init and is asserted in tests/test_gpu_lookup_direct.py."""

import pytest

from pygmu2_amd import device
from pygmu2_amd.build import build

from lookup_plan import BLOCK, ENV, ENV_CASES, GRID_CAP, LDS_FLOATS, LDS_MAX_FLOATS, SWITCH_CASES, export, restated

OK = device._ABI.constant("PGX_OK")


@pytest.fixture(scope="module")
def lib():
    build()
    return device.load_library()


@pytest.fixture(autouse=True)
def _no_limit_from_outside(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)


def test_the_restatement_puts_every_case_on_its_branch():
    for window_len, channels, cubic, n, staged, grid in SWITCH_CASES:
        got = restated(n, window_len, channels, cubic)
        assert got[0] == staged and grid in (None, got[1]), (window_len, channels, cubic, n, got)
    for env, window_len, channels, cubic, n, staged in ENV_CASES:
        assert restated(n, window_len, channels, cubic, env)[0] == staged, (env, window_len, channels, cubic, n)


def test_export_answers_the_switch_table(lib):
    for window_len, channels, cubic, n, staged, grid in SWITCH_CASES:
        rc, got_staged, got_grid = export(lib, n, window_len, channels, cubic)
        assert rc == OK and got_staged == staged, (window_len, channels, cubic, n, rc, got_staged)
        assert got_grid == restated(n, window_len, channels, cubic)[1]
        if grid is not None:
            assert got_grid == grid, (window_len, channels, cubic, n, got_grid)


@pytest.mark.parametrize("env", [None, "0", "1", "2559", "2560", "2561", "16383", "16384", "16385", "100000"])
def test_export_follows_the_environment_on_every_call(lib, monkeypatch, env):
    if env is not None:
        monkeypatch.setenv(ENV, env)
    for case in ENV_CASES:
        if case[0] == env:
            assert export(lib, case[4], case[1], case[2], case[3])[:2] == (OK, case[5]), case
    limit = min(LDS_FLOATS if env is None else int(env), LDS_MAX_FLOATS)
    for floats in sorted({1, 4, limit - 1, limit, limit + 1, LDS_MAX_FLOATS, LDS_MAX_FLOATS + 1}):
        if floats < 1:
            continue
        for n in (1, floats // 4, floats // 2, floats, 4 * floats):
            for cubic in (0, 1):
                if n >= 1:
                    assert export(lib, n, floats, 1, cubic) == (OK,) + restated(n, floats, 1, cubic, env), (floats, n)


def test_export_sweeps_every_threshold(lib):
    seen = set()
    # the size limit, in floats, for every channel count that divides its neighbourhood differently
    for channels in (1, 2, 3, 5, 8):
        for window_len in sorted({1, 2, 4, 255, 256, 257} | {LDS_FLOATS // channels + d for d in (-1, 0, 1, 2)}):
            floats = window_len * channels
            for cubic in (0, 1):
                taps = 4 if cubic else 2
                breakeven = -(-floats // (taps * channels))              # the least n with n * taps * channels >= floats
                per_group = max(breakeven, BLOCK)
                sizes = {1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 48000, 1 << 20, BLOCK * GRID_CAP, BLOCK * GRID_CAP + 1}
                sizes |= {breakeven + d for d in (-1, 0, 1)}
                sizes |= {k * per_group + d for k in (1, 2, 3, 17) for d in (-1, 0, 1)}
                for n in sorted(s for s in sizes if s >= 1):
                    want = restated(n, window_len, channels, cubic)
                    assert export(lib, n, window_len, channels, cubic) == (OK,) + want, (n, window_len, channels, cubic)
                    seen.add(want[0])
                    if want[0]:
                        assert 1 <= want[1] <= max(n // per_group, 1)   # each group gathers at least what it stages
    assert seen == {0, 1}
    # beyond the cap of the grid, gathered: 2561 floats
    assert export(lib, 1 << 40, 2561, 1, 0) == (OK, 0, GRID_CAP)
    assert export(lib, 1 << 40, 2560, 1, 0) == (OK, 1, GRID_CAP)


def test_export_refuses_what_pgx_wavetable_refuses(lib):
    """pgx_wavetable: n <= 0 is PGX_OK before anything is looked at and nothing is launched; window_len < 1 or
    channels < 1 is PGX_ERR_INVALID.  The plan says the same, and a null `out` is invalid too."""
    for n in (0, -1, -(1 << 40)):
        assert export(lib, n, 2560, 1, 0) == (OK, 0, 0)
        assert export(lib, n, 0, 0, 1) == (OK, 0, 0)
        assert lib.pgx_wavetable_plan(n, 2560, 1, 0, None) == OK
    for window_len, channels in ((0, 1), (-5, 1), (4, 0), (4, -1), (0, 0)):
        assert export(lib, 4096, window_len, channels, 0) == (device.ERR_INVALID, -7, -7)      # out untouched
        assert b"pgx_wavetable_plan" in lib.pgx_last_error()
    assert lib.pgx_wavetable_plan(4096, 2560, 1, 0, None) == device.ERR_INVALID
    assert export(lib, 4096, 2560, 1, 7) == (OK, 1, 4096 // 640)                               # cubic: any non-zero
