"""CPU: NoisePE without a device.  The numpy restatement (tests/noise_oracle.py) reproduces every stored block of the
reference-rendered fixtures (bit for bit wherever the case is compared to the bit); the pure-Python model of the device
algorithm -- skip table, skip-ahead, XSL-RR output, conversion -- equals numpy's own draws at near and far offsets, and
the table compiled into the library equals the one made from Python integers; the class's host side -- validation,
properties, repr, extent, purity, export -- is the reference's as the fixtures recorded it."""

import ctypes

import numpy as np
import pytest

import pygmu2_amd as pg
import noise_oracle as P
import spec_build
from fixture_harness import bits_equal, load_cases, split_blocks, within
from pygmu2_amd import device
from pygmu2_amd.build import build

CASES, NPZ = load_cases("noise")
ALL = CASES["cases"]
BY_NAME = {c["name"]: c for c in ALL}
SEEDS = (0, 1, 12345, 2 ** 63 + 5, 2 ** 100 + 7)
OFFSETS = (0, 1, 2 ** 20 + 3, 2 ** 32 + 1, 2 ** 40)


def build_pg(case):
    return spec_build.build_case(case, (P.KIND,))


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_restatement_equals_fixture(case):
    outs, _ = P.run_case(case)
    flat = NPZ[case["name"]]
    stored = split_blocks(case, flat)
    assert stored
    peak = float(np.max(np.abs(flat)))
    for i, want in stored.items():
        assert within(case["compare"], outs[i], want, peak), f"{case['name']}: block {i} differs ({case['compare']})"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("offset", OFFSETS)
def test_device_model_equals_numpy_draws(seed, offset):
    assert bits_equal(P.model_draws(seed, offset, 300), P.numpy_draws(seed, offset, 300))


def test_device_model_reaches_2_pow_62_and_beyond():
    for seed, offset in ((0, 2 ** 62 + 9), (2 ** 100 + 7, 2 ** 63), (12345, 2 ** 64 - 5)):
        state, inc = P.seeded(seed)
        bit_gen = np.random.PCG64(seed)
        bit_gen.advance(offset)
        assert P.pcg_skip(state, inc, offset) == int(bit_gen.state["state"]["state"])


def test_skip_table_against_python_integers():
    """(M^(2^k), S_(2^k)) by repeated stepping for small k, by the group law for all k, and the compiled table."""
    table = P.skip_table()
    M, mask = P.PCG_MULT, P.MASK128
    assert table[0] == (M, 1) and len(table) == 64
    a, s = 1, 0
    for n in range(1, 2 ** 10 + 1):                       # a = M^n, s = S_n, literally
        s = (s + a) & mask
        a = a * M & mask
        if n & (n - 1) == 0:
            assert table[n.bit_length() - 1] == (a, s)
    for k, (a, c) in enumerate(table):
        assert a == pow(M, 2 ** k, 2 ** 128)
        assert (c * (M - 1) - (a - 1)) & mask == 0        # S_n * (M - 1) == M^n - 1
    build()
    words = np.zeros(256, dtype=np.uint64)
    assert device.load_library().pgx_noise_skip_table(words.ctypes.data_as(ctypes.c_void_p)) == 0
    words = [int(w) for w in words]
    compiled = [((words[4 * k] << 64) | words[4 * k + 1], (words[4 * k + 2] << 64) | words[4 * k + 3]) for k in range(64)]
    assert compiled == table


def test_draws_do_not_depend_on_the_cut():
    rng = np.random.default_rng(9)
    parts = np.concatenate([rng.uniform(-1.0, 1.0, size=n) for n in (1, 7, 64, 1000)]).astype(np.float32)
    assert bits_equal(parts, P.model_draws(9, 0, 1072))
    for mode in P.MODES:
        whole = P.NoiseStream(9, mode, 0.0, 3.0).render(1072)
        cut = P.NoiseStream(9, mode, 0.0, 3.0)
        assert bits_equal(np.concatenate([cut.render(n) for n in (1, 7, 64, 1000)]), whole)


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_host_side_matches_reference(case):
    pe, made = build_pg(case)
    ext = pe.extent()
    assert [ext.start, ext.end] == case["extent"]
    assert len(made) == len(case["new_pes"]) > 0
    for m, ref in zip(made, case["new_pes"]):
        assert repr(m) == ref["repr"]
        assert [m.extent().start, m.extent().end] == ref["extent"] == [None, None]
        assert m.is_pure() is ref["pure"] is False
        assert m.channel_count() == ref["channels"] == 1
        assert m.inputs() == [] == ref["inputs"]
        assert (m.min_value, m.max_value, m.mode.value) == (ref["min_value"], ref["max_value"], ref["mode"])
    assert list(P.NoiseNode(case["graph"], case["sr"]).extent()) == case["extent"]


def test_fixture_covers_what_it_must():
    assert int(CASES["numpy"].split(".")[0]) >= 2
    names = set(BY_NAME)
    for mode in P.MODES:
        for seed in SEEDS:
            case = BY_NAME[f"{mode}_seed_{seed}"]
            assert [n for _, n in case["blocks"]] == [1, 63, 64, 3968] and case["graph"]["seed"] == seed
        assert BY_NAME[f"{mode}_starts_ignored"]["blocks"] == [[0, 128], [1000, 128], [-500, 128], [0, 128]]
        assert BY_NAME[f"{mode}_reset_restart"]["ops"] == {"2": "reset", "4": "restart"}
        assert len(BY_NAME[f"{mode}_stream_64"]["blocks"]) == 16
        for rname, rng in (("unit", [0.0, 1.0]), ("cutoff", [100.0, 2000.0]), ("huge", [-1e6, 1e6]), ("point", [-0.3, -0.3])):
            g = BY_NAME[f"{mode}_range_{rname}"]["graph"]
            assert [g["min_value"], g["max_value"]] == rng
        assert np.all(NPZ[f"{mode}_range_point"] == np.float32(-0.3))
    # a reset and a restart go back to the seed: blocks 2 and 4 repeat block 0
    for mode in P.MODES:
        blocks = split_blocks(BY_NAME[f"{mode}_reset_restart"], NPZ[f"{mode}_reset_restart"])
        assert bits_equal(blocks[2], blocks[0]) and bits_equal(blocks[4], blocks[0]) and not bits_equal(blocks[1], blocks[0])
    rails = NPZ["brown_rails"][:, 0]
    assert rails[3941] == 1.0 and rails[7511] == -1.0 and np.max(np.abs(rails[:3941])) < 1.0
    for name in ("patch_noise_sh_slew_biquad", "graph_biquad_white", "graph_gain_adsr", "graph_comb", "graph_mix_two_seeds",
                 "graph_crop", "graph_delay"):
        assert name in names
    two = P.find_nodes(P.NoiseNode(BY_NAME["graph_mix_two_seeds"]["graph"], 48000))
    assert len(two) == 2 and two[0].kw["seed"] != two[1].kw["seed"]
    assert sum(1 for c in ALL if c.get("fuzz")) >= 30
    for c in ALL:
        kinds = P.kinds_of(c["graph"])
        assert P.KIND in kinds
        if kinds == {P.KIND}:
            assert c["compare"] == "bits", c["name"]
        if "SlewLimiterPE" in kinds:
            assert c["compare"] == "peak", c["name"]
    assert {c["compare"] for c in ALL} == {"bits", "peak", "fuzz"}


def test_export_and_properties():
    for name in ("NoisePE", "NoiseMode"):
        assert getattr(pg, name).__name__ == name
        assert name not in pg.__all__            # entering the fuzz census of exported PEs is a later change
    assert [m.value for m in pg.NoiseMode] == ["white", "pink", "brown"]
    pg.set_sample_rate(48000)
    pe = pg.NoisePE()
    assert (pe.min_value, pe.max_value, pe.seed, pe.mode) == (-1.0, 1.0, None, pg.NoiseMode.WHITE)
    assert pe.inputs() == [] and pe.is_pure() is False and pe.channel_count() == 1
    assert (pe.extent().start, pe.extent().end) == (None, None)
    assert repr(pe) == "NoisePE(mode=white, range=[-1.0, 1.0])"
    pe = pg.NoisePE(0, 5, seed=2 ** 100 + 7, mode=pg.NoiseMode.BROWN)
    assert (pe.min_value, pe.max_value, pe.seed, pe.mode) == (0.0, 5.0, 2 ** 100 + 7, pg.NoiseMode.BROWN)
    assert repr(pe) == "NoisePE(mode=brown, range=[0.0, 5.0])"
    assert pg.NoisePE(2.0, 2.0).max_value == 2.0
    assert isinstance(pe, pg.SourcePE) and pe._LOOK_AHEAD_SAFE and set(pe._STATE_FIELDS) == {"_consumed", "_filter"}


def test_errors_follow_the_reference():
    pg.set_sample_rate(48000)
    with pytest.raises(ValueError, match="NoisePE requires max_value >= min_value"):
        pg.NoisePE(1.0, 0.5)
    for mode in pg.NoiseMode:
        pe = pg.NoisePE(mode=mode, seed=1)
        with pytest.raises(ValueError, match="duration must be >= 0"):
            pe.render(0, -1)
        empty = pe.render(7, 0)                                   # no kernel, no device needed
        assert empty.start == 7 and empty.duration == 0 and empty.channels == 1
    with pytest.raises(ValueError, match="Unknown NoiseMode: white"):     # a string is not a member: refused at render
        pg.NoisePE(mode="white").render(0, 16)
    with pytest.raises(ValueError, match="draws must be >= 0"):
        pg.NoisePE().advance(-1)


def test_struct_mirrors_match_c_layout():
    assert device.NOISE_PARAMS.itemsize == 56 and device.NOISE_STATE.itemsize == 32
    assert device.NOISE_PARAMS.fields["consumed"][1] == 32 and device.NOISE_PARAMS.fields["span"][1] == 44
