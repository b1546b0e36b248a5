"""CPU: RandomSelectPE's surface against what the fixture records of the reference (tests/golden/random_select_cases.json),
the order in which it consumes its random.Random, and the constants include/pygmu_hip.h shares with device.py."""

import random

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, restart_bank
import fixture_harness as H
import random_select_oracle as R

DATA, NPZ = H.load_cases("random_select")
FACTS = DATA["facts"]


@pytest.fixture(autouse=True)
def _rate():
    pg.set_sample_rate(DATA["sr"])


def _pe(**kw):
    return pg.RandomSelectPE(pg.PeriodicTrigger(hz=10.0), [pg.ConstantPE(1.0), pg.ConstantPE(3.0)], **kw)


def test_bound_but_not_exported():
    assert pg.RandomSelectPE.__name__ == "RandomSelectPE"
    assert "RandomSelectPE" not in pg.__all__


def test_validation_errors_are_the_reference_s():
    trig = pg.PeriodicTrigger(hz=10.0)
    a, b = pg.ConstantPE(1.0), pg.ConstantPE(2.0, channels=2)
    pe = _pe(weights=[1, 2], seed=1)
    refusals = {"no_inputs": lambda: pg.RandomSelectPE(trig, []),
                "weights_length": lambda: pg.RandomSelectPE(trig, [a, b], weights=[1.0]),
                "channel_mismatch": lambda: pe.resolve_channel_count([1, 2, 2, 3]),
                "no_audio_inputs": lambda: pe.resolve_channel_count([1])}
    assert sorted(refusals) == sorted(FACTS["errors"])
    for key, make in refusals.items():
        with pytest.raises(ValueError) as e:
            make()
        assert str(e.value) == FACTS["errors"][key]["text"], key


def test_surface_is_the_reference_s():
    pe = _pe(weights=[1, 2], seed=1)
    assert [type(i).__name__ for i in pe.inputs()] == FACTS["inputs"]
    assert pe.inputs()[0] is pe._trigger and pe.inputs()[1:] == pe._sources
    assert pe.is_pure() is FACTS["pure"] is False
    ext = pe.extent()
    assert [ext.start, ext.end] == FACTS["extent"]
    assert pe.channel_count() == FACTS["channels"]
    assert pe.resolve_channel_count([1, 2, 2]) == FACTS["resolve"]["[1, 2, 2]"]
    assert not getattr(pe, "_LOOK_AHEAD_SAFE", False)


class FakeBank:
    """Stands in for restart_bank.RestartBank: supplies the event count of each block, asks for that many selections."""

    def __init__(self, counts):
        self.counts = list(counts)
        self.origin = None
        self.asked = []                                   # per block: (the active index handed in, the selections)

    def forget(self):
        self.origin = None

    def render(self, start, duration, active, choose):
        count = self.counts.pop(0)
        self.asked.append((active, list(choose(count))))
        if count:
            self.origin = start
        return "the block"


@pytest.mark.parametrize("weights", [None, [0.1, 0.4, 0.2, 0.3]], ids=["uniform", "weighted"])
def test_draws_follow_random_choices_in_order(weights, monkeypatch):
    """on_start: one draw; every event: one; reset_state(): one, and the origin is forgotten; on_stop keeps the
    generator, so the sequence goes on after a stop / start.  Segment k after a start plays draw k + 1."""
    monkeypatch.setattr(restart_bank, "_ENABLED", True)
    seed, n = 1234, 4
    ref = random.Random(seed)
    want = [ref.choices(list(range(n)), weights=weights, k=1)[0] for _ in range(12)]
    pe = pg.RandomSelectPE(pg.PeriodicTrigger(hz=10.0), [pg.ConstantPE(float(v)) for v in range(n)], weights=weights,
                           seed=seed)
    fake = pe._bank = FakeBank([3, 0, 2, 1, 2])
    pe.on_start()                                         # draw 0
    assert pe._selector._active_index == want[0]
    pe._render(0, 100)                                    # three events: draws 1, 2, 3
    pe._render(100, 100)                                  # none: draw 3 runs on
    assert fake.origin == 0 and pe._impl._origin == 0
    pe.reset_state()                                      # draw 4; silence until the next event
    assert pe._impl._origin is None and pe._selector._active_index == want[4]
    pe._render(200, 100)                                  # draws 5, 6
    pe.on_stop()
    assert pe._selector._active_index is None and pe._impl._origin is None
    pe.on_start()                                         # draw 7
    pe._render(300, 100)                                  # draw 8
    pe._render(400, 100)                                  # draws 9, 10
    assert fake.asked == [(want[0], want[1:4]), (want[3], []), (want[4], want[5:7]), (want[7], want[8:9]),
                          (want[8], want[9:11])]
    assert pe._selector._active_index == want[10]


def test_the_composed_selector_draws_the_same_sequence():
    """The selector under TriggerRestartPE: a reset is a draw, whichever path asks."""
    seed, weights = 77, [3, 1, 2]
    ref = random.Random(seed)
    want = [ref.choices([0, 1, 2], weights=weights, k=1)[0] for _ in range(6)]
    sel = pg.RandomSelectPE(pg.PeriodicTrigger(hz=10.0), [pg.ConstantPE(float(v)) for v in range(3)], weights=weights,
                            seed=seed)._selector
    got = []
    sel.on_start()
    got.append(sel._active_index)
    for _ in range(2):
        sel.reset_state()
        got.append(sel._active_index)
    got += sel.draw(3)
    assert got == want


def test_header_constants_match_the_binding():
    header = device._ABI.constants
    tile, segs = header["PGX_RESTART_TILE"], header["PGX_RESTART_MAX_SEGMENTS"]
    assert (tile, segs) == (device.RESTART_TILE, device.RESTART_MAX_SEGMENTS) == (2048, 1024)
    assert header["PGX_RESTART_WORKSPACE_INT64"] == device.RESTART_WORKSPACE_INT64 == 4 * segs == 4 * 1024
    assert device.RESTART_TAKE.itemsize == 24


def test_eligibility():
    """Index-only candidates enter the bank -- SlicePE over such a source too; one that carries state keeps all out."""
    arr = pg.ArrayPE(R.array_data(100, 1, 1))
    assert restart_bank.eligible(pg.SinePE(440.0)) and restart_bank.eligible(pg.SlicePE(arr, 10, 50))
    assert not restart_bank.eligible(pg.BlitSawPE(220.0))
    assert not restart_bank.eligible(pg.SinePE(frequency=pg.SinePE(2.0)))
    assert not restart_bank.eligible(pg.IdentityPE())


def test_the_restatements_on_a_hand_case():
    trig = np.array([0, 1, np.nan, -1, 2, 0, 0, 1, 0, 0], dtype=np.float32)
    assert R.plan(trig) == [3, 1, 7, 3]
    assert R.plan(np.zeros(4, np.float32)) == [0, 4, -1, 0]
    a = np.arange(10, dtype=np.float32).reshape(-1, 1) + 100
    b = np.arange(2, dtype=np.float32).reshape(-1, 1) + 200
    out = R.gather(trig, 1, 5, [0, 1, 0, 1], [(a, 3), (b, 0)])[:, 0]
    # frame 0: local 5 of take 0 (first 3) -> a[2]; event at 1 plays b for 2 frames then silence; event at 4 plays a
    # from local 0, which lies before the take's first frame 3: silence; event at 7 plays b
    assert out.tolist() == [102, 200, 201, 0, 0, 0, 0, 200, 201, 0]
    assert not R.gather(trig, 1, -1, [0, -1, -1, -1], [(a, 0)]).any()
