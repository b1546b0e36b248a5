"""
GPU: PortamentoPE and pgx_portamento.  (The module is named to be collected after the test_gpu_* modules: the GPU suite
stood at 5 000 ids before it, and new ids go behind the existing ones, not between them.)

* The PE against every block the reference rendered (tests/golden/portamento.npz), bit for bit.
* One whole render against the same span pulled in blocks of 1, 63, 64, 65 and 1 000 frames -- blocks wholly before the
  second note included -- and against the numpy restatement of the closed form (tests/portamento_oracle.py).
* The C entry under tests/guarded_alloc.py: every buffer guarded, outputs poisoned (0xFF: NaN), inputs read back
  unchanged, every float between and after the lines still poison.  Against the restatement, bit for bit, at batch 1 and
  3 with lines of different lengths, a one-note line and out_stride > n * channels; with a ramp beginning on every lane
  edge of a wave (an item is one frame of a line of several channels, four frames of a mono line; a wave takes 64
  items, a workgroup 1 024 frames), so that the wave finds one ramp for all its lanes or sends each lane to search; on
  a table of many short ramps with shared beginnings; with `out` 4, 8 and 12 bytes off a 16-byte boundary; n = 1 .. 9;
  512 and 513 ramps (read from LDS / from global memory); channels 1, 2, 3; a negative start; launches so long that a
  workgroup takes several runs of 1 024 frames.
* Bad arguments return PGX_ERR_INVALID and write nothing.
* SinePE(frequency=TransformPE(PortamentoPE(notes), func=pitch_to_freq)) equals the same chain over an ArrayPE that
  holds the line's own samples, bit for bit.
"""

import contextlib
import types

import numpy as np
import pytest

import fixture_harness as H
import portamento_oracle as PO
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

DATA, NPZ = H.load_cases(PO.FIXTURE)
CASES = DATA["cases"]
F32, F64 = np.float32, np.float64
SR = 44100
LDS_RAMPS = 512                 # kPortaLdsRamps
WAVE_ITEMS = 64
GROUP_FRAMES = 1024             # kPortaFrames
RESIDENT_GROUPS = 2048          # 256 CUs x 8: beyond this many a workgroup takes more than one run of GROUP_FRAMES


@pytest.fixture(scope="module")
def dev():
    from pygmu2_amd import device
    device.ensure_init()
    return device


@pytest.fixture(autouse=True)
def _sample_rate():
    import pygmu2_amd as pg
    pg.set_sample_rate(SR)
    yield
    pg.set_sample_rate(SR)


# ------------------------------------------------------------------------------------------------- the PE
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_blocks_match_the_reference(case):
    import pygmu2_amd as pg
    pg.set_sample_rate(case["sr"])
    pe = PO.build(pg, case)
    outs = H.render_blocks(pe, case["sr"], case["requests"])
    flat, at = NPZ[case["name"]], 0
    for (s, n), got in zip(case["requests"], outs):
        H.assert_bits(f"{case['name']} [{s}, +{n})", got, flat[at:at + n])
        at += n
    assert at == flat.shape[0]


MELODY = [(69.1, 0, 700), (73.0, 700, 500), (76.5, 1200, 40), (64.25, 1240, 900), (71.0, 1500, 600)]
SPAN = (-300, 2900)             # 300 frames before the first note, 1 000 before the second


@pytest.fixture(scope="module")
def whole():
    """[SPAN) of MELODY in one render, two channels -> (the samples, the restatement's)."""
    import pygmu2_amd as pg
    pg.set_sample_rate(SR)
    pe = pg.PortamentoPE(MELODY, channels=2)
    got = np.array(pe.render(SPAN[0], SPAN[1]).data)
    got.setflags(write=False)
    want = PO.line(PO.table(MELODY, 0.1, 0.3, SR), SPAN[0], SPAN[1], 2)
    return got, want


def test_whole_render_is_the_closed_form(whole):
    got, want = whole
    H.assert_bits("whole render", got, want)
    assert len(np.unique(got[:, 0])) > 500 and np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("block", [1, 63, 64, 65, 1000])
def test_blocks_of_any_length_give_the_whole_render(whole, block):
    import pygmu2_amd as pg
    pe = pg.PortamentoPE(MELODY, channels=2)
    blocks = [[s, min(block, SPAN[0] + SPAN[1] - s)] for s in range(SPAN[0], SPAN[0] + SPAN[1], block)]
    assert blocks[0][0] + blocks[0][1] <= MELODY[1][1]          # at least one block lies wholly before the second note
    outs = H.render_blocks(pe, SR, blocks)
    H.assert_bits(f"blocks of {block}", np.concatenate(outs), whole[0])


def test_pitch_line_drives_an_oscillator_like_its_own_samples():
    import pygmu2_amd as pg
    notes = [(69.0, 0, 1000), (73.0, 1000, 1000), (76.0, 2000, 1000)]
    n = 3000
    line = PO.line(PO.table(notes, 0.05, 0.3, SR), 0, n)
    blocks = [[0, 1000], [1000, 1000], [2000, 1000]]

    def chain(pitch):
        return pg.SinePE(frequency=pg.TransformPE(pitch, func=pg.pitch_to_freq))

    got = np.concatenate(H.render_blocks(chain(pg.PortamentoPE(notes, max_ramp_seconds=0.05)), SR, blocks))
    want = np.concatenate(H.render_blocks(chain(pg.ArrayPE(line)), SR, blocks))
    H.assert_bits("SinePE over the pitch line", got, want)
    assert float(np.max(np.abs(got))) > 0.99


# ------------------------------------------------------------------------------------------------- the C entry
POISON = 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@contextlib.contextmanager
def _buffers(dev, **spec):
    """Guarded device buffers: an array is uploaded (and must come back unchanged), a (shape, dtype) pair stays 0xFF."""
    with guarded() as g:
        bufs = {k: dev.DeviceBuffer.from_host(v) if isinstance(v, np.ndarray) else dev.DeviceBuffer(*v)
                for k, v in spec.items()}
        ns = types.SimpleNamespace(**bufs)
        try:
            yield ns
            assert g.allocations == len(spec)
            for k, v in spec.items():
                if isinstance(v, np.ndarray):
                    got = bufs[k].to_host()
                    assert got.dtype == v.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), \
                        f"the call wrote its input {k!r}"
        finally:
            ns.__dict__.clear()
            bufs.clear()


def _run(dev, tables, start, n, channels, pad=0, skew=0):
    """pgx_portamento over the lines of `tables`, `pad` floats between lines, `out` `skew` floats past the buffer's
    256-byte aligned beginning; asserts the restatement on every line and poison on every float that no line owns."""
    lib = dev.ensure_init()
    batch = len(tables)
    at, length, v0, v1, offsets = PO.pack(tables)
    stride = n * channels + pad
    total = skew + batch * stride + 3
    with _buffers(dev, at=at, length=length, v0=v0, v1=v1, offsets=offsets, out=((total,), F32)) as b:
        assert b.out.ptr % 256 == 0
        dev.check(lib.pgx_portamento(b.out.ptr + 4 * skew, stride, batch, start, n, channels, b.at.ptr, b.length.ptr,
                                     b.v0.ptr, b.v1.ptr, b.offsets.ptr), "pgx_portamento")
        got = b.out.to_host()
    owned = np.zeros(total, bool)
    for k, tab in enumerate(tables):
        lo = skew + k * stride
        owned[lo:lo + n * channels] = True
        H.assert_bits(f"line {k} of {batch}", got[lo:lo + n * channels].reshape(n, channels), PO.line(tab, start, n, channels))
    assert np.all(_bits(got)[~owned] == POISON), "a float outside every line was written"


def _notes_table(notes, **kw):
    return PO.table(notes, kw.get("max_ramp_seconds", 0.1), kw.get("ramp_fraction", 0.3), SR)


def _ramps(at, length, v0, v1):
    return (np.asarray(at, np.int64), np.asarray(length, np.int64), np.asarray(v0, F64), np.asarray(v1, F64))


def _random_table(seed, count, first, span, longest):
    """`count` ramps over [first, first + span): sorted beginnings with ties, lengths 1 .. longest (glides that the next
    ramp cuts, glides that finish), pitches that float32 does not hold."""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.integers(first, first + span, count))
    at[count // 3] = at[count // 3 - 1]                                     # at least one shared beginning
    return _ramps(at, rng.integers(1, longest + 1, count), rng.uniform(20.0, 110.0, count), rng.uniform(20.0, 110.0, count))


LINES = {
    "melody": _notes_table(MELODY),
    "one_note": _notes_table([(61.3, 40, 100)]),
    "two_notes": _notes_table([(50.0, -100, 10), (90.7, 20, 2000)]),
    "dense": _random_table(1, 300, -50, 2200, 30),
}


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("names,pad", [(("melody",), 0), (("melody", "one_note", "dense"), 0),
                                       (("two_notes", "dense", "one_note"), 5)],
                         ids=["batch1", "batch3", "batch3_padded"])
def test_batches_of_lines(dev, channels, names, pad):
    """Lines of 4, 1, 1 and 300 ramps.  Unpadded, the lines of one channel lie 2 053 floats apart and begin 0, 4 and 8
    bytes off a 16-byte boundary; pad = 5 floats between lines is out_stride > n * channels."""
    _run(dev, [LINES[k] for k in names], -37, 2053, channels, pad=pad)


# a ramp beginning `d` frames into the request: on lane 0, 1, 63 of a wave and lane 0 of the next, for waves of 64
# frames (several channels) and of 64 four-frame items (one channel: 256 frames, also inside an item), at the first
# and the last frame of a workgroup's 1 024, and in the second workgroup
EDGES = sorted({w * k + e for w in (WAVE_ITEMS, 4 * WAVE_ITEMS) for k in (0, 1, 2) for e in (-1, 0, 1, 2, 3, 4, 5)}
               | {GROUP_FRAMES + e for e in (-1, 0, 1)} | {GROUP_FRAMES + 4 * WAVE_ITEMS + 1})
EDGES = [d for d in EDGES if d >= 0]


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_a_ramp_begins_on_every_lane_edge(dev, channels):
    start, n = 1000, 1400
    assert {0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1025} <= set(EDGES) and max(EDGES) < n - 10
    misses = []
    for d in EDGES:
        # an earlier ramp that has finished, then the glide that begins d frames in and lasts 10, or 1 (a step)
        for length in (10, 1):
            tab = _ramps([start - 500, start + d], [100, length], [40.1, 47.3], [47.3, 80.9])
            try:
                _run(dev, [tab], start, n, channels)
            except AssertionError as e:
                misses.append(f"[d={d} len={length}] {e}")
    assert not misses, f"{len(misses)} combination(s) failed:\n" + "\n".join(misses)


@pytest.mark.parametrize("skew", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 9, 1031])
def test_out_off_a_16_byte_boundary(dev, skew, n):
    """One channel, `out` 4, 8, 12 bytes past a 16-byte boundary: up to three single frames, whole vectors, up to three
    single frames; the short requests have no whole vector at all, or one."""
    _run(dev, [LINES["dense"]], 777, n, 1, skew=skew)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_a_single_frame(dev, channels):
    for start in (-51, 699, 700, 1239, 1240, 1 << 40):
        _run(dev, [LINES["melody"]], start, 1, channels)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("count", [LDS_RAMPS - 1, LDS_RAMPS, LDS_RAMPS + 1, 3000])
def test_tables_either_side_of_the_lds_limit(dev, channels, count):
    """Ramps about 9 frames apart: a request of 4 099 frames from the table's middle crosses some 450 of them, several
    per wave; one before the table (the first ramp's held value) and one past its end (the last ramp's)."""
    tab = _random_table(count, count, -4000, 9 * count, 12)
    first, last = int(tab[0][0]), int(tab[0][-1])
    for start, n in ((first + (last - first) // 2, 4099), (first - 300, 700), (last - 200, 700)):
        _run(dev, [tab], start, n, channels)
    _run(dev, [tab, LINES["one_note"], tab], first + 100, 1500, channels, pad=1)


@pytest.mark.parametrize("channels,batch,n", [(1, 32, 70_001), (2, 256, 9_001)])
def test_workgroups_that_take_several_runs(dev, channels, batch, n):
    """A launch of more than RESIDENT_GROUPS runs of 1 024 frames gives each workgroup several runs side by side, and
    its waves carry their place in the table from one run to the next: `batch` lines share the grid, so 2 048 / batch
    workgroups per line, and n frames are more runs than that.  Ramps about 170 frames apart, so the place moves on."""
    per_line = RESIDENT_GROUPS // batch
    assert per_line < -(-n // GROUP_FRAMES) <= 2 * per_line
    tables = [_random_table(5, 400, -1000, n + 2000, 300), LINES["melody"], _random_table(6, 600, 0, n, 40), LINES["one_note"]]
    _run(dev, [tables[k % 4] for k in range(batch)], -123, n, channels, pad=2)


def test_negative_and_distant_starts(dev):
    tab = _ramps([-5000, -4000, 1 << 40], [300, 2000, 1000], [60.0, 66.6, 50.0], [66.6, 50.0, 99.9])
    for start in (-5100, -4100, -2100, (1 << 40) - 100):
        for channels in (1, 2):
            _run(dev, [tab], start, 1500, channels)


def test_bad_arguments_are_refused_and_write_nothing(dev):
    lib = dev.ensure_init()
    at, length, v0, v1, offsets = PO.pack([LINES["melody"], LINES["one_note"]])
    n, ch = 64, 2
    with _buffers(dev, at=at, length=length, v0=v0, v1=v1, offsets=offsets, out=((2 * n * ch,), F32)) as b:
        good = dict(out=b.out.ptr, stride=n * ch, batch=2, start=0, n=n, channels=ch, at=b.at.ptr, length=b.length.ptr,
                    v0=b.v0.ptr, v1=b.v1.ptr, offsets=b.offsets.ptr)

        def call(**change):
            a = dict(good, **change)
            return lib.pgx_portamento(a["out"], a["stride"], a["batch"], a["start"], a["n"], a["channels"], a["at"],
                                      a["length"], a["v0"], a["v1"], a["offsets"])

        for change in (dict(out=None), dict(at=None), dict(length=None), dict(v0=None), dict(v1=None), dict(offsets=None),
                       dict(channels=0), dict(channels=-1), dict(stride=n * ch - 1), dict(stride=0), dict(batch=65536)):
            assert call(**change) == dev.ERR_INVALID, change
            assert b"pgx_portamento" in lib.pgx_last_error()
        for change in (dict(n=0), dict(n=-5), dict(batch=0), dict(batch=-1)):
            assert call(**change) == 0, change                     # nothing to do
        assert np.all(_bits(b.out.to_host()) == POISON)             # nothing was launched
        assert call() == 0
        got = b.out.to_host().reshape(2, n, ch)
    for k, name in enumerate(("melody", "one_note")):
        H.assert_bits(name, got[k], PO.line(LINES[name], 0, n, ch))
