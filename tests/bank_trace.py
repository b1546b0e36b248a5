"""
The harness of the CPU launch-trace tests (test_voice_bank_trace.py, test_noise_bank_trace.py, test_pan_bank_trace.py,
test_bank_kinds_trace.py): what a voice bank launches, in which order, on which stream, with which buffers.

voice_bank.py talks to the device through a handful of seams; with stand-ins there `try_build_bank(...).render_mix(...)`
runs without a GPU and every call it would have made is written down:

* the library (`voice_bank.lib()`, `_kernels.lib()`): every pgx_* call with the stream it lands on.  The stand-in keeps
  the stream state itself (pgx_stream_fork / fork_after -> side stream 1, select, join / detach -> main stream 0) and
  answers pgx_stream_is_forked from it.  Launches return 0.  The host-side queries are answered, not recorded:
      pgx_*_segments(instances, ...)  -> 4 below 128 instances, else 1 (both the segmented and the one-segment paths occur)
      pgx_*_bytes(...)                -> 65536
      pgx_biquad_table_doubles()      -> 64
      pgx_voice_tiles_max_warm()      -> 2048
* the buffers (`DeviceBuffer` of voice_bank, device and _kernels): a subclass that allocates nothing.  Buffer number i has
  the base address i << 40, so offset_ptr() and rows() work; from_host / upload are recorded as "h2d" with a short hash of
  the bytes, zero_ / zero=True as "zero", the release (__del__) as "free".
* the events (`device.Event`): "event_record".

Canonical form: one entry per call, [name, stream, args...].  Which arguments are pointers comes from device._SIGNATURES;
a pointer is written "b<k>+<byte offset>" with k the order in which its buffer first appears in the trace (not its
allocation order: moving a lazy allocation changes nothing, aliasing and double-buffer swaps show).  Each pull of the
script adds ["pull", start, frames] and ["return", pointer, frames, channels, row of a window?].  A buffer that is still
alive after gc.collect() at the end of a case is written ["unreleased", "b<k>"].

The launch entries must equal the recorded ones exactly.  No buffer may be released EARLIER than recorded (counted in
entries in front of its release: an early return to the pool is how a side stream ends up reading a recycled block); a
later release is reported (a warning) and wants an explanation.

A fixture is one JSON line [case, trace] per case; `python tests/test_<...>_trace.py --record` writes it (record_main).
No conftest, no fixtures: the test files import what they use.
"""

import functools
import gc
import hashlib
import itertools
import json
import os
import sys
import warnings

import numpy as np
import pytest

BASE_SHIFT = 40
_BASES = itertools.count(1)         # buffer numbers, never reused: a buffer that outlives its case is not mistaken


class Recorder:
    """The trace, the stream state and the address book of one case."""

    def __init__(self, recording=True):
        import ctypes
        from pygmu2_amd import device
        self.recording = recording
        self.entries = []
        self.stream = 0
        self.forked = False
        self.names = {}              # buffer / event number -> canonical name, in order of first appearance
        self.alive = set()           # numbers of the buffers that exist
        self.pointer_args = {name: [i for i, t in enumerate(args) if t is ctypes.c_void_p]
                             for name, _, args in device._SIGNATURES}

    def new_base(self) -> int:
        return next(_BASES) << BASE_SHIFT

    def name(self, address):
        if address is None:
            return None
        base = address >> BASE_SHIFT
        if base not in self.names:
            self.names[base] = f"b{len(self.names)}"
        return f"{self.names[base]}+{address & ((1 << BASE_SHIFT) - 1)}"

    def note(self, what, *args):
        if self.recording:
            self.entries.append([what, self.stream, *args])

    def released(self, address):
        base = address >> BASE_SHIFT
        if self.recording and base in self.names:        # (a buffer no call ever saw: nothing to say)
            self.entries.append(["free", self.names[base]])


class Library:
    """Stands in for the ctypes library: attribute `pgx_<name>` is a function."""

    def __init__(self, rec):
        self._rec = rec

    def pgx_stream_is_forked(self):
        return 1 if self._rec.forked else 0

    def _stream_call(self, name, forked, stream):
        rec = self._rec

        def call(*args):
            rec.note(name, *[rec.name(a) if name == "pgx_stream_fork_after" else a for a in args])
            rec.forked = forked
            rec.stream = args[0] if stream is None else stream
            return 0
        return call

    def __getattr__(self, name):
        if not name.startswith("pgx_"):
            raise AttributeError(name)
        rec = self._rec
        if name.endswith("_segments"):
            fn = lambda instances, *rest: 4 if instances < 128 else 1
        elif name.endswith("_bytes"):
            fn = lambda *args: 65536
        elif name == "pgx_biquad_table_doubles":
            fn = lambda: 64
        elif name == "pgx_voice_tiles_max_warm":
            fn = lambda: 2048
        elif name in ("pgx_stream_fork", "pgx_stream_fork_after"):
            fn = self._stream_call(name, True, 1)
        elif name == "pgx_stream_select":
            fn = self._stream_call(name, True, None)
        elif name in ("pgx_stream_join", "pgx_stream_detach"):
            fn = self._stream_call(name, False, 0)
        elif not rec.recording:
            fn = lambda *args: 0
        else:
            pointers = rec.pointer_args[name]                   # KeyError: not a function of the C ABI

            def fn(*args):
                rec.entries.append([name, rec.stream, *[rec.name(a) if i in pointers else a for i, a in enumerate(args)]])
                return 0
        self.__dict__[name] = fn
        return fn


def install(monkeypatch, recording=True):
    """Put the stand-ins in place (monkeypatch undoes it) -> the Recorder."""
    from pygmu2_amd import _kernels, device, voice_bank
    rec = Recorder(recording)
    library = Library(rec)

    class Buffer(device.DeviceBuffer):
        __slots__ = ()

        def __init__(self, shape, dtype=np.float32, *, zero=False):
            self.shape = tuple(int(v) for v in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
            self.dtype = np.dtype(dtype)
            self.nbytes = self.dtype.itemsize
            for v in self.shape:
                self.nbytes *= v
            self.ptr = rec.new_base()
            self._owner = True
            rec.alive.add(self.ptr >> BASE_SHIFT)
            if zero and self.nbytes:
                rec.note("zero", rec.name(self.ptr))

        @classmethod
        def from_host(cls, array):
            a = np.ascontiguousarray(array)
            buf = cls(a.shape, a.dtype)
            if a.nbytes:
                rec.note("h2d", rec.name(buf.ptr), hashlib.sha1(a.tobytes()).hexdigest()[:8])
            return buf

        def upload(self, array):
            a = np.ascontiguousarray(array, dtype=self.dtype)
            assert a.nbytes == self.nbytes
            if a.nbytes:
                rec.note("h2d", rec.name(self.ptr), hashlib.sha1(a.tobytes()).hexdigest()[:8])

        def zero_(self):
            if self.nbytes:
                rec.note("zero", rec.name(self.ptr))

        def to_host(self):
            raise AssertionError("a bank does not read back")

        begin_to_host = to_host

        def __del__(self):
            if getattr(self, "_owner", False) is True and self.ptr:
                rec.alive.discard(self.ptr >> BASE_SHIFT)
                rec.released(self.ptr)
            self.ptr = 0

    class Event:
        def __init__(self):
            self.ptr = rec.new_base()

        def record(self):
            rec.note("event_record", rec.name(self.ptr))

    for module in (voice_bank, _kernels):
        monkeypatch.setattr(module, "lib", lambda: library)
        monkeypatch.setattr(module, "DeviceBuffer", Buffer)
    monkeypatch.setattr(device, "DeviceBuffer", Buffer)
    monkeypatch.setattr(device, "Event", Event)
    return rec


def run(monkeypatch, voices, pulls, *, switches=(), mix_windows=False, built=None):
    """-> the canonical trace of a bank of `voices()` (called with the stand-ins in place, at 48 kHz) under the script
    `pulls`: (start, frames) pairs and "reset".  switches: {name: value} set on voice_bank; built(bank): asked once the
    bank stands."""
    from pygmu2_amd import config, voice_bank
    rec = install(monkeypatch)
    for switch, value in dict(switches).items():
        monkeypatch.setattr(voice_bank, switch, value)
    monkeypatch.setattr(config, "_sample_rate", 48000)
    inputs = voices()
    bank = voice_bank.try_build_bank(inputs)
    assert bank is not None and bank.k == len(inputs)
    del inputs
    if built is not None:
        built(bank)
    if mix_windows:
        bank.set_mix_windows()
    for pull in pulls:
        if pull == "reset":
            rec.note("reset")
            bank.reset()
            continue
        rec.note("pull", *pull)
        out = bank.render_mix(*pull)
        rec.note("return", rec.name(out.dev.ptr), out.duration, out.channels, bool(out._bank_window))
        del out
    del bank
    gc.collect()
    rec.recording = False
    return rec.entries + [["unreleased", label] for number, label in rec.names.items() if number in rec.alive]


def launches(trace):
    return [entry for entry in trace if entry[0] not in ("free", "unreleased")]


def release_points(trace):
    """buffer -> entries in front of its release (a buffer never released: more than there are)."""
    points, seen = {}, 0
    for entry in trace:
        if entry[0] == "free":
            points[entry[1]] = seen
        elif entry[0] == "unreleased":
            points[entry[1]] = len(trace) + 1
        else:
            seen += 1
    return points


@functools.lru_cache(None)
def recorded(fixture):
    """{case: trace} of a fixture file (read once; nobody changes it)."""
    with open(fixture) as f:
        return {name: trace for name, trace in (json.loads(line) for line in f if line.strip())}


def recorded_names(fixture):
    """The cases of a fixture file in the file's order, repeats and all."""
    with open(fixture) as f:
        return [json.loads(line)[0] for line in f if line.strip()]


def assert_matches(name, got, want):
    """The launches of `got` are those of the recorded `want`, entry for entry; no buffer is released earlier than
    recorded; one released later is a warning."""
    got = json.loads(json.dumps(got))
    a, b = launches(got), launches(want)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"{name}: entry {i} is {x}, recorded {y} (after {a[max(0, i - 3):i]})"
    assert len(a) == len(b), f"{name}: {len(a)} entries, recorded {len(b)}"
    now, then = release_points(got), release_points(want)
    early = {buf: (now.get(buf), at) for buf, at in then.items() if buf not in now or now[buf] < at}
    assert not early, f"{name}: released earlier than recorded (buffer: entries in front now, recorded): {early}"
    late = {buf: (now[buf], at) for buf, at in then.items() if now[buf] > at}
    if late:
        warnings.warn(f"{name}: released later than recorded (buffer: entries in front now, recorded): {late}")


def record_main(fixture, cases, run_case):
    """The `--record` entry point of a trace test file: run_case(monkeypatch, case) of every case, one line each."""
    if sys.argv[1:] != ["--record"]:
        sys.exit(sys.modules["__main__"].__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(fixture, "w") as f:
        for case in cases:
            patch = pytest.MonkeyPatch()
            try:
                trace = run_case(patch, case)
            finally:
                patch.undo()
            f.write(json.dumps([case, trace], separators=(",", ":")) + "\n")
            print(case, len(trace))
