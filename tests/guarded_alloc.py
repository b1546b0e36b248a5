"""A guarded, poisoning device allocator for tests: `with guarded() as g:` puts a 16 KiB guard band on either side of
every device allocation the PE layer makes inside the block, fills the payload with 0xFF, and at the end of the block
reads every guard back and raises one GuardViolation (an AssertionError) that lists what was damaged.

How it hooks in.  Every device allocation made from Python goes through two attributes of the loaded library object:
`pgx_malloc` in DeviceBuffer.__init__ and `pgx_free` in DeviceBuffer.__del__ (pygmu2_amd/device.py).  Inside the block
both are replaced, on that object, by Python callables.  A request of `bytes` becomes a real pgx_malloc(bytes + 2 * G)
and the caller gets raw + G; G is a multiple of 256, so the payload keeps the 256-byte alignment the kernels'
aligned16 tests see in production.  32-bit word i of a guard is 0xFFF00000 | (i & 0xFFFFF): every word a float32 NaN,
every aligned pair a float64 NaN, no two words equal -- a read overrun that is used puts NaN into the output, and a
constant-valued write overrun cannot reproduce the pattern.  (0xFFC00000 | i, the float32 quiet-NaN prefix alone, leaves
the float64 exponent at 0x7FC: a finite -1e307.  Bits 20 and 21 are set too, so that the pair is a NaN as well.)
The payload's 0xFF bytes are NaN as float32 and float64 and -1 as signed integers, so scratch that is read before it
is written shows as well; DeviceBuffer(zero=True) zeroes its payload afterwards, as before.

Frees inside the block are deferred (DeviceBuffer.__del__ swallows exceptions, nothing may raise there): the block is
quarantined, checked with the live ones at the end of the `with`, and only then really freed -- so nothing allocated
inside ever shares pool memory with something freed inside.  A buffer that outlives the block stays registered: the
free wrapper stays installed for the rest of the process once used, translates such a pointer back to its raw block,
and passes pointers it does not know straight through.

The sizing functions of include/pygmu_hip.h (every pgx_*_bytes but the comm layer's: SIZING_PREFIXES names the
families) are wrapped the same way while a block is open, to count which of them the rendered graphs asked:
`g.sizing_calls`.

Offsets in a report are relative to the payload's edge: in the back guard 0 is the first byte past the payload; in the
front guard -1 is the byte just before it.

Not covered: allocations the library makes for itself in C++ never pass through Python and carry no guards (today
the comm layer's two scratch words; a DFT plan is a DeviceBuffer and is guarded when it is made inside a block, but
spectral.plan_for keeps the two latest, so one made by an earlier test is not); an overrun from one voice's row into
the next row of the same [K][n][ch] batch buffer is interior to one allocation and is not seen; and a read overrun
whose value is discarded leaves no trace.
"""

import ctypes as C
import os
import sys
import threading

import numpy as np

G = 16384                       # bytes per guard: one 4096-frame mono tile of float32, the largest step of any tail loop
assert G % 256 == 0
POISON = 0xFF
_WORDS = G // 4
_PATTERN_WORDS = (np.uint32(0xFFF00000) | (np.arange(_WORDS + 1, dtype=np.uint32) & np.uint32(0xFFFFF))).astype("<u4")
_PATTERN_BYTES = _PATTERN_WORDS.view(np.uint8)
STACK_FRAMES = 4                # innermost frames under pygmu2_amd/ kept per allocation
MAX_WORDS_SHOWN = 8

SIZING_PREFIXES = ("pgx_biquad_", "pgx_scan2_", "pgx_envelope_scratch_", "pgx_window_", "pgx_blitsaw_",
                   "pgx_voice_tiles_", "pgx_ladder_", "pgx_comb_", "pgx_slew_scratch_", "pgx_adsr_", "pgx_convolve_",
                   "pgx_convolve_fft_", "pgx_analog_osc_", "pgx_analog_osc_bank_", "pgx_dft_", "pgx_tralfam_",
                   "pgx_reverse_echo_")

_PKG_MARK = os.sep + "pygmu2_amd" + os.sep


def guard_pattern(phase=0):
    """The G bytes a guard holds whose first byte sits `phase` bytes past a 4-byte boundary (0 for the front guard and
    for every payload whose size is a multiple of four): the aligned words are the pattern's words."""
    return _PATTERN_BYTES[phase:phase + G]


def is_sizing_name(name):
    """A function that sizes device memory for a kernel (pgx_comm_unique_id_bytes sizes a host blob)."""
    return name.startswith("pgx_") and name.endswith("_bytes") and not name.startswith("pgx_comm_")


def sizing_names(lib):
    """The sizing functions the library object carries (device.load_library declares every prototype, so they are
    attributes of the object already)."""
    return sorted(n for n in set(dir(lib)) | set(vars(lib)) if is_sizing_name(n))


def _is_exact_fit(nbytes):
    return nbytes >= 256 and nbytes & (nbytes - 1) == 0


class Violation:
    __slots__ = ("bytes", "side", "first", "last", "words", "stack")

    def __init__(self, nbytes, side, first, last, words, stack):
        self.bytes, self.side, self.first, self.last, self.words, self.stack = nbytes, side, first, last, words, stack

    def __str__(self):
        where = " <- ".join(f"{f}:{n} {fn}" for f, n, fn in self.stack) or "(no frame under pygmu2_amd/)"
        return (f"allocation of {self.bytes} bytes: {self.side} guard damaged, bytes {self.first}..{self.last} from the "
                f"payload's edge; words (found/pattern) {' '.join(self.words)}; allocated at {where}")


class GuardViolation(AssertionError):
    def __init__(self, violations):
        self.violations = list(violations)
        super().__init__(f"{len(self.violations)} guard band(s) damaged:\n" + "\n".join(f"  {v}" for v in self.violations))


class _Record:
    __slots__ = ("raw", "user", "bytes", "stack", "owner", "quarantined")


class _Hook:
    """What is installed on one library object: the real entry points, the registry of guarded blocks, the open
    contexts (innermost last)."""

    def __init__(self, lib):
        self.lib = lib
        self.lock = threading.RLock()
        self.records = {}               # user pointer -> _Record
        self.contexts = []
        self.real_malloc = None
        self.real_free = None
        self.real_sizing = {}

    # -- installation
    def enter(self, ctx):
        with self.lock:
            if not self.contexts:
                self.real_malloc = self.lib.pgx_malloc
                self.lib.pgx_malloc = self.malloc
                if self.real_free is None:                      # stays for the rest of the process once used
                    self.real_free = self.lib.pgx_free
                    self.lib.pgx_free = self.free
                for name in sizing_names(self.lib):
                    self.real_sizing[name] = getattr(self.lib, name)
                    setattr(self.lib, name, self._counting(name, self.real_sizing[name]))
            self.contexts.append(ctx)

    def leave(self, ctx):
        with self.lock:
            self.contexts.remove(ctx)
            if not self.contexts:
                self.lib.pgx_malloc = self.real_malloc
                for name, fn in self.real_sizing.items():
                    setattr(self.lib, name, fn)
                self.real_sizing = {}

    def _counting(self, name, fn):
        def sizing(*args):
            with self.lock:
                for ctx in self.contexts:
                    ctx.sizing_calls[name] = ctx.sizing_calls.get(name, 0) + 1
            return fn(*args)
        sizing.__name__ = name
        return sizing

    # -- the replaced entry points
    def malloc(self, ref, nbytes):
        nbytes = int(nbytes)
        raw = C.c_void_p(0)
        rc = self.real_malloc(C.byref(raw), nbytes + 2 * G)
        if rc:
            return rc
        lib, base = self.lib, raw.value
        user = base + G
        rc = (lib.pgx_memcpy_h2d(base, guard_pattern().ctypes.data, G)
              or lib.pgx_memcpy_h2d(user + nbytes, guard_pattern(nbytes % 4).ctypes.data, G))
        with self.lock:
            ctx = self.contexts[-1] if self.contexts else None
            if not rc and ctx is not None and ctx.poison:
                rc = lib.pgx_memset(user, POISON, nbytes)
            if rc:
                self.real_free(base)
                return rc
            rec = _Record()
            rec.raw, rec.user, rec.bytes, rec.owner, rec.quarantined = base, user, nbytes, ctx, False
            rec.stack = _package_frames()
            self.records[user] = rec
            if ctx is not None:
                ctx.records.append(rec)
                ctx.allocations += 1
                ctx.exact_fit += _is_exact_fit(nbytes)
        target = getattr(ref, "_obj", None)                     # C.byref(p): the c_void_p behind it
        if target is None:
            target = ref.contents
        target.value = user
        return 0

    def free(self, ptr):
        ptr = getattr(ptr, "value", ptr)
        if not ptr:
            return 0
        with self.lock:
            rec = self.records.get(ptr)
            if rec is None:
                return self.real_free(ptr)                      # not ours: straight through
            if rec.owner is not None:
                rec.quarantined = True                          # checked, then freed, when its context ends
                return 0
            del self.records[ptr]                               # outlived its context: checked then, freed now
            return self.real_free(rec.raw)


_hooks = {}


def _hook_of(lib):
    hook = _hooks.get(id(lib))
    if hook is None or hook.lib is not lib:
        hook = _hooks[id(lib)] = _Hook(lib)
    return hook


def _package_frames():
    out, f = [], sys._getframe(2)
    while f is not None and len(out) < STACK_FRAMES:
        name = f.f_code.co_filename
        if _PKG_MARK in name:
            out.append((name[name.rindex(_PKG_MARK) + 1:], f.f_lineno, f.f_code.co_name))
        f = f.f_back
    return out


class guarded:
    """with guarded(poison=True) as g: ...   g.allocations, g.exact_fit (requests that were themselves a power of two
    >= 256: no pool slack behind them even without guards), g.sizing_calls {name: count}, g.check() for a check in
    mid-block (-> the violations found so far; nothing is raised before the block ends).  lib: the library object to
    hook (default: the loaded libpygmu_hip.so)."""

    def __init__(self, poison=True, lib=None):
        self.poison = bool(poison)
        self._lib = lib
        self._hook = None
        self.records = []
        self.allocations = 0
        self.exact_fit = 0
        self.sizing_calls = {}
        self.violations = []
        self._seen = set()

    def __enter__(self):
        if self._lib is None:
            from pygmu2_amd import device
            self._lib = device.ensure_init()
        self._hook = _hook_of(self._lib)
        self._hook.enter(self)
        return self

    def check(self):
        """Wait for the device, read both guards of every allocation made in this block back and compare."""
        lib = self._lib
        rc = lib.pgx_stream_sync()
        if rc:
            raise RuntimeError(f"pgx_stream_sync failed with status {rc}")
        got = np.empty(G, dtype=np.uint8)
        for rec in self.records:
            for side, at, phase in (("front", rec.raw, 0), ("back", rec.user + rec.bytes, rec.bytes % 4)):
                rc = lib.pgx_memcpy_d2h(got.ctypes.data, at, G)
                if rc:
                    raise RuntimeError(f"pgx_memcpy_d2h of a guard failed with status {rc}")
                want = guard_pattern(phase)
                bad = np.flatnonzero(got != want)
                if bad.size:
                    self._report(rec, side, got, want, int(bad[0]), int(bad[-1]), phase)
        return list(self.violations)

    def _report(self, rec, side, got, want, first, last, phase):
        key = (id(rec), side, first, last)
        if key in self._seen:
            return
        self._seen.add(key)
        shift = 0 if side == "back" else -G
        words = []
        for w in range((first + phase) // 4, (last + phase) // 4 + 1):
            lo, hi = max(w * 4 - phase, 0), min(w * 4 - phase + 4, G)
            if np.any(got[lo:hi] != want[lo:hi]):
                words.append(f"{bytes(got[lo:hi][::-1]).hex()}/{bytes(want[lo:hi][::-1]).hex()}")
                if len(words) == MAX_WORDS_SHOWN:
                    words.append("...")
                    break
        self.violations.append(Violation(rec.bytes, side, first + shift, last + shift, words, rec.stack))

    def __exit__(self, exc_type, exc, tb):
        hook = self._hook
        try:
            self.check()
        except Exception:
            if exc_type is None:
                raise
        finally:
            with hook.lock:
                for rec in self.records:
                    rec.owner = None
                    if rec.quarantined:
                        hook.records.pop(rec.user, None)
                        hook.real_free(rec.raw)
                self.records = []
            hook.leave(self)
        if self.violations:
            if exc_type is None:
                raise GuardViolation(self.violations)
            print(f"guarded(): {GuardViolation(self.violations)}", file=sys.stderr)     # the other exception stands
        return False
