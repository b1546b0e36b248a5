"""Host: the logic of tests/guarded_alloc.py against a fake library object whose device memory is ctypes host buffers --
layout and alignment, the guard pattern and the poison, what a planted write is reported as, deferred and late frees,
nested and repeated contexts, and that a violation never masks another exception."""

import ctypes as C

import numpy as np
import pytest

import guarded_alloc as GA
from guarded_alloc import G, GuardViolation, guarded


class FakeLib:
    """pgx_malloc / pgx_free / pgx_memset / pgx_memcpy_* / pgx_stream_sync over host memory, 256-byte aligned like the
    pool's blocks, with the bookkeeping the tests ask about."""

    def __init__(self):
        self.live = {}              # pointer -> (backing buffer, bytes)
        self.freed = []
        self.requests = []
        self.syncs = 0

    def pgx_malloc(self, ref, nbytes):
        buf = C.create_string_buffer(int(nbytes) + 256)
        ptr = (C.addressof(buf) + 255) & ~255
        self.live[ptr] = (buf, int(nbytes))
        self.requests.append(int(nbytes))
        ref._obj.value = ptr
        return 0

    def pgx_free(self, ptr):
        ptr = getattr(ptr, "value", ptr)
        if ptr not in self.live:
            return -1
        del self.live[ptr]
        self.freed.append(ptr)
        return 0

    def pgx_memset(self, ptr, value, nbytes):
        C.memset(ptr, value, nbytes)
        return 0

    def pgx_memcpy_h2d(self, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0

    def pgx_memcpy_d2h(self, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0

    def pgx_stream_sync(self):
        self.syncs += 1
        return 0

    def pgx_window_workspace_bytes(self, n, ch, half):
        return 4 * n * ch + half

    def pgx_comm_unique_id_bytes(self):
        return 128


def alloc(lib, nbytes):
    """What DeviceBuffer.__init__ does."""
    p = C.c_void_p(0)
    assert lib.pgx_malloc(C.byref(p), nbytes) == 0
    return p.value


def peek(ptr, n):
    return np.frombuffer(C.string_at(ptr, n), dtype=np.uint8)


def poke(ptr, value=None):
    """One byte written; by default one that differs from what is there."""
    C.memset(ptr, C.string_at(ptr, 1)[0] ^ 0xFF if value is None else value, 1)


def test_pattern_words_are_distinct_nans():
    words = GA.guard_pattern().view("<u4")
    assert words.size == G // 4 and np.unique(words).size == words.size
    assert words[0] == 0xFFF00000 and words[5] == 0xFFF00005
    assert np.all(np.isnan(words.view("<f4"))) and np.all(np.isnan(words.view("<f8")))
    assert G % 256 == 0 and G == 4096 * 4


@pytest.mark.parametrize("nbytes", [1, 4, 255, 256, 1000, 4096, 16384, 65536 + 2])
def test_layout_alignment_pattern_and_poison(nbytes):
    lib = FakeLib()
    with guarded(lib=lib) as g:
        p = alloc(lib, nbytes)
        assert lib.requests == [nbytes + 2 * G]
        raw = next(iter(lib.live))
        assert p == raw + G and p % 256 == 0
        assert np.array_equal(peek(raw, G), GA.guard_pattern())
        assert np.all(peek(p, nbytes) == 0xFF)
        back = peek(p + nbytes, G)
        assert np.array_equal(back, GA.guard_pattern(nbytes % 4))
        # the aligned words of the back guard are the pattern's words whatever the payload's size
        skip = (-nbytes) % 4
        assert np.array_equal(back[skip:skip + 8].view("<u4"), GA.guard_pattern().view("<u4")[(skip > 0):(skip > 0) + 2])
        assert np.all(np.isnan(peek(p, nbytes)[:nbytes // 4 * 4].view("<f4")))
    assert g.allocations == 1
    assert g.exact_fit == (1 if nbytes in (256, 4096, 16384) else 0)


def test_poison_off_leaves_the_payload_alone():
    lib = FakeLib()
    with guarded(poison=False, lib=lib):
        p = alloc(lib, 64)
        assert not np.any(peek(p, 64))                  # create_string_buffer's zeros


def test_clean_run_reports_nothing_and_counts():
    lib = FakeLib()
    with guarded(lib=lib) as g:
        ptrs = [alloc(lib, n) for n in (100, 256, 1024, 3000)]
        for p, n in zip(ptrs, (100, 256, 1024, 3000)):
            C.memset(p, 0x11, n)                        # the whole payload, to the byte
        assert g.check() == []
    assert (g.allocations, g.exact_fit, g.violations) == (4, 2, [])
    assert lib.syncs == 2                               # the check in mid-block, the one at the end


@pytest.mark.parametrize("where,side,offset", [("end", "back", 0), ("far_end", "back", G - 1), ("before", "front", -1),
                                               ("far_before", "front", -G)])
@pytest.mark.parametrize("nbytes", [1024, 1002])
def test_planted_one_byte_write_is_reported(where, side, offset, nbytes):
    lib = FakeLib()
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib):
            p = alloc(lib, nbytes)
            alloc(lib, 512)                             # a clean neighbour: not reported
            target = {"end": p + nbytes, "far_end": p + nbytes + G - 1, "before": p - 1, "far_before": p - G}[where]
            poke(target)
    (v,) = e.value.violations
    assert (v.bytes, v.side, v.first, v.last) == (nbytes, side, offset, offset)
    assert len(v.words) == 1 and v.words[0].split("/")[0] != v.words[0].split("/")[1]
    text = str(e.value)
    assert f"{nbytes} bytes" in text and f"{side} guard" in text and f"{offset}..{offset}" in text


def test_a_run_of_damaged_words_is_listed_as_hex():
    lib = FakeLib()
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib):
            p = alloc(lib, 4096)
            C.memmove(p + 4096, np.full(3, 1.1, np.float32).ctypes.data, 12)
    (v,) = e.value.violations
    assert (v.side, v.first, v.last) == ("back", 0, 11)
    assert v.words == ["3f8ccccd/fff00000", "3f8ccccd/fff00001", "3f8ccccd/fff00002"]


def test_a_constant_overrun_equal_to_one_pattern_word_is_still_seen():
    lib = FakeLib()
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib):
            p = alloc(lib, 256)
            C.memmove(p + 256, np.full(4, 0xFFF00000, "<u4").ctypes.data, 16)
    (v,) = e.value.violations
    assert (v.first, v.last) == (4, 12)                 # word 0 is the pattern's own; bytes 4, 8 and 12 differ


def test_mid_block_check_collects_without_raising_and_does_not_repeat():
    lib = FakeLib()
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib) as g:
            p = alloc(lib, 256)
            poke(p - 1)
            found = g.check()
            assert len(found) == 1 and found[0].side == "front"
    assert len(e.value.violations) == 1


def test_deferred_free_really_frees_once_at_exit():
    lib = FakeLib()
    with guarded(lib=lib):
        p = alloc(lib, 300)
        raw = p - G
        assert lib.pgx_free(p) == 0
        assert raw in lib.live and lib.freed == []      # quarantined
        q = alloc(lib, 300)
        assert q != p                                   # so never handed out again inside the block
        assert lib.pgx_free(p) == 0                     # a second free of the same pointer changes nothing
    assert lib.freed == [raw]
    assert list(lib.live) == [q - G]
    assert lib.pgx_free(q) == 0
    assert lib.freed == [raw, q - G] and not lib.live


def test_quarantined_blocks_are_still_checked():
    lib = FakeLib()
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib):
            p = alloc(lib, 300)
            poke(p + 300)
            lib.pgx_free(p)
    assert e.value.violations[0].bytes == 300 and not lib.live


def test_buffer_freed_after_the_context_is_freed_by_its_raw_pointer():
    lib = FakeLib()
    with guarded(lib=lib):
        p = alloc(lib, 1000)
    outside = alloc(lib, 64)                            # the real malloc again: no guards, no offset
    assert lib.requests == [1000 + 2 * G, 64]
    assert lib.pgx_free(p) == 0 and lib.freed == [p - G]
    assert lib.pgx_free(outside) == 0 and lib.freed == [p - G, outside]     # unknown to the wrapper: straight through
    assert lib.pgx_free(12345) == -1                    # and the library's own answer comes back
    assert lib.pgx_free(None) == 0 and lib.pgx_free(0) == 0


def test_repeated_and_nested_contexts():
    lib = FakeLib()
    real = lib.pgx_malloc
    for _ in range(2):
        with guarded(lib=lib) as g:
            lib.pgx_free(alloc(lib, 256))
        assert g.allocations == 1 and lib.pgx_malloc == real and not lib.live
    with guarded(lib=lib) as outer:
        a = alloc(lib, 256)
        with pytest.raises(GuardViolation) as e:
            with guarded(lib=lib) as inner:
                b = alloc(lib, 512)
                poke(b + 512)
                lib.pgx_free(a)                         # the outer block's buffer: stays until the outer block ends
        assert [v.bytes for v in e.value.violations] == [512]
        assert (a - G) in lib.live and lib.pgx_malloc != real       # still hooked for the outer block
        c = alloc(lib, 1024)
    assert (inner.allocations, outer.allocations) == (1, 2)         # a and c
    assert lib.pgx_malloc == real and (a - G) not in lib.live
    assert sorted(lib.live) == sorted([b - G, c - G])


def test_a_violation_does_not_mask_a_propagating_exception(capsys):
    lib = FakeLib()
    with pytest.raises(KeyError, match="the real failure"):
        with guarded(lib=lib) as g:
            p = alloc(lib, 256)
            poke(p + 256)
            raise KeyError("the real failure")
    assert len(g.violations) == 1 and "back guard" in capsys.readouterr().err
    assert lib.pgx_malloc.__self__ is lib               # unhooked all the same


def test_failed_allocation_passes_the_status_through():
    lib = FakeLib()
    lib.pgx_malloc = lambda ref, n: -4
    with guarded(lib=lib) as g:
        p = C.c_void_p(0)
        assert lib.pgx_malloc(C.byref(p), 100) == -4 and not p.value
    assert g.allocations == 0


def test_sizing_calls_are_counted_inside_the_block_only():
    lib = FakeLib()
    assert GA.sizing_names(lib) == ["pgx_window_workspace_bytes"]   # the comm layer's is not a kernel's
    lib.pgx_window_workspace_bytes(10, 2, 3)
    with guarded(lib=lib) as g:
        assert lib.pgx_window_workspace_bytes(10, 2, 3) == 83
        lib.pgx_window_workspace_bytes(1, 1, 0)
    lib.pgx_window_workspace_bytes(10, 2, 3)
    assert g.sizing_calls == {"pgx_window_workspace_bytes": 2}


def test_every_listed_prefix_names_a_sizing_function_of_the_header():
    """The coverage condition of tests/test_gpu_guard_bands.py is only as good as this list."""
    from pygmu2_amd import device
    declared = {n for n in device._ABI.functions if n.endswith("_bytes")}
    for prefix in GA.SIZING_PREFIXES:
        assert any(n.startswith(prefix) for n in declared), prefix
    assert {n for n in device.EXPORTED_SYMBOLS if GA.is_sizing_name(n)} == {n for n in declared if GA.is_sizing_name(n)}


def test_allocation_stack_keeps_frames_under_the_package():
    lib = FakeLib()
    code = compile("def from_package(lib, alloc):\n    return alloc(lib, 256)\n",
                   "/somewhere/pygmu2_amd/fake_pe.py", "exec")
    ns = {}
    exec(code, ns)
    with pytest.raises(GuardViolation) as e:
        with guarded(lib=lib):
            def through_device(lib, n):                 # stands for DeviceBuffer.__init__: the frame that calls pgx_malloc
                p = C.c_void_p(0)
                lib.pgx_malloc(C.byref(p), n)
                return p.value
            p = ns["from_package"](lib, through_device)
            poke(p - 1)
    (v,) = e.value.violations
    assert v.stack == [("pygmu2_amd/fake_pe.py", 2, "from_package")]
    assert "pygmu2_amd/fake_pe.py:2 from_package" in str(e.value)


# ---------------------------------------------------------------------------------------------- the sweep's lists
def test_the_sweep_lists_every_fixture_case_and_only_fixture_free_bank_functions():
    """tests/test_gpu_guard_bands.py builds its parameter lists at import: every case of every family's fixture, and
    of the bank modules the functions that ask for nothing but their own parameters and `monkeypatch`."""
    import inspect
    import json
    import os
    import test_gpu_guard_bands as S
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    per_family = {}
    for family, _, _ in S.SWEEP:
        per_family[family] = per_family.get(family, 0) + 1
    for family, fixture in [("cases", "cases.json"), ("channels", "channels_cases.json"), ("fuzz", "fuzz_cases.json")]:
        with open(os.path.join(golden, fixture)) as f:
            assert per_family[family] == len(json.load(f)), family
    for family in ("control", "playback", "noise", "sources", "tralfam", "tuning", "score"):
        with open(os.path.join(golden, f"{family}_cases.json")) as f:
            assert per_family[family] == len(json.load(f)["cases"]), family
    for family in ("random_select", "reverse_echo"):                # one run per (case, pattern)
        with open(os.path.join(golden, f"{family}_cases.json")) as f:
            assert per_family[family] >= len(json.load(f)["cases"]), family
    with open(os.path.join(golden, "channels_cases.json")) as f:
        long = {c["name"] for c in json.load(f) if c["pattern"] == "long"}      # what crosses the dispatchers' switches
    assert long and long <= {name for family, name, _ in S.SWEEP if family == "channels"}
    modules = {e[1].__module__ for e in S.BANKS}
    assert modules == set(S.BANK_MODULES)
    for test_id, fn, kw, wants_monkeypatch in S.BANKS:
        marks = [m.name for m in getattr(fn, "pytestmark", [])]
        assert "usefixtures" not in marks, test_id
        assert set(inspect.signature(fn).parameters) == set(kw) | ({"monkeypatch"} if wants_monkeypatch else set()), test_id
    assert len({e[0] for e in S.BANKS}) == len(S.BANKS)
