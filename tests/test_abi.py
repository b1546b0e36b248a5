"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/pygmu_hip.h declares; without a GPU the compute entry points refuse to run
(no silent CPU fallback).  The binding is read from that header (pygmu2_amd/_abi.py): what the reader derives -- every
prototype, every struct layout -- is what a C++ compiler sees in the same file, and the reader refuses what it cannot
read."""

import ctypes
import os
import re
import subprocess

import pytest

from pygmu2_amd import _abi, device
from pygmu2_amd.build import LIB_PATH, _hipcc, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = device._ABI


@pytest.fixture(scope="module")
def lib():
    build()
    return device.load_library()


def _header_text():
    text = open(os.path.join(ROOT, "include", "pygmu_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _header_symbols():
    return sorted(set(re.findall(r"\b(pgx_[a-z0-9_]+)\s*\(", _header_text())))


def test_library_exports_every_declared_symbol(lib):
    declared = _header_symbols()
    assert len(declared) >= 40
    raw = ctypes.CDLL(LIB_PATH)
    missing = [s for s in declared if not hasattr(raw, s)]
    assert not missing, f"declared in pygmu_hip.h but not exported: {missing}"


def test_binding_covers_every_declared_symbol(lib):
    assert sorted(device.EXPORTED_SYMBOLS) == _header_symbols()
    assert lib.pgx_abi_version() == 1


# ---------------------------------------------------------------------------------------------- reader against compiler
# uint64_t before size_t in C++, after it here: where the two are one type both sides say 'u'
KIND = {ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_double: "d", ctypes.c_float: "f", ctypes.c_size_t: "z",
        ctypes.c_uint64: "u"}

PROBE_HEAD = """
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "pygmu_hip.h"
template <class T> constexpr char kind() {
    if (std::is_pointer<T>::value) return 'p';
    if (std::is_same<T, int>::value) return 'i';
    if (std::is_same<T, int64_t>::value) return 'l';
    if (std::is_same<T, double>::value) return 'd';
    if (std::is_same<T, float>::value) return 'f';
    if (std::is_same<T, uint64_t>::value) return 'u';
    if (std::is_same<T, size_t>::value) return 'z';
    return '?';
}
template <class F> struct prototype;
template <class R, class... A> struct prototype<R (*)(A...)> {
    static void print(const char *name) {
        const char kinds[] = {kind<R>(), kind<A>()..., 0};
        printf("F %s %s\\n", name, kinds);
    }
};
int main() {
"""


def _is_pointer(cls):
    return cls in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(cls, ctypes._Pointer)


def _kinds(restype, argtypes):
    return "".join("p" if _is_pointer(c) else KIND[c] for c in [restype] + argtypes)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """The lines of a host program generated from the reader's tables and compiled against the header:
    `S struct sizeof field:offsetof:sizeof ...` and `F function kinds`."""
    lines = [PROBE_HEAD]
    for name, dtype in ABI.structs.items():
        lines.append(f'    printf("S {name} %zu", sizeof({name}));')
        lines += [f'    printf(" {f}:%zu:%zu", offsetof({name}, {f}), sizeof({name}::{f}));' for f in dtype.names]
        lines.append('    printf("\\n");')
    lines += [f'    prototype<decltype(&{name})>::print("{name}");' for name in ABI.functions]
    lines += ["    return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi_probe")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("\n".join(lines))
    args = ["-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    try:
        subprocess.check_call([os.environ.get("CXX") or "g++"] + args)
    except (OSError, subprocess.CalledProcessError):
        subprocess.check_call([_hipcc(), "-x", "c++"] + args)
    return subprocess.check_output([str(exe)], text=True).splitlines()


def test_struct_mirrors_match_c_layout(probe):
    """sizeof of every struct, offsetof and sizeof of every field: the packed dtypes are the compiler's layout."""
    got = [line.split()[1:] for line in probe if line.startswith("S ")]
    want = [[name, str(dt.itemsize)] + [f"{f}:{dt.fields[f][1]}:{dt.fields[f][0].itemsize}" for f in dt.names]
            for name, dt in ABI.structs.items()]
    assert len(want) == 21 and got == want
    assert device.SINE_PARAMS.itemsize == 24
    assert device.SINE_STATEFUL_PARAMS.itemsize == 32
    assert device.BIQUAD_VAR_PARAMS.itemsize == 32
    assert device.BLITSAW_PARAMS.itemsize == 32
    assert device.LADDER_PARAMS.itemsize == 40
    assert device.GATE_PARAMS.itemsize == 24
    assert device.ADSR_PARAMS.itemsize == 40
    assert device.NOISE_STATE.fields["pink"][0].shape == (7,) and device.KS_NOTE.fields["params"][0].str == "<u8"


def test_prototypes_match_the_compiler_s(probe):
    """Arity, every scalar type, and that every pointer is a pointer, for every prototype."""
    got = [tuple(line.split()[1:]) for line in probe if line.startswith("F ")]
    want = [(name, _kinds(res, args)) for name, (res, args) in ABI.functions.items()]
    assert len(want) == len(device._SIGNATURES) >= 165 and got == want
    assert not any("?" in kinds for _, kinds in got)
    assert dict(got)["pgx_reverse_echo"] == "ipplidd" + "pd" * 3 + "plppplplp"
    assert [(n, r, a) for n, (r, a) in ABI.functions.items()] == device._SIGNATURES


HOST_POINTER_FUNCTIONS = [
    "pgx_device_count", "pgx_device_name", "pgx_malloc", "pgx_host_malloc", "pgx_d2h_begin", "pgx_d2h_query",
    "pgx_event_create", "pgx_event_elapsed_ms", "pgx_mix_n", "pgx_biquad_sine_runs_plan", "pgx_comm_info",
    "pgx_comm_stats", "pgx_allreduce_sum", "pgx_allreduce_scalar_host"]


def test_host_pointers_are_typed_and_device_pointers_are_not():
    """PGX_HOST parameter: a typed pointer or c_char_p.  Any other pointer: c_void_p, an integer to ctypes."""
    marked = []
    for name, params in re.findall(r"\b(pgx_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        argtypes = ABI.functions[name][1]
        params = [] if params.strip() == "void" else params.split(",")
        assert len(params) == len(argtypes), name
        for text, cls in zip(params, argtypes):
            if "PGX_HOST" in text:
                marked.append(name)
                assert cls is ctypes.c_char_p or issubclass(cls, ctypes._Pointer), (name, text)
            elif "*" in text or "[" in text:
                assert cls is ctypes.c_void_p, (name, text)
            else:
                assert cls in KIND, (name, text)
    assert sorted(set(marked)) == sorted(HOST_POINTER_FUNCTIONS) and len(marked) == 17
    f = ABI.functions
    assert f["pgx_device_name"][1] == [ctypes.c_char_p, ctypes.c_size_t]
    assert f["pgx_malloc"][1][0] is f["pgx_mix_n"][1][1] is ctypes.POINTER(ctypes.c_void_p)
    assert f["pgx_biquad_sine_runs_plan"][1][2] is ctypes.POINTER(ctypes.c_int)
    assert f["pgx_allreduce_scalar_host"][1][0] is ctypes.POINTER(ctypes.c_double)
    assert f["pgx_last_error"] == (ctypes.c_char_p, []) and f["pgx_stream_handle"] == (ctypes.c_void_p, [])


# ---------------------------------------------------------------------------------------------- the reader is strict
def _header(body):
    return '#ifdef __cplusplus\nextern "C" {\n#endif\n' + body + '\n#ifdef __cplusplus\n}\n#endif\n'


def test_reader_reads_the_forms_of_the_header():
    abi = _abi.parse(_header("""
        typedef enum { PGX_OK = 0, PGX_ERR_INVALID = -1 } pgx_status;
        #define PGX_N 8   /* a comment */
        #define PGX_M (4 * PGX_N + 2)
        #define PGX_X 2.5e-1
        typedef struct { double a, b; const float *p; float q[3]; int32_t pad; } pgx_t;
        size_t pgx_f(void);
        const char *pgx_g(const pgx_t *t, PGX_HOST int64_t *n, int out[5], uint64_t u);
    """))
    assert abi.constants == {"PGX_OK": 0, "PGX_ERR_INVALID": -1, "PGX_N": 8, "PGX_M": 34, "PGX_X": 0.25}
    assert abi.struct("pgx_t") == [("a", "<f8"), ("b", "<f8"), ("p", "<u8"), ("q", "<f4", (3,)), ("pad", "<i4")]
    assert abi.struct("pgx_t").itemsize == 40
    assert abi.functions == {"pgx_f": (ctypes.c_size_t, []),
                             "pgx_g": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                                         ctypes.c_void_p, ctypes.c_uint64])}
    with pytest.raises(_abi.AbiError, match="pgx_lost"):
        abi.struct("pgx_lost")
    with pytest.raises(_abi.AbiError, match="PGX_LOST"):
        abi.constant("PGX_LOST")


@pytest.mark.parametrize("body, complaint", [
    ("int pgx_a(int n);\nint pgx_b(unsigned n);", r"pygmu_hip\.h:5: unknown type 'unsigned'"),
    ("int pgx_a(int n);\nint pgx_b(long long n);", r"pygmu_hip\.h:5: cannot read the declaration"),
    ("int pgx_a(int64_t);", r"pygmu_hip\.h:4: "),
    ("int pgx_a(pgx_later *p);", r"unknown type 'pgx_later'"),
    ("int pgx_a(PGX_HOST void *p);", r"PGX_HOST cannot describe"),
    ("\n\nextern int pgx_errno;", r"pygmu_hip\.h:6: not a #define, enum, struct or prototype"),
    ("int pgx_a(int n) { return n; }", r"pygmu_hip\.h:4: not a #define"),
    ("static inline int pgx_a(int n);", r"cannot read the declaration"),
    ("#define PGX_FLAG", r"pygmu_hip\.h:4: not a #define"),
    ("#include <math.h>", r"pygmu_hip\.h:4: not a #define"),
    ("typedef struct {\n    double a;\n    long b;\n} pgx_t;", r"pygmu_hip\.h:6: cannot read the field 'long b'"),
    ("typedef struct { double a; int (*f)(int); } pgx_t;", r"not a #define|cannot read the field"),
    ("typedef struct { double a : 3; } pgx_t;", r"cannot read the field"),
    ("typedef struct { void v; } pgx_t;", r"cannot read the field"),
    ("typedef struct { double a; int b } pgx_t;", r"field without ';'"),
    ("#define PGX_N sizeof(int)", r"pygmu_hip\.h:4: cannot evaluate 'sizeof\(int\)'"),
    ("#define PGX_N (1 << 4)", r"cannot evaluate"),
    ("#define PGX_N 16u", r"cannot evaluate"),
    ("#define PGX_N (2 * PGX_LATER)", r"cannot evaluate"),
    ("typedef enum { PGX_OK } pgx_status;", r"cannot evaluate"),
])
def test_reader_refuses_what_it_cannot_read(body, complaint):
    with pytest.raises(_abi.AbiError, match=complaint):
        _abi.parse(_header(body))


def test_reader_needs_the_block_and_the_file(tmp_path):
    with pytest.raises(_abi.AbiError, match='extern "C"'):
        _abi.parse("int pgx_a(void);")
    missing = str(tmp_path / "nowhere" / "pygmu_hip.h")
    with pytest.raises(RuntimeError, match=re.escape(missing)):
        _abi.load(missing)
    assert _abi.load(device.HEADER_PATH).functions == ABI.functions


def test_binding_takes_the_status_codes_from_the_header():
    assert (device.ERR_INVALID, device.ERR_NOMEM) == (-1, -4)
    assert ABI.constants["PGX_OK"] == 0 and ABI.constants["PGX_ERR_RUNTIME"] == -2 and ABI.constants["PGX_ERR_NOT_INIT"] == -3
    assert device.CONTROL_WORKSPACE_DOUBLES == 1040 and device.TIMEWARP_WORKSPACE_DOUBLES == 768
    assert device.SCORE_INLINE == 16


@pytest.mark.skipif(device.device_available(), reason="a GPU is present")
def test_no_cpu_fallback_without_gpu(lib):
    import pygmu2_amd as pg
    pg.set_sample_rate(44100)
    with pytest.raises(RuntimeError, match="no HIP device|GPU"):
        pg.SinePE(440.0).render(0, 16)
    # entry points refuse to run before pgx_init
    assert lib.pgx_fill(None, 16, 0.0) == -3
    assert b"pgx_init" in lib.pgx_last_error()
    # pure planning helpers work without a device
    assert lib.pgx_biquad_workspace_bytes(1, 1_000_000, 1, 0) > 0
    assert lib.pgx_biquad_workspace_bytes(512, 48_000, 1, 0) == 0
    assert lib.pgx_biquad_workspace_bytes(1, 1_000_000, 1, 512) == 0      # settled single launch
    assert lib.pgx_biquad_workspace_bytes(1, 1_000_000, 1, 1 << 20) > 0    # too slow a decay: exact pair
    assert lib.pgx_convolve_workspace_bytes(96_000, 65_536, 2) > 0
