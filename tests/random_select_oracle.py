"""Shared by tools/gen_golden_random_select.py (over the reference's classes) and the RandomSelectPE tests (over
pygmu2_amd's): the builder that turns a case of tests/golden/random_select_cases.json into a graph over a namespace of PE
classes, the three block patterns, and numpy restatements of pgx_restart_plan / pgx_restart_gather."""

from __future__ import annotations

import numpy as np

SR = 8000


# ---------------------------------------------------------------------------------------------- graphs
def array_data(n: int, channels: int, key: int) -> np.ndarray:
    """Deterministic (n, channels) float32 in [-1, 1] without a zero, by integer arithmetic (the same everywhere)."""
    i = np.arange(n, dtype=np.int64)[:, None]
    c = np.arange(channels, dtype=np.int64)[None, :]
    v = (i * 7919 + c * 104_729 + key * 1_299_709 + (i * i) % 977) % 2001 - 1000
    v = np.where(v == 0, 1, v)
    return (v.astype(np.float64) / 1000.0).astype(np.float32)


def trigger_data(n: int, events) -> np.ndarray:
    """(n, 1) float32 zeros with events = [[frame, value], ...] written in."""
    out = np.zeros((n, 1), dtype=np.float32)
    for at, value in events:
        out[int(at), 0] = value
    return out


def build(K, spec, made=None):
    """spec -> PE over the classes of namespace K.  made: list that collects the RandomSelectPEs, in build order."""
    if not isinstance(spec, dict):
        return spec
    t = spec["t"]
    sub = lambda s: build(K, s, made)                                          # noqa: E731
    if t == "const":
        return K.ConstantPE(spec["v"], channels=spec.get("ch", 1))
    if t == "sine":
        return K.SinePE(frequency=sub(spec["f"]), amplitude=spec.get("amp", 1.0))
    if t == "saw":
        return K.BlitSawPE(frequency=spec["f"], amplitude=spec.get("amp", 1.0))
    if t == "array":
        return K.ArrayPE(array_data(spec["n"], spec["ch"], spec["key"]))
    if t == "slice":
        return K.SlicePE(sub(spec["src"]), spec["start"], spec["dur"])
    if t == "ptrig":
        return K.PeriodicTrigger(hz=spec["hz"], phase=spec.get("phase", 0.0))
    if t == "atrig":
        return K.ArrayPE(trigger_data(spec["n"], spec["events"]))
    if t == "restart":
        return K.TriggerRestartPE(sub(spec["trigger"]), sub(spec["src"]))
    if t == "rsel":
        pe = K.RandomSelectPE(trigger=sub(spec["trigger"]), inputs=[sub(s) for s in spec["inputs"]],
                              weights=spec.get("weights"), seed=spec.get("seed"))
        if made is not None:
            made.append(pe)
        return pe
    raise ValueError(t)


def contig(start, sizes):
    out, s = [], start
    for n in sizes:
        out.append([s, n])
        s += n
    return out


def patterns(n: int, small: int = 250):
    """name -> blocks over the same [0, n) frames: one block, equal small blocks, ragged blocks with blocks of one frame."""
    equal = contig(0, [small] * (n // small) + ([n % small] if n % small else []))
    sizes, left, k = [], n, 0
    ragged = (1, 63, 1, 64, 65, 257, 1, 511, 100)
    while left > 0:
        s = min(left, ragged[k % len(ragged)])
        sizes.append(s)
        left -= s
        k += 1
    return {"whole": [[0, n]], "equal": equal, "ragged": contig(0, sizes)}


def expected(case, pattern, npz):
    """The reference's output of `pattern`, concatenated: stored, or -- where the generator found it equal to the one
    block render -- the stored one block render."""
    key = f"{case['name']}/{pattern}"
    if key in npz.files:
        return npz[key]
    assert case["same_as_whole"][pattern], key
    return npz[f"{case['name']}/whole"]


def selects(spec) -> bool:
    return isinstance(spec, dict) and (spec["t"] == "rsel" or any(
        selects(v) or (isinstance(v, list) and any(selects(x) for x in v)) for v in spec.values()))


# ---------------------------------------------------------------------------------------------- restatements
def plan(trig: np.ndarray):
    """pgx_restart_plan's summary for one trigger column: [count, first (n), last (-1), longest stretch (0)]."""
    n = len(trig)
    with np.errstate(invalid="ignore"):
        at = np.flatnonzero(trig > 0)
    if not len(at):
        return [0, n, -1, 0]
    return [len(at), int(at[0]), int(at[-1]), int(np.max(np.diff(np.append(at, n))))]


def gather(trig: np.ndarray, channels: int, carry_local: int, sel, takes):
    """pgx_restart_gather: takes = [(data (len, channels) float32, first)], sel[k] = the take of ordinal k (-1: none)."""
    n = len(trig)
    with np.errstate(invalid="ignore"):
        fired = trig > 0
    ordinal = np.cumsum(fired)
    t = np.arange(n, dtype=np.int64)
    last = np.maximum.accumulate(np.where(fired, t, -1))
    local = np.where(ordinal == 0, np.int64(carry_local) + t, t - last)
    out = np.zeros((n, channels), dtype=np.float32)
    sel = np.asarray(sel, dtype=np.int64)
    slot = np.where(ordinal < len(sel), sel[np.minimum(ordinal, len(sel) - 1)], -1)
    if carry_local < 0:
        slot = np.where(ordinal == 0, -1, slot)
    for s, (data, first) in enumerate(takes):
        rel = local - first
        hit = (slot == s) & (rel >= 0) & (rel < len(data))
        out[hit] = data[rel[hit]]
    return out
