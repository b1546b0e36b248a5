"""Shared by tools/gen_golden_score.py (over the reference's classes) and the score tests (over pygmu2_amd's): the
builder that turns a case of tests/golden/score_cases.json into a graph over a namespace of PE
classes, the block patterns, and numpy restatements the tests check the bank's host tables and kernels against."""

from __future__ import annotations

import numpy as np

SR = 8000


# ---------------------------------------------------------------------------------------------- graphs
def array_data(n: int, channels: int, key: int) -> np.ndarray:
    """Deterministic (n, channels) float32 in [-1, 1], by integer arithmetic (the same on every machine)."""
    i = np.arange(n, dtype=np.int64)[:, None]
    c = np.arange(channels, dtype=np.int64)[None, :]
    v = (i * 7919 + c * 104_729 + key * 1_299_709 + (i * i) % 977) % 2001 - 1000
    return (v.astype(np.float64) / 1000.0).astype(np.float32)


def build_source(K, src):
    """One note source: an unbounded or array PE, cropped to its length when the spec says so."""
    t = src["type"]
    wide = {"channels": src["channels"]} if "channels" in src else {}      # the oscillators: one column, repeated
    if t == "ks":
        kw = {"rho": src["rho"], "seed": src["seed"]}
        if "duration" in src:
            kw.update(duration=src["duration"], rho_damping=src["rho_damping"])
        pe = K.KarplusStrongPE(src["freq"], **kw, **wide)
    elif t == "saw":
        pe = K.BlitSawPE(src["freq"], amplitude=src["amp"], **wide)
    elif t == "sine":
        pe = K.SinePE(src["freq"], amplitude=src["amp"], **wide)
    elif t == "noise":
        pe = K.NoisePE(min_value=-src["amp"], max_value=src["amp"], seed=src["seed"])
    elif t == "array":
        pe = K.ArrayPE(array_data(src["n"], src["channels"], src["key"]))
    else:
        raise ValueError(t)
    if "crop" in src:
        pe = K.CropPE(pe, src["crop"][0], src["crop"][1])
    return pe


def build_case(K, case):
    """The PE under test: a SequencePE (kind "sequence", built with the case's argument form) or the hand-built
    MixPE(DelayPE(CropPE(note, 0, len), start), ...) of the examples (kind "handbuilt")."""
    if case["kind"] == "handbuilt":
        return K.MixPE(*[K.DelayPE(build_source(K, n["src"]), n["start"]) for n in case["notes"]])
    pairs = [(build_source(K, n["src"]), n["start"]) for n in case["notes"]]
    form = case.get("form", "pairs")
    if form == "list":
        return K.SequencePE(pairs, mode=case["mode"])
    if form == "bare":
        return K.SequencePE(pairs[0][0], pairs[0][1], mode=case["mode"])
    return K.SequencePE(*pairs, mode=case["mode"])


def patterns(first: int, end: int):
    """name -> blocks for a score that sounds in [first, end)."""
    def contig(a, b, step):
        return [[s, min(step, b - s)] for s in range(a, b, step)]
    span = end - first
    return {
        "whole": [[first - 100, span + 300]],
        "blocks_256": contig(first - 256, end + 256, 256),
        "blocks_777": contig(first - 100, end + 777, 777),
        "gaps": [[first - 5000, 300], [first + span // 3, 64], [end + 10, 500], [first + span // 2, 1]],
        "seek_back": [[first, 1000], [first + 500, 1000], [first + 1500, 777], [first + 300, 256],
                      [first + 2277, max(1, span - 2277) + 50]],
    }


def expected(case, pattern, npz):
    """The reference's output of `pattern`, concatenated: stored, or -- where the generator found it equal to the
    whole render -- cut from the stored whole render."""
    key = f"{case['name']}/{pattern}"
    if key in npz.files:
        return npz[key]
    assert case["same_as_whole"][pattern]
    whole = npz[f"{case['name']}/whole"]
    w0, wn = case["patterns"]["whole"][0]
    parts = []
    for s, n in case["patterns"][pattern]:
        part = np.zeros((n, whole.shape[1]), dtype=np.float32)
        lo, hi = max(s, w0), min(s + n, w0 + wn)
        if hi > lo:
            part[lo - s:hi - s] = whole[lo - w0:hi - w0]
        parts.append(part)
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------- restatements
def brute_active(starts, ends, a, b):
    return [i for i in range(len(starts)) if starts[i] < b and ends[i] > a and ends[i] > starts[i]]


def brute_tile_lists(first, frames, n_frames, tile):
    n_tiles = -(-n_frames // tile)
    lists = [[] for _ in range(n_tiles)]
    for i, (f, n) in enumerate(zip(first, frames)):
        for t in range(n_tiles):
            if f < (t + 1) * tile and f + n > t * tile:
                lists[t].append(i)
    return lists


def ordered_sum(segments, n_frames, channels):
    """float32 sum in list order of the (first, data (n, channels)) segments where they lie; zero elsewhere."""
    out = np.zeros((n_frames, channels), dtype=np.float32)
    for first, data in segments:
        out[first:first + len(data)] = out[first:first + len(data)] + data
    return out
