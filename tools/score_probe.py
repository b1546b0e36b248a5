"""
Score bank against MixPE's generic path (PYGMU_SCORE_BANK=0: the path every such graph took before the bank existed),
at 48 kHz, on the hand-built MixPE(DelayPE(CropPE(note, 0, len), start), ...) of examples 19 and 29:

  mozart60      example 19's plucked line: 60 KarplusStrongPE notes, polyphony 1-3
  plucks1000    1 000 plucks over 60 s, polyphony about 8
  saws1000      the same score with BlitSawPE notes
  chord64       64 plucks struck together, 2 s

each streamed in 1 024-frame blocks and rendered whole.  Per row and mode: wall time of one pass ending in a device
synchronise, after a warm-up pass, bank on and off (a graph each) alternating in the same process, median of 3 (min and max are kept:
the spread); ms per second of audio; launches per block (the bank's own two kernels, counted by score_bank.STATS, and
the notes it pulls through their own render(); for the generic path the inputs it renders over the whole block plus
its ceil(k / 16) mix launches, counted on the host from the extents); for the whole renders the growth of the device
pool over the render (hipMemGetInfo before and after, the pool trimmed before: what was live at the peak, rounded up
by the pool) next to (sum len_i + T) * 4 bytes.  The two paths' outputs are compared at the timed sizes on fresh
graphs (np.array_equal).  chord64 is also timed with 16 and with 64 strings per workgroup of pgx_karplus_score
instead of the bank's own choice (0 in the table: a wave per string while the chip has room).  The pool's one-off
reserve of larger blocks behind the first large one is switched off (PGX_POOL_RESERVE=0) so that the growth is what
the render asked for.

    python tools/score_probe.py [--quick]      writes profiles/score_probe.jsonl and profiles/score_probe.md
"""

from __future__ import annotations

import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PGX_POOL_RESERVE", "0")
import pygmu2_amd as pg                                   # noqa: E402
from pygmu2_amd import device, score_bank                 # noqa: E402

SR = 48_000
BLOCK = 1024
OUT = os.environ.get("SCORE_PROBE_OUT", os.path.join(ROOT, "profiles"))


def pluck(i, freq):
    return pg.KarplusStrongPE(float(freq), rho=0.996, seed=i)


def saw(i, freq):
    return pg.BlitSawPE(float(freq), amplitude=0.2)


def score(starts, lens, freqs, make):
    notes = [pg.DelayPE(pg.CropPE(make(i, f), 0, int(n)), int(s)) for i, (s, n, f) in enumerate(zip(starts, lens, freqs))]
    return pg.MixPE(*notes)


def rows(quick):
    rng = np.random.default_rng(19)
    k = 60
    lens = (rng.choice([0.125, 0.25, 0.25, 0.5, 0.75], k) * SR).astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(lens[:-1])))
    ring = lens + SR // 4                                    # a pluck rings a quarter second into the next notes
    midi = rng.integers(57, 82, k)
    yield "mozart60", starts, ring, 440.0 * 2.0 ** ((midi - 69) / 12), pluck
    k, seconds = (200, 12) if quick else (1000, 60)
    lens = rng.integers(int(0.24 * SR), int(0.72 * SR), k)   # mean 0.48 s: 1 000 of them over 60 s sound 8 at a time
    starts = np.sort(rng.integers(0, seconds * SR - int(lens.max()), k))
    freqs = np.exp(rng.uniform(np.log(65.0), np.log(1047.0), k))
    yield f"plucks{k}", starts, lens, freqs, pluck
    yield f"saws{k}", starts, lens, freqs, saw
    k = 64
    yield "chord64", np.zeros(k, dtype=np.int64), np.full(k, 2 * SR), 110.0 * 2.0 ** (np.arange(k) / 12.0), pluck


def one_pass(mix, total, streamed):
    device.synchronize()
    t0 = time.perf_counter()
    if streamed:
        for s in range(0, total, BLOCK):
            mix.render(s, min(BLOCK, total - s))
    else:
        mix.render(0, total)
    device.synchronize()
    return time.perf_counter() - t0


def host_counts(starts, lens, total):
    """Generic path, per 1 024-frame block: inputs rendered over the whole block + ceil(k / 16) mix launches."""
    ends = starts + lens
    per = []
    for s in range(0, total, BLOCK):
        k = int(np.sum((starts < s + BLOCK) & (ends > s)))
        per.append(k + -(-k // 16))
    return float(np.mean(per))


def pool_growth(hip, fn):
    device.check(device.ensure_init().pgx_pool_trim(), "pgx_pool_trim")
    device.synchronize()
    free0, free1, tot = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    hip.hipMemGetInfo(ctypes.byref(free0), ctypes.byref(tot))
    out = fn()
    device.synchronize()
    hip.hipMemGetInfo(ctypes.byref(free1), ctypes.byref(tot))
    return out, int(free0.value) - int(free1.value)


def main():
    quick = "--quick" in sys.argv
    pg.set_sample_rate(SR)
    hip = ctypes.CDLL("libamdhip64.so")
    os.makedirs(OUT, exist_ok=True)
    records = []
    for name, starts, lens, freqs, make in rows(quick):
        total = int(np.max(starts + lens))
        total += (-total) % BLOCK
        seconds = total / SR
        ideal = (int(np.sum(lens)) + total) * 4
        groups = (0, 16, 64) if name == "chord64" else (0,)
        for streamed in (True, False):
            for group in groups:
                score_bank.KS_GROUP = group
                # the outputs of the two paths at this size, on fresh graphs; the whole renders give the pool growth
                outs, growth = {}, {}
                for bank in (True, False):
                    score_bank.set_enabled(bank)
                    fresh = score(starts, lens, freqs, make)
                    if streamed:
                        outs[bank] = np.concatenate([fresh.render(s, min(BLOCK, total - s)).data
                                                     for s in range(0, total, BLOCK)])
                    else:
                        snip, growth[bank] = pool_growth(hip, lambda: fresh.render(0, total))
                        outs[bank] = snip.data
                    del fresh
                equal = bool(np.array_equal(outs[True], outs[False]))
                del outs
                # a graph per path: streamed through the generic path the inputs hold look-ahead windows of their own,
                # which the other path would have to settle first
                mixes = {True: score(starts, lens, freqs, make), False: score(starts, lens, freqs, make)}
                times = {True: [], False: []}
                stats = None
                for rep in range(4):                             # pass 0 warms both paths up
                    for bank in (True, False):
                        score_bank.set_enabled(bank)
                        before = dict(score_bank.STATS)
                        t = one_pass(mixes[bank], total, streamed)
                        if rep:
                            times[bank].append(t)
                        if bank:
                            stats = {key: score_bank.STATS[key] - before[key] for key in before}
                score_bank.set_enabled(True)
                med = {b: float(np.median(v)) for b, v in times.items()}
                blocks = -(-total // BLOCK) if streamed else 1
                rec = {
                    "row": name, "notes": len(starts), "mode": "blocks_1024" if streamed else "whole", "ks_group": group,
                    "audio_s": seconds, "equal": equal,
                    "bank_ms_per_audio_s": 1e3 * med[True] / seconds, "off_ms_per_audio_s": 1e3 * med[False] / seconds,
                    "bank_runs_ms": [1e3 * t for t in times[True]], "off_runs_ms": [1e3 * t for t in times[False]],
                    "ratio_bank_over_off": med[True] / med[False],
                    "bank_kernels_per_block": stats["launches"] / blocks, "bank_uploads_per_block": stats["uploads"] / blocks,
                    "off_launches_per_block": host_counts(starts, lens, total) if streamed else None,
                    "ideal_bytes": ideal,
                    "bank_pool_growth_bytes": growth.get(True), "off_pool_growth_bytes": growth.get(False),
                }
                records.append(rec)
                print(json.dumps(rec), flush=True)
    score_bank.KS_GROUP = 0
    with open(os.path.join(OUT, "score_probe.jsonl"), "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    write_md(records, os.path.join(OUT, "score_probe.md"))


def write_md(records, path):
    def spread(runs):
        return f"{min(runs):.1f}-{max(runs):.1f}"
    lines = ["# Score bank probe (tools/score_probe.py)", "",
             f"MI355X ({device.device_name()}), 48 kHz, median of 3 passes after a warm-up pass, bank on and off (a graph each) alternating in "
             "one process, every pass ended by a device synchronise.  `off` is PYGMU_SCORE_BANK=0: MixPE's generic path.  "
             "`runs` is the min-max of the three passes in ms: the spread a difference has to exceed.", "",
             "| row | mode | strings / workgroup | bank ms per s of audio | off ms per s of audio | bank / off | bank runs ms | "
             "off runs ms | bank kernels (+ uploads) per block | off launches per block | outputs equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        off_l = "" if r["off_launches_per_block"] is None else f"{r['off_launches_per_block']:.1f}"
        lines.append(f"| {r['row']} | {r['mode']} | {r['ks_group']} | {r['bank_ms_per_audio_s']:.3f} | "
                     f"{r['off_ms_per_audio_s']:.3f} | {r['ratio_bank_over_off']:.3f} | {spread(r['bank_runs_ms'])} | "
                     f"{spread(r['off_runs_ms'])} | {r['bank_kernels_per_block']:.2f} (+ {r['bank_uploads_per_block']:.2f}) | "
                     f"{off_l} | {r['equal']} |")
    lines += ["", "Whole renders: growth of the device pool over the render against (sum len_i + T) * 4 bytes.  hipMemGetInfo moves in "
              "the runtime's own granules and the runtime keeps freed blocks of its own: figures of a few tens of MB are indicative "
              "only (chord64's `off` figure read 0, 10 and 25 MB in three runs of the probe); the 1 000-note rows are far outside "
              "that.", "",
              "| row | (sum len + T) * 4 | bank pool growth | multiple | off pool growth | multiple |", "|---|---|---|---|---|---|"]
    for r in records:
        if r["mode"] == "whole" and r["ks_group"] == 0:
            b, o, i = r["bank_pool_growth_bytes"], r["off_pool_growth_bytes"], r["ideal_bytes"]
            lines.append(f"| {r['row']} | {i / 1e6:.1f} MB | {b / 1e6:.1f} MB | {b / i:.2f} | {o / 1e6:.1f} MB | {o / i:.2f} |")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
