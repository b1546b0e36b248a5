"""
Modulated-sine voice banks (voice_bank._SineModNode: the modulators as batched levels, then one pgx_sine_stateful_bank)
against the per-voice path (`mix._bank = False`: how every MixPE of FM voices was rendered before the bank took the class),
and the two plans of the entry against each other, at 48 kHz, look-ahead on, on two graphs:

    fm      MixPE of K x SinePE(frequency=TransformPE(SinePE(m_i), Affine(d_i, c_i)), amplitude=0.1)
    bell    MixPE of K x GainPE(<fm voice i>, gain=AdsrTriggeredPE(PeriodicTrigger(1 + 0.01 i), 0.005, 0.3, 0.2, 0.0, 0.1))
    c_i = 110 * 2^(i / 48), m_i = 1.5 c_i, d_i = m_i

K = 4, 8, 16, 64, 256, 512, streamed in blocks of 1 024 and of 48 000 frames.  The protocol of tools/pan_bank_probe.py: per
row a graph per path; a pass is one whole stream from a fresh start (renderer start, the pulls, a device synchronise, stop)
-- 248 blocks of 1 024 frames (a sum of look-ahead's windows 8 + 16 + ... + 128), 8 blocks of 48 000 --; a warm-up pass,
then three timed passes per path, the paths alternating in the same process; the median (min and max are kept: the spread)
as microseconds per block.  The first block of each bank path is compared with the per-voice path's on fresh graphs, bit
for bit.  Every (graph, block length) is a process of its own under its own time limit, and the first one that fails ends
the probe.

Paths: `walk` -- the bank with voice_bank.SINE_MOD_WALK_MIN_ROWS = 1 (no workspace: one workgroup per voice, one launch);
`parallel` -- the bank with the switch out of reach (a workspace: a workgroup per tile and voice, two launches; blocks of up
to two tiles are walked either way, so blocks of 1 024 frames have no such path); `off` -- `mix._bank = False`.  `bank` in
the report is the plan the switch's current value chooses for the row.

The result decides two constants of voice_bank.py.  SINE_MOD_WALK_MIN_ROWS: the smallest K from which the walk is not
slower than the two-launch form at that K and at every larger K measured.  SINE_MOD_MIN_VOICES: the smallest K from which
the bank is not slower than the per-voice path at that K and at every larger K measured, at both block lengths, on both
graphs.  A difference counts when it exceeds the spread of the passes (the fastest pass of the one is slower than the
slowest pass of the other).  The probe sets the measured minimums to voice_bank.MIN_VOICES, so that the smaller banks are
built at all.

    python tools/fm_bank_probe.py [--kind fm|bell]      appends to profiles/fm_bank_probe.jsonl and writes
                                                        profiles/fm_bank_probe.md
    python tools/fm_bank_probe.py --report              the table again from the records
    python tools/fm_bank_probe.py --step KIND BLOCK     one (graph, block length), its records on stdout
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 48_000
KINDS = ("fm", "bell")
VOICES = (4, 8, 16, 64, 256, 512)
BLOCKS = (1024, 48_000)
STREAM_BLOCKS = {1024: 248, 48_000: 8}
TILE = 2048                       # the entry's tile: blocks of up to two are walked whatever the workspace
WALK_ROWS = {"walk": 1, "parallel": 1 << 30}
STEP_SECONDS = 280
OUT = os.environ.get("FM_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def paths(block: int):
    return ("walk", "parallel", "off") if block > 2 * TILE else ("walk", "off")


def voice(pg, kind, i):
    from pygmu2_amd.transforms import Affine
    c = 110.0 * 2 ** (i / 48.0)
    m = 1.5 * c
    fm = pg.SinePE(frequency=pg.TransformPE(pg.SinePE(m), func=Affine(m, c)), amplitude=0.1)
    if kind == "fm":
        return fm
    if kind == "bell":
        return pg.GainPE(fm, gain=pg.AdsrTriggeredPE(pg.PeriodicTrigger(1.0 + 0.01 * i), 0.005, 0.3, 0.2, 0.0, 0.1))
    raise KeyError(kind)


def row(kind: str, k: int, block: int) -> dict:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    for name in ("SINE_MOD_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES"):
        setattr(voice_bank, name, voice_bank.MIN_VOICES)
    default_rows = voice_bank.SINE_MOD_WALK_MIN_ROWS
    names = paths(block)

    def mix(path):
        m = pg.MixPE(*[voice(pg, kind, i) for i in range(k)])
        if path == "off":
            m._bank = False
        return m

    def select(path):
        voice_bank.SINE_MOD_WALK_MIN_ROWS = WALK_ROWS.get(path, default_rows)

    def stream(path, m, blocks):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
        select(path)
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(m)
        r.start()
        device.synchronize()
        t0 = time.perf_counter()
        for b in range(blocks):
            m.render(b * block, block)
        device.synchronize()
        t = time.perf_counter() - t0
        r.stop()
        return t

    first = {}
    for path in names:
        m = mix(path)
        select(path)
        first[path] = np.array(m.render(0, block).data)
        assert bool(m._bank) == (path != "off")
        assert path == "off" or any(type(node) is voice_bank._SineModNode for node in m._bank._nodes())
        del m
    equal = {path: bool(np.array_equal(first[path].view(np.uint32), first["off"].view(np.uint32)))
             for path in names if path != "off"}
    del first

    graphs = [(path, mix(path)) for path in names]
    blocks = STREAM_BLOCKS[block]
    times = {path: [] for path in names}
    for rep in range(4):                                  # pass 0 warms the paths up
        for path, m in graphs:
            t = stream(path, m, blocks)
            if rep:
                times[path].append(1e6 * t / blocks)
    voice_bank.SINE_MOD_WALK_MIN_ROWS = default_rows
    rec = {"kind": kind, "voices": k, "block": block, "stream_blocks": blocks, "device": device.device_name()}
    for path in ("walk", "parallel", "off"):
        rec[f"{path}_us_per_block"] = float(np.median(times[path])) if path in times else None
        rec[f"{path}_runs_us"] = times.get(path)
        if path != "off":
            rec[f"{path}_equal"] = equal.get(path)
    return rec


def bank_plan(r) -> str:
    """The plan voice_bank's switch, as it stands, chooses for the row."""
    from pygmu2_amd import voice_bank
    return "walk" if r["parallel_runs_us"] is None or r["voices"] >= voice_bank.SINE_MOD_WALK_MIN_ROWS else "parallel"


def slower(r, a, b) -> bool:
    """Path a is slower than path b by more than the spread of the passes."""
    return r[f"{a}_us_per_block"] > r[f"{b}_us_per_block"] and min(r[f"{a}_runs_us"]) > max(r[f"{b}_runs_us"])


def smallest_from_which(records, lost):
    """The smallest K from which no row of K, nor of any larger K measured, is lost; None when the largest K loses."""
    best = None
    for k in sorted({r["voices"] for r in records}, reverse=True):
        if any(lost(r) for r in records if r["voices"] == k):
            break
        best = k
    return best


def winning_minimum(records):
    return smallest_from_which(records, lambda r: slower(r, bank_plan(r), "off"))


def walk_minimum(records):
    return smallest_from_which([r for r in records if r["parallel_runs_us"] is not None],
                               lambda r: slower(r, "walk", "parallel"))


def write_md(records, path):
    from pygmu2_amd import voice_bank

    def spread(runs):
        return "-" if runs is None else f"{min(runs):.1f}-{max(runs):.1f}"

    def us(v):
        return "-" if v is None else f"{v:.1f}"

    name = records[0]["device"].strip() if records else "?"
    lines = ["# Modulated-sine voice bank probe (tools/fm_bank_probe.py)", "",
             f"MI355X, {name}, 48 kHz, look-ahead on.  `fm`: MixPE of K SinePE(frequency=TransformPE(SinePE(m_i), Affine(d_i, "
             "c_i))); `bell`: the same under GainPE(..., gain=AdsrTriggeredPE(PeriodicTrigger)).  A pass is one whole stream from "
             "a fresh start (start, the pulls, a device synchronise, stop); median of 3 passes after a warm-up pass, the paths (a "
             "graph each) alternating in one process; us per block = pass / blocks.  `walk`: the bank, "
             "SINE_MOD_WALK_MIN_ROWS = 1 -- no workspace, one workgroup per voice, one launch.  `parallel`: the bank with the "
             "switch out of reach -- a workgroup per tile of 2 048 frames and voice, two launches (blocks of up to two tiles are "
             "walked either way: no such path at 1 024 frames).  `off` is `mix._bank = False`: the voices rendered one by one -- "
             "the code of the commit before the bank --, which look_ahead.py streams in windows of 8, 16 ... blocks where the "
             "blocks are small.  `bank` is the plan SINE_MOD_WALK_MIN_ROWS = "
             f"{voice_bank.SINE_MOD_WALK_MIN_ROWS} chooses for the row.  `runs` is the min-max of the three passes: the spread a "
             "difference has to exceed.", ""]
    for kind in KINDS:
        rows = [r for r in records if r["kind"] == kind]
        if not rows:
            continue
        lines += [f"## `{kind}`", "",
                  "| voices | block | blocks per stream | walk us per block | parallel us per block | off us per block | bank | "
                  "bank / off | walk / parallel | walk runs | parallel runs | off runs | first block: walk = off | parallel = off |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            plan = bank_plan(r)
            ratio = "-" if r["parallel_us_per_block"] is None else f"{r['walk_us_per_block'] / r['parallel_us_per_block']:.3f}"
            lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {us(r['walk_us_per_block'])} | "
                         f"{us(r['parallel_us_per_block'])} | {us(r['off_us_per_block'])} | {plan} | "
                         f"{r[plan + '_us_per_block'] / r['off_us_per_block']:.3f} | {ratio} | {spread(r['walk_runs_us'])} | "
                         f"{spread(r['parallel_runs_us'])} | {spread(r['off_runs_us'])} | {r['walk_equal']} | "
                         f"{'-' if r['parallel_equal'] is None else r['parallel_equal']} |")
        lines += ["", "Smallest K from which the bank is not slower than the per-voice path (beyond the spread) at that K and at "
                  f"every larger K measured, both block lengths: {winning_minimum(rows)}.",
                  "Smallest K from which the walk is not slower than the two-launch form (beyond the spread) at that K and at "
                  f"every larger K measured: {walk_minimum(rows)}.", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines).rstrip("\n") + "\n")


def read_records(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def main():
    if "--step" in sys.argv:
        at = sys.argv.index("--step")
        for k in VOICES:
            print(json.dumps(row(sys.argv[at + 1], k, int(sys.argv[at + 2]))), flush=True)
        return 0
    os.makedirs(OUT, exist_ok=True)
    jsonl, md = os.path.join(OUT, "fm_bank_probe.jsonl"), os.path.join(OUT, "fm_bank_probe.md")
    kinds = (sys.argv[sys.argv.index("--kind") + 1],) if "--kind" in sys.argv else KINDS
    records = [r for r in read_records(jsonl) if "--report" in sys.argv or r["kind"] not in kinds]
    status = 0
    for kind in () if "--report" in sys.argv else kinds:
        for block in BLOCKS:
            # a process and a time limit per (graph, block length); one that fails or overruns ends the probe
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(block)],
                                      stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
            except subprocess.TimeoutExpired:
                print(f"step {kind} block={block}: over {STEP_SECONDS} s", flush=True)
                status = 124
                break
            if done.returncode != 0:
                print(f"step {kind} block={block}: exit {done.returncode}", flush=True)
                status = done.returncode
                break
            for line in done.stdout.strip().splitlines():
                if line.startswith("{"):
                    records.append(json.loads(line))
                    print(line, flush=True)
        if status:
            break
    records.sort(key=lambda r: (KINDS.index(r["kind"]), r["block"], r["voices"]))
    with open(jsonl, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    if records:
        write_md(records, md)
    return status


if __name__ == "__main__":
    sys.exit(main())
