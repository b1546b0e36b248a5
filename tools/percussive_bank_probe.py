"""
Percussive voice banks (voice_bank._SvfNode: pgx_svf_bank; _TriggerNode / _AdsrTriggeredNode: pgx_periodic_trigger_bank,
pgx_adsr_triggered with batch = K) against the per-voice path (`mix._bank = False`: how every such MixPE was rendered
before the bank took SVFilterPE and AdsrTriggeredPE), at 48 kHz, look-ahead on, on two graphs:

    svf   MixPE of K x SVFilterPE(BlitSawPE(f_i), 1200, 2.0)
    trig  MixPE of K x GainPE(BiquadPE(BlitSawPE(f_i), 2000, 0.707),
                              gain=AdsrTriggeredPE(PeriodicTrigger(2 + 0.01 i), .005, .04, .05, .6, .08))

(`trig` over the constant BiquadPE, which is banked from MIN_VOICES voices on already: what differs between the two paths
of that graph below the new minimum is the envelope alone.)

K = 4, 8, 16, 32, 64, 256, streamed in blocks of 512, 4 096 and 48 000 frames.  Per step: a graph per path; a pass is one
whole stream from a fresh start (renderer start, the pulls, a device synchronise, stop) -- STREAM_BLOCKS pulls, a sum of
look-ahead's windows 8 + 16 + ... + 128 + 256 + 256 ..., so that the per-voice path ends with a window it has used up; a
warm-up pass, then three timed passes per path, alternating in the same process; the median (min and max are kept: the
spread) as microseconds per block.  Paths of `svf`: the bank with the segmented plan (a workspace: the reduce and the
apply launch, as the PE itself), the bank with the walk (no workspace: one workgroup per row, one launch), the per-voice
path.  Paths of `trig`: the bank, the per-voice path.  The first block of each bank path is compared with the per-voice
path's on fresh graphs.  Every step is a process of its own under its own time limit, and the first step that fails ends
the probe.

The result decides three constants of voice_bank.py: SVF_MIN_VOICES and ADSR_TRIGGERED_MIN_VOICES, each the smallest K
from which the bank is faster at that K and at every larger K measured, at every block length; and SVF_WALK_MIN_ROWS,
the smallest number of rows (K: the voices are mono) from which the walk is not slower than the segmented plan in any
row of that K or a larger one.  The probe itself sets the minimums to voice_bank.MIN_VOICES, so that the smaller banks
are built at all, and the walk per path.

    python tools/percussive_bank_probe.py [--kind svf|trig]      appends to profiles/percussive_bank_probe.jsonl and
                                                                 writes profiles/percussive_bank_probe.md
    python tools/percussive_bank_probe.py --report               the table again from the records
    python tools/percussive_bank_probe.py --step KIND K BLOCK    one step, its record on stdout
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
KINDS = ("svf", "trig")
VOICES = (4, 8, 16, 32, 64, 256)
BLOCKS = (512, 4096, 48_000)
STREAM_BLOCKS = {512: 2040, 4096: 2040, 48_000: 248}      # 8 + 16 + 32 + 64 + 128 (+ 7 x 256): every pass ends with a window
STEP_SECONDS = 240
NEVER = 1 << 40
OUT = os.environ.get("PERCUSSIVE_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def voice(pg, kind, i):
    saw = pg.BlitSawPE(109.37 * 2 ** ((i % 72) / 12))
    if kind == "svf":
        return pg.SVFilterPE(saw, 1200.0, 2.0)
    envelope = pg.AdsrTriggeredPE(pg.PeriodicTrigger(2.0 + 0.01 * i), 0.005, 0.04, 0.05, 0.6, 0.08)
    return pg.GainPE(pg.BiquadPE(saw, frequency=2000.0, q=0.707), gain=envelope)


def step(kind: str, k: int, block: int) -> dict:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    voice_bank.SVF_MIN_VOICES = voice_bank.ADSR_TRIGGERED_MIN_VOICES = voice_bank.MIN_VOICES      # banks below them too
    paths = (("bank", True, NEVER), ("off", False, NEVER)) + ((("walk", True, 1),) if kind == "svf" else ())

    def mix(bank):
        m = pg.MixPE(*[voice(pg, kind, i) for i in range(k)])
        if not bank:
            m._bank = False
        return m

    def stream(m, blocks, walk_rows):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
        voice_bank.SVF_WALK_MIN_ROWS = walk_rows
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
    for name, bank, walk_rows in paths:
        voice_bank.SVF_WALK_MIN_ROWS = walk_rows
        m = mix(bank)
        first[name] = np.array(m.render(0, block).data)
        assert bool(m._bank) == bank
        del m
    peak = float(np.max(np.abs(first["off"])))
    err = {name: float(np.max(np.abs(first[name].astype(np.float64) - first["off"]))) / peak for name in first}
    equal = bool(np.array_equal(first["bank"], first["off"]))
    del first

    graphs = [(name, mix(bank), walk_rows) for name, bank, walk_rows in paths]
    blocks = STREAM_BLOCKS[block]
    times = {name: [] for name, _, _ in graphs}
    for rep in range(4):                                  # pass 0 warms every path up
        for name, m, walk_rows in graphs:
            t = stream(m, blocks, walk_rows)
            if rep:
                times[name].append(1e6 * t / blocks)
    med = {name: float(np.median(v)) for name, v in times.items()}
    rec = {"kind": kind, "voices": k, "block": block, "stream_blocks": blocks, "device": device.device_name(),
           "equal": equal, "bank_err_over_peak": err["bank"],
           "bank_us_per_block": med["bank"], "off_us_per_block": med["off"], "bank_over_off": med["bank"] / med["off"],
           "bank_runs_us": times["bank"], "off_runs_us": times["off"]}
    if kind == "svf":
        rec.update({"walk_us_per_block": med["walk"], "walk_over_bank": med["walk"] / med["bank"],
                    "walk_runs_us": times["walk"], "walk_err_over_peak": err["walk"]})
    return rec


def winning_minimum(records, column="bank_us_per_block", against="off_us_per_block", strict=True):
    """The smallest K from which `column` beats `against` (strict: is faster; else: is not slower) in every row of K and
    of every larger K measured, or None."""
    best = None
    for k in sorted({r["voices"] for r in records}, reverse=True):
        rows = [r for r in records if r["voices"] == k]
        if all(r[column] < r[against] if strict else r[column] <= r[against] for r in rows):
            best = k
        else:
            break
    return best


def write_md(records, path):
    def spread(runs):
        return f"{min(runs):.1f}-{max(runs):.1f}"
    name = records[0]["device"] if records else "?"
    lines = ["# Percussive voice bank probe (tools/percussive_bank_probe.py)", "",
             f"MI355X ({name}), 48 kHz, look-ahead on.  `svf`: MixPE of K SVFilterPE(BlitSawPE(f), 1200, 2) voices; `trig`: MixPE "
             "of K GainPE(BiquadPE(BlitSawPE(f), 2000, 0.707), gain=AdsrTriggeredPE(PeriodicTrigger)) voices.  A pass is one "
             "whole stream from a fresh start (start, the pulls, a device synchronise, stop); median of 3 passes after a warm-up "
             "pass, the paths (a graph each) alternating in one process; us per block = pass / blocks.  `off` is `mix._bank = "
             "False`: the voices rendered one by one, which look_ahead.py streams in windows of 8, 16 ... 256 blocks.  `bank` "
             "is the bank (for `svf`: with the segmented plan, a workspace), `walk` the SVF bank with one workgroup per row (no "
             "workspace).  `runs` is the min-max of the three passes: the spread a difference has to exceed.", ""]
    for kind in KINDS:
        rows = [r for r in records if r["kind"] == kind]
        if not rows:
            continue
        lines += [f"## `{kind}`: the bank against the per-voice path", "",
                  "| voices | block | blocks per stream | bank us per block | off us per block | bank / off | bank runs | off runs | "
                  "first block equal | first block: max err / peak |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['bank_us_per_block']:.1f} | "
                         f"{r['off_us_per_block']:.1f} | {r['bank_over_off']:.3f} | {spread(r['bank_runs_us'])} | "
                         f"{spread(r['off_runs_us'])} | {r['equal']} | {r['bank_err_over_peak']:.2e} |")
        lines += ["", "Smallest K from which the bank is faster at that K and at every larger K measured, every row: "
                  f"{winning_minimum(rows)}.", ""]
        if kind != "svf":
            continue
        lines += ["## `svf`: the walk (no workspace) against the segmented plan", "",
                  "| voices (= rows) | block | blocks per stream | walk us per block | segmented us per block | walk / segmented | "
                  "walk runs | segmented runs | first block: max err / peak against off |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['walk_us_per_block']:.1f} | "
                         f"{r['bank_us_per_block']:.1f} | {r['walk_over_bank']:.3f} | {spread(r['walk_runs_us'])} | "
                         f"{spread(r['bank_runs_us'])} | {r['walk_err_over_peak']:.2e} |")
        lines += ["", "(Blocks of up to two tiles of 1024 frames are walked either way: the 512-frame rows measure one kernel "
                  "twice.)  Smallest number of rows from which the walk is not slower at that K and at every larger K measured, "
                  f"every row: {winning_minimum(rows, 'walk_us_per_block', 'bank_us_per_block', strict=False)}.", ""]
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
        print(json.dumps(step(sys.argv[at + 1], int(sys.argv[at + 2]), int(sys.argv[at + 3]))), flush=True)
        return 0
    os.makedirs(OUT, exist_ok=True)
    jsonl, md = os.path.join(OUT, "percussive_bank_probe.jsonl"), os.path.join(OUT, "percussive_bank_probe.md")
    kinds = (sys.argv[sys.argv.index("--kind") + 1],) if "--kind" in sys.argv else KINDS
    records = [r for r in read_records(jsonl) if "--report" in sys.argv or r["kind"] not in kinds]
    status = 0
    for kind in () if "--report" in sys.argv else kinds:
        for block in BLOCKS:
            for k in VOICES:
                # a process and a time limit per step; a step that fails or overruns ends the probe
                try:
                    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(k), str(block)],
                                          stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
                except subprocess.TimeoutExpired:
                    print(f"step {kind} K={k} block={block}: over {STEP_SECONDS} s", flush=True)
                    status = 124
                    break
                if done.returncode != 0:
                    print(f"step {kind} K={k} block={block}: exit {done.returncode}", flush=True)
                    status = done.returncode
                    break
                line = done.stdout.strip().splitlines()[-1]
                records.append(json.loads(line))
                print(line, flush=True)
            if status:
                break
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
