"""
Swept-filter voice bank (voice_bank._BiquadVarNode: pgx_biquad_varying_bank) against the per-voice path
(`mix._bank = False`: how every such MixPE was rendered before the bank took BiquadPEs with PE parameters), at 48 kHz,
on the ordinary subtractive voice -- a sawtooth into a low-pass whose cutoff follows an envelope, under an envelope:

    MixPE of K x GainPE(BiquadPE(BlitSawPE(f_i), frequency=TransformPE(AdsrGatedPE(PeriodicGate(g_i, 0.5), .01, .1, .7, .2),
                                                                       Affine(2500, 300)), q=2.0),
                        gain=AdsrGatedPE(PeriodicGate(g_i, 0.5), .01, .1, .7, .2))

K = 4, 8, 16, 64, 256, 512, streamed in blocks of 4 096 and of 48 000 frames.  Per step: a graph per path; a pass is one
whole stream from a fresh start (renderer start, the pulls, a device synchronise, stop) -- a short stream of 8 blocks
and a long one of 248 (STREAMS), because the per-voice path renders a stream in look-ahead windows of 8, 16 ... blocks;
a warm-up pass, then three timed passes per path, alternating in the same process; the median (min and max are kept:
the spread) as microseconds per block.  Three paths: the bank with the segmented plan (a workspace: the reduce and the
apply launch, as the PE itself), the bank with the walk (no workspace: one workgroup per row, one launch), and the
per-voice path.  The first block of each bank path is compared with the per-voice path's on fresh graphs.  Every step
is a process of its own under its own time limit, and the first step that fails ends the probe.

The result decides two constants of voice_bank.py: BIQUAD_VAR_MIN_VOICES, the smallest K from which the bank (whichever
plan the constants give it) is faster at that K and at every larger K measured, at both block lengths and both stream
lengths; and BIQUAD_VAR_WALK_MIN_ROWS, the smallest number of rows (K: the voices are mono) from which the walk is not
slower than the segmented plan at both block lengths, at that K and every larger one.  The probe itself sets the first
to voice_bank.MIN_VOICES, so that the smaller banks are built at all, and the second per path.

    python tools/swept_bank_probe.py            writes profiles/swept_bank_probe.jsonl and profiles/swept_bank_probe.md
    python tools/swept_bank_probe.py --step K BLOCK      one step, its records on stdout
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
VOICES = (4, 8, 16, 64, 256, 512)
BLOCKS = (4096, 48_000)
STREAMS = (8, 248)             # blocks per stream: look-ahead's first window, and 8 + 16 + 32 + 64 + 128 (ends with a window)
STEP_SECONDS = 240
NEVER = 1 << 40
OUT = os.environ.get("SWEPT_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def voice(pg, i):
    def envelope():
        return pg.AdsrGatedPE(pg.PeriodicGate(2.0 + 0.01 * i, 0.5), 0.01, 0.1, 0.7, 0.2)
    cutoff = pg.TransformPE(envelope(), func=pg.transforms.Affine(2500.0, 300.0))
    saw = pg.BlitSawPE(109.37 * 2 ** ((i % 72) / 12))
    return pg.GainPE(pg.BiquadPE(saw, frequency=cutoff, q=2.0), gain=envelope())


def step(k: int, block: int) -> list:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    voice_bank.BIQUAD_VAR_MIN_VOICES = voice_bank.MIN_VOICES      # what is being measured: banks below it too

    def mix(bank):
        m = pg.MixPE(*[voice(pg, i) for i in range(k)])
        if not bank:
            m._bank = False
        return m

    def stream(m, blocks, walk_rows):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
        voice_bank.BIQUAD_VAR_WALK_MIN_ROWS = walk_rows
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
    for name, bank, walk_rows in (("bank", True, NEVER), ("walk", True, 1), ("off", False, NEVER)):
        voice_bank.BIQUAD_VAR_WALK_MIN_ROWS = walk_rows
        m = mix(bank)
        first[name] = np.array(m.render(0, block).data)
        assert bool(m._bank) == bank
        del m
    peak = float(np.max(np.abs(first["off"])))
    equal = bool(np.array_equal(first["bank"], first["off"]))
    walk_err = float(np.max(np.abs(first["walk"].astype(np.float64) - first["off"]))) / peak
    del first

    modes = (("bank", mix(True), NEVER), ("off", mix(False), NEVER), ("walk", mix(True), 1))
    records = []
    for blocks in STREAMS:
        times = {name: [] for name, _, _ in modes}
        for rep in range(4):                              # pass 0 warms every path up
            for name, m, walk_rows in modes:
                t = stream(m, blocks, walk_rows)
                if rep:
                    times[name].append(1e6 * t / blocks)
        med = {name: float(np.median(v)) for name, v in times.items()}
        records.append({"voices": k, "block": block, "stream_blocks": blocks, "equal": equal, "walk_err_over_peak": walk_err,
                        "device": device.device_name(), "bank_us_per_block": med["bank"],
                        "walk_us_per_block": med["walk"], "off_us_per_block": med["off"],
                        "bank_over_off": med["bank"] / med["off"], "walk_over_bank": med["walk"] / med["bank"],
                        "bank_runs_us": times["bank"], "walk_runs_us": times["walk"], "off_runs_us": times["off"]})
    return records


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
    lines = ["# Swept-filter voice bank probe (tools/swept_bank_probe.py)", "",
             f"MI355X ({name}), 48 kHz, MixPE of K GainPE(BiquadPE(BlitSawPE(f), frequency=TransformPE(AdsrGatedPE(PeriodicGate)), "
             "q=2), gain=AdsrGatedPE(PeriodicGate)) voices.  A pass is one whole stream from a fresh start (start, the pulls, a "
             "device synchronise, stop); median of 3 passes after a warm-up pass, the paths (a graph each) alternating in one "
             "process; us per block = pass / blocks.  `off` is `mix._bank = False`: the voices rendered one by one, which "
             "look_ahead.py streams in windows of 8, 16 ... blocks.  `bank` is the bank with the segmented plan (a workspace), "
             "`walk` the bank with one workgroup per row (no workspace).  `runs` is the min-max of the three passes: the "
             "spread a difference has to exceed.", "",
             "## Bank (segmented plan) against the per-voice path", "",
             "| voices | block | blocks per stream | bank us per block | off us per block | bank / off | bank runs | off runs | "
             "first block equal |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['bank_us_per_block']:.1f} | "
                     f"{r['off_us_per_block']:.1f} | {r['bank_over_off']:.3f} | {spread(r['bank_runs_us'])} | "
                     f"{spread(r['off_runs_us'])} | {r['equal']} |")
    lines += ["", "Smallest K from which the bank is faster at that K and at every larger K measured, every row: "
              f"{winning_minimum(records)}.", "",
              "## The walk (no workspace) against the segmented plan", "",
              "| voices (= rows) | block | blocks per stream | walk us per block | segmented us per block | walk / segmented | "
              "walk runs | segmented runs | first block: max err / peak against off |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['walk_us_per_block']:.1f} | "
                     f"{r['bank_us_per_block']:.1f} | {r['walk_over_bank']:.3f} | {spread(r['walk_runs_us'])} | "
                     f"{spread(r['bank_runs_us'])} | {r['walk_err_over_peak']:.2e} |")
    lines += ["", "Smallest number of rows from which the walk is not slower at that K and at every larger K measured, every "
              f"row: {winning_minimum(records, 'walk_us_per_block', 'bank_us_per_block', strict=False)}."]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if "--step" in sys.argv:
        at = sys.argv.index("--step")
        for rec in step(int(sys.argv[at + 1]), int(sys.argv[at + 2])):
            print(json.dumps(rec), flush=True)
        return 0
    os.makedirs(OUT, exist_ok=True)
    records = []
    status = 0
    for block in BLOCKS:
        for k in VOICES:
            # a process and a time limit per step; a step that fails or overruns ends the probe
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(k), str(block)],
                                      stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
            except subprocess.TimeoutExpired:
                print(f"step K={k} block={block}: over {STEP_SECONDS} s", flush=True)
                status = 124
                break
            if done.returncode != 0:
                print(f"step K={k} block={block}: exit {done.returncode}", flush=True)
                status = done.returncode
                break
            for line in done.stdout.strip().splitlines()[-len(STREAMS):]:
                records.append(json.loads(line))
                print(line, flush=True)
        if status:
            break
    with open(os.path.join(OUT, "swept_bank_probe.jsonl"), "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    if records:
        write_md(records, os.path.join(OUT, "swept_bank_probe.md"))
    return status


if __name__ == "__main__":
    sys.exit(main())
