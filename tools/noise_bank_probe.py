"""
Noise voice banks (voice_bank._NoiseNode: pgx_noise_white / pgx_noise_pink / pgx_noise_brown with batch = K) against the
per-voice path (`mix._bank = False`: how every MixPE of NoisePEs was rendered before the bank took the class), at 48 kHz,
look-ahead on, on four graphs:

    white, pink, brown   MixPE of K x NoisePE(seed=i, mode=...)
    hihat                MixPE of K x GainPE(SVFilterPE(NoisePE(seed=i), f_i, 2.0, HIGHPASS),
                                             gain=AdsrTriggeredPE(PeriodicTrigger(4 + 0.01 i), .001, .02, .03, .3, .05))

K = 4, 8, 16, 64, 256, 512, streamed in blocks of 1 024 and of 48 000 frames.  Per row: a graph per path; a pass is one
whole stream from a fresh start (renderer start, the pulls, a device synchronise, stop) -- STREAM_BLOCKS pulls: 248 blocks
of 1 024 frames, a sum of look-ahead's windows 8 + 16 + ... + 128, so that the per-voice path ends with a window it has
used up; 8 blocks of 48 000 frames (a pink launch lasts 17 ns per frame whatever else runs: 512 voices one by one are
0.4 s per block) --; a warm-up pass, then three timed passes per path, alternating in the same process; the median (min
and max are kept: the spread) as microseconds per block.  The first block of the bank is compared with the per-voice
path's on fresh graphs.  Every (graph, block length) is a process of its own under its own time limit, and the first
one that fails ends the probe.

The result decides voice_bank.NOISE_MIN_VOICES: for the slowest mode, the smallest K from which the bank is not slower at
that K and at every larger K measured, at both block lengths (and at least MIN_VOICES).  The probe itself sets the
minimums to voice_bank.MIN_VOICES, so that the smaller banks are built at all.

    python tools/noise_bank_probe.py [--kind white|pink|brown|hihat]   appends to profiles/noise_bank_probe.jsonl and
                                                                       writes profiles/noise_bank_probe.md
    python tools/noise_bank_probe.py --report                          the table again from the records
    python tools/noise_bank_probe.py --step KIND BLOCK                 one (graph, block length), its records on stdout
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
KINDS = ("white", "pink", "brown", "hihat")
VOICES = (4, 8, 16, 64, 256, 512)
BLOCKS = (1024, 48_000)
STREAM_BLOCKS = {1024: 248, 48_000: 8}
STEP_SECONDS = 280
OUT = os.environ.get("NOISE_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def voice(pg, kind, i):
    if kind != "hihat":
        return pg.NoisePE(seed=i, mode=pg.NoiseMode(kind))
    envelope = pg.AdsrTriggeredPE(pg.PeriodicTrigger(4.0 + 0.01 * i), 0.001, 0.02, 0.03, 0.3, 0.05)
    return pg.GainPE(pg.SVFilterPE(pg.NoisePE(seed=i), 6000.0 + 10.0 * (i % 200), 2.0, pg.BiquadMode.HIGHPASS), gain=envelope)


def row(kind: str, k: int, block: int) -> dict:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    for name in ("NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES"):      # banks below them too
        setattr(voice_bank, name, voice_bank.MIN_VOICES)

    def mix(bank):
        m = pg.MixPE(*[voice(pg, kind, i) for i in range(k)])
        if not bank:
            m._bank = False
        return m

    def stream(m, blocks):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
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
    for name, bank in (("bank", True), ("off", False)):
        m = mix(bank)
        first[name] = np.array(m.render(0, block).data)
        assert bool(m._bank) == bank
        del m
    peak = float(np.max(np.abs(first["off"])))
    err = float(np.max(np.abs(first["bank"].astype(np.float64) - first["off"]))) / peak
    equal = bool(np.array_equal(first["bank"], first["off"]))
    del first

    graphs = [("bank", mix(True)), ("off", mix(False))]
    blocks = STREAM_BLOCKS[block]
    times = {name: [] for name, _ in graphs}
    for rep in range(4):                                  # pass 0 warms both paths up
        for name, m in graphs:
            t = stream(m, blocks)
            if rep:
                times[name].append(1e6 * t / blocks)
    med = {name: float(np.median(v)) for name, v in times.items()}
    return {"kind": kind, "voices": k, "block": block, "stream_blocks": blocks, "device": device.device_name(),
            "equal": equal, "bank_err_over_peak": err,
            "bank_us_per_block": med["bank"], "off_us_per_block": med["off"], "bank_over_off": med["bank"] / med["off"],
            "bank_runs_us": times["bank"], "off_runs_us": times["off"]}


def winning_minimum(records):
    """The smallest K from which the bank is not slower than the per-voice path in every row of K and of every larger K
    measured, or None."""
    best = None
    for k in sorted({r["voices"] for r in records}, reverse=True):
        if all(r["bank_us_per_block"] <= r["off_us_per_block"] for r in records if r["voices"] == k):
            best = k
        else:
            break
    return best


def write_md(records, path):
    def spread(runs):
        return f"{min(runs):.1f}-{max(runs):.1f}"
    name = records[0]["device"].strip() if records else "?"      # (the runtime may report no marketing name: the arch then)
    lines = ["# Noise voice bank probe (tools/noise_bank_probe.py)", "",
             f"MI355X, {name}, 48 kHz, look-ahead on.  `white` / `pink` / `brown`: MixPE of K NoisePE(seed=i) voices of that "
             "mode; `hihat`: MixPE of K GainPE(SVFilterPE(NoisePE(seed=i), f_i, 2, hp), gain=AdsrTriggeredPE(PeriodicTrigger)) "
             "voices.  A pass is one whole stream from a fresh start (start, the pulls, a device synchronise, stop); median of 3 "
             "passes after a warm-up pass, the two paths (a graph each) alternating in one process; us per block = pass / "
             "blocks.  `off` is `mix._bank = False`: the voices rendered one by one -- the code of the commit before the bank --, "
             "which look_ahead.py streams in windows of 8, 16 ... blocks where the blocks are small.  `runs` is the min-max "
             "of the three passes: the spread a difference has to exceed.", ""]
    minimums = {}
    for kind in KINDS:
        rows = [r for r in records if r["kind"] == kind]
        if not rows:
            continue
        lines += [f"## `{kind}`", "",
                  "| voices | block | blocks per stream | bank us per block | off us per block | bank / off | bank runs | off runs | "
                  "first block equal | first block: max err / peak |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['bank_us_per_block']:.1f} | "
                         f"{r['off_us_per_block']:.1f} | {r['bank_over_off']:.3f} | {spread(r['bank_runs_us'])} | "
                         f"{spread(r['off_runs_us'])} | {r['equal']} | {r['bank_err_over_peak']:.2e} |")
        minimums[kind] = winning_minimum(rows)
        lines += ["", "Smallest K from which the bank is not slower at that K and at every larger K measured, both block "
                  f"lengths: {minimums[kind]}.", ""]
    modes = [minimums.get(kind) for kind in ("white", "pink", "brown") if kind in minimums]
    if modes:
        worst = "none measured" if any(m is None for m in modes) else str(max(modes))
        lines += ["## The minimum", "", f"Largest of the three modes' minimums (the slowest mode decides): {worst}.", ""]
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
    jsonl, md = os.path.join(OUT, "noise_bank_probe.jsonl"), os.path.join(OUT, "noise_bank_probe.md")
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
