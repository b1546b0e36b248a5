"""
Panned voice banks (voice_bank._PanNode: pgx_pan_gains once, pgx_pan_mix_batch per block) against the per-voice path
(`mix._bank = False`: how every MixPE of SpatialPE voices was rendered before the bank took the class) and against the
bank with the fused root switched off (voice_bank.FUSED_PAN_MIX = False: pgx_pan_bank + pgx_mix_batch -- what
pgx_pan_mix_batch buys), at 48 kHz, look-ahead on, on three graphs:

    sine      MixPE of K x SpatialPE(SinePE(220 + 3 i, 0.1), SpatialConstantPower(azimuth=a_i))
    readme    MixPE of K x SpatialPE(<README.md's voice i>, SpatialConstantPower(azimuth=a_i))
    autopan   MixPE of K x SpatialPE(BiquadPE(BlitSawPE(f_i), 2000, 0.707),
                                     SpatialLinear(azimuth=SinePE(0.2 + 0.01 i, amplitude=60)))
    a_i = -90 + 180 i / (K - 1)

K = 4, 8, 16, 64, 256, 512, streamed in blocks of 1 024 and of 48 000 frames.  The protocol of tools/noise_bank_probe.py:
per row a graph per path; a pass is one whole stream from a fresh start (renderer start, the pulls, a device
synchronise, stop) -- 248 blocks of 1 024 frames (a sum of look-ahead's windows 8 + 16 + ... + 128), 8 blocks of 48 000
--; a warm-up pass, then three timed passes per path, the paths alternating in the same process; the median (min and max
are kept: the spread) as microseconds per block.  The first block of the bank is compared with the per-voice path's on
fresh graphs, bit for bit.  Every (graph, block length) is a process of its own under its own time limit, and the first
one that fails ends the probe.

The result decides whether voice_bank needs a PAN_MIN_VOICES: per graph, the smallest K from which the bank is not slower
at that K and at every larger K measured, at both block lengths; a difference counts when it exceeds the spread of the
passes (the bank's fastest pass is slower than the per-voice path's slowest).  The probe sets the other measured minimums
to voice_bank.MIN_VOICES, so that the smaller banks are built at all.

    python tools/pan_bank_probe.py [--kind sine|readme|autopan]   appends to profiles/pan_bank_probe.jsonl and writes
                                                                  profiles/pan_bank_probe.md
    python tools/pan_bank_probe.py --report                       the table again from the records
    python tools/pan_bank_probe.py --step KIND BLOCK              one (graph, block length), its records on stdout
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
KINDS = ("sine", "readme", "autopan")
VOICES = (4, 8, 16, 64, 256, 512)
BLOCKS = (1024, 48_000)
STREAM_BLOCKS = {1024: 248, 48_000: 8}
PATHS = ("bank", "layered", "off")
STEP_SECONDS = 280
OUT = os.environ.get("PAN_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def voice(pg, kind, i, k):
    from pygmu2_amd.sharding import c5_voice
    azimuth = -90.0 + 180.0 * i / (k - 1)
    if kind == "sine":
        return pg.SpatialPE(pg.SinePE(220.0 + 3.0 * i, amplitude=0.1), method=pg.SpatialConstantPower(azimuth=azimuth))
    if kind == "readme":
        return pg.SpatialPE(c5_voice(pg, i), method=pg.SpatialConstantPower(azimuth=azimuth))
    if kind == "autopan":
        return pg.SpatialPE(pg.BiquadPE(pg.BlitSawPE(27.5 * 2 ** (i / 48.0)), frequency=2000.0, q=0.707),
                            method=pg.SpatialLinear(azimuth=pg.SinePE(0.2 + 0.01 * i, amplitude=60.0)))
    raise KeyError(kind)


def row(kind: str, k: int, block: int) -> dict:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    for name in ("NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES", "BIQUAD_VAR_MIN_VOICES"):
        setattr(voice_bank, name, voice_bank.MIN_VOICES)

    def mix(path):
        m = pg.MixPE(*[voice(pg, kind, i, k) for i in range(k)])
        if path == "off":
            m._bank = False
        return m

    def stream(path, m, blocks):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
        voice_bank.FUSED_PAN_MIX = path != "layered"
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
        voice_bank.FUSED_PAN_MIX = True
        return t

    first = {}
    for path in PATHS:
        m = mix(path)
        voice_bank.FUSED_PAN_MIX = path != "layered"
        first[path] = np.array(m.render(0, block).data)
        voice_bank.FUSED_PAN_MIX = True
        assert bool(m._bank) == (path != "off")
        assert path == "off" or type(m._bank.root) is voice_bank._PanNode
        del m
    peak = float(np.max(np.abs(first["off"])))
    err = float(np.max(np.abs(first["bank"].astype(np.float64) - first["off"]))) / peak
    equal = bool(np.array_equal(first["bank"].view(np.uint32), first["off"].view(np.uint32)))
    layered_equal = bool(np.array_equal(first["bank"].view(np.uint32), first["layered"].view(np.uint32)))
    del first

    graphs = [(path, mix(path)) for path in PATHS]
    blocks = STREAM_BLOCKS[block]
    times = {path: [] for path in PATHS}
    for rep in range(4):                                  # pass 0 warms the paths up
        for path, m in graphs:
            t = stream(path, m, blocks)
            if rep:
                times[path].append(1e6 * t / blocks)
    med = {path: float(np.median(v)) for path, v in times.items()}
    return {"kind": kind, "voices": k, "block": block, "stream_blocks": blocks, "device": device.device_name(),
            "equal": equal, "layered_equal": layered_equal, "bank_err_over_peak": err,
            "bank_us_per_block": med["bank"], "layered_us_per_block": med["layered"], "off_us_per_block": med["off"],
            "bank_over_off": med["bank"] / med["off"], "bank_over_layered": med["bank"] / med["layered"],
            "bank_runs_us": times["bank"], "layered_runs_us": times["layered"], "off_runs_us": times["off"]}


def slower(r, a="bank", b="off") -> bool:
    """Path a is slower than path b by more than the spread of the passes."""
    return r[f"{a}_us_per_block"] > r[f"{b}_us_per_block"] and min(r[f"{a}_runs_us"]) > max(r[f"{b}_runs_us"])


def winning_minimum(records):
    """The smallest K from which the bank is not slower than the per-voice path in every row of K and of every larger K
    measured, or None."""
    best = None
    for k in sorted({r["voices"] for r in records}, reverse=True):
        if not any(slower(r) for r in records if r["voices"] == k):
            best = k
        else:
            break
    return best


def write_md(records, path):
    def spread(runs):
        return f"{min(runs):.1f}-{max(runs):.1f}"
    name = records[0]["device"].strip() if records else "?"      # (the runtime may report no marketing name: the arch then)
    lines = ["# Panned voice bank probe (tools/pan_bank_probe.py)", "",
             f"MI355X, {name}, 48 kHz, look-ahead on.  `sine`: MixPE of K SpatialPE(SinePE, SpatialConstantPower(a_i)); `readme`: "
             "README.md's voice under SpatialConstantPower(a_i); `autopan`: BiquadPE(BlitSawPE) under SpatialLinear(azimuth="
             "SinePE(0.2 + 0.01 i, amplitude=60)).  A pass is one whole stream from a fresh start (start, the pulls, a device "
             "synchronise, stop); median of 3 passes after a warm-up pass, the three paths (a graph each) alternating in one "
             "process; us per block = pass / blocks.  `bank`: the voice bank, its root one pgx_pan_mix_batch.  `layered`: the "
             "same bank with voice_bank.FUSED_PAN_MIX = False -- pgx_pan_bank into [K][n][2], then pgx_mix_batch.  `off` is "
             "`mix._bank = False`: the voices rendered one by one -- the code of the commit before the bank --, which "
             "look_ahead.py streams in windows of 8, 16 ... blocks where the blocks are small.  `runs` is the min-max of the "
             "three passes: the spread a difference has to exceed.", ""]
    for kind in KINDS:
        rows = [r for r in records if r["kind"] == kind]
        if not rows:
            continue
        lines += [f"## `{kind}`", "",
                  "| voices | block | blocks per stream | bank us per block | layered us per block | off us per block | bank / off | "
                  "bank / layered | bank runs | layered runs | off runs | first block: bank = off | bank = layered |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['bank_us_per_block']:.1f} | "
                         f"{r['layered_us_per_block']:.1f} | {r['off_us_per_block']:.1f} | {r['bank_over_off']:.3f} | "
                         f"{r['bank_over_layered']:.3f} | {spread(r['bank_runs_us'])} | {spread(r['layered_runs_us'])} | "
                         f"{spread(r['off_runs_us'])} | {r['equal']} | {r['layered_equal']} |")
        lost = [f"{r['voices']} voices x {r['block']} frames" for r in rows if slower(r, "bank", "layered")]
        lines += ["", "Smallest K from which the bank is not slower (beyond the spread) at that K and at every larger K measured, "
                  f"both block lengths: {winning_minimum(rows)}.",
                  "Rows where the fused root is slower than pgx_pan_bank + pgx_mix_batch beyond the spread: "
                  + (", ".join(lost) if lost else "none") + ".", ""]
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
    jsonl, md = os.path.join(OUT, "pan_bank_probe.jsonl"), os.path.join(OUT, "pan_bank_probe.md")
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
