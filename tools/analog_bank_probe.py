"""
AnalogOscPE voice bank against the per-voice path (`mix._bank = False`: how every such MixPE was rendered before the
bank took these classes), at 48 kHz, on the reference's PWM voice under an envelope:

    MixPE of K x GainPE(AnalogOscPE(f_i, duty_cycle=TransformPE(SinePE(r_i), Affine(0.4, 0.5)), "rectangle"),
                        gain=AdsrGatedPE(PeriodicGate(g_i, 0.5), 0.01, 0.05, 0.6, 0.03))

K = 4, 8, 64, 512, streamed in blocks of 4 096 and of 48 000 frames.  Per step: a graph per path; a pass is one whole
stream from a fresh start (renderer start, the pulls, a device synchronise, stop) -- a short stream of 8 blocks and a
long one (STREAMS), because the per-voice path renders a stream in look-ahead windows of 8, 16 ... 256 blocks and a
handful of blocks in the middle of a stream cost it either nothing or a whole window; a warm-up pass, then three timed
passes per path, alternating in the same process; the median (min and max are kept: the spread) as microseconds per
block.  A third column is the bank under voice_bank.BANK_WINDOWS_ANY_ROOT, the experiment switch that lets any bank of
up to 256 voices stream in windows of 2, 4, 8 blocks.  The two paths' outputs are compared on fresh graphs over two
blocks (np.array_equal).  Every step is a process of its own under its own time limit, and the first step that fails
ends the probe (what `timeout ... step && timeout ... step && ...` does in a shell).

The result decides voice_bank.ANALOG_OSC_MIN_VOICES: the smallest K from which the bank is faster at that K and at
every larger K measured, at both block lengths and both stream lengths (the probe itself sets the switch to
voice_bank.MIN_VOICES, so that the smaller banks are built at all).

    python tools/analog_bank_probe.py            writes profiles/analog_bank_probe.jsonl and profiles/analog_bank_probe.md
    python tools/analog_bank_probe.py --step K BLOCK      one step, its record on stdout
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
VOICES = (4, 8, 64, 512)
BLOCKS = (4096, 48_000)
# blocks per stream.  The per-voice path streams through look_ahead.py's windows of 8, 16 ... 256 blocks, so a stream is
# timed whole, from a fresh start: a short one (the first window) and a long one that ends with a window (8 + ... + 256
# + 256 + 256 blocks of 4 096 frames: 87 s of audio; 8 + ... + 64 blocks of 48 000 frames: two minutes)
STREAMS = {4096: (8, 1016), 48_000: (8, 120)}
STEP_SECONDS = 150
OUT = os.environ.get("ANALOG_BANK_PROBE_OUT", os.path.join(ROOT, "profiles"))


def voice(pg, i):
    duty = pg.TransformPE(pg.SinePE(frequency=0.7 + 0.031 * i), func=pg.transforms.Affine(0.4, 0.5))
    osc = pg.AnalogOscPE(109.37 * 2 ** ((i % 72) / 12), duty, "rectangle")
    gate = pg.PeriodicGate(3.0 + 0.017 * i, 0.5)
    return pg.GainPE(osc, gain=pg.AdsrGatedPE(gate, 0.01, 0.05, 0.6, 0.03))


def step(k: int, block: int) -> list:
    import numpy as np

    import pygmu2_amd as pg
    from pygmu2_amd import device, voice_bank

    pg.set_sample_rate(SR)
    voice_bank.ANALOG_OSC_MIN_VOICES = voice_bank.MIN_VOICES      # what is being measured: banks below it too

    def mix(bank):
        m = pg.MixPE(*[voice(pg, i) for i in range(k)])
        if not bank:
            m._bank = False
        return m

    def stream(m, blocks, windows=False):
        """One stream from a fresh start: start, `blocks` pulls, a device synchronise, stop.  -> seconds"""
        voice_bank.BANK_WINDOWS_ANY_ROOT = windows
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
        voice_bank.BANK_WINDOWS_ANY_ROOT = False
        return t

    outs = {}
    for bank in (True, False):
        m = mix(bank)
        outs[bank] = np.concatenate([m.render(s, block).data for s in (0, block)])
        assert bool(m._bank) == bank
        del m
    equal = bool(np.array_equal(outs[True], outs[False]))
    del outs

    # (mode, MixPE, windows): the bank, the per-voice path, and the bank under voice_bank.BANK_WINDOWS_ANY_ROOT (an
    # experiment switch, off by default: windows of 2, 4, 8 blocks for banks of up to BANK_WINDOW_MAX_VOICES voices)
    modes = (("bank", mix(True), False), ("off", mix(False), False), ("bank_windows", mix(True), True))
    records = []
    for blocks in STREAMS[block]:
        times = {name: [] for name, _, _ in modes}
        for rep in range(4):                              # pass 0 warms every path up
            for name, m, windows in modes:
                t = stream(m, blocks, windows)
                if rep:
                    times[name].append(1e6 * t / blocks)
        med = {name: float(np.median(v)) for name, v in times.items()}
        records.append({"voices": k, "block": block, "stream_blocks": blocks, "equal": equal,
                        "device": device.device_name(), "bank_us_per_block": med["bank"],
                        "off_us_per_block": med["off"], "bank_windows_us_per_block": med["bank_windows"],
                        "bank_over_off": med["bank"] / med["off"], "bank_runs_us": times["bank"],
                        "off_runs_us": times["off"], "bank_windows_runs_us": times["bank_windows"]})
    return records


def winning_minimum(records, long_streams):
    """The smallest K from which the bank is faster at K and at every larger K measured (both block lengths; the long
    streams or the short ones), or None."""
    rows = [r for r in records if (r["stream_blocks"] > 8) == long_streams]
    best = None
    for k in sorted({r["voices"] for r in rows}, reverse=True):
        if all(r["bank_us_per_block"] < r["off_us_per_block"] for r in rows if r["voices"] == k):
            best = k
        else:
            break
    return best


def write_md(records, path):
    def spread(runs):
        return f"{min(runs):.1f}-{max(runs):.1f}"
    name = records[0]["device"] if records else "?"
    lines = ["# AnalogOscPE voice bank probe (tools/analog_bank_probe.py)", "",
             f"MI355X ({name}), 48 kHz, MixPE of K GainPE(AnalogOscPE(f, duty=TransformPE(SinePE), rectangle), "
             "gain=AdsrGatedPE(PeriodicGate)) voices.  A pass is one whole stream from a fresh start (start, the pulls, a device "
             "synchronise, stop); median of 3 passes after a warm-up pass, the paths (a graph each) alternating in one process; "
             "us per block = pass / blocks.  `off` is `mix._bank = False`: the voices rendered one by one, which look_ahead.py "
             "streams in windows of 8, 16 ... 256 blocks.  `bank + windows` is the bank under `voice_bank.BANK_WINDOWS_ANY_ROOT` "
             "(off by default).  `runs` is the min-max of the three passes: the spread a difference has to exceed.", "",
             "| voices | block | blocks per stream | bank us per block | off us per block | bank / off | bank + windows us per block | "
             "bank runs | off runs | bank + windows runs | outputs equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        lines.append(f"| {r['voices']} | {r['block']} | {r['stream_blocks']} | {r['bank_us_per_block']:.1f} | "
                     f"{r['off_us_per_block']:.1f} | {r['bank_over_off']:.3f} | {r['bank_windows_us_per_block']:.1f} | "
                     f"{spread(r['bank_runs_us'])} | {spread(r['off_runs_us'])} | {spread(r['bank_windows_runs_us'])} | "
                     f"{r['equal']} |")
    lines += ["", "Smallest K from which the bank is faster at that K and at every larger K measured, both block lengths: "
              f"streams of 8 blocks {winning_minimum(records, False)}, long streams {winning_minimum(records, True)}."]
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
            for line in done.stdout.strip().splitlines()[-len(STREAMS[block]):]:
                records.append(json.loads(line))
                print(line, flush=True)
        if status:
            break
    with open(os.path.join(OUT, "analog_bank_probe.jsonl"), "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    if records:
        write_md(records, os.path.join(OUT, "analog_bank_probe.md"))
    return status


if __name__ == "__main__":
    sys.exit(main())
