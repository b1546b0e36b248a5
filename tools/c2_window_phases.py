#!/usr/bin/env python3
"""Where a BiquadPE(SinePE) window's time goes: k_biquad_sine_runs at 16 M, 33 M, 2^26 and 134 M frames, as

    time per launch = fixed cost + rounds x cost per round          (a round: one 1024-frame chunk per resident wave)

for the default build with deadline pacing off and on (a switch of the library, not a build), the build without the hot
path's stores (PGX_SB_RUNS_NO_STORE, csrc/pgx_biquad.hip) and the store, prologue and priority variants that were measured
and not kept (experiments/c2_window_variants.patch), and from the
PGX_SB_RUNS_STAMPS build each wave's own clock: the prologue, the first chunk, the spread of the waves' exits and the idle
time between one launch's last exit and the next one's first entry.

    python tools/c2_window_phases.py build [--patched] [--only a,b]  # no GPU needed: experiments/variants/c2w_<name>.so
    python tools/c2_window_phases.py run [--out DIR] [--passes N]   # GPU: three passes, variants interleaved, one process each
    python tools/c2_window_phases.py run --only default,plain_serial
    python tools/c2_window_phases.py run --only default_unpaced,default_paced,stamps_unpaced,stamps_paced

`build` compiles csrc/pgx_biquad.hip (with --patched: a patched copy of it) once per variant and links it with the other
objects of the last library build (pygmu2_amd/csrc/_obj).  `run` writes c2_window_phases.jsonl (raw rows) and
c2_window_phases.md (medians and fits) into DIR (default: runs/).
The fit takes fixed cost and cost per round from the two sizes that fit the 256 MB memory-side cache (64 and 132 MB),
predicts 2^26 from them and prices a storing round of the 134 M-frame window as (t - fixed - warm-up round) / run.
"""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDIR = os.path.join(ROOT, "experiments", "variants")
# (frames, launches timed): about 20 - 40 ms of launches per size, after as many untimed milliseconds -- a burst of a few
# milliseconds runs at another clock than a stream ("Bursts and streams")
SIZES = ((16_000_000, 1000), (33_000_000, 600), (1 << 26, 400), (134_000_000, 300))
SR = 44100.0

# name -> extra compile flags
VARIANTS = {
    "default": [],
    "no_store": ["-DPGX_SB_RUNS_NO_STORE"],
    "stamps": ["-DPGX_SB_RUNS_STAMPS"],
    "pace_eighths": ["-DPGX_SB_RUNS_PACE_SHIFT=3"],          # pacing thresholds at -1/8, +1/8, +3/8 tau
    "pace_halves": ["-DPGX_SB_RUNS_PACE_SHIFT=1"],           # ... at -1/2, +1/2, +3/2 tau
}
# Deadline pacing is a switch of the library (pgx_biquad_sine_set_pacing, PGX_SB_SINE_PACING), not a build: name ->
# (the build it runs, its environment).  `default` and `stamps` themselves run with the library's default.
SWITCHED = {
    "default_unpaced": ("default", {"PGX_SB_SINE_PACING": "0"}),
    "default_paced": ("default", {"PGX_SB_SINE_PACING": "1"}),
    "stamps_unpaced": ("stamps", {"PGX_SB_SINE_PACING": "0"}),
    "stamps_paced": ("stamps", {"PGX_SB_SINE_PACING": "1"}),
    "pace_eighths_paced": ("pace_eighths", {"PGX_SB_SINE_PACING": "1"}),
    "pace_halves_paced": ("pace_halves", {"PGX_SB_SINE_PACING": "1"}),
}
# The variants that were measured and not kept live in experiments/c2_window_variants.patch (PGX_SB_RUNS_VARIANT: bit 0
# write-through stores -- the one kept --, bit 1 a chunk's four LDS reads ahead of its four stores, bit 2 the per-lane
# table loads in front of the barrier, bit 3 write-through for the last two chunks of a range only, bit 4 the wave's issue
# priority turning with its chunks).  `build --patched` compiles them from a patched copy of the source.
PATCHED = {
    "plain_serial": ["-DPGX_SB_RUNS_VARIANT=0"],
    "sc1_serial": ["-DPGX_SB_RUNS_VARIANT=1"],
    "plain_batched": ["-DPGX_SB_RUNS_VARIANT=2"],
    "sc1_batched": ["-DPGX_SB_RUNS_VARIANT=3"],
    "plain_early": ["-DPGX_SB_RUNS_VARIANT=4"],
    "sc1_early": ["-DPGX_SB_RUNS_VARIANT=5"],
    "sc1_batched_early": ["-DPGX_SB_RUNS_VARIANT=7"],
    "sc1_last2": ["-DPGX_SB_RUNS_VARIANT=9"],
    "sc1_last2_early": ["-DPGX_SB_RUNS_VARIANT=13"],
    "plain_turn": ["-DPGX_SB_RUNS_VARIANT=16"],
    "sc1_turn": ["-DPGX_SB_RUNS_VARIANT=17"],
    "sc1_batched_turn": ["-DPGX_SB_RUNS_VARIANT=19"],
    "sc1_batched_early_turn": ["-DPGX_SB_RUNS_VARIANT=23"],
    "no_store_turn": ["-DPGX_SB_RUNS_NO_STORE", "-DPGX_SB_RUNS_VARIANT=16"],
    "stamps_plain_serial": ["-DPGX_SB_RUNS_VARIANT=0", "-DPGX_SB_RUNS_STAMPS"],
    "stamps_sc1_serial": ["-DPGX_SB_RUNS_VARIANT=1", "-DPGX_SB_RUNS_STAMPS"],
    "stamps_sc1_last2": ["-DPGX_SB_RUNS_VARIANT=9", "-DPGX_SB_RUNS_STAMPS"],
    "stamps_plain_turn": ["-DPGX_SB_RUNS_VARIANT=16", "-DPGX_SB_RUNS_STAMPS"],
    "stamps_sc1_turn": ["-DPGX_SB_RUNS_VARIANT=17", "-DPGX_SB_RUNS_STAMPS"],
}


def lib_of(name):
    return os.path.join(VDIR, f"c2w_{SWITCHED.get(name, (name,))[0]}.so")


def build(only=None, patched=False):
    sys.path.insert(0, ROOT)
    from pygmu2_amd import build as B
    B.build()
    unit = "pgx_biquad.hip"                                  # the unit that holds k_biquad_sine_runs
    source, variants = os.path.join(B.CSRC, unit), dict(VARIANTS)
    if patched:
        os.makedirs(VDIR, exist_ok=True)
        source = os.path.join(VDIR, "pgx_biquad_variants.hip")
        subprocess.check_call(["patch", "-s", "-o", source, os.path.join(B.CSRC, unit),
                               os.path.join(ROOT, "experiments", "c2_window_variants.patch")])
        variants.update(PATCHED)
    obj_dir = os.path.join(B.CSRC, "_obj")
    others = [os.path.join(obj_dir, s.replace(".hip", ".o")) for s in B.SOURCES if s != unit]
    os.makedirs(VDIR, exist_ok=True)
    flags = [f for f in B.FLAGS if f != "-shared"]
    def one(item):
        name, extra = item
        obj = os.path.join(VDIR, f"c2w_{name}.o")
        subprocess.check_call([B._hipcc()] + flags + extra + ["-I" + os.path.join(ROOT, "include"), "-I" + B.CSRC, "-c",
                                                             source, "-o", obj])
        subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_of(name), obj] + others +
                              ["-ldl"])
        print("[c2_window_phases] built", lib_of(name), flush=True)

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(one, [(k, v) for k, v in variants.items() if not only or k in only]))


# ---------------------------------------------------------------------------------------------- one process per variant
def worker(stamps):
    """Runs in a process whose PGX_LIB_PATH names the variant; prints one JSON row per size."""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, ROOT)
    import pygmu2_amd as pg
    from pygmu2_amd import device
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    lib = device.ensure_init()
    lib.pgx_biquad_sine_set_runs(1)
    c = rbj_coefficients(pg.BiquadMode.LOWPASS, 1000.0, 0.707, 0.0, SR)
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    settle = settle_frames(c[3], c[4])
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((SIZES[-1][0], 1), np.float32)
    w = 2.0 * np.pi * 440.0
    raw = C.CDLL(device.LIB_PATH)
    for frames, launches in SIZES:
        plan = (C.c_int * 5)()
        assert lib.pgx_biquad_sine_runs_plan(frames, settle, plan) == 1, frames
        run, head, tail, warm, waves = plan

        def launch():
            device.check(lib.pgx_biquad_sine(out.ptr, 10 ** 9, frames, SR, w, 1.0, 0.0, coef.ptr, tables.ptr, settle,
                                             state.ptr, None))

        for _ in range(launches // 2):
            launch()
        e0, e1 = device.Event(), device.Event()
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        device.synchronize()
        row = {"frames": frames, "rounds": run + warm, "run": run, "warm": warm, "waves": waves,
               "us": round(e1.elapsed_ms_since(e0) / launches * 1e3, 3)}
        info = (C.c_int64 * 3)()                               # the last launch: its duration and its tau, in ticks
        device.check(raw.pgx_biquad_sine_pacing_info(info))
        row.update(pacing_ticks=info[1], pacing_tau=info[2])
        if stamps:
            buf = np.zeros((2, 4096, 4), dtype=np.uint64)
            count = raw.pgx_biquad_sine_runs_stamps(C.c_void_p(buf.ctypes.data))
            assert count >= 2, count
            last, prev = buf[(count - 1) & 1, :waves].astype(np.int64), buf[count & 1, :waves].astype(np.int64)
            us = lambda ticks: round(float(ticks) / 100.0, 2)                  # wall_clock64: 100 MHz
            if os.environ.get("C2W_DUMP_STAMPS"):                              # every wave's four stamps, per size
                np.save(os.environ["C2W_DUMP_STAMPS"] + f"_{frames}.npy", last - last[:, 0].min())
            exits = last[:, 3] - last[:, 0].min()
            row.update(stamp_entry_spread_us=us(last[:, 0].max() - last[:, 0].min()),
                       stamp_prologue_us=us(np.median(last[:, 1] - last[:, 0])),
                       stamp_prologue_max_us=us((last[:, 1] - last[:, 0]).max()),
                       stamp_first_chunk_us=us(np.median(last[1:, 2] - last[1:, 1])),
                       stamp_exit_min_us=us(exits.min()), stamp_exit_median_us=us(np.median(exits)),
                       stamp_exit_max_us=us(exits.max()), stamp_exit_spread_us=us(exits.max() - exits.min()),
                       # (the earliest exit is the last wave's, whose run is the remainder: shorter than the others')
                       stamp_exit_p01_us=us(np.percentile(exits, 1)), stamp_exit_p99_us=us(np.percentile(exits, 99)),
                       stamp_idle_between_launches_us=us(last[:, 0].min() - prev[:, 3].max()),
                       stamp_start_to_start_us=us(last[:, 0].min() - prev[:, 0].min()))
        print(json.dumps(row), flush=True)


def fit(us_by_frames, rounds_by_frames, runs_by_frames):
    """fixed and per-round cost from the two cache-resident sizes; the 2^26 prediction; a storing round at 134 M."""
    (f0, _), (f1, _), (f2, _), (f3, _) = SIZES
    per_round = (us_by_frames[f1] - us_by_frames[f0]) / (rounds_by_frames[f1] - rounds_by_frames[f0])
    fixed = us_by_frames[f0] - per_round * rounds_by_frames[f0]
    warm_rounds = rounds_by_frames[f3] - runs_by_frames[f3]
    return {"fixed_us": round(fixed, 2), "us_per_round": round(per_round, 3),
            "predicted_2p26_us": round(fixed + per_round * rounds_by_frames[f2], 2), "measured_2p26_us": us_by_frames[f2],
            "us_per_storing_round_134M": round((us_by_frames[f3] - fixed - warm_rounds * per_round) / runs_by_frames[f3], 3)}


def run(out_dir, only, passes=3):
    names = [n for n in list(VARIANTS) + list(SWITCHED) + list(PATCHED)
             if os.path.exists(lib_of(n)) and (not only or n in only)]
    assert names, "no variant library: run `build` first"
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    with open(os.path.join(out_dir, "c2_window_phases.jsonl"), "w") as raw:
        for p in range(passes):
            for name in names:
                env = dict(os.environ, PGX_LIB_PATH=lib_of(name), **SWITCHED.get(name, (name, {}))[1])
                if name.startswith("stamps") and p == 0:
                    env["C2W_DUMP_STAMPS"] = os.path.join(out_dir, f"c2_window_stamps_{name}")
                cmd = [sys.executable, os.path.abspath(__file__), "worker"] + (["--stamps"] if name.startswith("stamps") else [])
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
                if r.returncode != 0:          # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"{name}: worker exit {r.returncode}")
                for line in r.stdout.splitlines():
                    if line.startswith("{"):
                        row = dict(json.loads(line), variant=name, **{"pass": p})
                        rows.append(row)
                        raw.write(json.dumps(row) + "\n")
                        raw.flush()
                        print(json.dumps(row), flush=True)
    md = ["| variant | " + " | ".join(f"{f} (each pass, µs)" for f, _ in SIZES) +
          " | fixed µs | µs / round | 2²⁶ predicted | µs / storing round, 134 M |", "|---|" + "---|" * 8]
    stamp_md = []
    for name in names:
        mine = [r for r in rows if r["variant"] == name]
        med, rounds, runs, cells = {}, {}, {}, []
        for f, _ in SIZES:
            t = sorted(r["us"] for r in mine if r["frames"] == f)
            med[f] = statistics.median(t)
            rounds[f] = next(r["rounds"] for r in mine if r["frames"] == f)
            runs[f] = next(r["run"] for r in mine if r["frames"] == f)
            cells.append(" / ".join(f"{x:.1f}" for x in t))
        ft = fit(med, rounds, runs)
        md.append(f"| {name} | " + " | ".join(cells) + f" | {ft['fixed_us']} | {ft['us_per_round']} | "
                  f"{ft['predicted_2p26_us']} | {ft['us_per_storing_round_134M']} |")
        print(json.dumps(dict(ft, variant=name, medians_us=med)), flush=True)
        if name.startswith("stamps"):
            keys = [k for k in mine[0] if k.startswith("stamp_")]
            stamp_md += ["", f"Stamps, `{name}` (median of the passes; the last of the timed launches):", "",
                         "| frames | " + " | ".join(k[6:-3].replace("_", " ") for k in keys) + " |",
                         "|---|" + "---|" * len(keys)]
            for f, _ in SIZES:
                stamp_md.append(f"| {f} | " + " | ".join(
                    f"{statistics.median(r[k] for r in mine if r['frames'] == f):.2f}" for k in keys) + " |")
    with open(os.path.join(out_dir, "c2_window_phases.md"), "w") as f:
        f.write("\n".join(md + stamp_md) + "\n")
    print("\n".join(md + stamp_md))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "build":
        build(sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None, "--patched" in sys.argv)
    elif mode == "worker":
        worker("--stamps" in sys.argv)
    elif mode == "run":
        out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "runs")
        only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
        run(out_dir, only, int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 3)
    else:
        raise SystemExit(__doc__)
