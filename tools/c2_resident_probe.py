#!/usr/bin/env python3
"""The closed-form BiquadPE(SinePE) window kernel (k_biquad_tone, csrc/pgx_tone.hip) at window sizes that stay in the
256 MiB memory-side cache: 16 M, 24 M, 30 M and 32 M frames, each into one buffer that is rewritten and into two buffers
that take turns, as the look-ahead windows of a stream do (two live windows).  The C2 chain at start 10^9, called as a
window calls it (carried state in, no snapshot), HIP events over 20 - 40 ms of launches after half as many untimed, one
process per variant, variants interleaved, three passes.  Per variant and buffer count: time = fixed + slope x M frames,
least squares over the four sizes.

Variants (switches of pgx_tone.hip, compiled into experiments/variants/c2r_<name>.so):
    as_is       what ships: 16 KB per workgroup, write-through (sc1) stores
    plain       plain stores instead of sc1                                   -DPGX_TONE_STORE_AUX=0
    two_pieces  two 16 KB pieces per workgroup: half the workgroups, one anchor sincos per 32 frames (every second
                anchor of as_is is replaced by a rotation: not the same bits)  -DPGX_TONE_GROUPS=8

    python tools/c2_resident_probe.py build                           # no GPU needed
    python tools/c2_resident_probe.py run [--out DIR] [--passes N]    # GPU; writes DIR/c2_resident_probe.{jsonl,md}
    python tools/c2_resident_probe.py single [--out DIR] [--passes N] # GPU; writes DIR/c2_single_window_probe.{jsonl,md}

`single` asks what one live window would buy a stream: the package's own library at 36 M frames (the stream's window
today) and at 40 - 67 M frames, beyond what two buffers keep in the cache, each into one rewritten buffer and into two in
turn, the same protocol.  It reports the cost per M frames and whether one buffer at some size >= 48 M is cheaper than
two buffers at 36 M with ranges that do not touch.

DIR defaults to runs/.
"""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDIR = os.path.join(ROOT, "experiments", "variants")
# (frames, launches timed): 8.3 TB/s is about 0.5 us per M frames
SIZES = ((16_000_000, 3000), (24_000_000, 2200), (30_000_000, 1800), (32_000_000, 1700))
# `single`: 36 M (two live windows of a stream today) and the sizes one live window could take
SINGLE_SIZES = ((36_000_000, 1500), (40_000_000, 1350), (48_000_000, 1100), (56_000_000, 950), (60_000_000, 900),
                (64_000_000, 850), (67_000_000, 800))
SINGLE_BASE, SINGLE_FROM = 36_000_000, 48_000_000
SR = 44100.0
VARIANTS = {"as_is": [], "plain": ["-DPGX_TONE_STORE_AUX=0"], "two_pieces": ["-DPGX_TONE_GROUPS=8"]}


def lib_of(name):
    return os.path.join(VDIR, f"c2r_{name}.so")


def build():
    sys.path.insert(0, ROOT)
    from pygmu2_amd import build as B
    B.build()
    obj_dir = os.path.join(B.CSRC, "_obj")
    others = [os.path.join(obj_dir, s.replace(".hip", ".o")) for s in B.SOURCES if s != "pgx_tone.hip"]
    os.makedirs(VDIR, exist_ok=True)
    flags = [f for f in B.FLAGS if f != "-shared"]
    for name, extra in VARIANTS.items():
        obj = os.path.join(VDIR, f"c2r_{name}.o")
        subprocess.check_call([B._hipcc()] + flags + extra + ["-I" + os.path.join(ROOT, "include"), "-I" + B.CSRC, "-c",
                                                             os.path.join(B.CSRC, "pgx_tone.hip"), "-o", obj])
        subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_of(name), obj] + others +
                              ["-ldl"])
        print("[c2_resident_probe] built", lib_of(name), flush=True)


def worker(sizes=SIZES):
    """Runs in a process whose PGX_LIB_PATH names the variant; prints one JSON row per (size, buffers)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import pygmu2_amd as pg
    from pygmu2_amd import device
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    lib = device.ensure_init()
    c = rbj_coefficients(pg.BiquadMode.LOWPASS, 1000.0, 0.707, 0.0, SR)
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    settle = settle_frames(c[3], c[4])
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer((1, 2), np.float64, zero=True)
    w = 2.0 * np.pi * 440.0
    plan = lib.pgx_biquad_tone_plan(SR, w, 1.0, 0.0, *c, tables.ptr, settle)
    assert plan
    outs = [device.DeviceBuffer((sizes[-1][0], 1), np.float32) for _ in range(2)]
    for frames, launches in sizes:
        for buffers in (1, 2):
            turn = [0]

            def launch():
                turn[0] ^= buffers - 1
                device.check(lib.pgx_biquad_tone_window(plan, outs[turn[0]].ptr, 10 ** 9, frames, state.ptr, None))

            for _ in range(launches // 2):
                launch()
            e0, e1 = device.Event(), device.Event()
            e0.record()
            for _ in range(launches):
                launch()
            e1.record()
            device.synchronize()
            us = e1.elapsed_ms_since(e0) / launches * 1e3
            print(json.dumps({"frames": frames, "buffers": buffers, "launches": launches, "us": round(us, 3),
                              "tb_s": round(4.0 * frames / us / 1e6, 3)}), flush=True)
    lib.pgx_biquad_tone_plan_free(plan)


def fit(points):
    """Least squares of us = fixed + slope * (frames / 1e6)."""
    xs, ys = [f / 1e6 for f, _ in points], [u for _, u in points]
    mx, my = statistics.fmean(xs), statistics.fmean(ys)
    slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    return my - slope * mx, slope


def run(out_dir, passes):
    names = [n for n in VARIANTS if os.path.exists(lib_of(n))]
    assert names, "no variant library: run `build` first"
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    with open(os.path.join(out_dir, "c2_resident_probe.jsonl"), "w") as raw:
        for p in range(passes):
            for name in names:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker"], capture_output=True, text=True,
                                   timeout=240, env=dict(os.environ, PGX_LIB_PATH=lib_of(name)))
                if r.returncode != 0:          # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"{name}: worker exit {r.returncode}")
                for line in r.stdout.splitlines():
                    if line.startswith("{"):
                        row = dict(json.loads(line), variant=name, **{"pass": p})
                        rows.append(row)
                        raw.write(json.dumps(row) + "\n")
                        raw.flush()
    md = ["# `k_biquad_tone` at cache-resident window sizes, one buffer and two in turn", "",
          f"µs per launch, median [min – max] of {passes} passes; fit: fixed µs + µs per M frames (TB/s of the slope):", "",
          "| variant | buffers | " + " | ".join(f"{f // 10 ** 6} M" for f, _ in SIZES) + " | fit |", "|---|---|" + "---|" * (len(SIZES) + 1)]
    for name in names:
        for buffers in (1, 2):
            cells, points = [], []
            for f, _ in SIZES:
                t = sorted(r["us"] for r in rows if r["variant"] == name and r["frames"] == f and r["buffers"] == buffers)
                points.append((f, statistics.median(t)))
                cells.append(f"{points[-1][1]:.2f} [{t[0]:.2f} – {t[-1]:.2f}]")
            fixed, slope = fit(points)
            md.append(f"| {name} | {buffers} | " + " | ".join(cells) + f" | {fixed:.2f} + {slope:.3f} ({4.0 / slope:.2f}) |")
    with open(os.path.join(out_dir, "c2_resident_probe.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print("\n".join(md))


def run_single(out_dir, passes):
    os.makedirs(out_dir, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "PGX_LIB_PATH"}          # the package's own library
    rows = []
    with open(os.path.join(out_dir, "c2_single_window_probe.jsonl"), "w") as raw:
        for p in range(passes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker-single"], capture_output=True,
                               text=True, timeout=240, env=env)
            if r.returncode != 0:              # nothing more is started on the device after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"worker exit {r.returncode}")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    row = dict(json.loads(line), **{"pass": p})
                    rows.append(row)
                    raw.write(json.dumps(row) + "\n")
                    raw.flush()

    def per_m(frames, buffers):
        t = sorted(r["us"] / (frames / 1e6) for r in rows if r["frames"] == frames and r["buffers"] == buffers)
        return statistics.median(t), t[0], t[-1]

    md = ["# `k_biquad_tone`: one rewritten buffer against two in turn, 36 M to 67 M frames", "",
          f"µs per launch and µs per M frames, median [min – max] of {passes} passes, each pass a process of its own:", "",
          "| frames | buffers | µs per launch | µs per M frames |", "|---|---|---|---|"]
    for f, _ in SINGLE_SIZES:
        for buffers in (1, 2):
            t = sorted(r["us"] for r in rows if r["frames"] == f and r["buffers"] == buffers)
            m = per_m(f, buffers)
            md.append(f"| {f // 10 ** 6} M | {buffers} | {statistics.median(t):.2f} [{t[0]:.2f} – {t[-1]:.2f}] | "
                      f"{m[0]:.4f} [{m[1]:.4f} – {m[2]:.4f}] |")
    base = per_m(SINGLE_BASE, 2)
    better = [f for f, _ in SINGLE_SIZES if f >= SINGLE_FROM and per_m(f, 1)[0] < base[0] and per_m(f, 1)[2] < base[1]]
    md += ["", f"Two buffers at {SINGLE_BASE // 10 ** 6} M: {base[0]:.4f} [{base[1]:.4f} – {base[2]:.4f}] µs per M frames.  "
           + ("One buffer is cheaper, ranges apart, at " + ", ".join(f"{f // 10 ** 6} M" for f in better) + ": go."
              if better else f"No size from {SINGLE_FROM // 10 ** 6} M on is cheaper into one buffer with ranges apart: no-go.")]
    with open(os.path.join(out_dir, "c2_single_window_probe.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "build":
        build()
    elif mode == "worker":
        worker()
    elif mode == "worker-single":
        worker(SINGLE_SIZES)
    elif mode == "single":
        out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "runs")
        run_single(out_dir, int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 3)
    elif mode == "run":
        out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "runs")
        run(out_dir, int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 3)
    else:
        raise SystemExit(__doc__)
