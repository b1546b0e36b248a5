"""
Every channel-aware PE at 3, 4, 5 and 8 channels -- the case list shared by tools/gen_golden_channels.py (the
reference's renders: tests/golden/channels_cases.json + channels.npz), tests/test_oracle_channels.py (the oracle against
those renders, and the comparison against itself) and tests/test_gpu_channels.py (the HIP path against both).

Cases are written in the spec language of oracle/golden_cases.py.  A processor reads an rng ArrayPE whose columns all
differ, so a swapped or repeated channel index changes the result; a source is built with `channels=C` (its columns are
equal: `"tiled": True`).  Elementwise, lookup and source kinds run at C in (3, 4, 5, 8): a float4 straddles frames at 3,
lies inside one frame at 5, and a frame is one or two float4s at 4 and 8.  Chain-parallel recurrences run at (3, 5, 8).

Pull patterns
-------------
BLOCKS  [-37, 1] [-36, 17] [-19, 257] [238, 1000] [1238, 4099], contiguous from a negative start (state is carried;
        n * C mod 4 takes 0, 1 and 3 at C = 3 and 5), then [9000, 64] after a gap.
long    BLOCKS with one more contiguous block [5337, L] before the gap, L the smallest length past a switch in the
        kernel's dispatcher that BLOCKS does not reach (table below).
stream  24 blocks of 256 frames from -300, one of them 17 frames long, a step back of 300 frames before block 13 and a
        seek of 3000 frames before block 19 (as `_stream` of oracle/gen_golden_fuzz.py): one case per recurrence family
        at C = 3, rendered with look-ahead on and off.

Length switches (entry point; the switch as its dispatcher states it; the length that crosses it)
-------------------------------------------------------------------------------------------------
pgx_biquad_const     one workgroup per chain while ceil(n / 4096) <= 2 (biquad_settled_plan: `halves <= 2`); beyond,
                     with a warm-up of one half-tile (settle 1024 for the case's section), head + tail = 2 halves and
                     `halves > head + tail` gives the segmented settled kernel -- or, without tables, biquad_plan's
                     reduce / apply pair (nseg = 3): n > 8192.                                           L = 8193
pgx_biquad_varying   scan2_plan: one workgroup while ceil(n / 1024) <= 2, reduce / apply beyond: n > 2048.
pgx_svf              the same plan.                                  BLOCKS' 4099 is past it, its 1000 below: no L
pgx_ladder           ladder_plan: segmented when n >= 2 * (settle + seg_len), seg_len = max(32, ceil(n * C / 16384));
                     ladder_settle_frames(1200 Hz, 0.3, 48 kHz, x2) = 1024, so n >= 2112.
                                                                     BLOCKS' 4099 is past it, its 1000 below: no L
pgx_ladder, PE cutoff  LadderPE._settle_frames_for_streams: no segments below STREAM_SEGMENT_MIN_FRAMES = 8192 frames;
                     from there the warm-up planned for the sweep's lowest cutoff (1.5 x 672 = 1008 at 2 kHz) is far
                     below n / 2: n >= 8192.                                                             L = 8192
pgx_comb, constant   poly_plan: one segment while ceil(n / D) <= 1024 steps (kPolySingleSteps); D = 4 frames at
                     12 kHz / 48 kHz: n > 4096.                      BLOCKS' 4099 is past it, its 1000 below: no L
pgx_comb, PE freq    k_comb_delays in several workgroups when n > 4096 (kCtlTile; BLOCKS' 4099); the three-pass
                     segment path when n >= 3 * kSegLen = 12 288 (comb_stream_segmented).              L = 12 288
pgx_window           k_window_blocks runs when (n + 2 * half_window) / 64 >= 1: with window 0 BLOCKS' 1 and 17 are
                     below it, 257 past it.                                                                  no L
pgx_karplus_strong   the line lives in LDS while lanes * max_line * 4 <= 64 KiB: one string of more than 16 384 frames
                     (2 Hz at 44.1 kHz: 22 050) takes the global-memory kernel; the feedback shows after one pass
                     of the line.                                                       L = 22 051 (frequency 2 Hz)
pgx_envelope         k_env_newton's tile shape changes at n > 1024, 2048 and 4096 (BLOCKS' 1000 and 4099; 2049 is the
                     envelope cases' L); all windows at once from n >= 16 * 8192 = 131 072 (kEnvMwMinFrames).
                                                                           L = 2049; and one case at C = 3, L = 131 072
pgx_adsr             mono: no channel path.
(pgx_slew's multi-window rounds start at 131 072 frames as well; SlewLimiterPE reads channel 0 of a wider source and
gives one channel, so a longer block adds no channel path to its family cases.)

Families with oracles of their own
----------------------------------
WavetablePE / TimeWarpPE, SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE, TralfamPE / SlicePE / SetExtentPE
and SequencePE are not in the spec language of oracle/graph_eval.py.  Their cases at 3, 4, 5 and 8 channels (`ch<C>_*`)
are listed in their own generators (tools/gen_golden_playback.py, gen_golden_control.py, gen_golden_tralfam.py,
gen_golden_score.py: `channel_cases` or the block at the end of `cases`), stored in their own fixtures and run by their
own host and GPU modules in the class each family has there.  The reference's NoisePE has one channel and no
`channels` parameter: nothing to add.
"""

from __future__ import annotations

from oracle.golden_cases import S

ELEMENTWISE_C = (3, 4, 5, 8)
CHAIN_C = (3, 5, 8)

BLOCKS = [[-37, 1], [-36, 17], [-19, 257], [238, 1000], [1238, 4099]]
GAP_BLOCK = 64
LONG_AT = 5337                      # where BLOCKS ends: a long block goes here


def blocks(long=None):
    out = [list(b) for b in BLOCKS]
    end = LONG_AT
    if long is not None:
        out.append([end, int(long)])
        end += int(long)
    out.append([end + 3663, GAP_BLOCK])
    return out


def stream_blocks():
    out, pos = [], -300
    for i in range(24):
        if i == 13:
            pos -= 300
        if i == 19:
            pos += 3000
        n = 17 if i == 7 else 256
        out.append([pos, n])
        pos += n
    return out


def _frames(blks):
    return max(s + n for s, n in blks) + 200


def cases():
    out = []
    seeds = iter(range(1000, 100000))

    def noise(ch, n, scale=0.5, **kw):
        return S("ArrayPE", data=dict({"rng": next(seeds), "n": int(n), "ch": int(ch), "scale": scale}, **kw))

    def add(kind, variant, c, sr, graph, *, long=None, tiled=False, pattern=None, blks=None):
        blks = blks if blks is not None else (stream_blocks() if pattern == "stream" else blocks(long))
        pattern = pattern or ("long" if long is not None else "blocks")
        out.append({"name": f"{kind}_{variant}_c{c}" + ("_stream" if pattern == "stream" else ""), "kind": kind, "C": c,
                    "sr": sr, "graph": graph, "blocks": blks, "pattern": pattern, "tiled": bool(tiled),
                    "long_index": len(BLOCKS) if long is not None else None})

    fm = S("MixPE", inputs=[S("ConstantPE", value=440.0), S("SinePE", frequency=5.0, amplitude=50.0)])
    sweep = S("MixPE", inputs=[S("ConstantPE", value=1200.0), S("SinePE", frequency=3.0, amplitude=900.0)])
    N = _frames(blocks())

    # ------------------------------------------------------------------------------------------------ sources
    for c in ELEMENTWISE_C:
        add("ConstantPE", "quarter", c, 44100, S("ConstantPE", value=0.25, channels=c), tiled=True)
        add("IdentityPE", "gain", c, 44100, S("GainPE", source=S("IdentityPE", channels=c), gain=1.3e-4), tiled=True)
        add("DiracPE", "unit", c, 44100, S("DiracPE", channels=c), tiled=True)
        add("SinePE", "pure", c, 44100, S("SinePE", frequency=440.0, amplitude=0.8, phase=0.3, channels=c), tiled=True)
        add("SinePE", "fm", c, 44100, S("SinePE", frequency=fm, amplitude=0.5, channels=c), tiled=True)
        add("BlitSawPE", "m20", c, 48000,
            S("BlitSawPE", frequency=110.0, amplitude=0.7, initial_phase=0.25, m=20, leak=0.995, channels=c), tiled=True)
        add("SuperSawPE", "6v", c, 48000,
            S("SuperSawPE", frequency=110.0, amplitude=0.8, voices=6, detune_cents=35.0, mix_mode="linear", channels=c,
              seed=7), tiled=True)
        add("AnalogOscPE", "rect", c, 44100,
            S("AnalogOscPE", frequency=517.0, duty_cycle=0.41, waveform="rectangle", channels=c), tiled=True)
        add("AnalogOscPE", "saw", c, 44100,
            S("AnalogOscPE", frequency=331.0, duty_cycle=0.3, waveform="sawtooth", channels=c), tiled=True)
        add("AnalogOscPE", "saw_fm", c, 44100,
            S("AnalogOscPE", frequency=S("PiecewisePE", points=[[0, 90.0], [3000, 1370.0], [6000, -240.0]],
                                         transition_type="linear", extend_mode="hold_both"),
              duty_cycle=S("TransformPE", source=S("SinePE", frequency=3.1), ops=[["affine", 0.35, 0.5]]),
              waveform="sawtooth", channels=c), tiled=True)
        add("PiecewisePE", "exp", c, 44100,
            S("PiecewisePE", points=[[-30, 2.0], [500, -1.0], [200, 0.0], [5000, 0.7]], transition_type="exponential",
              extend_mode="hold_both", channels=c), tiled=True)
        add("PiecewisePE", "linear_zero", c, 44100,
            S("PiecewisePE", points=[[-20, 0.0], [100, 1.0], [400, 0.25], [401, 0.9], [5100, 0.5]],
              transition_type="linear", extend_mode="zero", channels=c), tiled=True)
        add("ArrayPE", "zero", c, 44100, noise(c, 9040))
        add("ArrayPE", "hold_both", c, 44100, dict(noise(c, 9030), extend_mode="hold_both"))
    for c in CHAIN_C:
        add("KarplusStrongPE", "two_phase", c, 44100,
            S("KarplusStrongPE", frequency=196.0, rho=0.998, duration=2500, rho_damping=0.95, amplitude=0.5, seed=7,
              channels=c), tiled=True)
    add("KarplusStrongPE", "beyond_lds", 3, 44100,
        S("KarplusStrongPE", frequency=2.0, rho=0.99, amplitude=0.4, seed=11, channels=3), long=22051, tiled=True)

    # ------------------------------------------------------------------------------------------------ element / index
    trig = S("PeriodicTrigger", hz=23.0)
    for c in ELEMENTWISE_C:
        add("GainPE", "const", c, 44100, S("GainPE", source=noise(c, N), gain=0.37))
        add("GainPE", "mono_pe", c, 44100, S("GainPE", source=noise(c, N), gain=S("SinePE", frequency=5.0)))
        add("GainPE", "wide_pe", c, 44100, S("GainPE", source=noise(c, N), gain=noise(c, N, 1.0)))
        add("MixPE", "two_trees", c, 44100,
            S("MixPE", inputs=[noise(c, N), S("GainPE", source=S("SinePE", frequency=330.0, channels=c), gain=0.25)]))
        add("MixPE", "cropped", c, 44100,
            S("MixPE", inputs=[S("CropPE", source=noise(c, N), start=-30, duration=900),
                               S("CropPE", source=noise(c, N), start=700, duration=8400)]))
        add("CropPE", "hold", c, 44100, S("CropPE", source=noise(c, N), start=-30, duration=9050, extend_mode="hold_both"))
        cache = dict(S("CachePE", source=noise(c, N)), share="c")
        add("CachePE", "twice", c, 44100, S("MixPE", inputs=[cache, S("GainPE", source=cache, gain=-0.5)]))
        add("DelayPE", "int", c, 44100, S("DelayPE", source=noise(c, N), delay=100))
        add("DelayPE", "linear", c, 44100, S("DelayPE", source=noise(c, N), delay=10.5, interpolation="linear"))
        add("DelayPE", "cubic", c, 44100, S("DelayPE", source=noise(c, N), delay=3.25, interpolation="cubic"))
        add("DelayPE", "pe_cubic", c, 44100,
            S("DelayPE", source=noise(c, N),
              delay=S("MixPE", inputs=[S("ConstantPE", value=100.0), S("SinePE", frequency=5.0, amplitude=50.0)]),
              interpolation="cubic"))
        add("LoopPE", "count_xfade", c, 48000,
            S("LoopPE", source=noise(c, 3000), loop_start=200, loop_end=2600, count=4, crossfade_seconds=0.01))
        for mode in ("max", "min", "mean", "rms"):
            for tag, window in (("w0", 0.0), ("w4ms", 0.004)):
                add("WindowPE", f"{mode}_{tag}", c, 44100,
                    S("WindowPE", source=noise(c, N), window=window, mode=mode, rectify=mode != "mean"))
                if tag == "w4ms":            # a 353-frame extremum can stand still over 64 frames: store the 257 too
                    out[-1]["budget"] = 340 * c
        add("TransformPE", "chain", c, 44100,
            S("TransformPE", source=noise(c, N, 0.7), ops=[["clip", 0.0, 1.0], ["sqrt"], ["affine", 2900.0, 100.0]]))
        add("TriggerRestartPE", "array", c, 44100, S("TriggerRestartPE", trigger=trig, src=noise(c, N)))
        add("SpatialPE", "linear", c, 44100, S("SpatialPE", source=noise(c, N), method="linear", azimuth=-35.0))
        add("SpatialPE", "constant_power", c, 44100,
            S("SpatialPE", source=noise(c, N), method="constant_power", azimuth=S("SinePE", frequency=0.7, amplitude=120.0)))
        add("SpatialPE", "hrtf", c, 44100, S("SpatialPE", source=noise(c, N), method="hrtf", azimuth=45.0))
    for a, b in ((3, 3), (8, 3), (3, 8)):
        add("SpatialPE", f"adapter_{a}_to_{b}", a, 44100, S("SpatialPE", source=noise(a, N), method="adapter", channels=b))

    # ------------------------------------------------------------------------------------------------ recurrences
    for c in CHAIN_C:
        for mode in ("lowpass", "highpass", "bandpass", "notch", "allpass", "peaking", "lowshelf", "highshelf"):
            long = 8193 if mode == "lowpass" else None
            add("BiquadPE", f"const_{mode}", c, 44100,
                S("BiquadPE", source=noise(c, _frames(blocks(long))), frequency=1500.0, q=1.3, mode=mode, gain_db=4.5),
                long=long)
        add("BiquadPE", "pe_cutoff", c, 48000,
            S("BiquadPE", source=noise(c, N), frequency=sweep, q=2.0, mode="peaking", gain_db=-6.0))
        add("SVFilterPE", "const", c, 44100,
            S("SVFilterPE", source=noise(c, N), frequency=1500.0, q=1.3, mode="bandpass", gain_db=4.5))
        add("SVFilterPE", "pe_cutoff", c, 48000,
            S("SVFilterPE", source=noise(c, N), frequency=sweep, q=0.9, mode="highshelf", gain_db=9.0))
        add("CombPE", "const", c, 48000, S("CombPE", source=noise(c, N), frequency=12000.0, feedback=0.7))
        add("CombPE", "pe_freq", c, 48000,
            S("CombPE", source=noise(c, _frames(blocks(12288))),
              frequency=S("MixPE", inputs=[S("ConstantPE", value=400.0), S("SinePE", frequency=3.0, amplitude=380.0)]),
              feedback=0.8, min_frequency=30.0, smoothing_samples=200), long=12288)
        add("EnvelopePE", "peak", c, 44100,
            S("EnvelopePE", source=noise(c, _frames(blocks(2049)), 0.6), attack=0.005, release=0.05, mode="peak"), long=2049)
        add("EnvelopePE", "rms_lookahead", c, 44100,
            S("EnvelopePE", source=noise(c, _frames(blocks(2049)), 0.6), attack=0.01, release=0.1, lookahead=0.004,
              mode="rms"), long=2049)
        add("LadderPE", "const", c, 48000,
            S("LadderPE", source=noise(c, N), frequency=1200.0, resonance=0.3, mode="lp24", drive=1.0, oversample=2))
        add("LadderPE", "pe_cutoff", c, 48000,
            S("LadderPE", source=noise(c, _frames(blocks(8192))),
              frequency=S("MixPE", inputs=[S("ConstantPE", value=2600.0), S("SinePE", frequency=2.0, amplitude=600.0)]),
              resonance=0.3, mode="bp12"), long=8192)
        add("CompressorPE", "peak_lookahead", c, 44100,
            S("CompressorPE", source=noise(c, N), threshold=-24.0, ratio=3.0, attack=0.005, release=0.05, knee=0.0,
              makeup_gain=2.0, lookahead=0.003, detection="peak"))
        add("CompressorPE", "default", c, 44100, S("CompressorPE", source=noise(c, N)))
        add("LimiterPE", "default", c, 44100, S("LimiterPE", source=noise(c, N), ceiling=-6.0))
        add("ExpanderPE", "soft", c, 44100,
            S("ExpanderPE", source=noise(c, N), threshold=-20.0, knee=6.0, gate_range=-40.0))
        for env_c in sorted({1, c} | ({2} if c == 3 else set())):
            for link in (True, False):
                add("DynamicsPE", f"env{env_c}_{'linked' if link else 'unlinked'}", c, 44100,
                    S("DynamicsPE", source=noise(c, N),
                      envelope=S("EnvelopePE", source=noise(env_c, N, 0.6), attack=0.002, release=0.02),
                      threshold=-18.0, ratio=4.0, knee=6.0, stereo_link=link))
        add("GainPE", "adsr_voice", c, 48000,
            S("GainPE", source=S("BiquadPE", source=S("BlitSawPE", frequency=98.0, channels=c), frequency=2000.0, q=0.707),
              gain=S("AdsrGatedPE", gate=S("PeriodicGate", frequency=11.0, duty_cycle=0.5), attack_time=0.01,
                     decay_time=0.02, sustain_level=0.7, release_time=0.02)), tiled=True)
    add("EnvelopePE", "peak_all_windows", 3, 44100,
        S("EnvelopePE", source=noise(3, 131500, 0.6), attack=0.005, release=0.05, mode="peak"),
        blks=[[-37, 300], [263, 131072], [131335, 64]])
    out[-1].update(pattern="long", long_index=1)

    # ------------------------------------------------------------------------------------------------ convolution
    conv_blocks = [[-37, 1], [-36, 17], [-19, 257], [238, 1000], [1238, 1199], [2700, 64]]       # the source ends at 3000
    for c in ELEMENTWISE_C:
        for tag, taps in (("direct", 129), ("fft", 2048)):
            for sc, fc in ((c, 1), (1, c), (c, c)):
                add("ConvolvePE", f"{tag}_{sc}x{fc}", c, 10000,
                    S("ConvolvePE", src=noise(sc, 3000, 1.0), fir=noise(fc, taps, 1.0, decay=taps / 6.0)),
                    blks=[list(b) for b in conv_blocks])
        add("ReverbPE", "mix_03", c, 10000,
            S("ReverbPE", source=noise(c, 3000), ir=noise(1, 300, 0.2, decay=60.0), mix=0.3, fft_size=1024),
            blks=[list(b) for b in conv_blocks])

    # ------------------------------------------------------------------------------------------------ streams, C = 3
    M = _frames(stream_blocks())
    for kind, graph in (
            ("BiquadPE", S("BiquadPE", source=noise(3, M), frequency=1500.0, q=1.3, mode="lowpass")),
            ("BiquadPE_pe", S("BiquadPE", source=noise(3, M), frequency=sweep, q=2.0, mode="peaking", gain_db=-6.0)),
            ("SVFilterPE", S("SVFilterPE", source=noise(3, M), frequency=sweep, q=0.9, mode="lowpass")),
            ("LadderPE", S("LadderPE", source=noise(3, M), frequency=1200.0, resonance=0.3)),
            ("CombPE", S("CombPE", source=noise(3, M), frequency=441.0, feedback=0.7)),
            ("EnvelopePE", S("EnvelopePE", source=noise(3, M, 0.6), attack=0.01, release=0.1, lookahead=0.004, mode="rms")),
            ("CompressorPE", S("CompressorPE", source=noise(3, M), lookahead=0.003, detection="peak")),
            ("BlitSawPE", S("BlitSawPE", frequency=110.0, amplitude=0.7, m=20, channels=3)),
            ("KarplusStrongPE", S("KarplusStrongPE", frequency=196.0, rho=0.998, amplitude=0.5, seed=7, channels=3)),
            ("WindowPE", S("WindowPE", source=noise(3, M), window=0.004, mode="mean", rectify=False)),
            ("DelayPE", S("DelayPE", source=noise(3, M), delay=3.25, interpolation="cubic"))):
        add(kind.split("_")[0], "pe" if kind.endswith("_pe") else "s", 3, 44100, graph, pattern="stream",
            tiled=kind in ("BlitSawPE", "KarplusStrongPE"))
    names = [c["name"] for c in out]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    return out


def is_source_case(case):
    """Built with `channels=C`: every column the same (the column swap proves nothing there)."""
    return case["tiled"]


def bank_cases():
    """MixPEs of 24 voices of one signature at C = 3 (the voice bank: [K][n][C] strides, chain / channels with
    batch > 1).  Checked against the oracle only."""
    def adsr(i):
        return S("AdsrGatedPE", gate=S("PeriodicGate", frequency=7.0 + 0.5 * i, duty_cycle=0.5), attack_time=0.01,
                 decay_time=0.02, sustain_level=0.7, release_time=0.02)

    voices = {
        "sine": lambda i: S("SinePE", frequency=110.0 * 2 ** (i / 12.0), amplitude=0.04, phase=0.1 * i, channels=3),
        "saw_biquad_adsr": lambda i: S("GainPE", source=S("BiquadPE", source=S("BlitSawPE", frequency=55.0 * 2 ** (i / 12.0),
                                                                              amplitude=0.1, channels=3),
                                                          frequency=2000.0, q=0.707), gain=adsr(i)),
        "ladder": lambda i: S("LadderPE", source=S("BlitSawPE", frequency=55.0 * 2 ** (i / 12.0), amplitude=0.1, channels=3),
                              frequency=1200.0, resonance=0.3, mode="lp24", drive=1.0, oversample=2),
    }
    return [{"name": f"bank24_{tag}_c3", "kind": "MixPE", "C": 3, "sr": 48000, "pattern": "blocks", "tiled": True,
             "long_index": None, "graph": S("MixPE", inputs=[make(i) for i in range(24)]),
             "blocks": [[0, 257], [257, 1000], [1257, 4099]]} for tag, make in voices.items()]


# ---------------------------------------------------------------------------------------------------- the comparison
def rel_tol(case, i):
    """test_gpu_parity.py's bar, 1e-5 of the block's peak; three times that on a stream pattern and from a long block
    on (as tests/test_gpu_fuzz_all.py: resonant stages multiply what their input is off by)."""
    from test_gpu_fuzz import REL_TOL
    long_at = case.get("long_index")
    return 3 * REL_TOL if case["pattern"] == "stream" or (long_at is not None and i >= long_at) else REL_TOL


def compare_block(case, i, got, want):
    """How the GPU test judges block `i` of a case: (accepted, err / (rel * peak + floor) -- 0 for a bit-exact case,
    message).  A graph of bit-exact kinds only (fuzz_graphs_all.bit_exact) must equal the expectation; any other is held
    to `rel_tol` of the expected block's peak plus test_gpu_parity.py's floor."""
    import numpy as np
    from fuzz_graphs_all import bit_exact
    from test_gpu_parity import ABS_FLOOR
    if got.dtype != np.float32 or got.shape != want.shape:
        return False, np.inf, f"{case['name']} block {i}: {got.dtype} {got.shape}, expected float32 {want.shape}"
    if bit_exact(case["graph"]):
        same = np.array_equal(got, want)
        return same, 0.0, "" if same else (f"{case['name']} block {i} (bit-exact graph): {int(np.count_nonzero(got != want))} "
                                           f"of {want.size} samples differ, max "
                                           f"{float(np.max(np.abs(got.astype(np.float64) - want))):.3e}")
    if not np.all(np.isfinite(got)):
        return False, np.inf, f"{case['name']} block {i}: non-finite output"
    peak = float(np.max(np.abs(want))) if want.size else 0.0
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) if want.size else 0.0
    bound = rel_tol(case, i) * peak + ABS_FLOOR
    return err <= bound, err / bound, f"{case['name']} block {i} {case['blocks'][i]}: max|d| {err:.3e} > {bound:.3e} (peak {peak:.3e})"
