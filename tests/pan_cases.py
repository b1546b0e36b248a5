"""The panned-voice graphs of tests/test_pan_bank_trace.py, tests/test_gpu_panned_voices.py and
tools/gen_golden_panned_mix.py, as SPECs (oracle/golden_cases.py's format): one place, so that the trace, the twin
renders and the reference fixture are about the same voices."""

from oracle.golden_cases import S

SR = 48000
K = 5
# scalar azimuths, voice i takes AZIMUTHS[i % 9] (+ 7 degrees per round): inside the field, on its ends, clipped on both
# sides, both zeros
AZIMUTHS = (-35.5, 45.0, -135.0, 200.0, 0.0, 90.0, -90.0, -0.0, 90.0001)


def azimuth(i):
    return AZIMUTHS[i % len(AZIMUTHS)] + 7.0 * (i // len(AZIMUTHS))


def sine(i, channels=1):
    return S("SinePE", frequency=220.0 + 37.0 * i, amplitude=0.2, channels=channels)


def lfo(i):
    """An azimuth that swings past +-90 within a few blocks of 1 024 frames, every voice somewhere else."""
    return S("SinePE", frequency=3.0 + 0.5 * i, amplitude=120.0, phase=0.7 * i)


def saw_lowpass(i):
    return S("BiquadPE", source=S("BlitSawPE", frequency=110.0 * 2 ** (i / 12.0)), frequency=2000.0, q=0.707)


def readme_voice(i):
    """README.md's voice (BASELINE config 5): BlitSaw -> Biquad LP 2 kHz -> x ADSR(PeriodicGate)."""
    return S("GainPE",
             source=S("BiquadPE", source=S("BlitSawPE", frequency=27.5 * 2 ** ((60 * i) / 48.0)), frequency=2000.0,
                      q=0.707),
             gain=S("AdsrGatedPE", gate=S("PeriodicGate", frequency=2.0 + 0.01 * i, duty_cycle=0.5),
                    attack_time=0.01, decay_time=0.1, sustain_level=0.7, release_time=0.2))


def pan(source, method, az):
    return S("SpatialPE", source=source, method=method, azimuth=az)


def voice(kind, i):
    if kind == "scalar":
        return pan(sine(i), "constant_power", azimuth(i))
    if kind == "lfo":
        return pan(saw_lowpass(i), "linear", lfo(i))
    if kind == "readme":
        return pan(readme_voice(i), "constant_power", azimuth(i))
    if kind == "nested":
        return S("GainPE", source=pan(sine(i), "constant_power", azimuth(i)), gain=0.5)
    if kind == "three_channel":
        return pan(sine(i, 3), "linear", azimuth(i))
    if kind == "adapt_up":
        return S("SpatialPE", source=sine(i), method="adapter", channels=2)
    if kind == "adapt_down":
        return S("SpatialPE", source=sine(i, 3), method="adapter", channels=1)
    raise KeyError(kind)


# kind -> the class of the bank's root node (voice_bank)
ROOTS = {"scalar": "_PanNode", "lfo": "_PanNode", "readme": "_PanNode", "nested": "_GainNode",
         "three_channel": "_PanNode", "adapt_up": "_AdaptNode", "adapt_down": "_AdaptNode"}


def mix(kind, count=K):
    return S("MixPE", inputs=[voice(kind, i) for i in range(count)])


def declined(kind):
    """Five voices that are no bank, each for one reason (voice_bank's keying rules)."""
    if kind == "hrtf":
        inputs = [S("SpatialPE", source=sine(i), method="hrtf", azimuth=az)
                  for i, az in enumerate((-90.0, -45.0, 30.0, 45.0, 90.0))]
    elif kind == "mixed_methods":
        inputs = [pan(sine(i), "linear" if i == 2 else "constant_power", azimuth(i)) for i in range(K)]
    elif kind == "scalar_and_pe":
        inputs = [pan(sine(i), "linear", lfo(i) if i == 3 else azimuth(i)) for i in range(K)]
    elif kind == "stereo_azimuth":
        inputs = [pan(sine(i), "linear", dict(lfo(i), channels=2)) for i in range(K)]
    elif kind == "shared_azimuth":
        inputs = [pan(sine(i), "linear", dict(lfo(0), share="lfo0") if i in (0, 4) else lfo(i)) for i in range(K)]
    else:
        raise KeyError(kind)
    return S("MixPE", inputs=inputs)


DECLINED = ("hrtf", "mixed_methods", "scalar_and_pe", "stereo_azimuth", "shared_azimuth")
