"""The modulated-sine graphs of tests/test_gpu_fm_voices.py and tools/gen_golden_fm_voices.py, as SPECs
(oracle/golden_cases.py's format): one place, so that the twin renders and the reference fixture are about the same voices.

    fm       SinePE(frequency=TransformPE(SinePE(m_i), Affine(d_i, c_i)), amplitude=a_i)       two-operator FM
    am_pm    SinePE(c_i, amplitude=TransformPE(SinePE(r_i), Affine(0.1, 0.15)),                 tremolo and phase modulation:
                    phase=TransformPE(SinePE(m_i), Affine(b_i, 0)))                              a phase in play
    nested   SinePE(frequency=TransformPE(<an fm voice>, Affine(D_i, C_i)))                     a modulator that is a modulated sine
    bell     GainPE(<fm voice>, gain=AdsrTriggeredPE(PeriodicTrigger(r_i), ...))                the bank as a level

Modulation indices (deviation / modulator frequency) stay below 2: the phase of a voice is then a few thousand radians at
the end of a fixture case, where float64 and the reference's float32 control streams still agree to the fixture's rule."""

from oracle.golden_cases import S

SR = 48000
K = 5
KINDS = ("fm", "am_pm", "nested", "bell")
# kind -> the class of the bank's root node (voice_bank)
ROOTS = {"fm": "_SineModNode", "am_pm": "_SineModNode", "nested": "_SineModNode", "bell": "_GainNode"}


def affine(source, scale, offset):
    return S("TransformPE", source=source, ops=[["affine", scale, offset]])


def carrier(i):
    return 220.0 * 2 ** ((3 * i) / 12.0)


def fm_voice(i, amplitude=None):
    """Carrier c_i, modulator 1.5 c_i (+ a detune), deviation 0.8 .. 1.2 times the modulator's frequency."""
    c = carrier(i)
    m = 1.5 * c + 0.7 * i
    return S("SinePE", frequency=affine(S("SinePE", frequency=m), (0.8 + 0.1 * i) * m, c),
             amplitude=0.15 + 0.01 * i if amplitude is None else amplitude)


def voice(kind, i):
    if kind == "fm":
        return fm_voice(i)
    if kind == "am_pm":
        c = carrier(i)
        return S("SinePE", frequency=c, amplitude=affine(S("SinePE", frequency=3.0 + 0.5 * i), 0.1, 0.15),
                 phase=affine(S("SinePE", frequency=2.0 * c + 1.0), 1.0 + 0.2 * i, 0.0))
    if kind == "nested":
        c = 110.0 * 2 ** ((2 * i) / 12.0)
        return S("SinePE", frequency=affine(fm_voice(i, amplitude=1.0), 0.5 * c, c), amplitude=0.18)
    if kind == "bell":
        return S("GainPE", source=fm_voice(i),
                 gain=S("AdsrTriggeredPE", trigger=S("PeriodicTrigger", hz=6.0 + 1.5 * i), attack_time=0.002, decay_time=0.05,
                        sustain_time=0.01, sustain_level=0.4, release_time=0.04))
    raise KeyError(kind)


def mix(kind, count=K):
    return S("MixPE", inputs=[voice(kind, i) for i in range(count)])
