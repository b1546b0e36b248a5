"""
pygmu2_amd -- MI355X-native render path for pygmu2-style audio graphs.

Same public names as the reference package for the accelerated hot path:
ProcessingElement / SourcePE / Snippet / Extent / Renderer / NullRenderer and the PEs
SinePE, BlitSawPE, SuperSawPE, BiquadPE, LadderPE, CombPE, MixPE, GainPE, ConvolvePE,
AdsrGatedPE, AdsrTriggeredPE, PeriodicGate, PeriodicTrigger, ConstantPE, ArrayPE,
DiracPE, IdentityPE, CachePE, CropPE, SVFilterPE, EnvelopePE, TransformPE, DelayPE, PiecewisePE,
TriggerRestartPE, ReverbPE, WavWriterPE, WavReaderPE, KarplusStrongPE, AnalogOscPE, WavetablePE, TimeWarpPE,
SampleHoldPE, TrackHoldPE, SlewLimiterPE, FunctionGenPE, NoisePE, TralfamPE, SlicePE, SetExtentPE, SequencePE,
ReversePitchEchoPE, PortamentoPE, ControlPE, MeltysynthPE
(+ render_to_file, rho_for_decay_db, pitch_to_freq and the other unit conversions).  Snippet payloads live in HBM; all DSP runs in
hand-written HIP kernels for gfx950 behind the C ABI of include/pygmu_hip.h.
"""

from .config import (ErrorMode, get_error_mode, get_sample_rate, handle_error, set_error_mode,
                     set_sample_rate)
from .extent import ExtendMode, Extent
from .snippet import Snippet
from .processing_element import ProcessingElement
from .source_pe import SourcePE
from .renderer import PEProfile, ProfileReport, Renderer
from .null_renderer import NullRenderer
from .gate_signal import GateSignal
from .trigger_signal import TriggerSignal
from .constant_pe import ConstantPE
from .identity_pe import IdentityPE
from .dirac_pe import DiracPE
from .array_pe import ArrayPE
from .cache_pe import CachePE
from .crop_pe import CropPE
from .sine_pe import SinePE
from .gain_pe import GainPE
from .mix_pe import MixPE
from .biquad_pe import BiquadMode, BiquadPE
from .blit_saw_pe import BlitSawPE
from .super_saw_pe import SuperSawPE
from .ladder_pe import LadderMode, LadderPE
from .comb_pe import CombPE
from .periodic_gate import PeriodicGate
from .periodic_trigger import PeriodicTrigger
from .adsr_pe import AdsrGatedPE, AdsrTriggeredPE
from .convolve_pe import ConvolvePE
from .svfilter_pe import SVFilterPE
from .envelope_pe import DetectionMode, EnvelopePE
from .transform_pe import TransformPE
from . import transforms
from .delay_pe import DelayPE, InterpolationMode
from .piecewise_pe import PiecewisePE, TransitionType
from .trigger_restart_pe import TriggerRestartPE
from .reverb_pe import ReverbPE
from .spatial_pe import (SpatialAdapter, SpatialConstantPower, SpatialHRTF, SpatialLinear, SpatialMethod,
                         SpatialPE)
from .loop_pe import LoopPE
from .window_pe import WindowMode, WindowPE
from .dynamics_pe import DynamicsMode, DynamicsPE, db_to_ratio, ratio_to_db
from .compressor_pe import CompressorPE, ExpanderPE, LimiterPE
from .wav_writer_pe import WavWriterPE
from .wav_reader_pe import WavReaderPE
from .karplus_strong_pe import KarplusStrongPE, rho_for_decay_db
from .analog_osc_pe import AnalogOscPE
# WavetablePE and TimeWarpPE are bound here (pg.WavetablePE works) but are NOT in __all__ yet: every PE named there
# must have fuzz-corpus cases and a graph-oracle evaluator under oracle/ (tests/test_oracle_fuzz_golden.py), and those
# arrive with the change that enters the two classes into that census.  tests/test_gpu_playback_fuzz.py stands in.
from .wavetable_pe import OutOfBoundsMode, WavetablePE
from .timewarp_pe import TimeWarpPE
# The control-signal PEs: the same arrangement -- bound here (pg.SampleHoldPE, pg.TrackHoldPE, pg.SlewLimiterPE, pg.SlewMode,
# pg.FunctionGenPE work) but NOT in __all__ until they have fuzz-corpus cases and evaluators under oracle/;
# tests/test_gpu_control_fuzz.py stands in.
from .sample_hold_pe import SampleHoldPE
from .track_hold_pe import TrackHoldPE
from .slew_limiter_pe import SlewLimiterPE, SlewMode
from .function_gen_pe import FunctionGenPE
# NoisePE / NoiseMode: again the same arrangement (pg.NoisePE, pg.NoiseMode work, neither is in __all__);
# tests/test_gpu_noise_fuzz.py stands in for the census.
from .noise_pe import NoiseMode, NoisePE
# TralfamPE, SlicePE, SetExtentPE and the `spectral` module (the arbitrary-length DFT behind TralfamPE): the same
# arrangement once more (pg.TralfamPE, pg.SlicePE, pg.SetExtentPE work, none is in __all__); tests/test_gpu_tralfam.py
# renders them against fixtures of the reference.
from .set_extent_pe import SetExtentPE
from .slice_pe import SlicePE
from .tralfam_pe import TralfamPE
from . import spectral
# SequencePE / SequenceMode and the unit conversions: the same arrangement (pg.SequencePE, pg.SequenceMode,
# pg.pitch_to_freq ... work, none is in __all__); tests/test_gpu_score.py renders scores against fixtures of the
# reference.  score_bank is what MixPE renders such scores through.
from .sequence_pe import SequenceMode, SequencePE
from .conversions import (freq_to_pitch, pitch_to_freq, ratio_to_semitones, samples_to_seconds, seconds_to_samples,
                          semitones_to_ratio)
from . import score_bank
# The temperaments and the global tuning: the same arrangement (pg.JustIntonation, pg.set_temperament ... work, none is
# in __all__); tests/test_tuning_host.py and tests/test_gpu_tuning.py hold them to fixtures of the reference.
from . import temperament
from .temperament import (CustomTemperament, EqualTemperament, JustIntonation, PythagoreanTuning, Temperament,
                          get_reference_frequency, get_temperament, set_baroque_pitch, set_concert_pitch,
                          set_reference_frequency, set_temperament, set_verdi_tuning)
# RandomSelectPE and the restart bank it and TriggerRestartPE render through: the same arrangement (pg.RandomSelectPE and
# pg.restart_bank work, neither is in __all__): the fuzz census of tests/test_oracle_fuzz_golden.py needs an evaluator
# under oracle/ for every name listed there; tests/test_gpu_random_select.py holds it to fixtures of the reference.
from . import restart_bank
from .random_select_pe import RandomSelectPE
# ReversePitchEchoPE: the same arrangement (pg.ReversePitchEchoPE works, it is not in __all__): the fuzz census of
# tests/test_oracle_fuzz_golden.py needs an evaluator under oracle/ for every name listed there;
# tests/test_gpu_reverse_echo.py holds it to fixtures of the reference.
from .reverse_pitch_echo_pe import ReversePitchEchoPE
# PortamentoPE and ControlPE: the same arrangement (pg.PortamentoPE and pg.ControlPE work, neither is in __all__): the
# fuzz census of tests/test_oracle_fuzz_golden.py needs an evaluator under oracle/ for every name listed there;
# tests/test_portamento_host.py and tests/test_portamento_gpu.py hold the glide line to fixtures of the reference,
# tests/test_stream_control_pe.py the control.
from .portamento_pe import PortamentoPE
from .control_pe import ControlPE
# MeltysynthPE and the `soundfont` package (the SF2 reader and the synthesizer's control plane): the same arrangement
# (pg.MeltysynthPE and pg.soundfont work, neither is in __all__): the fuzz census of tests/test_oracle_fuzz_golden.py
# needs an evaluator under oracle/ for every name listed there; tests/test_soundfont_host.py holds the reader and the
# control plane, tests/test_zzz_gpu_soundfont.py the device, to fixtures of the reference.
from . import soundfont
from .meltysynth_pe import MeltysynthPE
from .utils import render_to_file
from . import device, diagnostics

__all__ = [
    "ErrorMode", "get_error_mode", "get_sample_rate", "handle_error", "set_error_mode", "set_sample_rate",
    "ExtendMode", "Extent", "Snippet", "ProcessingElement", "SourcePE", "PEProfile", "ProfileReport",
    "Renderer", "NullRenderer", "GateSignal", "TriggerSignal", "ConstantPE", "IdentityPE", "DiracPE",
    "ArrayPE", "CachePE", "CropPE", "SinePE", "GainPE", "MixPE", "BiquadMode", "BiquadPE", "BlitSawPE",
    "SuperSawPE", "LadderMode", "LadderPE", "CombPE", "PeriodicGate", "PeriodicTrigger", "AdsrGatedPE",
    "AdsrTriggeredPE", "ConvolvePE", "SVFilterPE", "DetectionMode", "EnvelopePE", "TransformPE",
    "transforms", "DelayPE", "InterpolationMode", "PiecewisePE", "TransitionType", "TriggerRestartPE",
    "ReverbPE", "SpatialPE", "SpatialMethod", "SpatialAdapter", "SpatialLinear", "SpatialConstantPower",
    "SpatialHRTF", "LoopPE", "WindowMode", "WindowPE", "DynamicsMode", "DynamicsPE", "CompressorPE", "LimiterPE",
    "ExpanderPE", "db_to_ratio", "ratio_to_db", "WavWriterPE", "WavReaderPE", "render_to_file", "device", "diagnostics",
    "KarplusStrongPE", "rho_for_decay_db", "AnalogOscPE", "OutOfBoundsMode",
]
