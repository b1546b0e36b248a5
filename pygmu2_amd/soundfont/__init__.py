"""SoundFont (.sf2) host model and control plane behind MeltysynthPE: sf2.py reads the file, synth.py runs the voices
block by block and emits the render table that pgx_soundfont_render plays on the device."""

from .sf2 import Instrument, Preset, Region, SampleHeader, SoundFont, SoundFontError
from .synth import DCOLS, ICOLS, Channel, Synthesizer, Voice, mix_mode

__all__ = ["SoundFont", "SoundFontError", "SampleHeader", "Region", "Instrument", "Preset", "Synthesizer", "Channel",
           "Voice", "mix_mode", "ICOLS", "DCOLS"]
