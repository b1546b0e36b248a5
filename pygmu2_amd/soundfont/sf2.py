"""
SoundFont 2 reader: RIFF `sfbk` with its three lists -- INFO, sdta (the 16-bit `smpl` chunk; `sm24` is skipped) and pdta
(phdr, pbag, pgen, inst, ibag, igen, shdr; pmod and imod are skipped) -- into presets, instruments, regions and sample
headers, the way the reference's meltysynth port reads them (meltysynth/model/).

A region is a 61-slot generator table: the defaults, then the global zone's generators, then the local zone's.  A zone
list starts with a global zone when its first zone is empty or does not end in the terminal generator (sampleID for an
instrument, instrument for a preset).  The sample data stays int16 (`wave`): s / 32768 is exact in float32 and in
float64, so the device widens it itself.

Every malformed file raises SoundFontError (a ValueError).
"""

from __future__ import annotations

import struct

import numpy as np

GEN_COUNT = 61
# generator numbers this package reads by name
G_START_OFS, G_END_OFS, G_STARTLOOP_OFS, G_ENDLOOP_OFS, G_START_COARSE = 0, 1, 2, 3, 4
G_MODLFO_PITCH, G_VIBLFO_PITCH, G_MODENV_PITCH, G_CUTOFF, G_Q, G_MODLFO_CUTOFF, G_MODENV_CUTOFF = 5, 6, 7, 8, 9, 10, 11
G_END_COARSE, G_MODLFO_VOLUME, G_CHORUS, G_REVERB, G_PAN = 12, 13, 15, 16, 17
G_MODLFO_DELAY, G_MODLFO_FREQ, G_VIBLFO_DELAY, G_VIBLFO_FREQ = 21, 22, 23, 24
G_MODENV_DELAY, G_MODENV_ATTACK, G_MODENV_HOLD, G_MODENV_DECAY, G_MODENV_SUSTAIN, G_MODENV_RELEASE = 25, 26, 27, 28, 29, 30
G_MODENV_KEY_HOLD, G_MODENV_KEY_DECAY = 31, 32
G_VOLENV_DELAY, G_VOLENV_ATTACK, G_VOLENV_HOLD, G_VOLENV_DECAY, G_VOLENV_SUSTAIN, G_VOLENV_RELEASE = 33, 34, 35, 36, 37, 38
G_VOLENV_KEY_HOLD, G_VOLENV_KEY_DECAY, G_INSTRUMENT, G_KEY_RANGE, G_VEL_RANGE = 39, 40, 41, 43, 44
G_STARTLOOP_COARSE, G_KEY_NUMBER, G_VELOCITY, G_ATTENUATION, G_ENDLOOP_COARSE = 45, 46, 47, 48, 50
G_COARSE_TUNE, G_FINE_TUNE, G_SAMPLE_ID, G_SAMPLE_MODES, G_SCALE_TUNING, G_EXCLUSIVE_CLASS, G_ROOT_KEY = 51, 52, 53, 54, 56, 57, 58

_INSTRUMENT_DEFAULTS = {G_CUTOFF: 13500, G_MODLFO_DELAY: -12000, G_VIBLFO_DELAY: -12000, G_MODENV_DELAY: -12000,
                        G_MODENV_ATTACK: -12000, G_MODENV_HOLD: -12000, G_MODENV_DECAY: -12000,
                        G_MODENV_RELEASE: -12000, G_VOLENV_DELAY: -12000, G_VOLENV_ATTACK: -12000,
                        G_VOLENV_HOLD: -12000, G_VOLENV_DECAY: -12000, G_VOLENV_RELEASE: -12000, G_KEY_RANGE: 0x7F00,
                        G_VEL_RANGE: 0x7F00, G_KEY_NUMBER: -1, G_VELOCITY: -1, G_SCALE_TUNING: 100, G_ROOT_KEY: -1}
_PRESET_DEFAULTS = {G_KEY_RANGE: 0x7F00, G_VEL_RANGE: 0x7F00}
_INFO_TEXT = {"isng": "target_sound_engine", "INAM": "bank_name", "irom": "rom_name", "ICRD": "creation_date",
              "IENG": "author", "IPRD": "target_product", "ICOP": "copyright", "ICMT": "comments", "ISFT": "tools"}
_SAMPLE_TYPES = {0, 1, 2, 4, 8, 0x8001, 0x8002, 0x8004, 0x8008}


class SoundFontError(ValueError):
    pass


class _Reader:
    def __init__(self, data: bytes):
        self.data, self.pos = data, 0

    def take(self, n: int) -> bytes:
        if n < 0 or self.pos + n > len(self.data):
            raise SoundFontError(f"the file ends inside a chunk (byte {self.pos}, {n} more wanted)")
        out = self.data[self.pos:self.pos + n]
        self.pos += n
        return out

    def unpack(self, fmt: str):
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt)))

    def four_cc(self) -> str:
        return "".join(chr(b) if 32 <= b <= 126 else "?" for b in self.take(4))

    def u32(self) -> int:
        return self.unpack("I")[0]


def _text(raw: bytes) -> str:
    try:
        return raw.split(b"\0", 1)[0].decode("ascii")
    except UnicodeDecodeError:
        raise SoundFontError("a name is not ASCII") from None


def _open_list(r: _Reader, kind: str) -> int:
    if r.four_cc() != "LIST":
        raise SoundFontError(f"the LIST chunk of '{kind}' was not found")
    end = r.u32()
    end += r.pos
    got = r.four_cc()
    if got != kind:
        raise SoundFontError(f"the type of the LIST chunk must be '{kind}', but was '{got}'")
    return end


class SampleHeader:
    __slots__ = ("name", "start", "end", "start_loop", "end_loop", "sample_rate", "original_pitch", "pitch_correction",
                 "link", "sample_type")

    def __init__(self, raw: bytes):
        self.name = _text(raw[:20])
        (self.start, self.end, self.start_loop, self.end_loop, self.sample_rate, self.original_pitch,
         self.pitch_correction, self.link, self.sample_type) = struct.unpack("<iiiiiBbHH", raw[20:46])
        if self.sample_type not in _SAMPLE_TYPES:
            raise SoundFontError(f"the sample '{self.name}' has the unknown type {self.sample_type}")


class Region:
    """One zone of a preset (`.instrument`) or of an instrument (`.sample`) over its global zone: `gs`, 61 integers."""
    __slots__ = ("gs", "instrument", "sample")

    def __init__(self, defaults, global_zone, local_zone):
        gs = [0] * GEN_COUNT
        for k, v in defaults.items():
            gs[k] = v
        for kind, value in global_zone + local_zone:
            gs[kind] = value
        self.gs, self.instrument, self.sample = gs, None, None

    def contains(self, key: int, velocity: int) -> bool:
        kr, vr = self.gs[G_KEY_RANGE], self.gs[G_VEL_RANGE]
        return (kr & 0xFF) <= key <= ((kr >> 8) & 0xFF) and (vr & 0xFF) <= velocity <= ((vr >> 8) & 0xFF)


class Instrument:
    __slots__ = ("name", "regions")


class Preset:
    __slots__ = ("name", "patch_number", "bank_number", "library", "genre", "morphology", "regions")


def _records(r: _Reader, size: int, width: int, what: str):
    if size % width:
        raise SoundFontError(f"the {what} list is invalid")
    return [r.take(width) for _ in range(size // width)]


def _generators(r, size):
    out = []
    for raw in _records(r, size, 4, "generator"):
        kind, value = struct.unpack("<Hh", raw)
        if kind >= GEN_COUNT:
            raise SoundFontError(f"{kind} is not a generator")
        out.append((kind, value))
    return out[:-1]                                     # the last record is the terminator


def _zones(bags, generators):
    """pbag / ibag records -> one generator list per zone (the last bag only closes the one before it)."""
    if len(bags) <= 1:
        raise SoundFontError("no valid zone was found")
    starts = [struct.unpack("<HH", raw)[0] for raw in bags]
    zones = []
    for first, nxt in zip(starts, starts[1:]):
        if nxt < first or nxt > len(generators):
            raise SoundFontError("a zone points outside the generator list")
        zones.append(generators[first:nxt])
    return zones


def _regions(owner: str, zones, first: int, nxt: int, defaults, terminal: int):
    if nxt - first <= 0:
        raise SoundFontError(f"'{owner}' has no zone")
    span = zones[first:nxt]
    if not span:
        raise SoundFontError(f"'{owner}' points outside the zone list")
    if not span[0] or span[0][-1][0] != terminal:
        return [Region(defaults, span[0], z) for z in span[1:]]
    return [Region(defaults, [], z) for z in span]


class SoundFont:
    """`info` (dict), `wave` (int16 numpy array), `sample_headers`, `instruments`, `presets`."""

    def __init__(self, data: bytes):
        r = _Reader(bytes(data))
        if r.four_cc() != "RIFF":
            raise SoundFontError("the RIFF chunk was not found")
        r.u32()
        form = r.four_cc()
        if form != "sfbk":
            raise SoundFontError(f"the type of the RIFF chunk must be 'sfbk', but was '{form}'")
        self.info = self._read_info(r)
        self.wave = self._read_samples(r)
        self.bits_per_sample = 16
        self._read_parameters(r)

    @classmethod
    def from_file(cls, path: str) -> "SoundFont":
        with open(path, "rb") as f:
            return cls(f.read())

    @property
    def wave_data(self) -> np.ndarray:
        """The samples as the reference holds them: float64 of s / 32768."""
        return self.wave.astype(np.float64) * (1.0 / 32768.0)

    @staticmethod
    def _read_info(r):
        info = {"version": (0, 0), "rom_version": (0, 0), **{v: "" for v in _INFO_TEXT.values()}}
        end = _open_list(r, "INFO")
        while r.pos < end:
            sub, size = r.four_cc(), r.u32()
            if sub in ("ifil", "iver"):
                info["version" if sub == "ifil" else "rom_version"] = r.unpack("HH")
            elif sub in _INFO_TEXT:
                info[_INFO_TEXT[sub]] = _text(r.take(size))
            else:
                raise SoundFontError(f"the INFO list contains an unknown ID '{sub}'")
        return info

    @staticmethod
    def _read_samples(r):
        end = _open_list(r, "sdta")
        wave = None
        while r.pos < end:
            sub, size = r.four_cc(), r.u32()
            if sub == "smpl":
                wave = np.frombuffer(r.take(size // 2 * 2), dtype="<i2").astype(np.int16)
            elif sub == "sm24":
                r.take(size)
            else:
                raise SoundFontError(f"the sdta list contains an unknown ID '{sub}'")
        if wave is None:
            raise SoundFontError("no valid sample data was found")
        return wave

    def _read_parameters(self, r):
        end = _open_list(r, "pdta")
        chunks = {}
        while r.pos < end:
            sub, size = r.four_cc(), r.u32()
            if sub in ("pmod", "imod"):
                r.take(size)
            elif sub in ("pgen", "igen"):
                chunks[sub] = _generators(r, size)
            elif sub in ("phdr", "pbag", "inst", "ibag", "shdr"):
                width = {"phdr": 38, "pbag": 4, "inst": 22, "ibag": 4, "shdr": 46}[sub]
                chunks[sub] = _records(r, size, width, sub)
            else:
                raise SoundFontError(f"the pdta list contains an unknown ID '{sub}'")
        for sub in ("phdr", "pbag", "pgen", "inst", "ibag", "igen", "shdr"):
            if sub not in chunks:
                raise SoundFontError(f"the {sub.upper()} sub-chunk was not found")

        self.sample_headers = [SampleHeader(raw) for raw in chunks["shdr"]][:-1]

        zones = _zones(chunks["ibag"], chunks["igen"])
        heads = [(_text(raw[:20]), struct.unpack("<H", raw[20:22])[0]) for raw in chunks["inst"]]
        if len(heads) <= 1:
            raise SoundFontError("no valid instrument was found")
        self.instruments = []
        for (name, first), (_, nxt) in zip(heads, heads[1:]):
            inst = Instrument()
            inst.name = name
            inst.regions = _regions(name, zones, first, nxt, _INSTRUMENT_DEFAULTS, G_SAMPLE_ID)
            for region in inst.regions:
                sid = region.gs[G_SAMPLE_ID]
                if not 0 <= sid < len(self.sample_headers):
                    raise SoundFontError(f"the instrument '{name}' contains an invalid sample ID '{sid}'")
                region.sample = self.sample_headers[sid]
            self.instruments.append(inst)

        zones = _zones(chunks["pbag"], chunks["pgen"])
        heads = [(_text(raw[:20]),) + struct.unpack("<HHHiii", raw[20:38]) for raw in chunks["phdr"]]
        if len(heads) <= 1:
            raise SoundFontError("no valid preset was found")
        self.presets = []
        for head, nxt in zip(heads, heads[1:]):
            p = Preset()
            p.name, p.patch_number, p.bank_number, first, p.library, p.genre, p.morphology = head
            p.regions = _regions(p.name, zones, first, nxt[3], _PRESET_DEFAULTS, G_INSTRUMENT)
            for region in p.regions:
                iid = region.gs[G_INSTRUMENT]
                if not 0 <= iid < len(self.instruments):
                    raise SoundFontError(f"the preset '{p.name}' contains an invalid instrument ID '{iid}'")
                region.instrument = self.instruments[iid]
            self.presets.append(p)
