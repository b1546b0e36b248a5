"""The audio plane of MeltysynthPE restated in numpy float64: what pgx_soundfont_render computes from a render table
(include/pygmu_hip.h lays the table out), and what the reference's Oscillator._fill_block_*_np, BiQuadFilter.process and
Synthesizer._write_block compute from the same numbers.  tools/gen_golden_soundfont.py refuses to write its fixtures
unless this restatement, fed with the table it recorded from the reference, reproduces the reference's samples bit for
bit; tests/test_zzz_gpu_soundfont.py uses it as the reference for hand-made tables.  Also the fixture loaders."""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SF2_PATH = os.path.join(GOLDEN, "soundfont_tiny.sf2")

ICOLS, DCOLS = 8, 11
I_VOICE, I_FLAGS, I_END, I_START_LOOP, I_END_LOOP, I_MIX_L, I_MIX_R = range(7)
D_POSITION, D_RATIO, D_A0, D_MIX_L, D_MIX_R = 0, 1, 2, 7, 9
F_CLEAR, F_LOOP, F_FILTER = 1, 2, 4
MIX_SKIP, MIX_CONST, MIX_SLOPE = 0, 1, 2


def load_cases():
    with open(os.path.join(GOLDEN, "soundfont_cases.json")) as f:
        return json.load(f)


def load_data():
    return np.load(os.path.join(GOLDEN, "soundfont.npz"))


def session_table(data, name):
    return data[f"{name}/block_rows"], data[f"{name}/rows_i"], data[f"{name}/rows_d"]


def requests_of(session):
    return [step[1] for step in session["steps"] if step[0] == "render"]


def mix_mode(previous_gain, current_gain, inverse_block_size):
    """Synthesizer._write_block's rule for one side of one voice: (mode, a, b)."""
    if max(previous_gain, current_gain) < 1.0e-3:
        return MIX_SKIP, 0.0, 0.0
    if abs(current_gain - previous_gain) < 1.0e-3:
        return MIX_CONST, float(current_gain), 0.0
    return MIX_SLOPE, float(previous_gain), inverse_block_size * (current_gain - previous_gain)


class AudioPlane:
    def __init__(self, wave_i16, block_size, polyphony):
        self.data = np.asarray(wave_i16).astype(np.float64) * (1.0 / 32768.0)
        self.block_size = int(block_size)
        self.state = np.zeros((polyphony, 4))            # x1, x2, y1, y2

    def _gather(self, index):
        index = np.asarray(index, dtype=np.int64)
        inside = (index >= 0) & (index < len(self.data))
        out = np.zeros(index.shape)
        out[inside] = self.data[index[inside]]
        return out

    def oscillator(self, ri, rd):
        n = self.block_size
        positions = rd[D_POSITION] + np.arange(n, dtype=np.float64) * rd[D_RATIO]
        if ri[I_FLAGS] & F_LOOP:
            start_loop, end_loop = int(ri[I_START_LOOP]), int(ri[I_END_LOOP])
            with np.errstate(all="ignore"):
                wrapped = (positions - start_loop) % float(end_loop - start_loop) + start_loop
            lo = wrapped.astype(np.int64)
            frac = wrapped - lo
            hi = np.where(lo + 1 >= end_loop, start_loop, lo + 1)
            return (1 - frac) * self._gather(lo) + frac * self._gather(hi)
        out = np.zeros(n)
        live = positions < int(ri[I_END])
        lo = positions[live].astype(np.int64)
        frac = positions[live] - lo
        out[live] = (1 - frac) * self._gather(lo) + frac * self._gather(lo + 1)
        return out

    def filter(self, ri, rd, block):
        state = self.state[ri[I_VOICE]]
        if ri[I_FLAGS] & F_CLEAR:
            state[:] = 0.0
        if not ri[I_FLAGS] & F_FILTER:
            state[:] = (block[-1], block[-2], block[-1], block[-2])
            return block
        a0, a1, a2, a3, a4 = (float(v) for v in rd[D_A0:D_A0 + 5])
        x1, x2, y1, y2 = (float(v) for v in state)
        out = np.empty(len(block))
        for t, x in enumerate(block.tolist()):
            y = a0 * x + a1 * x1 + a2 * x2 - a3 * y1 - a4 * y2
            x2, x1, y2, y1 = x1, x, y1, y
            out[t] = y
        state[:] = (x1, x2, y1, y2)
        return out

    def render(self, block_rows, rows_i, rows_d):
        """-> (n_blocks * block_size, 2) float64, before the rounding to float32."""
        n = self.block_size
        ramp = np.arange(n, dtype=np.float64)
        out = np.zeros((n * (len(block_rows) - 1), 2))
        for b in range(len(block_rows) - 1):
            dest = out[b * n:(b + 1) * n]
            for r in range(block_rows[b], block_rows[b + 1]):
                ri, rd = rows_i[r], rows_d[r]
                block = self.filter(ri, rd, self.oscillator(ri, rd))
                for side, mode_col, gain_col in ((0, I_MIX_L, D_MIX_L), (1, I_MIX_R, D_MIX_R)):
                    if ri[mode_col] == MIX_CONST:
                        dest[:, side] += rd[gain_col] * block
                    elif ri[mode_col] == MIX_SLOPE:
                        dest[:, side] += (rd[gain_col] + rd[gain_col + 1] * ramp) * block
        return out


def replay(session, synthesizer, render):
    """Play a session's steps: events and attribute writes on `synthesizer`, render(frames) per request -> the list of
    what the render calls returned and the active voice count after each."""
    pieces, active = [], []
    for step in session["steps"]:
        if step[0] == "ev":
            getattr(synthesizer, step[1])(*step[2])
        elif step[0] == "set":
            setattr(synthesizer, step[1], step[2])
        else:
            pieces.append(render(step[1]))
            active.append(int(synthesizer.active_voice_count))
    return pieces, active


def join_tables(tables):
    """Tables of consecutive advance() calls -> one table."""
    offsets, base = [np.zeros(1, dtype=np.int32)], 0
    for block_rows, _, _ in tables:
        offsets.append(block_rows[1:] + base)
        base += int(block_rows[-1])
    return (np.concatenate(offsets).astype(np.int32),
            np.concatenate([t[1].reshape(-1, ICOLS) for t in tables]) if tables else np.zeros((0, ICOLS), np.int32),
            np.concatenate([t[2].reshape(-1, DCOLS) for t in tables]) if tables else np.zeros((0, DCOLS)))


def table_difference(got, want):
    """None, or the first place where two tables differ (every integer equal, every double bit for bit)."""
    for name, g, w in zip(("block_rows", "rows_i", "rows_d"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{name}: shape {g.shape} != {w.shape}"
        same = g == w if g.dtype.kind == "i" else g.view(np.uint64) == w.view(np.uint64)
        if not np.all(same):
            at = tuple(int(v) for v in np.argwhere(~same)[0])
            return f"{name}{list(at)}: {g[at]!r} != {w[at]!r} ({int(np.sum(~same))} entries differ)"
    return None


def requests_over_blocks(session, blocks):
    """The session's requests cut from `blocks` (frames of whole blocks, in order) the way Synthesizer.render walks its
    block grid: a request takes what the last block left over first; reset() drops the rest of the block."""
    bs = session["block_size"]
    got, read, b = [blocks[:0]], bs, -1
    for step in session["steps"]:
        if step[0] == "ev" and step[1] == "reset":
            read = bs
        if step[0] != "render":
            continue
        need = step[1]
        while need:
            if read == bs:
                b, read = b + 1, 0
            take = min(bs - read, need)
            got.append(blocks[b * bs + read:b * bs + read + take])
            read, need = read + take, need - take
    return np.concatenate(got)
