"""NoisePE on the CPU, twice over, shared by the fixture generator (tools/gen_golden_noise.py, over the reference's
classes) and the tests (over pygmu2_amd's).

(a) The numpy restatement (`NoiseStream`): the reference's draws (np.random.default_rng(seed).uniform(-1, 1, n) as
    float32) and its PINK / BROWN loops and range scaling as the float32 operations that numpy >= 2 makes of them, one
    rounding per `*` and `+`, in the reference's order, block by block with carried state.  The six pink taps are one
    float32 vector per step (they are independent of one another), everything around them is elementwise.
(b) A pure-Python model of the DEVICE algorithm (`skip_table`, `pcg_skip`, `pcg_draw`, `model_draws`): the 128-bit LCG
    reached by the seed-independent table skip-ahead, the XSL-RR output function and the conversion to float32, on
    Python integers.

Graphs are golden-case SPECs (oracle/golden_cases.py, tests/control_oracle.py) with one more kind:
    {"pe": "NoisePE", "seed": int, "mode": "white" | "pink" | "brown", "min_value": number, "max_value": number}
which may sit anywhere, a MixPE input included.  NoiseNode derives from control_oracle.ControlNode (and so from
oracle.graph_eval.Node) and rebuilds its children as NoiseNodes."""

from __future__ import annotations

import numpy as np

import control_oracle as C
from oracle.graph_eval import INF
from oracle.spec_builder import is_spec, kinds_of      # noqa: F401  (kinds_of: shared with the tests)

KIND = "NoisePE"
MODES = ("white", "pink", "brown")


# ---------------------------------------------------------------------------------------------- (a) the restatement
F = np.float32
PINK_A = np.array([0.99886, 0.99332, 0.96900, 0.86650, 0.55000, -0.7616], dtype=F)
PINK_G = np.array([0.0555179, 0.0750759, 0.1538520, 0.3104856, 0.5329522, 0.0168980], dtype=F)


class NoiseStream:
    """One started NoisePE: render(n) consumes the next n draws (noise_pe.py:111-165)."""

    def __init__(self, seed, mode="white", min_value=-1.0, max_value=1.0):
        assert mode in MODES
        self.seed, self.mode = seed, mode
        self.min_value, self.max_value = float(min_value), float(max_value)
        self.reset()

    def reset(self):
        self.rng = np.random.default_rng(self.seed)
        self.taps = np.zeros(7, dtype=F)
        self.level = F(0.0)

    def white(self, n):
        return self.rng.uniform(-1.0, 1.0, size=n).astype(F)

    def pink(self, n):
        w = self.white(n)
        prod = w[:, None] * PINK_G[None, :]            # w * g_k
        prod[:, 5] = -prod[:, 5]                       # t - p and t + (-p) are the same float32
        taps = np.empty((n, 6), dtype=F)
        b, t = self.taps[:6].copy(), np.empty(6, dtype=F)
        for i in range(n):                             # b_k = a_k * b_k + w * g_k
            np.multiply(PINK_A, b, out=t)
            np.add(t, prod[i], out=b)
            taps[i] = b
        b6 = np.empty(n, dtype=F)
        b6[0] = self.taps[6]
        b6[1:] = w[:-1] * F(0.115926)
        s = taps[:, 0] + taps[:, 1]
        for k in (2, 3, 4, 5):
            s = s + taps[:, k]
        s = s + b6
        s = s + w * F(0.5362)
        self.taps[:6] = b
        self.taps[6] = w[-1] * F(0.115926)
        return s * F(0.11)

    def brown(self, n):
        steps = self.white(n) * F(0.02)
        out = np.empty(n, dtype=F)
        last, lo, hi = self.level, F(-1.0), F(1.0)
        for i, d in enumerate(steps):
            last = last + d
            if last < lo:
                last = lo
            elif last > hi:
                last = hi
            out[i] = last
        self.level = last
        return out

    def render(self, n):
        if n <= 0:
            return np.zeros((0, 1), dtype=F)
        x = getattr(self, self.mode)(n)
        if not (self.min_value == -1.0 and self.max_value == 1.0):           # noise_pe.py:102-109
            with np.errstate(over="ignore"):
                span = F(self.max_value - self.min_value)
                x = ((x + F(1.0)) * F(0.5)) * span + F(self.min_value)
        assert x.dtype == F
        return x.reshape(-1, 1)


# ---------------------------------------------------------------------------------------------- (b) the device model
PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
MASK128 = (1 << 128) - 1
MASK64 = (1 << 64) - 1


def skip_table():
    """[(M^(2^k), S_(2^k))], k = 0..63, S_n = 1 + M + ... + M^(n-1): n LCG steps are s -> M^n * s + inc * S_n."""
    table, a, c = [], PCG_MULT, 1
    for _ in range(64):
        table.append((a, c))
        c = c * (a + 1) & MASK128
        a = a * a & MASK128
    return table


_TABLE = skip_table()


def pcg_skip(state, inc, distance):
    k = 0
    while distance:
        if distance & 1:
            a, c = _TABLE[k]
            state = (a * state + c * inc) & MASK128
        distance >>= 1
        k += 1
    return state


def pcg_draw(state):
    """The float32 that uniform(-1, 1) makes of an (already stepped) state."""
    hi, lo = state >> 64, state & MASK64
    x, rot = hi ^ lo, hi >> 58
    u = ((x >> rot) | (x << ((64 - rot) & 63))) & MASK64
    return F(-1.0 + 2.0 * ((u >> 11) * 2.0 ** -53))


def seeded(seed):
    s = np.random.PCG64(seed).state["state"]
    return int(s["state"]), int(s["inc"])


def model_draws(seed, offset, n):
    """Draws offset .. offset + n - 1 of default_rng(seed).uniform(-1, 1, ...).astype(float32), the device's way."""
    state, inc = seeded(seed)
    state = pcg_skip(state, inc, offset)
    out = np.empty(n, dtype=F)
    for i in range(n):
        state = (state * PCG_MULT + inc) & MASK128
        out[i] = pcg_draw(state)
    return out


def numpy_draws(seed, offset, n):
    bit_gen = np.random.PCG64(seed)
    if offset:
        bit_gen.advance(offset)
    return np.random.Generator(bit_gen).uniform(-1.0, 1.0, size=n).astype(F)


# ---------------------------------------------------------------------------------------------- graph evaluation
class NoiseNode(C.ControlNode):
    """control_oracle.ControlNode plus the kind NoisePE, at any depth of the graph."""

    def __init__(self, spec, sr, shared=None):
        super().__init__(spec, sr)
        for k, v in self.kw.items():
            if is_spec(v):
                self.sub[k] = NoiseNode(v, sr)
            elif k == "inputs":
                self.sub[k] = [NoiseNode(s, sr) for s in v]

    def reset(self, recursive=True):
        if self.kind == KIND:
            kw = self.kw
            self.stream = NoiseStream(kw.get("seed"), kw.get("mode", "white"), kw.get("min_value", -1.0),
                                      kw.get("max_value", 1.0))
        super().reset(recursive)

    def channels(self):
        return 1 if self.kind == KIND else super().channels()

    def extent(self):
        return INF if self.kind == KIND else super().extent()

    def render(self, start, n):
        if self.kind == KIND:
            return self.stream.render(n)           # `start` is ignored (noise_pe.py:151-165)
        return super().render(start, n)


def find_nodes(node, kinds=(KIND,)):
    return C.find_nodes(node, kinds)


def run_case(case):
    """Every block of a case through the restatement.  `ops`: "restart" (renderer stop + start) or "reset"
    (reset_state() of every NoisePE of the graph) before a block index."""
    g = NoiseNode(case["graph"], case["sr"])
    ops = {int(k): v for k, v in case.get("ops", {}).items()}
    outs = []
    for i, (s, n) in enumerate(case["blocks"]):
        if ops.get(i) == "restart":
            g.stop()
            g.reset()
        elif ops.get(i) == "reset":
            for node in find_nodes(g):
                node.reset(recursive=False)
        outs.append(g.render(int(s), int(n)))
    return outs, g
