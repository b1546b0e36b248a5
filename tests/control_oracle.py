"""SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE on the CPU: numpy restatements of the four `_render`s
(the reference's operations in the reference's order: a sequential walk for the holds and the slew limiter,
sequential np.cumsum for the generator's phase and np.sum for the carried one), shared by the fixture generator
(tools/gen_golden_control.py, over the reference's classes) and the tests (over pygmu2_amd's).

Graphs are golden-case SPECs (oracle/golden_cases.py) with four more kinds:
    {"pe": "SampleHoldPE", "source": SPEC, "trigger": SPEC, "initial_value": number}
    {"pe": "TrackHoldPE", "source": SPEC, "gate": SPEC, "initial_value": number}
    {"pe": "SlewLimiterPE", "source": SPEC, "rise_rate": number, "fall_rate": number | null, "mode": "linear"|"exponential"}
    {"pe": "FunctionGenPE", "frequency" / "duty_cycle" / "phase": number | SPEC, "waveform": ..., "channels": int}
Every other kind is evaluated by oracle/graph_eval.py (ControlNode derives from its Node); oracle/spec_builder.py builds
all of them, and tests/fixture_harness.py loads the fixture and holds the bounds."""

from __future__ import annotations

import numpy as np

from oracle.graph_eval import INF, Node, _isect
from oracle.spec_builder import is_spec

NEW_KINDS = ("SampleHoldPE", "TrackHoldPE", "SlewLimiterPE", "FunctionGenPE")


# ---------------------------------------------------------------------------------------------- the four renders
def hold_block(held, src, control, threshold):
    """sample_hold_pe.py:73-85 / track_hold_pe.py:73-85 -> (float32 samples, the held value after the block)."""
    out = np.empty(len(src), dtype=np.float32)
    for i in range(len(src)):
        if control[i] > threshold:
            held = float(src[i])
        out[i] = held
    return out, held


def slew_block(current, src, rise_dt, fall_dt, exponential):
    """slew_limiter_pe.py:113-134 -> (float32 samples, the carried value after the block)."""
    out = np.empty(len(src), dtype=np.float32)
    x = src.astype(np.float64).tolist()
    if exponential:
        rise_k, fall_k = min(rise_dt, 1.0), min(fall_dt, 1.0)
        for i, v in enumerate(x):
            error = v - current
            current += (rise_k if error > 0 else fall_k) * error
            out[i] = current
    else:
        for i, v in enumerate(x):
            delta = v - current
            if delta > rise_dt:
                delta = rise_dt
            elif delta < -fall_dt:
                delta = -fall_dt
            current += delta
            out[i] = current
    return out, current


def saw_morph(phase, duty):
    """function_gen_pe.py:121-155."""
    eps = 1e-12
    a = 1.0 - duty
    up, down = duty <= eps, duty >= 1.0 - eps
    mid = ~(up | down)
    y = np.empty_like(phase)
    y[up] = 2.0 * phase[up] - 1.0
    y[down] = 1.0 - 2.0 * phase[down]
    am, p = np.clip(a[mid], eps, 1.0 - eps), phase[mid]
    rising = p < am
    ym = np.empty_like(p)
    ym[rising] = -1.0 + 2.0 * (p[rising] / am[rising])
    ym[~rising] = 1.0 - 2.0 * ((p[~rising] - am[~rising]) / (1.0 - am[~rising]))
    y[mid] = ym
    return y


def function_gen_block(state, start, n, freq, duty, ph, sr, waveform, channels, pure):
    """function_gen_pe.py:157-193.  freq / duty / ph: float64 arrays of n values.  state: {"phase", "end"}.
    -> (float32 (n, channels), float64 phases, clipped duty)."""
    dt = freq / float(sr)
    if pure:
        base = np.mod(np.arange(start, start + n, dtype=np.float64) * float(dt[0]), 1.0)
    else:
        if state["end"] is None or start != state["end"]:
            state["phase"] = 0.0
        inc = np.concatenate(([0.0], np.cumsum(dt[:-1], dtype=np.float64)))
        base = np.mod(state["phase"] + inc, 1.0)
        state["phase"] = float(np.mod(state["phase"] + float(np.sum(dt)), 1.0))
        state["end"] = start + n
    phase = np.mod(base + ph, 1.0)
    duty = np.clip(duty, 0.0, 1.0)
    y = np.where(phase < duty, 1.0, -1.0) if waveform == "rectangle" else saw_morph(phase, duty)
    return np.tile(y.reshape(-1, 1), (1, channels)).astype(np.float32), phase, duty


# ---------------------------------------------------------------------------------------------- graph evaluation
class ControlNode(Node):
    """oracle.graph_eval.Node plus the four new kinds, at any depth of the graph."""

    def __init__(self, spec, sr, shared=None):
        super().__init__(spec, sr, {})
        for k, v in self.kw.items():
            if is_spec(v):
                self.sub[k] = ControlNode(v, sr)
            elif k == "inputs":
                self.sub[k] = [ControlNode(s, sr) for s in v]
        self.log = []                # FunctionGenPE: per block {"phase", "duty", "dt", "restart"}
        self.reset()

    def _control_name(self):
        return "trigger" if self.kind == "SampleHoldPE" else "gate"

    def reset(self, recursive=True):
        if self.kind in ("SampleHoldPE", "TrackHoldPE"):
            self.held = float(self.kw.get("initial_value", 0.0))
        elif self.kind == "SlewLimiterPE":
            self.current = 0.0
        elif self.kind == "FunctionGenPE":
            self.fg = {"phase": 0.0, "end": None}
        super().reset(recursive)

    def channels(self):
        if self.kind == "FunctionGenPE":
            return int(self.kw.get("channels", 1))
        if self.kind in NEW_KINDS:
            return 1
        return super().channels()

    def extent(self):
        if self.kind == "FunctionGenPE":
            ext = INF
            for name in ("frequency", "duty_cycle", "phase"):              # inputs() order
                if name in self.sub:
                    ext = _isect(ext, self.sub[name].extent())
            return ext
        if self.kind in NEW_KINDS:
            return INF
        return super().extent()

    def _values(self, name, default, start, n):
        if name in self.sub:
            return self.sub[name].render(start, n)[:, 0].astype(np.float64)
        return np.full((n,), float(self.kw.get(name, default)), dtype=np.float64)

    def render(self, start, n):
        if self.kind not in NEW_KINDS or n == 0:
            return super().render(start, n)
        if self.kind in ("SampleHoldPE", "TrackHoldPE"):
            control = self.sub[self._control_name()].render(start, n)[:, 0]
            src = self.sub["source"].render(start, n)[:, 0]
            out, self.held = hold_block(self.held, src, control, 0.0 if self.kind == "SampleHoldPE" else 0.5)
            return out.reshape(-1, 1)
        if self.kind == "SlewLimiterPE":
            src = self.sub["source"].render(start, n)[:, 0]
            rise = float(self.kw["rise_rate"])
            fall = self.kw.get("fall_rate")
            fall = rise if fall is None else float(fall)
            sr = float(self.sr)
            out, self.current = slew_block(self.current, src, rise / sr, fall / sr,
                                           self.kw.get("mode", "linear") == "exponential")
            return out.reshape(-1, 1)
        freq = self._values("frequency", 1.0, start, n)
        duty = self._values("duty_cycle", 0.5, start, n)
        ph = self._values("phase", 0.0, start, n)
        pure = not self.sub
        restart = (not pure) and (self.fg["end"] is None or start != self.fg["end"])
        out, phase, duty = function_gen_block(self.fg, start, n, freq, duty, ph, self.sr,
                                              str(self.kw.get("waveform", "rectangle")).lower(),
                                              int(self.kw.get("channels", 1)), pure)
        self.log.append({"phase": phase, "duty": duty, "dt": freq / float(self.sr), "restart": restart})
        return out

    def stop(self):
        """Renderer.stop(): FunctionGenPE alone resets on it (function_gen_pe.py:108-109)."""
        if self.kind == "FunctionGenPE":
            self.fg = {"phase": 0.0, "end": None}
        for s in self.sub.values():
            for c in (s if isinstance(s, list) else [s]):
                if isinstance(c, ControlNode):
                    c.stop()


def find_nodes(node, kinds):
    out = [node] if node.kind in kinds else []
    for s in node.sub.values():
        for c in (s if isinstance(s, list) else [s]):
            out += find_nodes(c, kinds)
    return out


def run_case(case):
    """Every block of a case through the restatement; `ops` entries of the case ("reset" / "restart" before a block
    index) are applied as the generator applies them to the reference graph."""
    g = ControlNode(case["graph"], case["sr"])
    ops = {int(k): v for k, v in case.get("ops", {}).items()}
    outs = []
    for i, (s, n) in enumerate(case["blocks"]):
        if ops.get(i) == "restart":
            g.stop()
            g.reset()
        elif ops.get(i) == "reset":
            for node in find_nodes(g, NEW_KINDS):
                node.reset(recursive=False)
        outs.append(g.render(int(s), int(n)))
    return outs, g
