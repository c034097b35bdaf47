"""The ``auto`` precision policy, host logic only: f16mx is kept where it measurably agrees with f16x3 on the weights actually loaded.  Each network
measures ONE forward of a seeded probe batch in both modes (unet.py ``_auto_resolve``, state in ``ProbeState``); a sampler applies ~100 forwards to its own
output, so the model classes put a ``ChainProbe`` on top.  Both decide by ``worst_row_rel_l2`` and key their records by ``tensor_sig`` of the weights.
Nothing here touches the HIP library: networks and chain are handed in, so the protocol runs without a GPU (tests/test_autoprec_cpu.py)."""
from __future__ import annotations

import torch


def worst_row_rel_l2(a: torch.Tensor, b: torch.Tensor) -> tuple[float, list[float]]:
    """(max, per row) of |a - b| / |b| over the rows of two [B, ...] tensors, in fp64: the worst row decides, a batch mean would hide it."""
    a, b = a.double().flatten(1), b.double().flatten(1)
    rows = ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)).tolist()
    return max(rows), rows


def tensor_sig(tensors) -> tuple:
    """Identity of a set of weights: storage and in-place version of every tensor (load_state_dict, .to(), an optimizer step all change it)."""
    return tuple((p.data_ptr(), p._version) for p in tensors)


class ProbeState:
    """Auto-mode state of one network: the bar, the probe size, the signature / report of the weights last measured, and every report by
    (weight set, signature) so that entering / leaving ema_scope repeats no measurement."""

    def __init__(self, tolerance: float, probe_hw: tuple[int, int]):
        self.tolerance, self.probe_hw = float(tolerance), tuple(probe_hw)
        self.sig: tuple | None = None  # tensor_sig of the weights ``report`` was measured on
        self.report: dict | None = None
        self.busy, self.cache = False, {}  # cache: (weight set, sig) -> report


class ChainProbe:
    """The chain probe of a model in auto mode.  Where its networks settled on f16mx, ``steps`` steps of the model's chain (fixed noise key, every row
    active) are run in the chosen modes and in f16x3; f16mx is kept only if every row of the final state agrees to ``tolerance``, otherwise ALL the
    networks run in f16x3 for these weights (``auto_override``).  The rows: the CALLER's when there are any -- the batch a sampler was called with, or
    the ``probe`` of set_precision / calibrate_precision; first and middle row, at their own size -- else two seeded synthetic refmaps at 128x128.
    Records are kept per (weight set, network signatures, "data" | "synth").  ``step_name`` / ``probe_text`` / ``caller_rows`` word the model's report."""

    def __init__(self, tolerance: float, steps: int, probe: torch.Tensor | None = None, *, step_name: str, probe_text: str, caller_rows: str = "rows of the caller"):
        self.tolerance, self.steps, self.probe = tolerance, steps, probe
        self.step_name, self.probe_text, self.caller_rows = step_name, probe_text, caller_rows
        self.done, self.busy = {}, False  # done: (weight set, network sigs, "data" | "synth") -> report
        self.report: dict | None = None

    def set_probe(self, rows: torch.Tensor) -> None:
        """New rows of the caller: they are measured even if a probe of these weights on earlier rows is on record."""
        self.probe = rows
        self.done = {k: v for k, v in self.done.items() if k[-1] != "data"}

    @torch.no_grad()
    def measure(self, nets: dict, weight_set: str, run_chain, rows: torch.Tensor | None = None, device=None) -> None:
        """``nets``: label -> network (precision, _set_mode, auto_report, auto_sig, auto_override).  ``run_chain(x)``: the chain from the rows ``x``
        [B, ...] in whatever modes the networks are in NOW -> its final state [B, ...].  ``rows``: the batch of the caller, if any."""
        if self.busy or any(n.auto_report is None for n in nets.values()):
            return
        rows = self.probe if rows is None else rows
        sigs = (weight_set,) + tuple(n.auto_sig for n in nets.values())
        # (no rows, but measured on the caller's rows before: that record stands)
        key = sigs + ("data" if rows is not None or sigs + ("data",) in self.done else "synth",)
        if key in self.done:
            self.report = self.done[key]
            return
        if all(n.precision != "f16mx" for n in nets.values()):
            return
        self.busy = True
        try:
            caller = rows is not None
            if caller:
                x = rows[[0, rows.shape[0] // 2]] if rows.shape[0] > 1 else rows[:1]
            else:
                from . import synth  # (torch only, like this module)

                x = synth.synth_refmaps(2, 128, 128, 4321)
            x = x.detach().to(device=device, dtype=torch.float32).contiguous()
            chosen = {label: n.precision for label, n in nets.items()}
            a = run_chain(x).double().flatten(1)
            for n in nets.values():
                n._set_mode("f16x3")
            err, per_row = worst_row_rel_l2(a, run_chain(x))
            kept = err <= self.tolerance and bool(torch.isfinite(a).all())
            for label, n in nets.items():
                if kept:
                    n._set_mode(chosen[label])
                else:
                    n.auto_override("f16x3", f"chain probe: {self.steps} {self.step_name} differ from f16x3 by {err:.2e} > {self.tolerance:.0e}")
            self.report = {"kept": kept, "rel_l2_chain_vs_f16x3": err, "rows": [float(f"{r:.3e}") for r in per_row], "steps": self.steps,
                           "tolerance": self.tolerance, **({"modes": chosen} if len(nets) > 1 else {}),  # (one network: the mode kept is f16mx)
                           "probe_source": "caller" if caller else "synthetic",
                           "probe": self.probe_text.format(dims="x".join(map(str, x.shape)), rows=self.caller_rows if caller else "seeded refmaps", steps=self.steps)}
            self.done[key] = self.report
        finally:
            self.busy = False
