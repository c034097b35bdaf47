"""The auto precision protocol (drmnet_amd/autoprec.py) on the CPU: ChainProbe driven by stand-in networks and a fake chain whose output depends on
the stand-ins' current modes -- ``base`` in f16x3, ``base * (1 + eps_row)`` as soon as one network is on f16mx -- so every figure is known exactly."""
import pytest
import torch

from drmnet_amd.autoprec import ChainProbe, ProbeState, tensor_sig, worst_row_rel_l2

EPS = (1e-3, 4e-3)  # rel-L2 of the two probe rows, f16mx against f16x3


class Net:
    """What ChainProbe asks of a network: precision, _set_mode, auto_report, auto_sig, auto_override."""

    def __init__(self, precision="f16mx", sig=("w", 0), measured=True):
        self.precision, self.auto_sig = precision, sig
        self.auto_report = {"chosen": precision} if measured else None
        self.mode_calls, self.overrides = [], []

    def _set_mode(self, mode):
        self.precision = mode
        self.mode_calls.append(mode)

    def auto_override(self, mode, why):
        self.auto_report = dict(self.auto_report, chosen=mode, overridden_by=why)
        self.overrides.append((mode, why))
        if self.precision != mode:
            self._set_mode(mode)


class Chain:
    def __init__(self, nets, bad=None, inside=None):
        self.nets, self.bad, self.inside, self.calls = nets, bad, inside, []

    def __call__(self, x):
        modes = tuple(n.precision for n in self.nets.values())
        self.calls.append((modes, x.clone()))
        if self.inside is not None:
            self.inside()
        out = x.double().flatten(1) * 2 + 1
        if "f16mx" in modes:
            out = out * (1 + torch.tensor(EPS[: x.shape[0]], dtype=torch.float64)[:, None])
            if self.bad is not None:
                out[0, 0] = self.bad
        return out


def setup(tol, modes=("f16mx", "f16mx"), probe=None, **chain_kw):
    nets = {"illnet": Net(modes[0], ("i", 0)), "refnet": Net(modes[1], ("r", 0))}
    cp = ChainProbe(tol, 8, probe, step_name="fake steps", probe_text="{dims} {rows}, {steps} fake steps, worst row")
    return cp, nets, Chain(nets, **chain_kw)


def rows5():
    return torch.arange(5.0)[:, None, None, None].expand(5, 3, 2, 4) + torch.linspace(0.1, 0.9, 24).reshape(3, 2, 4)


def test_worst_row_decides_and_modes_follow():
    # a bar between the two rows' errors: the worse row decides -> every network overridden to f16x3, with the reason
    cp, nets, chain = setup(2e-3, modes=("f16mx", "f16x3"))
    cp.measure(nets, "live", chain, rows5())
    rep = cp.report
    assert not rep["kept"] and rep["rel_l2_chain_vs_f16x3"] == pytest.approx(EPS[1], rel=1e-9) and rep["rows"] == [1e-3, 4e-3]
    assert [m for m, _ in chain.calls] == [("f16mx", "f16x3"), ("f16x3", "f16x3")]  # exactly two runs: as chosen, then all f16x3
    why = "chain probe: 8 fake steps differ from f16x3 by 4.00e-03 > 2e-03"
    for n in nets.values():
        assert n.precision == "f16x3" and n.overrides == [("f16x3", why)] and n.auto_report["overridden_by"] == why
    assert list(rep) == ["kept", "rel_l2_chain_vs_f16x3", "rows", "steps", "tolerance", "modes", "probe_source", "probe"]
    assert rep["modes"] == {"illnet": "f16mx", "refnet": "f16x3"} and rep["steps"] == 8 and rep["tolerance"] == 2e-3
    assert rep["probe_source"] == "caller" and rep["probe"] == "2x3x2x4 rows of the caller, 8 fake steps, worst row"
    # a bar above both: kept, and the modes the networks had before are back -- a mixed pair included
    for modes in (("f16mx", "f16mx"), ("f16mx", "f16x3"), ("f16x3", "f16mx")):
        cp, nets, chain = setup(1e-2, modes=modes)
        cp.measure(nets, "live", chain, rows5())
        assert cp.report["kept"] and cp.report["rel_l2_chain_vs_f16x3"] == pytest.approx(EPS[1], rel=1e-9) and len(chain.calls) == 2
        assert tuple(n.precision for n in nets.values()) == modes and cp.report["modes"] == dict(zip(nets, modes))
        assert all(n.overrides == [] and "overridden_by" not in n.auto_report for n in nets.values())


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_result_is_never_kept(bad):
    cp, nets, chain = setup(float("inf"), bad=bad)  # (inf <= inf: only the isfinite condition stands in the way)
    cp.measure(nets, "live", chain, rows5())
    assert cp.report["kept"] is False and all(n.precision == "f16x3" and len(n.overrides) == 1 for n in nets.values())


def test_row_choice_and_single_network_report():
    x = rows5()
    cp, nets, chain = setup(1.0)
    cp.measure(nets, "live", chain, x)
    assert all(torch.equal(got, x[[0, 2]]) for _, got in chain.calls)  # rows 0 and n // 2, at their own size
    assert all(got.dtype == torch.float32 and got.is_contiguous() for _, got in chain.calls)
    cp, nets, chain = setup(1.0)
    cp.measure(nets, "live", chain, x[3:4])
    assert all(torch.equal(got, x[3:4]) for _, got in chain.calls) and cp.report["rows"] == [1e-3]
    assert cp.report["probe"].startswith("1x3x2x4 rows of the caller")
    # no rows at all: the seeded synthetic pair at 128 x 128
    cp, nets, chain = setup(1.0)
    cp.measure(nets, "live", chain)
    assert [tuple(got.shape) for _, got in chain.calls] == [(2, 3, 128, 128)] * 2 and torch.equal(chain.calls[0][1], chain.calls[1][1])
    assert cp.report["probe_source"] == "synthetic" and cp.report["probe"] == "2x3x128x128 seeded refmaps, 8 fake steps, worst row"
    # one network: no "modes" (the mode kept can only be f16mx); the model's own wording of the caller's rows
    unet = {"unet": Net()}
    cp = ChainProbe(1.0, 3, step_name="DDIM steps", probe_text="{dims} {rows}: first {steps} steps", caller_rows="conditioning rows of the caller")
    cp.measure(unet, "live", Chain(unet), x)
    assert list(cp.report) == ["kept", "rel_l2_chain_vs_f16x3", "rows", "steps", "tolerance", "probe_source", "probe"]
    assert cp.report["probe"] == "2x3x2x4 conditioning rows of the caller: first 3 steps" and unet["unet"].precision == "f16mx"


def test_records_and_what_invalidates_them():
    x = rows5()
    cp, nets, chain = setup(1.0)
    cp.measure(nets, "live", chain, x)
    rep = cp.report
    calls = [list(n.mode_calls) for n in nets.values()]
    cp.report = None
    cp.measure(nets, "live", chain, x.flip(0))  # same signatures: the SAME report object, no run, no mode touched
    assert cp.report is rep and len(chain.calls) == 2 and [n.mode_calls for n in nets.values()] == calls
    cp.measure(nets, "live", chain)  # a record made on the caller's rows stands for a later call without rows
    assert cp.report is rep and len(chain.calls) == 2
    nets["refnet"].auto_sig = ("r", 1)  # other weights
    cp.measure(nets, "live", chain, x)
    assert cp.report is not rep and len(chain.calls) == 4
    cp.measure(nets, "ema", chain, x)  # another weight set
    assert len(chain.calls) == 6 and len(cp.done) == 3
    cp.measure(nets, "live", chain, x)
    assert len(chain.calls) == 6  # ... and back: on record


def test_synthetic_record_does_not_stand_in_for_data_and_set_probe():
    x = rows5()
    cp, nets, chain = setup(1.0)
    cp.measure(nets, "live", chain)
    rep_s = cp.report
    assert rep_s["probe_source"] == "synthetic" and len(chain.calls) == 2
    cp.measure(nets, "live", chain, x)  # rows of the caller: measured although a synthetic record exists
    rep_d = cp.report
    assert rep_d is not rep_s and rep_d["probe_source"] == "caller" and len(chain.calls) == 4
    cp.measure(nets, "live", chain)
    assert cp.report is rep_d and len(chain.calls) == 4
    # set_probe: the caller records go, the synthetic one stays; the new rows are what a call without rows measures on
    cp.set_probe(x * 3)
    assert list(cp.done.values()) == [rep_s] and cp.probe is not None
    cp.measure(nets, "live", chain)
    assert len(chain.calls) == 6 and torch.equal(chain.calls[-1][1], (x * 3)[[0, 2]]) and cp.report["probe_source"] == "caller"
    # the probe given at construction is used the same way
    cp, nets, chain = setup(1.0, probe=x)
    cp.measure(nets, "live", chain)
    assert cp.report["probe_source"] == "caller" and torch.equal(chain.calls[0][1], x[[0, 2]])


def test_nothing_runs_without_f16mx_or_without_a_network_report():
    cp, nets, chain = setup(1e-9, modes=("f16x3", "f16x3"))
    cp.measure(nets, "live", chain, rows5())
    assert chain.calls == [] and cp.report is None and cp.done == {} and all(n.mode_calls == [] and n.overrides == [] for n in nets.values())
    cp, nets, chain = setup(1e-9)
    nets["refnet"].auto_report = None  # (not measured yet)
    cp.measure(nets, "live", chain, rows5())
    assert chain.calls == [] and cp.report is None and cp.done == {} and all(n.mode_calls == [] and n.precision == "f16mx" for n in nets.values())


def test_reentrant_call_returns_at_once():
    seen = []

    def inside():
        seen.append(cp.busy)
        before = len(chain.calls)
        cp.measure(nets, "live", chain, rows5())
        assert len(chain.calls) == before and cp.report is None

    cp, nets, chain = setup(1.0, inside=inside)
    cp.measure(nets, "live", chain, rows5())
    assert seen == [True, True] and len(chain.calls) == 2 and cp.report["kept"] and not cp.busy

    def boom(x):
        raise RuntimeError("chain failed")

    cp2 = setup(1.0)[0]
    with pytest.raises(RuntimeError):  # (busy is released when the chain raises)
        cp2.measure(nets, "live", boom, rows5())
    assert not cp2.busy and cp2.done == {}


def test_worst_row_rel_l2_and_tensor_sig():
    b = torch.tensor([[3.0, 4.0], [0.0, 2.0], [0.0, 0.0]])
    a = torch.tensor([[3.0, 4.5], [0.0, 2.0], [0.0, 0.0]])
    err, rows = worst_row_rel_l2(a, b)
    assert rows == [pytest.approx(0.1), 0.0, 0.0] and err == pytest.approx(0.1)  # (an all-zero reference row: 0 / 1e-300, not 0 / 0)
    err, rows = worst_row_rel_l2(torch.ones(2, 3, 2, 2), torch.full((2, 3, 2, 2), 2.0))  # rows are flattened
    assert rows == [pytest.approx(0.5)] * 2 and err == pytest.approx(0.5)
    assert worst_row_rel_l2(torch.tensor([[1e-30]]), torch.tensor([[1e-30]]).double() * 2)[0] == pytest.approx(0.5)  # fp64 inside
    p, q = torch.zeros(4), torch.zeros(4)
    sig = tensor_sig([p, q])
    assert sig == tensor_sig([p, q]) == ((p.data_ptr(), p._version), (q.data_ptr(), q._version)) and sig != tensor_sig([q, p])
    q.add_(1)  # an in-place edit bumps the signature
    assert tensor_sig([p, q]) != sig and tensor_sig([p, q])[0] == sig[0]
    assert tensor_sig([p, q.clone()]) != tensor_sig([p, q])  # other storage
    st = ProbeState(5e-5, [128, 128])
    assert (st.tolerance, st.probe_hw, st.sig, st.report, st.busy, st.cache) == (5e-5, (128, 128), None, None, False, {})
