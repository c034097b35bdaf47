"""GPU tests of the auto precision policy (drmnet_amd/autoprec.py; the protocol itself runs on the CPU in test_autoprec_cpu.py): the per-network
probe on the loaded weights, its report cache, and the chain probe of DRMNet / ObsNet on synthetic rows and on the caller's batch."""
import pytest
import torch

from conftest import gold, rel_l2
from drmnet_amd import synth
from oracle import unet as ou
from test_gpu_nets import full_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


@pytest.mark.parametrize("rule,expect", [("normal", "f16mx"), ("stress:10", "f16x3")])
def test_auto_precision_measures_the_loaded_weights(dev, rule, expect):
    """set_precision("auto") (bench.py's default): one seeded probe forward in f16x3 and one in f16mx on the weights actually loaded; f16mx is kept
    only if the two agree to 5e-5.  The synthetic weights of the benches and fixtures pass (RefNet ~3e-6); the same network with GroupNorm gains x 10
    amplifies rounding noise forty-fold (f16mx 9e-4 against the reference, f16x3 1e-5) and must be sent to f16x3; new weights are re-measured."""
    from drmnet_amd.unet import EncoderUNetModel

    g = gold("stress10_refnet")
    m = EncoderUNetModel(**ou.REFNET_CFG)
    synth.load_synth(m, int(g["seed"]), rule=rule)
    m = m.to(dev).set_precision("auto")
    assert m.auto_report is None  # nothing measured before the first forward
    xc, _ = full_inputs(2, 32, 64)
    out = m(xc.to(dev), torch.from_numpy(g["t"])[:2].to(dev))
    rep = m.auto_report
    print(f"auto precision on RefNet with {rule} weights: {rep}")
    assert rep["chosen"] == expect == m.precision and (rep["rel_l2_f16mx_vs_f16x3"] <= rep["tolerance"]) == (expect == "f16mx")
    if rule != "normal":
        e = rel_l2(out.cpu(), g["out64_2x32x64"])
        assert e < 1e-4  # (in f16x3 the stressed network is back inside the contract: 1.4e-5)
        synth.load_synth(m, synth.SEED_REFNET)  # other weights -> measured again on the next forward
        m(xc.to(dev), torch.from_numpy(g["t"])[:2].to(dev))
        assert m.auto_report["chosen"] == "f16mx" == m.precision
    assert m.set_precision("f16x3").auto_report is None  # an explicit mode leaves auto


def test_auto_precision_probe_rows_and_cache(dev):
    """[r5] The per-network probe is a batch (two inputs x three timesteps, worst row decides) and its reports are kept per (weight set, weight
    signature): toggling between the live weights and an EMA shadow does not repeat a measurement."""
    from drmnet_amd.unet import EncoderUNetModel

    m = EncoderUNetModel(**ou.TINY_ENC_CFG)
    synth.load_synth(m, 5)
    m = m.to(dev).set_precision("auto")
    rep = m.calibrate_precision()
    assert len(rep["rows"]) == 6 and rep["rel_l2_f16mx_vs_f16x3"] == pytest.approx(max(rep["rows"]), rel=1e-3)
    cache = m._auto.cache
    assert len(cache) == 1
    ema = [p.detach().clone() * 1.01 for p in m.param_tensors()]
    m.use_weights("ema", ema)
    rep_e = m.calibrate_precision()
    assert len(cache) == 2 and rep_e is not rep
    m.use_weights("live")
    assert m.calibrate_precision() is rep  # the stored report, no new measurement
    m.use_weights("ema", ema)
    assert m.calibrate_precision() is rep_e and len(cache) == 2


def test_auto_precision_chain_probe_overrules_the_single_forward_probe(dev):
    """[r5, VERDICT r4 item 6] A per-network probe compares one forward; the samplers apply ~100 of them to their own output.  In auto mode DRMNet runs
    eight reverse steps (ObsNet: eight DDIM steps) in the chosen modes and in f16x3 and keeps f16mx only if the chains agree to half the contract.
    Weights that pass the single-forward probe but fail the chain probe (here: the chain tolerance put below what f16mx can deliver) must land on
    f16x3 -- both networks -- while the per-network reports still show that each one passed on its own."""
    from drmnet_amd.drmnet import DRMNet
    from drmnet_amd.obsnet import ObsNetDiffusion

    unet_t = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(ou.TINY_UNET_CFG)}
    enc_t = {"target": "ldm.modules.diffusionmodules.openaimodel.EncoderUNetModel", "params": dict(ou.TINY_ENC_CFG)}

    def build():
        m = DRMNet(illnet_config=unet_t, refnet_config=enc_t, max_timesteps=12, image_size=16, concat_mode=True, use_ema=False, gamma=0.9, epsilon=0.01, delta=0.025,
                   z0=[1, 1, 1, 1, 0, 1], brdf_param_names=["p"] * 6)
        synth.load_synth(m.illnet_model.diffusion_model, 21)
        synth.load_synth(m.refnet_model.diffusion_model, 22)
        zman = [(k, tuple(v.shape)) for k, v in m.illnet_model.z_emb_layer.state_dict().items()]
        m.illnet_model.z_emb_layer.load_state_dict(synth.synth_state_dict(zman, synth.SEED_ZEMB))
        return m.to(dev)

    def auto(m, chain_tol):  # (the tiny networks amplify rounding noise more than the shipped ones: 1e-4 per forward in f16mx -- the test is about the mechanism,
        m.AUTO_CHAIN_TOLERANCE = chain_tol  #  so the per-network bar is put where they pass it and the chain bar decides)
        m.set_precision("auto")
        for net in (m.illnet_model.diffusion_model, m.refnet_model.diffusion_model):
            net.set_precision_auto(tolerance=1e-3)
        return m

    m = auto(build(), 1e-1)
    rep = m.calibrate_precision()
    ill, ref = m.illnet_model.diffusion_model, m.refnet_model.diffusion_model
    print(f"chain probe (tiny DRMNet): {rep}; illnet {ill.auto_report}; refnet {ref.auto_report}")
    assert rep["kept"] and rep["rel_l2_chain_vs_f16x3"] <= rep["tolerance"] and ill.precision == ref.precision == "f16mx"
    LrK = synth.synth_refmaps(2, 16, 32, 5).to(dev)
    out_auto = m.p_sample_loop(LrK, [LrK], [LrK], verbose=False, seed=3, early_exit=False)[0]
    # [r6] the first batch the sampler sees is handed to the chain probe (rows of the caller, once per weight signature): that record stands from then on
    rep_d = m.auto_chain_report
    assert rep_d is not rep and rep_d["probe_source"] == "caller" and rep["probe_source"] == "synthetic" and rep_d["kept"]
    m.p_sample_loop(LrK, [LrK], [LrK], verbose=False, seed=4, early_exit=False)
    assert m.calibrate_precision() is rep_d  # measured once for these weights

    # the case the chain probe exists for, as it occurs: every network passes its single-forward probe at 1e-3 (1.2e-4 / 1.7e-5), and eight steps of the
    # undamped tiny sampler blow the f16mx-vs-f16x3 difference up to ~3e-3 -- the SAME bar applied to the chain sends both networks to f16x3
    m2 = auto(build(), 1e-3)
    rep2 = m2.calibrate_precision()
    assert rep2["rel_l2_chain_vs_f16x3"] > 1e-3 > max(m2.illnet_model.diffusion_model.auto_report["rel_l2_f16mx_vs_f16x3"], m2.refnet_model.diffusion_model.auto_report["rel_l2_f16mx_vs_f16x3"])
    ill2, ref2 = m2.illnet_model.diffusion_model, m2.refnet_model.diffusion_model
    assert not rep2["kept"] and ill2.precision == ref2.precision == "f16x3"
    assert ill2.auto_report["chosen"] == "f16x3" and "chain probe" in ill2.auto_report["overridden_by"]
    assert ill2.auto_report["rel_l2_f16mx_vs_f16x3"] <= ill2.auto_report["tolerance"]  # ... although the single forward had passed
    out_x3 = m2.p_sample_loop(LrK, [LrK], [LrK], verbose=False, seed=3, early_exit=False)[0]
    m3 = build().set_precision("f16x3")
    assert torch.equal(out_x3, m3.p_sample_loop(LrK, [LrK], [LrK], verbose=False, seed=3, early_exit=False)[0])  # it really runs in f16x3
    assert rel_l2(out_auto.cpu(), out_x3.cpu()) < 1e-1  # (tiny undamped networks, 12 steps in f16mx: see above)

    # ObsNet: the same mechanism on the first eight DDIM steps
    obs = ObsNetDiffusion(unet_config=unet_t, linear_start=1e-4, linear_end=0.09, log_every_t=2000, timesteps=1000, first_stage_key="LrK",
                          cond_stage_key="raw_refmap", padding_mode="noise", image_size=16, channels=3, concat_mode=True, ddim_steps=50,
                          clip_denoised=False, masked_loss=False, use_ema=False)
    synth.load_synth(obs.model.diffusion_model, 23)
    obs = obs.to(dev).set_precision("auto")
    obs.model.diffusion_model.set_precision_auto(tolerance=1e-3)
    obs._auto_chain.tolerance = 1e-3
    rep_o = obs.calibrate_precision()
    print(f"chain probe (tiny ObsNet): {rep_o}")
    assert rep_o is not None and rep_o["kept"] == (obs.model.diffusion_model.precision == "f16mx")
    obs._auto_chain.done.clear()
    obs._auto_chain.tolerance = 1e-9
    obs.model.diffusion_model._set_mode("f16mx")
    obs._auto_chain_probe()
    assert obs.model.diffusion_model.precision == "f16x3" and not obs.auto_chain_report["kept"]
    # what bench.py relies on for its explicit-mode passes: assigning None switches the chain probe off, and the mode set next is not second-guessed
    obs._auto_chain = None
    obs.set_precision("f16mx")
    assert torch.isfinite(obs.p_sample_loop(LrK, tuple(LrK.shape), verbose=False, start_T=3, seed=2)).all()
    assert obs.model.diffusion_model.precision == "f16mx" and obs.auto_chain_report is None


def test_auto_precision_gates_on_the_callers_batch(dev):
    """[r6, VERDICT r5 item 5b] The auto gate decides on the CALLER's data: p_sample_loop / ddim_sampling hand rows of their first batch to the chain
    probe (set_precision("auto", probe=...) / calibrate_precision(probe=...) take them explicitly), so the error that decides is the one measured on
    those rows, not on the seeded synthetic pair.  Shown on the tiny sampler: the caller-probe measures its own number (different rows, different
    size than the synthetic probe); a tolerance just below that number flips both networks to f16x3 (bit-identical to an f16x3 model from then on),
    a tolerance just above keeps f16mx; another batch of the same model does not re-measure; new data through calibrate_precision(probe=) does."""
    from drmnet_amd.drmnet import DRMNet
    from drmnet_amd.obsnet import ObsNetDiffusion

    unet_t = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(ou.TINY_UNET_CFG)}
    enc_t = {"target": "ldm.modules.diffusionmodules.openaimodel.EncoderUNetModel", "params": dict(ou.TINY_ENC_CFG)}

    def build(chain_tol, probe=None):
        m = DRMNet(illnet_config=unet_t, refnet_config=enc_t, max_timesteps=12, image_size=16, concat_mode=True, use_ema=False, gamma=0.9, epsilon=0.01, delta=0.025,
                   z0=[1, 1, 1, 1, 0, 1], brdf_param_names=["p"] * 6)
        synth.load_synth(m.illnet_model.diffusion_model, 21)
        synth.load_synth(m.refnet_model.diffusion_model, 22)
        zman = [(k, tuple(v.shape)) for k, v in m.illnet_model.z_emb_layer.state_dict().items()]
        m.illnet_model.z_emb_layer.load_state_dict(synth.synth_state_dict(zman, synth.SEED_ZEMB))
        m = m.to(dev)
        m.AUTO_CHAIN_TOLERANCE = chain_tol
        m.set_precision("auto", probe=probe)
        for net in (m.illnet_model.diffusion_model, m.refnet_model.diffusion_model):
            net.set_precision_auto(tolerance=1e-2)  # (per-network bar where the tiny networks pass it: the chain bar decides, as in the test above)
        return m

    LrK = synth.synth_refmaps(5, 16, 32, 5).to(dev)
    kw = dict(verbose=False, seed=3, early_exit=False)
    m = build(1.0)
    out = m.p_sample_loop(LrK, [LrK], [LrK], **kw)[0]
    rep = m.auto_chain_report
    e = rep["rel_l2_chain_vs_f16x3"]
    print(f"caller-batch chain probe (tiny DRMNet, rows 0 and 2 of a 5x3x16x32 batch): {rep}")
    assert rep["probe_source"] == "caller" and rep["probe"].startswith("2x3x16x32 rows of the caller") and rep["kept"] and 0 < e < 1.0
    rep_s = build(1.0).calibrate_precision()  # no data yet: the synthetic pair at 128 x 128 -- another measurement
    assert rep_s["probe_source"] == "synthetic" and rep_s["rel_l2_chain_vs_f16x3"] != e
    m.p_sample_loop(LrK.flip(0), [LrK.flip(0)], [LrK.flip(0)], **kw)
    assert m.auto_chain_report is rep  # the next batch re-measures nothing
    # the same rows against a bar just below / just above what they measure
    m_lo, m_hi = build(e * 0.5), build(e * 2.0)
    out_lo = m_lo.p_sample_loop(LrK, [LrK], [LrK], **kw)[0]
    out_hi = m_hi.p_sample_loop(LrK, [LrK], [LrK], **kw)[0]
    assert not m_lo.auto_chain_report["kept"] and m_lo.illnet_model.diffusion_model.precision == m_lo.refnet_model.diffusion_model.precision == "f16x3"
    assert "chain probe" in m_lo.illnet_model.diffusion_model.auto_report["overridden_by"]
    assert m_hi.auto_chain_report["kept"] and "f16mx" in (m_hi.illnet_model.diffusion_model.precision, m_hi.refnet_model.diffusion_model.precision)
    assert abs(m_lo.auto_chain_report["rel_l2_chain_vs_f16x3"] - e) <= 1e-3 * e and abs(m_hi.auto_chain_report["rel_l2_chain_vs_f16x3"] - e) <= 1e-3 * e
    x3 = build(1.0).set_precision("f16x3")
    assert torch.equal(out_lo, x3.p_sample_loop(LrK, [LrK], [LrK], **kw)[0])  # flipped: it really runs in f16x3
    assert torch.equal(out_hi, out)
    # explicit probe rows: set_precision("auto", probe=...) measures on them before any sampling; calibrate_precision(probe=...) re-measures on new ones
    hdr = LrK * 1.0e4  # (a 1e4-range HDR refmap batch)
    m_p = build(1.0, probe=hdr)
    rep_p = m_p.calibrate_precision()
    assert rep_p["probe_source"] == "caller" and rep_p["rel_l2_chain_vs_f16x3"] != e
    rep_q = m_p.calibrate_precision(probe=LrK)
    print(f"1e4-range HDR rows: {rep_p['rel_l2_chain_vs_f16x3']:.2e}; ordinary rows {rep_q['rel_l2_chain_vs_f16x3']:.2e}")
    assert rep_q is not rep_p and abs(rep_q["rel_l2_chain_vs_f16x3"] - e) <= 1e-3 * e

    # ObsNet: the conditioning of the first sampler call
    from drmnet_amd.ddim import DDIMSampler

    obs = ObsNetDiffusion(unet_config=unet_t, linear_start=1e-4, linear_end=0.09, log_every_t=2000, timesteps=1000, first_stage_key="LrK",
                          cond_stage_key="raw_refmap", padding_mode="noise", image_size=16, channels=3, concat_mode=True, ddim_steps=50,
                          clip_denoised=False, masked_loss=False, use_ema=False)
    synth.load_synth(obs.model.diffusion_model, 23)
    obs = obs.to(dev).set_precision("auto")
    obs.model.diffusion_model.set_precision_auto(tolerance=1e-2)
    obs._auto_chain.tolerance = 1.0
    smp = DDIMSampler(obs)
    smp.make_schedule(50, ddim_eta=1.0, verbose=False)
    x, _ = smp.ddim_sampling(LrK, tuple(LrK.shape), seed=2, log_every_t=0, verbose=False)
    rep_o = obs.auto_chain_report
    print(f"caller-batch chain probe (tiny ObsNet): {rep_o}")
    assert rep_o["probe_source"] == "caller" and rep_o["probe"].startswith("2x3x16x32 conditioning rows of the caller") and torch.isfinite(x).all()
    eo = rep_o["rel_l2_chain_vs_f16x3"]
    obs2 = ObsNetDiffusion(unet_config=unet_t, linear_start=1e-4, linear_end=0.09, log_every_t=2000, timesteps=1000, first_stage_key="LrK",
                           cond_stage_key="raw_refmap", padding_mode="noise", image_size=16, channels=3, concat_mode=True, ddim_steps=50,
                           clip_denoised=False, masked_loss=False, use_ema=False)
    synth.load_synth(obs2.model.diffusion_model, 23)
    obs2 = obs2.to(dev).set_precision("auto")
    obs2.model.diffusion_model.set_precision_auto(tolerance=1e-2)
    obs2._auto_chain.tolerance = eo * 0.5
    obs2.p_sample_loop(LrK, tuple(LrK.shape), verbose=False, start_T=3, seed=2)  # (the ancestral loop hands its conditioning over too)
    assert not obs2.auto_chain_report["kept"] and obs2.model.diffusion_model.precision == "f16x3" and obs2.auto_chain_report["probe_source"] == "caller"
