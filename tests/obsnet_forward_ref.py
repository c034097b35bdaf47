"""float64 numpy restatement of ObsNet's forward process and diffusion losses (drmnet_amd/csrc/obs_forward.hip), written from their definition:
the conditioning of ObsNetDiffusion.get_input for "masked_LrK", q_sample, and ObsNetDiffusion.p_losses in eval mode after the network.  Used by
tests/test_obsnet_forward_cpu.py and tests/test_gpu_obsnet_forward.py; nothing here touches a GPU."""
import numpy as np

f64 = lambda a: np.asarray(a, dtype=np.float64)


def _term(d, loss_type):
    if loss_type == "l1":
        return np.abs(d)
    if loss_type == "l2":
        return d * d
    raise NotImplementedError(loss_type)


def forward_process(x, mask, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, noisy_observe, padding_mode, e1, e2, e3):
    """x [B, C, H, W], mask [B, 1, H, W], t [B], the draws like x -> (cond, x_noisy, noise) in float64, and the per-element sums of the
    absolute values of the terms of cond and of x_noisy (what a rounding bound on the fp32 kernel scales with)."""
    x, mask = f64(x), f64(mask)
    if mask.shape[-2:] != x.shape[-2:]:
        raise ValueError("the mask must have the size of x")
    if padding_mode not in ("noise", "zeros"):
        raise NotImplementedError(padding_mode)
    terms = [mask * x]
    if noisy_observe > 0:
        terms.append(float(np.float32(noisy_observe)) * f64(e1))
    if padding_mode == "noise":
        terms.append((1.0 - mask) * f64(e2))
    a = f64(sqrt_alphas_cumprod)[np.asarray(t)][:, None, None, None]
    s = f64(sqrt_one_minus_alphas_cumprod)[np.asarray(t)][:, None, None, None]
    q_terms = [a * x, s * f64(e3)]
    return sum(terms), sum(q_terms), f64(e3), sum(np.abs(v) for v in terms), sum(np.abs(v) for v in q_terms)


def per_row_loss(model_out, target, loss_type, invmask=None):
    """L_b: the row mean of f(model_out - target), or sum(f invmask) / (sum(invmask) C) with invmask [B, 1, H, W] (0 / 0 = NaN)."""
    f = _term(f64(model_out) - f64(target), loss_type)
    B, C = f.shape[0], f.shape[1]
    if invmask is None:
        return f.reshape(B, -1).mean(axis=1)
    w = f64(invmask)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f * w).reshape(B, -1).sum(axis=1) / (w.reshape(B, -1).sum(axis=1) * C)


def diffusion_losses(model_out, target, t, logvar, lvlb_weights, loss_type, l_simple_weight, original_elbo_weight, invmask=None):
    """-> float64 [3] = (loss_simple, loss_vlb, loss)."""
    L = per_row_loss(model_out, target, loss_type, invmask)
    t = np.asarray(t)
    lv, w = f64(logvar)[t], f64(lvlb_weights)[t]
    loss_simple = L.mean()
    loss_vlb = (w * L).mean()
    return np.array([loss_simple, loss_vlb, l_simple_weight * (L / np.exp(lv) + lv).mean() + original_elbo_weight * loss_vlb])


def masked_rms(a, invmask):
    """sqrt(mean_b sum(a^2 invmask) / (sum(invmask) C)): the rms under the weighting of the masked loss."""
    return float(np.sqrt(per_row_loss(a, np.zeros_like(f64(a)), "l2", invmask).mean()))


def nearest_indices(src, dst):
    """OpenCV's INTER_NEAREST rule per axis: source index = min(floor(dst_index * src / dst), src - 1)."""
    return np.minimum(np.floor(np.arange(dst) * (src / dst)).astype(np.int64), src - 1)
