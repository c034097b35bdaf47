"""float64 numpy restatement of the validation losses (drmnet_amd/csrc/losses.hip), written from their definition: DRMNet.p_losses in eval
mode after the two networks.  Used by tests/test_forward_cpu.py and tests/test_gpu_forward.py; nothing here touches a GPU."""
import math

import numpy as np


def _term(d, loss_type):
    if loss_type == "l1":
        return np.abs(d)
    if loss_type == "l2":
        return d * d
    raise NotImplementedError(loss_type)


def brdf_out(z_out, reversed_k, z0, gamma):
    """(zk_out, zK_out): clamp(z0 + gamma^reversed_k (z_out - z0), 0, 1) and clamp(z_out, 0, 1).  The power is exp(reversed_k ln gamma) in
    float64 rounded to float32, as get_schedule takes it; everything else is float64."""
    z_out, z0 = np.asarray(z_out, dtype=np.float64), np.asarray(z0, dtype=np.float64)
    pw = np.exp(np.asarray(reversed_k, dtype=np.float64) * math.log(gamma)).astype(np.float32).astype(np.float64)[:, None]
    return np.clip(z0 + pw * (z_out - z0), 0.0, 1.0), np.clip(z_out, 0.0, 1.0)


def validation_losses(model_out, Lr_k, Lr_km1, K, z_out, z_k, z_K, reversed_k, z0, gamma, loss_type, l_refmap_weight, l_refcode_weight):
    """-> float64 [3] = (loss_refmap, loss_refcode, loss).  Lr_k is the (noised) input the networks saw.  Rows with K == 0 are selected out
    of loss_refmap before anything is computed on them; no selected row gives NaN."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    sel = np.asarray(K) != 0
    if sel.any():
        loss_refmap = _term(f64(model_out)[sel] - (f64(Lr_km1)[sel] - f64(Lr_k)[sel]), loss_type).mean()
    else:
        loss_refmap = np.nan
    zk_out, zK_out = brdf_out(z_out, reversed_k, z0, gamma)
    loss_refcode = (_term(zk_out - f64(z_k), loss_type).mean() + _term(zK_out - f64(z_K), loss_type).mean()) / 2.0
    return np.array([loss_refmap, loss_refcode, l_refmap_weight * loss_refmap + l_refcode_weight * loss_refcode])
