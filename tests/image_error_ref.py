"""float64 numpy restatement of the image-space error sums (drmnet_amd/csrc/image_error.hip) and of the figures made from them
(drmnet_amd/relight.py: image_errors_batch), written from their definition in include/drmnet_hip.h.  It takes nothing from drmnet_amd.
Used by tests/test_image_error_cpu.py and tests/test_gpu_image_error.py; the CPU file checks it against relight.image_errors."""
import numpy as np

SUMS = ("n", "aa", "bb", "ab", "l2", "n_log", "d", "dd", "l2_scaled", "dd_centred")
FIGURES = ("n", "rel_l2", "scale", "rel_l2_scaled", "rmse_log10", "n_log", "rmse_log10_scaled")
COUNTS = ("n", "n_log")
RTOL, ATOL = 1e-10, 1e-12  # the bar of the GPU tests: |got - want| <= RTOL |want| + ATOL on every figure, counts exact


def error_sums(a, b, mask) -> np.ndarray:
    """the ten sums of one pair: a, b [..., 3] (channel-last), mask [...] (non-zero = counted), two passes in float64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.asarray(mask) != 0
    assert a.shape == b.shape and a.shape[-1] == 3 and m.shape == a.shape[:-1], (a.shape, b.shape, m.shape)
    a, b = a[m], b[m]
    s = np.zeros(len(SUMS))
    s[0] = m.sum()
    s[1], s[2], s[3], s[4] = np.sum(a * a), np.sum(b * b), np.sum(a * b), np.sum((a - b) ** 2)
    both = (a > 0) & (b > 0)
    with np.errstate(invalid="ignore"):
        d = np.log10(a[both]) - np.log10(b[both])
        s[5], s[6], s[7] = both.sum(), np.sum(d), np.sum(d * d)
        scale = s[3] / s[1] if s[1] > 0 else 0.0
        mean = s[6] / s[5] if s[5] > 0 else 0.0
        s[8] = np.sum((scale * a - b) ** 2)
        s[9] = np.sum((d - mean) ** 2)
    return s


def errors(s) -> dict:
    """the figures of relight.image_errors from the ten sums, with its zero-denominator rules, and rmse_log10_scaled"""
    s = np.asarray(s, dtype=np.float64)
    assert s.shape == (len(SUMS),)
    nb = np.sqrt(s[2])

    def rel(dsq):
        d = np.sqrt(dsq)
        return float(d / nb) if nb > 0 else (0.0 if d == 0 else float("inf"))

    return {"n": int(s[0]), "rel_l2": rel(s[4]), "scale": float(s[3] / s[1]) if s[1] > 0 else 0.0, "rel_l2_scaled": rel(s[8]),
            "rmse_log10": float(np.sqrt(s[7] / s[5])) if s[5] > 0 else 0.0, "n_log": int(s[5]),
            "rmse_log10_scaled": float(np.sqrt(s[9] / s[5])) if s[5] > 0 else 0.0}


def difference(got: dict, want: dict, keys=FIGURES) -> float:
    """asserts the bar on every figure of ``keys`` (counts exact, a non-finite figure the same non-finite figure) -> the largest
    |got - want| / (|want| + ATOL / RTOL) met: the difference relative to the figure, and the bar is RTOL on that scale"""
    worst = 0.0
    for k in keys:
        g, w = got[k], want[k]
        if k in COUNTS:
            assert g == w, (k, g, w)
        elif not np.isfinite(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (k, g, w)
        else:
            assert abs(g - w) <= RTOL * abs(w) + ATOL, (k, g, w, abs(g - w))
            worst = max(worst, abs(g - w) / (abs(w) + ATOL / RTOL))
    return worst


def images(seed: int, count: int, H: int, W: int, holes: int = 3) -> np.ndarray:
    """``count`` float32 images [count, H, W, 3], log-uniform in [1e-4, 1e2], with up to ``holes`` entries per image set to 0 or below (they
    drop out of the log terms)"""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-4.0, 2.0, size=(count, H, W, 3))).astype(np.float32)
    for i in range(count):
        flat = x[i].reshape(-1)
        at = rng.choice(flat.size, size=min(holes, flat.size // 3), replace=False)
        flat[at] = np.array([0.0, -0.25, -3.0], dtype=np.float32)[: len(at)]
    return x


def masks(seed: int, H: int, W: int) -> np.ndarray:
    """uint8 [3, H, W]: full, empty, scattered (about half the pixels, other values than 1 among them)"""
    rng = np.random.default_rng(seed)
    scattered = (rng.random((H, W)) < 0.5) * rng.integers(1, 255, size=(H, W))
    return np.stack([np.ones((H, W)), np.zeros((H, W)), scattered]).astype(np.uint8)
