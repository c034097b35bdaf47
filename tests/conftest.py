import os
import sys

# torch's CPU exp / sin / cos / sqrt round as the code branch MKL picks for the host CPU does.  The bit-exact fixtures (the timestep embedding,
# the stress weights' checksums) were recorded on MKL's AVX-512 branch: pin it (MKL conditional numerical reproducibility) before torch loads MKL.
os.environ.setdefault("MKL_CBWR", "AVX512")

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLD = os.path.join(ROOT, "tests", "golden")

# Per-mode bars on a single network forward / sampler state against the reference (rel-L2).  fp32 / f16x3 / f16mx are the modes held to the
# north-star contract (1e-4); f16mx (bench.py's default arithmetic) is asserted at 5e-5 on whole networks, half the contract
# (VERDICT r03 item 1); f16 and bf16 are the reduced-precision modes of BASELINE configs[2] with their own stated tolerances.
NET_TOL = {"fp32": 2e-5, "f16x3": 2e-5, "f16mx": 5e-5, "f16": 5e-3, "bf16": 3e-2}
CONTRACT = 1e-4
ACCURATE_MODES = ["fp32", "f16x3", "f16mx"]
SPLIT_MODES = ["f16x3", "f16mx"]


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """GPU tests fail loudly (not skip) when selected on a box whose GPU/HIP library is missing,
    but are never selected by the CPU run (-m "not gpu")."""
    return


def gold(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def rel_l2(a, b):
    a = torch.as_tensor(a).double().flatten()
    b = torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="session")
def manifests():
    import json

    with open(os.path.join(GOLD, "manifests.json")) as f:
        return json.load(f)
