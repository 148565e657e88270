"""Generates tests/golden/densify/densify_modes.npz from the REFERENCE ITSELF (run where the reference's tree is present): its
GaussianSplattingRenderer.densify() + .prune() (gs/gaussian_splatting.py, imported through tests/refshim.py) on the five cases
of tests/test_densify.py -- the raw fields, the Adam moments and the densify statistics they leave behind, as
"<mode>__<name>" arrays.  tests/test_densify.py compares gsgen_amd.densify with these where the reference is absent.

    python tests/golden/make_golden_densify.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import refshim  # noqa: E402
import test_densify as TD  # noqa: E402


def generate():
    import types
    refshim.install()
    dm = types.ModuleType("kornia.geometry.depth")  # (what the test's fixture stubs, too)
    dm.depth_to_3d = None
    sys.modules["kornia.geometry.depth"] = dm
    sys.modules["kornia"].__path__ = []
    sys.modules["kornia.geometry"].__path__ = []
    import gs.gaussian_splatting as M
    out = {}
    for mode in TD.MODES:
        for name, v in TD.reference_outcome(M, mode).items():
            out[f"{mode}__{name}"] = v.numpy()
    os.makedirs(os.path.dirname(TD.GOLDEN), exist_ok=True)
    np.savez_compressed(TD.GOLDEN, **out)
    print(TD.GOLDEN, {m: int(out[f"{m}__N"]) for m in TD.MODES})


if __name__ == "__main__":
    if not refshim.available():
        raise SystemExit("needs the reference's tree")
    generate()
