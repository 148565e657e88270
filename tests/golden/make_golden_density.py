"""Generates tests/golden/density/density_grid.npz from the REFERENCE ITSELF (run in the authoring container only): the reference's
get_density_val_grid_from_ckpt (utils/export.py:66-120, imported through tests/refshim.py) on the CPU, on a checkpoint of 1600
Gaussians at reso = 24, K = 3.

pytorch3d is absent here, so the K_nearest_neighbors the reference calls (utils/ops.py:117-134) is replaced by a brute force with
the kNN kernel's distance formula (dx*dx + dy*dy + dz*dz, d = p_j - q, fp32, left to right) and tie rule (ascending index), column 0
dropped as the reference drops it.  The means are continuous random draws without duplicates, so no lattice point is equidistant
from two centres and the neighbour set does not hang on the tie rule.  Everything else is the reference's code: its linspace
lattice, qsvec2covmat_batched, torch.inverse of the fp32 covariance, its bmm chain.

The fixture holds the raw fields, L, the lattice axis (the reference's torch.linspace on the CPU: a device linspace need not give
the same bits), the reference's grid, the fp64 restatement's grid with its per-point rounding bound (tests/density_cases.py), and
the reference's own max-abs and RMS error against fp64.

    python tests/golden/make_golden_density.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import refshim  # noqa: E402
import density_cases as DC  # noqa: E402

N, RESO, K = 1600, 24, 3
OUT = os.path.join(HERE, "density")


def checkpoint():
    rng = np.random.default_rng(33)
    return dict(mean=(rng.normal(size=(N, 3)) * 0.6).astype(np.float32), qvec=rng.normal(size=(N, 4)).astype(np.float32),
                svec=np.log(rng.uniform(0.005, 0.06, (N, 3))).astype(np.float32), alpha=rng.normal(size=(N,)).astype(np.float32))


@torch.no_grad()
def K_nearest_neighbors(mean, K, query=None, return_dist=False):
    q = mean if query is None else query
    d2, idx = DC.brute_query(mean.numpy(), q.numpy(), K)
    idx = torch.from_numpy(idx.astype(np.int64))
    nn = mean[idx]
    return (nn[:, 1:], idx[:, 1:], torch.from_numpy(d2)[:, 1:]) if return_dist else (nn[:, 1:], idx[:, 1:])


def reference():
    refshim.install()
    dm = types.ModuleType("kornia.geometry.depth")  # utils/ops.py:5 (unused on this path)
    dm.depth_to_3d = None
    sys.modules["kornia.geometry.depth"] = dm
    sys.modules["kornia"].__path__ = []
    sys.modules["kornia.geometry"].__path__ = []
    if "plyfile" not in sys.modules:  # utils/export.py:10 (to_ply only)
        try:
            import plyfile  # noqa: F401
        except ImportError:
            pm = types.ModuleType("plyfile")
            pm.PlyData = pm.PlyElement = None
            sys.modules["plyfile"] = pm
    import utils.export as E
    E.K_nearest_neighbors = K_nearest_neighbors
    E.trange = range  # (no progress bar)
    return E


def generate():
    E = reference()
    c = checkpoint()
    assert np.unique(c["mean"], axis=0).shape[0] == N
    ckpt = {k: torch.tensor(v) for k, v in c.items()}
    grid, L = E.get_density_val_grid_from_ckpt(ckpt, reso=RESO, K=K)
    axis = torch.linspace(-L, L, RESO).numpy()
    pts = DC.lattice(axis, axis, axis)
    d2, idx = DC.brute_query(c["mean"], pts, K + 1)
    assert (d2[:, 1:] > d2[:, :-1]).all(), "a lattice point equidistant from two centres: draw other means"
    scale = torch.exp(ckpt["svec"]).numpy()  # (the activations as torch rounds them: what the fp64 restatement starts from)
    opacity = torch.sigmoid(ckpt["alpha"]).numpy()
    g64, bound = DC.density64(c["mean"], c["qvec"], scale, opacity, pts, DC.kept(idx, K, 1))
    ref = grid.numpy().reshape(-1)
    err = np.abs(ref.astype(np.float64) - g64)
    res = dict(c, L=np.array(L, np.float64), axis=axis, reso=np.array(RESO), K=np.array(K), scale=scale, opacity=opacity,
               grid_ref=ref.reshape(RESO, RESO, RESO), grid64=g64.reshape(RESO, RESO, RESO), bound=bound.reshape(RESO, RESO, RESO),
               nn_idx=idx, ref_max_abs=np.array(err.max()), ref_rms=np.array(np.sqrt((err ** 2).mean())))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "density_grid.npz"), **res)
    return res


if __name__ == "__main__":
    if not refshim.available():
        raise SystemExit("needs /root/reference")
    r = generate()
    f = os.path.join(OUT, "density_grid.npz")
    print(os.path.getsize(f) // 1024, "KiB", "L", float(r["L"]), "grid max", float(r["grid64"].max()), "nonzero", int((r["grid64"] > 0).sum()),
          "reference max|err|", float(r["ref_max_abs"]), "rms", float(r["ref_rms"]),
          "reference points beyond the bound", int((np.abs(r["grid_ref"].astype(np.float64) - r["grid64"]) > r["bound"]).sum()))
