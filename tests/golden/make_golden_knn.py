"""Generates tests/golden/knn/*.npz from the REFERENCE ITSELF (run in the authoring container only): the reference's
GaussianSplattingRenderer (gs/gaussian_splatting.py, imported through tests/refshim.py) on a CPU cloud of 1600 Gaussians that holds
exact duplicates.

pytorch3d is absent here, so the reference's K_nearest_neighbors / nearest_neighbor (utils/ops.py:104-134) are replaced by a brute
force with the kNN kernel's distance formula (dx*dx + dy*dy + dz*dz, d = p_j - p_i, fp32, left to right) and tie rule (ascending
index): the recorded neighbour order is exactly what gsgen_amd/csrc/knn.hip must produce.  Everything else is the reference's code.

    densify_compat.npz   raw fields and Adam state before, raw fields and Adam state after densify_by_compatness(3), the neighbours
    densify_shrink.npz   raw fields and Adam state after densify_by_shrink_then_compatness(1.5, 3) from the same start
    penalties.npz        each penalty's value and the gradients of the five raw fields, the nearest neighbour of every Gaussian

    python tests/golden/make_golden_knn.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import refshim  # noqa: E402

N = 1600
OUT = os.path.join(HERE, "knn")
FIELDS = ("mean", "qvec", "svec", "color", "alpha")
from knn_cases import PENALTIES, PENALTY_STEP  # noqa: E402  (the penalty configurations the tests replay)


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def cfg_of(d):
    return Cfg({k: cfg_of(v) if isinstance(v, dict) else v for k, v in d.items()})


def model_cfg(penalty=None):
    return cfg_of(dict(device="cpu", svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16,
                       frustum_culling_radius=6.0, tile_culling_type="aabb", tile_culling_thresh=0.01, tile_culling_radius=6.0,
                       T_thresh=1e-4, skip_frustum_culling=False, normal_as_rgb=False, debug=False, depth_detach=True,
                       background=dict(type="fixed", device="cpu", color=[0.1, 0.2, 0.3], random_aug=False,
                                       random_aug_prob=0.0),
                       densify=dict(enabled=True), prune=dict(enabled=False), penalty=penalty or {}))


LR = dict(mean=0.005, qvec=0.003, svec=0.003, color=0.01, alpha=0.003, bg=0.003)
OPT = cfg_of(dict(type="Adam", opt_args=dict(eps=1e-15)))


def cloud():
    """raw fields: a jittered lattice-free cloud with exact duplicates; scales around the spacing so that some neighbour pairs
    touch and others leave a gap"""
    rng = np.random.default_rng(21)
    n0 = N - 100
    mean = rng.normal(size=(n0, 3)).astype(np.float32) * 0.6
    mean = np.concatenate([mean, mean[rng.integers(0, n0, 100)]])  # 100 exact duplicates
    perm = rng.permutation(N)
    mean = mean[perm]
    qvec = rng.normal(size=(N, 4)).astype(np.float32)
    svec = np.log(rng.uniform(0.005, 0.06, (N, 3))).astype(np.float32)
    color = rng.normal(size=(N, 3)).astype(np.float32)
    alpha = rng.normal(size=(N,)).astype(np.float32)
    return dict(mean=mean, qvec=qvec, svec=svec, color=color, alpha=alpha)


def brute_knn(mean, K):
    """(dist2, idx) [N, K] in the kernel's order"""
    p = mean.detach().to(torch.float32)
    d = p[None, :, :] - p[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    bits = d2.contiguous().view(torch.int32).to(torch.int64)
    key = (bits << 32) | torch.arange(p.shape[0], dtype=torch.int64)[None, :]
    k = torch.topk(key, K, dim=1, largest=False, sorted=True).values
    return (k >> 32).to(torch.int32).view(torch.float32), k & 0xFFFFFFFF


@torch.no_grad()
def K_nearest_neighbors(mean, K, query=None, return_dist=False):
    dist, idx = brute_knn(mean, K)
    nn = mean[idx]
    return (nn[:, 1:], idx[:, 1:], dist[:, 1:]) if return_dist else (nn[:, 1:], idx[:, 1:])


@torch.no_grad()
def nearest_neighbor(mean):
    _, idx = brute_knn(mean, 2)
    return mean[idx[:, 1]], idx[:, 1]


class Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, step):
        self.scalars[name] = float(value)


def reference():
    refshim.install()
    dm = types.ModuleType("kornia.geometry.depth")  # utils/ops.py:5 (unused on this path)
    dm.depth_to_3d = None
    sys.modules["kornia.geometry.depth"] = dm
    sys.modules["kornia"].__path__ = []
    sys.modules["kornia.geometry"].__path__ = []
    import gs.gaussian_splatting as M
    M.K_nearest_neighbors = K_nearest_neighbors
    M.nearest_neighbor = nearest_neighbor
    return M


def make_model(M, c, penalty=None, with_adam=True):
    t = {k: torch.tensor(v) for k, v in c.items()}
    t["raw"] = True
    model = M.GaussianSplattingRenderer(model_cfg(penalty), t)
    if with_adam:
        model.setup_lr(LR)
        model.set_optimizer(OPT)
        g = torch.Generator().manual_seed(3)
        for p in list(model.parameters()):  # one Adam step on fixed gradients: every group, bg included, has state
            p.grad = torch.randn(p.shape, generator=g)
        model.optimizer.step()
        model.optimizer.zero_grad(set_to_none=True)
    return model


def raw_of(model):
    return {"mean": model.mean, "qvec": model.qvec, "svec": model.svec_before_activation, "color": model.color_before_activation,
            "alpha": model.alpha_before_activation}


def snapshot(model, prefix, out):
    for k, v in raw_of(model).items():
        out[f"{prefix}_{k}"] = v.detach().numpy().copy()
    for g in model.optimizer.param_groups:
        st = model.optimizer.state.get(g["params"][0], None)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            out[f"{prefix}_adam_{g['name']}_{key}"] = st[key].detach().numpy().copy()


def generate():
    M = reference()
    c = cloud()
    os.makedirs(OUT, exist_ok=True)
    # ---- densify_by_compatness(3)
    model = make_model(M, c)
    res = {}
    snapshot(model, "before", res)
    res["knn4_idx"] = brute_knn(model.mean, 4)[1].numpy().astype(np.int32)
    n_new = model.densify_by_compatness(3)
    snapshot(model, "after", res)
    res["n_new"] = np.array(n_new)
    np.savez_compressed(os.path.join(OUT, "densify_compat.npz"), **res)
    # ---- densify_by_shrink_then_compatness(1.5, 3)
    model = make_model(M, c)
    res = {}
    n_new = model.densify_by_shrink_then_compatness(1.5, 3)  # (the means do not change: densify_compat.npz's knn4_idx holds)
    snapshot(model, "after", res)
    res["n_new"] = np.array(n_new)
    np.savez_compressed(os.path.join(OUT, "densify_shrink.npz"), **res)
    # ---- penalties, one at a time
    res = {"step": np.array(PENALTY_STEP)}
    for k, v in c.items():
        res["raw_" + k] = v
    res["nn_idx"] = brute_knn(torch.tensor(c["mean"]), 2)[1][:, 1].numpy().astype(np.int32)
    for name, pen in PENALTIES.items():
        model = make_model(M, c, pen, with_adam=False)
        w = Writer()
        loss = model.auxiliary_loss(PENALTY_STEP, w)
        loss.backward()
        res[f"{name}_value"] = np.array(loss.detach().numpy(), np.float32)
        for k, p in raw_of(model).items():
            res[f"{name}_grad_{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
        res[f"{name}_scalars"] = np.array(sorted(w.scalars.items()), dtype=object).astype(str)
    np.savez_compressed(os.path.join(OUT, "penalties.npz"), **res)
    return res


if __name__ == "__main__":
    if not refshim.available():
        raise SystemExit("needs /root/reference")
    generate()
    for f in sorted(os.listdir(OUT)):
        z = np.load(os.path.join(OUT, f))
        print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KiB", {k: z[k].shape for k in list(z.keys())[:4]},
              "n_new" in z and int(z["n_new"]))
