"""Shared set-up of the kNN model tests (tests/test_knn_model_host.py on the CPU, tests/test_gpu_knn.py on the GPU): this repo's
GaussianSplattingRenderer in the state tests/golden/make_golden_knn.py put the reference's into, and the comparisons."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn")
FIELDS = ("mean", "qvec", "svec", "color", "alpha")
ATTR = {"mean": "mean", "qvec": "qvec", "svec": "svec_before_activation", "color": "color_before_activation",
        "alpha": "alpha_before_activation"}
PENALTIES = {  # name -> the cfg.penalty node it configures alone
    "alpha_center_weighted": {"alpha": {"type": "center_weighted", "value": 100.0}},
    "alpha_uniform_l2": {"alpha": {"type": "uniform_l2", "value": [0, 2.0, 4.0, 10]}},
    "mean_uniform_l2": {"mean": {"type": "uniform_l2", "value": 0.5}},
    "scale": {"scale": {"value": 3.0}},
    "NN": {"NN": {"value": 2.0}},
    "compat_l1": {"compat": {"type": "l1", "value": 10.0}},
    "compat_l2": {"compat": {"type": "l2", "value": [0, 1.0, 20.0, 20, "sqrt"]}},
}
PENALTY_STEP = 5
LR = dict(mean=0.005, qvec=0.003, svec=0.003, color=0.01, alpha=0.003, bg=0.003)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def cfg(device, penalty=None, densify=None):
    return dict(device=device, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4,
                depth_detach=True, background=dict(type="fixed", color=[0.1, 0.2, 0.3]),
                densify=densify or dict(enabled=True), prune=dict(enabled=False), penalty=penalty or {})


def model_from_raw(raw, device, penalty=None, densify=None):
    from gsgen_amd.model import GaussianSplattingRenderer
    t = {k: torch.tensor(np.ascontiguousarray(raw[k]), device=device) for k in FIELDS}
    t["raw"] = True
    return GaussianSplattingRenderer(cfg(device, penalty, densify), t)


def model_with_adam(z, device, densify=None):
    """the golden 'before' state: raw fields + one Adam step's state in every group (bg included)"""
    m = model_from_raw({k: z["before_" + k] for k in FIELDS}, device, densify=densify)
    m.setup_lr(LR)
    m.set_optimizer(dict(type="Adam", opt_args=dict(eps=1e-15)))
    params = {"bg": m.bg.bg_color, **{k: getattr(m, ATTR[k]) for k in FIELDS}}
    for name, p in params.items():
        m.optimizer.state[p] = {"step": torch.tensor(z[f"before_adam_{name}_step"]),  # (torch keeps Adam's step on the CPU)
                                **{key: torch.tensor(z[f"before_adam_{name}_{key}"], device=device) for key in ("exp_avg", "exp_avg_sq")}}
    return m


def check_after(m, z, bitwise, ref_bg=None):
    """raw fields and Adam state of the model against the golden 'after' record"""
    def eq(got, want, what):
        got = got.detach().cpu().numpy()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if bitwise:
            np.testing.assert_array_equal(got, want, err_msg=what)
        else:
            np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6, err_msg=what)
    for k in FIELDS:
        eq(getattr(m, ATTR[k]), z["after_" + k], k)
    groups = {g["name"]: g["params"][0] for g in m.optimizer.param_groups}
    for k in FIELDS:
        assert groups[k] is getattr(m, ATTR[k]), f"optimiser group {k} does not hold the new parameter"
    for name in ("bg",) + FIELDS:
        st = m.optimizer.state[groups[name]]
        for key in ("exp_avg", "exp_avg_sq", "step"):
            eq(st[key], z[f"after_adam_{name}_{key}"], f"adam {name} {key}")
