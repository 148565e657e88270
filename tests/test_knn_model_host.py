"""The compatness densification and the penalty losses of gsgen_amd.model / gsgen_amd.densify on the CPU, fed the neighbours recorded
in tests/golden/knn (the kNN kernel itself is tested on the emulator, tests/test_knn_host.py, and on the GPU): they reproduce the
reference's own results (tests/golden/make_golden_knn.py) bit for bit."""
import numpy as np
import pytest
import torch

import knn_cases as KC
from gsgen_amd import densify as D
from gsgen_amd import knn as KNN
from gsgen_amd import model as MD


def _golden_neighbours(monkeypatch, table):
    """gsgen_amd.knn's entry points answering with a recorded neighbour table (the CPU has no kernel)"""
    t = torch.as_tensor(table).long()

    def K_nearest_neighbors(mean, K, query=None, return_dist=False):
        assert K == t.shape[1] and mean.shape[0] == t.shape[0]
        return mean.detach()[t[:, 1:]], t[:, 1:]

    def nearest_neighbor(mean):
        assert mean.shape[0] == t.shape[0]
        return mean.detach()[t[:, 1]], t[:, 1]
    monkeypatch.setattr(KNN, "K_nearest_neighbors", K_nearest_neighbors)
    monkeypatch.setattr(KNN, "nearest_neighbor", nearest_neighbor)


def test_compatness_rows_are_the_references():
    z = KC.load("densify_compat")
    raw = {k: torch.tensor(z["before_" + k]) for k in KC.FIELDS}
    new = D.compatness_rows(raw, torch.exp(raw["svec"]), torch.log, torch.tensor(z["knn4_idx"]).long()[:, 1:])
    n = raw["mean"].shape[0]
    assert new["mean"].shape[0] == int(z["n_new"])
    for k in KC.FIELDS:
        np.testing.assert_array_equal(new[k].numpy(), z["after_" + k][n:], err_msg=k)


def test_model_densify_by_compatness_matches_the_reference(monkeypatch):
    z = KC.load("densify_compat")
    _golden_neighbours(monkeypatch, z["knn4_idx"])
    m = KC.model_with_adam(z, "cpu")
    assert m.densify_by_compatness(3) == int(z["n_new"])
    assert m.N == z["after_mean"].shape[0]
    KC.check_after(m, z, bitwise=True)


def test_model_densify_by_shrink_then_compatness_matches_the_reference(monkeypatch):
    z0, z = KC.load("densify_compat"), KC.load("densify_shrink")
    _golden_neighbours(monkeypatch, z0["knn4_idx"])
    m = KC.model_with_adam(z0, "cpu")
    assert m.densify_by_shrink_then_compatness(1.5, 3) == int(z["n_new"])
    KC.check_after(m, z, bitwise=True)


def test_densify_dispatches_on_the_type(monkeypatch):
    """use_legacy + shrink_then_compatness (conf/shrink_then_densify.yaml): the legacy step FIRST, then shrink-then-compatness;
    without use_legacy the type picks one method; the statistics are reset afterwards"""
    z = KC.load("densify_compat")
    calls = []
    for name in ("densify_by_compatness", "densify_by_shrink_then_compatness"):
        monkeypatch.setattr(MD.GaussianSplattingRenderer, name, lambda self, *a, _n=name, **k: calls.append((_n, a, k)) or 0)
    for name in ("densify_legacy", "densify_official"):
        real = getattr(D, name)
        monkeypatch.setattr(D, name, lambda *a, _n=name, _f=real, **k: calls.append((_n,)) or _f(*a, **k))
    base = dict(enabled=True, warm_up=0, end=100, period=10, mean2d_thresh=1e9, split_thresh=0.02)
    for dcfg, want in ((dict(base, type="shrink_then_compatness", use_legacy=True, surface_shrink=2.0, K=4),
                        [("densify_legacy",), ("densify_by_shrink_then_compatness", (2.0,), {"K": 4})]),
                       (dict(base, type="compatness", use_legacy=True), [("densify_legacy",), ("densify_by_compatness", (), {"K": 3})]),
                       (dict(base, type="compatness", use_legacy=False), [("densify_by_compatness", (), {"K": 3})]),
                       (dict(base, type="shrink_then_compatness", use_legacy=False),
                        [("densify_by_shrink_then_compatness", (1.5,), {"K": 3})]),
                       (dict(base, type="official", use_legacy=False), [("densify_official",)]),
                       (dict(base, type="official", use_legacy=True), [("densify_legacy",)])):
        calls.clear()
        m = KC.model_with_adam(z, "cpu", densify=dcfg)
        m.mean_2d_grad_accum.fill_(1.0)
        m.densify(10, verbose=False)
        assert calls == want, (dcfg, calls)
        assert float(m.mean_2d_grad_accum.abs().sum()) == 0.0


def test_densify_legacy_step_runs_before_compatness(monkeypatch):
    """use_legacy + shrink_then_compatness with Gaussians over the gradient threshold: the compatness step sees the legacy step's
    new set (split / cloned rows included), not the old one"""
    z = KC.load("densify_compat")
    seen = []
    monkeypatch.setattr(MD.GaussianSplattingRenderer, "densify_by_shrink_then_compatness",
                        lambda self, *a, **k: seen.append(self.N) or 0)
    dcfg = dict(enabled=True, warm_up=0, end=100, period=10, mean2d_thresh=0.5, split_thresh=0.02, type="shrink_then_compatness",
                use_legacy=True)
    m = KC.model_with_adam(z, "cpu", densify=dcfg)
    n0 = m.N
    m.mean_2d_grad_accum[: n0 // 4] = 1.0
    m.cnt.fill_(1.0)
    grown = m.densify(10, verbose=False)
    assert grown > 0 and seen == [m.N] and m.N > n0


@pytest.mark.parametrize("name", ["alpha_center_weighted", "alpha_uniform_l2", "mean_uniform_l2", "scale", "NN", "compat_l1",
                                  "compat_l2"])
def test_penalties_match_the_reference(monkeypatch, name):
    z = KC.load("penalties")
    n = z["raw_mean"].shape[0]
    _golden_neighbours(monkeypatch, np.stack([np.arange(n), z["nn_idx"]], 1))
    m = KC.model_from_raw({k: z["raw_" + k] for k in KC.FIELDS}, "cpu", penalty=KC.PENALTIES[name])

    class W:
        scalars = {}

        def add_scalar(self, k, v, step):
            self.scalars[k] = float(v)
    w = W()
    loss = m.auxiliary_loss(int(z["step"]), w)
    loss.backward()
    np.testing.assert_array_equal(loss.detach().numpy(), z[name + "_value"])
    for k in KC.FIELDS:
        g = getattr(m, KC.ATTR[k]).grad
        g = torch.zeros_like(getattr(m, KC.ATTR[k])) if g is None else g
        np.testing.assert_allclose(g.numpy(), z[f"{name}_grad_{k}"], rtol=1e-6, atol=1e-9, err_msg=k)
    assert {k: float(v) for k, v in z[name + "_scalars"]} == w.scalars


def test_penalty_schedule_and_unsupported_keys():
    assert MD.schedule_value([0, 2.0, 4.0, 10], 5) == 3.0
    assert MD.schedule_value([2.0, 4.0, 10], 20) == 4.0
    assert MD.schedule_value([0, 1.0, 20.0, 20, "sqrt"], 5) == 20.0 - 19.0 * 0.5
    z = KC.load("penalties")
    raw = {k: z["raw_" + k] for k in KC.FIELDS}
    for key in ("move", "specular", "normal"):
        m = KC.model_from_raw(raw, "cpu", penalty={key: {"value": 1.0}})
        with pytest.raises(NotImplementedError):
            m.auxiliary_loss(0)
        m = KC.model_from_raw(raw, "cpu", penalty={key: {"value": 0.0}, "alpha": {"type": "uniform_l1", "value": 1.0}})
        assert float(m.auxiliary_loss(0)) == pytest.approx(float(m.alpha.mean()))
    assert float(KC.model_from_raw(raw, "cpu").auxiliary_loss(0)) == 0.0


def test_knn_ops_refuse_cpu_tensors_and_bad_K():
    pts = torch.zeros(4, 3)
    for K in (0, 33, 5):  # (outside 1..32, and more neighbours than points: refused before any device is touched)
        with pytest.raises(ValueError, match=f"K = {K}"):
            KNN.knn_points(pts, K)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        KNN.knn_points(torch.zeros(4, 2), 2)
    with pytest.raises(ValueError, match="CUDA"):
        KNN.knn_points(pts, 2)
    with pytest.raises(NotImplementedError):
        KNN.K_nearest_neighbors(pts, 2, query=torch.zeros(2, 3))
