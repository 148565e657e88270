"""Vertex normals and colours of the exported mesh on the MI355X (gsgen_amd.mesh.vertex_attributes, colored_density_mesh,
colored_mesh_from_ckpt, GaussianSplattingRenderer.to_mesh) and their way into .obj and .ply files, on the seeded cloud of
test_gpu_mesh.test_density_mesh_and_mesh_from_ckpt_on_a_seeded_cloud (N = 200, seed 200, L = 1.5, reso 33)."""
import numpy as np
import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu

from gsgen_amd import io as GIO  # noqa: E402
from gsgen_amd import mesh as GM  # noqa: E402

DEV = "cuda"
N, L, RESO = 200, 1.5, 33


def seeded_ckpt():
    gen = torch.Generator().manual_seed(200)
    ckpt = {"mean": (torch.randn(N, 3, generator=gen) * 0.3).clamp(-0.7, 0.7), "qvec": torch.randn(N, 4, generator=gen),
            "svec": torch.log(0.1 + 0.1 * torch.rand(N, 3, generator=gen)), "alpha": torch.full((N,), 2.0)}
    ckpt["color"] = torch.randn(N, 3, generator=gen)  # (drawn after the fields of the geometry test: they are its draws)
    return {k: v.to(DEV) for k, v in ckpt.items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def test_normals_agree_with_the_winding_and_colours_lie_in_the_hull():
    """The field K = 8, skip_nearest = False (continuous where the eight nearest do not change; the reference's own K = 3 with the
    nearest dropped is not: DESIGN.md "Vertex normals and colours").  At most 0.1 % of the triangles may have the mean of their
    three vertex normals point against their face normal (fp64 on the CPU: 0 of 3 744); every normal has unit length within 1e-6;
    every colour lies within [min, max] of the colours of the vertex's eight nearest centres; the result is field_at's."""
    from gsgen_amd.density import field_at
    from gsgen_amd.knn import knn_raw
    c = seeded_ckpt()
    scale, opacity, color = torch.exp(c["svec"]), torch.sigmoid(c["alpha"]), torch.sigmoid(c["color"])
    verts, tris, normals, colors = GM.colored_density_mesh(c["mean"], c["qvec"], scale, opacity, color, L, RESO, K=8, skip_nearest=False)
    pv, pt = GM.density_mesh(c["mean"], c["qvec"], scale, opacity, L, RESO, K=8, skip_nearest=False)
    assert torch.equal(bits(verts), bits(pv)) and torch.equal(tris, pt) and tris.shape[0] > 1000
    assert normals.shape == verts.shape and colors.shape == verts.shape and normals.dtype == torch.float32
    length = normals.double().norm(dim=1)
    print(f"normals: | |n| - 1 | max {float((length - 1).abs().max()):.3e}")
    assert float((length - 1).abs().max()) <= 1e-6
    v, t, n = verts.double().cpu(), tris.long().cpu(), normals.double().cpu()
    face = torch.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]], dim=1)
    against = ((n[t].mean(1) * face).sum(1) <= 0).sum().item()
    print(f"normals against the winding: {against} of {t.shape[0]} triangles")
    assert against <= 0.001 * t.shape[0]
    _, idx = knn_raw(c["mean"], 8, query=verts)
    near = color[idx.long()]  # [V, 8, 3]
    assert bool((colors >= near.min(1).values).all()) and bool((colors <= near.max(1).values).all())
    f = field_at(c["mean"], c["qvec"], scale, opacity, verts, 8, False, color=color)
    assert torch.equal(bits(colors), bits(f.rgb))
    want = -f.grad.double() / f.grad.double().norm(dim=1, keepdim=True)
    assert float((normals.double() - want).abs().max()) <= 1e-6
    n2, c2 = GM.vertex_attributes(verts, c["mean"], c["qvec"], scale, opacity, color, 8, False)
    assert torch.equal(bits(n2), bits(normals)) and torch.equal(bits(c2), bits(colors))
    n3, c3 = GM.vertex_attributes(verts, c["mean"], c["qvec"], scale, opacity, None, 8, False)
    assert c3 is None and torch.equal(bits(n3), bits(normals))


def test_zero_gradients_and_empty_meshes():
    c = seeded_ckpt()
    scale, opacity, color = torch.exp(c["svec"]), torch.sigmoid(c["alpha"]), torch.sigmoid(c["color"])
    far = torch.tensor([[1e6, 0.0, 0.0], [float("nan"), 0.0, 0.0], [0.0, 0.0, 0.1]], device=DEV)
    n, col = GM.vertex_attributes(far, c["mean"], c["qvec"], scale, opacity, color)
    assert bool((n[:2] == 0).all()) and abs(float(n[2].norm()) - 1) <= 1e-6  # underflown and non-finite: zero normals
    assert bool((col[1] == 0).all()) and bool(torch.isfinite(col).all())
    v, t, n, col = GM.colored_density_mesh(c["mean"], c["qvec"], scale, opacity, color, L, RESO, thresh=1e9)  # nothing inside
    assert v.shape == t.shape == n.shape == col.shape == (0, 3) and n.dtype == torch.float32 and n.is_cuda
    n, col = GM.vertex_attributes(v, c["mean"], c["qvec"], scale, opacity)
    assert n.shape == (0, 3) and col is None


def test_ckpt_and_model_entry_points_and_the_files(tmp_path):
    c = seeded_ckpt()
    pv, pt, pL = GM.mesh_from_ckpt(c, reso=RESO, K=3, thresh=0.5, L=L)
    verts, tris, normals, colors, gotL = GM.colored_mesh_from_ckpt(c, reso=RESO, K=3, thresh=0.5, L=L)
    assert gotL == pL == L and torch.equal(bits(verts), bits(pv)) and torch.equal(tris, pt)  # the geometry did not move by a bit
    n2, c2 = GM.vertex_attributes(verts, c["mean"], c["qvec"], torch.exp(c["svec"]), torch.sigmoid(c["alpha"]), torch.sigmoid(c["color"]),
                                  3, True)
    assert torch.equal(bits(n2), bits(normals)) and torch.equal(bits(c2), bits(colors))
    import gsgen_amd
    assert gsgen_amd.colored_mesh_from_ckpt is GM.colored_mesh_from_ckpt and gsgen_amd.vertex_attributes is GM.vertex_attributes
    assert gsgen_amd.colored_density_mesh is GM.colored_density_mesh
    raw = {k: c[k].cpu().numpy() for k in ("mean", "qvec", "svec", "alpha", "color")}
    m = KC.model_from_raw(raw, DEV)
    obj, ply = tmp_path / "model.obj", tmp_path / "model.ply"
    mv, mt, mn, mc, mL = m.to_mesh(reso=RESO, K=3, thresh=0.5, L=L, path=obj)
    assert mL == L and torch.equal(bits(mv), bits(verts)) and torch.equal(mt, tris)
    assert torch.equal(bits(mn), bits(normals)) and torch.equal(bits(mc), bits(colors))
    auto = m.to_mesh(reso=RESO, path=ply)
    assert auto[4] == c["mean"].abs().max().item() * 1.1 and auto[1].shape[0] > 100
    with pytest.raises(ValueError, match="obj"):
        m.to_mesh(reso=RESO, L=L, path=tmp_path / "model.stl")
    hv, ht, hn, hc = (x.cpu().numpy() for x in (verts, tris, normals, colors))
    assert 0 < hc.min() and hc.max() < 1  # (sigmoid colours: the writers' clip does nothing)
    rv, rt, rn, rc = GIO.read_obj_attributes(obj)
    assert rv.tobytes() == hv.tobytes() and np.array_equal(rt, ht) and rn.tobytes() == hn.tobytes() and rc.tobytes() == hc.tobytes()
    ov, ot = GIO.read_obj(obj)  # the plain reader: the geometry of the coloured file
    assert ov.tobytes() == hv.tobytes() and np.array_equal(ot, ht)
    GIO.write_ply_mesh(ply, verts, tris, normals, colors)
    qv, qt, qn, qc = GIO.read_ply_mesh(ply)
    assert qv.tobytes() == hv.tobytes() and np.array_equal(qt, ht) and qn.tobytes() == hn.tobytes()
    assert qc.dtype == np.uint8 and np.array_equal(qc, np.rint(hc.astype(np.float64) * 255).astype(np.uint8))
    GIO.write_obj(tmp_path / "plain.obj", verts, tris)  # without attributes: the bytes of the writer as it was
    text = "".join("v %.9g %.9g %.9g\n" % tuple(r) for r in hv.astype(np.float64).tolist()) + "".join("f %d %d %d\n" % tuple(r) for r in (ht + 1).tolist())
    assert (tmp_path / "plain.obj").read_bytes() == text.encode()
