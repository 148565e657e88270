"""Writes tests/golden/mesh/*.npz: small fields and the mesh the reference's own marching cubes (shap_e/rendering/mc.py, torch on
the CPU) makes of them.  Run once by hand, never by the tests:

    python tests/golden/make_golden_mesh.py /path/to/reference

Each file holds `field` (float32 [X,Y,Z]), `thresh` (float32 scalar), `verts` (float32 [V,3]) and `faces` (uint16 [F,3]): the
reference is called on `field - thresh` (fp32) with min_point = 0 and size = shape - 1, so its vertices are in lattice index
coordinates.  Every axis has n - 1 a power of two, which makes the reference's v / (n - 1) * (n - 1) round trip exact, and no
field value equals its threshold.  The reference's mesh.py imports `blobfile` for file output that is not used here: an empty
module of that name stands in for it.
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh")


def fields():
    ax = np.linspace(-1.0, 1.0, 17)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    f = {}
    f["sphere"] = (0.45 - (x * x + y * y + z * z), 0.0)
    f["torus"] = (0.04 - ((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z), 0.0)
    blob = lambda cx, cy, cz, s: np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))  # noqa: E731
    f["blobs"] = (blob(-0.3, -0.1, 0.0, 0.3) + blob(0.35, 0.2, 0.1, 0.25) - 0.5, 0.0)
    # the same two blobs as a density with the surface at 0.5: the non-zero threshold
    f["blobs_thresh"] = (blob(-0.3, -0.1, 0.0, 0.3) + blob(0.35, 0.2, 0.1, 0.25), 0.5)

    def noise(shape, seed):
        g = np.full(shape, -1.0)
        inner = tuple(slice(1, n - 1) for n in shape)
        g[inner] = np.random.default_rng(seed).standard_normal(g[inner].shape)
        return g
    f["noise"] = (noise((17, 17, 17), 2), 0.0)
    f["noise_17x5x9"] = (noise((17, 5, 9), 3), 0.0)
    f["noise_3x17x2"] = (np.random.default_rng(4).standard_normal((3, 17, 2)), 0.0)  # (no room for a border: an open mesh)
    return {k: (np.ascontiguousarray(v, np.float32), np.float32(t)) for k, (v, t) in f.items()}


def main(reference):
    sys.path.insert(0, reference)
    sys.modules.setdefault("blobfile", types.ModuleType("blobfile"))
    from shap_e.rendering.mc import marching_cubes
    os.makedirs(OUT, exist_ok=True)
    for name, (field, thresh) in fields().items():
        s = field - thresh
        assert s.dtype == np.float32 and (s != 0).all() and all((n - 1) & (n - 2) == 0 for n in field.shape)
        size = torch.tensor([n - 1 for n in field.shape], dtype=torch.float32)
        mesh = marching_cubes(torch.from_numpy(s), torch.zeros(3), size)
        verts, faces = mesh.verts.numpy().astype(np.float32), mesh.faces.numpy()
        assert faces.max(initial=0) < 65536
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, field=field, thresh=thresh, verts=verts, faces=faces.astype(np.uint16))
        print(f"{name}: {field.shape} V {len(verts)} F {len(faces)} {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main(sys.argv[1])
