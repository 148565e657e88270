"""On-disk formats of the reference: the trainer's checkpoint
(trainer.py:255-266), the 17-field float32 `.ply` (utils/export.py:157-203) and the 32-byte-record
`.splat` of the web viewer sorted by volume * opacity (utils/export.py:206-283).  Host code only,
vectorised (the reference packs record by record with struct.pack); byte-identical output.  Also the
Wavefront `.obj` that `to_mesh` writes through mcubes.export_obj (utils/export.py:123-155), with optional vertex normals and colours
(gsgen_amd.mesh.vertex_attributes), and the same mesh as a binary `.ply` (write_ply_mesh).

`params` is the dict the reference saves under "params": raw (pre-activation) tensors or arrays
mean [N,3], qvec [N,4] (w,x,y,z), svec [N,3] (log scale), color [N,3] (logit), alpha [N] (logit).
"""
import numpy as np

PLY_FIELDS = ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "opacity", "scale_0", "scale_1", "scale_2",
              "rot_0", "rot_1", "rot_2", "rot_3")
SPLAT_DTYPE = np.dtype([("pos", "<f4", 3), ("scale", "<f4", 3), ("rgba", "u1", 4), ("rot", "u1", 4)])


def _np(params, key):
    v = params[key]
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v, np.float32)


def _sigmoid(x):
    """torch.sigmoid, as utils/export.py uses it: the u8 truncation that follows is sensitive to the last bit, and
    a numpy 1 / (1 + exp(-x)) differs from torch's kernel on rare values"""
    import torch
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


# ---- checkpoint ---------------------------------------------------------------------------------
def save_checkpoint(path, params, cfg=None, step=0):
    """{"params", "cfg", "step"} through torch.save, as Trainer.save (trainer.py:255-266)."""
    import torch
    state = {"params": {k: (v if hasattr(v, "detach") else torch.as_tensor(np.asarray(v))) for k, v in params.items()},
             "cfg": cfg if cfg is not None else {}, "step": int(step)}
    torch.save(state, path)


def load_checkpoint(path, map_location="cpu"):
    """-> (params, cfg, step); accepts both the wrapped and the bare-params layout the reference's
    exporters accept (utils/export.py:163-165)."""
    import torch
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    if "params" in ckpt:
        return ckpt["params"], ckpt.get("cfg"), ckpt.get("step", 0)
    return ckpt, None, 0


# ---- .ply -----------------------------------------------------------------------------------------
def ply_table(params):
    """[N,17] float32 in PLY_FIELDS order; raw parameter values, colour scaled by 255
    (utils/export.py:185-195: no activations applied, normals zero)."""
    pos = _np(params, "mean")
    rgb = _np(params, "color") * np.float32(255.0)
    opacity = _np(params, "alpha").reshape(-1, 1)
    return np.concatenate((pos, np.zeros_like(pos), rgb, opacity, _np(params, "svec"), _np(params, "qvec")), axis=1)


def write_ply(path, params):
    """binary_little_endian PLY, one `vertex` element of 17 float properties (what
    plyfile.PlyData([PlyElement.describe(elements, "vertex")]).write() produces)."""
    tab = np.ascontiguousarray(ply_table(params), "<f4")
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {tab.shape[0]}"]
    header += [f"property float {name}" for name in PLY_FIELDS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(tab.tobytes())


def read_ply(path):
    """-> dict of raw parameter arrays (inverse of write_ply)."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "binary_little_endian" not in lines[1]:
        raise ValueError("not a binary little-endian PLY")
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    names = [ln.split()[2] for ln in lines if ln.startswith("property float")]
    if tuple(names) != PLY_FIELDS:
        raise ValueError(f"unexpected properties {names}")
    tab = np.frombuffer(blob, "<f4", count=n * 17, offset=end).reshape(n, 17)
    return {"mean": tab[:, 0:3].copy(), "color": tab[:, 6:9] / np.float32(255.0), "alpha": tab[:, 9].copy(),
            "svec": tab[:, 10:13].copy(), "qvec": tab[:, 13:17].copy()}


# ---- .splat -------------------------------------------------------------------------------------
def splat_records(params):
    """The records of utils/export.py:241-281 as a structured array, in file order:
    position f32x3 | exp(svec) f32x3 | sigmoid(color), sigmoid(alpha) * 255 truncated to u8 |
    normalised quaternion * 128 + 128 truncated to u8 (a component of exactly 1.0 wraps to 0, as in
    the reference); sorted by prod(scale) * opacity_u8 descending, ties in index order."""
    pos = _np(params, "mean")
    rgb = (_sigmoid(_np(params, "color")) * 255.0).astype(np.uint8).clip(0, 255)
    opacity = (_sigmoid(_np(params, "alpha")).reshape(-1, 1) * 255.0).astype(np.uint8).clip(0, 255)
    svec = np.exp(_np(params, "svec"))
    qvec = _np(params, "qvec")
    qvec = qvec / np.linalg.norm(qvec, axis=1, keepdims=True)
    qvec = (qvec * 128 + 128).astype(np.uint8).clip(0, 255)
    volume = np.prod(svec, axis=1) * opacity[..., 0]
    # sorted(range(n), key=volume, reverse=True) is stable: equal keys keep ascending index
    order = np.argsort(-volume.astype(np.float64), kind="stable")
    rec = np.empty(pos.shape[0], SPLAT_DTYPE)
    rec["pos"], rec["scale"] = pos[order], svec[order]
    rec["rgba"][:, :3], rec["rgba"][:, 3] = rgb[order], opacity[order, 0]
    rec["rot"] = qvec[order]
    return rec


def write_splat(path, params):
    splat_records(params).tofile(path)


def read_splat(path):
    return np.fromfile(path, SPLAT_DTYPE)


# ---- .obj -----------------------------------------------------------------------------------------
def _mesh_arrays(who, verts, tris, normals, colors):
    """host arrays of a mesh, checked: verts [V,3] float32, tris [F,3] int64, normals / colors [V,3] float32 or None"""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a  # noqa: E731
    v, t = np.asarray(host(verts), np.float32).reshape(-1, 3), np.asarray(host(tris), np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"gsgen_amd.io.{who}: triangle indices {t.min()}..{t.max()} for {len(v)} vertices")
    attrs = []
    for name, a in (("normals", normals), ("colors", colors)):
        if a is not None:
            a = np.asarray(host(a), np.float32).reshape(-1, 3)
            if len(a) != len(v):
                raise ValueError(f"gsgen_amd.io.{who}: {len(a)} {name} for {len(v)} vertices")
        attrs.append(a)
    return v, t, attrs[0], attrs[1]


def write_obj(path, verts, tris, normals=None, colors=None):
    """`v x y z` lines, then `f a b c` lines with 1-based vertex indices: the layout of mcubes.export_obj.  verts [V,3] and tris
    [F,3] are tensors or arrays.  Coordinates are written with 9 significant digits, which identify a float32: read_obj returns the
    same bits.  colors [V,3] go on the vertex line, `v x y z r g b`, clipped to [0, 1] (the widely read extension of the format);
    normals [V,3] go as `vn` lines after the vertices, one per vertex, and the faces become `f a//a b//b c//c`.  With neither, the
    file is what mcubes.export_obj writes."""
    v, t, n, c = _mesh_arrays("write_obj", verts, tris, normals, colors)
    with open(path, "w") as f:
        if c is None:
            f.write("".join("v %.9g %.9g %.9g\n" % (x, y, z) for x, y, z in v.astype(np.float64).tolist()))
        else:
            vc = np.concatenate((v, np.clip(c, np.float32(0), np.float32(1))), axis=1).astype(np.float64)
            f.write("".join("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(row) for row in vc.tolist()))
        if n is None:
            f.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in (t + 1).tolist()))
        else:
            f.write("".join("vn %.9g %.9g %.9g\n" % (x, y, z) for x, y, z in n.astype(np.float64).tolist()))
            f.write("".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (t + 1).tolist()))


def read_obj(path):
    """-> (verts float32 [V,3], tris int64 [F,3], 0-based) of a file of `v` and triangular `f` lines; `f` entries may carry
    /texture/normal suffixes, which are dropped; other lines are ignored"""
    v, t = [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"gsgen_amd.io.read_obj: {path}: a face of {len(p) - 1} vertices (triangles only)")
                t.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float64).reshape(-1, 3).astype(np.float32), np.asarray(t, np.int64).reshape(-1, 3)


def read_obj_attributes(path):
    """-> (verts float32 [V,3], tris int64 [F,3], normals float32 [V,3] or None, colors float32 [V,3] or None) of a file that
    write_obj wrote: colours from `v x y z r g b` lines (all vertices or none), normals from `vn` lines through the faces'
    `a//a` entries, which must name the vertex's own normal (one normal per vertex)"""
    v, c, n, t = [], [], [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
                if len(p) >= 7:
                    c.append([float(x) for x in p[4:7]])
            elif p[0] == "vn":
                n.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"gsgen_amd.io.read_obj_attributes: {path}: a face of {len(p) - 1} vertices (triangles only)")
                for x in p[1:4]:
                    s = x.split("/")
                    if len(s) == 3 and s[2] != s[0]:
                        raise ValueError(f"gsgen_amd.io.read_obj_attributes: {path}: face entry {x}: normals are per vertex here")
                t.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    if (c and len(c) != len(v)) or (n and len(n) != len(v)):
        raise ValueError(f"gsgen_amd.io.read_obj_attributes: {path}: {len(c)} colours and {len(n)} normals for {len(v)} vertices")
    arr = lambda a: np.asarray(a, np.float64).reshape(-1, 3).astype(np.float32)  # noqa: E731
    return arr(v), np.asarray(t, np.int64).reshape(-1, 3), arr(n) if n else None, arr(c) if c else None


# ---- mesh .ply --------------------------------------------------------------------------------------
def _ply_mesh_dtypes(has_normals, has_colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if has_normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if has_colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields), np.dtype([("n", "u1"), ("idx", "<i4", 3)])


def write_ply_mesh(path, verts, tris, normals=None, colors=None):
    """binary_little_endian PLY of a triangle mesh: element vertex with float x y z, float nx ny nz when normals are given, uchar
    red green blue when colors are given (round(clip(c, 0, 1) * 255)); element face with `list uchar int vertex_indices`.  What
    MeshLab, Blender and Open3D read; nothing third-party."""
    v, t, n, c = _mesh_arrays("write_ply_mesh", verts, tris, normals, colors)
    if len(t) and t.max() > 0x7fffffff:
        raise ValueError("gsgen_amd.io.write_ply_mesh: vertex indices beyond int32")
    vdt, fdt = _ply_mesh_dtypes(n is not None, c is not None)
    vt = np.empty(len(v), vdt)
    vt["x"], vt["y"], vt["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        vt["nx"], vt["ny"], vt["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        u8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
        vt["red"], vt["green"], vt["blue"] = u8[:, 0], u8[:, 1], u8[:, 2]
    ft = np.empty(len(t), fdt)
    ft["n"], ft["idx"] = 3, t
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    header += [f"property {kinds[vdt[name].str]} {name}" for name in vdt.names]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vt.tobytes())
        f.write(ft.tobytes())


def read_ply_mesh(path):
    """-> (verts float32 [V,3], tris int64 [F,3], normals float32 [V,3] or None, colors uint8 [V,3] or None): the inverse of
    write_ply_mesh (triangles only; the property sets it writes)"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "binary_little_endian" not in lines[1]:
        raise ValueError("not a binary little-endian PLY")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith("property") and not ln.startswith("property list")]
    has_n, has_c = ("float", "nx") in props, ("uchar", "red") in props
    vdt, fdt = _ply_mesh_dtypes(has_n, has_c)
    if [p[1] for p in props] != list(vdt.names) or "property list uchar int vertex_indices" not in lines:
        raise ValueError(f"gsgen_amd.io.read_ply_mesh: {path}: unexpected properties {props}")
    vt = np.frombuffer(blob, vdt, count=nv, offset=end)
    ft = np.frombuffer(blob, fdt, count=nf, offset=end + nv * vdt.itemsize)
    if nf and (ft["n"] != 3).any():
        raise ValueError(f"gsgen_amd.io.read_ply_mesh: {path}: triangles only")
    col = lambda names: np.stack([vt[k] for k in names], 1)  # noqa: E731
    return (col(("x", "y", "z")), ft["idx"].astype(np.int64).reshape(-1, 3), col(("nx", "ny", "nz")) if has_n else None,
            col(("red", "green", "blue")) if has_c else None)
