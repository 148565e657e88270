"""Run lengths of the push binning's emit pass on a bench workload, on the host: how many keys each (chunk, tile) pair holds -- the
runs its flush stores --, which share of them fits the staging array, and how many 32-byte sectors the stores touch.
    python tools/emit_run_histogram.py [cfg2] [capacity ...]        (needs the oracle: a checker's tool, no GPU)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import bench, scenes

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
caps = [int(a) for a in sys.argv[2:]] or [8192, 12288]
CHUNK, B = 2048, 8
sc, W, H = bench.make_workload(cfg)
N = sc["mean"].shape[0]
nchunks = (N + CHUNK - 1) // CHUNK
cams = bench.camera_poses(B, 0, W, H)
nth, ntw = (H + 15) // 16, (W + 15) // 16
T = nth * ntw
hist = np.zeros(CHUNK + 1, np.int64)
keys = 0
stat = {c: dict(staged=0, sect_staged=0, lines_staged=0) for c in caps}
for cam in cams:
    cam = scenes.Camera(W, H, *cam.intr[:4], c2w=cam.c2w) if not hasattr(cam, "tiles") else cam
    g = scenes.oracle_geometry(sc, cam)
    idx = np.nonzero(g["mask"])[0]
    x0, y0 = g["tl"][:, 0].clip(0), g["tl"][:, 1].clip(0)
    x1, y1 = g["br"][:, 0].clip(max=ntw - 1), g["br"][:, 1].clip(max=nth - 1)
    w, h = (x1 - x0 + 1).clip(0), (y1 - y0 + 1).clip(0)
    n = (w * h).astype(np.int64)
    rep = np.repeat(np.arange(len(n)), n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    tile = (y0[rep] + k // w[rep]) * ntw + x0[rep] + k % w[rep]
    C = np.bincount((idx[rep] // CHUNK) * T + tile, minlength=nchunks * T).reshape(nchunks, T)
    assert C.sum() == g["D"]
    keys += int(C.sum())
    hist += np.bincount(C[C > 0], minlength=CHUNK + 1)
    tile_off = np.cumsum(C.sum(0)) - C.sum(0)
    start = tile_off[None, :] + np.cumsum(C, 0) - C           # a run's first key in the pair list
    for cap, s in stat.items():
        fits = (np.cumsum(C, 1) <= cap) & (C > 0)
        a, l = start[fits] * 8, C[fits] * 8
        s["staged"] += int(C[fits].sum())
        s["sect_staged"] += int(((a + l - 1) // 32 - a // 32 + 1).sum())
        s["lines_staged"] += int(((a + l - 1) // 128 - a // 128 + 1).sum())
print(f"{cfg}: {B} views, {N} Gaussians in {nchunks} chunks, {T} tiles, {keys} keys = {keys * 8 / 1e6:.1f} MB; "
      f"{keys / (B * nchunks):.0f} keys per chunk, {int(hist.sum())} runs, mean run {keys / hist.sum():.2f} keys")
edges = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 24, 32, 64, CHUNK + 1]
print("run length (keys): runs, share of the keys")
for lo, hi in zip(edges[:-1], edges[1:]):
    r = np.arange(lo, hi)
    print(f"  {lo:4d}{'' if hi == lo + 1 else f' .. {hi - 1}':>8s}: {int(hist[lo:hi].sum()):8d} {float((hist[lo:hi] * r).sum()) / keys * 100:6.1f} %")
for cap, s in stat.items():
    direct = keys - s["staged"]
    print(f"capacity {cap}: {s['staged'] / keys * 100:.1f} % of the keys staged; their runs touch {s['sect_staged']} 32-byte sectors "
          f"({s['sect_staged'] * 32 / 1e6:.1f} MB, {s['sect_staged'] * 32 / (8 * s['staged']):.2f} x their bytes) in {s['lines_staged']} 128-byte lines; "
          f"{direct} keys stored one by one ({direct * 32 / 1e6:.1f} MB at a sector each): "
          f"{(s['sect_staged'] + direct) * 32 / 1e6:.1f} MB = {(s['sect_staged'] + direct) * 32 / (8 * keys):.2f} x if no sector is merged with a later chunk's")
