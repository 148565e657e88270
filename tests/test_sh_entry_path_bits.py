"""The entry loops of the polynomial SH compositing kernels, held BIT FOR BIT to the commit before their instruction overhead was
trimmed (broadcast operands without copies, votes on scalar masks, scalar trip tests, a guard whose rare side pays for itself,
atomic addresses from the scalar unit): that work may remove instructions that compute nothing and must not change one operation on
a pixel's, a gradient's or a summary word's way.

Every case runs the routed batch (gsgen_vol_render_sh_batch_routed + its backward in BOTH gradient forms) and the per-camera routed
pair (gsgen_vol_render_sh_routed / gsgen_vol_render_backward_sh_routed) and compares images, T, every word of the walk summary, the
routing flags and all gradient tensors with what the parent commit produced, per backend:

    tests/golden/sh_entry_path_bits/cpu.npz    the CPU host build of the kernels (`make -C oracle emu`)
    tests/golden/sh_entry_path_bits/gpu.npz    an MI355X

written by tests/golden/make_sh_entry_path_bits.py in a checkout of the parent commit.  The fixtures hold the walk summaries and
routing flags as they are and, of every other tensor, its SHA-256 and its fp64 sum: the raw tensors of all cases come to 10 MB per
backend, a committed file may hold 1 MiB.  A digest that matches is bit equality; one that does not says which tensor of which run
moved (the sums say roughly how far), not where.

Shapes, scenes and launches are those of tests/test_sh_walk_summary.py (two views of 48 x 40: 3 x 3 tiles with a partial right
column and bottom row; 500 splats; every splat listed in ONE tile per view, so a gradient is a sum of at most two values and the
device's atomics cannot reorder it).  Its nine cases -- ordinary, guard trip, non-PSD covariance, non-contributing entries,
saturation in mid-batch, past the 256-entry cap, flagged tile with and without no_fallback, two segments -- and, new here:
  * the middle tile's list cut to exactly 1, 31, 32, 33 and 64 entries (the staged batch is 32: the trip bounds' edges),
  * a splat whose rows fail the Taylor tier's test and pass the polynomial bound (a constant coefficient of 150: its row sums
    beyond 40 scaled logits, poly_transform scales it back and keeps it from the tier; its higher bands are small),
  * ONE splat beyond the coefficient bound at the front of the middle tile: less than a quarter of its batch, so the tile stays the
    polynomial kernels' and the splat takes the per-entry exact tier."""
import hashlib
import os

import numpy as np
import pytest

import test_sh_walk_summary as ws
from test_sh_walk_summary import emu, gpu  # noqa: F401  (the two backends' fixtures)

GOLDEN = os.path.join(ws.ROOT, "tests", "golden")
B, T = ws.B, ws.T


def fixture_path(kind):
    # (a directory of its own: tests/golden/*.npz are the reference's golden vectors, which other suites sweep by glob)
    return os.path.join(GOLDEN, "sh_entry_path_bits", f"{kind}.npz")


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def case_ordinary():
    return ws.Views()


def case_list_of(k):
    """the middle tile's list is exactly k new splats (sigma 4 pixels, alpha 0.3, centres inside the tile)"""
    def make():
        V = ws.Views()
        rng = np.random.default_rng(100 + k)
        new = []
        for _ in range(k):
            off = rng.uniform(-6.0, 6.0, 2)
            sh = np.concatenate([rng.normal(0, 1.0, (3, 1)), rng.normal(0, 0.002, (3, 15))], 1)
            new.append(V.add([V.pixel(v, 23.5 + off[0], 23.5 + off[1]) for v in range(B)], [ws.iso(V.sigma(v, 4.0)) for v in range(B)], 0.3, sh=sh))
        for v in range(B):
            V.lists[v][4] = list(new)
        return V
    return make


def _front_of_middle_tile(row):
    V = ws.Views()
    i = V.add([V.pixel(v, 22.0, 25.0) for v in range(B)], [ws.iso(V.sigma(v, 3.0)) for v in range(B)], 0.4, sh=row)
    for v in range(B):
        V.lists[v][4].insert(0, i)
    return V


def case_beyond_taylor():
    rng = np.random.default_rng(21)
    row = rng.normal(0, 0.002, (3, 16)).astype(np.float32)
    row[:, 0] = (150.0, -0.4, 1.5)
    return _front_of_middle_tile(row)


def case_exact_tier_entry():
    rng = np.random.default_rng(22)
    row = rng.normal(0, 0.3, (3, 16)).astype(np.float32)
    row[:, 9:] = 3.0
    return _front_of_middle_tile(row)


# name -> (scene, keyword arguments of run_batch)
CASES = {
    "ordinary": (case_ordinary, {}),
    "guard_trip": (ws.case_guard_trip, {}),
    "non_psd": (ws.case_non_psd, {}),
    "non_contributing": (ws.case_non_contributing, {}),
    "mid_batch_saturation": (ws.case_mid_batch_saturation, {}),
    "past_the_cap": (ws.case_past_the_cap, {}),
    "flagged_tile": (ws.case_flagged_tile, {}),
    "flagged_tile_no_fallback": (ws.case_flagged_tile, dict(no_fallback=1)),
    "two_segments": (ws.case_mid_batch_saturation, dict(nseg=2, fill=0x07)),
    **{f"list_of_{k}": (case_list_of(k), {}) for k in (1, 31, 32, 33, 64)},
    "beyond_taylor": (case_beyond_taylor, {}),
    "exact_tier_entry": (case_exact_tier_entry, {}),
}


# ---- what a case leaves ----------------------------------------------------------------------------------------------------------------

def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def record(A, name):
    """{key: array} of one case: digests and sums of every tensor of the three runs, the summaries and flags as they are"""
    make, kw = CASES[name]
    d = ws.device_inputs(A, make())
    runs = {"percam": ws.run_per_camera(A, d)}
    for moments in (False, True):
        runs["batch_moments" if moments else "batch_plain"] = ws.run_batch(A, d, moments, **kw)
    out = {}
    for run, r in runs.items():
        tensors = {"gsh": r["gsh"], "ga": r["ga"]}
        for v in range(B):
            tensors.update({f"img{v}": r["img"][v], f"T{v}": r["T"][v], f"gm{v}": r["gm"][v], f"gc{v}": r["gc"][v]})
        for k, a in tensors.items():
            out[f"{name}|{run}|{k}|sha256"] = digest(a)
            with np.errstate(all="ignore"):
                out[f"{name}|{run}|{k}|sum"] = np.float64(np.asarray(a, np.float64).sum())
        if "workspace" in r:
            out[f"{name}|{run}|walk"] = ws.walk_summary(A, r)
            out[f"{name}|{run}|flags"] = ws.routing_flags(A, r)
    return out


def check(A, name):
    with np.load(fixture_path(A.kind)) as f:
        want = {k: f[k] for k in f.files if k.startswith(name + "|")}
    got = record(A, name)
    assert sorted(got) == sorted(want)
    bad = []
    for k in sorted(got):
        if k.endswith("|sum"):
            continue
        if not np.array_equal(got[k], want[k]):
            s = k.rsplit("|", 1)[0] + "|sum"
            bad.append((k, float(got[s]), float(want[s])) if k.endswith("|sha256") else (k, got[k].tolist(), want[k].tolist()))
    assert not bad, bad
    # ... and the case is what it says (of the parent's own words: a fixture of the wrong scene would pass the comparison above)
    walk = want[f"{name}|batch_plain|walk"]
    if name.startswith("list_of_"):
        assert (walk[:, 4, 0] == int(name[8:])).all()
    elif name == "past_the_cap":
        assert (walk[:, 4, 0] > 256).all()
    elif name == "guard_trip":
        assert walk[0, 0, 1 + ws.WALK_K] & 3 == 3
    elif name == "flagged_tile":
        assert (want[f"{name}|batch_plain|flags"][:, 4] == 1).all()
    elif name in ("flagged_tile_no_fallback", "exact_tier_entry", "beyond_taylor"):
        assert not want[f"{name}|batch_plain|flags"].any() and (walk[:, 4, 1] & 1).all()
    elif name == "two_segments":
        assert (walk == 0x07070707).all()


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_entry_path_bits(emu, name):  # noqa: F811
    check(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_entry_path_bits(gpu, name):  # noqa: F811
    check(gpu, name)
