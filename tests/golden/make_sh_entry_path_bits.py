"""Writes the fixtures of tests/test_sh_entry_path_bits.py: what the cases of that file produce on the commit this is run in.

    python tests/golden/make_sh_entry_path_bits.py cpu     # the CPU host build of this checkout's kernels (make -C oracle emu)
    python tests/golden/make_sh_entry_path_bits.py gpu     # the device, through the library gsgen_amd._capi.load() finds
                                                           # (GSGEN_HIP_LIB=<a build of the parent's sources> from any checkout)

Run in a checkout of the PARENT of the change under test (the test file and this one copied in); the test then holds the new
kernels to these bits.  Every case is recorded twice and the two recordings must agree: a fixture is only worth keeping if the
parent reproduces it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_sh_entry_path_bits as tb  # noqa: E402
import test_sh_walk_summary as ws  # noqa: E402


def main():
    kind = sys.argv[1]
    if kind == "cpu":
        import subprocess
        from gsgen_amd import _capi
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
        A = ws.HostArrays(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))
    else:
        A = ws.DeviceArrays()
    out = {}
    for name in tb.CASES:
        first, second = tb.record(A, name), tb.record(A, name)
        moved = [k for k in first if not np.array_equal(first[k], second[k], equal_nan=True)]
        assert not moved, (name, moved)
        out.update(first)
        print(f"[{kind}] {name}: {len(first)} entries, reproduced", flush=True)
    dst = sys.argv[2] if len(sys.argv) > 2 else tb.fixture_path(kind)
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


main()
