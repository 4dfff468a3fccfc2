"""The owner rule of the Lagrangian floats on tiles (floats_owner, floats_hop of msom_amd/csrc/floats_inl.h, the header the kernels
compile) on awkward inputs -- every seam and its nextafter neighbours, the cell-centre lines on either side of a seam, 0 and L,
+-1e300, +-0, NaN, +-inf, far outside a periodic box -- in a stand-alone program built with AddressSanitizer and UBSan
(tools/floats_tiles_host_check.cpp), which reads the corners of every located dual cell from a heap array of exactly the owner
tile's ghosted layer and compares the owner with brute force.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_and_local_corners_stay_in_range_under_sanitizers(tmp_path):
    exe = str(tmp_path / "floats_tiles_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "floats_tiles_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # tile sizes {1, 2, 16} x tiles per side {1, 2, 4}, walls and periodic
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 18
    assert "18 tilings checked, 0 failures" in r.stdout
