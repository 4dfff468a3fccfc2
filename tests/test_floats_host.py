"""The index and weight arithmetic of the Lagrangian floats (msom_amd/csrc/floats_inl.h, the header the kernels compile) on awkward
inputs -- walls, cell-centre lines, nextafter neighbours, +-1e300, +-0, NaN, far outside a periodic box -- in a stand-alone program
built with AddressSanitizer and UBSan (tools/floats_host_check.cpp), which reads the corners of every located dual cell from a heap
array of exactly the ghosted layer's size.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_indices_and_weights_stay_in_range_under_sanitizers(tmp_path):
    exe = str(tmp_path / "floats_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "floats_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # nx, ny in {1, 2, 3, 32, 48}, walls and periodic
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 50
    assert "50 grids checked, 0 failures" in r.stdout
