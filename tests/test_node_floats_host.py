"""The index and weight arithmetic of the vertex model's Lagrangian floats (the vertex part of msom_amd/csrc/floats_inl.h, the header
the kernels compile) on awkward inputs -- walls, vertex lines, nextafter neighbours of 0 and L0, +-1e300, +-0, NaN, inf -- in a
stand-alone program built with AddressSanitizer and UBSan (tools/node_floats_host_check.cpp), which reads the four corners of every
located cell from a heap array of exactly (N + 1)^2 doubles.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vertex_float_indices_and_weights_stay_in_range_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_floats_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "node_floats_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # N in {1, 2, 3, 32}, three domain sizes
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 12
    assert "12 grids checked, 0 failures" in r.stdout
