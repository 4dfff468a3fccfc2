"""The index arithmetic of the vertex model on tiles (msom_amd/csrc/node_tile_inl.h: tile windows, wall bits, update / sum / halo ranges,
the gather level and the piece offsets of the gather) against brute force over every global vertex, in a stand-alone program built with
AddressSanitizer and UBSan (tools/node_tile_host_check.cpp).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_index_arithmetic_equals_brute_force_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_tile_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "node_tile_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # N in {8 .. 256} x px, py in {1, 2, 4, 8}: 96 decompositions, of which the 7 with N = 8 and 8 tiles a side have one-cell tiles
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 89
    assert "89 decompositions checked, 7 refused, 0 failures" in r.stdout
