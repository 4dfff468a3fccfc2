"""The owner rule of the vertex model's Lagrangian floats on tiles (nfloats_owner, nfloats_local of msom_amd/csrc/floats_inl.h, the
header the kernels compile) on awkward inputs -- every seam and its nextafter neighbours, 0 and L0, +-1e300, +-0, NaN, +-inf -- in a
stand-alone program built with AddressSanitizer and UBSan (tools/node_floats_tiles_host_check.cpp), which reads the corners of every
located cell from a heap array of exactly the vertices the owner tile holds and compares the owner with brute force.  And that the
host (begin's partition in floats_host.hip, for both models) and the kernels take the owner and the local corners from those
functions, not from arithmetic of their own.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msom_amd", "csrc")


def test_owner_and_local_corners_stay_in_range_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_floats_tiles_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "node_floats_tiles_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # N = 2: one tile; N = 4: 1 or 2 tiles a side; N = 32, 64: 1, 2 or 4 a side, (2, 4) and (4, 1) among them
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 23
    assert "23 tilings checked, 0 failures" in r.stdout
    for line in ("N 2, 1 x 1 tiles", "N 4, 2 x 2 tiles", "N 32, 4 x 1 tiles", "N 64, 2 x 4 tiles", "N 64, 4 x 4 tiles"):
        assert line in r.stdout, line


def code_of(name):
    """a source file without its comments"""
    txt = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_host_and_kernels_read_the_same_functions():
    inl = code_of("floats_inl.h")
    for fn in ("nfloats_owner_axis", "nfloats_owner", "nfloats_local"):
        assert re.search(r"FL_HD static inline \w+ " + fn + r"\(", inl), fn
    host, emig, kern = code_of("floats_host.hip"), code_of("kernels_floats.hip"), code_of("kernels_node_floats.hip")
    # who owns a position: the host at begin (the partition of floats_host.hip, for both models) and the emigrate kernel, through the
    # one function, on nfloats_locate's cell; the layered model through floats_owner on floats_locate's
    assert "nfloats_owner(nfloats_locate(" in host and "nfloats_owner(c, t, &col, &row)" in emig and "nfloats_locate(hx, hy, fg)" in emig
    assert " floats_owner(floats_locate(" in host
    # the local corners: every tiled kernel body through nfloats_local, none by a subtraction of its own
    assert kern.count("nfloats_local(&c, ") == 3 and "- t.ox" not in kern and "- tx0" not in kern
    # neither the engine, nor a model's host file, nor the kernels divide by a tile size themselves
    for txt in (host, code_of("msom_floats.hip"), code_of("msomn_floats.hip"), emig, kern):
        assert "/ t.tnx" not in txt and "/ tl.tnx" not in txt and "/ t.tx" not in txt and "/ c.tl.tnx" not in txt
    # and the partition exists once: the models' files locate nothing
    for name in ("msom_floats.hip", "msomn_floats.hip"):
        assert "floats_locate(" not in code_of(name), name
