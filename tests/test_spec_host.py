"""The pieces of the wavenumber spectra that host and device share (msom_amd/csrc/spec_inl.h: the in-place line transform with its
padded layout and bit-reversed read-out, the shell ranges of the radial bins) in a stand-alone program built with AddressSanitizer and
UBSan (tools/spec_host_check.cpp): every line length 8 .. 4096 against a direct long double DFT, and the chain of passes of
kernels_spec.hip replayed with the same index arithmetic against a brute-force evaluation of the contract.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_line_transform_and_pass_chain_under_sanitizers(tmp_path):
    exe = str(tmp_path / "spec_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "spec_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 42 and "all ok" in r.stdout
