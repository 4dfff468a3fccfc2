"""The host bookkeeping of the modal solve (msom_amd/csrc/helm_inl.h: freeze rule, the 1.2 / 10 rule on nrelax, per-mode stats) driven by
scripted residual histories in a stand-alone program built with AddressSanitizer and UBSan (tools/helm_host_check.cpp).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_machine_equals_sequential_solves_under_sanitizers(tmp_path):
    exe = str(tmp_path / "helm_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "helm_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 9
