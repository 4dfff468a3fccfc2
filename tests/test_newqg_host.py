"""The newqg params.in parser (msom_amd/csrc/params.c: msom_newqg_params_*) in a stand-alone program built with AddressSanitizer and
UBSan (tools/newqg_host_check.c): over-long lines, over-long arrays, empty values, files.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_under_sanitizers(tmp_path):
    exe = str(tmp_path / "newqg_host_check")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "newqg_host_check.c"), os.path.join(ROOT, "msom_amd", "csrc", "params.c"), "-o", exe, "-lm"])
    r = subprocess.run([exe, str(tmp_path / "check.in")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 10
