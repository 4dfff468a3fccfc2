"""The per-column eigen solver of the vertical modes (msom_amd/csrc/modes_inl.h, the routine k_modes_eig runs per thread) compiled for
the host and driven by a stand-alone program under AddressSanitizer and UBSan (tools/modes_host_check.cpp): hard stratifications against
long double criteria, the uniform column against its closed form, the columns that must be refused (MODES_WEAK, MODES_BAD_S), the ends
of the fp64 range, data that cannot converge, for NL = 1, 2, 3, 6, 8 (register accessor) and 9, 16 (memory accessor, stride 64, lane 37).
No GPU.  Unfused arithmetic, and, where the CPU has FMA, a second build that contracts as the product build of the kernel does.

First measured (both builds alike to the digits shown): eigenvalues <= 0.040, residuals <= 0.039, D-orthonormality <= 0.049 of their bounds
(8 nl eps each); closed form: eigenvalues <= 0.044 of 8 nl eps lambda_max, vectors <= 0.044 of 4 nl eps / gap.
Negative controls, run once on a scratch copy of the header: without the MODES_WEAK rule the four refused-column checks fail with status 0
and the range check finds MODES_OK with d = inf (nl = 2, 8, 9); one rotation of ModesMemV::rotate scaled by 1 + 1e-9 makes the residual
(2.6e3 .. 2.8e4 times its bound) and the orthonormality (1.2e5 .. 7.3e5) fail for nl = 9 and 16 and for no other nl."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = 7 * 5 + 6 * 2 + 4      # per nl: 3 families, closed form, range; nl >= 2: bad S, no convergence; nl = 3, 6, 9, 16: refused


def has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


def test_eigen_solver_on_hard_columns_under_sanitizers(tmp_path):
    modes = [["-ffp-contract=off"]]
    if has_fma():       # without FMA the contracted build would be the same program
        modes.append(["-march=native", "-ffp-contract=fast"])
    exes = [str(tmp_path / f"modes_host_check{n}") for n in range(len(modes))]
    builds = [subprocess.Popen(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *mode,
                                os.path.join(ROOT, "tools", "modes_host_check.cpp"), "-o", exe])
              for mode, exe in zip(modes, exes)]           # side by side: the 120 unrolled rotations of NL = 16 take the compiler 20 s
    assert [b.wait() for b in builds] == [0] * len(modes)
    for mode, exe in zip(modes, exes):
        r = subprocess.run([exe], capture_output=True, text=True)
        print(" ".join(mode), r.stdout, r.stderr, sep="\n")
        assert r.returncode == 0, mode
        assert "FAIL" not in r.stdout and r.stdout.count(": ok") == CHECKS, mode
