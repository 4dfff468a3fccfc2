"""Host side of the newqg dialect (no GPU, no compute calls): the params.in parser of msom_create_newqg, its derived values and its
errors, and the Python surface."""
import ctypes as C

import pytest

import msom_amd
import newqg_ref as nq
from msom_amd import api

MAXARR = 64


class NewqgParams(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ("N", "Ny", "nl", "nitermax", "nitermin")]
                + [(k, C.c_double) for k in ("L0", "DT", "CFL", "TOLERANCE", "f0", "beta", "hEkb", "tau0", "nu", "gp_low", "sbc", "tend", "dtout")]
                + [("dh", C.c_double * MAXARR), ("bc_fac", C.c_double), ("iRd2_low", C.c_double)])


def parse(text, derive=True):
    L = api.load_library()
    p = NewqgParams()
    L.msom_newqg_params_defaults(C.byref(p))
    L.msom_newqg_params_parse_text(C.byref(p), text.encode())
    rc = L.msom_newqg_params_derive(C.byref(p)) if derive else 0
    return p, rc


def test_sample_file_is_accepted_as_it_stands():
    p, rc = parse(nq.SAMPLE)
    assert rc == 0
    assert (p.N, p.Ny, p.nl, p.L0, p.f0, p.nu, p.gp_low, p.CFL, p.TOLERANCE) == (128, 128, 1, 100.0, 46.5, 0.5, 2500.0, 0.2, 1e-5)
    assert (p.hEkb, p.tau0, p.beta, p.sbc, p.tend, p.dtout, p.dh[0]) == (0.0, 1e-3, 0.5, 0.0, 200.0, 0.1, 1.0)
    D = 100.0 / 128
    assert p.DT == 0.5 * min(5e-2, D * D / 0.5 / 4.0)
    assert p.bc_fac == 0.0
    assert p.iRd2_low == -(46.5 * 46.5) / (2500.0 * 1.0)
    # the reference restatement derives the same numbers
    r = nq.sample_par(128)
    assert (r.DT, r.bc_fac, r.iRd2_low) == (p.DT, p.bc_fac, p.iRd2_low)


def test_defaults_blanks_comments_unknown_keys():
    p, rc = parse("")
    assert rc == 0
    assert (p.N, p.Ny, p.nl, p.L0, p.DT, p.CFL, p.TOLERANCE) == (64, 64, 1, 1.0, 1e10, 0.5, 1e-3)
    assert (p.f0, p.beta, p.hEkb, p.tau0, p.nu, p.gp_low, p.sbc, p.tend, p.dtout, p.dh[0], p.dh[1]) == (1.0, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1.0, 0.0)
    assert (p.nitermax, p.nitermin, p.bc_fac, p.iRd2_low) == (100, 1, 0.0, 0.0)
    p, rc = parse("#!sh\n# N = 5\n  N   =  32 \nbogus = 7\nRom = 3\ndh = [ 0.5 ]\nf0 = 2 = 3\nL0 = 2\nNy = 16\nNITERMAX = 7\n\ngp_low = 4\n")
    assert rc == 0
    assert (p.N, p.Ny, p.L0, p.f0, p.dh[0], p.nitermax) == (32, 16, 2.0, 2.0, 0.5, 7)
    assert p.DT == 1e10 and p.iRd2_low == -(2.0 * 2.0) / (4.0 * 0.5)


def test_no_slip_factor_by_the_formula():
    p, rc = parse("N = 32\nL0 = 100\nsbc = 100\n")
    D = 100.0 / 32
    assert rc == 0 and p.bc_fac == 100.0 / ((0.5 * 100.0 + 1) * (D * D))


@pytest.mark.parametrize("text,what", [("nl = 2\n", "one layer"), ("N = 48\n", "powers of two"), ("N = 32\nNy = 24\n", "powers of two"),
                                       ("dh = [0.0]\n", "dh"), ("sbc = -2\n", "sbc"), ("sbc = -0.5\n", "sbc")])
def test_config_errors(text, what):
    L = api.load_library()
    p, rc = parse(text)
    assert rc == -3   # MSOM_ERR_CONFIG
    assert what in L.msom_last_error().decode()
    with pytest.raises(msom_amd.MsomError, match=what):
        msom_amd.NewQG(text)


def test_create_without_a_device_or_a_file_fails_loudly(tmp_path):
    import torch
    with pytest.raises(msom_amd.MsomError, match="not found"):
        msom_amd.NewQG(path=str(tmp_path / "missing.in"))
    if not torch.cuda.is_available():
        with pytest.raises(msom_amd.MsomError, match="no HIP device"):
            msom_amd.NewQG(nq.SAMPLE)


def test_python_surface_has_the_dialects_calls_only():
    for name in ("set", "get", "set_const", "update", "advance", "invertq", "comp_q", "step", "set_tnext", "ke", "mgstats", "write_nc", "read_nc",
                 "profile_read", "profile_reset", "sync", "bench_kernel", "param", "option", "close"):
        assert callable(getattr(msom_amd.NewQG, name)), name
    for name in ("pystep_bfn", "pyq2p", "pyp2q", "bfn_steps", "stats_begin", "modes_compute", "wavelet_filter", "run", "read_inputs", "remove_mean",
                 "write_bas"):
        assert not hasattr(msom_amd.NewQG, name), name
