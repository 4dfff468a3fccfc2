"""ctypes binding of libmsomhip (include/msom.h) and the host mirror of the reference's
Python surface (msqg/qg.i:29-36, msqg/qg_bfn.i, usage in msqg/qg_bfn.py:33-80)."""
import ctypes as C
import os

import numpy as np

from .state import read_state, write_state  # noqa: F401  (the state file in pure Python)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBDIR = os.path.join(_HERE, "lib")

FIELDS = dict(PSI=0, Q=1, ZETA=2, PSIPG=3, ZETAPG=4, QFORC=5, TMP=6, FR=7, S=8, DQ=9, RO=10, TOPO=11,
              QPRED=12, NOISE=13, SIGMA=14, PTR=15, PTR_RELAX=16, DPTR=17, PTR_PRED=18, RD=19, QOF=20,
              DE_BF=21, DE_VD=22, DE_J1=23, DE_J2=24, DE_J3=25, DE_FT=26, TMP2=27, PO_MFT=28,
              BFN_F1=29, BFN_F2=30, BFN_F3=31, BFN_OBS=32, BFN_GAIN=33)

# running statistics (msom_stats_*): accumulators 0 .. NACC - 1 (bit k of the mask), derived quantities, qo_me of time_filter
STATS = dict(PSI=0, Q=1, PSI2=2, Q2=3, KE=4, UQ=5, VQ=6, NACC=7, EKE=16, UQ_EDDY=17, VQ_EDDY=18, QME=32)

# vertical normal modes (msom_modes_*): what modes_get returns -- IBU and RD nl arrays, M2L (array k*nl + m: layer k from mode m) and
# L2M (array m*nl + k: mode m from layer k) nl*nl arrays
MODES = dict(IBU=0, RD=1, M2L=2, L2M=3, N=4)


class MsomError(RuntimeError):
    pass


class MGStats(C.Structure):
    """mgstats of Basilisk (mspg/elliptic.h:118-123)."""
    _fields_ = [("i", C.c_int), ("resb", C.c_double), ("resa", C.c_double), ("sum", C.c_double), ("nrelax", C.c_int)]

    def __repr__(self):
        return f"MGStats(i={self.i}, resb={self.resb:g}, resa={self.resa:g}, sum={self.sum:g}, nrelax={self.nrelax})"


class StateInfo(C.Structure):
    """msom_state_info_t of include/msom_state.h"""
    _fields_ = [(k, C.c_int) for k in ("version", "dialect", "nx", "ny", "nl", "nptr", "stochastic", "noise_mode", "mode_pv_invert",
                                        "flag_topo", "nrecords")] + [("iter", C.c_long), ("t", C.c_double), ("dt", C.c_double)]


_libs = {}
_dp = C.POINTER(C.c_double)


def load_library(strict=False):
    """Load the HIP library.  strict=True loads the validation build (-ffp-contract=off,
    reference expression order) that is bit-exact against the CPU oracle."""
    name = "libmsomhip_strict.so" if strict else "libmsomhip.so"
    if name in _libs:
        return _libs[name]
    path = os.path.join(_LIBDIR, name)
    if not os.path.exists(path):
        raise MsomError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(make -C msom_amd/csrc).  There is no CPU fallback.")
    L = C.CDLL(path)
    vp, ci, cd, cs = C.c_void_p, C.c_int, C.c_double, C.c_char_p
    sig = {
        "msom_last_error": (cs, []),
        "msom_version": (cs, []),
        "msom_create": (vp, [cs]),
        "msom_create_str": (vp, [cs]),
        "msom_create_newqg": (vp, [cs]),
        "msom_create_newqg_str": (vp, [cs]),
        "msom_destroy": (ci, [vp]),
        "msom_set_option": (ci, [vp, cs, cd]),
        "msom_get_param": (cd, [vp, cs]),
        "msom_set_field": (ci, [vp, ci, vp]),
        "msom_get_field": (ci, [vp, ci, vp]),
        "msom_field_layers": (ci, [vp, ci]),
        "msom_remove_mean": (ci, [vp, ci]),
        "msom_set_const": (ci, [vp]),
        "msom_read_inputs": (ci, [vp, cs]),
        "msom_update": (cd, [vp, vp, vp, cd]),
        "msom_advance": (ci, [vp, vp, vp, vp, cd]),
        "msom_invertq": (ci, [vp, vp, vp, C.POINTER(MGStats)]),
        "msom_comp_q": (ci, [vp, vp, vp]),
        "pystep_bfn": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci, cd, ci]),
        "pyq2p": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci]),
        "pyp2q": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci]),
        "msom_bfn_begin": (ci, [vp]),
        "msom_bfn_steps": (ci, [vp, ci, cd, cd, cd]),
        "msom_bfn_misfit": (ci, [vp, _dp]),
        "msom_stats_begin": (ci, [vp, C.c_uint]),
        "msom_stats_accumulate": (ci, [vp, cd]),
        "msom_stats_weight": (ci, [vp, _dp]),
        "msom_stats_get": (ci, [vp, ci, vp]),
        "msom_time_filter": (ci, [vp, cd]),
        # Lagrangian floats (include/msom_floats.h)
        "msom_floats_begin": (ci, [vp, ci, vp, vp, vp]),
        "msom_floats_end": (ci, [vp]),
        "msom_floats_get": (ci, [vp, vp, vp]),
        "msom_floats_velocity": (ci, [vp, vp, vp]),
        "msom_floats_sample": (ci, [vp, ci, vp]),
        "msom_floats_stage": (ci, [vp, ci, cd]),
        "msom_floats_record": (ci, [vp, ci, ci]),
        "msom_floats_track": (ci, [vp, ci, ci, _dp, vp, vp]),
        "msom_floats_dbg_ghosted": (ci, [vp, ci, vp]),
        "msom_modes_compute": (ci, [vp]),
        "msom_modes_layers": (ci, [vp, ci]),
        "msom_modes_get": (ci, [vp, ci, vp]),
        "msom_modes_project": (ci, [vp, ci, vp, vp]),
        "msom_modes_energy": (ci, [vp, _dp, _dp]),
        "msom_modes_set_rd": (ci, [vp, ci]),
        "msom_modes_mgstats": (ci, [vp, ci, C.POINTER(MGStats)]),
        "msom_spec_layout": (ci, [ci, ci, C.POINTER(ci), C.POINTER(C.c_long)]),
        "msom_spec_bins": (ci, [vp]),
        "msom_spec_kr": (ci, [vp, _dp]),
        "msom_spec_2d": (ci, [vp, vp, vp, ci, vp]),
        "msom_spec_cross": (ci, [vp, vp, vp, ci, _dp, _dp]),
        "msom_spec_fields": (ci, [vp, ci, ci, _dp, _dp]),
        "msom_spec_energy": (ci, [vp, _dp, _dp]),
        "msom_dbg_helm_relax": (ci, [vp, ci, vp, vp, ci, C.POINTER(ci)]),
        "msom_dbg_helm_residual": (ci, [vp, vp, vp, vp, _dp]),
        "msom_step": (ci, [vp, _dp]),
        "msom_set_tnext": (ci, [vp, cd]),
        "msom_time": (cd, [vp]),
        "msom_iter": (ci, [vp]),
        "msom_ke": (cd, [vp]),
        "msom_last_mgstats": (ci, [vp, C.POINTER(MGStats)]),
        "msom_run": (ci, [vp, cs, C.c_long]),
        "msom_write_bas": (ci, [vp, ci, cs]),
        "msom_read_bas": (ci, [vp, ci, cs]),
        "msom_write_nc": (ci, [vp, cs]),
        "msom_read_nc": (ci, [vp, ci, cs, cs, ci]),
        "msom_set_device": (ci, [ci]),
        "msom_comm_unique_id": (ci, [vp]),
        "msom_create_tiled": (vp, [cs, ci, ci, ci, vp]),
        "msom_tile_info": (ci, [vp] + [C.POINTER(ci)] * 6),
        "msom_dbg_nlevels": (ci, [vp]),
        "msom_dbg_level_dims": (ci, [vp, ci, C.POINTER(ci), C.POINTER(ci)]),
        "msom_dbg_relax": (ci, [vp, ci, vp, vp, ci]),
        "msom_dbg_residual": (ci, [vp, vp, vp, vp, _dp]),
        "msom_dbg_rhs_resid": (ci, [vp, ci, cd, vp, vp, _dp, _dp]),
        "msom_dbg_restrict": (ci, [vp, ci, vp, vp]),
        "msom_dbg_prolong": (ci, [vp, ci, vp, vp]),
        "msom_dbg_op": (ci, [vp, cs, ci, ci, cd, cd]),
        "msom_profile_read": (ci, [vp, cs, _dp, C.POINTER(C.c_long)]),
        "msom_profile_reset": (ci, [vp]),
        "msom_sync": (ci, [vp]),
        "msom_bench_kernel": (ci, [vp, cs, ci, _dp]),
        "msom_dbg_rccl_selftest": (ci, []),
        "msom_wavelet_filter": (ci, [vp, cd]),
        "msom_energy_tend": (ci, [vp, cd]),
        "msom_filter_de": (ci, [vp, ci, cd]),
        "msom_reset_de": (ci, [vp]),
        "pystep_de": (ci, [vp] + [vp, ci, ci, ci] * 7 + [ci]),
        "msom_dbg_wavelet_levels": (ci, [vp]),
        "msom_dbg_siglev": (ci, [vp, ci, vp]),
        "msom_dbg_wavelet_apply": (ci, [vp, ci]),
        # lossless checkpoint / restart (include/msom_state.h)
        "msom_state_save": (ci, [vp, cs, C.c_uint]),
        "msom_state_load": (ci, [vp, cs]),
        "msom_create_from_state": (vp, [cs]),
        "msom_state_check": (ci, [cs, C.POINTER(ci)]),
        "msom_state_info": (ci, [cs, C.POINTER(StateInfo), C.c_char_p, C.c_size_t]),
        "msom_state_dbg_flip": (ci, [vp, C.c_long]),
        # vertex-grid variant (qg-node/)
        "msomn_create": (vp, [cs]),
        "msomn_create_str": (vp, [cs]),
        "msomn_create_tiled": (vp, [cs, ci, ci, ci, vp]),
        "msomn_tile_info": (ci, [vp] + [C.POINTER(ci)] * 6),
        "msomn_destroy": (None, [vp]),
        "msomn_set_option": (ci, [vp, cs, cd]),
        "msomn_get_param": (cd, [vp, cs]),
        "msomn_field_layers": (ci, [vp, ci]),
        "msomn_set_field": (ci, [vp, ci, vp]),
        "msomn_get_field": (ci, [vp, ci, vp]),
        "msomn_set_const": (ci, [vp]),
        "msomn_update": (ci, [vp, ci, ci, cd, _dp]),
        "msomn_advance": (ci, [vp, ci, ci, ci, cd]),
        "msomn_invert_q": (ci, [vp, ci, C.POINTER(MGStats)]),
        "msomn_comp_q": (ci, [vp, ci, ci]),
        "msomn_rhs_pv": (ci, [vp, ci, ci]),
        "msomn_forcing": (ci, [vp]),
        "msomn_step": (ci, [vp, ci]),
        "msomn_set_tnext": (ci, [vp, cd]),
        "msomn_time": (cd, [vp]),
        "msomn_dt": (cd, [vp]),
        "msomn_iter": (ci, [vp]),
        "msomn_ke": (ci, [vp, _dp]),
        "msomn_last_mgstats": (ci, [vp, C.POINTER(MGStats)]),
        "msomn_stats_begin": (ci, [vp, C.c_uint]),
        "msomn_stats_accumulate": (ci, [vp, cd]),
        "msomn_stats_weight": (ci, [vp, _dp]),
        "msomn_stats_get": (ci, [vp, ci, vp]),
        "msomn_profile_read": (ci, [vp, cs, _dp, C.POINTER(C.c_long)]),
        "msomn_profile_reset": (ci, [vp]),
        "msomn_diag1d": (ci, [vp, _dp]),
        "msomn_write_nc": (ci, [vp, cs]),
        "msomn_read_nc": (ci, [vp, ci, cs, cs, ci]),
        "msomn_run": (ci, [vp, cs, C.c_long]),
        "msomn_dbg_relax": (ci, [vp, ci, vp, vp, ci]),
        "msomn_dbg_residual": (ci, [vp, vp, vp, vp, _dp]),
        "msomn_dbg_restrict": (ci, [vp, ci, vp, vp]),
        "msomn_dbg_prolong": (ci, [vp, ci, vp, vp]),
        "msomn_dbg_level_mask": (ci, [vp, ci, vp]),
        "msomn_dbg_del2_zeta": (ci, [vp]),
        "msomn_dbg_noise": (ci, [vp, vp, ci, vp]),
        "msomn_dbg_csig": (ci, [vp, ci, vp]),
        "msomn_noise_draw": (ci, [vp, ci]),
        "msomn_wavelet_filter": (ci, [vp, cd]),
        "msomn_dbg_wv_get": (ci, [vp, ci, ci, vp]),
        "msomn_dbg_wv_apply": (ci, [vp, vp, vp]),
        # lossless checkpoint / restart of the vertex model (include/msomn_state.h)
        "msomn_state_save": (ci, [vp, cs, C.c_uint]),
        "msomn_state_load": (ci, [vp, cs]),
        "msomn_create_from_state": (vp, [cs]),
        "msomn_create_tiled_from_state": (vp, [cs, ci, ci, ci, vp]),
        "msomn_state_dbg_flip": (ci, [vp, C.c_long]),
        # Lagrangian floats of the vertex model (include/msomn_floats.h)
        "msomn_floats_begin": (ci, [vp, ci, vp, vp, vp]),
        "msomn_floats_end": (ci, [vp]),
        "msomn_floats_get": (ci, [vp, vp, vp]),
        "msomn_floats_velocity": (ci, [vp, vp, vp]),
        "msomn_floats_sample": (ci, [vp, ci, vp]),
        "msomn_floats_stage": (ci, [vp, ci, cd]),
        "msomn_floats_record": (ci, [vp, ci, ci, ci]),
        "msomn_floats_track": (ci, [vp, ci, ci, _dp, vp, vp, vp]),
    }
    for fn, (res, args) in sig.items():
        f = getattr(L, fn)  # AttributeError if the library does not export a declared symbol
        f.restype, f.argtypes = res, args
    _libs[name] = L
    return L


def spec_layout(nx, ny, strict=False):
    """(nbins, count[nbins]) of the radial bins of an nx x ny grid (msom_spec_layout): host arithmetic, no handle and no GPU"""
    L = load_library(strict)
    nb = C.c_int()
    r = L.msom_spec_layout(int(nx), int(ny), C.byref(nb), None)
    if r != 0:
        raise MsomError(f"error {r}: {L.msom_last_error().decode()}")
    count = np.zeros(nb.value, dtype=np.int_)
    assert count.itemsize == C.sizeof(C.c_long)
    r = L.msom_spec_layout(int(nx), int(ny), C.byref(nb), count.ctypes.data_as(C.POINTER(C.c_long)))
    if r != 0:
        raise MsomError(f"error {r}: {L.msom_last_error().decode()}")
    return nb.value, count


def state_check(path, strict=False):
    """msom_state_check: walks the records of a state file and verifies every digest on the host (no handle, no GPU); the number of
    records, or MsomError with the library's code in .code"""
    L = load_library(strict)
    n = C.c_int()
    r = L.msom_state_check(os.fsencode(path), C.byref(n))
    if r != 0:
        e = MsomError(f"error {r}: {L.msom_last_error().decode()}")
        e.code = r
        raise e
    return n.value


def state_info(path, strict=False):
    """msom_state_info: dict of the header, t, dt, iter and the record names of a state file (host only)"""
    L = load_library(strict)
    info, names = StateInfo(), C.create_string_buffer(4096)
    r = L.msom_state_info(os.fsencode(path), C.byref(info), names, len(names))
    if r != 0:
        e = MsomError(f"error {r}: {L.msom_last_error().decode()}")
        e.code = r
        raise e
    out = {k: getattr(info, k) for k, _ in StateInfo._fields_}
    out["names"] = names.value.decode().split(",") if names.value else []
    return out


def from_state(path, strict=False):
    """msom_create_from_state: a single-tile model (QG or NewQG, as the file says) made from the params text in the file, loaded"""
    L = load_library(strict)
    h = L.msom_create_from_state(os.fsencode(path))
    if not h:
        raise MsomError(L.msom_last_error().decode())
    newqg = L.msom_get_param(h, b"model") == 1
    g = (NewQG if newqg else QG).__new__(NewQG if newqg else QG)
    g.L, g.h = L, h
    g.nl = int(g.param("nl"))
    g.nx, g.ny = int(g.param("nx")), int(g.param("ny"))
    if not newqg:
        g.tile = (1, 1, 0, 0)
    return g


def node_from_state(path, strict=False, tiled=None):
    """msomn_create_from_state: a vertex-grid model made from the params text in a state file saved with constants, loaded.
    tiled = (px, py, rank, uid): msomn_create_tiled_from_state, this rank's tile of the file's grid (collective: every rank calls it with
    the same file, whatever tiling wrote it); the handle has io_tiles = 1, and wavelet_tiles = 1 if the file is stochastic or filtered"""
    L = load_library(strict)
    if tiled is not None:
        px, py, rank, uid = tiled
        h = L.msomn_create_tiled_from_state(os.fsencode(path), px, py, rank, uid)
    else:
        h = L.msomn_create_from_state(os.fsencode(path))
    if not h:
        raise MsomError(L.msom_last_error().decode())
    g = NodeQG.__new__(NodeQG)
    g.L, g.h = L, h
    g._read_shape()
    return g


def _ptr(a):
    """numpy array (host) or an object with .data_ptr() (torch tensor, host or device)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _f64(a, shape=None):
    if hasattr(a, "data_ptr"):
        return a
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"array shape {a.shape} != {tuple(shape)}")
    return a


class QG:
    """One model instance = one `qg.e` process / one `import qg` of the reference."""

    def __init__(self, params=None, path=None, strict=False, tiled=None):
        self.L = load_library(strict)
        self.h = None
        if tiled is not None:
            px, py, rank, uid = tiled
            self.h = self.L.msom_create_tiled(params.encode(), px, py, rank, uid)
        elif path is not None:
            self.h = self.L.msom_create(path.encode())
        else:
            self.h = self.L.msom_create_str(params.encode())
        if not self.h:
            raise MsomError(self.L.msom_last_error().decode())
        self.nl = int(self.param("nl"))
        px_, py_, ix, iy, nx, ny = (C.c_int() for _ in range(6))
        self.L.msom_tile_info(self.h, *(C.byref(v) for v in (px_, py_, ix, iy, nx, ny)))
        self.nx, self.ny = nx.value, ny.value
        self.tile = (px_.value, py_.value, ix.value, iy.value)

    def close(self):
        if self.h:
            self.L.msom_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != 0:
            raise MsomError(f"error {r}: {self.L.msom_last_error().decode()}")

    # -- parameters / options
    def param(self, key):
        return self.L.msom_get_param(self.h, key.encode())

    def option(self, key, value):
        self._chk(self.L.msom_set_option(self.h, key.encode(), float(value)))

    # -- fields (pyset_field / pyget_field, msqg/qg.h:1164-1188)
    def shape(self, field):
        n = self.L.msom_field_layers(self.h, field)
        if n < 0 and FIELDS["BFN_F1"] <= field <= FIELDS["BFN_GAIN"]:
            n = self.nl     # allocated by the first msom_set_field / msom_get_field / msom_bfn_begin
        return (n, self.ny, self.nx)

    def set(self, field, a):
        a = _f64(a, self.shape(field))
        self._chk(self.L.msom_set_field(self.h, field, _ptr(a)))

    def get(self, field):
        a = np.empty(self.shape(field))
        self._chk(self.L.msom_get_field(self.h, field, _ptr(a)))
        return a

    def remove_mean(self, field):
        self._chk(self.L.msom_remove_mean(self.h, field))

    def set_const(self):
        self._chk(self.L.msom_set_const(self.h))

    def read_inputs(self, directory="."):
        self._chk(self.L.msom_read_inputs(self.h, directory.encode()))

    # -- hooks
    def update(self, q=None, dtmax=None, want=True):
        """update_qg: returns (dqdt, dtmax)."""
        q = None if q is None else _f64(q, self.shape(1))
        out = np.empty(self.shape(1)) if want else None
        d = self.L.msom_update(self.h, _ptr(q), _ptr(out), self.param("DT") if dtmax is None else dtmax)
        if d < 0:
            raise MsomError(self.L.msom_last_error().decode())
        return out, d

    def advance(self, qin, dqdt, dt):
        qin, dqdt = _f64(qin, self.shape(1)), _f64(dqdt, self.shape(1))
        out = np.empty(self.shape(1))
        self._chk(self.L.msom_advance(self.h, _ptr(out), _ptr(qin), _ptr(dqdt), dt))
        return out

    def invertq(self, q=None, psi0=None):
        q = None if q is None else _f64(q, self.shape(1))
        psi = np.zeros(self.shape(0)) if psi0 is None else np.array(psi0, dtype=np.float64, order="C")
        st = MGStats()
        self._chk(self.L.msom_invertq(self.h, _ptr(q), _ptr(psi), C.byref(st)))
        return psi, st

    def comp_q(self, psi):
        psi = _f64(psi, self.shape(0))
        q = np.empty(self.shape(1))
        self._chk(self.L.msom_comp_q(self.h, _ptr(psi), _ptr(q)))
        return q

    # -- msqg/qg_bfn.h
    def pystep_bfn(self, var, tend, direction=1.0, vartype=1):
        var = _f64(var)
        assert tend.dtype == np.float64 and tend.flags.c_contiguous
        self._chk(self.L.pystep_bfn(self.h, _ptr(var), *var.shape, _ptr(tend), *tend.shape, direction, vartype))

    def pyq2p(self, p, q):
        q = _f64(q)
        assert p.dtype == np.float64 and p.flags.c_contiguous
        self._chk(self.L.pyq2p(self.h, _ptr(p), *p.shape, _ptr(q), *q.shape))

    def pyp2q(self, p, q):
        p = _f64(p)
        assert q.dtype == np.float64 and q.flags.c_contiguous
        self._chk(self.L.pyp2q(self.h, _ptr(p), *p.shape, _ptr(q), *q.shape))

    # -- the loop of msqg/qg_bfn.py:47-73 on the device; state Q, observations BFN_OBS, gain BFN_GAIN, history BFN_F1..F3
    def bfn_begin(self):
        """zero AB3 history (msqg/qg_bfn.py:49-51)"""
        self._chk(self.L.msom_bfn_begin(self.h))

    def bfn_steps(self, nsteps, dt, direction=1.0, k=0.0):
        """nsteps times: F1 = pystep_bfn tendency of Q + (k * gain) * (obs - Q); Q += dt / 12 * (23 F1 - 16 F2 + 5 F3); rotate the history.
        dt is signed (backward: dt < 0, direction = -1)."""
        self._chk(self.L.msom_bfn_steps(self.h, int(nsteps), float(dt), float(direction), float(k)))

    def bfn_misfit(self):
        """sqrt(sum gain (obs - Q)^2 / sum gain)"""
        out = C.c_double()
        self._chk(self.L.msom_bfn_misfit(self.h, C.byref(out)))
        return out.value

    # -- running time means and eddy statistics on the device (STATS), time_filter of msqg/qg.h:491-507
    def stats_begin(self, mask):
        """allocate and zero the accumulators of `mask` (bit STATS[name] each) and the weight sum; option("stats", 1) then lets
        every step() take one sample of (q_n, psi_n) with weight dt_n"""
        self._chk(self.L.msom_stats_begin(self.h, int(mask)))

    def stats_accumulate(self, w):
        """one sample of the PSI and Q the model holds now, weight w"""
        self._chk(self.L.msom_stats_accumulate(self.h, float(w)))

    def stats_weight(self):
        out = C.c_double()
        self._chk(self.L.msom_stats_weight(self.h, C.byref(out)))
        return out.value

    def stats_get(self, which, out=None):
        """mean of accumulator `which` (sum / weight), a derived quantity (EKE, UQ_EDDY, VQ_EDDY) or QME; [nl][ny][nx] of this tile.
        out: optional destination, a numpy array or a tensor (host or device)"""
        a = np.empty((self.nl, self.ny, self.nx)) if out is None else out
        self._chk(self.L.msom_stats_get(self.h, int(which), _ptr(a)))
        return a

    def time_filter(self, dt):
        """qo_me = (1 - a) * qo_me + a * Q, a = dt / tau_f (option "tau_f", 20); read it back with stats_get(STATS["QME"])"""
        self._chk(self.L.msom_time_filter(self.h, float(dt)))

    # -- Lagrangian floats advected on the device with the model's RK2 stages (include/msom_floats.h).  On a tiled handle they need
    # option("floats_tiles", 1) before floats_begin (option("floats_msg_cap", K): records per migration message); every floats_* call
    # and param("floats_clamped" / "floats_lost" / "floats_unsent" / "floats_migrated") is then collective: every rank makes the same
    # calls in the same order, with the same global arrays, and receives the full arrays in the caller's order
    def floats_begin(self, x, y, layer):
        """n floats at (x, y) in domain coordinates, layer[k] in [0, nl); host arrays or device tensors (float64, float64, int32).
        From here on every step() moves them; option("floats", 0) pauses that (on tiles: alike on all ranks).  On tiles collective:
        every rank passes the same global arrays and keeps the floats it owns"""
        if not hasattr(layer, "data_ptr"):
            layer = np.ascontiguousarray(layer, dtype=np.int32)
        x, y = _f64(x), _f64(y)
        n = int(x.shape[0])
        if tuple(x.shape) != (n,) or tuple(y.shape) != (n,) or tuple(layer.shape) != (n,):
            raise ValueError(f"x, y, layer of shapes {tuple(x.shape)}, {tuple(y.shape)}, {tuple(layer.shape)}: want three [n]")
        self._chk(self.L.msom_floats_begin(self.h, n, _ptr(x), _ptr(y), _ptr(layer)))

    def floats_end(self):
        self._chk(self.L.msom_floats_end(self.h))

    def _floats_n(self):
        return max(int(self.param("floats")), 0)

    def floats_get(self):
        """(x, y): the current positions in the caller's order (on tiles collective: all n floats on every rank)"""
        x, y = np.empty(self._floats_n()), np.empty(self._floats_n())
        self._chk(self.L.msom_floats_get(self.h, _ptr(x), _ptr(y)))
        return x, y

    def floats_velocity(self):
        """(u, v) at the current positions from the PSI the model holds now (on tiles collective, and not between a stage 1 and its
        stage 2 by hand)"""
        u, v = np.empty(self._floats_n()), np.empty(self._floats_n())
        self._chk(self.L.msom_floats_velocity(self.h, _ptr(u), _ptr(v)))
        return u, v

    def floats_sample(self, field):
        """the bilinear interpolation of a field of nl layers at the floats, each in its layer (on tiles collective, as floats_velocity;
        the ghost ring is the tile's, which the model exchanges for PSI but not for Q)"""
        out = np.empty(self._floats_n())
        self._chk(self.L.msom_floats_sample(self.h, int(field), _ptr(out)))
        return out

    def floats_stage(self, stage, dt):
        """the advection by hand: stage 1 (xh = x + dt / 2 U(x)) after the first update(), stage 2 (x += dt U(xh)) after the second"""
        self._chk(self.L.msom_floats_stage(self.h, int(stage), float(dt)))

    def floats_record(self, every=1, capacity=1):
        """a trajectory buffer of `capacity` records on the device: record 0 now, then one behind every `every`-th step()"""
        self._chk(self.L.msom_floats_record(self.h, int(every), int(capacity)))

    def floats_track(self, first=0, count=None):
        """(t[count], x[count][n], y[count][n]) of records first .. first + count - 1 (count None: all that are written)"""
        if count is None:
            count = int(self.param("floats_records")) - first
        n = self._floats_n()
        t, x, y = np.empty(max(count, 0)), np.empty((max(count, 0), n)), np.empty((max(count, 0), n))
        self._chk(self.L.msom_floats_track(self.h, int(first), int(count), t.ctypes.data_as(_dp), _ptr(x), _ptr(y)))
        return t, x, y

    def floats_ghosted(self, field):
        """[nl][ny + 2][nx + 2]: a field of nl layers with its one-cell ghost ring, as the float kernels read it"""
        out = np.empty((self.nl, self.ny + 2, self.nx + 2))
        self._chk(self.L.msom_floats_dbg_ghosted(self.h, int(field), _ptr(out)))
        return out

    # -- vertical normal modes of the stretching operator on the device (MODES), msqg/eigmode.h
    def modes_compute(self):
        """eigen-decomposition of the stretching matrix of every column (once, where the stratification is uniform); after set_const"""
        self._chk(self.L.msom_modes_compute(self.h))

    def modes_get(self, which, out=None):
        """the arrays of MODES[name]: [nl or nl*nl][ny][nx] of this tile.  out: optional destination (numpy array or tensor)"""
        n = self.L.msom_modes_layers(self.h, int(which))
        if n < 0:
            self._chk(n)
        a = np.empty((n, self.ny, self.nx)) if out is None else out
        self._chk(self.L.msom_modes_get(self.h, int(which), _ptr(a)))
        return a

    def modes_project(self, a, to_modes, out=None):
        """layers -> modes (to_modes true: sum_k l2m[m][k] a_k) or modes -> layers (sum_m m2l[k][m] a_m) of a [nl][ny][nx] array, host
        or device.  out: optional destination, may be `a` itself; two device arrays are not waited for"""
        a = _f64(a, (self.nl, self.ny, self.nx))
        if out is None:
            out = np.empty((self.nl, self.ny, self.nx))
        self._chk(self.L.msom_modes_project(self.h, 1 if to_modes else 0, _ptr(a), _ptr(out)))
        return out

    def modes_energy(self):
        """(ke, pe): kinetic and potential energy of every mode from the PSI the model holds, summed over the domain (all tiles)"""
        ke, pe = np.empty(self.nl), np.empty(self.nl)
        self._chk(self.L.msom_modes_energy(self.h, ke.ctypes.data_as(_dp), pe.ctypes.data_as(_dp)))
        return ke, pe

    def modes_set_rd(self, mode=1):
        """RD = deformation radius of `mode`, so that the next wavelet_filter builds sig_filt = min(afilt * Rd, Lfmax) from the
        stratification (mode 1: the reference's MODE_PV_INVERT branch, msqg/qg.h:1055-1057)"""
        self._chk(self.L.msom_modes_set_rd(self.h, int(mode)))

    # -- isotropic wavenumber spectra and spectral fluxes on the device (msqg/scripts/fftlib.py, spectra.py, energy_offline.py)
    def spec_bins(self):
        """number of radial bins: max(nx, ny) / 2 - 2"""
        n = self.L.msom_spec_bins(self.h)
        if n < 0:
            self._chk(n)
        return n

    def spec_kr(self):
        """kr[r] = (r + 1) / (max(nx, ny) Delta)"""
        kr = np.empty(self.spec_bins())
        self._chk(self.L.msom_spec_kr(self.h, kr.ctypes.data_as(_dp)))
        return kr

    @staticmethod
    def _spec_pair(a, b):
        a = _f64(a)
        b = a if b is None else _f64(b)
        if len(a.shape) != 3 or tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"arrays of shape {tuple(a.shape)} and {tuple(b.shape)}: want two [layers][ny][nx]")
        return a, b

    def spec_2d(self, a, b=None, out=None):
        """Re(fft2(a) conj fft2(b)) Delta^4, fftshift-ed, of [layers][ny][nx] arrays (host or device; b None: a).  out: optional destination"""
        a, b = self._spec_pair(a, b)
        if out is None:
            out = np.empty(tuple(a.shape))
        self._chk(self.L.msom_spec_2d(self.h, _ptr(a), _ptr(b), int(a.shape[0]), _ptr(out)))
        return out

    def spec_cross(self, a, b=None, flux=False):
        """the isotropic cross-spectrum [layers][nbins] of a and b (b None: a), or with flux=True the spectral flux"""
        a, b = self._spec_pair(a, b)
        out = np.empty((int(a.shape[0]), self.spec_bins()))
        p = out.ctypes.data_as(_dp)
        self._chk(self.L.msom_spec_cross(self.h, _ptr(a), _ptr(b), int(a.shape[0]), None if flux else p, p if flux else None))
        return out

    def spec_fields(self, fa, fb, flux=False):
        """spec_cross of two fields the model holds; nothing but [layers][nbins] numbers leaves the device"""
        n = self.L.msom_field_layers(self.h, int(fa))
        out = np.empty((max(n, 0), self.spec_bins()))
        p = out.ctypes.data_as(_dp)
        self._chk(self.L.msom_spec_fields(self.h, int(fa), int(fb), None if flux else p, p if flux else None))
        return out

    def spec_energy(self):
        """(ke [nl][nbins], pe [nl - 1][nbins]): KE and PE wavenumber spectra of the PSI the model holds (spectra.py:113-139)"""
        nb = self.spec_bins()
        ke, pe = np.empty((self.nl, nb)), np.empty((max(self.nl - 1, 0), nb))
        self._chk(self.L.msom_spec_energy(self.h, ke.ctypes.data_as(_dp), pe.ctypes.data_as(_dp) if self.nl > 1 else None))
        return ke, pe

    # -- modal PV inversion: option("mode_pv_invert", 1) sends every inversion through the modes (MODE_PV_INVERT, msqg/qg.h:116-157)
    def modes_mgstats(self, mode):
        """mgstats of `mode` in the last modal solve (mgstats() gives the last mode's, as the reference's mgpsi)"""
        st = MGStats()
        self._chk(self.L.msom_modes_mgstats(self.h, int(mode), C.byref(st)))
        return st

    def helm_relax(self, lev, da, res, nhalf=2, count_per_mode=None):
        """nhalf red-black half-sweeps (colour 0 first) of a = (sum of the 4 neighbours - D^2 b) / (4 - D^2 iBu_m) on level `lev`, every mode
        in one launch; da, res: [mode][y][x] of that level.  count_per_mode[m]: sweeps mode m takes (None: all; 0: the mode keeps its da)"""
        da = np.array(da, dtype=np.float64, order="C")
        res = _f64(res)
        cnt = None if count_per_mode is None else (C.c_int * self.nl)(*[int(c) for c in count_per_mode])
        self._chk(self.L.msom_dbg_helm_relax(self.h, lev, _ptr(da), _ptr(res), int(nhalf), cnt))
        return da

    def helm_residual(self, a, b):
        """(res, maxres): res_m = b_m - lap(a_m) - iBu_m a_m on the finest level and max |res_m| per mode; a, b: [mode][ny][nx]"""
        a, b = _f64(a, (self.nl, self.ny, self.nx)), _f64(b, (self.nl, self.ny, self.nx))
        res = np.empty_like(a)
        mx = np.empty(self.nl)
        self._chk(self.L.msom_dbg_helm_residual(self.h, _ptr(a), _ptr(b), _ptr(res), mx.ctypes.data_as(_dp)))
        return res, mx

    # -- time loop
    def step(self):
        dt = C.c_double()
        self._chk(self.L.msom_step(self.h, C.byref(dt)))
        return dt.value

    def set_tnext(self, tnext):
        self._chk(self.L.msom_set_tnext(self.h, tnext))

    @property
    def t(self):
        return self.L.msom_time(self.h)

    @property
    def iter(self):
        return self.L.msom_iter(self.h)

    def ke(self):
        return self.L.msom_ke(self.h)

    def mgstats(self):
        st = MGStats()
        self._chk(self.L.msom_last_mgstats(self.h, C.byref(st)))
        return st

    def run(self, workdir=".", nsteps_max=-1):
        self._chk(self.L.msom_run(self.h, workdir.encode(), nsteps_max))

    # wavelet scale filter (msqg/qg.h:509-560)
    def wavelet_filter(self, dtflt):
        self._chk(self.L.msom_wavelet_filter(self.h, dtflt))

    # energy / PV budgets (msqg/qg_energy.h)
    def energy_tend(self, dt):
        self._chk(self.L.msom_energy_tend(self.h, dt))

    def filter_de(self, pm_field, dtflt):
        self._chk(self.L.msom_filter_de(self.h, pm_field, dtflt))

    def reset_de(self):
        self._chk(self.L.msom_reset_de(self.h))

    def pystep_de(self, po, bf, vd, j1, j2, j3, ft, onlyKE=0):
        """bas.pystep_de(p, bf, vd, j1, j2, j3, ft, flag_keonly) of msqg/scripts/energy_offline.py:113"""
        arrs = [_f64(po, (self.nl, self.ny, self.nx))] + [a for a in (bf, vd, j1, j2, j3, ft)]
        args = []
        for a in arrs:
            args += [_ptr(a), self.nl, self.ny, self.nx]
        self._chk(self.L.pystep_de(self.h, *args, int(onlyKE)))

    def wavelet_levels(self):
        n = self.L.msom_dbg_wavelet_levels(self.h)
        if n < 0:
            self._chk(n)
        return n

    def siglev(self, level):
        a = np.empty((1, self.ny >> level, self.nx >> level))
        self._chk(self.L.msom_dbg_siglev(self.h, level, _ptr(a)))
        return a

    def wavelet_apply(self, field):
        self._chk(self.L.msom_dbg_wavelet_apply(self.h, field))

    def write_bas(self, field, path):
        self._chk(self.L.msom_write_bas(self.h, field, path.encode()))

    def read_bas(self, field, path):
        self._chk(self.L.msom_read_bas(self.h, field, path.encode()))

    def write_nc(self, path):
        self._chk(self.L.msom_write_nc(self.h, path.encode()))

    def read_nc(self, field, path, varname, record=-1):
        self._chk(self.L.msom_read_nc(self.h, field, path.encode(), varname.encode(), record))

    # -- debug hooks
    def nlevels(self):
        return self.L.msom_dbg_nlevels(self.h)

    def level_dims(self, lev):
        nx, ny = C.c_int(), C.c_int()
        self._chk(self.L.msom_dbg_level_dims(self.h, lev, C.byref(nx), C.byref(ny)))
        return nx.value, ny.value

    def relax(self, lev, da, res, nsweeps=1):
        da = np.array(da, dtype=np.float64, order="C")
        res = _f64(res)
        self._chk(self.L.msom_dbg_relax(self.h, lev, _ptr(da), _ptr(res), nsweeps))
        return da

    def residual(self, a, b):
        a, b = _f64(a), _f64(b)
        res = np.empty_like(a)
        m = C.c_double()
        self._chk(self.L.msom_dbg_residual(self.h, _ptr(a), _ptr(b), _ptr(res), C.byref(m)))
        return res, m.value

    def dbg_rhs_resid(self, fused, dt):
        """QPRED = Q + dt dq in one tendency pass, then the first residual of its inversion on levels 0 and 1 (raw split arrays, NaN where
        nothing was written), max|res| and the sum of QPRED: fused = out of the pass itself, else from the solver's residual pass"""
        nl = int(self.param("nl"))
        r0 = np.empty((nl, int(self.param("split_ls_0"))))
        r1 = np.empty((nl, int(self.param("split_ls_1"))))
        mx, bs = C.c_double(), C.c_double()
        self._chk(self.L.msom_dbg_rhs_resid(self.h, int(bool(fused)), float(dt), _ptr(r0), _ptr(r1), C.byref(mx), C.byref(bs)))
        return r0, r1, mx.value, bs.value

    def restrict(self, lev_fine, fine):
        fine = _f64(fine)
        nl, ny, nx = fine.shape
        coarse = np.empty((nl, ny // 2, nx // 2))
        self._chk(self.L.msom_dbg_restrict(self.h, lev_fine, _ptr(fine), _ptr(coarse)))
        return coarse

    def prolong(self, lev_coarse, coarse):
        coarse = _f64(coarse)
        nl, ny, nx = coarse.shape
        fine = np.empty((nl, ny * 2, nx * 2))
        self._chk(self.L.msom_dbg_prolong(self.h, lev_coarse, _ptr(coarse), _ptr(fine)))
        return fine

    def op(self, name, f_in, f_out, add=0.0, fac=1.0):
        self._chk(self.L.msom_dbg_op(self.h, name.encode(), f_in, f_out, add, fac))

    # -- measurement
    def profile_read(self, kernel):
        ms, n = C.c_double(), C.c_long()
        self._chk(self.L.msom_profile_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_reset(self):
        self._chk(self.L.msom_profile_reset(self.h))

    def sync(self):
        """wait for the work queued on the handle's stream (msom_step may return before its last kernel has finished)"""
        self._chk(self.L.msom_sync(self.h))

    def bench_kernel(self, kernel, reps=20):
        ms = C.c_double()
        self._chk(self.L.msom_bench_kernel(self.h, kernel.encode(), reps, C.byref(ms)))
        return ms.value

    # -- lossless checkpoint / restart (include/msom_state.h)
    def save_state(self, path, constants=False):
        self._chk(self.L.msom_state_save(self.h, os.fsencode(path), 1 if constants else 0))

    def load_state(self, path):
        self._chk(self.L.msom_state_load(self.h, os.fsencode(path)))

    def state_dbg_flip(self, element):
        self._chk(self.L.msom_state_dbg_flip(self.h, int(element)))


class NewQG:
    """The cell-centred one-layer model with the optional Helmholtz ("1.5-layer", gp_low) inversion: one `qg.e` process of newqg/qg.c
    without its driver's sample forcing (set QFORC instead).  Fields PSI, Q, ZETA, DQ, QPRED, QFORC, arrays [1][ny][nx].  Only the
    calls the dialect has are defined here; the handle answers every other entry point of msom.h with MSOM_ERR_CONFIG."""

    FIELD_IDS = tuple(FIELDS[k] for k in ("PSI", "Q", "ZETA", "DQ", "QPRED", "QFORC"))

    def __init__(self, params=None, path=None, strict=False):
        self.L = load_library(strict)
        self.h = self.L.msom_create_newqg(path.encode()) if path is not None else self.L.msom_create_newqg_str(params.encode())
        if not self.h:
            raise MsomError(self.L.msom_last_error().decode())
        self.nl = 1
        self.nx, self.ny = int(self.param("nx")), int(self.param("ny"))

    close, __del__, _chk = QG.close, QG.__del__, QG._chk
    param, option = QG.param, QG.option
    set_const = QG.set_const
    update, advance, invertq, comp_q = QG.update, QG.advance, QG.invertq, QG.comp_q
    step, set_tnext, t, iter, ke, mgstats = QG.step, QG.set_tnext, QG.t, QG.iter, QG.ke, QG.mgstats
    write_nc, read_nc = QG.write_nc, QG.read_nc
    profile_read, profile_reset, sync, bench_kernel = QG.profile_read, QG.profile_reset, QG.sync, QG.bench_kernel
    save_state, load_state, state_dbg_flip = QG.save_state, QG.load_state, QG.state_dbg_flip

    def shape(self, field):
        return (self.L.msom_field_layers(self.h, field), self.ny, self.nx)

    def set(self, field, a):
        a = _f64(a, (1, self.ny, self.nx))
        self._chk(self.L.msom_set_field(self.h, field, _ptr(a)))

    def get(self, field):
        a = np.empty((1, self.ny, self.nx))
        self._chk(self.L.msom_get_field(self.h, field, _ptr(a)))
        return a

    def level_dims(self):
        """(nx, ny) of every multigrid level, finest first"""
        return [(self.nx >> k, self.ny >> k) for k in range(int(self.param("nlevels")))]


# ---------------------------------------------------------------------------
# module-level mirror of the reference's single-instance `import qg` surface
# (msqg/qg_bfn.py:33-37: read_params -> init_grid -> set_vars -> set_vars_bfn -> set_const)

_state = {"path": None, "model": None}


def read_params(path2file):
    _state["path"] = path2file


def init_grid(N):  # grid size comes from params.in; kept for call-compatibility
    return None


def set_vars():
    if _state["path"] is None:
        raise MsomError("read_params() must be called first")
    _state["model"] = QG(path=_state["path"])
    d = os.path.dirname(os.path.abspath(_state["path"]))
    _state["model"].option("quiet", 1)
    _state["model"].read_inputs(d)


def set_vars_bfn():
    return None


def set_const():
    _state["model"].set_const()


def pystep_bfn(var, tend, direction, vartype):
    _state["model"].pystep_bfn(var, tend, direction, vartype)


def bfn_begin():
    _state["model"].bfn_begin()


def bfn_steps(nsteps, dt, direction=1.0, k=0.0):
    """the loop of msqg/qg_bfn.py:62-73 on the device; state and inputs through the model's fields
    (FIELDS: Q, BFN_OBS, BFN_GAIN, BFN_F1..F3)"""
    _state["model"].bfn_steps(nsteps, dt, direction, k)


def bfn_misfit():
    return _state["model"].bfn_misfit()


def pyq2p(p, q):
    _state["model"].pyq2p(p, q)


def pyp2q(p, q):
    _state["model"].pyp2q(p, q)


def pystep_de(p, bf, vd, j1, j2, j3, ft, onlyKE=0):
    """msqg/qg_energy.i:31, called as bas.pystep_de(p,bf,vd,j1,j2,j3,ft,flag_keonly) (msqg/scripts/energy_offline.py:113)"""
    _state["model"].pystep_de(p, bf, vd, j1, j2, j3, ft, onlyKE)


def trash_vars():
    if _state["model"] is not None:
        _state["model"].close()
        _state["model"] = None


def trash_vars_bfn():
    return None


NODE_FIELDS = dict(PSI=0, Q=1, ZETA=2, TMP=3, PSIPG=4, S2=5, TOPO=6, QFORC=7, MASK=8, DQ=9, QPRED=10, QFORC3D=11, BS=12, S2S=13, PSIF=14)


class NodeQG:
    """Vertex-grid (masked-domain) model: one `qg.e` process of qg-node/qg.c.  Field arrays are
    [layers][N+1][N+1] (qg-node/netcdf_vertex_bas.h:253).
    tiled = (px, py, rank, uid): this rank's tile of a px x py decomposition (msomn_create_tiled); field arrays are then the tile's
    [layers][ny][nx] with nx = N / px + 1, ny = N / py + 1 vertices, the ones on the interior edges included
    (msom_amd.tiling.node_tile_window), and set(), set_const() and every call that computes are collective.  With
    set_option("io_tiles", 1) so are save_state / load_state / write_nc / read_nc / run: rank 0 writes the single tile's files, every
    rank reads its window of them (node_from_state(path, tiled=...) makes the tiles from a state file)."""

    def __init__(self, params=None, path=None, strict=False, tiled=None):
        self.L = load_library(strict)
        if tiled is not None:
            px, py, rank, uid = tiled
            self.h = self.L.msomn_create_tiled(params.encode(), px, py, rank, uid)
        else:
            self.h = self.L.msomn_create(path.encode()) if path is not None else self.L.msomn_create_str(params.encode())
        if not self.h:
            raise MsomError(self.L.msom_last_error().decode())
        self._read_shape()

    def _read_shape(self):
        self.N, self.nl = int(self.param("N")), int(self.param("nl"))
        self.nlevels = int(self.param("nlevels"))
        px_, py_, ix, iy, nx, ny = (C.c_int() for _ in range(6))
        self.L.msomn_tile_info(self.h, *(C.byref(v) for v in (px_, py_, ix, iy, nx, ny)))
        self.nx, self.ny = nx.value, ny.value
        self.tile = (px_.value, py_.value, ix.value, iy.value)

    def close(self):
        if self.h:
            self.L.msomn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != 0:
            e = MsomError(f"error {r}: {self.L.msom_last_error().decode()}")
            e.code = r
            raise e

    def _fid(self, f):
        return NODE_FIELDS[f] if isinstance(f, str) else int(f)

    def param(self, key):
        return self.L.msomn_get_param(self.h, key.encode())

    def set_option(self, key, v):
        self._chk(self.L.msomn_set_option(self.h, key.encode(), float(v)))

    def profile_read(self, slot):
        ms, n = C.c_double(), C.c_long()
        self._chk(self.L.msomn_profile_read(self.h, slot.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_reset(self):
        self._chk(self.L.msomn_profile_reset(self.h))

    def layers(self, f):
        return self.L.msomn_field_layers(self.h, self._fid(f))

    def shape(self, f):
        return (self.layers(f), self.ny, self.nx)

    def set(self, f, a):
        a = _f64(a, self.shape(f))
        self._chk(self.L.msomn_set_field(self.h, self._fid(f), _ptr(a)))

    def get(self, f):
        a = np.empty(self.shape(f))
        self._chk(self.L.msomn_get_field(self.h, self._fid(f), _ptr(a)))
        return a

    def set_const(self):
        self._chk(self.L.msomn_set_const(self.h))

    def update(self, q="Q", dq="DQ", dtmax=None):
        dt = C.c_double()
        self._chk(self.L.msomn_update(self.h, self._fid(q), self._fid(dq), self.param("DT") if dtmax is None else dtmax, C.byref(dt)))
        return dt.value

    def advance(self, out, inp, dq, dt):
        self._chk(self.L.msomn_advance(self.h, self._fid(out), self._fid(inp), self._fid(dq), dt))

    def invert_q(self, q="Q"):
        st = MGStats()
        self._chk(self.L.msomn_invert_q(self.h, self._fid(q), C.byref(st)))
        return st

    def comp_q(self, psi="PSI", q="Q"):
        self._chk(self.L.msomn_comp_q(self.h, self._fid(psi), self._fid(q)))

    def rhs_pv(self, q="Q", dq="DQ"):
        self._chk(self.L.msomn_rhs_pv(self.h, self._fid(q), self._fid(dq)))

    def forcing(self):
        self._chk(self.L.msomn_forcing(self.h))

    def step(self, with_forcing_event=False):
        self._chk(self.L.msomn_step(self.h, int(with_forcing_event)))

    def set_tnext(self, t):
        self._chk(self.L.msomn_set_tnext(self.h, t))

    @property
    def t(self):
        return self.L.msomn_time(self.h)

    @property
    def dt(self):
        return self.L.msomn_dt(self.h)

    @property
    def iter(self):
        return self.L.msomn_iter(self.h)

    def ke(self):
        v = C.c_double()
        self._chk(self.L.msomn_ke(self.h, C.byref(v)))
        return v.value

    def mgstats(self):
        st = MGStats()
        self._chk(self.L.msomn_last_mgstats(self.h, C.byref(st)))
        return st

    # -- running time means and eddy statistics on the device (STATS without QME; msomn_stats_* of include/msom.h)
    def stats_begin(self, mask):
        """allocate and zero the accumulators of `mask` (bit STATS[name] each) and the weight sum; set_option("stats", 1) then lets
        every step() take one sample of (q_n, psi_n) with weight dt_n"""
        self._chk(self.L.msomn_stats_begin(self.h, int(mask)))

    def stats_accumulate(self, w):
        """one sample of the PSI, Q and MASK the model holds now, weight w (collective on tiles)"""
        self._chk(self.L.msomn_stats_accumulate(self.h, float(w)))

    def stats_weight(self):
        out = C.c_double()
        self._chk(self.L.msomn_stats_weight(self.h, C.byref(out)))
        return out.value

    def stats_get(self, which, out=None):
        """mean of accumulator `which` (sum / weight) or a derived quantity (EKE, UQ_EDDY, VQ_EDDY; collective on tiles);
        [nl][ny][nx] of this tile.  out: optional destination, a numpy array or a tensor (host or device)"""
        a = np.empty((self.nl, self.ny, self.nx)) if out is None else out
        self._chk(self.L.msomn_stats_get(self.h, int(which), _ptr(a)))
        return a

    # -- Lagrangian floats advected on the device with the model's RK2 stages (include/msomn_floats.h).  On a tiled handle they need
    # set_option("floats_tiles", 1) before floats_begin (set_option("floats_msg_cap", K): records per migration message); every
    # floats_* call and param("floats_clamped" / "floats_lost" / "floats_unsent" / "floats_migrated" / "floats_on_land") is then
    # collective: every rank makes the same calls in the same order
    def floats_begin(self, x, y, layer):
        """n floats at (x, y) in [0, L0]^2, layer[k] in [0, nl); host arrays or device tensors (float64, float64, int32).  From here
        on every step() moves them; set_option("floats", 0) pauses that (on tiles: alike on all ranks).  A start on land is accepted.
        On tiles collective: every rank passes the same global arrays and keeps the floats it owns"""
        if not hasattr(layer, "data_ptr"):
            layer = np.ascontiguousarray(layer, dtype=np.int32)
        x, y = _f64(x), _f64(y)
        n = int(x.shape[0])
        if tuple(x.shape) != (n,) or tuple(y.shape) != (n,) or tuple(layer.shape) != (n,):
            raise ValueError(f"x, y, layer of shapes {tuple(x.shape)}, {tuple(y.shape)}, {tuple(layer.shape)}: want three [n]")
        self._chk(self.L.msomn_floats_begin(self.h, n, _ptr(x), _ptr(y), _ptr(layer)))
        self._floats_field = False   # a begin drops the trajectory buffer

    def floats_end(self):
        self._chk(self.L.msomn_floats_end(self.h))

    def _floats_n(self):
        return max(int(self.param("floats")), 0)

    def floats_get(self):
        """(x, y): the current positions in the caller's order (on tiles collective: all n floats on every rank)"""
        x, y = np.empty(self._floats_n()), np.empty(self._floats_n())
        self._chk(self.L.msomn_floats_get(self.h, _ptr(x), _ptr(y)))
        return x, y

    def floats_velocity(self):
        """(u, v) at the current positions from the PSI (+ PSIPG) the model holds now (on tiles collective, each float on its owner;
        not between a stage 1 and its stage 2)"""
        u, v = np.empty(self._floats_n()), np.empty(self._floats_n())
        self._chk(self.L.msomn_floats_velocity(self.h, _ptr(u), _ptr(v)))
        return u, v

    def floats_sample(self, field):
        """the bilinear interpolation of a field of nl layers at the floats, each in its layer (on tiles collective, as
        floats_velocity)"""
        out = np.empty(self._floats_n())
        self._chk(self.L.msomn_floats_sample(self.h, self._fid(field), _ptr(out)))
        return out

    def floats_stage(self, stage, dt):
        """the advection by hand: stage 1 (xh = x + dt / 2 U(x)) after the first update(), stage 2 (x += dt U(xh)) after the second
        update() and the final advance()"""
        self._chk(self.L.msomn_floats_stage(self.h, int(stage), float(dt)))

    def floats_record(self, every=1, capacity=1, field=None):
        """a trajectory buffer of `capacity` records on the device: record 0 now, then one behind every `every`-th step(); field: a
        field of nl layers whose value at the new positions is recorded with them ("Q": PV on parcels)"""
        self._chk(self.L.msomn_floats_record(self.h, int(every), int(capacity), -1 if field is None else self._fid(field)))
        self._floats_field = field is not None

    def floats_track(self, first=0, count=None):
        """(t[count], X[count][n], Y[count][n]) of records first .. first + count - 1 (count None: all that are written), and
        V[count][n] as a fourth when a field is recorded (on tiles collective: every record of all n floats on every rank)"""
        if count is None:
            count = int(self.param("floats_records")) - first
        n, c = self._floats_n(), max(count, 0)
        t, x, y = np.empty(c), np.empty((c, n)), np.empty((c, n))
        v = np.empty((c, n)) if getattr(self, "_floats_field", False) else None
        self._chk(self.L.msomn_floats_track(self.h, int(first), int(count), t.ctypes.data_as(_dp), _ptr(x), _ptr(y), _ptr(v)))
        return (t, x, y) if v is None else (t, x, y, v)

    def diag1d(self):
        out = (C.c_double * 3)()
        self._chk(self.L.msomn_diag1d(self.h, out))
        return np.array(out[:])

    def write_nc(self, path):
        self._chk(self.L.msomn_write_nc(self.h, path.encode()))

    def read_nc(self, f, path, var, record=-1):
        self._chk(self.L.msomn_read_nc(self.h, self._fid(f), path.encode(), var.encode(), record))

    def run(self, workdir=".", nsteps_max=-1):
        r = self.L.msomn_run(self.h, workdir.encode(), nsteps_max)
        if r < 0:
            self._chk(r)
        return r

    # multigrid pieces (parity tests); level k has (N >> k) + 1 vertices per side (a tile: its share of them, plus one)
    def _lshape(self, k, nl=None):
        return (self.nl if nl is None else nl, ((self.ny - 1) >> k) + 1, ((self.nx - 1) >> k) + 1)

    def dbg_relax(self, k, da, res, nsweeps):
        da = np.array(_f64(da, self._lshape(k)))
        res = _f64(res, self._lshape(k))
        self._chk(self.L.msomn_dbg_relax(self.h, k, _ptr(da), _ptr(res), nsweeps))
        return da

    def dbg_residual(self, a, b):
        a, b = _f64(a, self._lshape(0)), _f64(b, self._lshape(0))
        res = np.empty(self._lshape(0))
        mx = C.c_double()
        self._chk(self.L.msomn_dbg_residual(self.h, _ptr(a), _ptr(b), _ptr(res), C.byref(mx)))
        return res, mx.value

    def dbg_restrict(self, k, fine):
        fine = _f64(fine, self._lshape(k))
        out = np.empty(self._lshape(k + 1))
        self._chk(self.L.msomn_dbg_restrict(self.h, k, _ptr(fine), _ptr(out)))
        return out

    def dbg_prolong(self, k, coarse):
        coarse = _f64(coarse, self._lshape(k))
        out = np.empty(self._lshape(k - 1))
        self._chk(self.L.msomn_dbg_prolong(self.h, k, _ptr(coarse), _ptr(out)))
        return out

    def dbg_level_mask(self, k):
        out = np.empty(self._lshape(k, 1))
        self._chk(self.L.msomn_dbg_level_mask(self.h, k, _ptr(out)))
        return out

    def dbg_del2_zeta(self):
        self._chk(self.L.msomn_dbg_del2_zeta(self.h))

    def _cshape(self, k=0):
        """cells of level k of the noise / wavelet pyramids as this handle holds them: the tile's window ((ny - 1, nx - 1) >> k) below
        the gather level (param agg_level), the global level (N >> k a side) at and above it; one tile: always the global level (and so without the option wavelet_tiles,
        where the library refuses these calls on tiles)"""
        if self.tile[0] * self.tile[1] > 1 and self.param("wavelet_tiles") == 1 and k < int(self.param("agg_level")):
            return (self.ny - 1) >> k, (self.nx - 1) >> k
        return self.N >> k, self.N >> k

    # stochastic forcing (cell scalars; on tiles, option wavelet_tiles = 1: the tile's window, collective)
    def noise(self, set=None, filter=False):
        out = np.empty(self._cshape())
        a = None if set is None else _f64(set, self._cshape())
        self._chk(self.L.msomn_dbg_noise(self.h, _ptr(a), int(filter), _ptr(out)))
        return out

    def noise_draw(self, filter=True):
        """the next draw into n_stoch (option noise_mode 1: device generator, 0: host rand() stream), wavelet-filtered if `filter`;
        read it back with noise()"""
        self._chk(self.L.msomn_noise_draw(self.h, int(filter)))

    def csig(self, k):
        out = np.empty(self._cshape(k))
        self._chk(self.L.msomn_dbg_csig(self.h, k, _ptr(out)))
        return out

    # wavelet filter of the vertex model (qg_baroclinic_ms.h:346-400)
    def wavelet_filter(self, dtflt):
        self._chk(self.L.msomn_wavelet_filter(self.h, dtflt))

    def wv_get(self, what, k):
        out = np.empty(self._cshape(k))
        self._chk(self.L.msomn_dbg_wv_get(self.h, what, k, _ptr(out)))
        return out

    def wv_apply(self, cells):
        cells = _f64(cells, (self.nl,) + self._cshape())
        out = np.empty_like(cells)
        self._chk(self.L.msomn_dbg_wv_apply(self.h, _ptr(cells), _ptr(out)))
        return out

    # -- lossless checkpoint / restart (include/msomn_state.h)
    def save_state(self, path, constants=False):
        self._chk(self.L.msomn_state_save(self.h, os.fsencode(path), 1 if constants else 0))

    def load_state(self, path):
        self._chk(self.L.msomn_state_load(self.h, os.fsencode(path)))

    def state_dbg_flip(self, element):
        self._chk(self.L.msomn_state_dbg_flip(self.h, int(element)))
