"""msom_amd -- MI355X-native multi-layer quasi-geostrophic timestepper.

The product is the HIP library ``msom_amd/lib/libmsomhip.so`` (C ABI: ``include/msom.h``).
This package is the thin Python host mirror of the reference's SWIG module ``qg``
(msqg/qg.i, msqg/qg_bfn.i): same function names, same argument order, numpy arrays
``[layer][y][x]``.  There is no CPU fallback: importing works anywhere, creating a model
without the built HIP library or without a GPU raises.
"""
from .api import (  # noqa: F401
    FIELDS,
    MGStats,
    MODES,
    MsomError,
    NODE_FIELDS,
    NewQG,
    NodeQG,
    QG,
    STATS,
    bfn_begin,
    bfn_misfit,
    bfn_steps,
    from_state,
    init_grid,
    load_library,
    node_from_state,
    pyp2q,
    pyq2p,
    pystep_bfn,
    pystep_de,
    read_params,
    read_state,
    set_const,
    set_vars,
    set_vars_bfn,
    spec_layout,
    state_check,
    state_info,
    trash_vars,
    trash_vars_bfn,
    write_state,
)

__all__ = [
    "QG", "NodeQG", "NewQG", "NODE_FIELDS", "MGStats", "MsomError", "FIELDS", "STATS", "MODES", "load_library", "read_params", "init_grid", "set_vars",
    "set_vars_bfn", "set_const", "pystep_bfn", "bfn_begin", "bfn_steps", "bfn_misfit", "pystep_de", "pyq2p", "pyp2q", "trash_vars", "trash_vars_bfn", "spec_layout",
    "from_state", "node_from_state", "read_state", "write_state", "state_check", "state_info",
]
