"""The profile slots of a handle: msom_destroy, msom_profile_reset and msom_profile_read share one table of (name, slot) pairs.
Every one of the 17 names must read, reset must clear every slot, and a name that is not in the table is an argument error."""
import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F, MsomError

pytestmark = pytest.mark.gpu

SLOTS = ["sweep", "residual", "block2", "march2", "march3", "march4", "march_pl", "march_corr", "march_visit", "resid_max", "rhs",
         "red_prolong", "resid_correct", "resid_restrict", "helm_relax", "helm_residual", "helm_coarse"]


def test_profile_slots():
    N, nl = 16, 1
    g = QG(orc.double_gyre_params(N, nl))
    try:
        g.option("quiet", 1)
        g.set(F["PSI"], orc.synthetic_psi(nl, N, N))
        g.set_const()
        g.option("profile", 1)
        g.step()
        g.sync()
        launches = {}
        for name in SLOTS:
            ms, n = g.profile_read(name)
            assert n >= 0 and np.isfinite(ms) and ms >= 0, (name, ms, n)
            launches[name] = n
        print("launches per slot after one step:", launches)
        assert launches["rhs"] >= 1 and launches["residual"] >= 1, launches
        g.profile_reset()
        for name in SLOTS:
            assert g.profile_read(name) == (0.0, 0), name
        for name in ("no_such_slot", "march1", "Rhs", ""):
            with pytest.raises(MsomError, match=r"error -1: unknown kernel"):   # MSOM_ERR_ARG
                g.profile_read(name)
    finally:
        g.close()
