"""parity.oracle_from on the CPU: an oracle restarted from another oracle's state mid-run continues that run bit for bit.  The GPU shadow
tests (test_shadow_gpu.py) restart an oracle from the HIP engine's state before every step they check; were the restart lossy, a
difference they report could be the restart's, and an agreement could hide one."""
import numpy as np
import pytest

import parity


def _assert_oracles_bit_equal(a, b):
    from oracle import orc
    for f in orc.FIELDS:
        assert np.array_equal(a.get(f), b.get(f)), f
    for ra, rb in zip(a.rings(), b.rings()):
        assert np.array_equal(ra, rb), "rings"
    for pa, pb in zip(a.pairs(), b.pairs()):
        assert np.array_equal(pa, pb), "pairs"
    for ia, ib in zip(a.interactions(), b.interactions()):
        assert np.array_equal(ia, ib), "interactions"
    for xa, xb in zip(a.ids(), b.ids()):
        assert np.array_equal(xa, xb), "ids / status"
    assert np.array_equal(a.warn_counts(), b.warn_counts()), "warn_counts"          # (the guards that fired in the last step)


@pytest.mark.parametrize("kind", ["periodic", "walls-strait"])
def test_oracle_restarted_mid_run_continues_bit_for_bit(kind):
    from oracle import orc
    from subzero_jl_amd import fields
    if kind == "periodic":
        cfg = fields.make_config(n_floes=1500, seed=41)
    else:
        cfg = fields.make_config(n_floes=1500, seed=42, walls=True, topography=True, ocean="strait")
    a = fields.build_world(orc.World(), cfg); a.set_threads(parity.cores())
    k0, k1, dt = 24, 28, cfg["dt"]
    for t in range(k0):
        a.timestep_sim(t, dt, coupling_dt=1)
    # the state really is a mid-run one: contacts, stresses and the integrator's previous derivatives are all set
    assert np.count_nonzero(a.get("overarea")) > 100 and np.all(a.get("p_dudt") != 0) and np.any(a.get("sa11") != 0)
    if kind == "walls-strait":
        rows = a.interactions()[1]
        assert np.any((rows[:, 0] < 0) & (rows[:, 0] >= -4)) and np.any(rows[:, 0] < -4)      # wall and topography contacts
    b = parity.oracle_from(a, cfg); b.set_threads(parity.cores())
    for t in range(k0, k1):
        a.timestep_sim(t, dt, coupling_dt=1)
        b.timestep_sim(t, dt, coupling_dt=1)
    _assert_oracles_bit_equal(a, b)
