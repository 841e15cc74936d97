"""The two kernels of mfh_modal_transient alone (k_modal_march, k_modal_series, mfh_modal.hip) through the hook mfh_debug_modal_march, on tables that
mix rigid, under-damped, critical, over-damped and high-omega-dt modes. The coefficients are the LIBRARY's (they have their own test,
tests/test_modal_transient_reference.py), so this tests the recurrence: the device's states against the long-double twin of
tests/modal_transient_util.py on the same table, within ten times the float64 twin's own defect against it (every mode on its own scale: rel_max);
the probe sums within modal_util.expand_bound of the device's own modal coordinates; the energies within the bound that follows from the two; and
identical bits whatever the chunk length, for chained calls and for a repeated call."""
import numpy as np
import pytest

import meshfem_amd as M

import modal_transient_util as T
import modal_util as MU

pytestmark = pytest.mark.gpu

EPS = T.EPS
DT = 0.01
STEPS = (0, 1, 31, 32, 33, 2 * 32 + 3, 4000)


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def _table(m, seed=5):
    """(lam, c, coef [m, 8], g, q0, v0): modes cycling through rigid undamped, rigid damped, lightly damped, critical, over-damped (5 x critical),
    undamped with omega dt up to 30, the rest under-damped at random."""
    rng = np.random.default_rng(seed + m)
    lam = 10.0 ** rng.uniform(0.0, 5.0, m)
    w = np.sqrt(lam)
    c = 2.0 * w * rng.uniform(0.0, 0.2, m)
    kind = np.arange(m) % 8
    lam[kind == 0] = 0.0
    c[kind == 0] = 0.0
    lam[kind == 1] = 0.0
    c[kind == 1] = 0.5
    c[kind == 3] = 2.0 * w[kind == 3]
    c[kind == 4] = 10.0 * w[kind == 4]
    lam[kind == 5] = (rng.uniform(3.0, 30.0, np.count_nonzero(kind == 5)) / DT) ** 2
    c[kind == 5] = 0.0
    coef = M.modal_transient_coeffs(lam, c, DT)
    return lam, c, coef, rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)


def _amp(n_steps, seed=3):
    return np.random.default_rng(seed).standard_normal(n_steps + 1)


def _check_states(r, coef, g, amp, q0, v0, what):
    defect, QL, VL = T.twin_defect(coef, g, amp, DT, q0, v0)
    eq = T.rel_max(r["modal_coords"], QL)
    print("%s: q %.3e, defect of the twin %.3e" % (what, eq, defect))
    assert eq <= 10 * defect
    assert np.array_equal(r["q"], r["modal_coords"][-1])
    # the last row of q' is what the call returns (every row of q' enters the energies, checked there): each mode on the scale rel_max gives it
    scale_v = np.abs(VL).max(axis=0)
    assert np.all(np.abs(r["qdot"] - VL[-1]) <= 10 * defect * np.where(scale_v > 0, scale_v, 1.0))
    return defect, QL, VL


@pytest.mark.parametrize("m", [1, 63, 64, 65, 256])
def test_march_against_the_twin(ctx, m):
    """nSteps in {0, 1, 31, 32, 33, 67, 4000} at chunkSteps 32 (rows = nSteps + 1 fall before, on and behind the chunk edge), probes and the correction
    column cycling through {0, 1, 3, 17} x {off, on}, energies on."""
    lam, c, coef, g, q0, v0 = _table(m)
    rng = np.random.default_rng(m)
    for k, n_steps in enumerate(STEPS):
        amp = _amp(n_steps)
        n_probe, corr = (0, 1, 3, 17)[k % 4], bool((k // 2) % 2)
        Bp = rng.standard_normal((m + corr, n_probe)) if n_probe else None
        r = ctx.debug_modal_march(coef, g, amp, DT, q0, v0, chunk_steps=32, Bp=Bp, corr=corr, lam=lam, energies=True)
        defect, QL, VL = _check_states(r, coef, g, amp, q0, v0, "m %d, %d steps" % (m, n_steps))
        assert np.array_equal(r["modal_coords"][0], q0)
        if n_probe:
            Cm = np.vstack([r["modal_coords"].T] + ([amp[None, :]] if corr else []))
            ref = (Cm.astype(np.longdouble).T @ Bp.astype(np.longdouble))
            assert np.all(np.abs(r["probes"] - ref) <= MU.expand_bound(Bp, Cm))
        # energies: from |q - q_ref| <= dq = 10 defect max_n |q_ref| per mode (and dv alike) and the fma chains of m + 2 terms
        dq, dv = 10 * defect * np.abs(QL).max(axis=0).astype(np.float64), 10 * defect * np.abs(VL).max(axis=0).astype(np.float64)
        Q, V = QL.astype(np.float64), VL.astype(np.float64)
        E = T.energies_of(lam, g, amp, QL, VL).astype(np.float64)
        bke = np.sum(np.abs(V) * dv + 0.5 * dv * dv, axis=1) + (m + 3) * EPS * E[:, 0]
        bpe = np.sum(lam * (np.abs(Q) * dq + 0.5 * dq * dq), axis=1) + (m + 4) * EPS * E[:, 1]
        bw = np.abs(amp) * (np.abs(g) @ dq + (m + 3) * EPS * (np.abs(Q) @ np.abs(g)))
        for col, b in enumerate((bke, bpe, bw)):
            assert np.all(np.abs(r["energies"][:, col] - E[:, col]) <= b), (n_steps, col)


@pytest.mark.parametrize("corr", [False, True])
@pytest.mark.parametrize("n_probe", [1, 3, 17])
def test_probe_sums(ctx, n_probe, corr):
    """65 modes (four tiles of 16 and one of 1), 67 steps: the probe sums within expand_bound, and bit for bit the chain of k_modal_expand on the same
    numbers (the hook mfh_debug_modal_expand on the device's modal coordinates)."""
    m, n_steps = 65, 67
    lam, c, coef, g, q0, v0 = _table(m)
    amp = _amp(n_steps)
    Bp = np.random.default_rng(n_probe).standard_normal((m + corr, n_probe))
    r = ctx.debug_modal_march(coef, g, amp, DT, q0, v0, chunk_steps=32, Bp=Bp, corr=corr)
    Cm = np.vstack([r["modal_coords"].T] + ([amp[None, :]] if corr else []))
    ref = Cm.astype(np.longdouble).T @ Bp.astype(np.longdouble)
    assert np.all(np.abs(r["probes"] - ref) <= MU.expand_bound(Bp, Cm))
    assert np.array_equal(r["probes"], ctx.debug_modal_expand(Bp, Cm))


@pytest.mark.parametrize("m", [1, 65, 256])
def test_identical_bits(ctx, m):
    """chunkSteps 32 / 64 / default; one call against two chained calls cut at step 45 (no chunk edge); a repeated call."""
    lam, c, coef, g, q0, v0 = _table(m)
    n_steps = 2 * 64 + 3
    amp = _amp(n_steps)
    Bp = np.random.default_rng(m).standard_normal((m + 1, 3))
    kw = dict(Bp=Bp, corr=True, lam=lam, energies=True)
    keys = ("q", "qdot", "modal_coords", "probes", "energies")
    one = ctx.debug_modal_march(coef, g, amp, DT, q0, v0, chunk_steps=32, **kw)
    for chunk in (32, 64, 0):
        r = ctx.debug_modal_march(coef, g, amp, DT, q0, v0, chunk_steps=chunk, **kw)
        for k in keys:
            assert np.array_equal(r[k], one[k]), (chunk, k)
    cut = 45
    a = ctx.debug_modal_march(coef, g, amp[:cut + 1], DT, q0, v0, chunk_steps=32, **kw)
    b = ctx.debug_modal_march(coef, g, amp[cut:], DT, a["q"], a["qdot"], chunk_steps=32, **kw)
    for k in ("modal_coords", "probes", "energies"):
        assert np.array_equal(a[k], one[k][:cut + 1]), k
        assert np.array_equal(b[k], one[k][cut:]), k
    assert np.array_equal(b["q"], one["q"]) and np.array_equal(b["qdot"], one["qdot"])


def test_hook_refusals(ctx):
    lam, c, coef, g, q0, v0 = _table(4)
    for chunk in (-32, 31, 33):
        with pytest.raises(M.MeshFEMHipError):
            ctx.debug_modal_march(coef, g, _amp(5), DT, q0, v0, chunk_steps=chunk)
