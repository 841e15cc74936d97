"""Random vibration and response spectra on the device (mfh_modal_random, mfh_modal_quadratic; docs/design/04_23_modal_random.md) against the numpy
twins of tests/modal_random_util.py on the SAME modes (scipy's dense eigenpairs, tests/modal_util.py), on the four small meshes; against the
library's own sweep (Context.modal_harmonic) where the statement is about it.

The bar on a variance v_i = sigma_i^2 against the long-double twin, with and without the static correction:
    10 x max_i |v_float64 twin - v_long-double twin|  +  truncation max_i |phi_i|^2          (the twin's own rounding; what the factorisation left)
In runs with the correction the twin is given the static solutions the device used: Context.solve of each load on the same context at the same rtol
(option deterministic, so that the call's own static solve returns those bits, as tests/test_gpu_modal.py::test_static_limit_is_context_solve
relies on). Every figure is printed before it is asserted; measured on an MI355X the worst error / bar over the 144 runs is 0.47. The basis
handover from mfh_modes_many on the device is checked at the end of the file."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modal_random_util as R
import modal_util as MU
import modes_util as U

pytestmark = pytest.mark.gpu

EPS = U.EPS
RTOL = MU.RTOL_STATIC
MAXIT = 20000


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, options=(), clamped=True):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    if clamped:
        c.fix_variables(U.clamp_vars(key))
    return c


def _code(fn):
    with pytest.raises(M.MeshFEMHipError) as ei:
        fn()
    return ei.value.code


def _loads(key, nl, c=None):
    """nl real load shapes, zero on the clamp, and their static solutions: the bits of c.solve at the rtol of the calls (c given: the device's own
    static solutions under option deterministic), else a direct solve."""
    fc = np.asarray(H.load(key, "complex"))
    f = np.array([fc.real, fc.imag][:nl])
    if c is not None:
        us = np.array([c.solve(fa, rtol=RTOL, maxit=MAXIT) for fa in f])
    else:
        us = np.array([np.asarray(H.direct_solve(key, 1.0, 0.0, fa)).real for fa in f])
    return f, us


def _grid(lam):
    w = np.sqrt(lam)
    return np.linspace(0.31 * w[0], 1.17 * w[min(len(w), 12) - 1], 24)


def _spectrum(om, nl):
    s = 1.0 / (1.0 + (om / om[-1]) ** 2)
    if nl == 1:
        return s
    S = np.zeros((len(om), 2, 2), dtype=np.complex128)
    S[:, 0, 0], S[:, 1, 1] = s, 0.5 * s
    S[:, 0, 1] = (0.3 + 0.4j * np.cos(om / om[-1])) * s
    S[:, 1, 0] = np.conj(S[:, 0, 1])
    return S


def _twin(lam, X, f, us, om, S, kw, corrected, dtype):
    """(variances [3, n], covariances [3, nb, nb], B [nb, n]) of the twin in the precision of dtype: g, the correction columns and the forms."""
    Xd, fd = np.asarray(X, dtype=dtype), np.asarray(f, dtype=dtype)
    g = Xd @ fd.T
    B = Xd
    if corrected:
        r = np.asarray(us, dtype=dtype) - (g / np.asarray(lam, dtype=dtype)[:, None]).T @ Xd
        B = np.vstack([Xd, r])
    cov = R.covariance_twin(lam, g, om, S, correction=corrected, dtype=dtype, **kw)
    v = np.array([np.einsum("ji,jk,ki->i", B, cq, B) for cq in cov])
    return v, cov, B


def _bars(lam, X, f, us, om, S, kw, corrected, truncation):
    """(long-double variances [3, n], the bar on each [3])."""
    v_ld, cov, B = _twin(lam, X, f, us, om, S, kw, corrected, np.longdouble)
    v_64, _, _ = _twin(lam, X, f, us, om, S, kw, corrected, np.float64)
    phi2 = float((np.asarray(B, dtype=np.float64) ** 2).sum(axis=0).max())
    bars = [10.0 * float(np.abs(v_64[q] - v_ld[q]).max()) + truncation[q] * phi2 for q in range(3)]
    return v_ld, np.array(bars)


def _damping(key, case):
    (aR, bR), eta = H.damping(key, case)
    return dict(aR=aR, bR=bR, eta=eta), dict(damping=(aR, bR), loss_factor=eta)


# ---------------------------------------------------------------- against the twin
@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_against_the_twin(key, case):
    """m in {4, 12, 24} x correction on / off x one load and two with a complex cross term: sigma_u, sigma_v, sigma_a fields against the twin."""
    kw, args = _damping(key, case)
    c = _context(key, options=(("deterministic", 1),))
    worst = 0.0
    for m in (4, 12, 24):
        lam, X = MU.clamped_basis(key)
        lam, X = lam[:m], X[:m]
        c.set_modal_basis(lam, X, density=H.DENSITY)
        om = _grid(lam)
        for nl in (1, 2):
            f, us = _loads(key, nl, c)
            S = _spectrum(om, nl)
            for corrected in (False, True):
                r = c.modal_random(om, S, f, static_correction=corrected, velocity=True, acceleration=True, rtol=RTOL, maxit=MAXIT, **args)
                info = r["info"]
                v_ld, bars = _bars(lam, X, f, us, om, S, kw, corrected, info["truncation"])
                dev = np.array([r["sigma_u"], r["sigma_v"], r["sigma_a"]]) ** 2
                err = np.abs((dev - v_ld).astype(np.float64)).max(axis=1)
                worst = max(worst, float((err / bars).max()))
                print("%s %s m %d loads %d corrected %d: ranks %s passes %s truncation %s, error %s, bar %s" %
                      (_name(key), case, m, nl, corrected, info["ranks"], info["passes"], info["truncation"], err, bars))
                assert np.all(err <= bars)
                assert info["nb"] == m + (nl if corrected else 0) and info["staticSolves"] == (nl if corrected else 0)
                assert all(0 < rk <= min(info["nb"], 2 * nl * len(om)) for rk in info["ranks"])
                assert np.all(np.array([r["sigma_u"], r["sigma_v"], r["sigma_a"]])[:, U.clamp_vars(key)] == 0.0)
                assert r["cov"].shape == (3, info["nb"], info["nb"])
    print("%s %s: worst error / (10 x twin defect + truncation term) %.3e" % (_name(key), case, worst))
    c.close()


# ---------------------------------------------------------------- against the library's own sweep
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_against_the_sweep(key):
    """sigma_u^2 against sum_k w_k S_k |u^_i(w_k)|^2 from Context.modal_harmonic fields of the unit load (Rayleigh damping, with the correction: both
    calls make the same static solve). Bar: the twin bar of this file plus the sweep's own, modal_util.response_bound per frequency (a 2-norm bound,
    so it bounds every entry), carried through the square: sum_k w_k S_k (2 |u^_ref| b_k + b_k^2)."""
    kw, args = _damping(key, "rayleigh")
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:12], X[:12]
    om = _grid(lam)
    S = _spectrum(om, 1)
    n_free = len(H.free_of(key))
    c = _context(key, options=(("deterministic", 1),))
    f, us = _loads(key, 1, c)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = c.modal_random(om, S, f, rtol=RTOL, maxit=MAXIT, **args)
    sw = c.modal_harmonic(om, f[0], rtol=RTOL, maxit=MAXIT, **args)
    c.close()
    wq = R.trapezoid_weights(om)
    summed = ((wq * S)[:, None] * np.abs(sw["u"]) ** 2).sum(axis=0)
    _, bars = _bars(lam, X, f, us, om, S, kw, True, r["info"]["truncation"])
    rb = MU.response_bound(lam, X, f[0], om, u_s=us[0], n_free=n_free, **kw)
    uref, _ = MU.modal_response(lam, X, f[0], om, u_s=us[0], **kw)
    extra = ((wq * S)[:, None] * (2.0 * np.abs(uref) * rb[:, None] + (rb ** 2)[:, None])).sum(axis=0).max()
    err = np.abs(r["sigma_u"] ** 2 - summed).max()
    print("%s: sigma_u^2 against the summed sweep %.3e (bar %.3e + %.3e), largest variance %.3e" % (_name(key), err, bars[0], extra, summed.max()))
    assert err <= bars[0] + extra


# ---------------------------------------------------------------- fields and probes
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_probes_are_the_field_entries(key):
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:24], X[:24]
    free = H.free_of(key)
    pv = np.array([free[0], free[len(free) // 2], free[-1], free[0], U.clamp_vars(key)[0]], dtype=np.int64)
    kw, args = _damping(key, "structural")
    f, us = _loads(key, 2)
    om = _grid(lam)
    S = _spectrum(om, 2)
    c = _context(key, options=(("deterministic", 1),))
    c.set_modal_basis(lam, X, density=H.DENSITY)
    for corrected in (False, True):
        r = c.modal_random(om, S, f, static_correction=corrected, velocity=True, acceleration=True, probes=pv, probe_psd=True, rtol=RTOL, maxit=MAXIT, **args)
        p = r["probes"]
        for name in ("sigma_u", "sigma_v", "sigma_a"):
            assert np.array_equal(p[name], r[name][pv]), name
        assert np.array_equal(p["nu0"][:4], p["sigma_v"][:4] / (6.283185307179586 * p["sigma_u"][:4])) and p["nu0"][4] == 0.0
        # the response spectra of the probes against the twin's H_p S H_p^H, and their quadrature against the variance
        _, _, B = _twin(lam, X, f, us, om, S, kw, corrected, np.float64)
        g = X @ f.T
        ref = np.zeros((len(pv), len(om)))
        for k, w in enumerate(om):
            hp = B[:, pv].T @ R.transfer(lam, g, w, correction=corrected, **kw)
            ref[:, k] = np.einsum("pa,ab,pb->p", hp, np.asarray(S[k]), np.conj(hp)).real
        scale = np.abs(ref).max(axis=1, keepdims=True)
        tol = 1e-9 if corrected else 1e-12        # (the corrected rows carry the static solve at rtol 1e-12)
        assert p["psd"].shape == ref.shape and np.all(np.abs(p["psd"] - ref) <= tol * scale)
        quad = p["psd"] @ R.trapezoid_weights(om)
        assert np.all(np.abs(quad - p["sigma_u"] ** 2) <= 1e-10 * quad.max() + r["info"]["truncation"][0] * (B ** 2).sum(axis=0).max())
        # without fields nothing field-sized is returned, and the probes keep their bits; flags off: no sigma_v / sigma_a fields
        q = c.modal_random(om, S, f, static_correction=corrected, probes=pv, fields=False, rtol=RTOL, maxit=MAXIT, **args)
        assert q["sigma_u"] is None and np.array_equal(q["probes"]["sigma_u"], p["sigma_u"]) and np.array_equal(q["probes"]["nu0"], p["nu0"])
        assert q["probes"]["sigma_a"] is None and q["info"]["ranks"][2] == 0
        q = c.modal_random(om, S, f, static_correction=corrected, rtol=RTOL, maxit=MAXIT, **args)
        assert np.array_equal(q["sigma_u"], r["sigma_u"]) and q["sigma_v"] is None and q["sigma_a"] is None
    c.close()


def test_zero_crossings_of_one_mode():
    """A basis of one mode excited at a single frequency w0 = sqrt(lambda) (weight 1): sigma_v = w0 sigma_u, so nu0+ = sqrt(lambda) / 2 pi up to the
    roundings of two square roots, a product and a quotient. White noise on a resonance_grid over [0, 60 w0]: the same value to the quadrature
    error of the grid (1e-3)."""
    key = (3, 1)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:1], X[:1]
    f, _ = _loads(key, 1)
    w0 = float(np.sqrt(lam[0]))
    pv = H.free_of(key)[[0, -1]]
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = c.modal_random([w0], [2.0], f, weights=[1.0], modal_damping=0.02, static_correction=False, probes=pv, fields=False)
    assert np.all(np.abs(r["probes"]["nu0"] / (w0 / (2.0 * np.pi)) - 1.0) <= 8 * EPS)
    om = M.resonance_grid(lam, 0.02, (0.0, 60.0 * w0), per_halfpower=16)
    r = c.modal_random(om, np.ones(om.size), f, modal_damping=0.02, static_correction=False, probes=pv, fields=False)
    c.close()
    print("one mode, white noise, %d grid points: nu0 / (sqrt(lambda) / 2 pi) - 1 = %s" % (om.size, r["probes"]["nu0"] / (w0 / (2.0 * np.pi)) - 1.0))
    assert np.all(np.abs(r["probes"]["nu0"] / (w0 / (2.0 * np.pi)) - 1.0) <= 1e-3)


# ---------------------------------------------------------------- modal_quadratic, response spectra
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_modal_quadratic(key):
    """A diagonal C gives sqrt(sum_j c_j phi_ij^2) within the bound of the sum of squares with F = diag(sqrt(c)) (the roots of c are
    correctly rounded on either side); SRSS and CQC with a_j = Gamma_j Sd_j against a numpy double loop over the modes, within 1e-12 of the largest entry plus the truncation term;
    Gamma against X (rho M) r_d within the bound of the Gram sums; three matrices in one call, probes bit for bit the field entries."""
    m = 12
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:m], X[:m]
    free = H.free_of(key)
    pv = np.array([free[1], free[-2], U.clamp_vars(key)[-1]], dtype=np.int64)
    rM = H.DENSITY * U.pencil(key)[1]
    dim = U.fem_mesh(key).N
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    cd = np.random.default_rng(4).uniform(0.1, 2.0, m)
    cd[3] = 0.0
    rd = np.zeros(X.shape[1])
    rd[1::dim] = 1.0
    gamma = c.modal_coordinates(rd)
    Mr = rM @ rd
    assert np.all(np.abs(gamma - X @ Mr) <= MU.gram_bound(X, Mr[None, :], X.shape[1])[:, 0])
    zeta = np.linspace(0.02, 0.07, m)
    a = gamma * (1.0 / lam)                                   # Sd = 1 / w^2: a flat acceleration spectrum
    rho = M.cqc_matrix(lam, zeta)
    mats = np.array([np.diag(cd), np.outer(a, a) * np.eye(m), np.outer(a, a) * rho])
    r = c.modal_quadratic(mats, probes=pv)
    c.close()
    assert r["fields"].shape == (3, X.shape[1]) and np.array_equal(r["probes"], r["fields"][:, pv])
    assert r["info"]["ranks"][0] == m - 1 and r["info"]["passes"] == [1, 1, 1]
    Fd = np.diag(np.sqrt(cd))
    _, _, root_ref, root_bound = R.sumsq_prefixes(X, Fd, [m])[m]
    err = np.abs((r["fields"][0] - root_ref).astype(np.float64))
    assert np.all(err <= root_bound)
    for which, rr in ((1, np.eye(m)), (2, rho)):
        v = np.zeros(X.shape[1])
        for j in range(m):
            for k in range(m):
                v += rr[j, k] * a[j] * a[k] * X[j] * X[k]
        ref = np.sqrt(np.maximum(v, 0.0))
        bar = 1e-12 * ref.max() + np.sqrt(r["info"]["truncation"][which] * (X ** 2).sum(axis=0).max())
        print("%s %s: peak field against the double loop %.3e (bar %.3e, largest %.3e)" % (_name(key), "srss" if which == 1 else "cqc", np.abs(r["fields"][which] - ref).max(), bar, ref.max()))
        assert np.all(np.abs(r["fields"][which] ** 2 - v) <= 1e-12 * v.max() + r["info"]["truncation"][which] * (X ** 2).sum(axis=0).max())


def test_simulator_entries():
    """Simulator.responseSpectrum (SRSS and CQC, Sd a callable) against modal_quadratic's numpy reference on the caller's modes, its participation
    factors against modalEffectiveMass; Simulator.randomResponse against Context.modal_random bit for bit."""
    key = (3, 2)
    V, T, deg, _ = U.mesh_arrays(key)
    lam, X = MU.clamped_basis(key)
    m = 10
    lam, X = lam[:m], X[:m]
    dim = 3
    sim = M.Simulator(T, V, deg)
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    nodes = np.unique(U.clamp_vars(key) // dim)
    sim.applyDirichletNodes(nodes, np.zeros((len(nodes), dim)))
    probe_node = int(np.setdiff1d(np.arange(sim.numNodes()), nodes)[-1])
    sd = lambda w, z: 0.3 / (w * w) * (1.0 + z)
    zeta = 0.05
    for rule in ("srss", "cqc"):
        out = sim.responseSpectrum(2, sd, modal_damping=zeta, rule=rule, modes=(lam, X), density=H.DENSITY, probes=[[probe_node, 2]])
        si = sim.spectrum_info
        eff = H.DENSITY ** 2 * sim.modalEffectiveMass(X)[:, 2]
        assert np.all(np.abs(si["effective_mass"] - eff) <= 1e-10 * eff.max()) and 0.0 < si["mass_fraction"] <= 1.0 + 1e-12
        a = si["gamma"] * sd(np.sqrt(lam), zeta)
        rr = np.eye(m) if rule == "srss" else M.cqc_matrix(lam, np.full(m, zeta))
        v = np.einsum("ji,jk,ki->i", X * a[:, None], rr, X * a[:, None])
        R_ = out["R"].reshape(-1)
        assert np.all(np.abs(R_ ** 2 - v) <= 1e-12 * v.max() + si["info"]["truncation"][0] * (X ** 2).sum(axis=0).max())
        assert out["probes"][0] == R_[probe_node * dim + 2]
    f, _ = _loads(key, 1)
    om = _grid(lam)
    S = _spectrum(om, 1)
    out = sim.randomResponse(om, S, load=f[0].reshape(-1, dim), modal_damping=0.03, velocity=True, static_correction=False)
    ref = sim.ctx.modal_random(om, S, f, modal_damping=0.03, velocity=True, static_correction=False)
    assert np.array_equal(out["sigma_u"].reshape(-1), ref["sigma_u"]) and np.array_equal(out["sigma_v"].reshape(-1), ref["sigma_v"]) and out["sigma_a"] is None
    assert sim.random_info["staticSolves"] == 0 and sim.random_info["ranks"][0] > 0
    out = sim.randomResponse(om, S, load=f[0].reshape(-1, dim), modal_damping=0.03, rtol=RTOL, maxit=MAXIT)
    assert sim.random_info["staticSolves"] == 1 and out["sigma_u"].shape == (sim.numNodes(), dim)


# ---------------------------------------------------------------- refusals, states, neighbours
def test_refusals_and_states():
    key = (3, 1)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:8], X[:8]
    f3 = np.array([np.asarray(H.load(key)) * s for s in (1.0, 0.5, 0.25)])
    om = _grid(lam)
    S1 = _spectrum(om, 1)
    c = _context(key)
    run = lambda **kw: c.modal_random(om, S1, f3[:1], **{**dict(static_correction=False, modal_damping=0.02), **kw})
    assert _code(run) == _lib.ERR_STATE and _code(lambda: c.modal_quadratic(np.eye(8))) == _lib.ERR_STATE          # no basis
    c.set_modal_basis(lam, X, density=H.DENSITY)
    first = run()
    c.fix_variables([int(H.free_of(key)[-1])])
    assert _code(run) == _lib.ERR_STATE and _code(lambda: c.modal_quadratic(np.eye(8))) == _lib.ERR_STATE          # a stale basis
    c.clear_fixed()
    c.fix_variables(U.clamp_vars(key))
    assert np.array_equal(run()["sigma_u"], first["sigma_u"])
    c.set_density(np.full(c.n_elem, 2.0))
    assert _code(run) == _lib.ERR_STATE
    c.set_density(None)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    S3 = np.eye(3)[None] * S1[:, None, None]
    assert _code(lambda: c.modal_random(om, S3, f3, static_correction=True)) == _lib.ERR_UNSUPPORTED                 # three loads with the correction
    assert c.modal_random(om, S3, f3, static_correction=False, fields=False)["info"]["nb"] == 8
    for bad in (dict(rtol=2.0), dict(maxit=0), dict(damping=(-1.0, 0.0)), dict(loss_factor=-0.1), dict(modal_damping=-0.01), dict(probes=[c.bs * c.n_dof]),
                dict(tol=np.nan)):
        assert _code(lambda: run(**bad)) == _lib.ERR_INVALID, bad
    assert _code(lambda: c.modal_random(om[::-1].copy(), S1, f3[:1], static_correction=False)) == _lib.ERR_INVALID
    assert _code(lambda: c.modal_random(om, -S1, f3[:1], static_correction=False, modal_damping=0.02)) == _lib.ERR_INVALID          # a negative spectrum
    lam4 = lam.copy()
    lam4[2] = 4.0
    c.set_modal_basis(lam4, X, density=H.DENSITY)
    assert _code(lambda: c.modal_random([1.5, 2.0, 2.5], S1[:3], f3[:1], static_correction=False)) == _lib.ERR_INVALID               # undamped on an eigenfrequency: d_j = 0
    c.set_modal_basis(lam, X, density=H.DENSITY)
    fn = f3[:1].copy()
    fn[0, 5] = np.nan
    assert _code(lambda: c.modal_random(om, S1, fn, static_correction=False, modal_damping=0.02)) == _lib.ERR_INVALID
    assert _code(lambda: c.modal_random(om, S1, f3[:1], static_correction=True, modal_damping=0.02, rtol=1e-12, maxit=1)) == _lib.ERR_NOT_CONVERGED
    bad = np.eye(8)
    bad[2, 2] = -1.0
    assert _code(lambda: c.modal_quadratic(bad)) == _lib.ERR_INVALID                                                 # not positive semi-definite
    assert _code(lambda: c.modal_quadratic(np.full((8, 8), np.nan))) == _lib.ERR_INVALID
    assert c.lib.mfh_modal_quadratic(c.h, 5, _lib.ptr(np.zeros((5, 8, 8))), -1.0, None, 0, None, None, None) == _lib.ERR_INVALID
    z = c.modal_quadratic(np.zeros((8, 8)), probes=[3])                                                              # the zero matrix: rank 0, zeros
    assert z["info"]["ranks"] == [0] and not z["fields"].any() and not z["probes"].any()
    assert np.array_equal(run()["sigma_u"], first["sigma_u"])                                                        # the refused calls left the basis in place
    c.close()
    cf = _context(key, clamped=False)                                                                                # a free body: no correction, no omega = 0
    lamf = np.concatenate([np.zeros(1), lam[:3]])
    cf.set_modal_basis(lamf, X[:4], density=H.DENSITY)
    assert _code(lambda: cf.modal_random(om, S1, f3[:1], static_correction=True, modal_damping=0.02)) == _lib.ERR_UNSUPPORTED
    assert _code(lambda: cf.modal_random(np.concatenate([[0.0], om]), np.concatenate([[1.0], S1]), f3[:1], static_correction=False, modal_damping=0.02)) == _lib.ERR_INVALID
    cf.close()


def test_neighbours_keep_their_bits():
    """modal_harmonic (with the correction: it rewrites the two reserved columns) and modal_transient return the same bits before and after the new
    calls, which use those columns too."""
    key = (3, 2)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:12], X[:12]
    kw, args = _damping(key, "rayleigh")
    f, _ = _loads(key, 2)
    fc = f[0] + 1j * f[1]
    om = _grid(lam)
    c = _context(key, options=(("deterministic", 1),))
    c.set_modal_basis(lam, X, density=H.DENSITY)

    def snapshot():
        h = c.modal_harmonic(om[:5], fc, rtol=RTOL, maxit=MAXIT, **args)
        t = c.modal_transient(0.05 / np.sqrt(lam[0]), 40, f[0], amplitude=np.sin(np.arange(41) * 0.3), damping=args["damping"], rtol=RTOL, maxit=MAXIT,
                              snapshot_stride=10, probes=[int(H.free_of(key)[-1])])
        return [h["u"], h["modal_coords"], t["q"], t["qdot"], t["snapshots"], t["probes"]]
    before = snapshot()
    r1 = c.modal_random(om, _spectrum(om, 2), f, velocity=True, rtol=RTOL, maxit=MAXIT, **args)
    c.modal_quadratic(np.eye(12))
    after = snapshot()
    r2 = c.modal_random(om, _spectrum(om, 2), f, velocity=True, rtol=RTOL, maxit=MAXIT, **args)
    c.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(r1["sigma_u"], r2["sigma_u"]) and np.array_equal(r1["sigma_v"], r2["sigma_v"]) and np.array_equal(r1["cov"], r2["cov"])


# ---------------------------------------------------------------- one larger case
def test_mid_mesh_end_to_end():
    """37 905 unknowns: modal_basis(30), 2 % modal damping, about 2 000 grid points from resonance_grid over [0.2 w_1, 1.1 w_30], with the static
    correction (per_halfpower 4 on a background of 400 intervals). The RMS field against the weighted sum of the modal_harmonic fields of the same
    grid, taken in groups of 100 frequencies. Both come from the same basis (adopted on the device from modes_many), g and static solve on the same
    context. The bar is a fixed figure, 1e-10 of the largest variance plus truncation max |phi_i|^2, because the bound used on the small meshes
    needs the long-double twin and response_bound at 2 000 frequencies x 37 905 unknowns (1.2 GB of complex long doubles). What it has to cover:
    sums of about 2 000 x 31 terms of one sign on either side, (2 000 + 31 + 3) eps = 4.5e-13 relative in the worst case, and the two fma chains
    per entry, (31 + 1) eps each, through the square; 1e-10 is 200 x that."""
    key = U.MID
    c = _context(key, options=(("deterministic", 1),))
    lam, X, info = c.modal_basis(30, density=H.DENSITY, batch=12, rtol=1e-6, maxit=3000)
    w = np.sqrt(lam)
    om = M.resonance_grid(lam, 0.02, (0.2 * w[0], 1.1 * w[29]), per_halfpower=4, background=400)
    f = H.load(key, "real")
    S = 1.0 / (1.0 + (om / w[0]) ** 2)
    pv = H.free_of(key)[[0, -1]]
    r = c.modal_random(om, S, f, modal_damping=0.02, rtol=1e-10, maxit=MAXIT, probes=pv)
    wq = R.trapezoid_weights(om)
    summed = np.zeros(f.size)
    for k0 in range(0, len(om), 100):
        u = c.modal_harmonic(om[k0:k0 + 100], f, modal_damping=0.02, rtol=1e-10, maxit=MAXIT)["u"]
        summed += ((wq * S)[k0:k0 + 100, None] * (u.real ** 2 + u.imag ** 2)).sum(axis=0)
    # |phi_i|^2 over the columns of the device's basis: the modes and the correction column r_s = u_s - sum_j phi_j g_j / lambda_j
    us = c.solve(f, rtol=1e-10, maxit=MAXIT)
    c.close()
    rs = us - ((X @ f) / lam) @ X
    phi2 = float(((X ** 2).sum(axis=0) + rs ** 2).max())
    err = np.abs(r["sigma_u"] ** 2 - summed).max()
    print("mid mesh: %d grid points, rank %d in %d pass(es), truncation %.3e, covariance %.1f ms, factor %.1f ms, passes %.2f ms; sigma_u^2 against the summed "
          "sweep %.3e of %.3e" % (len(om), r["info"]["ranks"][0], r["info"]["passes"][0], r["info"]["truncation"][0], r["info"]["covarianceMs"],
                                  r["info"]["factorMs"], r["info"]["solveMs"], err, summed.max()))
    assert 1800 <= len(om) <= 2200 and r["info"]["staticSolves"] == 1 and r["info"]["nb"] == 31
    assert np.array_equal(r["probes"]["sigma_u"], r["sigma_u"][pv])
    assert err <= 1e-10 * summed.max() + r["info"]["truncation"][0] * phi2


# ---------------------------------------------------------------- the basis handover on the device
def _modal_results(c, key, lam):
    """One sweep with the correction and one random response on the basis in place."""
    kw, args = _damping(key, "rayleigh")
    f, _ = _loads(key, 2)
    om = _grid(lam)
    h = c.modal_harmonic(om[:6], f[0] + 1j * f[1], rtol=RTOL, maxit=MAXIT, **args)
    r = c.modal_random(om, _spectrum(om, 2), f, velocity=True, rtol=RTOL, maxit=MAXIT, probes=[int(H.free_of(key)[-1])], **args)
    q = c.modal_coordinates(f[0])
    return [h["u"], h["modal_coords"], r["sigma_u"], r["sigma_v"], r["cov"], r["probes"]["nu0"], q]


@pytest.mark.parametrize("nev,batch,take", [(6, 16, 6), (20, 8, 20), (20, 8, 11)], ids=["one-batch", "three-batches", "leading-11-of-20"])
@pytest.mark.parametrize("key", [(3, 1), (2, 2)], ids=_name)
def test_basis_handover_equals_the_round_trip(key, nev, batch, take):
    """set_modal_basis_from_modes after modes_many against set_modal_basis of what modes_many returned: the same orthoDefect and the same bits in a
    sweep, a random response and modal coordinates. One batch is the path that keeps the block of mfh_modes, several batches the deflation set with
    its sort; fewer modes than found take the leading ones."""
    c = _context(key, options=(("deterministic", 1),))
    lam, X, info = c.modes_many(nev, density=H.DENSITY, batch=batch, rtol=1e-6, maxit=3000)
    assert len(lam) == nev and np.all(np.diff(lam) >= 0.0)
    live = M.device_arena_stats(0)["live_bytes"]
    a_info = c.set_modal_basis(lam[:take], X[:take], density=H.DENSITY)
    a = _modal_results(c, key, lam[:take])
    c.set_modal_basis(None, None)
    assert M.device_arena_stats(0)["live_bytes"] >= live - 64          # (the kept set stays when the basis goes)
    b_info = c.set_modal_basis_from_modes(take, density=H.DENSITY)
    b = _modal_results(c, key, lam[:take])
    assert b_info["nModes"] == take and b_info["orthoDefect"] == a_info["orthoDefect"] and b_info["ld"] == a_info["ld"]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # Context.modal_basis goes through the device entry
    lam2, X2, info2 = c.modal_basis(nev, density=H.DENSITY, batch=batch, rtol=1e-6, maxit=3000)
    assert info2["modal_basis"]["nModes"] == nev and c.modal_basis_state() == (nev, True)
    b2 = _modal_results(c, key, lam2)
    c.set_modal_basis(lam2, X2, density=H.DENSITY)
    for x, y in zip(_modal_results(c, key, lam2), b2):
        assert np.array_equal(x, y)
    c.close()


def test_basis_handover_states():
    key = (3, 1)
    c = _context(key)
    adopt = lambda k=6: c.set_modal_basis_from_modes(k, density=H.DENSITY)
    assert _code(adopt) == _lib.ERR_STATE                                                       # no modes_many yet
    lam, X, _ = c.modes_many(6, density=H.DENSITY, rtol=1e-6, maxit=3000)
    assert adopt()["nModes"] == 6
    assert _code(lambda: adopt(7)) == _lib.ERR_INVALID and _code(lambda: adopt(0)) == _lib.ERR_INVALID
    assert _code(lambda: c.set_modal_basis_from_modes(6, density=0.0)) == _lib.ERR_INVALID
    assert c.modal_basis_state() == (6, True)                                                   # the refused calls left the basis in place
    c.fix_variables([int(H.free_of(key)[-1])])                                                  # another clamp: stale
    assert _code(adopt) == _lib.ERR_STATE
    c.clear_fixed()
    c.fix_variables(U.clamp_vars(key)[::-1].copy())                                             # the same set again: it serves
    assert adopt(3)["nModes"] == 3
    c.set_density(np.full(c.n_elem, 2.0))                                                       # another density field: stale, also after it is taken back
    assert _code(adopt) == _lib.ERR_STATE
    c.set_density(None)
    assert _code(adopt) == _lib.ERR_STATE
    c.modes_many(6, density=H.DENSITY, rtol=1e-6, maxit=3000)
    assert adopt()["nModes"] == 6
    V, T, deg, _ = U.mesh_arrays(key)
    c.mesh_update_vertices(np.ascontiguousarray(V) * 1.0)
    assert _code(adopt) == _lib.ERR_STATE and _code(lambda: c.modal_random(_grid(lam), _spectrum(_grid(lam), 1), _loads(key, 1)[0], static_correction=False)) == _lib.ERR_STATE
    c.close()
