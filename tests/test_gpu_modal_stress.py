"""RMS stress on the resident mode basis (mfh_modal_quadratic_stress, mfh_modal_random_stress; docs/design/04_24_modal_stress.md) against the numpy
twins of tests/modal_stress_util.py on the SAME modes (scipy's dense eigenpairs, tests/modal_util.py: all of them, up to the 256 a basis holds) on
the four small meshes, on the mid mesh with 20 modes, and against the library's own sweep.

The bar on a variance (the square of a returned value) is that of tests/test_modal_stress_reference.py:
    10 x max |float64 twin - long-double twin|  +  truncation x lambda_max x max_corner sum_j |s_j|^2       (lambda_max = 3 for von Mises, 1 per component)
The twin is the factor route on psd_factor_twin's factor (mfh_psd_factor's operations one for one); the reference of modal_quadratic_stress is the
double sum WITHOUT the factor (quadratic_stress_direct, long double). In runs with the static correction the twin takes the device's own covariance
and the static solutions the device used (Context.solve under option deterministic, as tests/test_gpu_modal_random.py does and for its reason).
Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import element_integrals_util as EU
import harmonic_util as H
import modal_random_util as R
import modal_stress_util as S
import modal_util as MU
import modes_util as U
from oracle import meshfem_oracle as O
from modal_stress_util import bars, matrices

pytestmark = pytest.mark.gpu

EPS = U.EPS
RTOL = MU.RTOL_STATIC
MAXIT = 20000
MAX_MODES = 256


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


def _elem_set(key, c):
    V, T, deg, _ = U.mesh_arrays(key)
    m = U.fem_mesh(key)
    assert np.array_equal(c.elem_nodes(), m.elem_nodes)
    return S.elem_set(m.N, deg, m.elem_nodes, V, c.material_get(0))


def _code(fn):
    with pytest.raises(M.MeshFEMHipError) as ei:
        fn()
    return ei.value.code


def _loads(key, nl, c):
    fc = np.asarray(H.load(key, "complex"))
    f = np.array([fc.real, fc.imag][:nl])
    us = np.array([c.solve(fa, rtol=RTOL, maxit=MAXIT) for fa in f])
    return f, us


def _grid(lam):
    w = np.sqrt(lam)
    return np.linspace(0.31 * w[0], 1.17 * w[min(len(w), 12) - 1], 24)


def _spectrum(om, nl):
    s = 1.0 / (1.0 + (om / om[-1]) ** 2)
    if nl == 1:
        return s
    Sm = np.zeros((len(om), 2, 2), dtype=np.complex128)
    Sm[:, 0, 0], Sm[:, 1, 1] = s, 0.5 * s
    Sm[:, 0, 1] = (0.3 + 0.4j * np.cos(om / om[-1])) * s
    Sm[:, 1, 0] = np.conj(Sm[:, 0, 1])
    return Sm


def _check_peak(r, a=None):
    vm = r["von_mises"] if a is None else r["von_mises"][a]
    value, elem, corner = r["peak"] if a is None else r["peak"][a]
    flat = int(np.argmax(vm))
    assert (elem, corner) == (flat // vm.shape[1], flat % vm.shape[1]) and value == vm.reshape(-1)[flat]


# ---------------------------------------------------------------- modal_quadratic_stress against the double sum
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_quadratic_stress_against_the_double_sum(key):
    """Diagonal, SRSS, CQC and rank-deficient matrices over ALL clamped modes (the first 256 on the 3D P2 mesh), one at a time and the four at once."""
    c = _context(key)
    s = _elem_set(key, c)
    lam, X = MU.clamped_basis(key)
    m = min(len(lam), MAX_MODES)
    lam, X = lam[:m], X[:m]
    Xn = X.reshape(m, -1, s.N)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    mats = matrices(lam, m, np.random.default_rng(11))
    names = list(mats)
    all4 = c.modal_quadratic_stress(np.array([mats[k] for k in names]), components=True)
    worst = 0.0
    for a, name in enumerate(names):
        r = c.modal_quadratic_stress(mats[name], components=True)
        assert np.array_equal(r["von_mises"][0], all4["von_mises"][a]) and np.array_equal(r["components"][0], all4["components"][a])
        _check_peak(all4, a)
        info = all4["info"]
        F, piv, _ = R.psd_factor_twin(mats[name])
        assert info["ranks"][a] == F.shape[1] and info["passes"][a] == -(-F.shape[1] // 32)
        _, bar_v, bar_c = bars(s, Xn, F, info["truncation"][a])
        vd, cd = S.quadratic_stress_direct(s, Xn, mats[name], True, np.longdouble)
        ev = float(np.abs((r["von_mises"][0] ** 2 - vd).astype(np.float64)).max())
        ec = float(np.abs((r["components"][0] ** 2 - cd).astype(np.float64)).max())
        worst = max(worst, ev / bar_v, ec / bar_c)
        print("%s %s: m %d rank %d passes %d truncation %.3e; von Mises^2 error %.3e (bar %.3e, largest %.3e), components^2 error %.3e (bar %.3e)" %
              (_name(key), name, m, info["ranks"][a], info["passes"][a], info["truncation"][a], ev, bar_v, float(vd.max()), ec, bar_c))
        assert ev <= bar_v and ec <= bar_c
    print("%s: worst error / bar %.3f" % (_name(key), worst))
    only = c.modal_quadratic_stress(mats["cqc"], von_mises=False, components=True, strain=True)
    assert only["von_mises"] is None and only["components"].shape == all4["components"][:1].shape
    z = c.modal_quadratic_stress(np.zeros((m, m)), components=True)                      # rank 0: zeros
    assert z["info"]["ranks"] == [0] and not z["von_mises"].any() and not z["components"].any()
    c.close()


def test_quadratic_stress_on_the_mid_mesh():
    """2 016 quadratic tets, 20 modes from the device's own eigensolver, the CQC matrix."""
    key = U.MID
    c = _context(key, options=(("deterministic", 1),))
    s = _elem_set(key, c)
    lam, X, _ = c.modal_basis(20, density=H.DENSITY, batch=12, rtol=1e-6, maxit=3000)
    Xn = np.asarray(X).reshape(20, -1, 3)
    Cm = matrices(lam, 20, np.random.default_rng(3))["cqc"]
    r = c.modal_quadratic_stress(Cm, components=True)
    c.close()
    _check_peak(r, 0)
    F, _, _ = R.psd_factor_twin(Cm)
    _, bar_v, bar_c = bars(s, Xn, F, r["info"]["truncation"][0])
    vd, cd = S.quadratic_stress_direct(s, Xn, Cm, True, np.longdouble)
    ev = float(np.abs((r["von_mises"][0] ** 2 - vd).astype(np.float64)).max())
    ec = float(np.abs((r["components"][0] ** 2 - cd).astype(np.float64)).max())
    print("mid mesh: von Mises^2 error %.3e (bar %.3e, largest %.3e), components^2 error %.3e (bar %.3e), passes %.2f ms" %
          (ev, bar_v, float(vd.max()), ec, bar_c, r["info"]["solveMs"]))
    assert ev <= bar_v and ec <= bar_c


# ---------------------------------------------------------------- modal_random_stress against the twin
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_random_stress_against_the_twin(key):
    """With and without the static correction, one load and two with a complex cross-spectrum: the twin is fed the device's own covariance and the
    columns the device used, B = [Phi | r_a], r_a = u_a - sum_j phi_j g_ja / lambda_j from the device's static solutions. 24 modes, not all of
    them (as tests/test_gpu_modal_random.py): with every clamped mode in the basis the correction columns r_a vanish and the corrected runs would
    test nothing; all modes are taken where no correction is involved, in test_quadratic_stress_against_the_double_sum."""
    c = _context(key, options=(("deterministic", 1),))
    s = _elem_set(key, c)
    lam, X = MU.clamped_basis(key)
    m = 24
    lam, X = lam[:m], X[:m]
    c.set_modal_basis(lam, X, density=H.DENSITY)
    om = _grid(lam)
    (aR, bR), _ = H.damping(key, "rayleigh")
    worst = 0.0
    for nl in (1, 2):
        f, us = _loads(key, nl, c)
        Sm = _spectrum(om, nl)
        for corrected in (False, True):
            r = c.modal_random_stress(om, Sm, f, static_correction=corrected, damping=(aR, bR), rtol=RTOL, maxit=MAXIT, components=True)
            info = r["info"]
            nb = m + (nl if corrected else 0)
            assert info["nb"] == nb and info["staticSolves"] == (nl if corrected else 0) and r["cov"].shape == (nb, nb)
            B = X
            if corrected:
                g = X @ f.T
                B = np.vstack([X, us - (g / lam[:, None]).T @ X])
            Bn = B.reshape(nb, -1, s.N)
            F, _, _ = R.psd_factor_twin(r["cov"])
            assert info["ranks"][0] == F.shape[1]
            (vld, cld), bar_v, bar_c = bars(s, Bn, F, info["truncation"][0])
            ev = float(np.abs((r["von_mises"] ** 2 - vld).astype(np.float64)).max())
            ec = float(np.abs((r["components"] ** 2 - cld).astype(np.float64)).max())
            worst = max(worst, ev / bar_v, ec / bar_c)
            print("%s loads %d corrected %d: rank %d truncation %.3e; von Mises^2 error %.3e (bar %.3e, largest %.3e), components^2 error %.3e (bar %.3e)" %
                  (_name(key), nl, corrected, info["ranks"][0], info["truncation"][0], ev, bar_v, float(vld.max()), ec, bar_c))
            assert ev <= bar_v and ec <= bar_c
            _check_peak(r)
    print("%s: worst error / bar %.3f" % (_name(key), worst))
    c.close()


# ---------------------------------------------------------------- against the library's own sweep
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_against_the_sweep(key):
    """Independent of the whole modal-variance path: sum_k w_k S_k |sigma(u^(w_k))|^2 from Context.modal_harmonic fields passed through
    element_integrals_util.strain_field (real and imaginary parts: s^H A s = Re^T A Re + Im^T A Im), white noise, one load, a short grid, with the
    correction. Bar: the relative agreement (largest difference over the largest variance) that the displacement variance of modal_random reaches
    against the same sweep on this mesh -- the comparison of tests/test_gpu_modal_random.py::test_against_the_sweep -- times 10, plus the
    truncation term. Both are printed. 12 modes with the correction, for the reason given in test_random_stress_against_the_twin."""
    c = _context(key, options=(("deterministic", 1),))
    s = _elem_set(key, c)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:12], X[:12]
    om = _grid(lam)[:10]
    Sw = np.ones(len(om))
    (aR, bR), _ = H.damping(key, "rayleigh")
    f, us = _loads(key, 1, c)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    kw = dict(damping=(aR, bR), rtol=RTOL, maxit=MAXIT)
    r = c.modal_random_stress(om, Sw, f, components=True, **kw)
    ru = c.modal_random(om, Sw, f, **kw)
    sw = c.modal_harmonic(om, f[0], **kw)
    c.close()
    wq = R.trapezoid_weights(om)
    u = sw["u"].reshape(len(om), -1, s.N)
    summed_u = (wq[:, None] * np.abs(sw["u"]) ** 2).sum(axis=0)
    rel_u = float(np.abs(ru["sigma_u"] ** 2 - summed_u).max() / summed_u.max())
    vm2 = np.zeros(r["von_mises"].shape)
    comp2 = np.zeros(r["components"].shape)
    for k in range(len(om)):
        for part in (u[k].real, u[k].imag):
            sg = EU.strain_field(s, part, stress=True)
            vm2 += wq[k] * S.v2(sg)
            comp2 += wq[k] * sg * sg
    B = np.vstack([X, us - ((X @ f.T) / lam[:, None]).T @ X]).reshape(13, -1, s.N)
    sj = np.array([EU.strain_field(s, b, stress=True) for b in B])
    trunc = r["info"]["truncation"][0]
    ev = float(np.abs(r["von_mises"] ** 2 - vm2).max())
    ec = float(np.abs(r["components"] ** 2 - comp2).max())
    bar_v = 10.0 * rel_u * vm2.max() + trunc * 3.0 * float((sj * sj).sum(axis=(0, -1)).max())
    bar_c = 10.0 * rel_u * comp2.max() + trunc * float((sj * sj).sum(axis=0).max())
    print("%s: displacement variance against the sweep %.3e relative; von Mises^2 %.3e relative (bar %.3e), components^2 %.3e relative (bar %.3e)" %
          (_name(key), rel_u, ev / vm2.max(), bar_v / vm2.max(), ec / comp2.max(), bar_c / comp2.max()))
    assert ev <= bar_v and ec <= bar_c


def test_one_mode_at_a_single_frequency():
    """A basis of one mode at one frequency (weight 1): the RMS von Mises field is |q| von_mises(phi_1), |q| = sqrt(C_00). The roundings between the
    two, u = 2^-53, vm the exact value at a corner:
      device     F = sqrt(C) (u, relative, on vm); the plane phi F, rounded per nodal value (u each): the corner stress is a sum over the nodes in
                 which these roundings do not cancel although the terms do, so they move the seminorm sqrt(v2) by at most u |q| Ns, Ns = sqrt(v2) of
                 the sums of the absolute terms of phi_1's corner stress (stress_sumsq_twin(sizes=True)); the new formula, 4 u vm.
      reference  the old formula on phi_1, u Vs + 5 u vm (tests/test_gpu_modal_stress_kernel.py; Vs <= Ns), times |q| (u), |q| itself a root (u).
    Together at most u |q| (Ns + Vs) + 12 u vm <= 14 u |q| Ns."""
    key = (3, 2)
    c = _context(key)
    s = _elem_set(key, c)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:1], X[:1]
    f = np.asarray(H.load(key, "real"))
    c.set_modal_basis(lam, X, density=H.DENSITY)
    w0 = float(np.sqrt(lam[0]))
    r = c.modal_random_stress([w0], [2.0], f, weights=[1.0], modal_damping=0.02, static_correction=False)
    q = float(np.sqrt(r["cov"][0, 0]))
    phi = X[0].reshape(-1, 3)
    ref = q * c.von_mises(phi)
    c.close()
    Ns = q * np.sqrt(S.stress_sumsq_twin(s, phi[None], True, np.float64, sizes=True)[0])
    ratio = float((np.abs(r["von_mises"] - ref) / (0.5 * EPS * Ns)).max())
    print("one mode: |rms - |q| von_mises(phi)| / (u |q| Ns) at most %.2f (bound 14); in units of u vm at most %.1f" %
          (ratio, float((np.abs(r["von_mises"] - ref) / (0.5 * EPS * ref)).max())))
    assert r["info"]["ranks"][0] == 1 and ratio <= 14.0


# ---------------------------------------------------------------- neighbours, refusals
def test_neighbours_keep_their_bits():
    key = (3, 2)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:12], X[:12]
    (aR, bR), _ = H.damping(key, "rayleigh")
    c = _context(key, options=(("deterministic", 1),))
    f, _ = _loads(key, 2, c)
    om = _grid(lam)
    c.set_modal_basis(lam, X, density=H.DENSITY)

    def snapshot():
        h = c.modal_harmonic(om[:5], f[0] + 1j * f[1], damping=(aR, bR), rtol=RTOL, maxit=MAXIT)
        rr = c.modal_random(om, _spectrum(om, 2), f, velocity=True, damping=(aR, bR), rtol=RTOL, maxit=MAXIT)
        return [h["u"], h["modal_coords"], rr["sigma_u"], rr["sigma_v"], rr["cov"]]
    before = snapshot()
    s1 = c.modal_random_stress(om, _spectrum(om, 2), f, damping=(aR, bR), rtol=RTOL, maxit=MAXIT, components=True)
    c.modal_quadratic_stress(np.eye(12))
    after = snapshot()
    s2 = c.modal_random_stress(om, _spectrum(om, 2), f, damping=(aR, bR), rtol=RTOL, maxit=MAXIT, components=True)
    c.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(s1["von_mises"], s2["von_mises"]) and np.array_equal(s1["components"], s2["components"]) and np.array_equal(s1["cov"], s2["cov"])


def _untouched(c):
    last = c.last_modal_stress
    return all(v is None or np.all(np.isnan(v)) for v in (last["von_mises"], last["components"]))


def test_refusals():
    """The status code of every refusal, and that the outputs (handed over filled with NaN) are untouched."""
    key = (3, 1)
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:8], X[:8]
    f3 = np.array([np.asarray(H.load(key)) * a for a in (1.0, 0.5, 0.25)])
    om = _grid(lam)
    S1 = _spectrum(om, 1)
    c = _context(key)
    run = lambda **kw: c.modal_random_stress(om, S1, f3[:1], **{**dict(static_correction=False, modal_damping=0.02, components=True), **kw})
    quad = lambda Cm=np.eye(8), **kw: c.modal_quadratic_stress(Cm, **{**dict(components=True), **kw})
    for fn in (run, quad):                                                                       # no basis
        assert _code(fn) == _lib.ERR_STATE and _untouched(c)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    first = run()
    c.set_density(np.full(c.n_elem, 2.0))                                                        # a stale basis
    for fn in (run, quad):
        assert _code(fn) == _lib.ERR_STATE and _untouched(c)
    c.set_density(None)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    for flag in (_lib.MODAL_RV_VELOCITY, _lib.MODAL_RV_ACCELERATION):                             # the velocity / acceleration flags
        assert _code(lambda: run(_rv_flags=flag)) == _lib.ERR_INVALID and _untouched(c)
    S3 = np.eye(3)[None] * S1[:, None, None]
    assert _code(lambda: c.modal_random_stress(om, S3, f3, static_correction=True, components=True)) == _lib.ERR_UNSUPPORTED and _untouched(c)
    bad = np.eye(8)
    bad[2, 2] = -1.0
    assert _code(lambda: quad(bad)) == _lib.ERR_INVALID and _untouched(c)                          # an indefinite C
    assert _code(lambda: quad(von_mises=False, components=False)) == _lib.ERR_INVALID              # nothing asked for
    assert _code(lambda: run(von_mises=False, components=False)) == _lib.ERR_INVALID
    info = _lib.ModalStressInfo()                                                                 # a requested output that is NULL
    assert c.lib.mfh_modal_quadratic_stress(c.h, 1, _lib.ptr(np.eye(8)), -1.0, _lib.MODAL_STRESS_VON_MISES, None, None, None) == _lib.ERR_INVALID
    vm = np.full((c.n_elem, 1), np.nan)
    assert c.lib.mfh_modal_quadratic_stress(c.h, 1, _lib.ptr(np.eye(8)), -1.0, 3, _lib.ptr(vm), None, ctypes.byref(info)) == _lib.ERR_INVALID
    assert np.all(np.isnan(vm))
    assert c.lib.mfh_modal_quadratic_stress(c.h, 5, _lib.ptr(np.zeros((5, 8, 8))), -1.0, 1, _lib.ptr(vm), None, None) == _lib.ERR_INVALID
    again = run()                                                                                # the refused calls left the basis in place
    assert np.array_equal(again["von_mises"], first["von_mises"]) and np.array_equal(again["components"], first["components"])
    c.close()
    V, T, deg, _ = U.mesh_arrays(key)                                                            # a scalar-operator context
    cs = M.Context(0)
    cs.mesh_build(T, V, deg)
    cs.set_operator(_lib.OP_LAPLACIAN)
    assert _code(lambda: cs.modal_quadratic_stress(np.eye(8))) == _lib.ERR_UNSUPPORTED and _untouched(cs)
    assert _code(lambda: cs.modal_random_stress(om, S1, np.zeros((1, cs.bs * cs.n_dof)), static_correction=False)) == _lib.ERR_UNSUPPORTED and _untouched(cs)
    cs.close()


# ---------------------------------------------------------------- the Simulator entries
def test_simulator_entries():
    """Simulator.randomStress and responseSpectrumStress against the Context calls, bit for bit."""
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
    sim.ctx.set_option("deterministic", 1)                  # (the participation factors go through the mass product: the same bits in both calls)
    sd = lambda w, z: 0.3 / (w * w) * (1.0 + z)
    zeta = 0.05
    for rule in ("srss", "cqc"):
        out = sim.responseSpectrumStress(2, sd, modal_damping=zeta, rule=rule, modes=(lam, X), density=H.DENSITY, components=True)
        si = sim.spectrum_stress_info
        ref_disp = sim.responseSpectrum(2, sd, modal_damping=zeta, rule=rule)
        assert np.array_equal(si["gamma"], sim.spectrum_info["gamma"]) and np.array_equal(si["a"], sim.spectrum_info["a"]) and ref_disp["R"] is not None
        rr = np.eye(m) if rule == "srss" else M.cqc_matrix(lam, np.full(m, zeta))
        ref = sim.ctx.modal_quadratic_stress(rr * np.outer(si["a"], si["a"]), components=True)
        assert np.array_equal(out["von_mises"], ref["von_mises"][0]) and np.array_equal(out["components"], ref["components"][0]) and out["peak"] == ref["peak"][0]
    f = np.asarray(H.load(key, "real"))
    om = _grid(lam)
    Sm = _spectrum(om, 1)
    out = sim.randomStress(om, Sm, load=f.reshape(-1, dim), modal_damping=0.03, static_correction=False, components=True)
    ref = sim.ctx.modal_random_stress(om, Sm, f, modal_damping=0.03, static_correction=False, components=True)
    assert np.array_equal(out["von_mises"], ref["von_mises"]) and np.array_equal(out["components"], ref["components"]) and out["peak"] == ref["peak"]
    assert sim.random_stress_info["staticSolves"] == 0 and sim.random_stress_info["ranks"][0] > 0
    out = sim.randomStress(om, Sm, load=f.reshape(-1, dim), modal_damping=0.03, rtol=RTOL, maxit=MAXIT)
    assert sim.random_stress_info["staticSolves"] == 1 and out["von_mises"].shape == (len(T), 4) and out["components"] is None
