"""mfh_newmark without a device: the refusals of invalid parameters (MFH_ERR_INVALID before any device work, on a host-only context) and the
reference recurrence of tests/dynamics_util.py against closed forms.
  dispersion   started from a mode shape at rest the trapezoidal rule gives u_n = phi cos(n theta), theta = 2 atan(omega dt / 2): the recurrence
               reproduces it to 1e-9 over 60 steps (measured: 1.4e-11 at worst on the four small meshes; the bar leaves the growth of the
               direct solves' rounding with cond(A) ~ 1e4 .. 1e5 some room)
  energy       undamped and unloaded it conserves 1/2 v.Mv + 1/2 u.Ku: 1e-11 relative over 100 steps (measured 6e-14)
  work         undamped under a constant load E - f.u is constant to the same bar"""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib, grid

import dynamics_util as D
import modes_util as U


def _host_context():
    V, T = grid.grid_tet_mesh(1, 1, 1)
    c = M.Context(-1)
    c.mesh_build(T, V, 1)
    return c


GOOD = dict(dt=0.1, n_steps=2, beta=0.25, gamma=0.5, density=1.0, damping=(0.0, 0.0))
BAD = [("dt zero", dict(dt=0.0)), ("dt negative", dict(dt=-1.0)), ("beta zero", dict(beta=0.0)), ("beta negative", dict(beta=-0.25)),
       ("gamma below a half", dict(gamma=0.49)), ("density zero", dict(density=0.0)), ("density negative", dict(density=-1.0)),
       ("negative mass damping", dict(damping=(-1e-3, 0.0))), ("negative stiffness damping", dict(damping=(0.0, -1e-3))),
       ("probe past the end", dict(probes=[10 ** 9])), ("negative probe", dict(probes=[-1]))]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_invalid_parameters_are_refused_before_device_work(what, change):
    c = _host_context()
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.newmark(**dict(GOOD, **change))
    assert ei.value.code == _lib.ERR_INVALID, what
    c.close()


def test_probe_range_is_the_number_of_variables():
    c = _host_context()
    n = c.bs * c.n_dof
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.newmark(probes=[n], **GOOD)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:           # in range: the call gets as far as asking for a device
        c.newmark(probes=[n - 1], **GOOD)
    assert ei.value.code == _lib.ERR_HIP
    c.close()


def test_energies_without_the_flag_are_refused():
    import ctypes as C
    c = _host_context()
    n = c.bs * c.n_dof
    u, v, a, en = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((3, 3))
    prm = _lib.NewmarkParams(0.1, 0.25, 0.5, 1.0, 0.0, 0.0, 1e-8, 2, 100, 0, 0)
    info = _lib.NewmarkInfo()
    st = c.lib.mfh_newmark(c.h, C.byref(prm), _lib.ptr(u), _lib.ptr(v), _lib.ptr(a), None, None, None, 0, None, None, _lib.ptr(en), C.byref(info))
    assert st == _lib.ERR_INVALID
    prm.flags = _lib.DYN_ENERGIES                             # the flag without the array
    st = c.lib.mfh_newmark(c.h, C.byref(prm), _lib.ptr(u), _lib.ptr(v), _lib.ptr(a), None, None, None, 0, None, None, None, C.byref(info))
    assert st == _lib.ERR_INVALID
    c.close()


def test_wrong_sizes_raise_value_error():
    c = _host_context()
    n = c.bs * c.n_dof
    for bad in (dict(u0=np.zeros(n + 1)), dict(f=np.zeros(n - 1)), dict(amplitude=np.ones(GOOD["n_steps"]))):
        with pytest.raises(ValueError):
            c.newmark(**dict(GOOD, **bad))
    c.close()


def test_valid_parameters_reach_the_device_check():
    c = _host_context()
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.newmark(**GOOD)
    assert ei.value.code == _lib.ERR_HIP
    c.close()


@pytest.mark.parametrize("key", U.SMALL, ids=lambda k: "%dD-P%d" % k)
def test_recurrence_reproduces_the_dispersion_of_the_trapezoidal_rule(key):
    for j in (0, 2):
        _, _, defect = D.dispersion_reference(key, j)
        print("%s mode %d: defect %.3e" % (key, j, defect))
        assert defect <= 1e-9


@pytest.mark.parametrize("key", U.SMALL, ids=lambda k: "%dD-P%d" % k)
def test_recurrence_conserves_energy_and_balances_work(key):
    K, Mm = U.pencil(key)
    free = D.free_of(key)
    i = D.case_inputs(key, "undamped")
    _, _, _, E = D.newmark_direct(K, Mm, free, i["dt"], 100, i["u0"], i["v0"], density=i["density"])
    tot = E[:, 0] + E[:, 1]
    print("%s: energy drift %.3e" % (key, np.abs(tot / tot[0] - 1).max()))
    assert np.abs(tot / tot[0] - 1).max() <= 1e-11
    _, _, _, E = D.newmark_direct(K, Mm, free, i["dt"], 100, i["u0"], i["v0"], f=i["f"], density=i["density"])
    bal = E[:, 0] + E[:, 1] - E[:, 2]
    print("%s: work balance drift %.3e" % (key, np.abs(bal - bal[0]).max() / (E[:, 0] + E[:, 1]).max()))
    assert np.abs(bal - bal[0]).max() <= 1e-11 * (E[:, 0] + E[:, 1]).max()
