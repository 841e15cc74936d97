"""k_modal_stress_sumsq through its hook (Context.debug_modal_stress_sumsq; docs/design/04_24_modal_stress.md) in all 12 instantiations
(dim 2 | 3) x (degree 1 | 2) x material (iso, ortho_field, general_field), with and without a periodic DoF map, and k_peak_of_array + k_peak_finish.

Meshes: the perturbed grids of tests/test_gpu_element_integrals.py (648 tets, 572 triangles: three workgroups, the last one partial). The twin
(tests/modal_stress_util.py) takes the tensors the context holds (Context.material_get), so that it starts from the kernel's own inputs.

Accuracy bar, per output entry: |device - long-double twin| / size <= 10 x max over the entries of |float64 twin - long-double twin| / size, with
size the entry's natural size (every term of the sums replaced by its absolute value: stress_sumsq_twin(sizes=True)). The worst ratio is printed."""
import numpy as np
import pytest

import element_integrals_util as EU
import meshfem_amd as M
import modal_stress_util as S
from meshfem_amd import grid
from oracle import meshfem_oracle as O

pytestmark = pytest.mark.gpu

EPS = S.EPS
U_ROUND = 0.5 * EPS                       # the unit roundoff
CASES = [(3, 2), (3, 1), (2, 2), (2, 1)]
MATERIALS = ("iso", "ortho_field", "general_field")
COUNTS = (1, 2, 31, 32, 33, 67)
GRID_CAP = 2048 * 256                     # elements one trip of the capped grid covers (MODAL_STRESS_GRID_CAP workgroups of 256 lanes)

_MESHES = {}


def _mesh(dim, deg):
    if (dim, deg) not in _MESHES:
        V, T = grid.grid_tet_mesh(3, 3, 3) if dim == 3 else grid.grid_tri_mesh(13, 11)
        V = EU.perturbed(V, 0.1)
        mesh = O.FEMMesh(T, V, deg)
        dof, n_dof, _ = O.periodic_dofs_for_nodes(mesh)
        _MESHES[dim, deg] = (V, np.asarray(T), mesh, dof, n_dof)
    return _MESHES[dim, deg]


def _setup(dim, deg, mode, periodic=False):
    """(context, element set with the context's tensors, node -> DoF table)"""
    V, T, mesh, dof, n_dof = _mesh(dim, deg)
    setter, _ = EU.material(mode, dim, len(T))
    c = M.Context(0)
    c.mesh_build(mesh.elems, mesh.verts, deg)
    setter(c)
    if periodic:
        assert c.apply_periodic_conditions() == n_dof and np.array_equal(c.get_dof_map()[0], dof)
    assert np.array_equal(c.elem_nodes(), mesh.elem_nodes)
    D = np.array([c.material_get(e) for e in range(c.n_elem)])
    s = S.elem_set(dim, deg, mesh.elem_nodes, V, D)
    return c, s, (dof if periodic else np.arange(c.n_node))


def _planes(c, count, seed):
    """count planes in VARIABLE numbering, of sizes spread over four decades"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(count, c.bs * c.n_dof)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(count, 1))


def _nodes(c, planes, dof):
    return np.asarray(planes).reshape(len(planes), c.n_dof, c.dim)[:, dof]


# ---------------------------------------------------------------- accuracy, every instantiation
FLAVOURS = [(dim, deg, mode, False) for dim, deg in CASES for mode in MATERIALS] + [(dim, deg, "general_field", True) for dim, deg in CASES]


@pytest.mark.parametrize("dim,deg,mode,periodic", FLAVOURS, ids=["%dD-P%d-%s%s" % (a, b, m, "-periodic" if p else "") for a, b, m, p in FLAVOURS])
def test_against_the_twin(dim, deg, mode, periodic):
    """Every instantiation on the plain mesh, and the node -> DoF table once per (dim, degree)."""
    c, s, dof = _setup(dim, deg, mode, periodic)
    assert c.n_elem > 512 and c.n_elem % 256 != 0 and (c.n_dof < c.n_node) == periodic
    planes = _planes(c, max(COUNTS), 100 * dim + 10 * deg + MATERIALS.index(mode))
    Un = _nodes(c, planes, dof)
    worst = 0.0
    for stress in ((True, False) if mode == "general_field" else (True,)):
        t64, tld = S.Twin(s, np.float64), S.Twin(s, np.longdouble)
        r64 = S.stress_sumsq_twin(t64, Un, stress, prefixes=COUNTS)
        rld = S.stress_sumsq_twin(tld, Un, stress, prefixes=COUNTS)
        size = S.stress_sumsq_twin(t64, Un, stress, prefixes=COUNTS, sizes=True)
        for count in COUNTS:
            vm, comp = c.debug_modal_stress_sumsq(planes[:count], strain=not stress)
            for name, dev, k in (("von Mises", vm, 0), ("components", comp, 1)):
                e, d = S.worst_ratio(dev, rld[count][k], r64[count][k], size[count][k])
                worst = max(worst, e / d)
                print("%dD P%d %s periodic=%d stress=%d planes %d %s: worst error / size %.3e, twin defect / size %.3e, ratio %.3f" %
                      (dim, deg, mode, periodic, stress, count, name, e, d, e / d))
                assert e <= 10.0 * d
    print("%dD P%d %s periodic=%d: worst error / twin defect %.3f (bar 10)" % (dim, deg, mode, periodic, worst))
    c.close()


# ---------------------------------------------------------------- grouping, roots, determinism
@pytest.mark.parametrize("dim,deg", CASES)
def test_grouping_and_determinism(dim, deg):
    """Planes per pass 1, 8, 16, 32 and the default give identical bits (the accumulators go through the output arrays between the passes); the root
    is np.sqrt of the stored sum bit for bit (IEEE square root on either side); two calls give identical bits."""
    c, s, dof = _setup(dim, deg, "ortho_field", periodic=(dim == 2))
    planes = _planes(c, 67, 5)
    ref = c.debug_modal_stress_sumsq(planes)
    for per in (1, 8, 16, 32):
        got = c.debug_modal_stress_sumsq(planes, planes_per_pass=per)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), per
        root = c.debug_modal_stress_sumsq(planes, planes_per_pass=per, sqrt=True)
        assert np.array_equal(root[0], np.sqrt(ref[0])) and np.array_equal(root[1], np.sqrt(ref[1])), per
    again = c.debug_modal_stress_sumsq(planes)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    only_vm = c.debug_modal_stress_sumsq(planes, components=False)
    assert only_vm[1] is None and np.array_equal(only_vm[0], ref[0])
    c.close()


# ---------------------------------------------------------------- one plane: the existing kernels
@pytest.mark.parametrize("mode", MATERIALS)
@pytest.mark.parametrize("dim,deg", CASES)
def test_one_plane_is_the_existing_kernels(dim, deg, mode):
    """With ONE plane and the root, the components are |k_strain_field's tensor| bit for bit: the same corner_tensor, and sqrt(x^2) = |x| exactly
    away from overflow and underflow of the square. The von Mises value is k_stress_measures' up to the difference of the two formulas on the same
    tensor x, vm the exact value, Vs = sqrt(v2 with every difference replaced by the sum of the sizes) >= vm, u = 2^-53:
      new  sqrt(fl(v2(x))): v2 is a sum of non-negative terms -- a difference (1 rounding), its square (1), three of them added (2), the shear squares
           (1) added (2) and tripled (1), the final sum (1): at most 6 u relative, halved by the root, plus the root's own u: |new - vm| <= 4 u vm.
      old  m sqrt(fl(v2(x / m))), m = max |x_c|: the divisions perturb every entry by u relatively, which moves the seminorm sqrt(v2) by at most u Vs
           (it is a 2-norm of linear forms of x; this is where a near-hydrostatic tensor loses digits relative to vm); then the same 3 u + u, and one more
           u for the product with m: |old - vm| <= u Vs + 5 u vm.
    So |new - old| <= (4 + 5) u vm + u Vs <= 10 u Vs, asserted with Vs from the kernel's own components."""
    c, s, dof = _setup(dim, deg, mode, periodic=False)
    planes = _planes(c, 1, 9)
    u_nodes = _nodes(c, planes, dof)[0]
    for stress in (True, False):
        vm, comp = c.debug_modal_stress_sumsq(planes, strain=not stress, sqrt=True)
        assert np.array_equal(comp, np.abs(c.strain_field(u_nodes, stress=stress)))
        old = c.von_mises(u_nodes, stress=stress)
        Vs = np.sqrt(S.v2_size(comp))
        ratio = float((np.abs(vm - old) / (U_ROUND * Vs)).max())
        print("%dD P%d %s stress=%d: |new - old| / (u Vs) at most %.2f (bound 10), in units of u vm at most %.2f" %
              (dim, deg, mode, stress, ratio, float((np.abs(vm - old) / (U_ROUND * old)).max())))
        assert ratio <= 10.0
    c.close()


# ---------------------------------------------------------------- zeros, translations, NaN
@pytest.mark.parametrize("dim,deg", CASES)
def test_zeros_translations_and_nan(dim, deg):
    """No planes -- rank 0: the hook fills the plane scratch with NaNs and launches the kernel as the drivers do for a zero matrix, with no plane and
    the accumulators starting from 0.0, so zeros come back only if the planes are not read -- and planes of zeros give exact zeros. A rigid translation has zero strain; what the device returns is the rounding of sums of at
    most 64 operations whose terms cancel: |root| <= 64 u sqrt(size). A NaN in one variable of one plane makes the von Mises sums of the elements
    that touch it NaN, every corner of them, and leaves every other element's bits alone."""
    c, s, dof = _setup(dim, deg, "iso", periodic=(dim == 3))
    n = c.bs * c.n_dof
    for planes in (np.zeros((0, n)), np.zeros((3, n)), np.zeros((40, n))):
        for root in (False, True):
            vm, comp = c.debug_modal_stress_sumsq(planes, sqrt=root)
            assert not vm.any() and not comp.any()
    shift = np.tile(np.array([0.7, -1.3, 2.9][:dim]), c.n_dof)[None]
    vm, comp = c.debug_modal_stress_sumsq(shift, sqrt=True)
    size_v, size_c = S.stress_sumsq_twin(s, _nodes(c, shift, dof), True, np.float64, sizes=True)
    print("%dD P%d translation: largest root %.3e of size %.3e" % (dim, deg, float(comp.max()), float(np.sqrt(size_c.max()))))
    assert np.all(comp <= 64 * U_ROUND * np.sqrt(size_c)) and np.all(vm <= 64 * U_ROUND * np.sqrt(size_v))
    planes = _planes(c, 35, 3)
    clean = c.debug_modal_stress_sumsq(planes)
    var = int(n // 2) + 1
    planes[33, var] = np.nan
    vm, comp = c.debug_modal_stress_sumsq(planes)
    touched = np.any(dof[s.en] == var // dim, axis=1)
    assert 0 < touched.sum() < c.n_elem
    assert np.all(np.isnan(vm[touched])) and np.array_equal(vm[~touched], clean[0][~touched]) and np.array_equal(comp[~touched], clean[1][~touched])
    assert np.all(np.isnan(comp[touched]).any(axis=(1, 2)))
    c.close()


# ---------------------------------------------------------------- more elements than one trip of the capped grid
def test_past_the_grid_cap():
    """2D P1, 540 800 triangles: more than the 2048 x 256 lanes of one trip, so the lanes of the first workgroups take a second element. Two planes,
    the bar of test_against_the_twin; the elements of the second trip are looked at on their own."""
    V, T = grid.grid_tri_mesh(520, 520)
    V = EU.perturbed(V, 0.1 / 520)
    c = M.Context(0)
    c.mesh_build(T, V, 1)
    c.material_isotropic(200.0, 0.35)
    assert c.n_elem > GRID_CAP
    s = S.elem_set(2, 1, c.elem_nodes(), V, c.material_get(0))
    planes = _planes(c, 2, 11)
    Un = planes.reshape(2, c.n_node, 2)
    vm, comp = c.debug_modal_stress_sumsq(planes)
    c.close()
    r64, rld = S.stress_sumsq_twin(s, Un, True, np.float64), S.stress_sumsq_twin(s, Un, True, np.longdouble)
    size = S.stress_sumsq_twin(s, Un, True, np.float64, sizes=True)
    for name, dev, k in (("von Mises", vm, 0), ("components", comp, 1)):
        e, d = S.worst_ratio(dev, rld[k], r64[k], size[k])
        e2, _ = S.worst_ratio(dev[GRID_CAP:], rld[k][GRID_CAP:], r64[k][GRID_CAP:], size[k][GRID_CAP:])
        print("past the cap, %s: worst error / size %.3e (second trip %.3e), twin defect / size %.3e" % (name, e, e2, d))
        assert e <= 10.0 * d and e2 <= 10.0 * d


# ---------------------------------------------------------------- the peak of an array
def _numpy_peak(v):
    nan = np.isnan(v)
    i = int(np.argmax(nan)) if nan.any() else int(np.argmax(v))
    return v[i], i


def test_peak_of_array():
    rng = np.random.default_rng(2)
    big = rng.normal(size=300001)                        # more than the 1024 x 256 lanes of one trip
    big[[17, 280000, 299999]] = 9.0                      # a tie, the last one in the second trip
    late = rng.normal(size=300001)
    late[290123] = 50.0
    with_nan = big.copy()
    with_nan[[270001, 299000]] = np.nan
    cases = [np.array([3.5]), np.array([np.nan]), np.array([1.0, 4.0, 4.0, -2.0]), np.array([-np.inf, -np.inf]), np.array([1.0, np.nan, 7.0, np.nan]),
             np.zeros(1000), big, late, with_nan, -np.abs(rng.normal(size=777))]
    c = M.Context(0)
    for v in cases:
        val, idx = c.debug_peak_of_array(v)
        rv, ri = _numpy_peak(v)
        assert idx == ri and (val == rv or (np.isnan(val) and np.isnan(rv))), (len(v), val, idx, rv, ri)
    c.close()
