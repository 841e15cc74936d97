"""Thin numpy-facing wrapper over the C ABI (one `Context` == one mfh_ctx)."""
import ctypes as C
import os

import numpy as np

from . import _lib as L
from ._lib import as_f64, as_i32, as_i64, ptr


def flat_len(dim):
    return dim * (dim + 1) // 2


def _probe_vars(probes):             # a `probes` argument as (the variables as int64 or None, how many)
    pv = None if probes is None else as_i64(np.asarray(probes).reshape(-1))
    return pv, 0 if pv is None else pv.size


def _modal_zeta(modal_damping, m):   # a `modal_damping` argument (a scalar or one ratio per mode) as m doubles, or None
    return None if modal_damping is None else as_f64(np.broadcast_to(np.asarray(modal_damping, dtype=np.float64), (m,)))


class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        st = self.lib.mfh_create(int(device), C.byref(h))
        if st != L.OK:
            raise L.MeshFEMHipError(st, "mfh_create(device=%d) failed with status %d: no usable HIP device "
                                        "(libmeshfem_hip has no CPU fallback)" % (device, st))
        self.h = h
        self.host_only = device == -1
        self.dim = self.deg = None
        self.op = L.OP_ELASTICITY
        self.op_degree = 0
        self.external = False
        # experiments: MFH_OPTIONS="name=value,name=value" presets mfh_set_option on every new context (A/B runs of the
        # measurement scripts without editing them); unset in normal use
        for kv in filter(None, os.environ.get("MFH_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            self.set_option(k.strip(), float(v))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mfh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != L.OK:
            raise L.MeshFEMHipError(st, self.lib.mfh_last_error(self.h).decode())

    # ---------------------------------------------------------------- mesh
    def mesh_build(self, elems, verts, deg):
        elems, verts = as_i32(elems), as_f64(verts)
        self.dim, self.deg = verts.shape[1], deg
        self._ck(self.lib.mfh_mesh_build(self.h, self.dim, deg, len(elems), len(verts), ptr(elems), ptr(verts)))
        self._sizes()

    def mesh_set(self, dim, deg, elem_nodes, node_pos, n_owned=None):
        """Explicit node table (any numbering); rows of K = the first n_owned nodes (halo nodes last)."""
        elem_nodes, node_pos = as_i32(elem_nodes), as_f64(node_pos)
        self.dim, self.deg = dim, deg
        n_node = len(node_pos)
        n_owned = n_node if n_owned is None else n_owned
        self._ck(self.lib.mfh_mesh_set(self.h, dim, deg, len(elem_nodes), n_node, n_owned, ptr(elem_nodes), ptr(node_pos)))
        self._sizes()

    def _sizes(self):
        v = [C.c_int64() for _ in range(5)]
        a, b = C.c_int32(), C.c_int32()
        self._ck(self.lib.mfh_mesh_sizes(self.h, *[C.byref(x) for x in v], C.byref(a), C.byref(b)))
        self.n_elem, self.n_node, self.n_vert, self.n_bdry_elem, self.n_bdry_node = [x.value for x in v]
        self.npe, self.npbe = a.value, b.value
        self.n_dof = self.n_node
        self.external = False
        self.op_degree = 0

    def elem_nodes(self):
        out = np.empty((self.n_elem, self.npe), dtype=np.int32)
        self._ck(self.lib.mfh_mesh_get_elem_nodes(self.h, ptr(out)))
        return out

    def node_positions(self):
        out = np.empty((self.n_node, self.dim))
        self._ck(self.lib.mfh_mesh_get_node_positions(self.h, ptr(out)))
        return out

    def boundary_elem_nodes(self):
        out = np.empty((self.n_bdry_elem, self.npbe), dtype=np.int32)
        self._ck(self.lib.mfh_mesh_get_boundary_elem_nodes(self.h, ptr(out)))
        return out

    def boundary_elem_parents(self):
        out = np.empty(self.n_bdry_elem, dtype=np.int32)
        self._ck(self.lib.mfh_mesh_get_boundary_elem_parents(self.h, ptr(out)))
        return out

    def boundary_elem_internal(self):
        """1 for boundary elements lying on the periodic cell boundary (BoundaryElementData::isInternal)"""
        out = np.empty(self.n_bdry_elem, dtype=np.uint8)
        self._ck(self.lib.mfh_mesh_get_boundary_elem_internal(self.h, ptr(out)))
        return out

    def boundary_nodes(self):
        out = np.empty(self.n_bdry_node, dtype=np.int32)
        self._ck(self.lib.mfh_mesh_get_boundary_nodes(self.h, ptr(out)))
        return out

    def boundary_elem_geometry(self):
        vol = np.empty(self.n_bdry_elem)
        nrm = np.empty((self.n_bdry_elem, self.dim))
        self._ck(self.lib.mfh_mesh_get_boundary_elem_geometry(self.h, ptr(vol), ptr(nrm)))
        return vol, nrm

    def elem_volumes(self):
        out = np.empty(self.n_elem)
        self._ck(self.lib.mfh_mesh_get_elem_volumes(self.h, ptr(out)))
        return out

    def mesh_update_vertices(self, verts):
        """New vertex positions on the same connectivity (Simulator::updateMeshNodePositions): keeps every setup phase."""
        v = as_f64(np.asarray(verts, dtype=np.float64)[:, :self.dim])
        if v.shape != (self.n_vert, self.dim):
            raise ValueError("expected %d x %d vertex positions" % (self.n_vert, self.dim))
        self._ck(self.lib.mfh_mesh_update_vertices(self.h, ptr(v)))

    # ---------------------------------------------------------------- materials
    def material_isotropic(self, E, nu):
        self._ck(self.lib.mfh_material_isotropic(self.h, float(E), float(nu)))

    def material_const(self, D):
        D = as_f64(D)
        assert D.shape == (flat_len(self.dim),) * 2
        self._ck(self.lib.mfh_material_const(self.h, ptr(D)))

    def material_iso_field(self, E, nu):
        E, nu = as_f64(E), as_f64(nu)
        assert len(E) == len(nu) == self.n_elem
        self._ck(self.lib.mfh_material_iso_field(self.h, ptr(E), ptr(nu)))

    def material_ortho_field(self, params):
        params = as_f64(params)
        assert params.shape == (self.n_elem, 9 if self.dim == 3 else 4)
        self._ck(self.lib.mfh_material_ortho_field(self.h, ptr(params)))

    def material_tensor_field(self, D):
        D = as_f64(D)
        assert D.shape == (self.n_elem,) + (flat_len(self.dim),) * 2
        self._ck(self.lib.mfh_material_tensor_field(self.h, ptr(D)))

    def material_get(self, e):
        out = np.empty((flat_len(self.dim),) * 2)
        self._ck(self.lib.mfh_material_get(self.h, int(e), ptr(out)))
        return out

    # ---------------------------------------------------------------- DoF map
    def dof_map(self, dof_for_node, n_dof):
        if dof_for_node is None:
            self._ck(self.lib.mfh_dof_map(self.h, None, 0))
            self.n_dof = self.n_node
        else:
            d = as_i32(dof_for_node)
            self._ck(self.lib.mfh_dof_map(self.h, ptr(d), int(n_dof)))
            self.n_dof = int(n_dof)

    def apply_periodic_conditions(self, eps=1e-7):
        n = C.c_int64()
        self._ck(self.lib.mfh_apply_periodic_conditions(self.h, float(eps), C.byref(n)))
        self.n_dof = n.value
        return n.value

    def dof_map_partitioned(self, dof_for_node, n_dof, n_owned_dof):
        """DoF map of a row-partitioned context (mfh_mesh_set): local DoFs owned-first, the rows of K are the first n_owned_dof."""
        dm = as_i32(dof_for_node)
        self._ck(self.lib.mfh_dof_map_partitioned(self.h, ptr(dm), int(n_dof), int(n_owned_dof)))
        self.n_dof = int(n_dof)

    def get_dof_map(self):
        out = np.empty(self.n_node, dtype=np.int32)
        n = C.c_int64()
        self._ck(self.lib.mfh_get_dof_map(self.h, ptr(out), C.byref(n)))
        return out, n.value

    # ---------------------------------------------------------------- assembly
    def symbolic(self, with_scatter=False):
        self._ck(self.lib.mfh_symbolic(self.h, int(with_scatter)))

    def symbolic_sizes(self):
        a, b = C.c_int64(), C.c_int64()
        c, d = C.c_int32(), C.c_int32()
        self._ck(self.lib.mfh_symbolic_sizes(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(n_chunk=a.value, n_contrib=b.value, chunk_slots=c.value, max_row_len=d.value)

    def matrix_info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.mfh_matrix_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def matrix_storage(self):
        """(upper_only, stored_blocks): option "matrix_storage". matrix_info / export_bsr describe K itself either way; the
        symbolic phase (symbolic_get) describes what is stored."""
        u, n = C.c_int32(), C.c_int64()
        self._ck(self.lib.mfh_matrix_storage(self.h, C.byref(u), C.byref(n)))
        return bool(u.value), n.value

    def symbolic_get(self, with_scatter=False):
        nr, nc, _ = self.matrix_info()
        nnzb = self.matrix_storage()[1]
        sz = self.symbolic_sizes()
        out = dict(rowPtr=np.empty(nr + 1, np.int32), colIdx=np.empty(nnzb, np.int32),
                   chunkRow=np.empty(sz["n_chunk"] + 1, np.int32), contribPtr=np.empty(sz["n_chunk"] + 1, np.int64),
                   contribCode=np.empty(sz["n_contrib"], np.uint32), contribSlot=np.empty(sz["n_contrib"], np.uint16))
        sc = np.empty(self.n_elem * self.npe * self.npe, np.int32) if with_scatter else None
        self._ck(self.lib.mfh_symbolic_get(self.h, ptr(out["rowPtr"]), ptr(out["colIdx"]), ptr(out["chunkRow"]),
                                           ptr(out["contribPtr"]), ptr(out["contribCode"]), ptr(out["contribSlot"]), ptr(sc)))
        if with_scatter:
            out["scatterSlot"] = sc
        out.update(sz)
        return out

    @property
    def bs(self):
        """Variables per DoF = block edge of K: dim for elasticity and the vector-valued mass operator, 1 for
        the scalar operators and for caller-supplied matrices."""
        return self.dim if (self.op in (L.OP_ELASTICITY, L.OP_MASS_VECTOR) and not self.external) else 1

    def matrix_set_upper_triplets(self, n, i, j, v):
        """SPSDSystem(K) for a caller-supplied SPD matrix (upper-triangle triplets, repeats summed)."""
        i, j = np.ascontiguousarray(i, dtype=np.uint64), np.ascontiguousarray(j, dtype=np.uint64)
        v = as_f64(v)
        assert len(i) == len(j) == len(v)
        self._ck(self.lib.mfh_matrix_set_upper_triplets(self.h, int(n), len(v), ptr(i), ptr(j), ptr(v)))
        self.external, self.op = True, L.OP_ELASTICITY
        self.n_dof = self.n_node = int(n)
        self.dim = 1

    def set_operator(self, op):
        """OP_ELASTICITY (default) | OP_LAPLACIAN | OP_MASS | OP_MASS_VECTOR: same mesh, pattern and kernels, 1x1
        blocks for the scalar operators (Laplacian.hh, MassMatrix.hh, Poisson.hh); OP_MASS_VECTOR is the mass matrix
        on interleaved displacement vectors (MassMatrix::construct_vector_valued), one stored value per block."""
        self._ck(self.lib.mfh_set_operator(self.h, int(op)))
        self.op = int(op)

    def set_operator_degree(self, degree):
        """0: the operators have the mesh's degree (default). 1: OP_LAPLACIAN / OP_MASS / OP_MASS_VECTOR on a quadratic
        mesh are the degree-1 operators on its vertices (Laplacian::construct<1>, MassMatrix::construct<1>); matrix_info,
        the exports, apply_K, fix_variables, solve and mass_lumped then work on n_vert rows. No effect on linear meshes."""
        self._ck(self.lib.mfh_set_operator_degree(self.h, int(degree)))
        if self.deg == 2:
            if int(degree) == 1 and self.op_degree != 1:
                self._n_dof_full = self.n_dof
                self.n_dof = self.n_vert
            elif int(degree) == 0 and self.op_degree == 1:
                self.n_dof = self._n_dof_full
            self.op_degree = int(degree)

    def mass_lumped(self):
        """Row sums of the full symmetric mass matrix of OP_MASS (n_dof values) or OP_MASS_VECTOR (every row sum
        repeated dim times), summed on the device over the stored values (mfh_mass_lumped)."""
        if not self._assembled_info():
            self.assemble()
        out = np.empty(self.bs * self.matrix_info()[0])              # rows of the degree view in force, as the library counts them
        self._ck(self.lib.mfh_mass_lumped(self.h, ptr(out), 0))
        return out

    def divergence(self, elem_vectors):
        """out[n] = sum over the elements e containing node n of v_e . int_e grad phi_n (the reference's
        differential_operators.divergence); linear meshes only."""
        v = as_f64(elem_vectors)
        if v.shape != (self.n_elem, self.dim):
            raise ValueError("expected one %d-vector per element" % self.dim)
        out = np.empty(self.n_node)
        self._ck(self.lib.mfh_divergence(self.h, ptr(v), ptr(out)))
        return out

    def precond_choice(self):
        """(kind, chosen automatically?, stretch of the mesh the choice looked at): mfh_precond_choice. With PRECOND_AUTO the choice is made now."""
        k, a, st = C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self.lib.mfh_precond_choice(self.h, C.byref(k), C.byref(a), C.byref(st)))
        return k.value, bool(a.value), st.value

    def matrix_free_info(self):
        a, mo, mb = C.c_int32(), C.c_int32(), C.c_int32()
        nb, ne, ni = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.mfh_matrix_free_info(self.h, C.byref(a), C.byref(mo), C.byref(nb), C.byref(ne), C.byref(ni), C.byref(mb)))
        return dict(active=bool(a.value), mode=mo.value, blocks=nb.value, block_rows=ne.value, interface_partials=ni.value,
                    max_block_rows=mb.value)

    def average_gradient(self, u_nodes):
        u = as_f64(u_nodes)
        out = np.empty((self.n_elem, self.dim))
        self._ck(self.lib.mfh_average_gradient(self.h, ptr(u), ptr(out)))
        return out

    def assemble(self, mode=L.ASSEMBLE_GATHER):
        self._ck(self.lib.mfh_assemble(self.h, int(mode)))

    def export_bsr(self):
        nr, nc, nnzb = self.matrix_info()
        rp, ci = np.empty(nr + 1, np.int32), np.empty(nnzb, np.int32)
        vals = np.empty((nnzb, self.bs, self.bs))
        self._ck(self.lib.mfh_export_bsr(self.h, ptr(rp), ptr(ci), ptr(vals)))
        return rp, ci, vals

    def export_scipy(self):
        import scipy.sparse as sp
        rp, ci, vals = self.export_bsr()
        nr, nc, _ = self.matrix_info()
        return sp.bsr_matrix((vals, ci, rp), shape=(nr * self.bs, nc * self.bs)).tocsr()

    def debug_device_node_tables(self):
        """(elem_nodes, node_pos) as the kernels see them (device copies; test hook)."""
        en, pos = np.empty((self.n_elem, self.npe), dtype=np.int32), np.empty((self.n_node, self.dim))
        self._ck(self.lib.mfh_debug_device_node_tables(self.h, ptr(en), ptr(pos)))
        return en, pos

    def debug_apply_operator(self, X, masked=False, flavour=0, Y=None):
        """(Y, dots) = the batched PCG's operator on the rows of X (test hook mfh_debug_apply_operator). Y: the incoming contents of
        the output (default NaN: every row must be written), returned unchanged by a closed gate (flavours 3, 4)."""
        X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        nr = X.shape[0]
        Y = np.full(X.shape, np.nan) if Y is None else np.array(np.broadcast_to(Y, X.shape), dtype=np.float64, order="C")
        dots = np.zeros(nr)
        self._ck(self.lib.mfh_debug_apply_operator(self.h, nr, int(bool(masked)), int(flavour), ptr(X), ptr(Y), ptr(dots)))
        return Y, dots

    def debug_apply_precond(self, R):
        """Z = M^-1 R on the rows of R with the preconditioner of the next solve (test hook mfh_debug_apply_precond)."""
        R = np.ascontiguousarray(np.atleast_2d(R), dtype=np.float64)
        Z = np.empty_like(R)
        self._ck(self.lib.mfh_debug_apply_precond(self.h, R.shape[0], ptr(R), ptr(Z)))
        return Z

    def export_upper_triplets(self):
        n = C.c_uint64(0)
        self._ck(self.lib.mfh_export_upper_triplets(self.h, None, None, None, C.byref(n)))
        i, j, v = np.empty(n.value, np.uint64), np.empty(n.value, np.uint64), np.empty(n.value)
        self._ck(self.lib.mfh_export_upper_triplets(self.h, ptr(i), ptr(j), ptr(v), C.byref(n)))   # n: entries written (zeros pruned)
        return i[:n.value], j[:n.value], v[:n.value]

    def element_stiffness(self, first=0, count=None):
        count = self.n_elem - first if count is None else count
        npe = self.dim + 1 if self.op_degree == 1 else self.npe       # the forced-degree-1 view has the corner nodes only
        ks = npe * (1 if self.op == L.OP_MASS_VECTOR else self.bs)    # (OP_MASS_VECTOR: the scalar element mass matrices it is assembled from)
        out = np.empty((count, ks, ks))
        self._ck(self.lib.mfh_element_stiffness(self.h, int(first), int(count), ptr(out)))
        return out

    # ---------------------------------------------------------------- solve
    def clear_fixed(self):
        self._ck(self.lib.mfh_clear_fixed(self.h))

    def fix_variables(self, vars_, vals=None):
        v = as_i64(vars_)
        x = None if vals is None else as_f64(vals)
        self._ck(self.lib.mfh_fix_variables(self.h, len(v), ptr(v), ptr(x)))

    def set_preconditioner(self, kind):
        self._ck(self.lib.mfh_set_preconditioner(self.h, int(kind)))

    def precond_info(self):
        a, m, t, note = C.c_int32(), C.c_int64(), C.c_double(), C.c_char_p()
        self._ck(self.lib.mfh_precond_info(self.h, C.byref(a), C.byref(m), C.byref(t), C.byref(note)))
        return dict(aggregates=a.value, coarse_dim=m.value, setup_ms=t.value, note=(note.value or b"").decode())

    def multigrid_info(self):
        a, b = C.c_int64(), C.c_int64()
        l0, l1, t = C.c_double(), C.c_double(), C.c_double()
        self._ck(self.lib.mfh_multigrid_info(self.h, C.byref(a), C.byref(b), C.byref(l0), C.byref(l1), C.byref(t)))
        return dict(fine_dof=a.value, coarse_dof=b.value, lambda_max_fine=l0.value, lambda_max_coarse=l1.value, setup_ms=t.value)

    def placement_info(self):
        """Kernel time (ms) of every candidate of the last placement trials (option placement_trials); [] when none ran."""
        out = (C.c_double * 16)()
        n = C.c_int32()
        self._ck(self.lib.mfh_placement_info(self.h, 16, out, C.byref(n)))
        return [float(out[k]) for k in range(min(16, n.value))]

    def multigrid_levels(self):
        """Aggregate levels of the multigrid hierarchy, finest first (mfh_multigrid_level_info)."""
        out = (C.c_int64 * (7 * 16))()
        n = C.c_int32()
        self._ck(self.lib.mfh_multigrid_level_info(self.h, 16, out, C.byref(n)))
        keys = ("aggregates", "rows", "entries", "partitioned", "peers", "halo_received", "owned_sent")
        return [dict(zip(keys, [int(out[7 * l + k]) for k in range(7)])) for l in range(min(n.value, 16))]

    def solve(self, f, rtol=1e-8, maxit=100000):
        f = as_f64(f)
        n = self.bs * self.n_dof
        nrhs = f.size // n
        assert f.size == nrhs * n
        u = np.empty_like(f)
        info = L.SolveInfo()
        st = self.lib.mfh_solve(self.h, nrhs, ptr(f), ptr(u), float(rtol), int(maxit), C.byref(info))
        self.last_info = info.as_dict()
        self._ck(st)
        return u

    def solve_batch(self, f, rtol=1e-8, maxit=100000):
        """All right-hand sides (rows of f) in batches sharing the operator passes; returns (u, [info per rhs])."""
        f = as_f64(f)
        n = self.bs * self.n_dof
        nrhs = f.size // n
        assert f.size == nrhs * n
        u = np.empty((nrhs, n))
        infos = (L.SolveInfo * nrhs)()
        st = self.lib.mfh_solve_batch(self.h, nrhs, ptr(f), ptr(u), float(rtol), int(maxit), infos)
        self.last_infos = [i.as_dict() for i in infos]
        self.last_info = self.last_infos[-1]
        self._ck(st)
        return u, self.last_infos

    def modes(self, nev, density=1.0, free=False, rtol=1e-6, maxit=500):
        """(lam, X, info): the nev smallest eigenpairs of K x = lam M x (mfh_modes), M = density x the consistent vector-valued mass matrix.
        free=False: clamped at the context's fixed variables; free=True: the free body, rigid-body modes excluded. X: [nev, dim * n_dof],
        rows M-orthonormal. info["residuals"] holds ||K x - lam M x|| / (lam ||M x||) per mode. Raises on MFH_ERR_NOT_CONVERGED like solve();
        what was reached is then in self.last_modes = (lam, X, info)."""
        nev = int(nev)
        n = self.bs * self.n_dof
        lam, X, res = np.zeros(max(nev, 0)), np.zeros((max(nev, 0), n)), np.zeros(max(nev, 0))
        info = L.ModesInfo()
        st = self.lib.mfh_modes(self.h, nev, float(density), L.MODES_FREE if free else 0, float(rtol), int(maxit), ptr(lam), ptr(X), ptr(res),
                                C.byref(info))
        d = info.as_dict()
        d["residuals"] = res
        self.last_modes = (lam, X, d)
        self._ck(st)
        return lam, X, d

    def modes_many(self, nev, density=1.0, free=False, locked=None, lambda_max=None, batch=0, rtol=1e-6, lock_factor=0.1, maxit=500):
        """(lam, X, info): the nev (<= 256 - len(locked)) smallest eigenpairs of K x = lam M x in the M-orthogonal complement of the rows of `locked`
        (any full-rank set, e.g. the X of an earlier call: that continues it), computed in batches of `batch` (0: 16) modes that are locked on the
        device one after the other (mfh_modes_many). lambda_max: stop once an eigenvalue above it has been found and return those below (then
        len(lam) = info["nFound"] and info["bandExhausted"] says whether the band is complete). lock_factor: batches that get locked run to
        rtol * lock_factor. lam ascending, X [nFound, dim * n_dof] M-orthonormal, info["residuals"] the full residuals recomputed after the last
        batch. Raises on MFH_ERR_NOT_CONVERGED like modes(); what was reached is then in self.last_modes_many = (lam, X, info)."""
        nev = int(nev)
        n = self.bs * self.n_dof
        Q = None
        if locked is not None:
            Q = as_f64(np.asarray(locked, dtype=np.float64).reshape(-1, n))
            if Q.shape[0] == 0:
                Q = None
        lam, X, res = np.zeros(max(nev, 0)), np.zeros((max(nev, 0), n)), np.zeros(max(nev, 0))
        prm = L.ModesManyParams(nev, 0 if Q is None else Q.shape[0], int(batch), L.MODES_FREE if free else 0, int(maxit), 0, float(density), float(rtol),
                                0.0 if lambda_max is None else float(lambda_max), float(lock_factor))
        info = L.ModesManyInfo()
        st = self.lib.mfh_modes_many(self.h, C.byref(prm), None if Q is None else ptr(Q), ptr(lam), ptr(X), ptr(res), C.byref(info))
        d = info.as_dict()
        k = d["nFound"] if st in (L.OK, L.ERR_NOT_CONVERGED) else 0
        d["residuals"] = res[:k]
        self.last_modes_many = (lam[:k], X[:k], d)
        self._ck(st)
        return self.last_modes_many

    def newmark(self, dt, n_steps, u0=None, v0=None, a0=None, f=None, amplitude=None, density=1.0, damping=(0.0, 0.0), beta=0.25, gamma=0.5,
                rtol=1e-8, maxit=10000, probes=None, snapshot_stride=0, energies=False):
        """Implicit Newmark time stepping of M u'' + C u' + K u = g(t) f on the device (mfh_newmark): M = density x the consistent vector-valued
        mass matrix, C = damping[0] M + damping[1] K, the context's fixed variables held at zero. u0 / v0: the state at step 0 (None: rest);
        a0: its acceleration (None: from M a0 = g0 f - C v0 - K u0; pass the "a" of an earlier call to continue that run); amplitude: g at the
        steps 0 .. n_steps (None: 1). Returns a dict: "u", "v", "a" (the state after the last step), "probes" [(n_steps + 1), len(probes)],
        "snapshots" [n_steps // snapshot_stride + 1, dim * n_dof] (snapshot_stride > 0), "energies" [(n_steps + 1), 3] = kinetic, strain,
        g f.u (energies=True) and "info". Raises on MFH_ERR_NOT_CONVERGED like solve(); what was reached (info["stepsDone"] steps) is then in
        self.last_newmark."""
        n = self.bs * self.n_dof
        n_steps = int(n_steps)
        rows = max(n_steps, 0) + 1

        def state(x):
            x = np.zeros(n) if x is None else np.array(x, dtype=np.float64).reshape(-1)
            if x.size != n:
                raise ValueError("newmark: a state vector needs dim * n_dof = %d entries, got %d" % (n, x.size))
            return np.ascontiguousarray(x)
        u, v, a = state(u0), state(v0), state(a0)
        f = None if f is None else as_f64(np.asarray(f, dtype=np.float64).reshape(-1))
        if f is not None and f.size != n:
            raise ValueError("newmark: f needs dim * n_dof = %d entries, got %d" % (n, f.size))
        amp = None if amplitude is None else as_f64(np.asarray(amplitude, dtype=np.float64).reshape(-1))
        if amp is not None and amp.size != rows:
            raise ValueError("newmark: amplitude needs n_steps + 1 = %d entries, got %d" % (rows, amp.size))
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((rows, n_probe)) if n_probe else None
        stride = int(snapshot_stride)
        snaps = np.zeros((max(n_steps, 0) // stride + 1, n)) if stride > 0 else None
        en = np.zeros((rows, 3)) if energies else None
        prm = L.NewmarkParams(float(dt), float(beta), float(gamma), float(density), float(damping[0]), float(damping[1]), float(rtol), n_steps,
                              int(maxit), stride, (L.DYN_HAVE_ACCEL if a0 is not None else 0) | (L.DYN_ENERGIES if energies else 0))
        info = L.NewmarkInfo()
        st = self.lib.mfh_newmark(self.h, C.byref(prm), ptr(u), ptr(v), ptr(a), ptr(f), ptr(amp), ptr(pv), n_probe, ptr(pout), ptr(snaps), ptr(en),
                                  C.byref(info))
        out = {"u": u, "v": v, "a": a, "probes": pout, "snapshots": snaps, "energies": en, "info": info.as_dict()}
        self.last_newmark = out
        self._ck(st)
        return out

    # ---------------------------------------------------------------- explicit dynamics (docs/design/04_20_explicit_dynamics.md)
    def mass_lumped_hrz(self):
        """The HRZ-lumped masses, dim * n_dof values (mfh_mass_lumped_hrz): per DoF the sum over its (element, local node) pairs of
        rho_e vol_e Mref_ii / trace(Mref), repeated for the components; positive on every element type, the context's density field inside."""
        out = np.empty(self.dim * self.n_dof)
        self._ck(self.lib.mfh_mass_lumped_hrz(self.h, ptr(out), 0))
        return out

    def explicit_dt(self, density=1.0, iters=0, x0=None):
        """The stability limit of central differences on (K, density x the HRZ-lumped mass) bracketed (mfh_explicit_dt): a dict with
        lambdaUpper >= lambda_max (Gershgorin, guaranteed), lambdaEst <= lambda_max (power iteration of `iters` steps, 0: 60, from x0 or the
        documented default start vector), dtSafe = 2 / sqrt(lambdaUpper), dtEst = 2 / sqrt(lambdaEst), iterations, ms, note."""
        n = self.bs * self.n_dof
        if x0 is not None:
            x0 = as_f64(np.asarray(x0, dtype=np.float64).reshape(-1))
            if x0.size != n:
                raise ValueError("explicit_dt: x0 needs dim * n_dof = %d entries, got %d" % (n, x0.size))
        info = L.ExplicitDtInfo()
        self._ck(self.lib.mfh_explicit_dt(self.h, float(density), int(iters), ptr(x0), C.byref(info)))
        return info.as_dict()

    def explicit(self, dt, n_steps, u0=None, v0=None, a0=None, f=None, amplitude=None, density=1.0, damping=0.0, probes=None, snapshot_stride=0,
                 energies=False, energy_stride=1, check_dt=True):
        """Central differences (velocity-Verlet form) on M_L u'' + damping M_L u' + K u = g(t) f on the device (mfh_explicit): M_L = density x
        the HRZ-lumped mass, the context's fixed variables held at zero. u0 / v0 / a0, f, amplitude, probes and snapshot_stride as in newmark().
        Returns a dict: "u", "v", "a" (the state after the last step), "probes", "snapshots", "energies" [n_steps // energy_stride + 1, 4] =
        kinetic, strain, g f.u, the leapfrog invariant (energies=True) and "info". check_dt=False runs a step above the stability estimate all
        the same; a run that blows up raises (MFH_ERR_NOT_CONVERGED), what was reached is then in self.last_explicit."""
        n = self.bs * self.n_dof
        n_steps = int(n_steps)
        rows = max(n_steps, 0) + 1

        def state(x):
            x = np.zeros(n) if x is None else np.array(x, dtype=np.float64).reshape(-1)
            if x.size != n:
                raise ValueError("explicit: a state vector needs dim * n_dof = %d entries, got %d" % (n, x.size))
            return np.ascontiguousarray(x)
        u, v, a = state(u0), state(v0), state(a0)
        f = None if f is None else as_f64(np.asarray(f, dtype=np.float64).reshape(-1))
        if f is not None and f.size != n:
            raise ValueError("explicit: f needs dim * n_dof = %d entries, got %d" % (n, f.size))
        amp = None if amplitude is None else as_f64(np.asarray(amplitude, dtype=np.float64).reshape(-1))
        if amp is not None and amp.size != rows:
            raise ValueError("explicit: amplitude needs n_steps + 1 = %d entries, got %d" % (rows, amp.size))
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((rows, n_probe)) if n_probe else None
        stride, estride = int(snapshot_stride), int(energy_stride)
        snaps = np.zeros((max(n_steps, 0) // stride + 1, n)) if stride > 0 else None
        en = np.zeros((max(n_steps, 0) // max(estride, 1) + 1, 4)) if energies else None
        prm = L.ExplicitParams(float(dt), float(density), float(damping), n_steps, stride, estride,
                               (L.EXP_HAVE_ACCEL if a0 is not None else 0) | (L.EXP_ENERGIES if energies else 0) | (0 if check_dt else L.EXP_NO_DT_CHECK))
        info = L.ExplicitInfo()
        st = self.lib.mfh_explicit(self.h, C.byref(prm), ptr(u), ptr(v), ptr(a), ptr(f), ptr(amp), ptr(pv), n_probe, ptr(pout), ptr(snaps), ptr(en),
                                   C.byref(info))
        out = {"u": u, "v": v, "a": a, "probes": pout, "snapshots": snaps, "energies": en, "info": info.as_dict()}
        self.last_explicit = out
        self._ck(st)
        return out

    def debug_explicit_step(self, dt, alpha, g, mode, last, y, u, v, inv, mass=None, f=None, a=None, probes=None, snapshot=True, energies=True):
        """k_explicit_step on host arrays (test hook mfh_debug_explicit_step): a dict of u, v, a after the kernel, probes, snapshot, energies[4]
        and flag."""
        y, inv = as_f64(y), as_f64(inv)
        n = y.size
        u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
        a = np.zeros(n) if a is None else np.array(a, dtype=np.float64)
        mass = None if mass is None else as_f64(mass)
        f = None if f is None else as_f64(f)
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros(n_probe) if n_probe else None
        snap = np.zeros(n) if snapshot else None
        en = np.zeros(4) if energies else None
        flag = np.zeros(1, dtype=np.int32)
        self._ck(self.lib.mfh_debug_explicit_step(self.h, n, float(dt), float(alpha), float(g), int(mode), int(last), ptr(y), ptr(u), ptr(v), ptr(inv),
                                                  ptr(mass), ptr(f), ptr(a), ptr(pv), n_probe, ptr(pout), ptr(snap), ptr(en), ptr(flag)))
        return {"u": u, "v": v, "a": a, "probes": pout, "snapshot": snap, "energies": en, "flag": int(flag[0])}

    def time_explicit_step(self, n, reps=50):
        """(ms per launch of k_explicit_step on n variables, ms per device-to-device copy of the bytes it moves) (mfh_time_explicit_step)."""
        step, copy = C.c_double(), C.c_double()
        self._ck(self.lib.mfh_time_explicit_step(self.h, int(n), int(reps), C.byref(step), C.byref(copy)))
        return step.value, copy.value

    def debug_hrz_weights(self):
        """[npe]: the HRZ weights of the element type as mass_lumped_hrz takes them from the mass table (test hook mfh_debug_hrz_weights)."""
        out = np.zeros(self.npe)
        self._ck(self.lib.mfh_debug_hrz_weights(self.h, ptr(out)))
        return out

    def debug_elem_abs_rowsums(self):
        """[n_elem, npe, dim]: the absolute row sums of the element stiffness matrices (test hook mfh_debug_elem_abs_rowsums)."""
        out = np.zeros((self.n_elem, self.npe, self.dim))
        self._ck(self.lib.mfh_debug_elem_abs_rowsums(self.h, ptr(out)))
        return out

    def harmonic(self, omega, f, f_imag=None, density=1.0, damping=(0.0, 0.0), loss_factor=0.0, rtol=1e-8, maxit=10000, probes=None, fields=True,
                 warm_start=True):
        """The frequency response (K + i w C - w^2 M) u^ = f^ at every w of omega (rad per unit time), on the device (mfh_harmonic): M = density x
        the consistent vector-valued mass matrix, C = damping[0] M + damping[1] K plus the structural term i loss_factor K, the context's fixed
        variables held at zero. f: the load, real or complex (f_imag: its imaginary plane given apart). Solved in the order given, each frequency
        warm-started from the previous solution unless warm_start=False. Returns a dict: "u" complex [nFreq, dim * n_dof] (fields=True, else
        None), "probes" complex [nFreq, len(probes)], "iterations" [nFreq], "true_residuals" [nFreq] = ||f^ - Z u^|| / ||f^|| and "info". Raises
        on MFH_ERR_NOT_CONVERGED like solve(); what was reached (info["freqsDone"] frequencies) is then in self.last_harmonic."""
        n = self.bs * self.n_dof
        om = as_f64(np.asarray(omega, dtype=np.float64).reshape(-1))
        nf = om.size
        f = np.asarray(f).reshape(-1)
        if f.size != n:
            raise ValueError("harmonic: f needs dim * n_dof = %d entries, got %d" % (n, f.size))
        f_re = np.ascontiguousarray(f.real, dtype=np.float64)
        f_im = np.ascontiguousarray(f.imag, dtype=np.float64) if np.iscomplexobj(f) else None
        if f_imag is not None:
            fi = np.asarray(f_imag, dtype=np.float64).reshape(-1)
            if fi.size != n:
                raise ValueError("harmonic: f_imag needs dim * n_dof = %d entries, got %d" % (n, fi.size))
            f_im = np.ascontiguousarray(fi if f_im is None else f_im + fi)
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((nf, n_probe, 2)) if n_probe else None
        fld = np.zeros((nf, 2, n)) if fields else None
        its, res = np.zeros(nf, dtype=np.int32), np.zeros(nf)
        prm = L.HarmonicParams(float(density), float(damping[0]), float(damping[1]), float(loss_factor), float(rtol), nf, int(maxit),
                               L.HARM_WARM_START if warm_start else 0)
        info = L.HarmonicInfo()
        st = self.lib.mfh_harmonic(self.h, C.byref(prm), ptr(om), ptr(f_re), ptr(f_im), ptr(pv), n_probe, ptr(pout), ptr(fld), ptr(its), ptr(res),
                                   C.byref(info))
        out = {"u": None if fld is None else fld[:, 0, :] + 1j * fld[:, 1, :],
               "probes": np.zeros((nf, 0), dtype=np.complex128) if pout is None else pout[:, :, 0] + 1j * pout[:, :, 1],
               "iterations": its, "true_residuals": res, "info": info.as_dict()}
        self.last_harmonic = out
        self._ck(st)
        return out

    # ---------------------------------------------------------------- modal superposition (docs/design/04_21_modal_superposition.md)
    def set_modal_basis(self, lam, X, density=1.0):
        """Keep the modes (lam [m], X [m, dim * n_dof], M-orthonormal at this density: the output of modes() / modes_many()) on the device as the
        basis of modal_coordinates() and modal_harmonic() (mfh_modal_set_basis). lam=None or an empty X drops the basis and its memory. Returns
        the info dict; info["orthoDefect"] = max |X (density M) X^T - I|. The basis belongs to the mesh, vertex positions, material, density
        field and fixed variables in force: after any of them changed the modal calls raise with code ERR_STATE."""
        n = self.bs * self.n_dof
        info = L.ModalBasisInfo()
        if lam is None or np.size(lam) == 0:
            self._ck(self.lib.mfh_modal_set_basis(self.h, 0, None, None, float(density), C.byref(info)))
            return info.as_dict()
        lam = as_f64(np.asarray(lam, dtype=np.float64).reshape(-1))
        X = as_f64(np.asarray(X, dtype=np.float64).reshape(-1, n))
        if X.shape[0] != lam.size:
            raise ValueError("set_modal_basis: %d eigenvalues for %d modes" % (lam.size, X.shape[0]))
        self._ck(self.lib.mfh_modal_set_basis(self.h, lam.size, ptr(lam), ptr(X), float(density), C.byref(info)))
        return info.as_dict()

    def modal_basis_state(self):
        """(nModes, valid): the modes of the basis in place (0: none) and whether the modal calls would accept it now (mfh_modal_basis_state)."""
        m, ok = C.c_int32(), C.c_int32()
        self._ck(self.lib.mfh_modal_basis_state(self.h, C.byref(m), C.byref(ok)))
        return m.value, bool(ok.value)

    def set_modal_basis_from_modes(self, n_modes, density=1.0):
        """Adopt the first n_modes modes the last modes_many() of this context left on the device as the basis of the modal calls
        (mfh_modal_set_basis_from_modes): what set_modal_basis(lam[:n_modes], X[:n_modes]) of its result sets, bit for bit, without the host round
        trip. Raises with code ERR_STATE if there is no such set or the mesh, material, density field or fixed variables changed since."""
        info = L.ModalBasisInfo()
        self._ck(self.lib.mfh_modal_set_basis_from_modes(self.h, int(n_modes), float(density), C.byref(info)))
        return info.as_dict()

    def modal_basis(self, nev, density=1.0, **kw):
        """modes_many(nev, density, **kw), its modes adopted on the device as the basis (set_modal_basis_from_modes; with a caller's `locked` set or
        fewer modes found than asked for: set_modal_basis of the result): (lam, X, info) of modes_many, info["modal_basis"] the basis's info."""
        lam, X, info = self.modes_many(nev, density=density, **kw)
        if len(lam) >= 1:
            info["modal_basis"] = self.set_modal_basis_from_modes(len(lam), density=density)
        else:
            info["modal_basis"] = self.set_modal_basis(lam, X, density=density)
        return lam, X, info

    def modal_coordinates(self, u):
        """q = X (density M) u, [nVec, nModes] (one row for a single field): the modal coordinates of the fields u in the basis of
        set_modal_basis (mfh_modal_coordinates)."""
        n = self.bs * self.n_dof
        u = np.asarray(u, dtype=np.float64)
        single = u.ndim == 1
        U2 = as_f64(u.reshape(-1, n))
        m = self.modal_basis_state()[0]
        q = np.zeros((U2.shape[0], m))
        self._ck(self.lib.mfh_modal_coordinates(self.h, ptr(U2), U2.shape[0], ptr(q) if q.size else None))
        return q[0] if single else q

    def modal_harmonic(self, omega, f, f_imag=None, damping=(0.0, 0.0), loss_factor=0.0, modal_damping=None, static_correction=True, residual_stride=None,
                       rtol=1e-8, maxit=10000, probes=None, fields=True):
        """The frequency response of harmonic() by superposition of the modes of set_modal_basis (mfh_modal_harmonic): u^(w) = sum_j phi_j q_j(w),
        q_j = phi_j^T f^ / (lam_j (1 + i (loss_factor + w damping[1])) - w^2 + i w damping[0] + 2 i zeta_j sqrt(lam_j) w), plus, with
        static_correction, the quasi-static response of the truncated modes from one solve K u_s = f^ per load plane at rtol / maxit. The density
        is the basis's. modal_damping: damping ratios zeta_j per mode. residual_stride: None = no residuals; k >= 0 = the true residual
        ||f^ - Z u^|| / ||f^|| of every k-th frequency (0: every one) through the operator of harmonic(). Returns the dict of harmonic() without
        "iterations", plus "modal_coords" complex [nFreq, nModes]; "true_residuals" holds -1 where nothing was computed."""
        n = self.bs * self.n_dof
        om = as_f64(np.asarray(omega, dtype=np.float64).reshape(-1))
        nf = om.size
        f = np.asarray(f).reshape(-1)
        if f.size != n:
            raise ValueError("modal_harmonic: f needs dim * n_dof = %d entries, got %d" % (n, f.size))
        f_re = np.ascontiguousarray(f.real, dtype=np.float64)
        f_im = np.ascontiguousarray(f.imag, dtype=np.float64) if np.iscomplexobj(f) else None
        if f_imag is not None:
            fi = np.asarray(f_imag, dtype=np.float64).reshape(-1)
            if fi.size != n:
                raise ValueError("modal_harmonic: f_imag needs dim * n_dof = %d entries, got %d" % (n, fi.size))
            f_im = np.ascontiguousarray(fi if f_im is None else f_im + fi)
        m = self.modal_basis_state()[0]
        zeta = _modal_zeta(modal_damping, m)
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((nf, n_probe, 2)) if n_probe else None
        fld = np.zeros((nf, 2, n)) if fields else None
        mc, res = np.zeros((nf, m, 2)), np.full(nf, -1.0)
        flags = (L.MODAL_STATIC_CORRECTION if static_correction else 0) | (0 if residual_stride is None else L.MODAL_RESIDUALS)
        prm = L.ModalHarmonicParams(float(damping[0]), float(damping[1]), float(loss_factor), float(rtol), int(maxit), nf,
                                    0 if residual_stride is None else int(residual_stride), flags)
        info = L.ModalHarmonicInfo()
        st = self.lib.mfh_modal_harmonic(self.h, C.byref(prm), ptr(om), ptr(zeta), ptr(f_re), ptr(f_im), ptr(pv), n_probe, ptr(pout), ptr(fld),
                                         ptr(mc) if mc.size else None, ptr(res), C.byref(info))
        out = {"u": None if fld is None else fld[:, 0, :] + 1j * fld[:, 1, :],
               "probes": np.zeros((nf, 0), dtype=np.complex128) if pout is None else pout[:, :, 0] + 1j * pout[:, :, 1],
               "modal_coords": mc[:, :, 0] + 1j * mc[:, :, 1], "true_residuals": res, "info": info.as_dict()}
        self.last_modal_harmonic = out
        self._ck(st)
        return out

    def debug_modal_expand(self, B, Cm, planes_per_pass=0):
        """out [nPlanes, n] = (B^T C)^T through k_modal_expand as the sweep launches it (test hook mfh_debug_modal_expand). B: [nb, n] (a row per
        column of the basis), Cm: [nb, nPlanes]."""
        B, Cm = as_f64(np.atleast_2d(B)), as_f64(np.atleast_2d(Cm))
        nb, n = B.shape
        assert Cm.shape[0] == nb
        out = np.zeros((Cm.shape[1], n))
        self._ck(self.lib.mfh_debug_modal_expand(self.h, n, nb, ptr(B), ptr(Cm), Cm.shape[1], int(planes_per_pass), ptr(out)))
        return out

    def debug_modal_gram(self, A, V):
        """G [na, nv] = A V^T through k_modal_gram and its second stage (test hook mfh_debug_modal_gram). A: [na <= 258, n], V: [nv <= 8, n] (a row per column)."""
        A, V = as_f64(np.atleast_2d(A)), as_f64(np.atleast_2d(V))
        assert A.shape[1] == V.shape[1]
        G = np.zeros((A.shape[0], V.shape[0]))
        self._ck(self.lib.mfh_debug_modal_gram(self.h, A.shape[1], A.shape[0], V.shape[0], ptr(A), ptr(V), ptr(G)))
        return G

    def time_modal_expand(self, n, nb, planes_per_pass=0, reps=5):
        """Device time (ms) per repetition of one pass of k_modal_expand on nb hashed columns of n rows (mfh_time_modal_expand)."""
        t = np.zeros(int(reps))
        self._ck(self.lib.mfh_time_modal_expand(self.h, int(n), int(nb), int(planes_per_pass), int(reps), ptr(t)))
        return t

    # ---------------------------------------------------------------- modal transient response (docs/design/04_22_modal_transient.md)
    def modal_transient(self, dt, n_steps, f, amplitude=None, q0=None, qdot0=None, u0=None, v0=None, damping=(0, 0), modal_damping=None,
                        static_correction=True, rtol=1e-8, maxit=10000, probes=None, snapshot_stride=0, modal_coords=False, energies=False,
                        chunk_steps=0):
        """The response to the load amplitude(t) f by exact integration of the modes of set_modal_basis (mfh_modal_transient): every mode obeys
        q'' + c_j q' + lam_j q = (phi_j^T f) a(t), c_j = damping[0] + damping[1] lam_j + 2 zeta_j sqrt(lam_j), with a(t) piecewise linear between
        amplitude[n] at n dt (None: 1), and is stepped without error; u = sum_j phi_j q_j (+ r_s a_n with static_correction: one solve K u_s = f
        at rtol / maxit, clamped bodies only). Start: q0 / qdot0 (modal) or u0 / v0 (fields, projected with modal_coordinates), not both; none:
        rest. Returns a dict like newmark(): "q", "qdot" (the state after the last step: pass them as q0 / qdot0 of the next call, whose
        amplitude[0] is this call's last value, to continue the run bit for bit), "probes" [n_steps + 1, len(probes)], "snapshots"
        [n_steps // snapshot_stride + 1, dim * n_dof] (snapshot_stride > 0), "modal_coords" [n_steps + 1, nModes], "energies" [n_steps + 1, 3] =
        1/2 sum qdot^2, 1/2 sum lam q^2, a sum g q, and "info". chunk_steps: steps per launch on the device (0: the default; a multiple of 32);
        it changes no result."""
        n = self.bs * self.n_dof
        n_steps = int(n_steps)
        rows = max(n_steps, 0) + 1
        if (q0 is not None or qdot0 is not None) and (u0 is not None or v0 is not None):
            raise ValueError("modal_transient: give the start as q0 / qdot0 or as u0 / v0, not both")
        f = as_f64(np.asarray(f, dtype=np.float64).reshape(-1))
        if f.size != n:
            raise ValueError("modal_transient: f needs dim * n_dof = %d entries, got %d" % (n, f.size))
        m = self.modal_basis_state()[0]

        def state(x, name):
            x = np.zeros(m) if x is None else np.array(x, dtype=np.float64).reshape(-1)
            if x.size != m:
                raise ValueError("modal_transient: %s needs one entry per mode (%d), got %d" % (name, m, x.size))
            return np.ascontiguousarray(x)
        if u0 is not None or v0 is not None:
            q0 = None if u0 is None else self.modal_coordinates(np.asarray(u0, dtype=np.float64).reshape(-1))
            qdot0 = None if v0 is None else self.modal_coordinates(np.asarray(v0, dtype=np.float64).reshape(-1))
        q, qd = state(q0, "q0"), state(qdot0, "qdot0")
        amp = None if amplitude is None else as_f64(np.asarray(amplitude, dtype=np.float64).reshape(-1))
        if amp is not None and amp.size != rows:
            raise ValueError("modal_transient: amplitude needs n_steps + 1 = %d entries, got %d" % (rows, amp.size))
        zeta = _modal_zeta(modal_damping, m)
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((rows, n_probe)) if n_probe else None
        stride = int(snapshot_stride)
        snaps = np.zeros((max(n_steps, 0) // stride + 1, n)) if stride > 0 else None
        mc = np.zeros((rows, m)) if modal_coords else None
        en = np.zeros((rows, 3)) if energies else None
        flags = (L.MODAL_TR_STATIC_CORRECTION if static_correction else 0) | (L.MODAL_TR_ENERGIES if energies else 0)
        prm = L.ModalTransientParams(float(dt), float(damping[0]), float(damping[1]), float(rtol), n_steps, int(maxit), stride, int(chunk_steps), flags, 0)
        info = L.ModalTransientInfo()
        st = self.lib.mfh_modal_transient(self.h, C.byref(prm), ptr(zeta), ptr(q) if m else None, ptr(qd) if m else None, ptr(f), ptr(amp), ptr(pv), n_probe,
                                          ptr(pout), ptr(snaps), ptr(mc) if mc is not None and mc.size else None, ptr(en), C.byref(info))
        out = {"q": q, "qdot": qd, "probes": np.zeros((rows, 0)) if pout is None else pout, "snapshots": snaps, "modal_coords": mc, "energies": en,
               "info": info.as_dict()}
        self.last_modal_transient = out
        self._ck(st)
        return out

    def debug_modal_march(self, coef8, g, amplitude, dt, q0, qdot0, chunk_steps=0, Bp=None, corr=False, lam=None, energies=False):
        """k_modal_march and k_modal_series on caller arrays (test hook mfh_debug_modal_march; no mesh needed). coef8: [m, 8] rows of
        modal_transient_coeffs, g: [m], amplitude: [n_steps + 1], Bp: [m + corr, nProbe] or None. Returns a dict: "q", "qdot" (after the last
        step), "modal_coords" [n_steps + 1, m], "probes" [n_steps + 1, nProbe], "energies" [n_steps + 1, 3] or None."""
        coef8, g, amp = as_f64(np.atleast_2d(coef8)), as_f64(np.asarray(g, dtype=np.float64).reshape(-1)), as_f64(np.asarray(amplitude, dtype=np.float64).reshape(-1))
        m, rows = coef8.shape[0], amp.size
        assert coef8.shape[1] == 8 and g.size == m
        q, qd = np.array(q0, dtype=np.float64).reshape(-1), np.array(qdot0, dtype=np.float64).reshape(-1)
        assert q.size == m and qd.size == m
        n_probe = 0
        if Bp is not None:
            Bp = as_f64(np.atleast_2d(Bp))
            assert Bp.shape[0] == m + int(bool(corr))
            n_probe = Bp.shape[1]
        lam = None if lam is None else as_f64(np.asarray(lam, dtype=np.float64).reshape(-1))
        mc = np.zeros((rows, m))
        pout = np.zeros((rows, n_probe)) if n_probe else None
        en = np.zeros((rows, 3)) if energies else None
        self._ck(self.lib.mfh_debug_modal_march(self.h, m, ptr(coef8), ptr(g), ptr(lam), float(dt), rows - 1, ptr(amp), int(chunk_steps), ptr(q), ptr(qd),
                                                ptr(Bp) if n_probe else None, n_probe, int(bool(corr)), ptr(mc), ptr(pout), ptr(en)))
        return {"q": q, "qdot": qd, "modal_coords": mc, "probes": np.zeros((rows, 0)) if pout is None else pout, "energies": en}

    def time_modal_series(self, n_modes, n_probe, n_steps, reps=5):
        """(series_ms, expand_ms), one entry per repetition: device time of k_modal_series and of the k_modal_expand route on the same shape, the two
        taking turns (mfh_time_modal_series)."""
        a, b = np.zeros(int(reps)), np.zeros(int(reps))
        self._ck(self.lib.mfh_time_modal_series(self.h, int(n_modes), int(n_probe), int(n_steps), int(reps), ptr(a), ptr(b)))
        return a, b

    # ---------------------------------------------------------------- random vibration, response spectra (docs/design/04_23_modal_random.md)
    def modal_quadratic(self, Cm, tol=-1.0, probes=None, fields=True):
        """sqrt(phi_i^T C phi_i) per variable i for symmetric positive semi-definite matrices C over the modes of set_modal_basis
        (mfh_modal_quadratic): Cm [m, m] or [nMat <= 4, m, m]. The host factors C = F F^T (psd_factor; tol < 0: its default) and the device sums
        squares, so the result is never negative. Returns a dict: "fields" [nMat, dim * n_dof] (None without fields), "probes" [nMat, len(probes)]
        (bit for bit the field entries), "info" (ranks, passes, truncation per matrix)."""
        n = self.bs * self.n_dof
        m = self.modal_basis_state()[0]
        Cm = as_f64(np.asarray(Cm, dtype=np.float64))
        if Cm.ndim == 2:
            Cm = Cm[None]
        if Cm.ndim != 3 or (m > 0 and Cm.shape[1:] != (m, m)):          # (no basis: the library answers with ERR_STATE)
            raise ValueError("modal_quadratic: the matrices are %d x %d (the modes of the basis), got %s" % (m, m, Cm.shape))
        Cm = np.ascontiguousarray(Cm)
        n_mat = Cm.shape[0]
        pv, n_probe = _probe_vars(probes)
        pout = np.zeros((n_mat, n_probe)) if n_probe else None
        fld = np.zeros((n_mat, n)) if fields else None
        info = L.ModalQuadraticInfo()
        self._ck(self.lib.mfh_modal_quadratic(self.h, n_mat, ptr(Cm), float(tol), ptr(pv), n_probe, ptr(pout), ptr(fld), C.byref(info)))
        d = info.as_dict()
        for k in ("ranks", "passes", "truncation"):
            d[k] = d[k][:n_mat]
        return {"fields": fld, "probes": np.zeros((n_mat, 0)) if pout is None else pout, "info": d}

    def modal_random(self, omega, S, f, weights=None, damping=(0.0, 0.0), loss_factor=0.0, modal_damping=None, static_correction=True, velocity=False,
                     acceleration=False, tol=-1.0, rtol=1e-8, maxit=10000, probes=None, fields=True, probe_psd=False):
        """The RMS response to the loads sum_a A_a(t) f_a whose amplitudes have the one-sided cross-spectral density S(omega) (mfh_modal_random),
        on the basis of set_modal_basis. omega: strictly ascending grid [nFreq]; S: [nFreq] (one load), or [nFreq, nLoad, nLoad] Hermitian;
        f: [dim * n_dof] or [nLoad, dim * n_dof] real load shapes; weights: quadrature weights (None: the trapezoid rule). Damping as
        modal_harmonic. static_correction: one static solve per load (at most two loads with it). Returns a dict: "sigma_u", "sigma_v" (velocity),
        "sigma_a" (acceleration): fields [dim * n_dof] or None; "probes": dict of "sigma_u", "sigma_v", "sigma_a", "nu0" (rate of upward zero
        crossings sigma_v / (2 pi sigma_u)) [len(probes)] and "psd" [len(probes), nFreq] with probe_psd; "cov": [3, nb, nb] = the modal covariances
        C^(0), C^(2), C^(4); "info"."""
        n = self.bs * self.n_dof
        om = as_f64(np.asarray(omega, dtype=np.float64).reshape(-1))
        nf = om.size
        f = as_f64(np.asarray(f, dtype=np.float64))
        f = f.reshape(1, -1) if f.ndim == 1 else f.reshape(f.shape[0], -1)
        if f.shape[1] != n:
            raise ValueError("modal_random: a load needs dim * n_dof = %d entries, got %d" % (n, f.shape[1]))
        nl = f.shape[0]
        Sc = np.asarray(S, dtype=np.complex128)
        if Sc.ndim == 1:
            Sc = Sc.reshape(-1, 1, 1)
        if Sc.shape != (nf, nl, nl):
            raise ValueError("modal_random: S needs the shape [nFreq, nLoad, nLoad] = %s, got %s" % ((nf, nl, nl), Sc.shape))
        Sri = np.ascontiguousarray(np.stack([Sc.real, Sc.imag], axis=-1))
        w = None if weights is None else as_f64(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w is not None and w.size != nf:
            raise ValueError("modal_random: %d weights for %d frequencies" % (w.size, nf))
        m = self.modal_basis_state()[0]
        zeta = _modal_zeta(modal_damping, m)
        pv, n_probe = _probe_vars(probes)
        prms = np.zeros((4, n_probe)) if n_probe else None
        ppsd = np.zeros((n_probe, nf)) if n_probe and probe_psd else None
        planes = 1 + int(bool(velocity)) + int(bool(acceleration))
        fld = np.zeros((planes, n)) if fields else None
        nbmax = m + 2
        cov = np.zeros(3 * nbmax * nbmax)
        flags = ((L.MODAL_RV_STATIC_CORRECTION if static_correction else 0) | (L.MODAL_RV_VELOCITY if velocity else 0) |
                 (L.MODAL_RV_ACCELERATION if acceleration else 0))
        prm = L.ModalRandomParams(float(damping[0]), float(damping[1]), float(loss_factor), float(rtol), float(tol), int(maxit), nf, nl, flags)
        info = L.ModalRandomInfo()
        st = self.lib.mfh_modal_random(self.h, C.byref(prm), ptr(om), ptr(w), ptr(zeta), ptr(f), ptr(Sri), ptr(pv), n_probe, ptr(prms), ptr(ppsd), ptr(fld),
                                       ptr(cov), C.byref(info))
        d = info.as_dict()
        self.last_modal_random = {"info": d}
        self._ck(st)
        nb = d["nb"]
        out = {"sigma_u": None, "sigma_v": None, "sigma_a": None, "cov": cov[:3 * nb * nb].reshape(3, nb, nb).copy(), "info": d}
        if fld is not None:
            names = ["sigma_u"] + (["sigma_v"] if velocity else []) + (["sigma_a"] if acceleration else [])
            for i, name in enumerate(names):
                out[name] = fld[i]
        pr = {"sigma_u": np.zeros(0), "sigma_v": np.zeros(0), "sigma_a": np.zeros(0), "nu0": np.zeros(0), "psd": ppsd}
        if n_probe:
            pr.update({"sigma_u": prms[0], "sigma_v": prms[1], "sigma_a": prms[2] if acceleration else None, "nu0": prms[3]})
        out["probes"] = pr
        self.last_modal_random = out
        return out

    def debug_modal_sumsq(self, B, F, piv=None, planes_per_pass=0, sqrt=False):
        """out [n] = sum_t (sum_j B[j] F[j][t])^2 through k_modal_sumsq as the calls above launch it (test hook mfh_debug_modal_sumsq). B: [nb, n]
        (a row per column of the basis), F: [nb, rank]. piv: the pivots of psd_factor, for the shortened column lists of the later passes."""
        B = as_f64(np.atleast_2d(B))
        F = np.asarray(F, dtype=np.float64)
        F = as_f64(F.reshape(B.shape[0], F.size // B.shape[0]))
        nb, n = B.shape
        rank = F.shape[1]
        pv = None if piv is None else as_i32(np.asarray(piv).reshape(-1))
        assert pv is None or pv.size == rank
        out = np.full(n, np.nan)
        self._ck(self.lib.mfh_debug_modal_sumsq(self.h, n, nb, ptr(B), ptr(F) if rank else None, rank, ptr(pv) if rank else None, int(planes_per_pass), int(bool(sqrt)),
                                                ptr(out)))
        return out

    def time_modal_sumsq(self, n, nb, planes_per_pass=0, reps=5):
        """(sumsq_ms, expand_ms, later_ms), one entry per repetition: device time of one pass of k_modal_sumsq and of one pass of k_modal_expand on
        the same nb hashed columns of n rows, the two taking turns, and of a second pass of a rank-2 NP factor (nb - NP columns, the accumulator read
        back; mfh_time_modal_sumsq)."""
        a, b, l = np.zeros(int(reps)), np.zeros(int(reps)), np.zeros(int(reps))
        self._ck(self.lib.mfh_time_modal_sumsq(self.h, int(n), int(nb), int(planes_per_pass), int(reps), ptr(a), ptr(b), ptr(l)))
        return a, b, l

    # ---------------------------------------------------------------- modal stress recovery (docs/design/04_24_modal_stress.md)
    def _stress_flags(self, von_mises, components, strain):
        return ((L.MODAL_STRESS_VON_MISES if von_mises else 0) | (L.MODAL_STRESS_COMPONENTS if components else 0) | (L.MODAL_STRESS_STRAIN if strain else 0))

    def _stress_result(self, n_mat, vm, comp, info, squeeze):
        d = info.as_dict()
        for k in ("ranks", "passes", "truncation", "peakVonMises", "peakCorner"):
            d[k] = d[k][:n_mat]
        nq = self._nq()
        peak = [(d["peakVonMises"][a], int(d["peakCorner"][a] // nq), int(d["peakCorner"][a] % nq)) for a in range(n_mat)]
        if squeeze:
            vm, comp, peak = (None if vm is None else vm[0]), (None if comp is None else comp[0]), peak[0]
        return {"von_mises": vm, "components": comp, "peak": peak, "info": d}

    def modal_quadratic_stress(self, Cm, tol=-1.0, von_mises=True, components=False, strain=False):
        """RMS stress per element corner for symmetric positive semi-definite matrices C over the modes of set_modal_basis
        (mfh_modal_quadratic_stress): Cm [m, m] or [nMat <= 4, m, m]; the SRSS / CQC rules are C_jk = rho_jk a_j a_k. Returns a dict: "von_mises"
        [nMat, nElem, NQ] = sqrt(E[sigma_vm^2]) (Segalman: the root of the mean square, not the mean), "components" [nMat, nElem, NQ, flatLen] =
        sqrt(E[sigma_c^2]) (None where not asked for), "peak": per matrix (largest von Mises value, element, corner), "info". strain=True: strains
        instead of stresses."""
        m = self.modal_basis_state()[0]
        Cm = as_f64(np.asarray(Cm, dtype=np.float64))
        if Cm.ndim == 2:
            Cm = Cm[None]
        if Cm.ndim != 3 or (m > 0 and Cm.shape[1:] != (m, m)):          # (no basis: the library answers with ERR_STATE)
            raise ValueError("modal_quadratic_stress: the matrices are %d x %d (the modes of the basis), got %s" % (m, m, Cm.shape))
        Cm = np.ascontiguousarray(Cm)
        n_mat = Cm.shape[0]
        nq, fl = self._nq(), flat_len(self.dim)
        vm = np.full((n_mat, self.n_elem, nq), np.nan) if von_mises else None
        comp = np.full((n_mat, self.n_elem, nq, fl), np.nan) if components else None
        info = L.ModalStressInfo()
        st = self.lib.mfh_modal_quadratic_stress(self.h, n_mat, ptr(Cm), float(tol), self._stress_flags(von_mises, components, strain), ptr(vm), ptr(comp), C.byref(info))
        self.last_modal_stress = {"von_mises": vm, "components": comp, "info": info.as_dict()}
        self._ck(st)
        self.last_modal_stress = self._stress_result(n_mat, vm, comp, info, False)
        return self.last_modal_stress

    def modal_random_stress(self, omega, S, f, weights=None, damping=(0.0, 0.0), loss_factor=0.0, modal_damping=None, static_correction=True, tol=-1.0,
                            rtol=1e-8, maxit=10000, von_mises=True, components=False, strain=False, _rv_flags=0):
        """RMS stress per element corner under the loads of modal_random (mfh_modal_random_stress; the same arguments, the displacement's
        covariance only). Returns a dict: "von_mises" [nElem, NQ] = sqrt(E[sigma_vm^2]), "components" [nElem, NQ, flatLen], "peak" (value,
        element, corner), "cov" [nb, nb] = C^(0), "info"."""
        n = self.bs * self.n_dof
        om = as_f64(np.asarray(omega, dtype=np.float64).reshape(-1))
        nf = om.size
        f = as_f64(np.asarray(f, dtype=np.float64))
        f = f.reshape(1, -1) if f.ndim == 1 else f.reshape(f.shape[0], -1)
        if f.shape[1] != n:
            raise ValueError("modal_random_stress: a load needs dim * n_dof = %d entries, got %d" % (n, f.shape[1]))
        nl = f.shape[0]
        Sc = np.asarray(S, dtype=np.complex128)
        if Sc.ndim == 1:
            Sc = Sc.reshape(-1, 1, 1)
        if Sc.shape != (nf, nl, nl):
            raise ValueError("modal_random_stress: S needs the shape [nFreq, nLoad, nLoad] = %s, got %s" % ((nf, nl, nl), Sc.shape))
        Sri = np.ascontiguousarray(np.stack([Sc.real, Sc.imag], axis=-1))
        w = None if weights is None else as_f64(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w is not None and w.size != nf:
            raise ValueError("modal_random_stress: %d weights for %d frequencies" % (w.size, nf))
        m = self.modal_basis_state()[0]
        zeta = _modal_zeta(modal_damping, m)
        nq, fl = self._nq(), flat_len(self.dim)
        vm = np.full((1, self.n_elem, nq), np.nan) if von_mises else None
        comp = np.full((1, self.n_elem, nq, fl), np.nan) if components else None
        nbmax = m + 2
        cov = np.zeros(nbmax * nbmax)
        flags = (L.MODAL_RV_STATIC_CORRECTION if static_correction else 0) | int(_rv_flags)
        prm = L.ModalRandomParams(float(damping[0]), float(damping[1]), float(loss_factor), float(rtol), float(tol), int(maxit), nf, nl, flags)
        info = L.ModalStressInfo()
        st = self.lib.mfh_modal_random_stress(self.h, C.byref(prm), ptr(om), ptr(w), ptr(zeta), ptr(f), ptr(Sri), self._stress_flags(von_mises, components, strain),
                                              ptr(vm), ptr(comp), ptr(cov), C.byref(info))
        self.last_modal_stress = {"von_mises": vm, "components": comp, "info": info.as_dict()}
        self._ck(st)
        out = self._stress_result(1, vm, comp, info, True)
        nb = out["info"]["nb"]
        out["cov"] = cov[:nb * nb].reshape(nb, nb).copy()
        self.last_modal_stress = out
        return out

    def debug_modal_stress_sumsq(self, U, planes_per_pass=0, components=True, strain=False, sqrt=False):
        """(vm [nElem, NQ], comp [nElem, NQ, flatLen] or None): the sums over the planes U [nPlanes, dim * n_dof] (variable numbering) of the squared
        von Mises value / the squared components of the corner stress, through k_modal_stress_sumsq planes_per_pass planes at a time (test hook
        mfh_debug_modal_stress_sumsq); their roots with sqrt."""
        n = self.bs * self.n_dof
        U = as_f64(np.asarray(U, dtype=np.float64).reshape(-1, n))
        nq, fl = self._nq(), flat_len(self.dim)
        vm = np.full((self.n_elem, nq), np.nan)
        comp = np.full((self.n_elem, nq, fl), np.nan) if components else None
        self._ck(self.lib.mfh_debug_modal_stress_sumsq(self.h, U.shape[0], ptr(U) if U.shape[0] else None, int(planes_per_pass),
                                                       self._stress_flags(True, components, strain), int(bool(sqrt)), ptr(vm), ptr(comp)))
        return vm, comp

    def debug_peak_of_array(self, v):
        """(max, argmax) of a host array through k_peak_of_array and k_peak_finish: ties to the lowest index, a NaN before every number."""
        v = as_f64(np.asarray(v, dtype=np.float64).reshape(-1))
        val, idx = C.c_double(), C.c_int64()
        self._ck(self.lib.mfh_debug_peak_of_array(self.h, v.size, ptr(v), C.byref(val), C.byref(idx)))
        return val.value, idx.value

    def time_modal_stress(self, n_planes=32, reps=5):
        """(stress_ms, measures_ms), one entry per repetition: device time of one pass of k_modal_stress_sumsq over n_planes hashed planes and of
        n_planes launches of k_stress_measures (von Mises only) on the same planes, the two taking turns (mfh_time_modal_stress)."""
        a, b = np.zeros(int(reps)), np.zeros(int(reps))
        self._ck(self.lib.mfh_time_modal_stress(self.h, int(n_planes), int(reps), ptr(a), ptr(b)))
        return a, b

    # ---------------------------------------------------------------- per-element density (docs/design/04_15_density.md)
    def set_density(self, rho):
        """The density field of the mass matrix of modes() and newmark() (mfh_set_density): one strictly positive value per element, or
        None for unit density. Their scalar density= multiplies the field. It survives mesh_update_vertices; a new mesh clears it."""
        if rho is None:
            self._ck(self.lib.mfh_set_density(self.h, None, 0, 0))
            return
        rho = as_f64(np.asarray(rho, dtype=np.float64).reshape(-1))
        self._ck(self.lib.mfh_set_density(self.h, ptr(rho), rho.size, 0))

    def mass_apply(self, x, out=None):
        """y = M x on a displacement vector of dim * n_dof entries (mfh_mass_apply): M the consistent vector-valued mass matrix with the
        context's density field, no fixed variables masked. Returns an array of x's shape (out: a C-contiguous float64 array to write)."""
        x = as_f64(x)
        n = self.dim * self.n_dof
        if x.size != n:
            raise ValueError("mass_apply: x needs dim * n_dof = %d entries, got %d" % (n, x.size))
        if out is None:
            out = np.empty(x.shape)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != n or np.shares_memory(out, x):
            raise ValueError("out: a C-contiguous float64 array of dim * n_dof values that does not overlap x")
        self._ck(self.lib.mfh_mass_apply(self.h, ptr(x), ptr(out), 0))
        return out

    def mass_properties(self, scale=1.0):
        """{"mass", "com", "second_moment", "inertia"} of the body with the context's density field times scale (mfh_mass_properties):
        second_moment = int rho (x - com)(x - com)^T [dim, dim]; inertia = tr(S) I - S in 3D (the tensor about the centre of mass), the
        polar moment tr(S) in 2D. Ordered sums on the device: the same call returns the same bits."""
        d = self.dim
        mass, com, S = C.c_double(), np.zeros(d), np.zeros((d, d))
        self._ck(self.lib.mfh_mass_properties(self.h, float(scale), C.byref(mass), ptr(com), ptr(S), 0))
        inertia = np.trace(S) * np.eye(3) - S if d == 3 else float(np.trace(S))
        return {"mass": mass.value, "com": com, "second_moment": S, "inertia": inertia}

    # ---------------------------------------------------------------- linear buckling (docs/design/04_16_buckling.md)
    def set_prestress(self, sigma):
        """The prestress field of geometric_apply() and buckling() (mfh_set_prestress): one symmetric tensor per element [nElem, flatLen] in the
        layout of average_stress (tensor shear entries), any finite values, or None to clear it. It survives mesh_update_vertices; a new mesh
        clears it."""
        if sigma is None:
            self._ck(self.lib.mfh_set_prestress(self.h, None, 0, 0))
            return
        sigma = as_f64(np.asarray(sigma, dtype=np.float64))
        fl = flat_len(self.dim)
        if sigma.ndim != 2 or sigma.shape[1] != fl:
            raise ValueError("sigma: [nElem, flatLen = %d]" % fl)
        self._ck(self.lib.mfh_set_prestress(self.h, ptr(sigma), sigma.shape[0], 0))

    def prestress_from_displacement(self, u_nodes):
        """Sets the prestress field to C_e : (element-average strain of u) for a per-node displacement [nNode, dim], on the device
        (mfh_prestress_from_displacement): what average_stress(u) returns, without the host trip."""
        u = as_f64(u_nodes)
        if u.size != self.n_node * self.dim:
            raise ValueError("prestress_from_displacement: u needs n_node * dim = %d entries, got %d" % (self.n_node * self.dim, u.size))
        self._ck(self.lib.mfh_prestress_from_displacement(self.h, ptr(u), 0))

    def geometric_apply(self, x, out=None):
        """y = Kg x on a displacement vector of dim * n_dof entries (mfh_geometric_apply): Kg the geometric stiffness of the context's prestress
        field, no fixed variables masked. Returns an array of x's shape (out: a C-contiguous float64 array to write)."""
        x = as_f64(x)
        n = self.dim * self.n_dof
        if x.size != n:
            raise ValueError("geometric_apply: x needs dim * n_dof = %d entries, got %d" % (n, x.size))
        if out is None:
            out = np.empty(x.shape)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != n or np.shares_memory(out, x):
            raise ValueError("out: a C-contiguous float64 array of dim * n_dof values that does not overlap x")
        self._ck(self.lib.mfh_geometric_apply(self.h, ptr(x), ptr(out), 0))
        return out

    def buckling(self, nev, rtol=1e-6, maxit=500):
        """(factors, X, info): the nev smallest load factors of (K + factor Kg) x = 0 on the clamped context (mfh_buckling), Kg the geometric
        stiffness of the prestress field. factors ascending, +inf where the prestress does not buckle the body; X: [nev, dim * n_dof], rows
        K-orthonormal; info["residuals"] holds ||Kg x - mu K x|| / (|mu| ||K x||) per mode, info["nBuckling"] the number of finite factors.
        Raises on MFH_ERR_NOT_CONVERGED like solve(); what was reached is then in self.last_buckling = (factors, X, info)."""
        nev = int(nev)
        n = self.bs * self.n_dof
        fac, X, res = np.zeros(max(nev, 0)), np.zeros((max(nev, 0), n)), np.zeros(max(nev, 0))
        info = L.BucklingInfo()
        st = self.lib.mfh_buckling(self.h, nev, 0, float(rtol), int(maxit), ptr(fac), ptr(X), ptr(res), C.byref(info))
        d = info.as_dict()
        d["residuals"] = res
        self.last_buckling = (fac, X, d)
        self._ck(st)
        return fac, X, d

    # ---------------------------------------------------------------- prestressed vibration (docs/design/04_18_prestressed_modes.md)
    def modes_prestressed(self, nev, load_factor, density=1.0, x0=None, rtol=1e-6, maxit=500):
        """(lam, X, info): the nev smallest eigenpairs of (K + load_factor Kg) x = lam density M x on the clamped context (mfh_modes_prestressed),
        Kg the geometric stiffness of the prestress field. lam ascending -- negative beyond the critical load, info["note"] then says how many;
        X: [nev, dim * n_dof], rows M-orthonormal; x0: [nev, dim * n_dof] shapes to start from (those of a neighbouring load factor).
        info["residuals"] holds ||A x - lam M x|| / (|lam| ||M x||) per mode. Raises on MFH_ERR_NOT_CONVERGED like solve(); what was reached is
        then in self.last_modes_prestressed = (lam, X, info)."""
        nev = int(nev)
        n = self.bs * self.n_dof
        lam, X, res = np.zeros(max(nev, 0)), np.zeros((max(nev, 0), n)), np.zeros(max(nev, 0))
        if x0 is not None:
            x0 = as_f64(x0)
            if x0.size != max(nev, 0) * n:
                raise ValueError("x0: [nev, dim * n_dof] = [%d, %d]" % (nev, n))
        info = L.ModesInfo()
        st = self.lib.mfh_modes_prestressed(self.h, nev, float(density), float(load_factor), 0, float(rtol), int(maxit),
                                            None if x0 is None else ptr(x0), ptr(lam), ptr(X), ptr(res), C.byref(info))
        d = info.as_dict()
        d["residuals"] = res
        self.last_modes_prestressed = (lam, X, d)
        self._ck(st)
        return lam, X, d

    def tangent_apply(self, x, load_factor, out=None):
        """y = (K + load_factor Kg) x on a displacement vector of dim * n_dof entries (mfh_tangent_apply), no fixed variables masked. Returns an
        array of x's shape (out: a C-contiguous float64 array to write)."""
        x = as_f64(x)
        n = self.dim * self.n_dof
        if x.size != n:
            raise ValueError("tangent_apply: x needs dim * n_dof = %d entries, got %d" % (n, x.size))
        if out is None:
            out = np.empty(x.shape)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != n or np.shares_memory(out, x):
            raise ValueError("out: a C-contiguous float64 array of dim * n_dof values that does not overlap x")
        self._ck(self.lib.mfh_tangent_apply(self.h, float(load_factor), ptr(x), ptr(out), 0))
        return out

    def debug_kron_pair(self, s, rho, x, yA, masked=True, two_pass=False):
        """(yA + s Kg x, rho M x) through the launcher of the prestressed loop (test hook mfh_debug_kron_pair): k_spmv_kron_pair, or with
        two_pass the two launches it replaces."""
        x = as_f64(x)
        a = np.array(as_f64(yA), dtype=np.float64).reshape(-1)
        b = np.empty(self.bs * self.n_dof)
        if x.size != b.size or a.size != b.size:
            raise ValueError("x, yA: dim * n_dof = %d entries" % b.size)
        self._ck(self.lib.mfh_debug_kron_pair(self.h, float(s), float(rho), 1 if masked else 0, 1 if two_pass else 0, ptr(x), ptr(a), ptr(b)))
        return a, b

    def debug_newmark_predict(self, dt, beta, gamma, density, damping, u, v, a, mask=None, want_xk=True):
        """(ut, vt, xm, xk) of k_newmark_predict on host arrays (test hook mfh_debug_newmark_predict)."""
        u, v, a = as_f64(u), as_f64(v), as_f64(a)
        n = u.size
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        ut, vt, xm = np.empty(n), np.empty(n), np.empty(n)
        xk = np.empty(n) if want_xk else None
        self._ck(self.lib.mfh_debug_newmark_predict(self.h, n, float(dt), float(beta), float(gamma), float(density), float(damping[0]), float(damping[1]),
                                                    ptr(m), ptr(u), ptr(v), ptr(a), ptr(ut), ptr(vt), ptr(xm), ptr(xk)))
        return ut, vt, xm, xk

    def debug_newmark_rhs(self, g, f, y, mask=None):
        """(b, b . b) of k_newmark_rhs and its second stage (test hook mfh_debug_newmark_rhs)."""
        y = as_f64(y)
        f = None if f is None else as_f64(f)
        n = y.size
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        b, bb = np.empty(n), np.zeros(1)
        self._ck(self.lib.mfh_debug_newmark_rhs(self.h, n, float(g), ptr(f), ptr(y), ptr(m), ptr(b), ptr(bb)))
        return b, float(bb[0])

    def debug_newmark_correct(self, dt, beta, gamma, x, ut, vt, probes=None, snapshot=True):
        """(u, v, a, probe values, snapshot row) of k_newmark_correct (test hook mfh_debug_newmark_correct)."""
        x, ut, vt = as_f64(x), as_f64(ut), as_f64(vt)
        n = x.size
        pv = None if probes is None else as_i64(probes)
        n_probe = 0 if pv is None else pv.size
        u, v, a = np.empty(n), np.empty(n), np.empty(n)
        pout = np.empty(n_probe) if n_probe else None
        snap = np.empty(n) if snapshot else None
        self._ck(self.lib.mfh_debug_newmark_correct(self.h, n, float(dt), float(beta), float(gamma), ptr(x), ptr(ut), ptr(vt), ptr(u), ptr(v), ptr(a),
                                                    ptr(pv), n_probe, ptr(pout), ptr(snap)))
        return u, v, a, pout, snap

    def debug_harmonic_apply(self, zK, zM, x, masked=True):
        """(zK K x + zM M x, x^T y) for complex zK, zM, x through the context's operator and k_spmv_kron_cacc (test hook
        mfh_debug_harmonic_apply; M with density 1; option harmonic_two_pass selects the two-launch form)."""
        x = np.asarray(x, dtype=np.complex128).reshape(-1)
        n = self.bs * self.n_dof
        assert x.size == n
        xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
        yr, yi, dot = np.empty(n), np.empty(n), np.zeros(2)
        zK, zM = complex(zK), complex(zM)
        self._ck(self.lib.mfh_debug_harmonic_apply(self.h, zK.real, zK.imag, zM.real, zM.imag, 1 if masked else 0, ptr(xr), ptr(xi), ptr(yr), ptr(yi),
                                                   ptr(dot)))
        return yr + 1j * yi, complex(dot[0], dot[1])

    def debug_pencil_apply(self, cK, cM, x, masked=True):
        """(cK K x + cM M x, x . y) through the context's operator and k_spmv_kron_acc (test hook mfh_debug_pencil_apply; M with density 1)."""
        x = as_f64(x)
        y, dot = np.empty(self.bs * self.n_dof), np.zeros(1)
        assert x.size == y.size
        self._ck(self.lib.mfh_debug_pencil_apply(self.h, float(cK), float(cM), 1 if masked else 0, ptr(x), ptr(y), ptr(dot)))
        return y, float(dot[0])

    def debug_pencil_precond(self, cK, cM, r):
        """z = Dinv r with the inverse diagonal blocks the Newmark and harmonic loops build for cK K + cM M (test hook mfh_debug_pencil_precond;
        M with density 1, the fixed variables decoupled)."""
        r = as_f64(r).reshape(-1)
        z = np.empty(self.bs * self.n_dof)
        assert r.size == z.size
        self._ck(self.lib.mfh_debug_pencil_precond(self.h, float(cK), float(cM), ptr(r), ptr(z)))
        return z

    def _ck_loop(self, st):
        """the status of a loop hook: MFH_ERR_NOT_CONVERGED (the loop ended at maxit: its iterate is what the caller asked for) passes"""
        if st != L.ERR_NOT_CONVERGED:
            self._ck(st)

    def debug_newmark_pcg(self, cK, cM, b, x0=None, rtol=1e-30, maxit=1):
        """(x, history [maxit + 1, 4] = {r.z, p.Ap, r.r, -}, its) of the PCG of mfh_newmark on cK K + cM M from x0 (test hook mfh_debug_newmark_pcg;
        M with density 1). its: the iteration that met rtol, -1 at maxit (x is then iterate maxit), -2 on a breakdown."""
        n = self.bs * self.n_dof
        b = as_f64(b).reshape(-1)
        x0 = None if x0 is None else as_f64(x0).reshape(-1)
        assert b.size == n and (x0 is None or x0.size == n)
        x, hist, its = np.full(n, np.nan), np.zeros((int(maxit) + 1, 4)), np.zeros(1, dtype=np.int32)
        self._ck_loop(self.lib.mfh_debug_newmark_pcg(self.h, float(cK), float(cM), float(rtol), int(maxit), ptr(b), ptr(x0), ptr(x), ptr(hist), ptr(its)))
        return x, hist, int(its[0])

    def debug_harmonic_cocg(self, zK, zM, jacobi_cM, f, x0=None, rtol=1e-30, maxit=1):
        """(x, history [maxit + 1, 4], chistory [maxit + 1, 2] complex = {r^T z, p^T Z p}, its) of the COCG of mfh_harmonic on zK K + zM M from x0,
        without its continuations (test hook mfh_debug_harmonic_cocg; M with density 1; jacobi_cM: the block-Jacobi blocks are those of
        K + jacobi_cM M). its as in debug_newmark_pcg."""
        n = self.bs * self.n_dof
        f = np.asarray(f).reshape(-1)
        assert f.size == n and (x0 is None or np.asarray(x0).size == n)
        f_re = np.ascontiguousarray(f.real, dtype=np.float64)
        f_im = np.ascontiguousarray(f.imag, dtype=np.float64) if np.iscomplexobj(f) else None
        x0 = None if x0 is None else np.asarray(x0, dtype=np.complex128).reshape(-1)
        x0_re = None if x0 is None else np.ascontiguousarray(x0.real)
        x0_im = None if x0 is None else np.ascontiguousarray(x0.imag)
        zK, zM = complex(zK), complex(zM)
        zk, zm = np.array([zK.real, zK.imag]), np.array([zM.real, zM.imag])
        xr, xi = np.full(n, np.nan), np.full(n, np.nan)
        hist, chist, its = np.zeros((int(maxit) + 1, 4)), np.zeros((int(maxit) + 1, 4)), np.zeros(1, dtype=np.int32)
        self._ck_loop(self.lib.mfh_debug_harmonic_cocg(self.h, ptr(zk), ptr(zm), float(jacobi_cM), float(rtol), int(maxit), ptr(f_re), ptr(f_im), ptr(x0_re),
                                                       ptr(x0_im), ptr(xr), ptr(xi), ptr(hist), ptr(chist), ptr(its)))
        return xr + 1j * xi, hist, chist[:, 0::2] + 1j * chist[:, 1::2], int(its[0])

    LOBPCG_PENCILS = {"vibration": 0, "buckling": 1, "prestressed": 2}

    def debug_lobpcg_block_size(self, pencil, nev, free_body=False, nq=0):
        """the block size m of the LOBPCG loop for nev modes on this context (test hook mfh_debug_lobpcg without a start block)"""
        m = np.zeros(1, dtype=np.int32)
        self._ck(self.lib.mfh_debug_lobpcg(self.h, self.LOBPCG_PENCILS[pencil], 1.0, 0.0, 1 if free_body else 0, int(nev), 1.0, 0, 0, None, int(nq), None,
                                           ptr(m), None, None, None, None, None, None))
        return int(m[0])

    def debug_lobpcg(self, pencil, S0, nev, density=1.0, load_factor=0.0, free_body=False, rtol=1e-30, maxit=1, Q=None):
        """The block LOBPCG loop of modes / modes_many / buckling / modes_prestressed itself from the start block S0 [m, n] (test hook
        mfh_debug_lobpcg; pencil: "vibration" | "buckling" | "prestressed"; Q [nq, n]: a B-orthonormal deflation set). A dict: X [m, n] the whole
        block as the loop left it; lam, res [maxit + 1, m] and sets [maxit + 1, 3] = {|W|, |P|, restarts} per convergence check (NaN / -1 past a
        stop); iterations (-1 at maxit); precondUsed; m."""
        n = self.bs * self.n_dof
        S0 = np.ascontiguousarray(S0, dtype=np.float64)
        assert S0.ndim == 2 and S0.shape[1] == n
        m = S0.shape[0]
        nq = 0
        if Q is not None:
            Q = np.ascontiguousarray(Q, dtype=np.float64)
            assert Q.ndim == 2 and Q.shape[1] == n
            nq = Q.shape[0]
        calls = int(maxit) + 1
        X, lam, res = np.full((m, n), np.nan), np.full((calls, m), np.nan), np.full((calls, m), np.nan)
        sets, its, used, bsz = np.full((calls, 3), -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        self._ck_loop(self.lib.mfh_debug_lobpcg(self.h, self.LOBPCG_PENCILS[pencil], float(density), float(load_factor), 1 if free_body else 0, int(nev),
                                                float(rtol), int(maxit), m, ptr(S0), nq, ptr(Q), ptr(bsz), ptr(X), ptr(lam), ptr(res), ptr(sets), ptr(its),
                                                ptr(used)))
        return {"X": X, "lam": lam, "res": res, "sets": sets, "iterations": int(its[0]), "precondUsed": int(used[0]), "m": int(bsz[0])}

    def debug_sym_gen_eig(self, A, B):
        """(w, V) of the dense pencil A v = w B v by the Rayleigh-Ritz routine of mfh_modes (test hook mfh_debug_sym_gen_eig)."""
        A, B = as_f64(A), as_f64(B)
        n = A.shape[0]
        w, V = np.empty(n), np.empty((n, n))
        self._ck(self.lib.mfh_debug_sym_gen_eig(n, ptr(A), ptr(B), ptr(w), ptr(V)))
        return w, V

    def debug_block_gram(self, A, B):
        """A^T B for A [n, p], B [n, q] through k_block_gram (test hook mfh_debug_block_gram)."""
        A, B = np.asfortranarray(A, dtype=np.float64), np.asfortranarray(B, dtype=np.float64)
        n, p, q = A.shape[0], A.shape[1], B.shape[1]
        G = np.empty((p, q))
        self._ck(self.lib.mfh_debug_block_gram(self.h, n, p, q, A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), ptr(G)))
        return G

    def debug_block_update(self, A, Cm):
        """A C for A [n, p], C [p, q] through k_block_update (test hook mfh_debug_block_update)."""
        A, Cm = np.asfortranarray(A, dtype=np.float64), as_f64(Cm)
        n, p, q = A.shape[0], A.shape[1], Cm.shape[1]
        Y = np.empty((n, q), order="F")
        self._ck(self.lib.mfh_debug_block_update(self.h, n, p, q, A.ctypes.data_as(C.c_void_p), ptr(Cm), Y.ctypes.data_as(C.c_void_p)))
        return Y

    def apply_K(self, u):
        u = as_f64(u)
        nr, nc, _ = self.matrix_info() if self._assembled_info() else (self.n_dof, self.n_dof, 0)
        out = np.empty(nr * self.bs)
        self._ck(self.lib.mfh_apply_K(self.h, ptr(u), ptr(out)))
        return out

    def _assembled_info(self):
        a = C.c_int64()
        return self.lib.mfh_matrix_info(self.h, C.byref(a), None, None) == L.OK

    # ---------------------------------------------------------------- Simulator-level helpers
    def bc_clear(self):
        self._ck(self.lib.mfh_bc_clear(self.h))

    def bc_dirichlet_box(self, mn, mx, value, relative=False, components=None):
        mn, mx, value = as_f64(mn), as_f64(mx), as_f64(value)
        mask = (1 << self.dim) - 1 if components is None else sum(1 << c for c in range(self.dim) if components[c])
        self._ck(self.lib.mfh_bc_dirichlet_box(self.h, ptr(mn), ptr(mx), int(relative), ptr(value), mask))

    def bc_neumann_box(self, mn, mx, value, kind=L.NEUMANN_TRACTION, relative=False):
        mn, mx = as_f64(mn), as_f64(mx)
        value = as_f64(np.atleast_1d(value))
        if len(value) < self.dim:
            value = np.concatenate([value, np.zeros(self.dim - len(value))])
        self._ck(self.lib.mfh_bc_neumann_box(self.h, ptr(mn), ptr(mx), int(relative), ptr(value), int(kind)))

    def bc_dirichlet_nodes(self, nodes, values, components=None):
        nodes = as_i64(nodes)
        values = as_f64(np.asarray(values, dtype=np.float64).reshape(len(nodes), self.dim))
        mask = (1 << self.dim) - 1 if components is None else sum(1 << c for c in range(self.dim) if components[c])
        self._ck(self.lib.mfh_bc_dirichlet_nodes(self.h, len(nodes), ptr(nodes), ptr(values), mask))

    def bc_neumann_elements(self, bdry_elems, tractions):
        be = as_i64(bdry_elems)
        t = as_f64(np.asarray(tractions, dtype=np.float64).reshape(len(be), self.dim))
        self._ck(self.lib.mfh_bc_neumann_elements(self.h, len(be), ptr(be), ptr(t)))

    def bc_delta_force(self, node, force):
        force = as_f64(force)
        self._ck(self.lib.mfh_bc_delta_force(self.h, int(node), ptr(force)))

    def bc_dirichlet_vars(self):
        n = C.c_int64(0)
        self._ck(self.lib.mfh_bc_dirichlet_vars(self.h, None, None, C.byref(n)))
        v, x = np.empty(n.value, np.int64), np.empty(n.value)
        self._ck(self.lib.mfh_bc_dirichlet_vars(self.h, ptr(v), ptr(x), C.byref(n)))
        return v, x

    def pin_node(self):
        n = C.c_int64()
        self._ck(self.lib.mfh_pin_node(self.h, C.byref(n)))
        return n.value

    def neumann_load(self):
        out = np.empty((self.n_dof, self.dim))
        self._ck(self.lib.mfh_neumann_load(self.h, ptr(out)))
        return out

    def constant_strain_load(self, cstrain_flat):
        e = as_f64(cstrain_flat)
        out = np.empty((self.n_dof, self.dim))
        self._ck(self.lib.mfh_constant_strain_load(self.h, ptr(e), ptr(out)))
        return out

    def _load_out(self, out, add):
        if out is None:
            if add:
                raise ValueError("add=True needs the vector to add to (out=...)")
            return np.empty((self.n_dof, self.dim))
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != self.n_dof * self.dim:
            raise ValueError("out: a C-contiguous float64 array of n_dof * dim values")
        return out

    def body_force_load(self, b, density=None, out=None, add=False):
        """Per-DoF load [nDoF, dim] of the body force density * b (mfh_body_force_load): b is one vector (dim,), one vector per element
        (nElem, dim) -- constant on each element -- or a nodal field (nNode, dim) interpolated with the mesh's shape functions; density:
        per element (nElem,) or None (= 1). out: the array to write (add=True: to add to). Gathered per DoF in a fixed order without atomics:
        the same call returns the same bits."""
        b = as_f64(b)
        d = self.dim
        kinds = [k for k, shp in ((L.BODY_CONSTANT, (d,)), (L.BODY_ELEMENT, (self.n_elem, d)), (L.BODY_NODE, (self.n_node, d))) if b.shape == shp]
        if len(kinds) != 1:
            raise ValueError("b of shape %s is %s: expected (dim,), (nElem, dim) or (nNode, dim)%s"
                             % (b.shape, "ambiguous" if kinds else "not a body force",
                                "; nElem == nNode on this mesh, call mfh_body_force_load with the kind" if kinds else ""))
        rho = None
        if density is not None:
            rho = as_f64(density)
            if rho.shape != (self.n_elem,):
                raise ValueError("density: one value per element")
        out = self._load_out(out, add)
        self._ck(self.lib.mfh_body_force_load(self.h, kinds[0], ptr(b), ptr(rho), L.LOAD_ADD if add else 0, ptr(out)))
        return out

    def stress_field_load(self, field, kind="stress", return_stress=False, out=None, add=False):
        """Per-DoF load [nDoF, dim] f_i = sum_e sigma_e . int_e grad phi_i of a per-element symmetric tensor field [nElem, flatLen] (tensor
        shear entries, the layout of average_stress): perElementStressFieldLoad (mfh_stress_field_load). kind "stress": field is sigma_e;
        kind "strain": sigma_e = C_e : field_e, and return_stress=True also returns that array: (load, C : field)."""
        if kind not in ("stress", "strain"):
            raise ValueError('kind: "stress" or "strain"')
        if return_stress and kind != "strain":
            raise ValueError('return_stress goes with kind="strain"')
        f = as_f64(field)
        if f.shape != (self.n_elem, flat_len(self.dim)):
            raise ValueError("field: [nElem, flatLen]")
        out = self._load_out(out, add)
        sig = np.empty_like(f) if return_stress else None
        self._ck(self.lib.mfh_stress_field_load(self.h, L.FIELD_LOAD_STRAIN if kind == "strain" else L.FIELD_LOAD_STRESS, ptr(f), ptr(sig),
                                                L.LOAD_ADD if add else 0, ptr(out)))
        return (out, sig) if return_stress else out

    def sim_solve(self, f=None, use_pin=False, rtol=1e-8, maxit=100000):
        fp = None if f is None else as_f64(f)
        u = np.empty((self.n_node, self.bs))
        info = L.SolveInfo()
        st = self.lib.mfh_sim_solve(self.h, ptr(fp), int(use_pin), ptr(u), float(rtol), int(maxit), C.byref(info))
        self.last_info = info.as_dict()
        self._ck(st)
        return u

    def sim_solve_constrained(self, f=None, flags=0, rigid_motion_rhs=None, rtol=1e-8, maxit=100000):
        """Simulator::solve with the pin / translation / rotation constraints of assembleConstrainedSystem
        (flags: SOLVE_PIN | SOLVE_NO_RIGID_MOTION | SOLVE_ALLOW_ILL_POSED; 0 = posedness analysis)."""
        fp = None if f is None else as_f64(f)
        rr = None if rigid_motion_rhs is None else as_f64(rigid_motion_rhs)
        u = np.empty((self.n_node, self.bs))
        info = L.SolveInfo()
        st = self.lib.mfh_sim_solve_constrained(self.h, ptr(fp), int(flags), ptr(rr), 0 if rr is None else len(rr), ptr(u),
                                                float(rtol), int(maxit), C.byref(info))
        self.last_info = info.as_dict()
        self._ck(st)
        return u

    def sim_solve_batch(self, f, flags=0, rtol=1e-8, maxit=100000):
        """Simulator::solve for several load vectors (rows of f, dim*nDoF each) on one constrained system: returns (u [nrhs, nNode, dim],
        [info per load]). Positive definite systems go through the batches of mfh_solve_batch (the multigrid V-cycle's coarse levels serve the
        whole batch), systems with constraint rows are solved one load after the other."""
        f = as_f64(f)
        n = self.bs * self.n_dof
        nrhs = f.size // n
        assert f.size == nrhs * n
        u = np.empty((nrhs, self.n_node, self.bs))
        infos = (L.SolveInfo * nrhs)()
        st = self.lib.mfh_sim_solve_batch(self.h, nrhs, ptr(f), int(flags), ptr(u), float(rtol), int(maxit), infos)
        self.last_infos = [i.as_dict() for i in infos]
        self.last_info = self.last_infos[-1]
        self._ck(st)
        return u, self.last_infos

    def solve_cell_problems(self, cstrains, flags=0, rtol=1e-8, maxit=100000):
        """w[k] = Simulator::solve(constantStrainLoad(cstrains[k])) for every row of cstrains (flattened, tensor shear) on the constrained system
        of the context (mfh_solve_cell_problems): returns (w [nStrains, nNode, dim], [info per strain])."""
        cs = as_f64(cstrains)
        fl = self.dim * (self.dim + 1) // 2
        ns = cs.size // fl
        assert cs.size == ns * fl
        w = np.empty((ns, self.n_node, self.bs))
        infos = (L.SolveInfo * ns)()
        st = self.lib.mfh_solve_cell_problems(self.h, ns, ptr(cs), int(flags), ptr(w), float(rtol), int(maxit), infos)
        self.last_infos = [i.as_dict() for i in infos]
        self.last_info = self.last_infos[-1]
        self._ck(st)
        return w, self.last_infos

    def average_strain(self, u_nodes):
        u = as_f64(u_nodes)
        out = np.empty((self.n_elem, flat_len(self.dim)))
        self._ck(self.lib.mfh_average_strain(self.h, ptr(u), ptr(out)))
        return out

    def strain_field(self, u_nodes, stress=False):
        """per-element strain (stress) interpolant values: [nElem, 1 | dim+1, flatLen]"""
        u = as_f64(u_nodes)
        out = np.empty((self.n_elem, 1 if self.deg == 1 else self.dim + 1, flat_len(self.dim)))
        self._ck(self.lib.mfh_strain_field(self.h, ptr(u), int(bool(stress)), ptr(out)))
        return out

    def boundary_strain_field(self, u_nodes, stress=False):
        """the parent element's strain (stress) interpolant at the corners of every boundary element: [nBE, 1 | dim, flatLen]"""
        u = as_f64(u_nodes)
        out = np.empty((self.n_bdry_elem, 1 if self.deg == 1 else self.dim, flat_len(self.dim)))
        self._ck(self.lib.mfh_boundary_strain_field(self.h, ptr(u), int(bool(stress)), ptr(out)))
        return out

    # ---------------------------------------------------------------- stress measures (VonMises.hh, SymmetricMatrix.hh, FieldPostProcessing.hh)
    def _nq(self):
        return 1 if self.deg == 1 else self.dim + 1

    def stress_measures(self, u_nodes, what, stress=True):
        """The requested measures (mask of MEASURE_*) of the stress (strain) of u at the corners of strain_field, fused on the device:
        (von Mises [nElem, NQ], eigenvalues [nElem, NQ, dim] ascending, eigenvectors [nElem, NQ, dim, dim] in columns); None where not requested."""
        u = as_f64(u_nodes)
        n, d = (self.n_elem, self._nq()), self.dim
        vm = np.empty(n) if what & L.MEASURE_VON_MISES else None
        ev = np.empty(n + (d,)) if what & L.MEASURE_EIGENVALUES else None
        vec = np.empty(n + (d, d)) if what & L.MEASURE_EIGENVECTORS else None
        self._ck(self.lib.mfh_stress_measures(self.h, ptr(u), int(bool(stress)), int(what), ptr(vm), ptr(ev), ptr(vec), 0))
        return vm, ev, vec

    def von_mises(self, u_nodes, stress=True):
        """von Mises value of the stress (strain) of u per element corner: [nElem, 1 | dim+1]"""
        return self.stress_measures(u_nodes, L.MEASURE_VON_MISES, stress)[0]

    def principal_values(self, u_nodes, stress=True, vectors=False):
        """Ascending principal stresses (strains) per element corner [nElem, NQ, dim]; with vectors=True also the principal directions
        [nElem, NQ, dim, dim], direction k in column k."""
        _, ev, vec = self.stress_measures(u_nodes, L.MEASURE_EIGENVALUES | (L.MEASURE_EIGENVECTORS if vectors else 0), stress)
        return (ev, vec) if vectors else ev

    def vertex_averaged_field(self, field):
        """C0 volume-weighted vertex average (vertexAveragedField) of element values laid out like strain_field's result: [nElem, NQ, ...]
        with the corner axis NQ = dim+1, or NQ = 1 for a per-element constant that every corner takes ([nElem] is read as [nElem, 1]).
        Any trailing shape (scalar, vector, flattened symmetric, full tensor); returns [nVert, ...]."""
        f = as_f64(field)
        if f.ndim == 1:
            f = f[:, None]
        if f.shape[0] != self.n_elem or f.shape[1] not in (1, self.dim + 1):
            raise ValueError("expected [nElem, 1 | dim+1, ...]")
        per_corner = f.shape[1] == self.dim + 1
        tail = f.shape[2:]
        ncomp = int(np.prod(tail)) if tail else 1
        out = np.empty((self.n_vert,) + tuple(tail))
        self._ck(self.lib.mfh_vertex_average(self.h, ptr(f), int(per_corner), ncomp, ptr(out), 0))
        return out

    def _vertex_averaged_strain(self, u_nodes, stress):
        u = as_f64(u_nodes)
        out = np.empty((self.n_vert, flat_len(self.dim)))
        self._ck(self.lib.mfh_vertex_averaged_strain(self.h, ptr(u), int(stress), ptr(out), 0))
        return out

    def vertex_averaged_stress(self, u_nodes):
        """vertex_averaged_field(strain_field(u, stress=True)) with the corner field kept on the device: [nVert, flatLen]"""
        return self._vertex_averaged_strain(u_nodes, 1)

    def vertex_averaged_strain(self, u_nodes):
        return self._vertex_averaged_strain(u_nodes, 0)

    def peak_von_mises(self, u_nodes, stress=True):
        """(max von Mises value over all element corners, flat corner index element * NQ + corner), reduced on the device. Ties: the
        lowest index; a NaN anywhere: NaN and the index of the first one."""
        u = as_f64(u_nodes)
        v, i = C.c_double(), C.c_int64()
        self._ck(self.lib.mfh_peak_von_mises(self.h, ptr(u), int(bool(stress)), C.byref(v), C.byref(i)))
        return v.value, i.value

    # ---------------------------------------------------------------- field sampler (FieldSampler.hh)
    def _points(self, P):
        P = as_f64(P)
        if P.ndim != 2 or P.shape[1] != self.dim:
            raise ValueError("expected query points [nP, dim]")
        return P

    def sampler_build(self):
        """Build the element grid of the field sampler now (it is otherwise built by the first query)."""
        self._ck(self.lib.mfh_sampler_build(self.h))

    def sampler_info(self):
        """{"elements": {...}, "boundary": {...}} with built, cells (per axis), items, pairs, max_cell_population, build_ms, host_ms of each grid."""
        st = L.SamplerStats()
        self._ck(self.lib.mfh_sampler_info(self.h, C.byref(st)))
        return {name: {"built": bool(g.built), "cells": [int(x) for x in g.cells], "items": int(g.items), "pairs": int(g.pairs),
                       "max_cell_population": int(g.max_cell_population), "build_ms": float(g.build_ms), "host_ms": float(g.host_ms)}
                for name, g in (("elements", st.elements), ("boundary", st.boundary))}

    def locate(self, P):
        """(I [nP] int32, B [nP, dim+1], C [nP, dim], sqDist [nP]) of the query points P [nP, dim]: the lowest-index element containing the point
        (min lambda >= -1e-12) with its barycentric coordinates, C = P and sqDist = 0; for a point outside the mesh the parent element of the
        closest boundary element, the coordinates of the closest point C in it and |P - C|^2. NaN / infinite points: I = -1 and NaN."""
        P = self._points(P)
        n = len(P)
        I, B, Cl, d2 = np.empty(n, dtype=np.int32), np.empty((n, self.dim + 1)), np.empty((n, self.dim)), np.empty(n)
        self._ck(self.lib.mfh_locate(self.h, n, ptr(P), ptr(I), ptr(B), ptr(Cl), ptr(d2), 0))
        return I, B, Cl, d2

    def contains(self, P, eps=1e-10):
        """FieldSampler::contains: squared distance to the mesh <= eps^2"""
        P = self._points(P)
        d2 = np.empty(len(P))
        self._ck(self.lib.mfh_locate(self.h, len(P), ptr(P), None, None, None, ptr(d2), 0))
        return d2 <= eps * eps

    def sample(self, P, field_values):
        """The field at the points P (at their closest points of the mesh where they lie outside). field_values has one row per vertex, per
        element or per node -- detected from the row count in that order, like the reference -- and any number of components per row."""
        P = self._points(P)
        f = as_f64(field_values)
        rows = f.shape[0] if f.ndim else 0
        if rows == self.n_vert:
            kind = L.FIELD_PER_VERTEX
        elif rows == self.n_elem:
            kind = L.FIELD_PER_ELEMENT
        elif rows == self.n_node:
            kind = L.FIELD_PER_NODE
        else:
            raise ValueError("Invalid fieldValues size")
        tail = f.shape[1:]
        ncomp = int(np.prod(tail)) if tail else 1
        out = np.empty((len(P),) + tuple(tail))
        self._ck(self.lib.mfh_sample_field(self.h, len(P), ptr(P), kind, ptr(f), ncomp, ptr(out), 0))
        return out

    def closest_node(self, P):
        """(NI [nP] int32, sqDist [nP]): the node of the located element whose shape function is largest at the point, and its squared
        distance to the query point (closestNodeAndSqDist)"""
        P = self._points(P)
        NI, d2 = np.empty(len(P), dtype=np.int32), np.empty(len(P))
        self._ck(self.lib.mfh_closest_node(self.h, len(P), ptr(P), ptr(NI), ptr(d2), 0))
        return NI, d2

    def average_stress(self, u_nodes):
        u = as_f64(u_nodes)
        out = np.empty((self.n_elem, flat_len(self.dim)))
        self._ck(self.lib.mfh_average_stress(self.h, ptr(u), ptr(out)))
        return out

    def integrated_stress(self, u_nodes, cstrain_flat=None):
        """sum_e vol_e C_e : (average strain_e(u) + cstrain) reduced on the device (flatLen values): the element loop of
        homogenizedElasticityTensor (PeriodicHomogenization.hh:72-100) without a per-element field on the host."""
        u = as_f64(u_nodes)
        cs = None if cstrain_flat is None else as_f64(cstrain_flat)
        out = np.empty(flat_len(self.dim))
        self._ck(self.lib.mfh_integrated_stress(self.h, ptr(u), None if cs is None else ptr(cs), ptr(out)))
        return out

    # ---------------------------------------------------------------- discrete shape derivatives (forward mode)
    def _delta_p(self, delta_p):
        dp = as_f64(delta_p)
        if dp.size != self.n_vert * self.dim:
            raise ValueError("deltaP must be a per-vertex field [nVert x dim]")
        return dp

    def apply_delta_K(self, u_nodes, delta_p):
        """(delta K) u for a per-node field u under the vertex perturbation delta_p; per-DoF result."""
        u, dp = as_f64(u_nodes), self._delta_p(delta_p)
        out = np.empty((self.n_dof, self.dim))
        self._ck(self.lib.mfh_apply_delta_K(self.h, ptr(u), ptr(dp), ptr(out)))
        return out

    def delta_constant_strain_load(self, cstrain_flat, delta_p):
        e, dp = as_f64(cstrain_flat), self._delta_p(delta_p)
        out = np.empty((self.n_dof, self.dim))
        self._ck(self.lib.mfh_delta_constant_strain_load(self.h, ptr(e), ptr(dp), ptr(out)))
        return out

    def delta_average_strain(self, u_nodes, delta_u, delta_p, stress=False):
        u, du, dp = as_f64(u_nodes), as_f64(delta_u), self._delta_p(delta_p)
        out = np.empty((self.n_elem, flat_len(self.dim)))
        self._ck(self.lib.mfh_delta_average_strain(self.h, ptr(u), ptr(du), ptr(dp), int(bool(stress)), ptr(out)))
        return out

    def mutual_energies(self, w, delta_p=None):
        """flatLen x flatLen matrix of sum_e int (e^ij + eps(w^ij)) : C : (e^kl + eps(w^kl)) dV, or its discrete shape
        derivative under delta_p. w: flatLen per-node fields."""
        fl = flat_len(self.dim)
        wa = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64).reshape(self.n_node, self.dim) for x in w]))
        if wa.shape[0] != fl:
            raise ValueError("need one fluctuation displacement per canonical strain")
        dp = None if delta_p is None else self._delta_p(delta_p)
        out = np.empty((fl, fl))
        self._ck(self.lib.mfh_mutual_energies(self.h, ptr(wa), ptr(dp), ptr(out)))
        return out

    def mutual_energy_differential(self, w):
        """d(mutual energies)/d(vertex positions): [nPairs, nVert, dim], pairs = upper triangle ij <= kl row-major."""
        fl = flat_len(self.dim)
        wa = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64).reshape(self.n_node, self.dim) for x in w]))
        if wa.shape[0] != fl:
            raise ValueError("need one fluctuation displacement per canonical strain")
        out = np.empty((fl * (fl + 1) // 2, self.n_vert, self.dim))
        self._ck(self.lib.mfh_mutual_energy_differential(self.h, ptr(wa), ptr(out)))
        return out

    # ---------------------------------------------------------------- device pointers (torch interop)
    def stream(self):
        return self.lib.mfh_stream(self.h)

    def set_stream(self, hip_stream):
        """Adopt a caller-owned hipStream_t (int handle, e.g. torch.cuda.current_stream().cuda_stream)."""
        self._ck(self.lib.mfh_set_stream(self.h, C.c_void_p(hip_stream)))

    def dev_spmv(self, x_ptr, y_ptr):
        self._ck(self.lib.mfh_dev_spmv(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr)))

    def dev_precond(self, r_ptr, z_ptr):
        self._ck(self.lib.mfh_dev_precond(self.h, C.c_void_p(r_ptr), C.c_void_p(z_ptr)))

    def tl_partitioned_begin(self, n_agg, agg_of_node, rel_pos, ac_ptr):
        """Caller-supplied (global) aggregates: this context's Galerkin contribution into the device
        buffer at ac_ptr ((n_agg*modes)^2 doubles)."""
        agg = np.ascontiguousarray(agg_of_node, dtype=np.int32)
        rp = np.ascontiguousarray(rel_pos, dtype=np.float64)
        n_local = self.matrix_info()[1]
        if agg.shape != (n_local,) or rp.shape != (n_local, 3):
            raise ValueError("agg_of_node / rel_pos must cover every local node")
        self._ck(self.lib.mfh_tl_partitioned_begin(self.h, int(n_agg), agg.ctypes.data_as(C.c_void_p),
                                                   rp.ctypes.data_as(C.c_void_p), C.c_void_p(ac_ptr)))

    def tl_partitioned_finish(self, ac_ptr):
        self._ck(self.lib.mfh_tl_partitioned_finish(self.h, C.c_void_p(ac_ptr)))

    def dev_tl_restrict(self, r_ptr, rc_ptr):
        self._ck(self.lib.mfh_dev_tl_restrict(self.h, C.c_void_p(r_ptr), C.c_void_p(rc_ptr)))

    def dev_tl_apply(self, r_ptr, rc_ptr, z_ptr):
        self._ck(self.lib.mfh_dev_tl_apply(self.h, C.c_void_p(r_ptr), C.c_void_p(rc_ptr), C.c_void_p(z_ptr)))

    def dev_pcg_update_xr(self, num_ptr, den_ptr, p_ptr, ap_ptr, x_ptr, r_ptr):
        self._ck(self.lib.mfh_dev_pcg_update_xr(self.h, *[C.c_void_p(q) for q in (num_ptr, den_ptr, p_ptr, ap_ptr, x_ptr, r_ptr)]))

    def dev_pcg_direction(self, num_ptr, den_ptr, z_ptr, p_ptr):
        self._ck(self.lib.mfh_dev_pcg_direction(self.h, *[C.c_void_p(q) for q in (num_ptr, den_ptr, z_ptr, p_ptr)]))

    def dev_dots(self, r_ptr, z_ptr, out_ptr):
        self._ck(self.lib.mfh_dev_dots(self.h, C.c_void_p(r_ptr), C.c_void_p(z_ptr), C.c_void_p(out_ptr)))

    def dev_mask_fixed(self, r_ptr):
        self._ck(self.lib.mfh_dev_mask_fixed(self.h, C.c_void_p(r_ptr)))

    def dev_set_fixed_values(self, u_ptr):
        self._ck(self.lib.mfh_dev_set_fixed_values(self.h, C.c_void_p(u_ptr)))

    # ---- row-partitioned solve through an mfh_comm
    def dist_setup(self, comm, peers, send_ptr, send_nodes, recv_ptr):
        peers, send_ptr, send_nodes, recv_ptr = as_i32(peers), as_i64(send_ptr), as_i32(send_nodes), as_i64(recv_ptr)
        self._ck(self.lib.mfh_dist_setup(self.h, comm.h, len(peers), ptr(peers), ptr(send_ptr), ptr(send_nodes), ptr(recv_ptr)))
        self._comm = comm          # keep the communicator (and its callbacks) alive as long as the context uses it

    def dist_two_level(self, n_agg, agg_of_node, rel_pos):
        agg_of_node, rel_pos = as_i32(agg_of_node), as_f64(rel_pos)
        self._ck(self.lib.mfh_dist_two_level(self.h, int(n_agg), ptr(agg_of_node), ptr(rel_pos)))

    def dist_solve(self, f_owned, rtol=1e-8, maxit=100000):
        """f_owned: [nrhs, dim * nOwned] (or flat for one right-hand side); returns (u_owned, [info per rhs])."""
        f = as_f64(f_owned)
        self.symbolic(False)                       # (the row count comes from the pattern; a no-op once it exists)
        nr, _, _ = self.matrix_info()
        n = self.bs * nr
        nrhs = f.size // n
        assert f.size == nrhs * n
        u = np.empty((nrhs, n))
        infos = (L.SolveInfo * nrhs)()
        st = self.lib.mfh_dist_solve(self.h, nrhs, ptr(f), ptr(u), float(rtol), int(maxit), infos)
        self.last_infos = [i.as_dict() for i in infos]
        self.last_info = self.last_infos[-1]
        self._ck(st)
        return u, self.last_infos

    def dist_apply_K(self, u_owned):
        u = as_f64(u_owned)
        out = np.empty_like(u)
        self._ck(self.lib.mfh_dist_apply_K(self.h, ptr(u), ptr(out)))
        return out

    def dist_stats(self):
        st = L.DistStats()
        self._ck(self.lib.mfh_dist_get_stats(self.h, C.byref(st)))
        return st.as_dict()

    def dev_memcpy(self, dst, src, nbytes, kind, stream=None):
        self._ck(self.lib.mfh_dev_memcpy(self.h, dst, src, int(nbytes), int(kind), stream))

    def dev_sync(self):
        self._ck(self.lib.mfh_dev_sync(self.h))

    # ---------------------------------------------------------------- measurement
    def timing(self):
        t = L.Timing()
        self._ck(self.lib.mfh_get_timing(self.h, C.byref(t)))
        return t.as_dict()

    def time_assembly_kernel(self, mode=L.ASSEMBLE_GATHER, reps=5):
        v = C.c_double()
        self._ck(self.lib.mfh_time_assembly_kernel(self.h, int(mode), int(reps), C.byref(v)))
        return v.value

    def time_spmv_kernel(self, reps=10):
        v = C.c_double()
        self._ck(self.lib.mfh_time_spmv_kernel(self.h, int(reps), C.byref(v)))
        return v.value

    def time_block_gram(self, n, p, q, reps=10):
        """(gram_ms, copy_ms): k_block_gram on n x p, n x q blocks against a device-to-device copy of the same bytes (mfh_time_block_gram)."""
        g, cp = C.c_double(), C.c_double()
        self._ck(self.lib.mfh_time_block_gram(self.h, int(n), int(p), int(q), int(reps), C.byref(g), C.byref(cp)))
        return g.value, cp.value

    def debug_deflate(self, BQ, Q, V, cols=None):
        """(G, Vout): G = BQ^T V[:, cols] through k_deflate_gram, Vout = V with V[:, cols] - Q G in the listed columns through k_deflate_update
        (test hook mfh_debug_deflate). BQ, Q [n, nq], V [n, nv <= 24]; cols: distinct columns of V (None: all)."""
        BQ, Q, V = (np.asfortranarray(a, dtype=np.float64) for a in (BQ, Q, V))
        n, nq, nv = V.shape[0], Q.shape[1], V.shape[1]
        if BQ.shape != Q.shape or Q.shape[0] != n:
            raise ValueError("debug_deflate: BQ and Q need the shape [n, nq], V [n, nv]")
        cols = np.ascontiguousarray(np.arange(nv) if cols is None else cols, dtype=np.int32)
        G, Vout = np.empty((nq, len(cols))), np.empty((n, nv), order="F")
        self._ck(self.lib.mfh_debug_deflate(self.h, n, nq, nv, len(cols), cols.ctypes.data_as(C.c_void_p), BQ.ctypes.data_as(C.c_void_p),
                                            Q.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), ptr(G), Vout.ctypes.data_as(C.c_void_p)))
        return G, Vout

    def time_deflate(self, n, nq, k, reps=10):
        """(gram_ms, update_ms, copy_ms): k_deflate_gram and k_deflate_update on nq + k columns of n rows against a device-to-device copy of the
        same columns (mfh_time_deflate)."""
        g, u, cp = C.c_double(), C.c_double(), C.c_double()
        self._ck(self.lib.mfh_time_deflate(self.h, int(n), int(nq), int(k), int(reps), C.byref(g), C.byref(u), C.byref(cp)))
        return g.value, u.value, cp.value

    def time_kron_pair(self, reps=40):
        """(pair_ms, separate_ms): one pair product of the prestressed loop as k_spmv_kron_pair and as the two launches it replaces (mfh_time_kron_pair)."""
        a, b = C.c_double(), C.c_double()
        self._ck(self.lib.mfh_time_kron_pair(self.h, int(reps), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_option(self, key, value):
        self._ck(self.lib.mfh_set_option(self.h, key.encode(), float(value)))

    def get_option(self, key):
        """The current value of option `key` of this context (0.0 / 1.0 for the on-off options)."""
        v = C.c_double()
        self._ck(self.lib.mfh_get_option(self.h, key.encode(), C.byref(v)))
        return v.value


def sym_measures(field, what, ctx=None):
    """Measures (mask of MEASURE_*) of a field of flattened symmetric matrices [..., flatLen] (tensor shear; flatLen 3: 2D, 6: 3D) on the
    device of `ctx` (default: a context of its own on device 0): (von Mises [...], eigenvalues [..., dim], eigenvectors [..., dim, dim])."""
    f = as_f64(field)
    dim = {3: 2, 6: 3}.get(f.shape[-1] if f.ndim else 0)
    if dim is None:
        raise ValueError("the last axis must hold 3 (2D) or 6 (3D) flattened entries")
    own = ctx is None
    c = Context(0) if own else ctx
    try:
        lead = f.shape[:-1]
        n = int(np.prod(lead)) if lead else 1
        vm = np.empty(lead) if what & L.MEASURE_VON_MISES else None
        ev = np.empty(lead + (dim,)) if what & L.MEASURE_EIGENVALUES else None
        vec = np.empty(lead + (dim, dim)) if what & L.MEASURE_EIGENVECTORS else None
        c._ck(c.lib.mfh_sym_measures(c.h, dim, n, ptr(f), int(what), ptr(vm), ptr(ev), ptr(vec), 0))
    finally:
        if own:
            c.close()
    return vm, ev, vec


def von_mises(field, ctx=None):
    """vonMises(field) of the reference as the scalar per matrix (VonMises.hh)"""
    return sym_measures(field, L.MEASURE_VON_MISES, ctx)[0]


def principal_values(field, vectors=False, ctx=None):
    """eigenvalues (ascending) and, with vectors=True, eigenvectors in columns (SymmetricMatrix.hh eigenDecomposition)"""
    _, ev, vec = sym_measures(field, L.MEASURE_EIGENVALUES | (L.MEASURE_EIGENVECTORS if vectors else 0), ctx)
    return (ev, vec) if vectors else ev


def vertex_averaged_field(ctx, field):
    """vertexAveragedField(mesh, f) on the mesh of `ctx`"""
    return ctx.vertex_averaged_field(field)


def device_cache_trim():
    """Return every cached device block of this process to the driver (mfh_device_cache_trim)."""
    L.load().mfh_device_cache_trim()


def device_cache_stats(device=0):
    lib = L.load()
    v = [C.c_int64() for _ in range(5)]
    lib.mfh_device_cache_stats(int(device), *[C.byref(x) for x in v])
    return dict(zip(("cached_bytes", "blocks", "hits", "misses", "flushes"), [x.value for x in v]))


def device_reserve(nbytes, device=0, wait=False):
    """One free segment of `nbytes` for the library's device arena, taken from the driver now (mfh_device_reserve) -- on a thread of its own
    unless `wait`: call it before reading / generating the mesh."""
    st = L.load().mfh_device_reserve(int(device), int(nbytes), 0 if wait else 1)
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_device_reserve failed")


def device_reserve_for(dim, deg, n_elem, device=0, wait=False):
    """mfh_device_reserve_for: the reservation for a context on a mesh of n_elem simplices of that kind -- the value array of K in a segment of
    its own, the rest in another. Returns the estimated total (bytes)."""
    lib = L.load()
    st = lib.mfh_device_reserve_for(int(device), int(dim), int(deg), int(n_elem), 0 if wait else 1)
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_device_reserve_for failed")
    return context_bytes_estimate(dim, deg, n_elem)[0]


def context_bytes_estimate(dim, deg, n_elem):
    """(total bytes, bytes of K's value array) a context on such a mesh holds at its peak (mfh_context_bytes_estimate)."""
    t, v = C.c_int64(), C.c_int64()
    st = L.load().mfh_context_bytes_estimate(int(dim), int(deg), int(n_elem), C.byref(t), C.byref(v))
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_context_bytes_estimate failed")
    return t.value, v.value


def device_arena_stats(device=0):
    """State of the library's device arena (mfh_device_arena_stats): bytes held / live / live high-water mark, segments, free chunks, ..."""
    lib = L.load()
    v = (C.c_int64 * 8)()
    lib.mfh_device_arena_stats(int(device), v)
    return dict(zip(("held_bytes", "live_bytes", "live_high_water_bytes", "segments", "free_chunks", "returned_to_driver_bytes",
                     "quarantined_bytes", "free_bound_bytes"), list(v)))


def modal_transient_coeffs(lam, c, dt):
    """The eight coefficients {A11, A12, b0_q, b1_q, A21, A22, b0_v, b1_v} of the exact step of q'' + c q' + lam q = a(t), a piecewise linear
    (mfh_modal_transient_coeffs; host only, no device): one row of eight per entry of the broadcast (lam, c), a single row for scalars."""
    lam_b, c_b = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.zeros(lam_b.shape + (8,))
    flat = out.reshape(-1, 8)
    lib = L.load()
    for i, (l, cc) in enumerate(zip(lam_b.reshape(-1), c_b.reshape(-1))):
        row = np.zeros(8)
        st = lib.mfh_modal_transient_coeffs(float(l), float(cc), float(dt), ptr(row))
        if st != L.OK:
            raise L.MeshFEMHipError(st, "mfh_modal_transient_coeffs: lam >= 0, c >= 0, dt > 0, all finite")
        flat[i] = row
    return out


def psd_factor(Cm, tol=-1.0):
    """(F [n, rank], piv [rank], truncation): the diagonally pivoted Cholesky factor C ~ F F^T of a symmetric positive semi-definite matrix (mfh_psd_factor;
    host only, no device; n <= 258; symmetry from the lower triangle). It stops when the largest remaining diagonal is <= tol (tol < 0: n eps max diag);
    truncation = the trace of the remainder. Rows keep their places: F[piv[s], t] == 0 for t > s. Raises with code ERR_INVALID for a matrix that is not
    positive semi-definite or not finite."""
    Cm = as_f64(np.atleast_2d(np.asarray(Cm, dtype=np.float64)))
    n = Cm.shape[0]
    if Cm.shape != (n, n):
        raise ValueError("psd_factor: a square matrix is needed, got %s" % (Cm.shape,))
    F, piv = np.zeros((n, n)), np.zeros(n, dtype=np.int32)
    rank, trunc = C.c_int32(), C.c_double()
    st = L.load().mfh_psd_factor(n, ptr(Cm), float(tol), ptr(F), C.byref(rank), ptr(piv), C.byref(trunc))
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_psd_factor: n <= 258, finite entries, a positive semi-definite matrix (no remaining diagonal below -tol)")
    return np.ascontiguousarray(F[:, :rank.value]), piv[:rank.value].copy(), trunc.value


def modal_covariance(lam, g, omega, S, weights=None, damping=(0.0, 0.0), loss_factor=0.0, modal_damping=None, correction=False):
    """[3, nb, nb]: the modal covariances C^(p) = sum_k w_k omega_k^p Re(H_k S_k H_k^H), p = 0, 2, 4 (mfh_modal_covariance; host only, no device).
    lam [m], g [m] or [m, nLoad] = Phi^T f_a, omega [nFreq] strictly ascending, S [nFreq] or [nFreq, nLoad, nLoad] Hermitian, weights [nFreq] or None
    (trapezoid). correction: nb = m + nLoad, the rows of the static-correction columns appended (nLoad <= 2)."""
    lam = as_f64(np.asarray(lam, dtype=np.float64).reshape(-1))
    m = lam.size
    g = as_f64(np.asarray(g, dtype=np.float64).reshape(m, -1))
    nl = g.shape[1]
    om = as_f64(np.asarray(omega, dtype=np.float64).reshape(-1))
    nf = om.size
    Sc = np.asarray(S, dtype=np.complex128)
    if Sc.ndim == 1:
        Sc = Sc.reshape(-1, 1, 1)
    if Sc.shape != (nf, nl, nl):
        raise ValueError("modal_covariance: S needs the shape [nFreq, nLoad, nLoad] = %s, got %s" % ((nf, nl, nl), Sc.shape))
    Sri = np.ascontiguousarray(np.stack([Sc.real, Sc.imag], axis=-1))
    w = None if weights is None else as_f64(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w is not None and w.size != nf:
        raise ValueError("modal_covariance: %d weights for %d frequencies" % (w.size, nf))
    zeta = _modal_zeta(modal_damping, m)
    nb = m + (nl if correction else 0)
    out = np.zeros((3, nb, nb))
    st = L.load().mfh_modal_covariance(m, ptr(lam), ptr(g), nl, float(damping[0]), float(damping[1]), float(loss_factor), ptr(zeta), nf, ptr(om), ptr(w), ptr(Sri),
                                       int(bool(correction)), ptr(out[0]), ptr(out[1]), ptr(out[2]))
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_modal_covariance: refused (a grid that is not strictly ascending or negative, omega = 0 with a zero eigenvalue, "
                                    "d_j = 0, a spectrum that is not Hermitian or has a negative diagonal, an entry that is not finite, more than two loads "
                                    "with the correction)")
    return out


def cqc_matrix(lam, zeta):
    """[m, m]: the correlation coefficients of the CQC rule for modes of eigenvalues lam and damping ratios zeta > 0 (a scalar or one per mode), Der
    Kiureghian's form for unequal damping (mfh_cqc_matrix; host only)."""
    lam = as_f64(np.asarray(lam, dtype=np.float64).reshape(-1))
    m = lam.size
    z = as_f64(np.broadcast_to(np.asarray(zeta, dtype=np.float64), (m,)))
    rho = np.zeros((m, m))
    st = L.load().mfh_cqc_matrix(m, ptr(lam), ptr(z), ptr(rho))
    if st != L.OK:
        raise L.MeshFEMHipError(st, "mfh_cqc_matrix: lam >= 0, zeta > 0, finite, at most 258 modes")
    return rho


def resonance_grid(lam, zeta, band, per_halfpower=8, background=64):
    """An ascending frequency grid on band = (w_lo, w_hi) for the spectra of lightly damped modes: `background` equal intervals over the band, merged,
    for every mode with sqrt(lam_j) inside the band, with points h_j = 2 zeta_j sqrt(lam_j) / per_halfpower apart (the half-power bandwidth divided by
    per_halfpower) over four bandwidths either side of sqrt(lam_j), and beyond them with spacings that grow by the factor 1 + 1 / per_halfpower per
    point out to the band's ends. Every spacing of a mode's points is proportional to 1 / per_halfpower, so the trapezoid rule on the grid is second
    order in it."""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    z = np.broadcast_to(np.asarray(zeta, dtype=np.float64), lam.shape)
    lo, hi = float(band[0]), float(band[1])
    p = int(per_halfpower)
    if not (hi > lo >= 0.0) or p < 1 or background < 1:
        raise ValueError("resonance_grid: band = (lo, hi) with 0 <= lo < hi, per_halfpower >= 1, background >= 1")
    parts = [np.linspace(lo, hi, int(background) + 1)]
    for l, zj in zip(lam, z):
        wn = np.sqrt(l)
        if not (lo <= wn <= hi) or not zj > 0.0 or not wn > 0.0:
            continue
        h = 2.0 * zj * wn / p
        core = wn + h * np.arange(-4 * p, 4 * p + 1)
        count = int(np.ceil(np.log(max((hi - lo) / h, 2.0)) / np.log1p(1.0 / p))) + 1
        steps = np.cumsum(h * (1.0 + 1.0 / p) ** np.arange(1, count + 1))
        parts += [core, core[-1] + steps, core[0] - steps]
    grid = np.unique(np.concatenate(parts))
    return grid[(grid >= lo) & (grid <= hi)]
