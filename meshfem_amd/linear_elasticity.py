"""`LinearElasticity.Simulator` with the reference's method names
(src/lib/MeshFEM/LinearElasticity.hh:434-1659) on top of the C ABI. Every numeric step runs in
libmeshfem_hip.so on the GPU; this class only forwards."""
import numpy as np

from . import _lib as L
from .core import Context, flat_len


class Simulator:
    def __init__(self, elems, vertices, degree=2, device=0):
        """== Simulator(elems, vertices) (:460-473): builds the FEMMesh, raises on inverted elements."""
        self.ctx = Context(device)
        self.ctx.mesh_build(elems, vertices, degree)
        self.N = self.ctx.dim
        self.degree = degree
        self.rtol, self.maxit = 1e-8, 100000
        self._use_pin = False
        self._no_rigid_motion = False
        self._rigid_motion_rhs = None
        self._bbox = None

    # ---- mesh queries (mesh.cc:47-70)
    def numNodes(self):
        return self.ctx.n_node

    def numElements(self):
        return self.ctx.n_elem

    def numDoFs(self):
        return self.ctx.n_dof

    def nodes(self):
        return self.ctx.node_positions()

    def elements(self):
        return self.ctx.elem_nodes()

    def boundingBox(self):
        """(min corner, max corner) of the mesh (BoundaryConditions.hh:452-470 builds the periodic cell from it); edge nodes are
        midpoints, so the box of the nodes is the box of anything that contains the vertices. Column by column: numpy's axis-0
        reduction of an (n, 3) array is three times slower."""
        if self._bbox is None:
            pos = self.nodes()
            self._bbox = (np.array([pos[:, k].min() for k in range(pos.shape[1])]), np.array([pos[:, k].max() for k in range(pos.shape[1])]))
        return self._bbox

    def updateMeshNodePositions(self, vertices):                        # :1279-1284
        self.ctx.mesh_update_vertices(vertices)
        self._bbox = None

    # ---- materials
    def setMaterial(self, tensor):
        self.ctx.material_const(np.asarray(tensor.D if hasattr(tensor, "D") else tensor))

    def setIsotropicMaterial(self, E, nu):
        self.ctx.material_isotropic(E, nu)

    def setIsotropicField(self, E, nu):
        self.ctx.material_iso_field(E, nu)

    def setOrthotropicField(self, params):
        self.ctx.material_ortho_field(params)

    # ---- boundary conditions (box regions of applyBoundaryConditions, :881-1027)
    def applyDirichletBox(self, mn, mx, value, relative=False, components=None):
        self.ctx.bc_dirichlet_box(mn, mx, value, relative, components)

    def applyNeumannBox(self, mn, mx, value, kind=L.NEUMANN_TRACTION, relative=False):
        self.ctx.bc_neumann_box(mn, mx, value, kind, relative)

    def applyDirichletNodes(self, nodes, values, components=None):      # DirichletNodesCondition, :991-1002
        self.ctx.bc_dirichlet_nodes(nodes, values, components)

    def applyNeumannElements(self, bdry_elems, tractions):             # NeumannElementsCondition, :966-990
        self.ctx.bc_neumann_elements(bdry_elems, tractions)

    def applyPeriodicConditions(self, epsilon=1e-7, ignoreMismatch=False, ignoreDims=()):    # :845-854
        self.ctx.set_option("periodic_ignore_mismatch", 1 if ignoreMismatch else 0)
        self.ctx.set_option("periodic_ignore_dims", sum(1 << int(d) for d in ignoreDims))
        return self.ctx.apply_periodic_conditions(epsilon)

    def removePeriodicConditions(self):                                 # :874-879
        self.ctx.dof_map(None, 0)

    def applyNoRigidMotionConstraint(self):                             # m_useRigidMotionConstraint (:1214-1228)
        self._no_rigid_motion = True

    def removeNoRigidMotionConstraint(self):
        self._no_rigid_motion = False

    def setRigidMotionConstraintRHS(self, rhs):
        self._rigid_motion_rhs = None if rhs is None else np.asarray(rhs, dtype=np.float64)

    def setUsePinNoRigidTranslationConstraint(self, use):               # PeriodicHomogenization.hh:44-45
        self._use_pin = bool(use)

    # ---- loads / solve
    def neumannLoad(self):                                              # :703-717
        return self.ctx.neumann_load()

    def constantStrainLoad(self, cstrain_flat):                         # :551-562
        return self.ctx.constant_strain_load(cstrain_flat)

    def perElementStressFieldLoad(self, stress):                        # :564-577
        """Per-DoF load of a per-element stress field [nElem, flatLen] (tensor shear): f_i = sum_e sigma_e . int_e grad phi_i."""
        return self.ctx.stress_field_load(stress, "stress")

    def perElementStrainFieldLoad(self, strain):
        """perElementStressFieldLoad(C_e : strain_e); with one strain everywhere this is constantStrainLoad."""
        return self.ctx.stress_field_load(strain, "strain")

    def _element_density(self, density):
        rho = np.asarray(density, dtype=np.float64)
        return np.full(self.numElements(), float(rho)) if rho.ndim == 0 else rho

    def bodyForceLoad(self, b, density=None):
        """Per-DoF load of the body force density * b: b one vector (N,), per element (nElem, N) or a nodal field (nNode, N); density per
        element or None (= 1). No counterpart in the reference."""
        return self.ctx.body_force_load(b, density)

    def gravityLoad(self, g, density=1.0):
        """Self-weight: the load of density * g for the acceleration vector g; density a scalar or per element."""
        return self.ctx.body_force_load(np.asarray(g, dtype=np.float64).reshape(self.N), self._element_density(density))

    def centrifugalLoad(self, omega, axis_point, axis_dir, density=1.0):
        """The load of a body spinning at angular velocity omega about the axis through axis_point along axis_dir (2D: about the point, the
        axis is normal to the plane and axis_dir is ignored): density * omega^2 * r_perp(x). The field is linear in x, so its nodal
        interpolation is exact."""
        x = self.nodes() - np.asarray(axis_point, dtype=np.float64).reshape(1, self.N)
        if self.N == 3:
            a = np.asarray(axis_dir, dtype=np.float64).reshape(3)
            a = a / np.linalg.norm(a)
            x = x - np.outer(x @ a, a)
        return self.ctx.body_force_load(np.ascontiguousarray(float(omega) ** 2 * x), self._element_density(density))

    def _thermal_strain(self, alpha, dT):
        a, t = np.asarray(alpha, dtype=np.float64), np.asarray(dT, dtype=np.float64)
        eps = np.zeros((self.numElements(), flat_len(self.N)))
        eps[:, :self.N] = (a * t * np.ones(self.numElements()))[:, None]
        return eps

    def thermalLoad(self, alpha, dT):
        """The load of the thermal strain eps_th = alpha dT I (alpha: scalar or per element, dT: per element or scalar):
        perElementStrainFieldLoad(eps_th); solve() of it gives the displacement of the heated body."""
        return self.ctx.stress_field_load(self._thermal_strain(alpha, dT), "strain")

    def thermalStress(self, u_nodes, alpha, dT):
        """stressField(u) - C : eps_th, the stress in the heated body, with stressField's corner layout [nElem, NQ, flatLen]."""
        _, sig_th = self.ctx.stress_field_load(self._thermal_strain(alpha, dT), "strain", return_stress=True)
        return self.stressField(u_nodes) - sig_th[:, None, :]

    def solve(self, f=None):                                            # :479-487, :657
        f = None if f is None else np.asarray(f, dtype=np.float64).ravel()
        flags = (L.SOLVE_PIN if self._use_pin else 0) | (L.SOLVE_NO_RIGID_MOTION if self._no_rigid_motion else 0)
        u = self.ctx.sim_solve_constrained(f, flags, self._rigid_motion_rhs, rtol=self.rtol, maxit=self.maxit)
        self.info = dict(self.ctx.last_info)
        return u

    def solveMany(self, loads):
        """solve() for several load vectors on the same constrained system (what solveCellProblems does with its constantStrainLoad vectors,
        PeriodicHomogenization.hh:47-53): returns the list of nodal displacement fields; self.infos holds one record per load."""
        F = np.stack([np.asarray(f, dtype=np.float64).ravel() for f in loads])
        flags = (L.SOLVE_PIN if self._use_pin else 0) | (L.SOLVE_NO_RIGID_MOTION if self._no_rigid_motion else 0)
        if self._rigid_motion_rhs is not None:          # (a right-hand side for the constraint rows: one load after the other)
            out, self.infos = [], []
            for f in F:
                out.append(self.solve(f))
                self.infos.append(self.info)
            return out
        u, infos = self.ctx.sim_solve_batch(F, flags, rtol=self.rtol, maxit=self.maxit)
        self.infos = infos
        self.info = dict(infos[-1])
        return [u[k] for k in range(len(F))]

    def solveConstantStrainLoads(self, cstrains):
        """[solve(constantStrainLoad(e)) for e in cstrains] in one call (the loop of solveCellProblems, PeriodicHomogenization.hh:47-53): the load
        vectors never visit the host where the library can form them on the device; self.infos holds one record per strain."""
        if self._rigid_motion_rhs is not None:
            return self.solveMany([self.constantStrainLoad(e) for e in cstrains])
        flags = (L.SOLVE_PIN if self._use_pin else 0) | (L.SOLVE_NO_RIGID_MOTION if self._no_rigid_motion else 0)
        w, infos = self.ctx.solve_cell_problems(np.asarray(cstrains, dtype=np.float64), flags, rtol=self.rtol, maxit=self.maxit)
        self.infos = infos
        self.info = dict(infos[-1])
        return [w[k] for k in range(len(w))]

    def setDensity(self, density):
        """The per-element density [nElem] of the mass matrix of vibrational_modes and transient (None: unit density). Their scalar density=
        multiplies it. It survives vertex updates; a new mesh clears it."""
        self.ctx.set_density(density)

    def _density_scalar(self, density):
        """density= of vibrational_modes / transient: an array of one value per element becomes the context's field and the scalar 1."""
        rho = np.asarray(density, dtype=np.float64)
        if rho.ndim == 0:
            return float(rho)
        if rho.shape != (self.numElements(),):
            raise ValueError("density: a scalar or one value per element")
        self.setDensity(rho)
        return 1.0

    def massProperties(self, density=1.0):
        """{"mass", "com", "second_moment", "inertia"} of the body under the density field of setDensity times the scalar density: the second
        moments int rho (x - com)(x - com)^T and the inertia tensor tr(S) I - S about the centre of mass (2D: the polar moment tr(S))."""
        return self.ctx.mass_properties(density)

    def applyMassMatrix(self, x_dofs):
        """M x on a per-DoF displacement vector [nDoF, N]: the consistent mass matrix with the density field of setDensity."""
        return self.ctx.mass_apply(np.asarray(x_dofs, dtype=np.float64).reshape(self.ctx.n_dof, self.N))

    def modalEffectiveMass(self, X):
        """[nev, N]: (x_j^T M r_d)^2 for the mode shapes x_j -- the nodal fields [nev, nNode, N] of vibrational_modes or per-DoF rows
        [nev, nDoF * N], M-orthonormal -- and the unit translations r_d. Summed over all modes of a body a column gives the mass that moves
        in direction d."""
        ctx = self.ctx
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 3 and X.shape[1] == ctx.n_node and ctx.n_dof != ctx.n_node:     # nodal fields under a DoF map: a DoF takes its first node's value
            dof = ctx.get_dof_map()[0]
            first = np.full(ctx.n_dof, -1, dtype=np.int64)
            first[dof[::-1]] = np.arange(ctx.n_node)[::-1]
            X = X[:, first, :]
        X = X.reshape(len(X), ctx.n_dof * self.N)
        out = np.empty((len(X), self.N))
        for d in range(self.N):
            r = np.zeros((ctx.n_dof, self.N))
            r[:, d] = 1.0
            out[:, d] = (X @ ctx.mass_apply(r).reshape(-1)) ** 2
        return out

    def vibrational_modes(self, nev, density=1.0, free=None, rtol=1e-6, maxit=500):
        """(frequencies, modes): the nev lowest natural frequencies sqrt(lam) / 2 pi of K x = lam M x (M = density x the consistent mass matrix;
        density: a scalar that multiplies the field of setDensity, or one value per element, which becomes that field)
        and the mode shapes as nodal fields [nev, nNode, N] -- the reference's smallestNonzeroGenEigenpairsPSDKnownKernel (Eigensolver.hh)
        on the device (mfh_modes). The Dirichlet variables of the applied boundary conditions are the clamp (their values play no part);
        free=None means "free body exactly when no Dirichlet condition is present". self.modes_info holds the solver's record."""
        v, _ = self.ctx.bc_dirichlet_vars()
        if free is None:
            free = len(v) == 0
        self.ctx.clear_fixed()
        if not free and len(v):
            self.ctx.fix_variables(v)
        lam, X, info = self.ctx.modes(nev, density=self._density_scalar(density), free=free, rtol=rtol, maxit=maxit)
        self.modes_info = info
        X = X.reshape(len(lam), self.ctx.n_dof, self.N)
        if self.ctx.n_dof != self.ctx.n_node:               # a DoF map (periodic conditions): every node takes its DoF's value
            dof, _ = self.ctx.get_dof_map()
            X = X[:, dof, :]
        return np.sqrt(lam) / (2.0 * np.pi), X

    # ---- more modes than one block holds (docs/design/04_19_many_modes.md)
    def _clamp_for_modes(self, free):
        v, _ = self.ctx.bc_dirichlet_vars()
        if free is None:
            free = len(v) == 0
        self.ctx.clear_fixed()
        if not free and len(v):
            self.ctx.fix_variables(v)
        return free, v

    def vibrational_modes_many(self, nev=None, fmax=None, density=1.0, free=None, locked=None, batch=0, rtol=1e-6, lock_factor=0.1, maxit=500):
        """(frequencies, modes) like vibrational_modes, for up to 256 modes (mfh_modes_many: batches of `batch` modes, each locked on the device
        before the next starts). fmax (Hz): all natural frequencies up to it -- lambdaMax = (2 pi fmax)^2; nev then defaults to the cap of
        256 - len(locked), and self.modes_many_info["bandExhausted"] says whether the band is complete. locked: per-DoF rows [k, nDoF * N] (or
        [k, nDoF, N]) to stay M-orthogonal to, e.g. the modes of an earlier call. The clamp is handled as in vibrational_modes."""
        if nev is None and fmax is None:
            raise ValueError("vibrational_modes_many: give nev, fmax or both")
        free, _ = self._clamp_for_modes(free)
        n = self.ctx.n_dof * self.N
        Q = None if locked is None else np.asarray(locked, dtype=np.float64).reshape(-1, n)
        if nev is None:
            nev = 256 - (0 if Q is None else len(Q))
        lam_max = None if fmax is None else (2.0 * np.pi * float(fmax)) ** 2
        lam, X, info = self.ctx.modes_many(nev, density=self._density_scalar(density), free=free, locked=Q, lambda_max=lam_max, batch=batch, rtol=rtol,
                                           lock_factor=lock_factor, maxit=maxit)
        self.modes_many_info = info
        X = X.reshape(len(lam), self.ctx.n_dof, self.N)
        if self.ctx.n_dof != self.ctx.n_node:               # a DoF map (periodic conditions): every node takes its DoF's value
            dof, _ = self.ctx.get_dof_map()
            X = X[:, dof, :]
        return np.sqrt(lam) / (2.0 * np.pi), X

    def modesForMassFraction(self, fraction=0.9, nmax=256, batch=16, density=1.0, rtol=1e-6, lock_factor=0.1, maxit=500):
        """(frequencies, modes, fractions[N]): the lowest modes of the clamped body, computed `batch` at a time until in every direction d the summed
        modalEffectiveMass reaches `fraction` of r_f^T M_ff r_f (r_f: the unit translation in d, zeroed on the clamp; the product through
        mass_apply) or nmax modes are there. Every call continues the one before through mfh_modes_many's locked set, so each runs to
        rtol * lock_factor: its modes are locked for the next. modes: per-DoF rows as nodal fields [k, nDoF, N]; fractions: what was reached.
        Clamped bodies only, without a DoF map."""
        ctx = self.ctx
        free, v = self._clamp_for_modes(False)
        if len(v) == 0:
            raise ValueError("modesForMassFraction: clamped bodies only (apply a Dirichlet condition)")
        if ctx.n_dof != ctx.n_node:
            raise ValueError("modesForMassFraction: not under a DoF map")
        if not (0.0 < fraction <= 1.0) or not (1 <= int(nmax) <= 256) or not (1 <= int(batch) <= 20):
            raise ValueError("modesForMassFraction: 0 < fraction <= 1, 1 <= nmax <= 256, 1 <= batch <= 20")
        rho = self._density_scalar(density)
        n = ctx.n_dof * self.N
        total = np.empty(self.N)
        for d in range(self.N):
            r = np.zeros((ctx.n_dof, self.N))
            r[:, d] = 1.0
            r.reshape(-1)[np.asarray(v, dtype=np.int64)] = 0.0
            total[d] = rho * float(r.reshape(-1) @ ctx.mass_apply(r).reshape(-1))
        lam_all, X_all, reached = np.zeros(0), np.zeros((0, n)), np.zeros(self.N)
        self.modes_many_info = None
        while len(lam_all) < int(nmax) and np.any(reached < fraction * total):
            nb = min(int(batch), int(nmax) - len(lam_all))
            lam, X, info = ctx.modes_many(nb, density=rho, locked=X_all if len(X_all) else None, batch=int(batch), rtol=rtol * lock_factor, maxit=maxit)
            self.modes_many_info = info
            lam_all, X_all = np.concatenate([lam_all, lam]), np.concatenate([X_all, X])
            reached = reached + rho * rho * self.modalEffectiveMass(X).sum(axis=0)
        order = np.argsort(lam_all, kind="stable")
        return np.sqrt(lam_all[order]) / (2.0 * np.pi), X_all[order].reshape(len(order), ctx.n_dof, self.N), reached / total

    # ---- linear buckling (docs/design/04_16_buckling.md)
    def setPrestress(self, stress):
        """The per-element prestress [nElem, flatLen] (tensor shear entries, the layout of averageStressField) of applyGeometricStiffness and
        buckling (None: no field). It survives vertex updates; a new mesh clears it."""
        self.ctx.set_prestress(stress)

    def applyGeometricStiffness(self, x_dofs):
        """Kg x on a per-DoF displacement vector [nDoF, N]: the geometric stiffness of the prestress field."""
        return self.ctx.geometric_apply(np.asarray(x_dofs, dtype=np.float64).reshape(self.ctx.n_dof, self.N))

    def buckling(self, nev, load=None, rtol=1e-6, maxit=500):
        """(factors, modes, u): solves the static problem under the current boundary conditions (load: a per-DoF vector such as bodyForceLoad's,
        None = neumannLoad()), makes the element-average stress of its displacement u the prestress on the device, and returns the nev smallest
        multiples of the load at which the clamped body buckles (mfh_buckling; +inf where it does not), the buckling shapes as nodal fields
        [nev, nNode, N] and u [nNode, N]. The Dirichlet variables of the applied conditions are the clamp, as in vibrational_modes.
        self.buckling_info holds the solver's record."""
        ctx = self.ctx
        u = self.solve(None if load is None else np.asarray(load, dtype=np.float64).reshape(ctx.n_dof, self.N))
        ctx.prestress_from_displacement(u)
        v, _ = ctx.bc_dirichlet_vars()
        ctx.clear_fixed()
        if len(v):
            ctx.fix_variables(v)
        try:
            fac, X, info = ctx.buckling(nev, rtol=rtol, maxit=maxit)
        finally:
            last = getattr(ctx, "last_buckling", None)
            self.buckling_info = last[2] if last else None
        X = X.reshape(len(fac), ctx.n_dof, self.N)
        if ctx.n_dof != ctx.n_node:                         # a DoF map (periodic conditions): every node takes its DoF's value
            dof, _ = ctx.get_dof_map()
            X = X[:, dof, :]
        return fac, X, u

    # ---- prestressed vibration (docs/design/04_18_prestressed_modes.md)
    def prestressedModes(self, nev, load=None, factors=(1.0,), density=1.0, rtol=1e-6, maxit=500):
        """(lam, modes, u): solves the static problem as buckling() does (load: a per-DoF vector, None = neumannLoad()), makes the element-average
        stress of its displacement u the prestress on the device, and returns for every multiple s in `factors` of that load, in order, the nev
        smallest eigenvalues of (K + s Kg) x = lam M x (mfh_modes_prestressed; frequencies sqrt(lam) / 2 pi while lam > 0, negative beyond the
        critical load): lam [nFactors, nev], the shapes as nodal fields [nFactors, nev, nNode, N] and u [nNode, N]. Every factor after the first
        starts from the shapes of the one before it. density as in vibrational_modes; the Dirichlet variables of the applied conditions are
        the clamp. self.prestressed_modes_info holds the solver's record of every factor."""
        ctx = self.ctx
        factors = [float(s) for s in np.atleast_1d(np.asarray(factors, dtype=np.float64))]
        rho = self._density_scalar(density)
        u = self.solve(None if load is None else np.asarray(load, dtype=np.float64).reshape(ctx.n_dof, self.N))
        ctx.prestress_from_displacement(u)
        v, _ = ctx.bc_dirichlet_vars()
        ctx.clear_fixed()
        if len(v):
            ctx.fix_variables(v)
        lams, shapes, X = [], [], None
        self.prestressed_modes_info = []
        for s in factors:
            try:
                lam, X, info = ctx.modes_prestressed(nev, s, density=rho, x0=X, rtol=rtol, maxit=maxit)
            finally:
                last = getattr(ctx, "last_modes_prestressed", None)
                self.prestressed_modes_info.append(last[2] if last else None)
            lams.append(lam)
            shapes.append(X.reshape(len(lam), ctx.n_dof, self.N))
        shapes = np.array(shapes)
        if ctx.n_dof != ctx.n_node:                         # a DoF map (periodic conditions): every node takes its DoF's value
            dof, _ = ctx.get_dof_map()
            shapes = shapes[:, :, dof, :]
        return np.array(lams), shapes, u

    def transient(self, dt, n_steps, amplitude=None, u0=None, v0=None, density=1.0, damping=(0, 0), beta=0.25, gamma=0.5, probes=None,
                  snapshot_stride=0, a0=None, energies=False, rtol=None, maxit=None, load=None):
        """The response to the load history amplitude[n] x f, f = neumannLoad() or the per-DoF vector `load` (a volume load, a sum of loads), by implicit Newmark time stepping on the device (mfh_newmark):
        M u'' + C u' + K u = g(t) f with M = density x the consistent mass matrix (density: a scalar or one value per element, as in vibrational_modes), C = damping[0] M + damping[1] K. The Dirichlet variables of the
        applied boundary conditions are the clamp, held at zero (their values play no part, as in vibrational_modes); u0 / v0 / a0: nodal fields
        [nNode, N] (None: rest; a0 None: from the equation of motion at step 0 -- pass the "a" of an earlier call to continue it). probes: (node,
        component) pairs whose displacement is recorded at every step. Returns a dict of nodal fields: "u", "v", "a" [nNode, N] after the last
        step, "probes" [n_steps + 1, len(probes)], "snapshots" [n_steps // snapshot_stride + 1, nNode, N] (snapshot_stride > 0), "energies"
        [n_steps + 1, 3] = kinetic, strain, g f.u (energies=True). self.transient_info holds the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        v, _ = ctx.bc_dirichlet_vars()
        ctx.clear_fixed()
        if len(v):
            ctx.fix_variables(v)
        mapped = ctx.n_dof != ctx.n_node                   # a DoF map (periodic conditions): a DoF takes the value of its first node
        dof = ctx.get_dof_map()[0] if mapped else None
        if mapped:
            first = np.full(ctx.n_dof, -1, dtype=np.int64)
            first[dof[::-1]] = np.arange(ctx.n_node)[::-1]

        def to_dofs(x):
            if x is None:
                return None
            x = np.asarray(x, dtype=np.float64).reshape(ctx.n_node, self.N)
            return x[first] if mapped else x

        def to_nodes(x):
            x = x.reshape(x.shape[:-1] + (ctx.n_dof, self.N))
            return x[..., dof, :] if mapped else x
        f = self.neumannLoad() if load is None else np.asarray(load, dtype=np.float64).reshape(ctx.n_dof, self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.newmark(dt, n_steps, u0=to_dofs(u0), v0=to_dofs(v0), a0=to_dofs(a0), f=None if not np.any(f) else f, amplitude=amplitude,
                            density=density, damping=damping, beta=beta, gamma=gamma, rtol=self.rtol if rtol is None else rtol,
                            maxit=self.maxit if maxit is None else maxit, probes=pv, snapshot_stride=snapshot_stride, energies=energies)
        finally:
            self.transient_info = getattr(ctx, "last_newmark", {}).get("info")
        out = dict(r)
        for k in ("u", "v", "a"):
            out[k] = to_nodes(r[k])
        if r["snapshots"] is not None:
            out["snapshots"] = to_nodes(r["snapshots"])
        del out["info"]
        return out

    # ---- explicit dynamics (docs/design/04_20_explicit_dynamics.md)
    def _clamp_dirichlet(self):
        v, _ = self.ctx.bc_dirichlet_vars()
        self.ctx.clear_fixed()
        if len(v):
            self.ctx.fix_variables(v)

    def lumpedMassHRZ(self):
        """[nDoF, N]: the HRZ-lumped masses under the density field of setDensity (every DoF's mass repeated for its components): positive on
        linear and quadratic elements alike, and summing to N times the mass of the body."""
        return self.ctx.mass_lumped_hrz().reshape(self.ctx.n_dof, self.N)

    def stableTimeStep(self, density=1.0, iters=0):
        """The stability limit of transient_explicit bracketed: a dict with dtSafe (stable for certain, from a Gershgorin bound) and dtEst (an upper
        bound of the limit 2 / sqrt(lambda_max) from `iters` power-iteration steps, 0: 60), lambdaUpper, lambdaEst. The Dirichlet variables of
        the applied boundary conditions are the clamp; density as in transient."""
        density = self._density_scalar(density)
        self._clamp_dirichlet()
        return self.ctx.explicit_dt(density=density, iters=iters)

    def transient_explicit(self, n_steps, dt=None, safety=0.9, amplitude=None, u0=None, v0=None, density=1.0, damping=0.0, probes=None,
                           snapshot_stride=0, a0=None, energies=False, energy_stride=1, load=None, check_dt=True):
        """The response to the load history amplitude[n] x f like transient, by explicit central differences with the HRZ-lumped mass matrix
        (mfh_explicit): one product with K per step, no solve -- for wave propagation, impact and short pulses. dt=None: safety x dtEst of
        stableTimeStep (self.explicit_time_step holds the step taken). damping: the mass-proportional Rayleigh coefficient. Fields come back as in
        transient; "energies" [n_steps // energy_stride + 1, 4] = kinetic, strain, g f.u, the leapfrog invariant. self.transient_info holds
        the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        self._clamp_dirichlet()
        if dt is None:
            dt = float(safety) * ctx.explicit_dt(density=density)["dtEst"]
        self.explicit_time_step = float(dt)
        mapped = ctx.n_dof != ctx.n_node                   # a DoF map (periodic conditions): a DoF takes the value of its first node
        dof = ctx.get_dof_map()[0] if mapped else None
        if mapped:
            first = np.full(ctx.n_dof, -1, dtype=np.int64)
            first[dof[::-1]] = np.arange(ctx.n_node)[::-1]

        def to_dofs(x):
            if x is None:
                return None
            x = np.asarray(x, dtype=np.float64).reshape(ctx.n_node, self.N)
            return x[first] if mapped else x

        def to_nodes(x):
            x = x.reshape(x.shape[:-1] + (ctx.n_dof, self.N))
            return x[..., dof, :] if mapped else x
        f = self.neumannLoad() if load is None else np.asarray(load, dtype=np.float64).reshape(ctx.n_dof, self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.explicit(dt, n_steps, u0=to_dofs(u0), v0=to_dofs(v0), a0=to_dofs(a0), f=None if not np.any(f) else f, amplitude=amplitude,
                             density=density, damping=damping, probes=pv, snapshot_stride=snapshot_stride, energies=energies,
                             energy_stride=energy_stride, check_dt=check_dt)
        finally:
            self.transient_info = getattr(ctx, "last_explicit", {}).get("info")
        out = dict(r)
        for k in ("u", "v", "a"):
            out[k] = to_nodes(r[k])
        if r["snapshots"] is not None:
            out["snapshots"] = to_nodes(r["snapshots"])
        del out["info"]
        return out

    def frequencyResponse(self, omegas, load=None, density=1.0, damping=(0, 0), loss_factor=0.0, probes=None, fields=True, warm_start=True,
                          rtol=None, maxit=None):
        """The steady state u^(w) of M u'' + C u' + K u = Re(f^ e^{i w t}) at every w of omegas (rad per unit time), on the device (mfh_harmonic):
        (K + i w C - w^2 M) u^ = f^ with M = density x the consistent mass matrix (density: a scalar or one value per element, as in transient),
        C = damping[0] M + damping[1] K plus the structural term i loss_factor K; f^ = neumannLoad() or the per-DoF vector `load` (real or
        complex: a volume load, a sum of loads). The Dirichlet variables of the applied boundary conditions are the clamp, held at zero.
        probes: (node, component) pairs. Returns a dict: "u" complex nodal fields [nFreq, nNode, N] (fields=True), "probes" complex
        [nFreq, len(probes)], "iterations", "true_residuals". self.harmonic_info holds the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        v, _ = ctx.bc_dirichlet_vars()
        ctx.clear_fixed()
        if len(v):
            ctx.fix_variables(v)
        mapped = ctx.n_dof != ctx.n_node                   # a DoF map (periodic conditions): every node takes its DoF's value
        dof = ctx.get_dof_map()[0] if mapped else None
        f = self.neumannLoad() if load is None else np.asarray(load).reshape(ctx.n_dof, self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.harmonic(omegas, f, density=density, damping=damping, loss_factor=loss_factor, rtol=self.rtol if rtol is None else rtol,
                             maxit=self.maxit if maxit is None else maxit, probes=pv, fields=fields, warm_start=warm_start)
        finally:
            self.harmonic_info = getattr(ctx, "last_harmonic", {}).get("info")
        out = dict(r)
        if r["u"] is not None:
            u = r["u"].reshape(len(r["u"]), ctx.n_dof, self.N)
            out["u"] = u[:, dof, :] if mapped else u
        del out["info"]
        return out

    def modalFrequencyResponse(self, omegas, n_modes=None, modes=None, load=None, density=1.0, damping=(0, 0), loss_factor=0.0, modal_damping=None,
                               static_correction=True, residual_stride=None, probes=None, fields=True, rtol=None, maxit=None, modes_rtol=1e-6,
                               batch=0):
        """frequencyResponse by superposition of the lowest modes (mfh_modal_harmonic, docs/design/04_21_modal_superposition.md): the same system,
        load, clamp, damping, probes and return value, at the cost of one pass over the resident mode basis per group of frequencies. n_modes: the
        basis is computed here (vibrational_modes_many's solver, up to 256 modes, modes_rtol / batch) and stays on the device; modes=(lam, X):
        M-orthonormal eigenpairs the caller has, per-DoF rows [m, nDoF * N]; neither: the basis of the previous call, which must still be valid:
        the same set of Dirichlet variables (calls in between that re-apply the same clamp, such as solve or frequencyResponse, keep it), mesh,
        vertex positions, material and density field -- a per-element `density` array in any call in between sets the field anew and makes
        the basis stale; the call then raises with code ERR_STATE (ctx.modal_basis_state() tells beforehand). static_correction: one static solve per load plane at rtol / maxit stands in for the truncated
        modes (clamped bodies only). modal_damping: damping ratios per mode (a scalar or one per mode). residual_stride: None, or k >= 0 for the
        true residual ||f^ - Z u^|| / ||f^|| at every k-th frequency (0: every one). Returns a dict: "u", "probes", "modal_coords" [nFreq, m],
        "true_residuals" (-1 where none was computed). self.modal_info holds the solver's record, self.modal_frequencies the basis's sqrt(lam) /
        2 pi where it was set here."""
        ctx = self.ctx
        density = self._density_scalar(density)
        mapped = ctx.n_dof != ctx.n_node
        dof = ctx.get_dof_map()[0] if mapped else None
        if n_modes is not None or modes is not None:
            v, _ = ctx.bc_dirichlet_vars()
            ctx.clear_fixed()
            if len(v):
                ctx.fix_variables(v)
            if modes is not None:
                lam, X = modes
                self.modal_basis_info = ctx.set_modal_basis(lam, np.asarray(X, dtype=np.float64).reshape(len(lam), -1), density=density)
            else:
                lam, X, info = ctx.modal_basis(int(n_modes), density=density, free=len(v) == 0, batch=batch, rtol=modes_rtol)
                self.modes_many_info, self.modal_basis_info = info, info["modal_basis"]
            self.modal_frequencies = np.sqrt(np.asarray(lam)) / (2.0 * np.pi)
        f = self.neumannLoad() if load is None else np.asarray(load).reshape(ctx.n_dof, self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.modal_harmonic(omegas, f, damping=damping, loss_factor=loss_factor, modal_damping=modal_damping, static_correction=static_correction,
                                   residual_stride=residual_stride, rtol=self.rtol if rtol is None else rtol, maxit=self.maxit if maxit is None else maxit,
                                   probes=pv, fields=fields)
        finally:
            self.modal_info = getattr(ctx, "last_modal_harmonic", {}).get("info")
        out = dict(r)
        if r["u"] is not None:
            u = r["u"].reshape(len(r["u"]), ctx.n_dof, self.N)
            out["u"] = u[:, dof, :] if mapped else u
        del out["info"]
        return out

    def modalTransient(self, dt, n_steps, amplitude=None, u0=None, v0=None, n_modes=None, modes=None, load=None, density=1.0, damping=(0, 0),
                       modal_damping=None, static_correction=True, probes=None, snapshot_stride=0, modal_coords=False, energies=False, q0=None,
                       qdot0=None, rtol=None, maxit=None, modes_rtol=1e-6, batch=0, chunk_steps=0):
        """transient() by exact integration of the lowest modes (mfh_modal_transient, docs/design/04_22_modal_transient.md): the same load, clamp
        and probes as (node, component) pairs, the load history taken as piecewise linear between amplitude[n]; no stability limit and no
        period error, one pass over the resident basis per snapshot and none at all for probes. n_modes / modes / neither: the basis, exactly
        as in modalFrequencyResponse (the density is the basis's). u0 / v0: nodal fields [nNode, N], projected on the modes; or q0 / qdot0: the
        "q" / "qdot" of an earlier call, to continue it. Returns a dict: "q", "qdot" (the modal state after the last step), "probes"
        [n_steps + 1, len(probes)], "snapshots" [n_steps // snapshot_stride + 1, nNode, N] (snapshot_stride > 0), "modal_coords"
        [n_steps + 1, m], "energies" [n_steps + 1, 3] restricted to the retained modes. self.modal_transient_info holds the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        mapped = ctx.n_dof != ctx.n_node
        dof = ctx.get_dof_map()[0] if mapped else None
        if n_modes is not None or modes is not None:
            v, _ = ctx.bc_dirichlet_vars()
            ctx.clear_fixed()
            if len(v):
                ctx.fix_variables(v)
            if modes is not None:
                lam, X = modes
                self.modal_basis_info = ctx.set_modal_basis(lam, np.asarray(X, dtype=np.float64).reshape(len(lam), -1), density=density)
            else:
                lam, X, info = ctx.modal_basis(int(n_modes), density=density, free=len(v) == 0, batch=batch, rtol=modes_rtol)
                self.modes_many_info, self.modal_basis_info = info, info["modal_basis"]
            self.modal_frequencies = np.sqrt(np.asarray(lam)) / (2.0 * np.pi)
        if mapped:
            first = np.full(ctx.n_dof, -1, dtype=np.int64)
            first[dof[::-1]] = np.arange(ctx.n_node)[::-1]

        def to_dofs(x):
            if x is None:
                return None
            x = np.asarray(x, dtype=np.float64).reshape(ctx.n_node, self.N)
            return x[first] if mapped else x
        f = self.neumannLoad() if load is None else np.asarray(load, dtype=np.float64).reshape(ctx.n_dof, self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.modal_transient(dt, n_steps, f, amplitude=amplitude, q0=q0, qdot0=qdot0, u0=to_dofs(u0), v0=to_dofs(v0), damping=damping,
                                    modal_damping=modal_damping, static_correction=static_correction, rtol=self.rtol if rtol is None else rtol,
                                    maxit=self.maxit if maxit is None else maxit, probes=pv, snapshot_stride=snapshot_stride, modal_coords=modal_coords,
                                    energies=energies, chunk_steps=chunk_steps)
        finally:
            self.modal_transient_info = getattr(ctx, "last_modal_transient", {}).get("info")
        out = dict(r)
        if r["snapshots"] is not None:
            s = r["snapshots"].reshape(len(r["snapshots"]), ctx.n_dof, self.N)
            out["snapshots"] = s[:, dof, :] if mapped else s
        del out["info"]
        return out

    def _ensure_modal_basis(self, n_modes, modes, density, batch, modes_rtol):
        """The basis of the modal calls, as modalFrequencyResponse settles it: computed here, the caller's, or the previous call's."""
        ctx = self.ctx
        if n_modes is None and modes is None:
            return
        v, _ = ctx.bc_dirichlet_vars()
        ctx.clear_fixed()
        if len(v):
            ctx.fix_variables(v)
        if modes is not None:
            lam, X = modes
            self.modal_basis_info = ctx.set_modal_basis(lam, np.asarray(X, dtype=np.float64).reshape(len(lam), -1), density=density)
        else:
            lam, X, info = ctx.modal_basis(int(n_modes), density=density, free=len(v) == 0, batch=batch, rtol=modes_rtol)
            self.modes_many_info, self.modal_basis_info = info, info["modal_basis"]
        self.modal_eigenvalues, self.modal_density = np.asarray(lam, dtype=np.float64).copy(), density
        self.modal_frequencies = np.sqrt(self.modal_eigenvalues) / (2.0 * np.pi)

    def randomResponse(self, omegas, psd, load=None, n_modes=None, modes=None, weights=None, density=1.0, damping=(0, 0), loss_factor=0.0,
                       modal_damping=None, static_correction=True, velocity=False, acceleration=False, probes=None, fields=True, probe_psd=False,
                       tol=-1.0, rtol=None, maxit=None, modes_rtol=1e-6, batch=0):
        """The RMS response to a stationary random load (mfh_modal_random, docs/design/04_23_modal_random.md): the load shapes `load` ([nDoF, N], or
        [nLoad, nDoF, N]; None: the Neumann load) with amplitudes of one-sided (cross-)spectral density psd ([nFreq] or [nFreq, nLoad, nLoad],
        Hermitian) on the ascending grid omegas (resonance_grid builds one that resolves the peaks). Basis (n_modes / modes / neither), clamp,
        damping and probes as in modalFrequencyResponse. Returns a dict: "sigma_u", "sigma_v", "sigma_a": nodal fields [nNode, N] (the latter two on
        request), "probes": dict of "sigma_u", "sigma_v", "sigma_a", "nu0" (upward zero crossings per unit time) and "psd" [len(probes), nFreq], "cov"
        [3, nb, nb]. self.random_info holds the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        mapped = ctx.n_dof != ctx.n_node
        dof = ctx.get_dof_map()[0] if mapped else None
        self._ensure_modal_basis(n_modes, modes, density, batch, modes_rtol)
        f = self.neumannLoad().reshape(1, -1) if load is None else np.asarray(load, dtype=np.float64).reshape(-1, ctx.n_dof * self.N)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        try:
            r = ctx.modal_random(omegas, psd, f, weights=weights, damping=damping, loss_factor=loss_factor, modal_damping=modal_damping,
                                 static_correction=static_correction, velocity=velocity, acceleration=acceleration, tol=tol,
                                 rtol=self.rtol if rtol is None else rtol, maxit=self.maxit if maxit is None else maxit, probes=pv, fields=fields,
                                 probe_psd=probe_psd)
        finally:
            self.random_info = getattr(ctx, "last_modal_random", {}).get("info")
        out = dict(r)
        for name in ("sigma_u", "sigma_v", "sigma_a"):
            if r[name] is not None:
                s = r[name].reshape(ctx.n_dof, self.N)
                out[name] = s[dof, :] if mapped else s
        del out["info"]
        return out

    def responseSpectrum(self, direction, Sd, modal_damping=0.05, rule="cqc", n_modes=None, modes=None, density=1.0, probes=None, fields=True,
                         tol=-1.0, modes_rtol=1e-6, batch=0):
        """The peak response to a design spectrum applied as a base motion in `direction` (0 .. N-1): R_i = sqrt(phi_i^T C phi_i) with
        C_jk = rho_jk a_j a_k, a_j = Gamma_j Sd_j, Gamma = Phi^T (density M) r_d the participation factors of the unit translation r_d
        (mfh_modal_quadratic). Sd: the spectral displacement per mode, or a callable Sd(omega, zeta) evaluated at the modes' sqrt(lam_j).
        rule: "srss" (rho = I) or "cqc" (cqc_matrix with modal_damping, a scalar or one ratio per mode). Basis and probes as in
        modalFrequencyResponse. Returns a dict: "R" [nNode, N] (None without fields), "probes" [len(probes)]. self.spectrum_info: "gamma",
        "effective_mass" (gamma^2), "mass_fraction" (their sum over the moving mass r_f^T (density M_ff) r_f), "a", "rho", and the solver's record."""
        ctx = self.ctx
        if rule not in ("cqc", "srss"):
            raise ValueError("responseSpectrum: rule is 'cqc' or 'srss'")
        d = int(direction)
        if not 0 <= d < self.N:
            raise ValueError("responseSpectrum: direction in 0 .. %d" % (self.N - 1))
        density = self._density_scalar(density)
        mapped = ctx.n_dof != ctx.n_node
        dof = ctx.get_dof_map()[0] if mapped else None
        self._ensure_modal_basis(n_modes, modes, density, batch, modes_rtol)
        m = ctx.modal_basis_state()[0]
        lam = getattr(self, "modal_eigenvalues", None)
        if lam is None or len(lam) != m:
            raise ValueError("responseSpectrum: the basis was not set through this Simulator (pass n_modes or modes)")
        r = np.zeros((ctx.n_dof, self.N))
        r[:, d] = 1.0
        gamma = ctx.modal_coordinates(r.reshape(-1))
        zeta = np.broadcast_to(np.asarray(modal_damping, dtype=np.float64), (m,))
        sd = np.asarray(Sd(np.sqrt(lam), zeta), dtype=np.float64) if callable(Sd) else np.asarray(Sd, dtype=np.float64)
        a = gamma * np.broadcast_to(sd, (m,))
        from .core import cqc_matrix
        rho = np.eye(m) if rule == "srss" else cqc_matrix(lam, zeta)
        pv = None
        if probes is not None:
            pr = np.asarray(probes, dtype=np.int64).reshape(-1, 2)
            pv = (dof[pr[:, 0]] if mapped else pr[:, 0]) * self.N + pr[:, 1]
        q = ctx.modal_quadratic(rho * np.outer(a, a), tol=tol, probes=pv, fields=fields)
        v, _ = ctx.bc_dirichlet_vars()
        rf = r.copy()
        rf.reshape(-1)[np.asarray(v, dtype=np.int64)] = 0.0
        moving = self.modal_density * float(rf.reshape(-1) @ ctx.mass_apply(rf).reshape(-1))
        self.spectrum_info = {"gamma": gamma, "effective_mass": gamma ** 2, "mass_fraction": float((gamma ** 2).sum() / moving), "a": a, "rho": rho,
                              "info": q["info"]}
        R = None
        if q["fields"] is not None:
            R = q["fields"][0].reshape(ctx.n_dof, self.N)
            R = R[dof, :] if mapped else R
        return {"R": R, "probes": q["probes"][0]}

    def randomStress(self, omegas, psd, load=None, n_modes=None, modes=None, weights=None, density=1.0, damping=(0, 0), loss_factor=0.0,
                     modal_damping=None, static_correction=True, von_mises=True, components=False, strain=False, tol=-1.0, rtol=None, maxit=None,
                     modes_rtol=1e-6, batch=0):
        """The RMS stress under the stationary random load of randomResponse (mfh_modal_random_stress, docs/design/04_24_modal_stress.md): the
        same loads, spectrum, basis, clamp and damping. Returns a dict: "von_mises" [nElem, NQ] = sqrt(E[sigma_vm^2]) (Segalman: the root of the mean
        square of the von Mises stress, not its mean), "components" [nElem, NQ, flatLen] = sqrt(E[sigma_c^2]) (on request), "peak" (value, element,
        corner), "cov" [nb, nb]; NQ = 1 for degree 1, N + 1 for degree 2 (stressField's layout). strain=True: strains instead.
        self.random_stress_info holds the solver's record."""
        ctx = self.ctx
        density = self._density_scalar(density)
        self._ensure_modal_basis(n_modes, modes, density, batch, modes_rtol)
        f = self.neumannLoad().reshape(1, -1) if load is None else np.asarray(load, dtype=np.float64).reshape(-1, ctx.n_dof * self.N)
        try:
            r = ctx.modal_random_stress(omegas, psd, f, weights=weights, damping=damping, loss_factor=loss_factor, modal_damping=modal_damping,
                                        static_correction=static_correction, tol=tol, rtol=self.rtol if rtol is None else rtol,
                                        maxit=self.maxit if maxit is None else maxit, von_mises=von_mises, components=components, strain=strain)
        finally:
            self.random_stress_info = getattr(ctx, "last_modal_stress", {}).get("info")
        out = dict(r)
        del out["info"]
        return out

    def responseSpectrumStress(self, direction, Sd, modal_damping=0.05, rule="cqc", n_modes=None, modes=None, density=1.0, von_mises=True,
                               components=False, strain=False, tol=-1.0, modes_rtol=1e-6, batch=0):
        """The peak stress under the design spectrum of responseSpectrum (mfh_modal_quadratic_stress): the same a_j = Gamma_j Sd_j and the same
        rules "srss" / "cqc", C_jk = rho_jk a_j a_k. Returns a dict: "von_mises" [nElem, NQ], "components" [nElem, NQ, flatLen] (on request), "peak"
        (value, element, corner). self.spectrum_stress_info: "gamma", "a", "rho" and the solver's record."""
        ctx = self.ctx
        if rule not in ("cqc", "srss"):
            raise ValueError("responseSpectrumStress: rule is 'cqc' or 'srss'")
        d = int(direction)
        if not 0 <= d < self.N:
            raise ValueError("responseSpectrumStress: direction in 0 .. %d" % (self.N - 1))
        density = self._density_scalar(density)
        self._ensure_modal_basis(n_modes, modes, density, batch, modes_rtol)
        m = ctx.modal_basis_state()[0]
        lam = getattr(self, "modal_eigenvalues", None)
        if lam is None or len(lam) != m:
            raise ValueError("responseSpectrumStress: the basis was not set through this Simulator (pass n_modes or modes)")
        r = np.zeros((ctx.n_dof, self.N))
        r[:, d] = 1.0
        gamma = ctx.modal_coordinates(r.reshape(-1))
        zeta = np.broadcast_to(np.asarray(modal_damping, dtype=np.float64), (m,))
        sd = np.asarray(Sd(np.sqrt(lam), zeta), dtype=np.float64) if callable(Sd) else np.asarray(Sd, dtype=np.float64)
        a = gamma * np.broadcast_to(sd, (m,))
        from .core import cqc_matrix
        rho = np.eye(m) if rule == "srss" else cqc_matrix(lam, zeta)
        q = ctx.modal_quadratic_stress(rho * np.outer(a, a), tol=tol, von_mises=von_mises, components=components, strain=strain)
        self.spectrum_stress_info = {"gamma": gamma, "a": a, "rho": rho, "info": q["info"]}
        return {"von_mises": None if q["von_mises"] is None else q["von_mises"][0], "components": None if q["components"] is None else q["components"][0],
                "peak": q["peak"][0]}

    def applyStiffnessMatrix(self, u_dofs):                             # :801-823
        return self.ctx.apply_K(np.asarray(u_dofs).ravel()).reshape(-1, self.N)

    def strainField(self, u_nodes):                                     # :511-517 (interpolant values per element)
        return self.ctx.strain_field(u_nodes)

    def stressField(self, u_nodes):                                     # :519-526
        return self.ctx.strain_field(u_nodes, stress=True)

    def elementStrain(self, i, u_nodes):                                # :493-497 (one element of strainField)
        return self.ctx.strain_field(u_nodes)[i]

    def averageStrainField(self, u_nodes):                              # :528-538
        return self.ctx.average_strain(u_nodes)

    def boundaryStrainField(self, u_nodes, stress=False):
        """strain (stress) interpolants restricted to the boundary elements (restrictInterpolant, InterpolantRestriction.hh:29-66):
        [nBdryElem, 1 | N, flatLen], values at the boundary element's corners in its own vertex order"""
        return self.ctx.boundary_strain_field(u_nodes, stress=stress)

    def averageStressField(self, u_nodes):                              # :539-549
        return self.ctx.average_stress(u_nodes)

    # ---- discrete shape derivatives (forward mode), :1297-1374
    def applyDeltaStiffnessMatrix(self, u_nodes, deltaP):               # :1301-1328  per-node u -> per-DoF load
        return self.ctx.apply_delta_K(u_nodes, deltaP)

    def deltaConstantStrainLoad(self, cstrain_flat, deltaP):            # :1331-1348
        return self.ctx.delta_constant_strain_load(cstrain_flat, deltaP)

    def deltaAverageStrainField(self, u_nodes, deltaU, deltaP):         # :1364-1374
        return self.ctx.delta_average_strain(u_nodes, deltaU, deltaP)

    def deltaAverageStressField(self, u_nodes, deltaU, deltaP):         # C : deltaAverageStrainField (deltaStress :280-286)
        return self.ctx.delta_average_strain(u_nodes, deltaU, deltaP, stress=True)

    def benchmarkReport(self):
        """Timings under the reference's timer-section names (GlobalBenchmark.hh:14-34; sections of
        LinearElasticity.hh:1206,1394-1399,482-485 and SparseMatrices.hh:283): milliseconds of the last operations.
        "Compress Matrix" is the once-per-mesh symbolic phase here (sumRepeated's sort/merge hoisted out of the
        numeric assembly); the CHOLMOD sections have no counterpart (PCG)."""
        t = self.ctx.timing()
        info = getattr(self, "info", None) or {}
        return {"Assemble System": t["geometry_ms"] + t["assemble_ms"], "Compress Matrix": t["symbolic_ms"],
                "Set System": t["upload_ms"], "Fix Variables": info.get("setup_ms", 0.0),
                "Elasticity Solve": info.get("solve_ms", 0.0), "PCG iterations": info.get("iterations", 0)}

    def assembleStiffnessMatrix(self):
        """m_assembleStiffnessMatrix (:1408-1466) + sumRepeated: upper triplets (i, j, v)."""
        self.ctx.assemble()
        return self.ctx.export_upper_triplets()

    def stiffnessMatrix(self):
        self.ctx.assemble()
        return self.ctx.export_scipy()
