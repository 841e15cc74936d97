"""FP64 references of the element-integral kernels (constantStrainLoad, averageStrainField, strainField, the forward-mode shape
derivatives, the mutual energies and their one-form) as batched einsums over the elements, fast enough for a few thousand P2 tets in
every (dim, degree, material mode) flavour -- the oracle states most of them as per-element Python loops. Written from the
mathematics (oracle/meshfem_oracle.py and the header comments of the kernels), on top of the oracle's batched pieces
(delta_gl_batch, gradphi_at_quadrature, delta_per_element_stiffness_batch, FEMMesh.embeddings_batch); pinned to the oracle's literal
functions by tests/test_element_integrals_reference.py.

An `ElemSet` is any set of elements of one mesh (all of it, or a window of a mesh too large for the oracle): node ids per element
(corners first; vertex v is node v), vertex positions, one flattened tensor D or one per element, and the DoF of every node.
Conventions as in the oracle: flattened symmetric tensors carry TENSOR shear components; u, w are per-node fields, loads per-DoF."""
import types

import numpy as np

from oracle import meshfem_oracle as O


# ------------------------------------------------------------------------------------------------ meshes and materials (shared by the GPU tests)
MODES = ("iso", "iso_field", "general", "ortho_field", "general_field", "ortho")   # material modes 0..5 of the context


def perturbed(V, amount, seed=0):
    """Interior vertices moved by up to `amount` (uniform, per coordinate); the boundary of the box stays put, so that periodic faces match."""
    V = np.array(V, dtype=np.float64)
    lo, hi = V.min(axis=0), V.max(axis=0)
    inner = np.all((V > lo + 1e-9) & (V < hi - 1e-9), axis=1)
    rng = np.random.default_rng(seed + V.shape[1])
    V[inner] += amount * rng.uniform(-1.0, 1.0, size=(int(inner.sum()), V.shape[1]))
    return V


def spd(rng, fl):
    A = rng.normal(size=(fl, fl))
    return A @ A.T + fl * np.eye(fl)


def material(mode, dim, n_elem, seed=0):
    """(setter of the context, D of every element [nElem, fl, fl] or the one D [fl, fl])."""
    from meshfem_amd import grid
    rng = np.random.default_rng(100 + seed)
    fl = dim * (dim + 1) // 2
    if mode == "iso":
        return (lambda c: c.material_isotropic(200.0, 0.35)), O.ElasticityTensor.isotropic(dim, 200.0, 0.35).D
    if mode == "iso_field":
        E, nu = rng.uniform(50.0, 300.0, n_elem), rng.uniform(0.1, 0.4, n_elem)
        return (lambda c: c.material_iso_field(E, nu)), np.stack([O.ElasticityTensor.isotropic(dim, a, b).D for a, b in zip(E, nu)])
    if mode == "general":
        D = spd(rng, fl)
        return (lambda c: c.material_const(D)), D
    if mode == "general_field":
        D = np.stack([spd(rng, fl) for _ in range(n_elem)])
        return (lambda c: c.material_tensor_field(D)), D
    if mode == "ortho_field":
        P = grid.synthetic_orthotropic_field(n_elem, dim, seed=seed)
        return (lambda c: c.material_ortho_field(P)), orthotropic_D(dim, P)
    assert mode == "ortho"
    D = (O.ElasticityTensor.orthotropic3d(100.0, 150.0, 120.0, 0.2, 0.25, 0.3, 40.0, 50.0, 60.0) if dim == 3
         else O.ElasticityTensor.orthotropic2d(100.0, 150.0, 0.25, 40.0)).D
    return (lambda c: c.material_const(D)), D


def orthotropic_D(dim, P):
    """ElasticityTensor::setOrthotropic (ElasticityTensor.hh:136-164) for every row of P: the inverse of the compliance matrix."""
    P = np.asarray(P, dtype=np.float64)
    fl = dim * (dim + 1) // 2
    S = np.zeros((len(P), fl, fl))
    if dim == 3:
        Ex, Ey, Ez, nyx, nzx, nzy, myz, mzx, mxy = P.T
        S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = 1 / Ex, 1 / Ey, 1 / Ez
        S[:, 0, 1] = S[:, 1, 0] = -nyx / Ey
        S[:, 0, 2] = S[:, 2, 0] = -nzx / Ez
        S[:, 1, 2] = S[:, 2, 1] = -nzy / Ez
        S[:, 3, 3], S[:, 4, 4], S[:, 5, 5] = 1 / myz, 1 / mzx, 1 / mxy
    else:
        Ex, Ey, nyx, mxy = P.T
        S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = 1 / Ex, 1 / Ey, 1 / mxy
        S[:, 0, 1] = S[:, 1, 0] = -nyx / Ey
    return np.linalg.inv(S)


# ------------------------------------------------------------------------------------------------ flattening
def flat_pairs(N):
    """(I, J): the matrix entry of every flattened component (Flattening.hh:62-83)."""
    ij = [O.unflatten_index(N, k) for k in range(O.flat_len(N))]
    return np.array([p[0] for p in ij]), np.array([p[1] for p in ij])


def flatten(N, S):
    """[..., N, N] symmetric matrices -> [..., flatLen]"""
    I, J = flat_pairs(N)
    return S[..., I, J]


def unflatten(N, v):
    F = np.array([[O.flatten_indices(N, i, j) for j in range(N)] for i in range(N)])
    return np.asarray(v)[..., F]


def rank4(N, D):
    """C_ijkl = D[flat(i,j), flat(k,l)] (ElasticityTensor.hh:274-277) for D [..., fl, fl]"""
    F = np.array([[O.flatten_indices(N, i, j) for j in range(N)] for i in range(N)])
    return np.asarray(D)[..., F[:, :, None, None], F[None, None, :, :]]


def sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


class ElemSet:
    def __init__(self, dim, deg, elem_nodes, verts, D, dof=None, n_dof=None):
        self.N = self.K = dim
        self.deg = deg
        self.en = np.asarray(elem_nodes, dtype=np.int64)
        self.nv = dim + 1
        shim = types.SimpleNamespace(verts=np.asarray(verts, dtype=np.float64), elems=self.en[:, :self.nv], K=dim, N=dim)
        self.vol, self.gl = O.FEMMesh.embeddings_batch(shim)            # [nE], [nE, N, nv]
        D = np.asarray(D, dtype=np.float64)
        self.D = D if D.ndim == 3 else D[None]                          # [nE | 1, fl, fl]
        self.C4 = rank4(dim, self.D)
        n_node = int(self.en.max()) + 1
        self.dof = np.arange(n_node) if dof is None else np.asarray(dof, dtype=np.int64)
        self.n_dof = (len(self.dof) if dof is None else int(self.dof.max()) + 1) if n_dof is None else int(n_dof)

    @classmethod
    def from_sim(cls, sim):
        """All elements of an oracle Simulator, with its materials and DoF map."""
        m = sim.mesh
        return cls(sim.N, sim.deg, m.elem_nodes, m.verts, np.stack([t.D for t in sim.D]), sim.dof_array(), sim.numDoFs())

    def corner(self, per_vertex):
        """extractElementCornerValues: [nE, nv, ...]"""
        return np.asarray(per_vertex, dtype=np.float64)[self.en[:, :self.nv]]

    def scatter(self, fe):
        """per-(element, node) values [nE, n, N] summed into the per-DoF vector"""
        out = np.zeros((self.n_dof, self.N))
        np.add.at(out, self.dof[self.en], fe)
        return out

    def stress(self, eps):
        """C_e : eps for flattened strains [nE, fl] or [nE, k, fl] (ElasticityTensor.hh:444-449: D times the shear-doubled strain)"""
        dbl = np.where(np.arange(self.D.shape[-1]) < self.N, 1.0, 2.0)
        D = np.broadcast_to(self.D, (len(self.en),) + self.D.shape[1:])
        return np.einsum("erc,e...c->e...r", D, eps * dbl)


# ------------------------------------------------------------------------------------------------ shape function gradients
def gradphi_at(deg, K, gl, pts):
    """grad phi_i at the barycentric points pts [np, K+1] (EmbeddedElement.hh:315-332): [nE, np, n, N] from gl [nE, N, K+1]"""
    pts = np.asarray(pts, dtype=np.float64)
    nE, N, nv = gl.shape
    glT = np.transpose(gl, (0, 2, 1))
    if deg == 1:
        return np.broadcast_to(glT[:, None], (nE, len(pts), nv, N)).copy()
    G = np.empty((nE, len(pts), O.num_nodes(K, 2), N))
    G[:, :, :nv] = glT[:, None] * (4.0 * pts - 1.0)[None, :, :, None]
    for e in range(O.num_edges(K)):
        s, t = O.EDGE_START[e], O.EDGE_END[e]
        G[:, :, nv + e] = 4.0 * (pts[None, :, t, None] * glT[:, None, s] + pts[None, :, s, None] * glT[:, None, t])
    return G


def interpolant_nodes(deg, K):
    """the nodes of the degree-(deg-1) interpolants of strains and gradients: one value (P1) or the corners (P2)"""
    return np.full((1, K + 1), 1.0 / (K + 1)) if deg == 1 else np.eye(K + 1)


def mean_gradphi(deg, K, gl):
    """(1 / vol) int grad phi_i: the mean of the nodal values of its (constant or linear) interpolant (Functions.hh:246-253): [nE, n, N]"""
    return gradphi_at(deg, K, gl, interpolant_nodes(deg, K)).mean(axis=1)


# ------------------------------------------------------------------------------------------------ the operations
def average_strain(s, u, gl=None):
    """averageStrainField (LinearElasticity.hh:99-123, :528-549): [nE, fl]; gl: other gradients than the mesh's (shape derivatives)"""
    gb = mean_gradphi(s.deg, s.K, s.gl if gl is None else gl)
    return flatten(s.N, sym(np.einsum("eic,eib->ecb", np.asarray(u)[s.en], gb)))


def average_gradient(s, u_scalar):
    """PoissonMesh::gradUAverage (Poisson.hh:121-131): [nE, N]"""
    return np.einsum("ei,eib->eb", np.asarray(u_scalar)[s.en], mean_gradphi(s.deg, s.K, s.gl))


def strain_field(s, u, stress=False):
    """strainField / stressField (LinearElasticity.hh:511-526): the nodal values of the per-element interpolant, [nE, 1 | nv, fl]"""
    G = gradphi_at(s.deg, s.K, s.gl, interpolant_nodes(s.deg, s.K))
    eps = flatten(s.N, sym(np.einsum("eic,eqib->eqcb", np.asarray(u)[s.en], G)))
    return s.stress(eps) if stress else eps


def boundary_strain_field(s, u, bdry_parent, bdry_verts, stress=False):
    """restrictInterpolant of Element::strain to the boundary elements (InterpolantRestriction.hh:29-66): [nBE, 1 | N, fl], the parent's
    value at the boundary element's corners in their own order. s must hold every parent (all elements of the mesh)."""
    vol = strain_field(s, u, stress)
    parent = np.asarray(bdry_parent, dtype=np.int64)
    if s.deg == 1:
        return vol[parent]
    local = (s.en[parent, None, :s.nv] == np.asarray(bdry_verts)[:, :, None]).argmax(axis=2)      # [nBE, N]
    return vol[parent[:, None], local]


def constant_strain_load(s, cstrain, delta_p=None):
    """constantStrainLoad (LinearElasticity.hh:551-562, :135-162): l_i = (C : cstrain) int grad phi_i, per DoF; with delta_p its first
    variation deltaConstantStrainLoad (:289-304, :1331-1348): int grad phi_i dV -> vol (rel mean(grad phi_i) + mean(delta grad phi_i))."""
    sig = np.einsum("eabcd,cd->eab", s.C4, np.asarray(cstrain, dtype=np.float64))
    if delta_p is None:
        gint = s.vol[:, None, None] * mean_gradphi(s.deg, s.K, s.gl)
    else:
        dgl, rel = O.delta_gl_batch(s.gl, s.corner(delta_p))
        gint = s.vol[:, None, None] * (rel[:, None, None] * mean_gradphi(s.deg, s.K, s.gl) + mean_gradphi(s.deg, s.K, dgl))
    return s.scatter(np.einsum("ecb,eib->eic", np.broadcast_to(sig, (len(s.en),) + sig.shape[1:]), gint))


def delta_average_strain(s, u, delta_u, delta_p):
    """deltaAverageStrainField (:1364-1374): strain(delta u) + the strain of u on the perturbed gradients (:259-277)"""
    dgl, _ = O.delta_gl_batch(s.gl, s.corner(delta_p))
    return average_strain(s, delta_u) + average_strain(s, u, gl=dgl)


def apply_delta_K(s, u, delta_p):
    """applyDeltaStiffnessMatrix (:1301-1328): per-node u -> per-DoF (delta K) u"""
    dKe = O.delta_per_element_stiffness_batch(s.deg, s.K, s.gl, s.vol, s.C4, s.corner(delta_p))
    fe = np.einsum("eij,ej->ei", dKe, np.asarray(u)[s.en].reshape(len(s.en), -1))
    return s.scatter(fe.reshape(len(s.en), s.en.shape[1], s.N))


def integrated_stress_terms(s, u, cstrain_flat=None):
    """the terms vol_e C_e : (average strain_e(u) + cstrain) of homogenizedElasticityTensor's element loop
    (PeriodicHomogenization.hh:72-100): [nE, fl]"""
    eps = average_strain(s, u)
    if cstrain_flat is not None:
        eps = eps + np.asarray(cstrain_flat, dtype=np.float64)[None]
    return s.vol[:, None] * s.stress(eps)


def _cell_strains(s, w, gl):
    """for every field w^ij: grad w at the quadrature points W [fl, nE, nq, N(p), N(c)] = d w_p / d x_c on the gradients gl, the weights"""
    G, wq = O.gradphi_at_quadrature(s.deg, s.K, gl)
    return np.stack([np.einsum("eip,eqic->eqpc", np.asarray(x)[s.en], G) for x in w]), wq


def mutual_energy_terms(s, w, delta_p=None):
    """per-element terms [nE, fl, fl] of the mutual energies sum_e int (e^ij + eps(w^ij)) : C : (e^kl + eps(w^kl)) dV, or with delta_p of
    their discrete shape derivative in the volume form quoted at PeriodicHomogenization.hh:484-491:
    int rel G^ij : C : G^kl + (delta eps)(w^ij) : C : G^kl + G^ij : C : (delta eps)(w^kl) dV  (C major-symmetric)."""
    N, fl = s.N, O.flat_len(s.N)
    W, wq = _cell_strains(s, w, s.gl)
    G = sym(W) + np.stack([O.canonical_strain(N, k) for k in range(fl)])[:, None, None]
    S = np.einsum("eabcd,ieqcd->ieqab", np.broadcast_to(s.C4, (len(s.en),) + (N,) * 4), G)
    if delta_p is None:
        return np.einsum("q,e,ieqab,jeqab->eij", wq, s.vol, G, S, optimize=True)
    dgl, rel = O.delta_gl_batch(s.gl, s.corner(delta_p))
    dG = sym(_cell_strains(s, w, dgl)[0])
    t = np.einsum("q,e,ieqab,jeqab->eij", wq, s.vol, dG, S, optimize=True)
    return np.einsum("q,e,ieqab,jeqab->eij", wq, s.vol * rel, G, S, optimize=True) + t + np.transpose(t, (0, 2, 1))


def longdouble_sum(terms):
    """(sum over the elements in extended precision, sum of the absolute terms: the scale of the rounding of any summation order)"""
    t = np.asarray(terms)
    return np.asarray(t.astype(np.longdouble).sum(axis=0), dtype=np.float64), np.abs(t).sum(axis=0)


def mutual_energy_differential(s, w, n_vert):
    """d(mutual energies) / d(vertex positions), [fl, fl, nVert, N] (homogenizedElasticityTensorDiscreteDifferential,
    PeriodicHomogenization.hh:372-480, before the division by |Y|). Under the unit perturbation e_c of corner k of an element,
    rel = gl_k[c] and delta grad phi_i = -gl_k (grad phi_i)[c], hence (delta eps)(w) = -sym(grad w[:, c] (x) gl_k): the element adds
    Q gl_k with  Q = int (G^ij : S^kl) I - (grad w^ij)^T S^kl - (grad w^kl)^T S^ij dV,  S = C : G."""
    N, fl = s.N, O.flat_len(s.N)
    W, wq = _cell_strains(s, w, s.gl)
    G = sym(W) + np.stack([O.canonical_strain(N, k) for k in range(fl)])[:, None, None]
    S = np.einsum("eabcd,ieqcd->ieqab", np.broadcast_to(s.C4, (len(s.en),) + (N,) * 4), G)
    out = np.zeros((fl, fl, n_vert, N))
    eye = np.eye(N)
    for i in range(fl):
        for j in range(i, fl):
            E = np.einsum("eqab,eqab->eq", G[i], S[j])
            Q = E[:, :, None, None] * eye - np.einsum("eqpc,eqpr->eqcr", W[i], S[j]) - np.einsum("eqpc,eqpr->eqcr", W[j], S[i])
            Q = np.einsum("q,e,eqcr->ecr", wq, s.vol, Q)
            np.add.at(out[i, j], s.en[:, :s.nv], np.einsum("ecr,erk->ekc", Q, s.gl))
            out[j, i] = out[i, j]
    return out
