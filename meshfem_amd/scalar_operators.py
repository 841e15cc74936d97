"""Scalar operators on the GPU path: mirrors of `Laplacian::construct`
(Laplacian.hh:97-104), `MassMatrix::construct` (MassMatrix.hh:103-128) and `PoissonMesh`
(Poisson.hh:55-132). They run on the kernels of the elasticity path with 1x1 blocks
(`Context.set_operator`): same mesh topology, pattern, gather lists, assembly kernel, SpMV and PCG.
`forceP1=True` gives the reference's forced-degree-1 variants on a quadratic mesh
(`Laplacian::construct<1>`, `MassMatrix::construct<1>`): a degree-1 view of the same context on its
vertices (`Context.set_operator_degree`), no second mesh. `mass_elasticity` is
`MassMatrix::construct_vector_valued` (one stored value per block on the device), `gradient` /
`divergence` the two remaining functions of the reference's `differential_operators` module."""
import numpy as np

from . import _lib as L
from .core import Context


def _context_for(elements, vertices, degree, device, op):
    c = Context(device)
    c.mesh_build(np.asarray(elements), np.asarray(vertices, dtype=np.float64), degree)
    c.set_operator(op)
    return c


class _Triplets:
    """Upper-triangle triplets after sumRepeated (column-major order, like TripletMatrix::dumpBinary)."""

    def __init__(self, n, i, j, v):
        self.m = self.n = n
        self.i, self.j, self.v = i, j, v

    @property
    def nnz(self):
        return len(self.v)

    def toSciPy(self, full=True):
        import scipy.sparse as sp
        A = sp.coo_matrix((self.v, (self.i.astype(np.int64), self.j.astype(np.int64))), shape=(self.m, self.n)).tocsr()
        if full:
            A = A + sp.triu(A, 1).T
        return A


def _select(c, op, forceP1):
    """Operator and degree view of a context (the degree is left as the caller finds it: see _assembled)."""
    if c.op == L.OP_ELASTICITY and c.op_degree == 0 and forceP1:
        c.set_operator(op)                                 # elasticity has no degree-1 view: leave it first
    c.set_operator_degree(1 if forceP1 else 0)
    c.set_operator(op)


def _assembled(c, op, forceP1, lumped=False):
    """Triplets of `op` on `c`; a caller's context gets its degree view back afterwards."""
    before = c.op_degree
    _select(c, op, forceP1)
    try:
        c.assemble()
        n = c.bs * c.matrix_info()[0]                      # rows of the degree view in force, as the library counts them
        if lumped:
            diag = c.mass_lumped()                         # row sums of the full symmetric matrix, summed on the device
            r = np.arange(n, dtype=np.uint64)
            return _Triplets(n, r, r.copy(), diag)
        i, j, v = c.export_upper_triplets()
        return _Triplets(n, i, j, v)
    finally:
        c.set_operator_degree(before)


def laplacian(elements, vertices, degree=1, device=0, ctx=None, forceP1=False):
    """== Laplacian::construct: upper triangle of the (positive semi-definite) FEM Laplacian; `forceP1`:
    Laplacian::construct<1> on the vertices of a quadratic mesh."""
    c = ctx or _context_for(elements, vertices, degree, device, L.OP_LAPLACIAN)
    return _assembled(c, L.OP_LAPLACIAN, forceP1)


def mass_matrix(elements, vertices, degree=1, lumped=False, device=0, ctx=None, forceP1=False):
    """== MassMatrix::construct: upper triangle of the mass matrix; `lumped` puts the row sums of the
    full matrix on the diagonal (MassMatrix.hh:110-124); `forceP1`: MassMatrix::construct<1>."""
    c = ctx or _context_for(elements, vertices, degree, device, L.OP_MASS)
    return _assembled(c, L.OP_MASS, forceP1, lumped)


def mass_elasticity(elements, vertices, degree, lumped=False, forceP1=False, ctx=None, device=0):
    """== MassMatrix::construct_vector_valued (MassMatrix.hh:131-147): the mass matrix on interleaved
    displacement vectors, entries (dim i + c, dim j + c, m_ij)."""
    c = ctx or _context_for(elements, vertices, degree, device, L.OP_MASS_VECTOR)
    return _assembled(c, L.OP_MASS_VECTOR, forceP1, lumped)


def _as_context(ctx_or_mesh, device=0):
    if isinstance(ctx_or_mesh, Context):
        return ctx_or_mesh
    if hasattr(ctx_or_mesh, "ctx"):                        # PoissonMesh, Simulator
        return ctx_or_mesh.ctx
    elements, vertices, degree = ctx_or_mesh               # (elements, vertices, degree)
    return _context_for(elements, vertices, degree, device, L.OP_LAPLACIAN)


def gradient(ctx_or_mesh, scalarField):
    """Per-element average gradient of a scalar nodal field (differential_operators.gradient; PoissonMesh::gradUAverage)."""
    return _as_context(ctx_or_mesh).average_gradient(scalarField)


def divergence(ctx_or_mesh, vectorField):
    """out[n] = sum_{e containing n} v_e . int_e grad phi_n for a per-element vector field
    (differential_operators.divergence); linear meshes only, like the reference."""
    return _as_context(ctx_or_mesh).divergence(vectorField)


class PoissonMesh:
    """== PoissonMesh<K, Deg, EmbeddingSpace>: -laplace u = 0 with Dirichlet values on boundary regions and the
    natural zero-Neumann condition elsewhere."""

    def __init__(self, elements, vertices, degree=1, device=0):
        self.ctx = _context_for(elements, vertices, degree, device, L.OP_LAPLACIAN)
        self.rtol, self.maxit = 1e-10, 100000
        self.info = None

    def numNodes(self):
        return self.ctx.n_node

    def nodes(self):
        return self.ctx.node_positions()

    def applyDirichletBox(self, min_corner, max_corner, value, relative=False):
        """One DirichletCondition of `applyBoundaryConditions` (Poisson.hh:69-84): boundary nodes inside the
        inclusive box get `value` (the reference encodes it as the displacement's first component)."""
        d = self.ctx.dim
        self.ctx.bc_dirichlet_box(min_corner, max_corner, [float(value)] + [0.0] * (d - 1), relative=relative,
                                  components=[True] + [False] * (d - 1))

    def solve(self):
        u = self.ctx.sim_solve(None, use_pin=False, rtol=self.rtol, maxit=self.maxit)
        self.info = self.ctx.last_info
        return u[:, 0]

    def gradUAverage(self, u):
        return self.ctx.average_gradient(u)
