/*
 * meshfem_hip.h -- C ABI of libmeshfem_hip.so: the MI355X (gfx950) implementation of MeshFEM's
 * per-element linear-elasticity stiffness assembly + sparse solve hot path.
 *
 * The reference (MeshFEM) has no FFI seam for this path: everything is C++ templates
 * instantiated in the caller.  Every entry point below therefore cites the
 * reference member function it replaces (paths relative to src/lib/MeshFEM/).  The C++ facade
 * (include/MeshFEMHip/LinearElasticity.hh) and the Python mirror (meshfem_amd/) are thin
 * wrappers around exactly these symbols.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every host buffer, the library owns device memory
 *   - every function returns mfh_status (0 = ok); mfh_last_error(ctx) gives the message that the
 *     C++ facade rethrows as std::runtime_error (the reference's error convention)
 *   - Real = double everywhere (Types.hh:8); vector fields are interleaved [x0 y0 z0 x1 ...]
 *     (Fields.hh:15-17,49); local node order is MeshFEM/Gmsh order (Simplex.hh:30-47)
 *   - one context per host thread / device; no hidden global state (the reference's static
 *     HomogenousMaterialGetter material, LinearElasticity.hh:31-39,426-427, is per-context here)
 *   - "_dev" entry points take DEVICE pointers (HIP allocations, e.g. torch tensors) and enqueue on
 *     the context's stream; they exist for the multi-GPU driver that runs RCCL collectives between
 *     the local kernels
 */
#ifndef MESHFEM_HIP_H
#define MESHFEM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfh_ctx mfh_ctx;
typedef int32_t mfh_status;

enum {
    MFH_OK = 0,
    MFH_ERR_INVALID = 1,   /* bad argument / bad mesh (e.g. negatively oriented element) */
    MFH_ERR_STATE = 2,     /* call order violated (e.g. solve before mesh) */
    MFH_ERR_HIP = 3,       /* HIP runtime failure (no device, OOM, launch failure) */
    MFH_ERR_NOT_CONVERGED = 4,
    MFH_ERR_UNSUPPORTED = 5
};

/* assembly strategies (north_star: "colored or atomic" scatter, chosen by rocprof evidence) */
enum {
    MFH_ASSEMBLE_GATHER = 0, /* owner-computes row chunks, LDS accumulation, K written once    */
    MFH_ASSEMBLE_ATOMIC = 1  /* element-major, global_atomic_add_f64 scatter (baseline variant) */
};

/* Neumann condition kinds (BoundaryConditions.hh NeumannType; LinearElasticity.hh:908-931) */
enum { MFH_NEUMANN_TRACTION = 0, MFH_NEUMANN_PRESSURE = 1, MFH_NEUMANN_FORCE = 2 };

/* operator assembled into K. The scalar operators run on the same machinery with 1x1 blocks: one variable per
 * DoF, vectors of length nDoF, `mfh_element_stiffness` gives npe x npe matrices, Dirichlet boxes use value[0]
 * (PoissonMesh::applyBoundaryConditions, Poisson.hh:57-89), `mfh_sim_solve(f = NULL)` solves with a zero
 * right-hand side (Poisson.hh:91-117).
 *   MFH_OP_LAPLACIAN  int grad phi_i . grad phi_j   (Laplacian::construct, Laplacian.hh:27-57; full degree)
 *   MFH_OP_MASS       int phi_i phi_j               (MassMatrix::construct, MassMatrix.hh:50-86; not lumped)
 *   MFH_OP_MASS_VECTOR  the mass matrix on interleaved displacement vectors (MassMatrix::construct_vector_valued, MassMatrix.hh:131-147):
 *                     dim variables per DoF like elasticity, block (i, j) = m_ij I_dim. ONE double per block is stored and assembled
 *                     (pattern, gather lists and values are MFH_OP_MASS's); mfh_apply_K / mfh_dev_spmv / mfh_solve multiply through
 *                     k_spmv_kron (8 bytes of matrix per block instead of 8 dim^2), Jacobi-preconditioned (the scalar diagonal for all
 *                     components); mfh_export_upper_triplets gives the reference's entries (dim i + c, dim j + c, m_ij), c < dim -- the
 *                     components do not couple, so this is NOT the dense triangle of the blocks. A request for the two-level or
 *                     multigrid preconditioner falls back to Jacobi with a note (mfh_precond_info), as for the scalar operators; the
 *                     matrix-free operator does not apply; row-partitioned contexts refuse the operator.
 * The degree of the three scalar-valued operators follows mfh_set_operator_degree. */
enum { MFH_OP_ELASTICITY = 0, MFH_OP_LAPLACIAN = 1, MFH_OP_MASS = 2, MFH_OP_MASS_VECTOR = 3 };

/* preconditioners */
enum {
    MFH_PRECOND_BLOCK_JACOBI = 0, MFH_PRECOND_JACOBI = 1, MFH_PRECOND_NONE = 2,
    /* block-Jacobi + additive coarse correction on per-aggregate rigid-body modes (falls back to
     * block-Jacobi for partitioned rows and the scalar operators; see mfh_precond_info) */
    MFH_PRECOND_TWO_LEVEL = 3,
    /* p-multigrid V-cycle for quadratic elasticity: Chebyshev-smoothed quadratic level (matrix-free operator) -> linear level on the
     * same vertices (its assembled stiffness matrix IS the Galerkin operator: P1 is a subspace of P2) -> rigid-body modes of
     * aggregates, merged 2^dim at a time down to a dense inverse. Linear elements enter the same hierarchy at its linear level (their own
     * assembled K). Mesh-independent iteration counts (tens instead of hundreds); several right-hand sides share the coarse levels of every
     * V-cycle (option "mg_batch"). On a row-partitioned context (mfh_dist_solve, the preconditioner set on EVERY rank) the nodal levels are
     * partitioned like the mesh and the aggregate levels partitioned or replicated by size; scalar operators fall back to
     * MFH_PRECOND_TWO_LEVEL (see mfh_precond_info). Options "mg_steps_fine", "mg_steps_coarse", "mg_ratio_fine", "mg_ratio_coarse", "mg_agg_nodes". */
    MFH_PRECOND_MULTIGRID = 4,
    /* the drivers' default: MFH_PRECOND_MULTIGRID unless the mesh as a whole is stretched by more than option "auto_stretch_max" (default 8:
     * sqrt of the ratio of the extreme eigenvalues of the mesh's edge covariance sum_e sum_edges e e^T, reduced on the device -- 1 for an isotropic
     * mesh whatever the shapes of its elements, s for a mesh stretched s : 1 : 1), where MFH_PRECOND_TWO_LEVEL is the faster one (measured
     * crossover, docs/design/04_4c_multigrid.md). The reference's direct solve knows no such cliff (SparseMatrices.hh:1984-2296); the choice is
     * made when a solve prepares itself and again after new vertices; mfh_precond_choice reads it. */
    MFH_PRECOND_AUTO = 5
};

typedef struct mfh_solve_info {
    int32_t iterations;      /* PCG iterations of the last right-hand side          */
    int32_t converged;       /* 1 if ||r||/||b|| <= rtol                            */
    double  rel_residual;    /* recurrence residual ||r||_2 / ||b||_2 at exit       */
    double  true_rel_residual; /* ||b - A x||_2 / ||b||_2 recomputed at exit        */
    double  solve_ms;        /* device time of the PCG loop (HIP events), last RHS  */
    double  setup_ms;        /* device time of rhs/preconditioner setup             */
    int32_t used_graph;      /* 1 if the PCG iterations were replayed from a captured hipGraph */
    int32_t reserved;
} mfh_solve_info;

typedef struct mfh_timing {
    double symbolic_ms;      /* host: BSR pattern + gather/scatter maps (once per mesh/DoF map) */
    double geometry_ms;      /* device: element embedding kernel (a1)                           */
    double assemble_ms;      /* device: last numeric assembly launch (a4+a6+a9)                 */
    double upload_ms;        /* host->device copies of the last mesh_set/build                  */
} mfh_timing;

/* ---------------------------------------------------------------- context
 * device >= 0: HIP device ordinal (fails with MFH_ERR_HIP when there is none: NO CPU fallback).
 * device == -1: host-only context; only the mesh / DoF-map / symbolic / boundary-condition host
 * logic works, every numeric entry point returns MFH_ERR_HIP. Used by the CPU test-suite.        */
mfh_status  mfh_create(int32_t device, mfh_ctx** out);
void        mfh_destroy(mfh_ctx* ctx);
const char* mfh_last_error(const mfh_ctx* ctx);
const char* mfh_version(void);
/* the HIP stream all work of this context is enqueued on (a hipStream_t) */
void*       mfh_stream(mfh_ctx* ctx);
/* adopt a caller-owned hipStream_t (e.g. torch's current stream) so that the _dev entry points are
 * stream-ordered with the caller's own kernels and RCCL collectives; the context never destroys it */
mfh_status  mfh_set_stream(mfh_ctx* ctx, void* hipStream);

/* ---------------------------------------------------------------- mesh
 * mfh_mesh_build   == FEMMesh(elems, vertices) ctor (FEMMesh.inl:11-82): vertex nodes = vertices,
 *                     edge nodes numbered nVert+k in first-encounter order over (element, local
 *                     edge) (FEMMesh.inl:22-36), edge node = midpoint (FEMMesh.hh:228-233);
 *                     boundary elements/vertices/nodes in the reference's enumeration order
 *                     (TetMesh.inl:36-91, TriMesh.inl:86-118, FEMMesh.inl:39-59); embeds every
 *                     element (FEMMesh.hh:58-66 -> EmbeddedElement.hh:162-241) and fails with
 *                     MFH_ERR_INVALID on a negative volume (LinearElasticity.hh:465-472).
 * mfh_mesh_set     == the same with the node table supplied by the caller (no topology built:
 *                     boundary-condition helpers are unavailable). nOwned < nNode restricts K to
 *                     the first nOwned block rows (row-partitioned multi-GPU; halo nodes last).
 * dim in {2,3}; deg in {1,2}; simplices only (tri if dim==2, tet if dim==3).                  */
mfh_status mfh_mesh_build(mfh_ctx* ctx, int32_t dim, int32_t deg, int64_t nElem, int64_t nVert,
                          const int32_t* elemVerts /* nElem x (dim+1) */,
                          const double* vertPos /* nVert x dim */);
mfh_status mfh_mesh_set(mfh_ctx* ctx, int32_t dim, int32_t deg, int64_t nElem, int64_t nNode, int64_t nOwned,
                        const int32_t* elemNodes /* nElem x nodesPerElem, MeshFEM local order, any numbering */,
                        const double* nodePos /* nNode x dim (only corner-node positions enter the embedding) */);
mfh_status mfh_mesh_sizes(const mfh_ctx* ctx, int64_t* nElem, int64_t* nNode, int64_t* nVert,
                          int64_t* nBdryElem, int64_t* nBdryNode, int32_t* nodesPerElem,
                          int32_t* nodesPerBdryElem);
mfh_status mfh_mesh_get_elem_nodes(const mfh_ctx* ctx, int32_t* out /* nElem x nodesPerElem */);
/* == Simulator::updateMeshNodePositions (LinearElasticity.hh:1279-1284; FEMMesh::setNodePositions): new vertex positions
 * [nVert x dim] on the SAME connectivity. Elements are re-embedded at the next assembly / solve; topology, boundary
 * numbering, DoF map, sparsity pattern, gather lists and matrix-free lists are kept (they depend on connectivity only), so a
 * shape-optimisation step costs one vertex upload + geometry kernel + numeric assembly instead of a mesh rebuild.
 * Boundary areas / normals are recomputed; boundary-condition VALUES already stored (tractions of pressure regions) are
 * not, exactly like the reference. Contexts built by mfh_mesh_set (row-partitioned ones among them) pass the positions of ALL
 * their nodes [nNode x dim], halo nodes with the coordinates their owners hold; the exchange lists of mfh_dist_setup stay. */
mfh_status mfh_mesh_update_vertices(mfh_ctx* ctx, const double* vertPos);
mfh_status mfh_mesh_get_node_positions(const mfh_ctx* ctx, double* out /* nNode x dim */);
mfh_status mfh_mesh_get_boundary_elem_nodes(const mfh_ctx* ctx, int32_t* out /* nBE x npbe, volume node ids */);
mfh_status mfh_mesh_get_boundary_nodes(const mfh_ctx* ctx, int32_t* out /* nBdryNode volume node ids */);
/* the volume element each boundary element is a face / edge of (BoundaryElementHandle -> opposite simplex) */
mfh_status mfh_mesh_get_boundary_elem_parents(const mfh_ctx* ctx, int32_t* out /* nBE */);
/* BoundaryElementData::isInternal: 1 on the periodic cell boundary once a periodic condition is installed (else 0) */
mfh_status mfh_mesh_get_boundary_elem_internal(const mfh_ctx* ctx, uint8_t* out /* nBE */);
mfh_status mfh_mesh_get_boundary_elem_geometry(const mfh_ctx* ctx, double* volume /* nBE */,
                                               double* normal /* nBE x dim */);
mfh_status mfh_mesh_get_elem_volumes(mfh_ctx* ctx, double* out /* nElem */);

/* ---------------------------------------------------------------- materials
 * mfh_material_const       == HomogenousMaterialGetter / Materials::Constant::setTensor
 *                             (LinearElasticity.hh:31-39): one flattened D (flatLen x flatLen,
 *                             Voigt xx,yy,zz,yz,xz,xy, Flattening.hh:47-60; tensor shear, not
 *                             engineering) for every element.
 * mfh_material_isotropic   == ElasticityTensor::setIsotropic(E,nu) (ElasticityTensor.hh:100-134;
 *                             2D is plane stress), constant.
 * mfh_material_iso_field   == per-element E,nu (ETensorStoreGetter, LinearElasticity.hh:20-29;
 *                             Simulate_cli.cc:116-135).
 * mfh_material_ortho_field == per-element setOrthotropic3D/2D (ElasticityTensor.hh:136-164),
 *                             params per element: 3D Ex,Ey,Ez,nuYX,nuZX,nuZY,muYZ,muZX,muXY;
 *                             2D Ex,Ey,nuYX,muXY. The compliance inverse runs on the device; the element
 *                             record keeps only the normal block and the shear stiffnesses of D (192 B).
 * mfh_material_tensor_field== per-element flattened D (flatLen x flatLen each).
 * Per-element isotropic / orthotropic parameters that give an indefinite tensor (E <= 0, nu outside (-1, 1/2), a
 * compliance matrix that is not positive definite, a non-positive shear modulus) are reported with MFH_ERR_INVALID when
 * the elements are embedded (next assembly / solve): the reference inverts blindly and fails later in CHOLMOD.    */
mfh_status mfh_material_const(mfh_ctx* ctx, const double* D);
mfh_status mfh_material_isotropic(mfh_ctx* ctx, double E, double nu);
mfh_status mfh_material_iso_field(mfh_ctx* ctx, const double* E, const double* nu);
mfh_status mfh_material_ortho_field(mfh_ctx* ctx, const double* params);
mfh_status mfh_material_tensor_field(mfh_ctx* ctx, const double* D);
/* element e's flattened D as the kernels use it (flatLen x flatLen) */
mfh_status mfh_material_get(mfh_ctx* ctx, int64_t elem, double* D);

/* ---------------------------------------------------------------- DoF map
 * == Simulator::applyPeriodicConditions' m_dofForNode (LinearElasticity.hh:825-854):
 * variable index = dim*dofForNode[node] + c.  NULL restores DoF(node)=node.                    */
mfh_status mfh_dof_map(mfh_ctx* ctx, const int32_t* dofForNode /* nNode or NULL */, int64_t nDoF);
/* PeriodicCondition (BoundaryConditions.hh:452-561): builds dofForNode from the bounding-box cell
 * with tolerance eps, installs it, flags internal boundary elements; returns nDoF.             */
mfh_status mfh_apply_periodic_conditions(mfh_ctx* ctx, double eps, int64_t* nDoF);
mfh_status mfh_get_dof_map(const mfh_ctx* ctx, int32_t* dofForNode /* nNode */, int64_t* nDoF);
/* The same on a ROW-PARTITIONED context (mfh_mesh_set; periodic cell problems across GPUs): the rank's local nodes map to local DoFs numbered
 * owned-first -- the rows of K are the first nOwnedDoF DoFs -- and the halo DoFs after them grouped by owner rank; mfh_dist_setup then takes its
 * lists in DoF numbers (send: owned DoFs, receive ranges: cover the halo DoFs). Every element that touches a node of an owned DoF must be local. */
mfh_status mfh_dof_map_partitioned(mfh_ctx* ctx, const int32_t* dofForNode /* nNode */, int64_t nDoF, int64_t nOwnedDoF);

/* ---------------------------------------------------------------- assembly
 * mfh_assemble == Simulator::m_assembleStiffnessMatrix (LinearElasticity.hh:1408-1466) followed
 * by TripletMatrix::sumRepeated + CSC build (SparseMatrices.hh:280-374,422-447): perElementStiffness
 * (LinearElasticity.hh:165-232) for every element, summed into a device-resident block-CSR K
 * (dim x dim blocks, FULL symmetric storage, structural zeros kept).                           */
mfh_status mfh_assemble(mfh_ctx* ctx, int32_t mode);
/* The symbolic phase alone (block-CSR pattern + gather lists; implied by mfh_assemble). It is the
 * hoisted, once-per-mesh part of sumRepeated's sort/merge (SparseMatrices.hh:280-374).          */
mfh_status mfh_symbolic(mfh_ctx* ctx, int32_t withScatterMap);
mfh_status mfh_symbolic_sizes(const mfh_ctx* ctx, int64_t* nChunk, int64_t* nContrib, int32_t* chunkSlots, int32_t* maxRowLen);
/* introspection of the symbolic structure (tests): any pointer may be NULL; the gather lists are
 * only retained on the host with option "keep_host_symbolic" (always in a host-only context)    */
mfh_status mfh_symbolic_get(const mfh_ctx* ctx, int32_t* rowPtr, int32_t* colIdx, int32_t* chunkRow, int64_t* contribPtr,
                            uint32_t* contribCode, uint16_t* contribSlot, int32_t* scatterSlot);
mfh_status mfh_matrix_info(const mfh_ctx* ctx, int64_t* nBlockRows, int64_t* nBlockCols, int64_t* nnzBlocks);
/* Storage of K (option "matrix_storage"): *upperOnly = 1 when only the blocks (r, c >= r) are stored and assembled -- the triangle the
 * reference's TripletMatrix holds --, *storedBlocks = their number. mfh_matrix_info and mfh_export_bsr describe K itself either way. */
mfh_status mfh_matrix_storage(const mfh_ctx* ctx, int32_t* upperOnly, int64_t* storedBlocks);
mfh_status mfh_export_bsr(mfh_ctx* ctx, int32_t* rowPtr /* nBlockRows+1 */, int32_t* colIdx /* nnzb */,
                          double* vals /* nnzb x dim*dim, row-major blocks */);
/* == TripletMatrix after m_assembleStiffnessMatrix + sumRepeated: upper triangle (row<=col) in
 * column-major sorted order with exact zeros pruned (SparseMatrices.hh:231-234,370-373); same
 * content as TripletMatrix::dumpBinary (SparseMatrices.hh:629-645). Call with i=j=v=NULL to get
 * a sufficient capacity in *nnz (the structural entries of the triangle); otherwise *nnz is the
 * capacity on entry and the number of entries written on return.                               */
mfh_status mfh_export_upper_triplets(mfh_ctx* ctx, uint64_t* i, uint64_t* j, double* v, uint64_t* nnz);
/* per-element dense Ke (debug/parity): full symmetric (n*dim)^2 row-major, local dof = dim*node+c */
mfh_status mfh_element_stiffness(mfh_ctx* ctx, int64_t firstElem, int64_t count, double* Ke);


/* SPSDSystem<Real>(K) for a CALLER-SUPPLIED symmetric positive (semi-)definite matrix (SparseMatrices.hh:2332-2348;
 * python binding sparse_matrices.SPSDSystem, sparse_matrices.cc:47-57): upper-triangle triplets, repeated entries
 * summed. Replaces any mesh in the context; afterwards mfh_fix_variables / mfh_solve / mfh_apply_K /
 * mfh_export_* work on it (one scalar variable per row, Jacobi-preconditioned CG). */
mfh_status mfh_matrix_set_upper_triplets(mfh_ctx* ctx, int64_t n, int64_t nnz, const uint64_t* i, const uint64_t* j, const double* v);
/* ---------------------------------------------------------------- constrained solve
 * mfh_fix_variables == SPSDSystem::fixVariables (SparseMatrices.hh:2389-2500): variables (scalar
 * indices dim*dof+c) pinned to values; K_rf u_f moves to the right-hand side (:2457-2470). Calls
 * accumulate like the reference; fixing a variable twice is an error ("Variable already fixed.").
 * mfh_solve == SPSDSystem::solve (SparseMatrices.hh:2515-2606) with CHOLMOD replaced by a HIP
 * preconditioned CG on the free variables; u holds fixed values at fixed variables (:2592-2605).
 * f/u: nrhs vectors of dim*nDoF doubles each.                                                  */
mfh_status mfh_clear_fixed(mfh_ctx* ctx);
mfh_status mfh_fix_variables(mfh_ctx* ctx, int64_t n, const int64_t* vars, const double* vals /* or NULL = 0 */);
mfh_status mfh_set_preconditioner(mfh_ctx* ctx, int32_t kind);
/* coarse-space facts of the last two-level setup: aggregates, coarse dimension, setup time (ms); note = why it fell back (or "") */
/* the preconditioner in use (for MFH_PRECOND_AUTO: the choice made for the mesh in hand -- made now if it has not been), whether it was chosen
 * automatically, and the stretch of the mesh the choice looked at (-1: not computed) */
mfh_status mfh_precond_choice(mfh_ctx* ctx, int32_t* kind, int32_t* isAuto, double* meshStretch);
mfh_status mfh_precond_info(const mfh_ctx* ctx, int32_t* nAggregates, int64_t* coarseDim, double* setup_ms, const char** note);
/* the hierarchy MFH_PRECOND_MULTIGRID built at the last solve: DoFs of the quadratic and of the linear level, the largest eigenvalues
 * of their Jacobi-preconditioned operators (the Chebyshev smoothers' upper bounds), setup time; zeros when it is not in use. On
 * linear elements there is no quadratic level: fineDoF == coarseDoF and lambdaMaxFine == 0. */
mfh_status mfh_multigrid_info(const mfh_ctx* ctx, int64_t* fineDoF, int64_t* coarseDoF, double* lambdaMaxFine, double* lambdaMaxCoarse,
                              double* setup_ms);
mfh_status mfh_solve(mfh_ctx* ctx, int32_t nrhs, const double* f, double* u,
                     double rtol, int32_t maxit, mfh_solve_info* info /* ONE entry: the last right-hand side */);
/* the same with one mfh_solve_info per right-hand side. Where batches pay, right-hand sides are solved in batches (3D: 6 or 2, 2D: 3), like
 * the reference factors once and back-substitutes per right-hand side (PeriodicHomogenization.hh:34-54): under MFH_PRECOND_MULTIGRID the
 * coarse levels of every V-cycle serve the whole batch (option "mg_batch", default on); the Chronopoulos-Gear batches of the other
 * preconditioners (option "batch_rhs") are off by default (measured slower). info[k].reserved = size of the batch rhs k was solved in;
 * info[k].solve_ms of a batch is the batch's device time. */
mfh_status mfh_solve_batch(mfh_ctx* ctx, int32_t nrhs, const double* f, double* u,
                           double rtol, int32_t maxit, mfh_solve_info* info /* nrhs entries */);
/* == Simulator::applyStiffnessMatrix (LinearElasticity.hh:801-823), using the assembled K       */
mfh_status mfh_apply_K(mfh_ctx* ctx, const double* u /* dim*nDoF */, double* Ku);

/* ---------------------------------------------------------------- Simulator-level helpers
 * Box regions are inclusive (BBox::containsPoint, Geometry.hh:276-279).
 * mfh_bc_dirichlet_box == DirichletCondition branch of applyBoundaryConditions (:939-949): every
 *   BOUNDARY NODE whose position lies in the box gets `value` on the components in compMask
 *   (bit c = component c); conflicting values (>1e-10) fail (LinearElasticity.hh:386-406).
 * mfh_bc_neumann_box == NeumannCondition branch (:897-933): every BOUNDARY ELEMENT whose vertex
 *   barycentre lies in the box; FORCE divides by the region area; PRESSURE uses value[0].
 * relative != 0 interprets the corners relative to the mesh bounding box ("box%",
 *   BoundaryConditions.cc:310-316).                                                             */
mfh_status mfh_bc_clear(mfh_ctx* ctx);
mfh_status mfh_bc_dirichlet_box(mfh_ctx* ctx, const double* minCorner, const double* maxCorner,
                                int32_t relative, const double* value, int32_t compMask);
mfh_status mfh_bc_neumann_box(mfh_ctx* ctx, const double* minCorner, const double* maxCorner,
                              int32_t relative, const double* value, int32_t kind);
/* == DirichletNodesCondition branch (:991-1002) and the carrier of expression-valued Dirichlet regions (ExpressionVector
 * components are evaluated per node by the caller): per-node displacement values [n x dim]; "Condition applied to
 * non-boundary node i" and "Conflicting dirichlet displacements." as in the reference. */
mfh_status mfh_bc_dirichlet_nodes(mfh_ctx* ctx, int64_t n, const int64_t* nodes, const double* values, int32_t componentMask);
/* == NeumannElementsCondition branch (:966-990) after matching and the force / region-area division, and the carrier of
 * expression-valued traction regions: sets the traction [n x dim] of the listed boundary elements. */
mfh_status mfh_bc_neumann_elements(mfh_ctx* ctx, int64_t n, const int64_t* bdryElems, const double* tractions);
mfh_status mfh_bc_delta_force(mfh_ctx* ctx, int64_t node, const double* force);
/* == m_getDirichletVarsAndValues (:1469-1518). vars==NULL returns the count.                   */
mfh_status mfh_bc_dirichlet_vars(mfh_ctx* ctx, int64_t* vars, double* vals, int64_t* n);
/* == m_pinNode (:1595-1618): first non-boundary node, else node 0.                             */
mfh_status mfh_pin_node(const mfh_ctx* ctx, int64_t* node);
/* == Simulator::neumannLoad (:703-717); out: dim*nDoF                                          */
mfh_status mfh_neumann_load(mfh_ctx* ctx, double* out);
/* == Simulator::constantStrainLoad (:551-562, :135-162); cstrain flattened (flatLen, TENSOR shear) */
mfh_status mfh_constant_strain_load(mfh_ctx* ctx, const double* cstrainFlat, double* out);
/* Volume loads (docs/design/04_14_volume_loads.md). Both gather over the (element, local node) pairs of every DoF in a fixed order -- ascending by
 * element, the images of a periodic DoF in one list -- and write every entry of out once: no floating-point atomics, the same call on the same
 * context returns the same bits, and out needs no zeroing by the caller (a DoF without elements gets 0).
 * flags: MFH_LOAD_ADD        out += the load (out holds dim*nDoF values on entry) instead of out = the load
 *        MFH_LOAD_ON_DEVICE  every array is a device pointer; the call returns after the context's stream is synchronised (as for mfh_mass_lumped)
 * MFH_ERR_STATE: no mesh (also: a matrix from mfh_matrix_set_upper_triplets); MFH_ERR_UNSUPPORTED: a row-partitioned context (nOwned < nNode: the
 * elements of other ranks are missing at the interface, as for mfh_vertex_average); MFH_ERR_INVALID, before anything is written: an unknown kind,
 * a null array that the kind needs, stressOut with MFH_FIELD_LOAD_STRESS, a density entry that is negative or not finite (a host array is scanned on
 * the host; a device array, MFH_LOAD_ON_DEVICE, by a reduction kernel on the device before the load kernel is launched).
 *   mfh_body_force_load   f_i = sum_e density_e int_e phi_i b (no counterpart in the reference: gravity, centrifugal and inertial forces). kind
 *                         MFH_BODY_CONSTANT: b is one vector [dim] (always a host pointer); MFH_BODY_ELEMENT: [nElem][dim], constant per element;
 *                         MFH_BODY_NODE: [nNode][dim], interpolated with the mesh's shape functions (the element mass coefficients int phi_i phi_j).
 *                         density: [nElem] or NULL (= 1). The nodal weights int phi_i / vol of a quadratic element are 0 (triangle) and -1/20
 *                         (tet) at the vertices: the load of a vertex DoF may point against b (see mfh_mass_lumped).
 *   mfh_stress_field_load == Simulator::perElementStressFieldLoad (LinearElasticity.hh:564-577 over perElementConstantStressLoad :135-151):
 *                         f_i = sum_e sigma_e . int_e grad phi_i. field: [nElem][flatLen], TENSOR shear, the layout of mfh_average_stress.
 *                         MFH_FIELD_LOAD_STRESS: field is sigma_e; MFH_FIELD_LOAD_STRAIN: field is a strain and sigma_e = C_e : eps_e (for one strain
 *                         everywhere: mfh_constant_strain_load), stressOut (optional) receives C_e : eps_e -- what a caller subtracts from the
 *                         stress of the solution to get the thermal stress C : (eps(u) - eps_th). Elasticity operator only (MFH_ERR_UNSUPPORTED). */
enum { MFH_BODY_CONSTANT = 0, MFH_BODY_ELEMENT = 1, MFH_BODY_NODE = 2 };
enum { MFH_FIELD_LOAD_STRESS = 0, MFH_FIELD_LOAD_STRAIN = 1 };
enum { MFH_LOAD_ADD = 1, MFH_LOAD_ON_DEVICE = 2 };
mfh_status mfh_body_force_load(mfh_ctx* ctx, int32_t kind, const double* b, const double* density /* nElem or NULL */,
                               int32_t flags, double* out /* dim*nDoF */);
mfh_status mfh_stress_field_load(mfh_ctx* ctx, int32_t kind, const double* field /* nElem x flatLen */,
                                 double* stressOut /* nElem x flatLen or NULL; STRAIN kind only */,
                                 int32_t flags, double* out /* dim*nDoF */);
/* == Simulator::solve(f) (:479-487 -> m_buildConstrainedSystem :1377-1404): assembles if needed,
 * fixes the Dirichlet variables (+ the pin node if usePin), PCG-solves, returns dofToNodeField
 * (:664-677) as nNode x dim. f==NULL uses neumannLoad() (:657).                                */
mfh_status mfh_sim_solve(mfh_ctx* ctx, const double* f /* dim*nDoF or NULL */, int32_t usePin,
                         double* uNodes /* nNode x dim */, double rtol, int32_t maxit, mfh_solve_info* info);
/* Simulator::solve with ALL of assembleConstrainedSystem (LinearElasticity.hh:1201-1249). flags:
 *   MFH_SOLVE_PIN               m_useNRTPinConstraint: translations removed by pinning a node (:1595-1618) instead of rows
 *   MFH_SOLVE_NO_RIGID_MOTION   m_useRigidMotionConstraint (`no_rigid_motion` in .bc files): rotation rows (:1525-1566,
 *                               skipped under periodic conditions) + translation rows or pin; rigidMotionRHS optional
 *   MFH_SOLVE_ALLOW_ILL_POSED   allowIllPosed: Dirichlet variables only
 *   0                           default: analyzeDirichletPosedness (:1169-1190) adds translation constraints for the
 *                               components without any Dirichlet condition; "Unimplemented" if nothing is constrained.
 * The reference hands the resulting KKT system to UMFPACK; here the <= 6 constraint rows are eliminated around SPD
 * PCG solves (one consistent singular solve when they exactly remove the rigid motions, k + 1 solves otherwise). */
enum { MFH_SOLVE_PIN = 1, MFH_SOLVE_NO_RIGID_MOTION = 2, MFH_SOLVE_ALLOW_ILL_POSED = 4 };
mfh_status mfh_sim_solve_constrained(mfh_ctx* ctx, const double* f, int32_t flags, const double* rigidMotionRHS,
                                     int32_t nRigidRHS, double* uNodes, double rtol, int32_t maxit, mfh_solve_info* info);
/* Simulator::solve for nrhs load vectors on ONE constrained system -- what solveCellProblems does with its 3 / 6 constantStrainLoad vectors
 * (PeriodicHomogenization.hh:34-54: one Simulator, one factorisation, one back-substitution per load). f: nrhs x dim*nDoF, uNodes:
 * nrhs x nNode*dim, info: nrhs entries. Where the constraints leave a positive definite system (Dirichlet conditions, or periodic conditions
 * with the pinned node) the right-hand sides go through mfh_solve_batch's batches -- under MFH_PRECOND_MULTIGRID the linear / aggregate /
 * dense levels of every V-cycle are run once for the whole batch (option "mg_batch") --; systems with constraint rows are solved one
 * right-hand side after the other as by mfh_sim_solve_constrained. */
mfh_status mfh_sim_solve_batch(mfh_ctx* ctx, int32_t nrhs, const double* f, int32_t flags, double* uNodes, double rtol, int32_t maxit,
                               mfh_solve_info* info);
/* == solveCellProblems' loop (PeriodicHomogenization.hh:47-53): w[k] = Simulator::solve(constantStrainLoad(cstrains[k])) for k < nStrains on the
 * system the context's conditions describe (the caller has applied the periodic conditions; flags as for mfh_sim_solve_constrained:
 * MFH_SOLVE_PIN | MFH_SOLVE_NO_RIGID_MOTION is solveCellProblems' configuration). cstrains: nStrains x flatLen, flattened with TENSOR shear
 * like mfh_constant_strain_load's argument (the caller passes -e_ij); wNodes: nStrains x nNode*dim. Under MFH_PRECOND_MULTIGRID on a quadratic
 * mesh nothing but the solutions crosses the PCIe bus: the load vectors are formed on the device through the matrix-free operator's lists
 * (the element routine with u = 0 and the constant strain added), the right-hand sides share the coarse levels of every V-cycle (option
 * "mg_batch"), dofToNodeField runs on the device. Every other configuration takes the general route (host load vectors, mfh_sim_solve_batch). */
mfh_status mfh_solve_cell_problems(mfh_ctx* ctx, int32_t nStrains, const double* cstrains, int32_t flags, double* wNodes, double rtol,
                                   int32_t maxit, mfh_solve_info* info);
/* == averageStrainField / averageStressField (:528-549, :99-123): per element, flattened (flatLen) */
mfh_status mfh_average_strain(mfh_ctx* ctx, const double* uNodes, double* strain /* nElem x flatLen */);
mfh_status mfh_average_stress(mfh_ctx* ctx, const double* uNodes, double* stress /* nElem x flatLen */);
/* sum_e vol_e C_e : (averageStrain_e(u) + cstrain)  [flatLen values]: the element loop of homogenizedElasticityTensor
 * (PeriodicHomogenization.hh:72-100: Eh.DRow(i) = 1/|Y| sum_e vol_e [E_e : strain(w_i) + E_e.DRow(i)]) reduced on the device; cstrainFlat
 * (flattened, tensor shear entries; NULL = none) stands for the affine displacement of the probe strain e_i. */
mfh_status mfh_integrated_stress(mfh_ctx* ctx, const double* uNodes, const double* cstrainFlat, double* out /* flatLen */);
/* == strainField / stressField, elementStrain / elementStress (:493-526; Element::strain :99-117): the nodal values of the
 * degree-(Deg-1) strain interpolant of every element -- one value for P1, the values at the dim+1 corners for P2 (edge
 * nodes of an upsampled field are the means of their end points). out: [nElem][1 | dim+1][flatLen]. */
mfh_status mfh_strain_field(mfh_ctx* ctx, const double* uNodes, int32_t wantStress, double* out);
/* The same interpolant restricted to the boundary elements (restrictInterpolant, InterpolantRestriction.hh:29-66, as used
 * for the boundary stresses of PeriodicHomogenization.hh:316-340 and the integrand of homogenizedElasticityTensorGradient
 * :226-288): values of the parent element's strain at the boundary element's corners, in the boundary element's vertex
 * order. out: [nBE][1 | dim][flatLen]. */
mfh_status mfh_boundary_strain_field(mfh_ctx* ctx, const double* uNodes, int32_t wantStress, double* out);
/* ---- stress measures on the device (VonMises.hh vonMises; SymmetricMatrix.hh eigenvalues / eigenDecomposition;
 * FieldPostProcessing.hh vertexAveragedField). Symmetric matrices are flattened as the strain fields above: flatLen entries, TENSOR shear.
 * `what` is a mask of MFH_MEASURE_*; an output that is not requested may be NULL, a requested one that is NULL is MFH_ERR_INVALID:
 *   vonMises      one scalar per matrix: sqrt of the squared Frobenius norm of vonMisesExtractor<N>() : s, i.e. sqrt(3/2 dev s : dev s) in 3D
 *                 and the plane-stress value sqrt(s00^2 + s11^2 - s00 s11 + 3 s01^2) in 2D (VonMises.hh:10-46)
 *   eigenvalues   dim per matrix, ascending (the order of Eigen's SelfAdjointEigenSolver)
 *   eigenvectors  dim x dim per matrix, row-major, the unit eigenvector of eigenvalue k in COLUMN k (sign unspecified)
 * No atomics anywhere: every call returns the same bits. onDevice != 0 (as for the lumped mass above): every array argument is a device
 * pointer, and the call returns after the context's stream has been synchronised.
 *   mfh_sym_measures       a caller's field of n matrices [n][flatLen]; needs the context for its device and stream only (no mesh)
 *   mfh_stress_measures    the strain (wantStress: stress) of uNodes at the corners the strain field above is given at, fused: the
 *                          tensor is never stored. Outputs [nElem][NQ], [nElem][NQ][dim], [nElem][NQ][dim][dim], NQ = 1 | dim+1.
 *                          Preconditions and error codes of the strain field.
 *   mfh_vertex_average     C0 volume-weighted average of per-element corner values at the mesh vertices: out[v] = sum_e vol_e f(e, v) /
 *                          sum_e vol_e over the elements around v, accumulated in element order. field: [nElem][NQ][nComp] with NQ = dim+1
 *                          (perCorner != 0) or 1 (a per-element constant every corner takes); any nComp >= 1; out: [nVert][nComp]. The
 *                          vertex of a single element takes that element's value unchanged. MFH_ERR_UNSUPPORTED on a row-partitioned
 *                          context (nOwned < nNode): the elements of other ranks are missing at the interface vertices.
 *   mfh_vertex_averaged_strain  the same average of the strain / stress field of uNodes ([nVert][flatLen]); the field stays on the device
 *   mfh_peak_von_mises     max and argmax of the von Mises value over all corners, reduced on the device in two stages without writing a
 *                          field (uNodes, value, cornerIndex: host pointers). cornerIndex = element NQ + corner; ties go to the lowest
 *                          index; a NaN anywhere gives NaN with the index of the first NaN. */
enum { MFH_MEASURE_VON_MISES = 1, MFH_MEASURE_EIGENVALUES = 2, MFH_MEASURE_EIGENVECTORS = 4 };
mfh_status mfh_sym_measures(mfh_ctx* ctx, int32_t dim, int64_t n, const double* field, int32_t what, double* vonMises,
                            double* eigenvalues, double* eigenvectors, int32_t onDevice);
mfh_status mfh_stress_measures(mfh_ctx* ctx, const double* uNodes, int32_t wantStress, int32_t what, double* vonMises,
                               double* eigenvalues, double* eigenvectors, int32_t onDevice);
mfh_status mfh_vertex_average(mfh_ctx* ctx, const double* field, int32_t perCorner, int32_t nComp, double* out, int32_t onDevice);
mfh_status mfh_vertex_averaged_strain(mfh_ctx* ctx, const double* uNodes, int32_t wantStress, double* out, int32_t onDevice);
mfh_status mfh_peak_von_mises(mfh_ctx* ctx, const double* uNodes, int32_t wantStress, double* value, int64_t* cornerIndex);
/* ---- field sampler on the device (FieldSampler.hh: closestElementAndPoint, closestElementAndBaryCoords, closestNodeAndSqDist, contains,
 * sample; docs/design/04_11_field_sampler.md). Query points P: [nP][dim]. The index -- a uniform cell grid over the elements, sorted on the
 * device, and a second one over the boundary elements for the points outside the mesh -- is built on first use (or by mfh_sampler_build) and
 * dropped by mfh_mesh_build, mfh_mesh_set, mfh_mesh_update_vertices and option "sampler_cell_scale" (factor on the cell sizes, default 1).
 *   mfh_locate         elem[i]: the LOWEST-index element with min lambda >= -1e-12 at P[i] (contains(p, lambda, 1e-12)); bary: its barycentric
 *                      coordinates [nP][dim+1]; closest = P[i], sqDist = 0. A point no element contains: the closest point C of the boundary
 *                      under the total order (squared distance, boundary element index); elem = that boundary element's parent, bary = the
 *                      coordinates of C in it, closest = C, sqDist = |P[i] - C|^2. A point with a NaN or infinite coordinate, and a point
 *                      outside a mesh that has no boundary elements (mfh_mesh_set): elem -1 and NaN. Any output may be NULL.
 *   mfh_sample_field   the field at (elem, bary) (MeshFieldSampler::sample): field has nComp >= 1 interleaved components per row and one row per
 *                      vertex (sum_k B_k f(v_k)), per element (f(elem)) or per node (the degree's shape functions at bary); out: [nP][nComp];
 *                      NaN rows where elem = -1. (elem, bary) stay on the device between the two kernels.
 *   mfh_closest_node   the node of elem whose shape function is largest at bary (lowest local index on ties) and its squared distance to P[i];
 *                      node -1 and NaN where elem = -1. Either output may be NULL.
 * No floating-point atomics: the same call on the same context returns the same bits. onDevice as for mfh_mass_lumped: every array is a
 * device pointer and the call returns after the context's stream has been synchronised. nP = 0 is valid.
 * MFH_ERR_STATE: no mesh (or a matrix from mfh_matrix_set_upper_triplets); MFH_ERR_UNSUPPORTED: a row-partitioned context (nOwned < nNode);
 * MFH_ERR_INVALID: a kind that is not one of MFH_FIELD_*, nComp < 1, a NULL array that is needed. */
enum { MFH_FIELD_PER_VERTEX = 0, MFH_FIELD_PER_ELEMENT = 1, MFH_FIELD_PER_NODE = 2 };
typedef struct mfh_sampler_grid_info {
    int32_t built;                 /* 0: this grid has not been needed yet (every other member is 0) */
    int32_t cells[3];              /* cells per axis (1 along z in 2D) */
    int64_t items;                 /* elements / boundary elements */
    int64_t pairs;                 /* (cell, item) entries */
    int64_t max_cell_population;
    double build_ms;               /* host clock around the build, synchronised */
    double host_ms;                /* the part of build_ms spent in the host passes (bounding box, mean item extents) */
} mfh_sampler_grid_info;
typedef struct mfh_sampler_stats { mfh_sampler_grid_info elements, boundary; } mfh_sampler_stats;
mfh_status mfh_sampler_build(mfh_ctx* ctx);
mfh_status mfh_sampler_info(const mfh_ctx* ctx, mfh_sampler_stats* out);
mfh_status mfh_locate(mfh_ctx* ctx, int64_t nP, const double* P, int32_t* elem, double* bary, double* closest, double* sqDist, int32_t onDevice);
mfh_status mfh_sample_field(mfh_ctx* ctx, int64_t nP, const double* P, int32_t kind, const double* field, int32_t nComp, double* out,
                            int32_t onDevice);
mfh_status mfh_closest_node(mfh_ctx* ctx, int64_t nP, const double* P, int32_t* node, double* sqDist, int32_t onDevice);

/* ---- discrete shape derivatives, forward mode (LinearElasticity.hh:234-330 at element level; Simulator level
 * :1297-1374). deltaP is a per-vertex perturbation field [nVert x dim] (indexed by the node id of the element corners:
 * vertex nodes come first in the FEM numbering); nodal fields are held fixed. Each is the original device kernel
 * evaluated on perturbed barycentric gradients (delta grad lambda, EmbeddedElement.hh:269-278; delta vol/vol, :366-372).
 *   mfh_apply_delta_K               == Simulator::applyDeltaStiffnessMatrix(u, deltaP) (:1301-1328): (delta K) u,
 *                                      u per NODE, result per DoF; deltaPerElementStiffness (:306-330) is never formed
 *   mfh_delta_constant_strain_load  == Simulator::deltaConstantStrainLoad(cstrain, deltaP) (:1331-1348)
 *   mfh_delta_average_strain        == Simulator::deltaAverageStrainField(u, deltaU, deltaP) (:1364-1374):
 *                                      (delta strain)(u) + strain(deltaU); wantStress != 0 contracts with C (deltaStress :280-286)
 *   mfh_mutual_energies             sum_e int (e^ij + eps(w^ij)) : C : (e^kl + eps(w^kl)) dV as a flatLen x flatLen
 *                                      matrix (= |Y| Ch, energy form of PeriodicHomogenization.hh:146-186); with deltaP != NULL
 *                                      its discrete shape derivative in the volume form of PeriodicHomogenization.hh:484-491
 *                                      (what deltaHomogenizedElasticityTensor :492-514 evaluates through boundary integrals).
 *                                      w: [flatLen][nNode][dim] per-node fluctuation displacements. */
mfh_status mfh_apply_delta_K(mfh_ctx* ctx, const double* uNodes, const double* deltaP, double* out /* dim*nDoF */);
mfh_status mfh_delta_constant_strain_load(mfh_ctx* ctx, const double* cstrainFlat, const double* deltaP, double* out /* dim*nDoF */);
mfh_status mfh_delta_average_strain(mfh_ctx* ctx, const double* uNodes, const double* deltaU, const double* deltaP,
                                    int32_t wantStress, double* out /* nElem x flatLen */);
mfh_status mfh_mutual_energies(mfh_ctx* ctx, const double* w, const double* deltaP /* or NULL */, double* out /* flatLen^2 */);
/* == homogenizedElasticityTensorDiscreteDifferential (PeriodicHomogenization.hh:372-480) before its division by |Y|:
 * the exact derivative of every mutual energy with respect to every vertex coordinate (reverse mode: all directions in
 * one element sweep). out: [pair][nVert][dim], pair = row-major index over the upper triangle ij <= kl of the
 * flatLen x flatLen tensor (flatLen (flatLen + 1) / 2 pairs). Contracting it with a perturbation field reproduces
 * mfh_mutual_energies(w, deltaP). */
mfh_status mfh_mutual_energy_differential(mfh_ctx* ctx, const double* w, double* out);
/* Select the operator (default MFH_OP_ELASTICITY). Keeps mesh, DoF map, pattern and gather lists; drops the
 * assembled values and the fixed variables (their numbering depends on the block size). */
mfh_status mfh_set_operator(mfh_ctx* ctx, int32_t op);
/* PoissonMesh::gradUAverage (Poisson.hh:121-131): per-element average gradient of a scalar nodal field (any operator may be selected:
 * this is the `gradient` of the reference's differential_operators module) */
mfh_status mfh_average_gradient(mfh_ctx* ctx, const double* uNodes /* nNode */, double* grad /* nElem x dim */);
/* Forced degree of MFH_OP_LAPLACIAN / MFH_OP_MASS / MFH_OP_MASS_VECTOR: 0 (default) the mesh's own, 1 = degree 1 on the vertices of a quadratic
 * mesh (Laplacian::construct<1>, MassMatrix::construct<1>, NodeGetter<1,...> MassMatrix.hh:38-46; vertex node = vertex, FEMMesh.inl:17-37). The
 * operators are then assembled from the corner nodes of every element on a P1 VIEW of the context: a pattern of its own on the vertex graph,
 * the context's device vertex positions, the corner columns of its node table and its element records -- no second mesh build. While the
 * view is in force mfh_symbolic / mfh_symbolic_sizes / mfh_assemble / mfh_matrix_info / mfh_matrix_storage / mfh_export_* / mfh_apply_K /
 * mfh_dev_spmv / mfh_element_stiffness /
 * mfh_fix_variables / mfh_clear_fixed / mfh_solve / mfh_solve_batch / mfh_mass_lumped work on it (nVert rows, vectors of nVert or dim nVert doubles);
 * selecting MFH_OP_ELASTICITY is MFH_ERR_STATE. Back at 0 the full-degree pattern and values are as they were. A no-op on linear meshes;
 * needs a mesh from mfh_mesh_build with the identity DoF map, all rows owned. */
mfh_status mfh_set_operator_degree(mfh_ctx* ctx, int32_t degree /* 0 | 1 */);
/* Lumped mass matrix (MassMatrix::construct(..., lumped = true), MassMatrix.hh:104-127): the row sums of the FULL symmetric mass matrix of the
 * operator (MFH_OP_MASS: nNode values of the degree view; MFH_OP_MASS_VECTOR: dim times that, every row sum repeated dim times), summed on the
 * device over the stored values (k_row_sums; with the upper-triangle storage an off-diagonal entry counts for both rows, :113-117).
 * onDevice != 0: diagOut is a device pointer. */
mfh_status mfh_mass_lumped(mfh_ctx* ctx, double* diagOut, int32_t onDevice);
/* `divergence` of the reference's differential_operators module (differential_operators.cc:79-88): out[n] = sum over the elements e that
 * contain node n of v_e . int_e grad phi_n, for a per-element vector field [nElem x dim]. Linear meshes only, like the reference
 * (MFH_ERR_UNSUPPORTED on quadratic ones). Gather form on the device, no atomics (k_divergence). */
mfh_status mfh_divergence(mfh_ctx* ctx, const double* elemVectors /* nElem x dim */, double* out /* nNode */);

/* ---------------------------------------------------------------- vibrational modes
 * The nev smallest eigenpairs of K x = lambda M x (1 <= nev <= 20): K the elasticity operator of the context, M = density (> 0) times the consistent
 * vector-valued mass matrix of the mesh's own degree (MassMatrix::construct_vector_valued; weighted by the per-element field of mfh_set_density when
 * one is set) -- the reference's
 * smallestNonzeroGenEigenpairsPSDKnownKernel (Eigensolver.hh; shift-invert Lanczos over CHOLMOD there). Here: LOBPCG on the device with the
 * context's preconditioner (docs/design/04_12_modes.md). lambda ascending; the rows of X are M-orthonormal, each with its entry of largest
 * modulus positive.
 *   flags == 0 (clamped): the fixed variables of the context (mfh_fix_variables; their values are taken as 0) are removed from the pencil and
 *     X is 0 there. They must leave no rigid motion free (MFH_ERR_UNSUPPORTED otherwise). Any DoF map mfh_solve accepts.
 *   MFH_MODES_FREE: no fixed variables and the identity DoF map (MFH_ERR_UNSUPPORTED otherwise). The 6 (3D) / 3 (2D) rigid-body modes are a known
 *     kernel: the iteration runs in their M-orthogonal complement and returns the smallest NON-ZERO eigenvalues. The preconditioner is the one
 *     the rigid-motion-constrained solve uses on its singular K (multigrid with the dense level pinned; block-Jacobi in place of two-level:
 *     info->note says so).
 * A mode counts as converged at ||K x - lambda M x||_2 / (lambda ||M x||_2) <= rtol (written to residuals, may be null). maxit reached:
 * MFH_ERR_NOT_CONVERGED with the outputs filled, like mfh_solve_batch. K and M are resident together (the mass values live in a buffer of their own
 * beside K's; mfh_set_operator is not involved). The product with M needs both triangles of the pattern: on a context that stores the upper one
 * (quadratic elasticity by default) the call re-runs the symbolic phase with both for its own duration -- info->note says so, option
 * "matrix_storage" is not changed and the next call of any other entry point sees the storage it would have seen. Unpartitioned contexts,
 * elasticity, not under the forced-degree-1 view (MFH_ERR_UNSUPPORTED). */
enum { MFH_MODES_FREE = 1 };
typedef struct mfh_modes_info {
    int32_t converged, iterations, nLocked, precondUsed, blockSize, restarts;   /* precondUsed: the MFH_PRECOND_* that was applied */
    double  maxResidual, solve_ms, setup_ms;
    const char* note;                                                            /* owned by the context, valid until its next call */
} mfh_modes_info;
mfh_status mfh_modes(mfh_ctx* ctx, int32_t nev, double density, int32_t flags, double rtol, int32_t maxit,
                     double* lambda /* nev */, double* X /* nev x dim*nDoF, row per mode */, double* residuals /* nev or NULL */,
                     mfh_modes_info* info);

/* More modes than one block holds (docs/design/04_19_many_modes.md): the nev smallest eigenpairs of K x = lambda M x in the M-orthogonal complement of
 * span(Q) -- and of the rigid-body modes under MFH_MODES_FREE -- computed batch by batch. Each batch is one run of mfh_modes' loop in the complement
 * of everything found so far: the finished batch is projected against the deflation set once more, M-orthonormalised and appended to it (hard
 * locking); the set (Q and M Q) stays on the device for the whole call, 2 (nLocked + nev) ld 8 bytes beside the ten blocks of the loop
 * (ld = dim nDoF rounded up to 32), and the projections run through two kernels made for "many locked columns x <= 24 active ones"
 * (k_deflate_gram, k_deflate_update). The block's guard columns seed the next batch's start block.
 *   Q (nLocked rows, host; NULL with nLocked 0): any full-rank set; zeroed on the fixed variables, made M-orthogonal to the rigid modes in the free
 *     case and M-orthonormalised at entry (MFH_ERR_INVALID if its Gram matrix is not positive definite -- this one refusal is found on the device,
 *     after the set-up; the context is left as after any other call). The X of one call as the Q of the next continues a run.
 *   batch (0: 16): modes per batch. A batch that completes nev runs to rtol, every earlier one -- and every one when lambdaMax is set -- to
 *     rtol lockFactor (0: 0.1): the residuals of locked vectors are a floor for the modes found after them.
 *   lambdaMax (> 0 and finite; otherwise none): stop after the first batch that returns an eigenvalue above it and return only those <= lambdaMax
 *     (info->nFound of them, info->bandExhausted = 1; nev reached first: bandExhausted = 0).
 * Outputs: lambda ascending over the whole call (a mode of a later batch that sorts before an earlier batch's largest by more than rtol -- a mode
 * the earlier batch missed, not the other member of a multiple eigenvalue -- counts in info->nOutOfOrder and is named in info->note), rows of X
 * M-orthonormal with mfh_modes' sign rule; rows from info->nFound on are zero. residuals (may be NULL) and info->maxResidual are the FULL
 * residuals ||r|| / (lambda ||M x||), r = K x - lambda M x recomputed from K x after the last batch and not projected against anything the call
 * itself locked; with a Q from the caller, which need not span an invariant subspace, r is that of the restricted pencil, r - M Q (Q^T r) (an
 * eigenvector of the restricted pencil has K x - lambda M x = M Q mu, not 0), in the loop as in the final pass. converged = all <= rtol,
 * otherwise MFH_ERR_NOT_CONVERGED with everything filled -- also when a batch stops at maxit: then nFound counts the batches up to and including
 * that one. info->maxLockDefect = the largest |Q^T M x| a finished batch showed before its last projection.
 * With nLocked = 0, nev <= batch and no lambdaMax the call is mfh_modes' and returns its bits (residuals included).
 * Refusals: what mfh_modes refuses (MFH_ERR_UNSUPPORTED / MFH_ERR_STATE); MFH_ERR_INVALID for counts out of range, nev + nLocked (+ 6 | 3 rigid
 * modes) beyond the dimension of the pencil, an entry of Q that is not finite, lockFactor outside (0, 1], rtol <= 0, density <= 0, maxit <= 0 --
 * all of these before any device work. */
typedef struct mfh_modes_many_params {
    int32_t nev;         /* modes wanted, 1 .. 256 - nLocked */
    int32_t nLocked;     /* rows of Q, 0 .. 255 */
    int32_t batch;       /* modes per batch, 1 .. 20; 0 = 16 */
    int32_t flags;       /* 0 | MFH_MODES_FREE */
    int32_t maxit;       /* per batch */
    int32_t reserved;    /* 0 */
    double  density, rtol;
    double  lambdaMax;   /* stop once the band [0, lambdaMax] is exhausted; +inf or <= 0: none */
    double  lockFactor;  /* batches that will be locked run to rtol * lockFactor; 0 = 0.1; (0, 1] */
} mfh_modes_many_params;
typedef struct mfh_modes_many_info {
    int32_t converged, nFound, batches, iterations, restarts, precondUsed;
    int32_t bandExhausted, nOutOfOrder;
    double  maxResidual, maxLockDefect, solve_ms, setup_ms;
    const char* note;                                                            /* owned by the context, valid until its next call */
} mfh_modes_many_info;
/* A converged call leaves the columns it found on the device (nLocked + nev columns of dim*nDoF doubles, arena memory) for
 * mfh_modal_set_basis_from_modes, until the context's next mfh_modes_many, a new mesh or a DoF map. */
mfh_status mfh_modes_many(mfh_ctx* ctx, const mfh_modes_many_params* params, const double* Q /* nLocked x dim*nDoF, host, or NULL */,
                          double* lambda /* nev */, double* X /* nev x dim*nDoF */, double* residuals /* nev or NULL */, mfh_modes_many_info* info);

/* ---------------------------------------------------------------- transient dynamics
 * Implicit Newmark time stepping of M u'' + C u' + K u = g(t) f on the device (docs/design/04_13_dynamics.md): K the elasticity operator of the
 * context, M = density times the consistent vector-valued mass matrix of the mesh's own degree, C = rayleighMass M + rayleighStiff K, the fixed
 * variables of the context (mfh_fix_variables; their values are taken as 0) held at zero -- their set may be empty. The reference has no time
 * integrator. With beta > 0, gamma >= 1/2 every step solves
 *     (cK K + cM M) u+ = g+ f + M (u~ / (beta dt^2)) + C (gamma / (beta dt) u~ - v~),    u~ = u + dt v + dt^2 (1/2 - beta) a,  v~ = v + dt (1 - gamma) a
 *     a+ = (u+ - u~) / (beta dt^2),   v+ = v~ + gamma dt a+,    cK = 1 + gamma rayleighStiff / (beta dt),  cM = density (1 / (beta dt^2) + gamma rayleighMass / (beta dt))
 * by PCG from the start vector u~ to ||r||_2 <= rtol ||b||_2 (the rule of mfh_solve) with the context's preconditioner: block-Jacobi on the diagonal
 * blocks of cK K + cM M itself; two-level / multigrid on K's hierarchy (cond <= 1 + cM / (cK lambda_1)); block-Jacobi of the sum in their place when
 * there are no fixed variables (K singular, the sum not) -- info->note says which. 2 beta < gamma is accepted (conditionally stable: info->note).
 *   u, v, a      dim*nDoF each: the state at step 0 in, the state after the last completed step out. Without MFH_DYN_HAVE_ACCEL a is not read:
 *                a0 comes from M a0 = g0 f - C v0 - K u0. Two calls chained through (u, v, a) with MFH_DYN_HAVE_ACCEL continue a run.
 *   f            the load shape (NULL: none); amplitude: g at the steps 0 .. nSteps (NULL: 1)
 *   probeVars    nProbe variables whose displacement is recorded at every step: probeOut[(nSteps+1) x nProbe]
 *   snapshots    the displacement at the steps 0, stride, 2 stride, ...: (nSteps/stride + 1) x dim*nDoF (NULL: none)
 *   energies     with MFH_DYN_ENERGIES, per step {1/2 v.Mv, 1/2 u.Ku, g f.u}: one more product with M and with K per step
 * A step whose PCG reaches maxit: MFH_ERR_NOT_CONVERGED, info->stepsDone and the outputs of the steps completed (a failure in the solve for a0
 * writes nothing). MFH_ERR_INVALID before any device work: dt <= 0, beta <= 0, gamma < 1/2, density <= 0, a negative Rayleigh coefficient, a
 * probe variable out of range, energies without its flag. Like mfh_modes the call holds both triangles of the pattern for its own duration
 * (info->note); elasticity, the mesh's own degree, unpartitioned contexts (MFH_ERR_UNSUPPORTED). */
enum { MFH_DYN_HAVE_ACCEL = 1, MFH_DYN_ENERGIES = 2 };
typedef struct mfh_newmark_params {
    double dt, beta, gamma, density, rayleighMass, rayleighStiff, rtol;
    int32_t nSteps, maxit, snapshotStride, flags;
} mfh_newmark_params;
typedef struct mfh_newmark_info {
    int32_t stepsDone, iterationsTotal, iterationsMax, iterationsInit, precondUsed;   /* PCG iterations of the steps / of the worst step / of the solve for a0 */
    double cK, cM, solve_ms, setup_ms;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_newmark_info;
mfh_status mfh_newmark(mfh_ctx* ctx, const mfh_newmark_params* params,
                       double* u, double* v, double* a,          /* dim*nDoF each; state in, state after the last completed step out */
                       const double* f,                          /* dim*nDoF or NULL */
                       const double* amplitude,                  /* nSteps+1 or NULL (= 1) */
                       const int64_t* probeVars, int32_t nProbe, double* probeOut,  /* (nSteps+1) x nProbe */
                       double* snapshots,                        /* (nSteps/stride + 1) x dim*nDoF or NULL */
                       double* energies,                         /* (nSteps+1) x 3: kinetic, strain, g_n f.u_n; needs MFH_DYN_ENERGIES */
                       mfh_newmark_info* info);

/* ---------------------------------------------------------------- explicit dynamics
 * Central differences on the device (docs/design/04_20_explicit_dynamics.md) for wave propagation, impact and short pulses, where accuracy and not
 * stability sets the time step: M_L u'' + aR M_L u' + K u = g(t) f with M_L = density x the HRZ-lumped mass matrix. One step costs one product with K
 * and one pass over the vectors; no system is solved. Contexts as for mfh_newmark (elasticity, the mesh's own degree, unpartitioned), but the
 * pattern keeps its storage: only the K product of the context is used.
 *
 *   mfh_mass_lumped_hrz  HRZ (Hinton-Rock-Zienkiewicz) lumping: m_d = sum over the (element e, local node i) pairs of DoF d of rho_e vol_e w_i with
 *                        w_i = Mref_ii / trace(Mref) of the element type's consistent mass matrix -- the diagonal of an SPD matrix, so every mass is
 *                        positive on every element type (the row sums of mfh_mass_lumped are zero or negative at the vertices of quadratic elements)
 *                        and the total mass is exact. rho: the context's density field (mfh_set_density), 1 without one. diagOut: dim*nDoF values,
 *                        the value of a DoF repeated for its components; fixed variables are not masked. flags: 0, or MFH_LOAD_ON_DEVICE (diagOut is a
 *                        device pointer; the call returns after the context's stream is synchronised). The pairs of a DoF are added in a fixed
 *                        order: the same call returns the same bits. Contexts and refusals as for mfh_mass_apply.
 *   mfh_explicit_dt      the stability limit dt_crit = 2 / sqrt(lambda_max) of the pencil (K, density M_L) on the free variables, bracketed:
 *                        lambdaUpper >= lambda_max, guaranteed: max over the free variables d of (sum over the pairs (e, i) of d of the absolute
 *                                    row sum of row (i, c) of K_e) / m_d -- Gershgorin on M_L^-1 K, weakened by the triangle inequality;
 *                        lambdaEst  <= lambda_max: the last Rayleigh quotient of `iters` (0: 60) steps x <- M_L^-1 K x of a power iteration, normalised
 *                                    in M_L, from x0 (dim*nDoF, host; its fixed entries are ignored) or, with x0 NULL, from
 *                                    x0[i] = (((i + 1) * 2654435761 mod 2^32) >> 8) / 2^24 - 1/2.
 *                        dtSafe = 2 / sqrt(lambdaUpper) is stable for certain, dtEst = 2 / sqrt(lambdaEst) is an upper bound of dt_crit that is
 *                        close to it after enough steps. MFH_ERR_INVALID: density <= 0, iters < 0, a start vector with no positive quotient.
 *   mfh_explicit         the velocity-Verlet form, state (u, v, a) at integer steps so that calls chain like mfh_newmark's:
 *                            v(n+1/2) = v(n) + dt/2 a(n),   u(n+1) = u(n) + dt v(n+1/2),
 *                            a(n+1) = (M_L^-1 (g(n+1) f - K u(n+1)) - aR v(n+1/2)) / (1 + aR dt/2),   v(n+1) = v(n+1/2) + dt/2 a(n+1),
 *                        a(0) = M_L^-1 (g(0) f - K u(0)) - aR v(0) unless MFH_EXP_HAVE_ACCEL passes it. The fixed variables of the context are held at
 *                        zero (a zero in the inverse-mass vector); their set may be empty. u, v, a, f, amplitude, probeVars / probeOut and snapshots
 *                        as for mfh_newmark. energies: with MFH_EXP_ENERGIES, at the steps 0, energyStride (0: 1), 2 energyStride, ... the row
 *                        {1/2 v.M_L v, 1/2 u.K u, g f.u, 1/2 v(n+1/2).M_L v(n+1/2) + 1/2 u(n+1).K u(n)}: the last is the invariant the scheme
 *                        conserves exactly without load and damping (the last row's is formed with the half step that would follow).
 *                        Step-size policy: without MFH_EXP_NO_DT_CHECK the call runs the power iteration of mfh_explicit_dt (60 steps, default start
 *                        vector) and refuses dt > dtEst with MFH_ERR_INVALID -- such a step is unstable for certain; info carries lambdaEst, dtEst. An
 *                        iteration without a positive quotient (no free variable) is refused as by mfh_explicit_dt.
 *                        Either way the step kernel raises a device flag on a value that is not finite; the host reads it every 256 steps and then
 *                        returns MFH_ERR_NOT_CONVERGED with info->stepsDone = the last clean read, the probe and energy rows up to it, and u, v, a
 *                        left as they were passed. MFH_ERR_INVALID before any device work: dt <= 0, density <= 0, rayleighMass < 0, a negative stride
 *                        or step count, an unknown flag, a probe variable out of range, energies without its flag or the flag without the array.
 * No floating-point atomics in any of the three: the same call on the same context returns the same bits where the context's K product does. */
enum { MFH_EXP_HAVE_ACCEL = 1, MFH_EXP_ENERGIES = 2, MFH_EXP_NO_DT_CHECK = 4 };
typedef struct mfh_explicit_dt_info {
    double lambdaUpper, lambdaEst, dtSafe, dtEst;
    int32_t iterations, reserved;
    double ms;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_explicit_dt_info;
typedef struct mfh_explicit_params {
    double dt, density, rayleighMass;
    int32_t nSteps, snapshotStride, energyStride, flags;
} mfh_explicit_params;
typedef struct mfh_explicit_info {
    int32_t stepsDone, reserved;
    double lambdaEst, dtEst, solve_ms, setup_ms;                                       /* lambdaEst, dtEst: 0 under MFH_EXP_NO_DT_CHECK */
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_explicit_info;
mfh_status mfh_mass_lumped_hrz(mfh_ctx* ctx, double* diagOut /* dim*nDoF */, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_explicit_dt(mfh_ctx* ctx, double density, int32_t iters /* 0 = 60 */, const double* x0 /* dim*nDoF or NULL */, mfh_explicit_dt_info* info);
mfh_status mfh_explicit(mfh_ctx* ctx, const mfh_explicit_params* params,
                        double* u, double* v, double* a,          /* dim*nDoF each; state in, state after the last step out */
                        const double* f,                          /* dim*nDoF or NULL */
                        const double* amplitude,                  /* nSteps+1 or NULL (= 1) */
                        const int64_t* probeVars, int32_t nProbe, double* probeOut,  /* (nSteps+1) x nProbe */
                        double* snapshots,                        /* (nSteps/snapshotStride + 1) x dim*nDoF or NULL */
                        double* energies,                         /* (nSteps/energyStride + 1) x 4; needs MFH_EXP_ENERGIES */
                        mfh_explicit_info* info);

/* ---------------------------------------------------------------- frequency response
 * The steady state of M u'' + C u' + K u = Re(f^ e^{i w t}) on the device (docs/design/04_17_harmonic.md): for every frequency w of a list
 *     (K + i w C - w^2 M) u^(w) = f^,    C = rayleighMass M + rayleighStiff K,   plus the structural term i lossFactor K,
 * with K, M and the fixed variables (held at zero; their set may be empty for w > 0) as in mfh_newmark. The operator is the pencil
 *     Z(w) = zK K + zM M,    zK = 1 + i (lossFactor + w rayleighStiff),   zM = density (-w^2 + i w rayleighMass),
 * complex symmetric, solved by COCG (the PCG recurrence with the unconjugated x^T y) to the Hermitian ||r||_2 <= rtol ||f^||_2 with a real symmetric
 * positive-definite preconditioner applied to the real and the imaginary plane: the context's two-level / multigrid hierarchy of K, or the
 * block-Jacobi of K + w^2 density M (rebuilt per frequency) -- always the latter when there are no fixed variables; info->note says which. The
 * reference has no counterpart.
 *   omega        nFreq frequencies in rad per unit time, solved in this order; with MFH_HARM_WARM_START each starts from the previous solution
 *   fRe, fIm     the load, dim*nDoF each (fIm NULL: real); entries on fixed variables are ignored. f^ = 0 gives u^ = 0 without an iteration
 *   probeVars    nProbe variables: probeOut[nFreq x nProbe x {re, im}], gathered on the device
 *   fields       nFreq x {re plane, im plane} x dim*nDoF (NULL: none); zero on the fixed variables
 *   iterations, trueResiduals   per frequency (either may be NULL): COCG iterations, and ||f^ - Z u^||_2 / ||f^||_2 from one more product after
 *                convergence (the recurrence's residual drifts on undamped, indefinite systems)
 * A frequency that reaches maxit, or whose residual norm is not finite: MFH_ERR_NOT_CONVERGED, info->freqsDone and the outputs of the frequencies
 * completed; the rest is not written. MFH_ERR_INVALID before any device work: null params, a frequency that is negative or not finite, w = 0
 * without fixed variables, density <= 0, a negative Rayleigh coefficient or loss factor, rtol outside (0, 1), maxit <= 0, nFreq < 0, an unknown
 * flag, a probe variable out of range, probes without their output. Contexts as for mfh_newmark (MFH_ERR_UNSUPPORTED); like it the call holds both
 * triangles of the pattern for its own duration. */
enum { MFH_HARM_WARM_START = 1 };
typedef struct mfh_harmonic_params {
    double density, rayleighMass, rayleighStiff, lossFactor, rtol;
    int32_t nFreq, maxit, flags;
} mfh_harmonic_params;
typedef struct mfh_harmonic_info {
    int32_t freqsDone, iterationsTotal, iterationsMax, precondUsed;
    double worstTrueResidual, setupMs, solveMs;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_harmonic_info;
mfh_status mfh_harmonic(mfh_ctx* ctx, const mfh_harmonic_params* params,
                        const double* omega,                      /* nFreq, rad per unit time */
                        const double* fRe, const double* fIm,     /* dim*nDoF each; fIm may be NULL */
                        const int64_t* probeVars, int32_t nProbe, double* probeOut,  /* nFreq x nProbe x {re, im} */
                        double* fields,                           /* nFreq x {re plane, im plane} x dim*nDoF, or NULL */
                        int32_t* iterations,                      /* nFreq or NULL */
                        double* trueResiduals,                    /* nFreq or NULL */
                        mfh_harmonic_info* info);

/* ---------------------------------------------------------------- modal superposition
 * Frequency sweeps on a mode basis that stays on the device (docs/design/04_21_modal_superposition.md). With eigenpairs (lambda_j, phi_j) of
 * (K, density M), M-orthonormal, the response of mfh_harmonic's system is
 *     u^(w) = sum_j phi_j q_j(w) [+ r_s / zK(w)],   q_j = (phi_j^T f^) / d_j,
 *     d_j = lambda_j (1 + i (lossFactor + w rayleighStiff)) - w^2 + i w rayleighMass + 2 i zeta_j sqrt(lambda_j) w,
 * exact for the full basis; a truncated basis leaves the error mfh_modal_harmonic measures on request (MFH_MODAL_RESIDUALS). r_s is the static
 * correction (mode acceleration) u_s - sum_j phi_j (phi_j^T f^) / lambda_j with K u_s = f^, zK = 1 + i (lossFactor + w rayleighStiff).
 *   mfh_modal_set_basis    copies nModes (1 .. 256; 0 drops the basis and its memory) modes -- rows of X, dim*nDoF each, e.g. the output of
 *                          mfh_modes / mfh_modes_many at the same density -- to the device, zeroes their entries on the fixed variables and reports
 *                          info->orthoDefect = max |X (density M) X^T - I|. Nothing is refused on the defect. lambda[j] >= 0 (0: a rigid mode of
 *                          a free body). MFH_ERR_INVALID before any device work: a count out of range, density <= 0, an entry that is not
 *                          finite, a negative lambda. The basis belongs to the mesh, vertex positions, material, density field and the set of
 *                          fixed variables in force: after any of them changed the calls below return MFH_ERR_STATE until a basis is set again
 *                          (clearing the fixed variables and fixing the same set again keeps it; a new mesh or DoF map drops it).
 *   mfh_modal_coordinates  q = X (density M) u for nVec fields (rows of u): the modal coordinates of e.g. a Newmark snapshot
 *   mfh_modal_harmonic     the sweep. omega, fRe, fIm, probeVars, probeOut, fields as in mfh_harmonic; the density is the basis's.
 *                          modalDamping: nModes damping ratios zeta_j >= 0 or NULL; modalCoords: nFreq x nModes x {re, im} or NULL.
 *                          MFH_MODAL_STATIC_CORRECTION: one solve K u_s = f^ per non-zero load plane with the context's solver and preconditioner
 *                          at rtol / maxit (MFH_ERR_NOT_CONVERGED, nothing written, if one fails); needs fixed variables (MFH_ERR_UNSUPPORTED)
 *                          and lambda_j > 0 (MFH_ERR_INVALID). MFH_MODAL_RESIDUALS: trueResiduals[k] = ||f^ - Z(w_k) u^||_2 / ||f^||_2 with the
 *                          operator product of mfh_harmonic at every residualStride-th frequency (0: every one), -1 at the others; refused with
 *                          modalDamping (no operator to test against). Refusals otherwise as mfh_harmonic's, plus w = 0 with a zero lambda or
 *                          d_j = 0 and a negative zeta (MFH_ERR_INVALID), no basis or a stale one (MFH_ERR_STATE).
 * Device memory of a sweep beside the basis ((nModes + 2) columns): with fields or residuals, staging rows for 16 frequencies (one full pass of the
 * expansion kernel: 32 x dim*nDoF doubles, 5.7 GB at 22.3 M unknowns) or 256 MB, whichever is more; where that allocation fails the call falls back
 * to 256 MB (one row at least) and says so in info->note. Contexts as for mfh_harmonic. */
enum { MFH_MODAL_STATIC_CORRECTION = 1, MFH_MODAL_RESIDUALS = 2 };
typedef struct mfh_modal_basis_info {
    int32_t nModes, reserved;
    int64_t ld;                                                                        /* doubles between two columns on the device */
    double orthoDefect, deviceBytes, setupMs;
} mfh_modal_basis_info;
typedef struct mfh_modal_harmonic_params {
    double rayleighMass, rayleighStiff, lossFactor, rtol;
    int32_t maxit, nFreq, residualStride, flags;
} mfh_modal_harmonic_params;
typedef struct mfh_modal_harmonic_info {
    int32_t staticSolves, staticIterations, groups, planesPerPass;
    double worstTrueResidual, setupMs, solveMs;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_modal_harmonic_info;
mfh_status mfh_modal_set_basis(mfh_ctx* ctx, int32_t nModes, const double* lambda /* nModes */, const double* X /* nModes x dim*nDoF */,
                               double density, mfh_modal_basis_info* info);
/* the same basis without the host round trip: adopts the first nModes (1 .. what was found) modes, in ascending order of lambda, that the context's last
 * converged mfh_modes_many left on the device -- a device-to-device copy into the modal layout with the signs of the host copy, the fixed rows zeroed, the
 * same orthoDefect pass; every later modal result equals the round trip's bit for bit. mfh_modes_many keeps that set (nLocked + nev columns of
 * dim*nDoF doubles, counted by the device statistics) until its next call, a new mesh or a DoF map. MFH_ERR_STATE: no such set, or one made under other
 * vertex positions, material, density field or fixed variables (the rules of the basis itself). */
mfh_status mfh_modal_set_basis_from_modes(mfh_ctx* ctx, int32_t nModes, double density, mfh_modal_basis_info* info);
mfh_status mfh_modal_coordinates(mfh_ctx* ctx, const double* u /* nVec x dim*nDoF */, int32_t nVec, double* q /* nVec x nModes */);
/* *nModes = modes of the basis in place (0: none), *valid = 1 if the modal calls would accept it now (either may be NULL) */
mfh_status mfh_modal_basis_state(mfh_ctx* ctx, int32_t* nModes, int32_t* valid);
mfh_status mfh_modal_harmonic(mfh_ctx* ctx, const mfh_modal_harmonic_params* params,
                              const double* omega,                      /* nFreq, rad per unit time */
                              const double* modalDamping,               /* nModes or NULL */
                              const double* fRe, const double* fIm,     /* dim*nDoF each; fIm may be NULL */
                              const int64_t* probeVars, int32_t nProbe, double* probeOut,  /* nFreq x nProbe x {re, im} */
                              double* fields,                           /* nFreq x {re plane, im plane} x dim*nDoF, or NULL */
                              double* modalCoords,                      /* nFreq x nModes x {re, im}, or NULL */
                              double* trueResiduals,                    /* nFreq, or NULL */
                              mfh_modal_harmonic_info* info);
/* Modal transient response on the same basis (docs/design/04_22_modal_transient.md): the load g(t) f with amplitude[n] at t_n = n dt taken as piecewise
 * linear between the steps; every mode obeys
 *     q_j'' + c_j q_j' + lambda_j q_j = (phi_j^T f) a(t),   c_j = rayleighMass + rayleighStiff lambda_j + 2 zeta_j sqrt(lambda_j),
 * and is stepped exactly: [q ; q']_{n+1} = A_j [q ; q']_n + g_j (b0_j a_n + b1_j (a_{n+1} - a_n) / dt). No stability limit, no period error; with the
 * full basis the result is the exact solution of the semi-discrete system for that load. u(t_n) = sum_j phi_j q_j(n) [+ r_s a_n] with the static
 * correction r_s of mfh_modal_harmonic (real plane; MFH_MODAL_TR_STATIC_CORRECTION: one solve K u_s = f at rtol / maxit, needs fixed variables --
 * MFH_ERR_UNSUPPORTED -- and lambda_j > 0 -- MFH_ERR_INVALID; MFH_ERR_NOT_CONVERGED, nothing written, if it fails).
 *   q, qdot        nModes each: the state at step 0 in, the state after the last step out; both NULL: from rest, no state returned. Two calls
 *                  chained through them continue a run (the second call's amplitude[0] is the first's last value): row 0 of the second call equals
 *                  the last row of the first and everything after it equals the single call bit for bit, whatever chunkSteps is.
 *   probeOut       (nSteps+1) x nProbe, the displacement at the variables probeVars: bit for bit the snapshot entries
 *   snapshots      every snapshotStride-th step from step 0, dim*nDoF each, or NULL; modalCoords: (nSteps+1) x nModes or NULL
 *   energies       (nSteps+1) x {1/2 sum q_j'^2, 1/2 sum lambda_j q_j^2, a_n sum g_j q_j}: mfh_newmark's triple restricted to the retained modes; the
 *                  array and MFH_MODAL_TR_ENERGIES come together
 *   chunkSteps     steps the device takes per launch (0: the default; otherwise a positive multiple of 32): no influence on any result
 * MFH_ERR_INVALID before any device work: null params, dt <= 0 or not finite, a negative count or stride, a negative Rayleigh coefficient or zeta,
 * an unknown flag, a chunkSteps that is neither 0 nor a positive multiple of 32, only one of q / qdot, energies without their flag or the flag
 * without the array, snapshots without a stride, a probe variable out of range, an amplitude, load or state entry that is not finite.
 * MFH_ERR_STATE: no basis or a stale one, by the rules above. nSteps = 0 returns row 0 of every output. Contexts as for mfh_modal_harmonic. */
enum { MFH_MODAL_TR_STATIC_CORRECTION = 1, MFH_MODAL_TR_ENERGIES = 2 };
typedef struct mfh_modal_transient_params {
    double dt, rayleighMass, rayleighStiff, rtol;                                      /* rtol, maxit: the static solve */
    int32_t nSteps, maxit, snapshotStride, chunkSteps, flags, reserved;
} mfh_modal_transient_params;
typedef struct mfh_modal_transient_info {
    int32_t stepsDone, staticSolves, staticIterations, chunkSteps, chunks, reserved;
    double setupMs, marchMs, seriesMs, expandMs;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_modal_transient_info;
mfh_status mfh_modal_transient(mfh_ctx* ctx, const mfh_modal_transient_params* params,
                               const double* modalDamping,               /* nModes or NULL */
                               double* q, double* qdot,                  /* nModes each, or both NULL */
                               const double* f,                          /* dim*nDoF */
                               const double* amplitude,                  /* nSteps+1, or NULL (= 1) */
                               const int64_t* probeVars, int32_t nProbe, double* probeOut,  /* (nSteps+1) x nProbe */
                               double* snapshots,                        /* (nSteps/snapshotStride + 1) x dim*nDoF, or NULL */
                               double* modalCoords,                      /* (nSteps+1) x nModes, or NULL */
                               double* energies,                         /* (nSteps+1) x 3, or NULL */
                               mfh_modal_transient_info* info);
/* host only, no context: the eight coefficients {A11, A12, b0_q, b1_q, A21, A22, b0_v, b1_v} of one mode: the first two rows of
 * exp(dt [[0,1,0,0],[-lambda,-c,1,0],[0,0,0,1],[0,0,0,0]]), for lambda >= 0 (0: a rigid mode), c >= 0 (under-damped, critical, over-damped) and
 * dt > 0, each within a few ulps of its natural size (MFH_ERR_INVALID otherwise) */
mfh_status mfh_modal_transient_coeffs(double lambda, double c, double dt, double* out8);

/* Random vibration and response spectra on the same basis (docs/design/04_23_modal_random.md). Both reduce to a quadratic form per row of the basis
 * B = [Phi | r_1 | r_2]:  v_i = phi_i^T C phi_i for a symmetric positive semi-definite nb x nb matrix C. The host factors C = F F^T (mfh_psd_factor) and
 * the device forms v_i = sum_t (sum_j B_j[i] F_jt)^2 >= 0, one pass over the basis per 32 columns of F (kernel k_modal_sumsq).
 * Host only, no context:
 *   mfh_psd_factor        Cholesky with diagonal pivoting of the n x n (n <= 258) row-major matrix C, symmetry taken from the lower triangle. It stops
 *                         when the largest remaining diagonal is <= tol (tol < 0: n eps max diag, the rule of LAPACK's dpstrf). F: n x n row-major, its
 *                         first *rank columns written, row j belonging to row j of C (no permutation of the rows; the rows of the pivots chosen before
 *                         column t are exactly zero from column t on); piv: n entries, the first *rank the pivots in order (or NULL);
 *                         *truncation = the trace of the positive semi-definite remainder C - F F^T (or NULL): phi^T (C - F F^T) phi <= truncation |phi|^2.
 *                         MFH_ERR_INVALID: n out of range, an entry that is not finite, a remaining diagonal below -tol (C is not positive
 *                         semi-definite). A zero matrix has rank 0.
 *   mfh_modal_covariance  C^(p) = sum_k w_k omega_k^p Re(H_k S_k H_k^H), p = 0, 2, 4: the covariances of the coordinates of displacement, velocity and
 *                         acceleration under loads of one-sided cross-spectral density S (Hermitian, nLoad x nLoad per frequency, with respect to
 *                         omega). H_k = [g_ja / d_j(omega_k) ; delta_ab / zK(omega_k)], nb x nLoad, the second block (nLoad rows) only with
 *                         correction = 1; d_j, zK as for mfh_modal_harmonic. g: nModes x nLoad row-major (g = Phi^T f_a). weights: nFreq quadrature
 *                         weights or NULL (the trapezoid rule on omega; needs nFreq >= 2). C0, C2, C4: nb x nb row-major, nb = nModes + correction nLoad,
 *                         any may be NULL. Plain double precision; every entry is summed over k in grid order, so the bits do not depend on the number
 *                         of host threads. MFH_ERR_INVALID: omega not strictly ascending or negative; omega = 0 with a zero lambda; d_j = 0; an S_k that
 *                         is not Hermitian entry by entry to 8 eps max |S_k| or has a negative diagonal; a negative lambda, zeta or damping
 *                         coefficient; an entry or a sum that is not finite. MFH_ERR_UNSUPPORTED: correction with nLoad > 2. nLoad <= 8, nModes <= 256.
 *   mfh_cqc_matrix        rho_jk = 8 sqrt(zeta_j zeta_k) (zeta_j + r zeta_k) r^(3/2) / ((1 - r^2)^2 + 4 zeta_j zeta_k r (1 + r^2) + 4 (zeta_j^2 + zeta_k^2) r^2),
 *                         r = omega_k / omega_j (Der Kiureghian's correlation of the CQC rule, unequal damping), m x m row-major, exactly symmetric with
 *                         a unit diagonal. zeta_j > 0, lambda_j >= 0 (MFH_ERR_INVALID otherwise); two zero eigenvalues: 1 at equal zeta, else 0.
 * On the basis of mfh_modal_set_basis (MFH_ERR_STATE without a valid one; contexts as for mfh_modal_harmonic):
 *   mfh_modal_quadratic   sqrt(phi_i^T C_a phi_i) for nMat <= 4 symmetric nModes x nModes matrices (row-major, one after the other) over the modes:
 *                         into fields (nMat x dim*nDoF, or NULL) and at the probes (probeOut nMat x nProbe), the probes bit for bit the field entries.
 *                         The response-spectrum rules are this call with C_jk = rho_jk a_j a_k. tol: as for mfh_psd_factor. A matrix the
 *                         factorisation refuses: MFH_ERR_INVALID, nothing written.
 *   mfh_modal_random      the RMS response to loads sum_a A_a(t) f_a (f: nLoad x dim*nDoF real load shapes) whose amplitudes have the spectrum S.
 *                         rmsFields: sigma_u, then sigma_v with MFH_MODAL_RV_VELOCITY, then sigma_a with MFH_MODAL_RV_ACCELERATION, dim*nDoF each, or NULL;
 *                         probeRms: 4 x nProbe = {sigma_u, sigma_v, sigma_a (0 without its flag), nu0+ = sigma_v / (2 pi sigma_u), the rate of upward zero
 *                         crossings}; probePsd: nProbe x nFreq, the response spectrum H_p S H_p^H of each probe, or NULL; cov: 3 x nb x nb = C^(0), C^(2),
 *                         C^(4), or NULL. MFH_MODAL_RV_STATIC_CORRECTION: one static solve per load that is not zero, the residual vectors r_a in the two
 *                         reserved columns of the basis as mfh_modal_harmonic writes them; at most two loads with it (MFH_ERR_UNSUPPORTED). nLoad <= 8.
 *                         The static solves, the validity rules and the refusals are mfh_modal_harmonic's, plus those of mfh_modal_covariance. Nothing
 *                         field-sized is done beyond the load projections when no field is asked for. */
enum { MFH_MODAL_RV_STATIC_CORRECTION = 1, MFH_MODAL_RV_VELOCITY = 2, MFH_MODAL_RV_ACCELERATION = 4 };
typedef struct mfh_modal_quadratic_info {
    int32_t ranks[4], passes[4];                                                       /* per matrix: columns of F, passes over the basis */
    double truncation[4];
    double factorMs, solveMs;
} mfh_modal_quadratic_info;
typedef struct mfh_modal_random_params {
    double rayleighMass, rayleighStiff, lossFactor, rtol, tol;                         /* rtol, maxit: the static solves; tol: mfh_psd_factor's */
    int32_t maxit, nFreq, nLoad, flags;
} mfh_modal_random_params;
typedef struct mfh_modal_random_info {
    int32_t ranks[3], passes[3];                                                       /* of C^(0), C^(2), C^(4); 0 where none was factored */
    int32_t staticSolves, staticIterations, nb, reserved;
    double truncation[3];
    double covarianceMs, factorMs, solveMs;
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_modal_random_info;
mfh_status mfh_psd_factor(int32_t n, const double* C, double tol, double* F, int32_t* rank, int32_t* piv, double* truncation);
mfh_status mfh_modal_covariance(int32_t nModes, const double* lambda, const double* g /* nModes x nLoad */, int32_t nLoad,
                                double rayleighMass, double rayleighStiff, double lossFactor, const double* modalDamping /* nModes or NULL */,
                                int32_t nFreq, const double* omega, const double* weights /* nFreq or NULL */,
                                const double* S /* nFreq x nLoad x nLoad x {re, im} */, int32_t correction,
                                double* C0, double* C2, double* C4 /* nb x nb each, or NULL */);
mfh_status mfh_cqc_matrix(int32_t m, const double* lambda, const double* zeta, double* rho /* m x m */);
mfh_status mfh_modal_quadratic(mfh_ctx* ctx, int32_t nMat, const double* C /* nMat x nModes x nModes */, double tol,
                               const int64_t* probeVars, int32_t nProbe, double* probeOut /* nMat x nProbe */,
                               double* fields /* nMat x dim*nDoF, or NULL */, mfh_modal_quadratic_info* info);
mfh_status mfh_modal_random(mfh_ctx* ctx, const mfh_modal_random_params* params,
                            const double* omega,                      /* nFreq, strictly ascending */
                            const double* weights,                    /* nFreq or NULL */
                            const double* modalDamping,               /* nModes or NULL */
                            const double* f,                          /* nLoad x dim*nDoF */
                            const double* S,                          /* nFreq x nLoad x nLoad x {re, im} */
                            const int64_t* probeVars, int32_t nProbe, double* probeRms,  /* 4 x nProbe */
                            double* probePsd,                         /* nProbe x nFreq, or NULL */
                            double* rmsFields,                        /* (1 + velocity + acceleration) x dim*nDoF, or NULL */
                            double* cov,                              /* 3 x nb x nb, or NULL */
                            mfh_modal_random_info* info);

/* ---------------------------------------------------------------- modal stress recovery (docs/design/04_24_modal_stress.md)
 * RMS stress under the loads of mfh_modal_quadratic / mfh_modal_random, per element corner in mfh_stress_measures' layout: [nElem][NQ] (von Mises) and
 * [nElem][NQ][flatLen] (components, tensor shear), NQ = 1 for degree 1 and dim + 1 for degree 2. With the covariance C = F F^T of the coordinates
 * (mfh_psd_factor) and the factor fields u_t = B F[:, t], B = [Phi | r_1 | r_2]:
 *     rmsComponents[c] = sqrt(E[sigma_c^2]) = sqrt(sum_t sigma_c(u_t)^2),
 *     rmsVonMises      = sqrt(E[sigma_vm^2]) = sqrt(sum_t vm(sigma(u_t))^2)      (Segalman; the 2D value is mfh_stress_measures' plane-stress form).
 * The von Mises figure is the root of the MEAN SQUARE of the von Mises stress, not the mean E[sigma_vm] (which is not a quadratic form and is smaller).
 * MFH_MODAL_STRESS_STRAIN: strains instead of stresses. No stress basis is stored: the planes u_t are expanded 32 at a time and dropped.
 * The squares are absolute (no scaling by the largest entry, unlike mfh_stress_measures): stresses whose squares leave the double range overflow or
 * flush. What a truncated factorisation leaves out of a corner's variance is at most truncation * 3 * sum_j |s_j|^2, s_j the corner's stress of column
 * j (3 = the largest eigenvalue of the von Mises form with tensor shear entries); info->truncation reports the trace, as for mfh_modal_quadratic.
 *   mfh_modal_quadratic_stress   nMat <= 4 matrices over the modes (the SRSS / CQC primitive, C_jk = rho_jk a_j a_k); outputs nMat x ... one after the other.
 *   mfh_modal_random_stress      sets up exactly as mfh_modal_random (loads, MFH_MODAL_RV_STATIC_CORRECTION in params->flags; the velocity and
 *                                acceleration flags are MFH_ERR_INVALID), forms C^(0) only (cov: nb x nb, or NULL) and runs the passes over all nb columns.
 * info->peakVonMises / peakCorner: the largest RMS von Mises value of each matrix and its flat corner index e NQ + q (ties: the lowest index; a NaN first).
 * Validity, MFH_ERR_STATE on a stale basis and the refusals are those of mfh_modal_quadratic / mfh_modal_random; the elasticity operator on the mesh's
 * own degree and an unpartitioned context are required (MFH_ERR_UNSUPPORTED); a requested output that is NULL, or flags without VON_MISES | COMPONENTS:
 * MFH_ERR_INVALID. On any refusal nothing is written. */
enum { MFH_MODAL_STRESS_VON_MISES = 1, MFH_MODAL_STRESS_COMPONENTS = 2, MFH_MODAL_STRESS_STRAIN = 4 /* strain instead of stress */ };
typedef struct mfh_modal_stress_info {
    int32_t ranks[4], passes[4];
    double truncation[4];
    double peakVonMises[4];
    int64_t peakCorner[4];
    int32_t staticSolves, staticIterations, nb, reserved;
    double covarianceMs, factorMs, solveMs;                                            /* solveMs: device events around the passes, the peak AND the copies of the outputs to the host */
    const char* note;                                                                  /* owned by the context, valid until its next call */
} mfh_modal_stress_info;
mfh_status mfh_modal_quadratic_stress(mfh_ctx* ctx, int32_t nMat, const double* C /* nMat x nModes x nModes */, double tol, int32_t flags,
                                      double* rmsVonMises /* nMat x nElem x NQ, or NULL */, double* rmsComponents /* nMat x nElem x NQ x flatLen, or NULL */,
                                      mfh_modal_stress_info* info);
mfh_status mfh_modal_random_stress(mfh_ctx* ctx, const mfh_modal_random_params* params, const double* omega, const double* weights,
                                   const double* modalDamping, const double* f, const double* S, int32_t stressFlags,
                                   double* rmsVonMises, double* rmsComponents, double* cov /* nb x nb = C^(0), or NULL */, mfh_modal_stress_info* info);

/* ---------------------------------------------------------------- per-element density, the product with M, mass properties
 * (docs/design/04_15_density.md.) The mass matrix of mfh_modes and mfh_newmark is assembled from a density field of the context:
 *     M = sum_e rho_e int_e phi_i phi_j   on displacement vectors (kron with the identity of size dim),   rho = 1 until a field is set.
 * The scalar `density` of mfh_modes and of mfh_newmark_params keeps its meaning: it multiplies whatever field is in force.
 *   mfh_set_density      rho: one value per element (n == nElem), copied to a device buffer the context owns; NULL restores unit density. flags: 0, or
 *                        MFH_LOAD_ON_DEVICE (rho is a device pointer). The field survives mfh_mesh_update_vertices, DoF maps and boundary
 *                        conditions; a new mesh (mfh_mesh_build / mfh_mesh_set) clears it. The resident mass values are reassembled by the next
 *                        call that needs them. MFH_ERR_INVALID before any device work -- the field in force stays -- on n != nElem or an entry
 *                        that is not finite or not strictly positive (M must stay positive definite: unlike mfh_body_force_load, 0 is refused; a
 *                        host array is scanned on the host, a device array by a kernel whose lanes store a flag). MFH_ERR_STATE: no mesh, a
 *                        host-only context, a matrix from mfh_matrix_set_upper_triplets. MFH_ERR_UNSUPPORTED: a row-partitioned context.
 *   mfh_mass_apply       y = M x on displacement vectors (dim*nDoF, under the context's DoF map), no fixed variables masked; x and y must not
 *                        overlap. flags as above (both arrays on the device). For participation factors and orthonormality checks of mfh_modes'
 *                        rows. The contexts mfh_modes accepts (elasticity, the mesh's own degree, unpartitioned); like it the call holds both
 *                        triangles of the pattern for its own duration.
 *   mfh_mass_properties  mass = scale int rho, com = the centre of mass, S = scale int rho (x - com)(x - com)^T (dim x dim, row-major, symmetric)
 *                        over the straight-sided elements, with the context's field (or rho = 1) and the scalar scale > 0 (the `density` of
 *                        mfh_modes). The 3D inertia tensor about the centre is tr(S) I - S, the 2D polar moment tr(S). Any output may be NULL;
 *                        flags is reserved (0). Two passes on the device -- mass and first moments, then second moments about the centre of
 *                        pass 1, so that nothing cancels for a body far from the origin -- each an ordered two-stage sum without
 *                        floating-point atomics: the same call returns the same bits. Errors as for mfh_set_density.
 * The operators MFH_OP_MASS / MFH_OP_MASS_VECTOR of mfh_set_operator (assembled into K's value buffer, with matrix-free forms) and mfh_mass_lumped
 * are separate from this and stay at unit density. */
mfh_status mfh_set_density(mfh_ctx* ctx, const double* rho /* nElem, or NULL = clear */, int64_t n, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_mass_apply(mfh_ctx* ctx, const double* x /* dim*nDoF */, double* y /* dim*nDoF */, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_mass_properties(mfh_ctx* ctx, double scale,
                               double* mass, double* com /* dim */, double* S /* dim*dim, row-major */,
                               int32_t flags /* 0 */);

/* ---------------------------------------------------------------- linear buckling: prestress, geometric stiffness, critical load factors
 * (docs/design/04_16_buckling.md.) The context owns a prestress field: one symmetric tensor sigma_e per element, [nElem][flatLen] in the layout
 * and shear convention of mfh_average_stress (TENSOR shear entries). Its geometric stiffness on displacement vectors is
 *     Kg[(i,a),(j,b)] = delta_ab sum_e int_e grad phi_i . sigma_e grad phi_j      (one scalar per node block, kron with the identity of size dim),
 * with the ELEMENT-AVERAGE stress: exact for linear elements, O(h) for quadratic ones, whose stress varies inside an element. sigma = I gives the
 * Laplacian. The reference has no counterpart (its Eigensolver.hh has no buckling entry).
 *   mfh_set_prestress    sigma: n == nElem tensors, any finite values (the field is indefinite by nature), copied to a device buffer the context
 *                        owns; NULL clears it. flags: 0, or MFH_LOAD_ON_DEVICE (sigma is a device pointer; it is scanned for non-finite entries by
 *                        a kernel whose lanes store a flag). The field survives mfh_mesh_update_vertices, DoF maps and boundary conditions; a new
 *                        mesh clears it. MFH_ERR_INVALID before any device work that changes state -- the field in force stays -- on n != nElem,
 *                        a non-finite entry or an unknown flag. MFH_ERR_STATE: no mesh, a host-only context, a matrix from
 *                        mfh_matrix_set_upper_triplets. MFH_ERR_UNSUPPORTED: a row-partitioned context.
 *   mfh_prestress_from_displacement   sigma_e = C_e : (element-average strain of u), u per NODE (nNode x dim, what mfh_sim_solve returns), written
 *                        on the device into the context's buffer by the kernel of mfh_average_stress: no host trip. Elasticity on the mesh's own
 *                        degree (MFH_ERR_UNSUPPORTED otherwise).
 *   mfh_geometric_apply  y = Kg x on displacement vectors (dim*nDoF, under the context's DoF map), no fixed variables masked; x and y must not
 *                        overlap. The contract and the contexts of mfh_mass_apply; MFH_ERR_STATE without a prestress field. Like mfh_mass_apply the
 *                        call holds both triangles of the pattern for its own duration: on a context that stores the upper triangle -- every
 *                        elasticity context with default options -- EVERY call re-runs the symbolic phase and reassembles Kg, and the next call
 *                        of another entry point rebuilds the upper-triangle pattern (cost: profiles/r12_buckling.md). Callers who apply Kg many
 *                        times set option "matrix_storage" 0 once; the buffer is then assembled once per prestress. Kg is always assembled by the
 *                        turn-taking (deterministic) flavour of the gather assembly, so two calls return the same bits in either case.
 *   mfh_buckling         the nev (1 .. 20) smallest eigenvalues mu of Kg x = mu K x on the clamped context, i.e. (K + factor Kg) x = 0 with
 *                        factor = -1/mu: the multiples of the prestress at which the body buckles, smallest first. The LOBPCG loop of mfh_modes
 *                        on the pencil (Kg, K): Kg indefinite, K the context's elasticity operator carrying the inner product, the context's
 *                        preconditioner of K. The fixed variables (values taken as 0) are removed from the pencil and must leave no rigid motion
 *                        free (MFH_ERR_UNSUPPORTED otherwise). A column counts as converged at ||Kg x - mu K x||_2 / (|mu| ||K x||_2) <= rtol
 *                        (written to residuals, may be null). mu ascending; the rows of X are K-orthonormal, each with its entry of largest
 *                        modulus positive, and zero at the fixed variables. A mu_j that is not negative beyond rounding (mu_j >= -1e-12 max|mu|:
 *                        no buckling in the direction of the prestress, e.g. pure tension) gives factors[j] = +INFINITY; info->nBuckling counts
 *                        the negative ones. flags is reserved (0). maxit reached: MFH_ERR_NOT_CONVERGED with the outputs filled. MFH_ERR_INVALID:
 *                        nev outside 1 .. 20 or more than the pencil has, an unknown flag. MFH_ERR_STATE: no prestress field, no mesh, a
 *                        host-only context, an external matrix. MFH_ERR_UNSUPPORTED: a row-partitioned context, an operator other than
 *                        elasticity, the forced-degree-1 view. Like mfh_modes the call holds both triangles of the pattern for its own duration
 *                        (info->note says so). */
typedef struct mfh_buckling_info {
    int32_t converged, iterations, nLocked, precondUsed, blockSize, restarts, nBuckling;   /* nBuckling: returned factors that are finite */
    double  maxResidual, solve_ms, setup_ms;
    const char* note;                                                                       /* owned by the context, valid until its next call */
} mfh_buckling_info;
mfh_status mfh_set_prestress(mfh_ctx* ctx, const double* sigma /* nElem x flatLen, or NULL = clear */, int64_t n, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_prestress_from_displacement(mfh_ctx* ctx, const double* uNodes /* nNode x dim */, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_geometric_apply(mfh_ctx* ctx, const double* x /* dim*nDoF */, double* y /* dim*nDoF */, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);
mfh_status mfh_buckling(mfh_ctx* ctx, int32_t nev, int32_t flags /* 0 */, double rtol, int32_t maxit,
                        double* factors /* nev */, double* X /* nev x dim*nDoF, row per mode */, double* residuals /* nev or NULL */,
                        mfh_buckling_info* info);

/* ---------------------------------------------------------------- prestressed vibration: the modes of (K + s Kg, density M)
 * (docs/design/04_18_prestressed_modes.md.) The frequencies of the clamped body UNDER the load whose stress is the prestress field in force
 * (mfh_set_prestress / mfh_prestress_from_displacement), at the multiple s = loadFactor of it: tension stiffens, compression softens, and the
 * first eigenvalue falls to zero as s reaches the critical factor of mfh_buckling. The reference has no counterpart.
 *   mfh_modes_prestressed   the nev (1 .. 20) smallest eigenpairs of (K + loadFactor Kg) x = lambda density M x: K, M, density and the density field
 *                        as in mfh_modes, Kg as in mfh_geometric_apply. The LOBPCG loop of mfh_modes on this pencil with the context's
 *                        preconditioner of K; convergence at ||A x - lambda M x||_2 / (|lambda| ||M x||_2) <= rtol; the outputs as mfh_modes
 *                        returns them (lambda ascending, rows of X M-orthonormal with the entry of largest modulus positive, zero at the fixed
 *                        variables, which must leave no rigid motion free). Only M is factored, so K + loadFactor Kg may be indefinite: beyond the
 *                        critical load the eigenvalues come out negative, are returned as they are, and info->note says how many and that the
 *                        prestressed state is unstable at this factor. X0 (may be NULL): nev rows that replace the first nev columns of the start
 *                        block (masked, then M-orthonormalised and Rayleigh-Ritz'ed with the rest): the shapes of a neighbouring load factor make
 *                        a sweep cheap. maxit reached: MFH_ERR_NOT_CONVERGED with the outputs filled. MFH_ERR_INVALID: what mfh_modes calls
 *                        invalid, a load factor or an entry of X0 that is not finite. MFH_ERR_UNSUPPORTED: flags != 0 -- in particular
 *                        MFH_MODES_FREE: rigid rotations are not in the kernel of Kg, so the known-kernel variant does not apply --, a clamp that
 *                        leaves rigid motions free, and what mfh_buckling calls unsupported. MFH_ERR_STATE: as mfh_buckling. All refusals come
 *                        before any device work that changes state. Like mfh_modes the call holds both triangles of the pattern for its own
 *                        duration (info->note says so).
 *   mfh_tangent_apply    y = (K + loadFactor Kg) x on displacement vectors (dim*nDoF, under the context's DoF map), no fixed variables masked; x and
 *                        y must not overlap. The contract, the contexts and the cost note of mfh_geometric_apply. */
mfh_status mfh_modes_prestressed(mfh_ctx* ctx, int32_t nev, double density, double loadFactor, int32_t flags /* 0 */, double rtol, int32_t maxit,
                                 const double* X0 /* nev x dim*nDoF or NULL */, double* lambda /* nev */, double* X /* nev x dim*nDoF, row per mode */,
                                 double* residuals /* nev or NULL */, mfh_modes_info* info);
mfh_status mfh_tangent_apply(mfh_ctx* ctx, double loadFactor, const double* x /* dim*nDoF */, double* y /* dim*nDoF */, int32_t flags /* 0 | MFH_LOAD_ON_DEVICE */);

/* ---------------------------------------------------------------- multi-GPU solve (one process per GPU)
 * The reference is single-process (TBB, Parallelism.hh:31-43): these entry points have no counterpart to cite beyond the
 * serial path they parallelise (Simulator::solve, LinearElasticity.hh:479-487; SPSDSystem::solve, SparseMatrices.hh:2515-2606).
 * Rows (nodes) are partitioned: every rank builds its context with mfh_mesh_set(..., nOwned) -- owned nodes first, halo
 * nodes after them GROUPED BY OWNER RANK -- and assembles its rows without communication. The solve needs, per PCG
 * iteration, one neighbour exchange of the halo entries and ONE all-reduce of 4 nrhs doubles (two with the two-level
 * preconditioner); both go through an mfh_comm:
 *   mfh_comm_create_rccl       RCCL communicator of `world` ranks created from a shared unique id (rank 0 calls
 *                              mfh_rccl_get_unique_id and distributes the 128 bytes by any means: MPI, a file, torch's store).
 *                              RCCL is looked up with dlopen (the process's own copy if it has one, e.g. PyTorch's), so the
 *                              library links against no particular communication stack.
 *   mfh_comm_create_callbacks  the two collectives supplied by the caller (MPI, torch.distributed/gloo in the CPU-staged
 *                              tests ...). Buffers are DEVICE pointers; the call must be ordered on `hipStream` (enqueue
 *                              there, or synchronise the stream, do the transfer and return).
 * mfh_dist_setup: peers = neighbouring ranks; sendNodes[sendPtr[k] .. sendPtr[k+1]) = OWNED local nodes whose values rank
 *   peers[k] reads (in the order that rank stores them); halo nodes nOwned + [recvPtr[k], recvPtr[k+1]) are owned by peers[k].
 * mfh_dist_two_level: the two-level preconditioner with GLOBAL aggregates (arguments as mfh_tl_partitioned_begin; the
 *   coarse operator is summed over the ranks, every rank inverts it redundantly).
 * mfh_dist_solve: f / u are nrhs vectors of dim * nOwned doubles (this rank's rows). Fixed variables (mfh_fix_variables,
 *   local numbering) must be given for halo nodes as well as owned ones.                                              */
typedef struct mfh_comm mfh_comm;
typedef struct mfh_rccl_unique_id { char internal[128]; } mfh_rccl_unique_id;
typedef mfh_status (*mfh_allreduce_fn)(void* user, double* devBuf, int64_t n, void* hipStream);
typedef mfh_status (*mfh_exchange_fn)(void* user, int32_t nPeers, const int32_t* peers, const double* const* sendBufs,
                                      const int64_t* sendCounts, double* const* recvBufs, const int64_t* recvCounts, void* hipStream);
mfh_status  mfh_rccl_get_unique_id(mfh_rccl_unique_id* id);
mfh_status  mfh_comm_create_rccl(mfh_ctx* ctx, const mfh_rccl_unique_id* id, int32_t rank, int32_t world, mfh_comm** out);
mfh_status  mfh_comm_create_callbacks(int32_t rank, int32_t world, void* user, mfh_allreduce_fn allreduce_sum,
                                      mfh_exchange_fn exchange, mfh_comm** out);
void        mfh_comm_destroy(mfh_comm* comm);
const char* mfh_comm_describe(const mfh_comm* comm);
/* in-place sum of n doubles in device memory over the ranks (blocking) */
mfh_status  mfh_comm_allreduce(mfh_ctx* ctx, mfh_comm* comm, double* devBuf, int64_t n);
/* ring shift of a known message + all-reduces with known sums (several rounds when peer transfers are enabled): checks the transport
 * in use end to end */
mfh_status  mfh_comm_selftest(mfh_ctx* ctx, mfh_comm* comm);
/* First contact with the devices and links of a node, before any solve (collective): device memory head-room, the devices of all ranks
 * and hipDeviceCanAccessPeer towards each, which IPC slabs are mapped (after mfh_comm_enable_peer), an all-reduce of ones, and the
 * bandwidth of a ring of messageBytes-long messages (send to rank + 1 while receiving from rank - 1) on the transport underneath and
 * through the peer transfers. Layout of `out` (>= 16 + 2 world doubles): meshfem_amd/csrc/mfh_solver.cpp, mfh_comm_preflight. */
mfh_status  mfh_comm_preflight(mfh_ctx* ctx, mfh_comm* comm, int64_t messageBytes, double* out, int64_t nOut);
/* Direct device-to-device transfers for the ranks of ONE node, layered on an existing communicator (collective; the HIP IPC handles
 * travel through the communicator's own all-reduce): every rank exports one slab of fine-grained device memory; the halo exchange of
 * the PCG then writes straight into the neighbours' slabs (stores over xGMI, one release flag per message, two buffers per pair) and
 * all-reduces of up to 2^21 doubles (the dot products: ONE single-workgroup kernel; the replicated coarse levels) are all-to-all
 * writes summed in rank order -- no library call and no host code per iteration, bit-identical sums on every rank. Larger
 * all-reduces and halo widths the staging was not sized for keep using the communicator underneath. The ranks must be separate
 * processes (several may share a device); needs HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose driver only supports dmabuf IPC.
 * A rank that waits longer than MFH_PEER_TIMEOUT_S (60) seconds for a neighbour gives up and the solve returns MFH_ERR_HIP: the
 * device is never left spinning. mfh_comm_selftest exercises the path; mfh_comm_disable_peer (collective) returns to the transport
 * underneath. A communicator serves ONE host thread and one collective at a time (like a context): the message numbers and staging
 * buffers of a pair are shared by everything that runs on it -- two contexts may name the same communicator in mfh_dist_setup, their
 * solves must not overlap. */
mfh_status  mfh_comm_enable_peer(mfh_ctx* ctx, mfh_comm* comm);
mfh_status  mfh_comm_disable_peer(mfh_ctx* ctx, mfh_comm* comm);
mfh_status  mfh_dist_setup(mfh_ctx* ctx, mfh_comm* comm, int32_t nPeers, const int32_t* peers, const int64_t* sendPtr /* nPeers+1 */,
                           const int32_t* sendNodes, const int64_t* recvPtr /* nPeers+1 */);
mfh_status  mfh_dist_two_level(mfh_ctx* ctx, int32_t nAgg, const int32_t* aggOfNode, const double* relPos);
mfh_status  mfh_dist_solve(mfh_ctx* ctx, int32_t nrhs, const double* fOwned, double* uOwned, double rtol, int32_t maxit,
                           mfh_solve_info* info /* nrhs entries, or NULL */);
/* (K u) on this rank's rows for a field given on its rows (halo entries fetched from the owners) */
mfh_status  mfh_dist_apply_K(mfh_ctx* ctx, const double* uOwned, double* KuOwned);
/* What the last mfh_dist_solve did on this rank. transport: what carried the halo exchange (1 RCCL send/recv, 2 peer copies over HIP
 * IPC, 3 caller callbacks). With option "dist_profile" 1 the first operator applications of a solve are bracketed by HIP events:
 * exchange_ms (pack done -> halo arrived, communication stream), interior_ms (the element blocks / row chunks that read no halo column),
 * exposed_wait_ms (how long the compute stream then still waited for the halo: 0 = the exchange is hidden), boundary_ms (the blocks
 * that read the halo), operator_ms (all of it), averages over profiled_applications. */
typedef struct mfh_dist_stats {
    int32_t world, rank, transport, peer_enabled;
    int64_t halo_nodes_sent, halo_nodes_received, halo_bytes_per_exchange /* sent + received, one right-hand side */;
    int64_t interior_items, boundary_items;
    double  exchange_ms, interior_ms, boundary_ms, exposed_wait_ms, operator_ms;
    int32_t profiled_applications, reserved;
    int64_t exchanges;                                   /* since mfh_dist_setup */
    int64_t peer_halo_messages, peer_halo_bytes;         /* through the peer transfers, since they were enabled */
    int64_t allreduces_small, allreduces_large, fallback_exchanges, fallback_allreduces;
} mfh_dist_stats;
mfh_status  mfh_dist_get_stats(mfh_ctx* ctx, mfh_dist_stats* out);
/* blocking copy helper for callback communicators that stage through the host: kind 0 host->device, 1 device->host,
 * 2 device->device; hipStream NULL = the context's stream */
mfh_status  mfh_dev_memcpy(mfh_ctx* ctx, void* dst, const void* src, int64_t bytes, int32_t kind, void* hipStream);

/* Device memory. The library allocates from a per-process ARENA (meshfem_amd/csrc/mfh_pool.cpp): released device memory is not returned to
 * the driver but kept in the hipMalloc segments it came in, where free neighbours are merged and any later request is cut from the smallest
 * free chunk that holds it; the driver is asked for a new segment only when nothing fits. Reason: on ROCm 7.2 / MI355X a hipMalloc that
 * follows large hipFree calls of the same process takes seconds (profiles/r04_malloc_probe.txt), and the setup phases of a context allocate
 * and release several times the memory they keep. The reference reserves its triplet storage once (LinearElasticity.hh:1441-1443).
 * Bounds: free bytes kept while contexts are alive <= MFH_DEVICE_CACHE_MB (default half of the device's memory; 0 = plain hipMalloc /
 * hipFree); when the LAST context of a device closes the arena is trimmed to at most MFH_DEVICE_CACHE_IDLE_MB of free memory (default a
 * quarter of the device), so that other allocators of the process (torch, RCCL) find the rest. A request the driver cannot serve releases every free segment and is repeated. mfh_device_cache_trim returns every free segment to
 * the driver at once. mfh_device_arena_stats: out8 = {bytes held, live bytes, live high-water mark, segments, free chunks, bytes returned
 * to the driver so far, bytes waiting for a device-wide synchronisation, bound on the free bytes}.
 * Debug aid: MFH_ARENA_GUARD=1 puts 512 pattern bytes behind every buffer and checks them when the buffer is released -- a kernel that wrote past
 * the end of its buffer aborts the process with the buffer's size (synchronous fills and read-backs: for test runs; scripts/r06/run_guard.sh). */
/* mfh_device_reserve: `bytes` taken from the driver now and kept as free space of the arena -- the reference's "reserve once"
 * (LinearElasticity.hh:1441-1443) for a caller that knows roughly what its mesh will need (mfh_context_bytes_estimate; mfh_device_reserve_for
 * does both). Contexts created afterwards cut their buffers from it: no call to the driver during their setup. With async != 0 the call returns
 * at once and the allocation runs on threads of its own (e.g. while the caller reads its mesh); the library's next allocation that finds nothing
 * waits for it. Worth it on a device nobody has used since boot, where the driver clears the memory a process takes beyond the first ~66 GB
 * while it is being allocated (profiles/r05_large_allocation_trace_119.log).
 * The reservation is made in TWO segments: one for the value array of K (its share of the request: mfh_device_reserve_for knows it from the mesh
 * kind, mfh_device_reserve assumes the 43 % of a quadratic 3D context) and one for everything else -- the arena never puts anything else into
 * the value array's segment (and gives the array a segment of its own when nothing was reserved): with everything in ONE hipMalloc the values and
 * all other buffers lie in one physical run, and the assembly kernel then runs at the slow end of its placement spread (3.27 against 2.9-3.1 ms at
 * 5 M quadratic tets, 24.4 against 22.6 ms at 40 M; docs/design/04_2_k_assemble_gather.md (xi)). A synchronous reservation the driver cannot
 * serve returns MFH_ERR_HIP. */
mfh_status mfh_context_bytes_estimate(int32_t dim, int32_t deg, int64_t nElem, int64_t* totalBytes, int64_t* kValueBytes);
mfh_status mfh_device_reserve_for(int32_t device, int32_t dim, int32_t deg, int64_t nElem, int32_t async);
mfh_status mfh_device_reserve(int32_t device, int64_t bytes, int32_t async);
/* option "placement_trials": kernel time (ms) of every candidate of the last trials, the first being the buffer of the symbolic phase; *n = how many */
mfh_status mfh_placement_info(const mfh_ctx* ctx, int32_t cap, double* ms, int32_t* n);
mfh_status mfh_device_cache_trim(void);
mfh_status mfh_device_cache_stats(int32_t device, int64_t* cachedBytes, int64_t* blocks, int64_t* hits, int64_t* misses, int64_t* flushes);
mfh_status mfh_device_arena_stats(int32_t device, int64_t* out8);

/* ---------------------------------------------------------------- introspection, options
 * (kernel timers, operator statistics, test hooks and the device-pointer building blocks: include/meshfem_hip_extras.h) */
mfh_status mfh_get_timing(const mfh_ctx* ctx, mfh_timing* out);
/* option knobs (string key, numeric value): "chunk_slots", "contrib_order" (0 rank-major, 1 element-major,
 * 2 slot-major), "check_every", "keep_host_symbolic", "agg_nodes" (target DoFs per aggregate of the two-level
 * preconditioner), "reembed" (1: every mfh_assemble re-runs the element-embedding kernel as well),
 * "matrix_free" (operator of mfh_solve / mfh_apply_K / mfh_dev_spmv: 0 = assembled block-CSR SpMV, 1 = matrix-free
 *   (k_mf_cluster + k_mf_rows: element stresses recomputed, K not read), -1 = auto (default): matrix-free for elasticity
 *   (quadratic: 6x faster than the assembled SpMV; linear: 1.2x at 1 M tets, 1.8x from 6 M on), assembled for the scalar operators; both give
 *   K x up to rounding),
 * "matrix_free_mode" (4 default: cluster variant, forces of a block of 512-1024 consecutive elements summed in LDS | 3 two-pass, forces in
 *   list order | 2 two-pass, forces element-major | 1 per-pair block evaluation), "mf_chunk_rows", "mf_chunk_pairs",
 * "mf_geometry_from_vertices" (1 default: with a constant material the matrix-free operator recomputes the element gradients from the
 *   corner positions instead of reading the element records), "mf_xcd_group" (32 default: consecutive element blocks per XCD),
 *   "mf_lane_stride" (37 default: lane-to-element stride inside a block, against same-address LDS atomics),
 * "pcg_graph" (1 default: blocks of check_every PCG iterations are replayed from a hipGraph),
 * "refine" (1 default: when a converged solve of mfh_solve / mfh_sim_solve* ends with a TRUE residual ||f - K u|| / ||b|| above twice the
 *   tolerance -- the recurrence residual drifts over thousands of iterations -- the correction K du = f - K u is solved to what is missing
 *   and added, up to three times: the answer is as good as the tolerance says, like a direct solver's; solves that end within it are untouched),
 * "matrix_storage" (which blocks of K are stored and assembled. 1: only the blocks (r, c >= r), the triangle the reference's TripletMatrix
 *   holds -- half the bytes and block arithmetic of the assembly; serves mfh_export_upper_triplets, mfh_export_bsr (mirrored on the host),
 *   the (block-)Jacobi and two-level PCG on the matrix-free operator, and mfh_apply_K / mfh_dev_spmv through k_spmv_sym (the transposed half
 *   of the product added with global atomics: 2.5x slower than the product from both triangles); the PCG on the assembled SpMV and the probing
 *   construction of the coarse operator return MFH_ERR_UNSUPPORTED on it. 0: both triangles. -1 default: automatic -- the upper triangle exactly when nothing
 *   multiplies by the stored K (elasticity on the matrix-free operator), both triangles otherwise; changing an option that
 *   decides this re-runs the symbolic phase on the next use. mfh_matrix_info / mfh_export_bsr describe K itself either way,
 *   mfh_matrix_storage what is stored),
 * "placement_trials" (0 default; N <= 8: at the first gather-mode assembly after a symbolic phase the buffer of the K values is allocated up to N more
 *   times, the assembly kernel timed on each (two passes), and the fastest kept -- where the driver puts these bytes moves the kernel between
 *   2.9 and 3.3 ms at 5 M quadratic tets, docs/design/04_2_k_assemble_gather.md (xi); costs ~10 ms and one more buffer of the size of K per trial,
 *   once per symbolic phase: for callers that assemble hundreds of times on one mesh. mfh_placement_info reads the candidates' times),
 * "pcg_variant" (1: Chronopoulos-Gear PCG, one reduction point per iteration and one fused vector kernel -- always used by
 *   mfh_dist_solve and for batches; 0: the classic two-reduction PCG, one right-hand side at a time; -1 default: classic for
 *   a single right-hand side on an unpartitioned context, where it is 6-14 % faster per iteration), "dist_pcg_variant"
 *   (mfh_dist_solve with one right-hand side: 1 default = Chronopoulos-Gear, ONE all-reduce per iteration; 0 = classic loop, two
 *   all-reduces and one vector pass less -- which is faster depends on the node's all-reduce latency), "batch_rhs" (0 default:
 *   1 solves several right-hand sides per operator pass of the Chronopoulos-Gear loop, see mfh_solve_batch; block-Jacobi / two-level only),
 * "mg_batch" (1 default: several right-hand sides under MFH_PRECOND_MULTIGRID on an unpartitioned quadratic context run one classic PCG loop
 *   each, in lockstep, and share the linear / aggregate / dense levels of every V-cycle; 0: one right-hand side at a time),
 * "mg_fuse" (1 default: with one Chebyshev step on the quadratic level of an unpartitioned hierarchy, the PCG loop's residual update also writes
 *   the V-cycle's pre-smoothed start and the cycle's last smoothing step also forms r.z -- two kernels and three vector passes less per
 *   iteration, the same iterates; 0: separate kernels),
 * "mg_dinv_fp32" (1 default: those two fused kernels read an FP32 copy of the quadratic level's inverse diagonal blocks -- a third of their traffic;
 *   the smoother only, both steps of a cycle the same copy; 0: the FP64 blocks),
 * "solve_homogeneous" (1: mfh_solve treats the fixed variables as fixed to ZERO whatever values were given -- the
 *   homogeneous solves K y = C^T of a Schur-complement elimination of constraint rows, SparseMatrices.hh:2572-2590),
 * "periodic_ignore_mismatch" (1: nodes of a periodic face without a partner keep their own DoF, PeriodicCondition's
 *   ignoreMismatch / matchPermittingMismatch; 0 default: a mismatch is an error like PeriodicBoundaryMatcher::match),
 * "periodic_ignore_dims" (bit a set: dimension a is NOT periodic, PeriodicCondition's ignoreDims) -- both read by the next
 *   mfh_apply_periodic_conditions,
 * "mg_steps_fine" / "mg_steps_coarse" (1 / 1: Chebyshev steps of MFH_PRECOND_MULTIGRID before and after the coarse correction on the quadratic /
 *   linear level), "mg_ratio_fine" / "mg_ratio_coarse" (0.3 / 0.3: the smoothers act on [ratio lambda_max, lambda_max]), "mg_coarse_cycles"
 *   (1: cycles of the linear level per application), "mg_eig_margin" (1.1: factor on the power-iteration estimates), "mg_agg_nodes",
 * "mg_coarse_fp32" (1 default: INSIDE the multigrid preconditioner the assembled matrix of the linear level and the stencil operators of the
 *   aggregate levels are read from FP32 copies -- products, sums and every vector stay FP64, and so do K, K x and the residuals of the PCG itself;
 *   the preconditioner is a fixed SPD operator either way, the solution is the FP64 one; 0: FP64 storage throughout),
 * "asm_packed_codes" (1 default: the device copy of the gather lists is chunk-relative and packed, see k_assemble_gather),
 * "asm_chunk_order" (0 default; 1: the assembly visits the row chunks in the order of the elements they gather from),
 * "deterministic" (1: run-to-run BIT-REPRODUCIBLE assembly, operator and PCG -- the counterpart of the reference's serial, reproducible
 *   scatter into the triplet list (LinearElasticity.hh:1454-1455; SparseMatrices.hh:288,319-324 switches its one unordered loop off). The
 *   default kernels accumulate with LDS / global atomics in the order the waves happen to arrive, so the last bits of K, K x and the dot
 *   products differ between two runs; with the option the waves of a workgroup add in wave order (assembly, interface rows of the
 *   operator) or into accumulators of their own summed in wave order (element blocks of the operator), every dot product goes through a
 *   fixed two-stage tree, and the PCG runs the classic loop. Two assemblies give identical bits, two solves identical displacements.
 *   Every preconditioner (the Galerkin products of the coarse levels keep one accumulator table per wave, the transfers between the
 *   aggregate levels gather); the global-atomic assembly variant and matrix_free_mode 1 - 3 are refused. Measured cost: bench.py
 *   variants.deterministic),
 * "dist_profile" (1: time the halo exchange against the interior work in the first operator applications of every mfh_dist_solve,
 *   see mfh_dist_get_stats),
 * "symbolic_device", "topology_device", "tl_probe", "tl_host_inverse" (validation variants of setup phases) */
mfh_status mfh_set_option(mfh_ctx* ctx, const char* key, double value);
/* the current value of an option of this context (0 / 1 for the on-off options; a forced-degree-1 view is not followed); an unknown key fails like
 * mfh_set_option's */
mfh_status mfh_get_option(const mfh_ctx* ctx, const char* key, double* value);
#ifdef __cplusplus
}
#endif
#endif /* MESHFEM_HIP_H */
