/* meshfem_hip_extras.h -- entry points of libmeshfem_hip.so that are NOT part of the drop-in boundary (include/meshfem_hip.h holds
 * that: SURVEY.md section 8b): measurement hooks of bench.py / scripts/, test hooks, and the device-pointer building blocks for
 * callers that write their own (distributed) solver loop around the library's kernels. Plain C like the main header. */
#ifndef MESHFEM_HIP_EXTRAS_H
#define MESHFEM_HIP_EXTRAS_H
#include "meshfem_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- measurement */
/* average device time (ms, HIP events on the context stream) of `reps` back-to-back launches of
 * the numeric assembly kernel alone (geometry kernel excluded) -- used by bench.py's roofline   */
mfh_status mfh_time_assembly_kernel(mfh_ctx* ctx, int32_t mode, int32_t reps, double* avg_ms);
/* device time (ms, one entry per repetition) of the mass assembly pass into the resident buffer of mfh_modes / mfh_newmark: the unit-density pass and,
 * field_ms != NULL, the density-weighted pass of the field set with mfh_set_density, launched in turns (scripts/density_probe.py). Needs both
 * triangles of the pattern (option "matrix_storage" 0 on quadratic meshes). */
mfh_status mfh_time_mass_assembly(mfh_ctx* ctx, int32_t reps, double* unit_ms /* reps */, double* field_ms /* reps or NULL */);
/* device time (ms, one entry per repetition) of the gather assembly pass into the resident geometric-stiffness buffer as the Laplacian, the
 * unit-density mass and the geometric stiffness of the prestress in force in the context's flavour, then the geometric stiffness in the turn-taking
 * (deterministic) flavour that the library itself launches for it, in turns (scripts/probe_buckling.py). Needs a prestress field and both triangles
 * of the pattern (option "matrix_storage" 0 on quadratic meshes). */
mfh_status mfh_time_geometric_assembly(mfh_ctx* ctx, int32_t reps, double* laplace_ms /* reps */, double* mass_ms /* reps */, double* geom_ms /* reps */,
                                       double* geom_det_ms /* reps */);
/* average device time (ms) of one pair product of the prestressed loop (yA += s Kg x, yB = rho M x on hashed vectors) over `reps` launches: the single
 * pass k_spmv_kron_pair, and the two launches (plus the density scaling) it replaces, in alternating groups after a warm-up of both
 * (scripts/probe_prestressed_modes.py). Needs a prestress field; holds both triangles of the pattern for its own duration. */
mfh_status mfh_time_kron_pair(mfh_ctx* ctx, int32_t reps, double* pair_ms, double* separate_ms);
/* average device time (ms) of `reps` launches of k_explicit_step (mfh_explicit's step kernel: five vectors read, two written) on hashed vectors of n
 * doubles, and of `reps` device-to-device copies that move the same bytes (3.5 n doubles read and written) in the same process: the kernel's floor
 * -- scripts/probe_explicit.py */
mfh_status mfh_time_explicit_step(mfh_ctx* ctx, int64_t n, int32_t reps, double* step_ms, double* copy_ms);
/* the same for one application of the operator the PCG uses (see "matrix_free") on internal scratch vectors */
mfh_status mfh_time_spmv_kernel(mfh_ctx* ctx, int32_t reps, double* avg_ms);
/* average device time (ms) of `reps` back-to-back k_block_gram calls (both stages) on hashed n x p and n x q blocks, and of `reps` device-to-device
 * copies of the same n (p + q) doubles in the same process: the kernel is bound by reading those bytes (the copy also writes them) --
 * scripts/probe_modes.py's roofline */
mfh_status mfh_time_block_gram(mfh_ctx* ctx, int64_t n, int32_t p, int32_t q, int32_t reps, double* gram_ms, double* copy_ms);
/* matrix-free operator in use? (see option "matrix_free"); for the cluster variant (mode 4): number of element blocks,
 * of (block, row) accumulators, of interface partial sums kept in HBM, and the largest block (LDS accumulators) */
mfh_status mfh_matrix_free_info(mfh_ctx* ctx, int32_t* active, int32_t* mode, int64_t* nBlocks, int64_t* nBlockRows,
                                int64_t* nInterface, int32_t* maxBlockRows);

/* the aggregate levels of the multigrid hierarchy (MFH_PRECOND_MULTIGRID), finest first: out7[l] = {aggregates of the level, rows this rank
 * smooths, entries of its vectors (rows + halo), 1 if the level is partitioned over the ranks (row-partitioned contexts: levels with more
 * than option mg_replicate_max aggregates) else 0 (replicated / unpartitioned context), exchange peers, halo aggregates received and owned
 * aggregates sent per exchange}; *nLevels = levels of the hierarchy (cap = rows of out7) */
mfh_status mfh_multigrid_level_info(const mfh_ctx* ctx, int32_t cap, int64_t* out7, int32_t* nLevels);

/* ---------------------------------------------------------------- test hooks */
/* test hook: in-place inverse of a dense SPD matrix (row-major n x n) with the threaded blocked
 * Cholesky that inverts the two-level preconditioner's coarse operator; MFH_ERR_INVALID if not SPD */
mfh_status mfh_debug_spd_inverse(int64_t n, double* A);
/* the same with the device implementation (blocked 64x64 Cholesky inverse in HBM) */
mfh_status mfh_debug_spd_inverse_device(mfh_ctx* ctx, int64_t n, double* A);
/* test hook: the DEVICE copies of the node table (nElem x nodesPerElem) and of the node positions (nNode x dim) that the kernels
 * read -- mfh_mesh_build writes them on the device from the uploaded vertices; they must equal what mfh_mesh_elem_nodes /
 * mfh_mesh_node_positions return from the host tables (FEMMesh.inl:17-59), bit for bit */
mfh_status mfh_debug_device_node_tables(mfh_ctx* ctx, int32_t* elemNodes, double* nodePos);
/* test hooks: one allocation / release through the library's device arena (meshfem_hip.h "Device memory"), as the library's own buffers
 * make them; tests/test_gpu_arena.py checks splitting, merging, the bounds and the trims with them */
mfh_status mfh_debug_arena_alloc(mfh_ctx* ctx, int64_t bytes, void** out);
mfh_status mfh_debug_arena_free(mfh_ctx* ctx, void* p);
/* test hook (host only, no context): the row chunks of the assembly kernel -- greedy, whole rows, at most chunkSlots slots each, a chunk ends at
 * every row listed in breaks -- scanned by `threads` host threads over ranges of `grain` rows and stitched (threads = 1: the plain sequential
 * scan the result must equal). Writes the chunks' first rows + nRows to chunkRow (capacity cap); *nOut = entries (chunks + 1) */
/* test hook: Y = K X for nr host vectors (rows of X and Y, dim * nDoF doubles each) through the operator of the batched PCG -- the batched
 * kernels (k_mf_cluster_nr / k_mf_rows_nr / k_spmv_nr) for nr > 1, the single-vector ones for nr = 1; masked != 0 zeroes the fixed rows.
 * Y's incoming contents are uploaded as y (a closed gate must leave them). flavour: 0 plain, dots[k] = the kernels' fused X[k] . Y[k];
 * 1 classic-PCG bookkeeping with the gate open (nr = 1); 2 Chronopoulos-Gear bookkeeping with the gate open; 3 / 4 the same two gates
 * closed. With 1 and 2, dots[k] is read from the scalar history where the PCG reads p . Ap (dots may be null). A batch size the kernels
 * are not built for: MFH_ERR_UNSUPPORTED. Inside a PCG the direction is zero on the fixed rows; masked runs of flavours 1-4 assume it. */
mfh_status mfh_debug_apply_operator(mfh_ctx* ctx, int32_t nr, int32_t masked, int32_t flavour, const double* X, double* Y, double* dots);
/* test hook: Z = M^-1 R (rows, dim * nDoF doubles each) with the preconditioner the next mfh_solve uses (built if need be), ungated:
 * nr = 1 the single-vector path (block-Jacobi / two-level / V-cycle), nr > 1 the batched one (two-level: k_tl_*_nr; multigrid on a
 * quadratic mesh: the batched V-cycle). MFH_ERR_UNSUPPORTED where the preconditioner has no batched path or the batch size no kernels */
mfh_status mfh_debug_apply_precond(mfh_ctx* ctx, int32_t nr, const double* R, double* Z);
mfh_status mfh_debug_row_chunks(int64_t nRows, const int32_t* rowPtr, int32_t chunkSlots, int64_t nBreaks, const int64_t* breaks, int64_t grain,
                                int32_t threads, int32_t* chunkRow, int64_t cap, int64_t* nOut);
/* test hook (host only, no context): the stopping rule of the PCG loops, fed a synthetic residual history of n records {rr[q] = r.r, pKp[q] = p.Kp,
 * known[q] != 0: that p.Kp is known} in order. threshold: on r.r; window: iterations without a best r.r 10 % below the last one that are reported
 * as stagnation (0: no such rule); lastComplete: the records after it are half-written (the end of a block of iterations: their p.Kp is not looked
 * at). *convergedAt = the first record at or below the threshold, -1 if there is none. When the rule reports a breakdown instead, its status is
 * returned and its message copied to msg (capacity msgCap; may be null) */
mfh_status mfh_debug_pcg_watch(int64_t n, const double* rr, const double* pKp, const uint8_t* known, double threshold, int32_t window,
                               int64_t lastComplete, int64_t* convergedAt, char* msg, int64_t msgCap);
/* test hook (host only, no context): the Rayleigh-Ritz step of mfh_modes -- all eigenpairs of the dense symmetric-definite pencil A v = w B v
 * (row-major n x n, n <= 72; the stored upper triangles are read) by Cholesky reduction to standard form and cyclic Jacobi. w ascending, column k
 * of V (row-major n x n) the eigenvector of w[k], V^T B V = I. MFH_ERR_INVALID: B not positive definite */
mfh_status mfh_debug_sym_gen_eig(int64_t n, const double* A, const double* B, double* w, double* V);
/* test hooks: the tall-skinny block kernels of mfh_modes on host arrays. A: n x p, B: n x q, column-major (column j at A + j n);
 * G = A^T B (p x q row-major) through k_block_gram and its fixed-order second stage. p, q in [1, 24] */
mfh_status mfh_debug_block_gram(mfh_ctx* ctx, int64_t n, int32_t p, int32_t q, const double* A, const double* B, double* G);
/* Y = A C through k_block_update: A n x p and Y n x q column-major, C p x q row-major */
mfh_status mfh_debug_block_update(mfh_ctx* ctx, int64_t n, int32_t p, int32_t q, const double* A, const double* C, double* Y);
/* test hook: the projection kernels of mfh_modes_many. BQ, Q: n x nq column-major (nq <= 262); V: n x nv column-major (nv <= 24); cols: k distinct
 * columns of V. G (nq x k row-major) = BQ^T V(cols) through k_deflate_gram and its fixed-order second stage; Vout = V with V(cols) - Q G in the
 * listed columns (k_deflate_update with C = G), every other column as it came */
mfh_status mfh_debug_deflate(mfh_ctx* ctx, int64_t n, int32_t nq, int32_t nv, int32_t k, const int32_t* cols, const double* BQ, const double* Q,
                             const double* V, double* G, double* Vout);
/* ms per call of k_deflate_gram (+ second stage) and of k_deflate_update on nq + k columns of n rows, against a device-to-device copy of the same
 * (nq + k) columns in the same process */
mfh_status mfh_time_deflate(mfh_ctx* ctx, int64_t n, int32_t nq, int32_t k, int32_t reps, double* gram_ms, double* update_ms, double* copy_ms);
/* test hook: the expansion kernel of mfh_modal_harmonic (k_modal_expand, mfh_modal.hip) on host arrays, launched as the sweep launches it.
 * B: n x nb column-major (nb <= 258), C: nb x nPlanes row-major; out: nPlanes x n, out[p][row] = sum_j B_j[row] C[j][p] as the fma chain over j
 * ascending from +0. planesPerPass: 1 .. 32 planes a pass writes (the kernel instantiation is the smallest of 8 / 16 / 32 that holds them);
 * 0 = the library's default */
mfh_status mfh_debug_modal_expand(mfh_ctx* ctx, int64_t n, int32_t nb, const double* B, const double* C, int32_t nPlanes, int32_t planesPerPass,
                                  double* out);
/* test hook: the Gram kernel of the modal layer (k_modal_gram and its fixed-order second stage, mfh_modal.hip) on host arrays. A: n x na
 * column-major (na <= 258), V: n x nv column-major (nv <= 8); G = A^T V, na x nv row-major */
mfh_status mfh_debug_modal_gram(mfh_ctx* ctx, int64_t n, int32_t na, int32_t nv, const double* A, const double* V, double* G);
/* device time (ms, one entry per repetition) of one pass of k_modal_expand<NP> (NP = planesPerPass in {8, 16, 32}; 0 = the default) on nb hashed
 * columns of n rows; mfh_time_deflate times k_deflate_update on the same shape in the same process (scripts/probe_modal.py) */
mfh_status mfh_time_modal_expand(mfh_ctx* ctx, int64_t n, int32_t nb, int32_t planesPerPass, int32_t reps, double* times);
/* test hook: the two kernels of mfh_modal_transient (k_modal_march, k_modal_series, mfh_modal.hip) on host arrays, run as the call runs them; needs no
 * mesh. coef8: nModes x 8 (rows as mfh_modal_transient_coeffs writes them), g: nModes, lambda: nModes (for the energies; NULL without), amplitude:
 * nSteps+1, chunkSteps: 0 = the default, else a positive multiple of 32; q, qdot: nModes each, state in / state after the last step out.
 * Bp: (nModes + corr) x nProbe row-major, row j = column j of the basis at the probe variables (corr = 1: one more row, the correction column).
 * Out (NULL: not wanted): modalCoords (nSteps+1) x nModes, probeOut (nSteps+1) x nProbe, energies (nSteps+1) x 3 */
mfh_status mfh_debug_modal_march(mfh_ctx* ctx, int32_t nModes, const double* coef8, const double* g, const double* lambda, double dt, int32_t nSteps,
                                 const double* amplitude, int32_t chunkSteps, double* q, double* qdot, const double* Bp, int32_t nProbe, int32_t corr,
                                 double* modalCoords, double* probeOut, double* energies);
/* device time (ms, one entry per repetition each) of k_modal_series and of the k_modal_expand route (the gathered probe rows as the kernel's rows, 32
 * steps per pass) for nProbe probes of nSteps rows on nModes hashed columns, the two taking turns in every repetition */
mfh_status mfh_time_modal_series(mfh_ctx* ctx, int32_t nModes, int32_t nProbe, int32_t nSteps, int32_t reps, double* seriesMs, double* expandMs);
/* test hook: the quadratic-form kernel of mfh_modal_quadratic / mfh_modal_random (k_modal_sumsq, mfh_modal.hip) on host arrays, launched as those calls
 * launch it. B: n x nb column-major (nb <= 258), F: nb x rank row-major; out: n, out[row] = sum_t (sum_j B_j[row] F[j][t])^2 (its square root with
 * sqrtFlag), the inner sums fma chains over j ascending from +0, the outer one fma(s_t, s_t, acc) over t ascending from +0. piv: NULL (every pass
 * streams all nb columns) or the rank <= nb pivots of mfh_psd_factor: the pass whose first column is t0 leaves out the columns piv[0 .. t0), whose
 * coefficients have to be exactly zero from t0 on (MFH_ERR_INVALID otherwise). planesPerPass: 1 .. 32 columns of F per pass, 0 = the default.
 * rank 0 returns zeros without reading B */
mfh_status mfh_debug_modal_sumsq(mfh_ctx* ctx, int64_t n, int32_t nb, const double* B, const double* F, int32_t rank, const int32_t* piv,
                                 int32_t planesPerPass, int32_t sqrtFlag, double* out);
/* device time (ms, one entry per repetition each) of one pass of k_modal_sumsq<NP> and of one pass of k_modal_expand<NP> on the same nb hashed columns
 * of n rows, the two taking turns in every repetition (NP = planesPerPass in {8, 16, 32}; 0 = the default); laterMs (or NULL): the SECOND pass of a
 * factor of rank 2 NP whose first NP pivots are the columns 0 .. NP - 1 -- it streams nc = nb - NP columns and reads the accumulator back (0 where
 * nb <= NP) */
mfh_status mfh_time_modal_sumsq(mfh_ctx* ctx, int64_t n, int32_t nb, int32_t planesPerPass, int32_t reps, double* sumsqMs, double* expandMs,
                                double* laterMs);
/* test hook: k_modal_stress_sumsq (mfh_modal_quadratic_stress / mfh_modal_random_stress) on a caller's planes over the context's mesh. U: nPlanes x
 * dim*nDoF (host, VARIABLE numbering), taken planesPerPass (1 .. 32; 0 = the default) at a time; flags: MFH_MODAL_STRESS_*; vm: nElem x NQ, the sums
 * over the planes of the squared von Mises value (always written), comp: nElem x NQ x flatLen with MFH_MODAL_STRESS_COMPONENTS; their roots with
 * sqrtFlag. nPlanes = 0: the kernel's rank-0 launch (no plane) over a scratch filled with NaNs, which writes zeros */
mfh_status mfh_debug_modal_stress_sumsq(mfh_ctx* ctx, int32_t nPlanes, const double* U, int32_t planesPerPass, int32_t flags, int32_t sqrtFlag,
                                        double* vm, double* comp);
/* test hook: k_peak_of_array + k_peak_finish on n host doubles: the largest value and its index (ties: the lowest index; a NaN before every number) */
mfh_status mfh_debug_peak_of_array(mfh_ctx* ctx, int64_t n, const double* v, double* value, int64_t* index);
/* device time (ms, one entry per repetition each) of one pass of k_modal_stress_sumsq over nPlanes <= 32 hashed planes and of nPlanes launches of
 * k_stress_measures (von Mises only) on the same planes, the two taking turns; contexts without a DoF map */
mfh_status mfh_time_modal_stress(mfh_ctx* ctx, int32_t nPlanes, int32_t reps, double* stressMs, double* measuresMs);

/* test hooks: the step kernels of mfh_newmark (mfh_dynamics.hip) on host arrays of n doubles. mask: n bytes or NULL (non-zero = fixed variable).
 * predict: ut = u + dt v + dt^2 (1/2 - beta) a, vt = v + dt (1 - gamma) a (both 0 where masked), w = gamma / (beta dt) ut - vt,
 *   xm = density (ut / (beta dt^2) + rayleighMass w), xk = rayleighStiff w (xk may be NULL) */
mfh_status mfh_debug_newmark_predict(mfh_ctx* ctx, int64_t n, double dt, double beta, double gamma, double density, double rayleighMass, double rayleighStiff,
                                     const uint8_t* mask, const double* u, const double* v, const double* a, double* ut, double* vt, double* xm, double* xk);
/* rhs: b = g f + y (f may be NULL), 0 where masked; *bb = b . b through the two-stage sum */
mfh_status mfh_debug_newmark_rhs(mfh_ctx* ctx, int64_t n, double g, const double* f, const double* y, const uint8_t* mask, double* b, double* bb);
/* correct: a = (x - ut) / (beta dt^2), v = vt + gamma dt a, u = x; probeOut[j] = x[probeVars[j]]; snapshot (n doubles or NULL) = x */
mfh_status mfh_debug_newmark_correct(mfh_ctx* ctx, int64_t n, double dt, double beta, double gamma, const double* x, const double* ut, const double* vt,
                                     double* u, double* v, double* a, const int64_t* probeVars, int32_t nProbe, double* probeOut, double* snapshot);
/* test hooks of mfh_explicit (mfh_explicit.hip). explicit_step: k_explicit_step on host arrays of n doubles, under the context's dyn_grid_cap.
 *   mode 0: v holds v(n-1/2); a(n) = (inv (g f - y) - alpha v) / (1 + alpha dt/2), v(n) = v + dt/2 a(n)
 *   mode 1: v holds v(n), a(n) = inv (g f - y) - alpha v;   mode 2: v holds v(n), a(n) is read from a
 *   then v(n+1/2) = v(n) + dt/2 a(n), u(n+1) = u + dt v(n+1/2). last == 0: u = u(n+1), v = v(n+1/2), a untouched; last != 0: u stays, v = v(n), a = a(n).
 *   probeOut[j] = u(n)[probeVars[j]]; snapshot (n doubles or NULL) = u(n); energies (4 doubles or NULL; needs mass) = {1/2 v(n).mass v(n), 1/2 u(n).y,
 *   g f.u(n), 1/2 v(n+1/2).mass v(n+1/2) + 1/2 u(n+1).y}; *flag = 1 if a value written is not finite. f may be NULL.
 * elem_abs_rowsums: out[(e npe + i) dim + c] = sum_j sum_d |K_e[(i, c), (j, d)]| (k_elem_abs_rowsums), nElem * npe * dim doubles */
mfh_status mfh_debug_explicit_step(mfh_ctx* ctx, int64_t n, double dt, double alpha, double g, int32_t mode, int32_t last, const double* y, double* u, double* v,
                                   const double* inv, const double* mass, const double* f, double* a, const int64_t* probeVars, int32_t nProbe,
                                   double* probeOut, double* snapshot, double* energies, int32_t* flag);
mfh_status mfh_debug_elem_abs_rowsums(mfh_ctx* ctx, double* out);
/* hrz_weights: the npe weights Mref_ii / trace(Mref) of the context's element type as mfh_mass_lumped_hrz takes them from the mass table */
mfh_status mfh_debug_hrz_weights(mfh_ctx* ctx, double* w);
/* y = cK K x + cM M x (M with density 1) through the context's operator and k_spmv_kron_acc, rows of fixed variables zeroed if masked != 0;
 * *dot (may be NULL) = x . y from the kernel's partials. cK == 0 skips the K product */
mfh_status mfh_debug_pencil_apply(mfh_ctx* ctx, double cK, double cM, int32_t masked, const double* x, double* y, double* dot);
/* y^ = zK K x^ + zM M x^ for complex zK, zM and x^ = xRe + i xIm (M with density 1) through the context's operator and k_spmv_kron_cacc -- or two
 * launches of k_spmv_kron_acc and k_harm_combine under option harmonic_two_pass -- rows of fixed variables zeroed if masked != 0; dot (may be NULL):
 * {Re, Im} of the unconjugated x^T y from the kernel's partials. zK == 0 skips the K products */
mfh_status mfh_debug_harmonic_apply(mfh_ctx* ctx, double zKre, double zKim, double zMre, double zMim, int32_t masked, const double* xRe, const double* xIm,
                                    double* yRe, double* yIm, double* dot);
/* test hooks: the two iterative loops on the pencil (NewmarkWork::solve of mfh_dynamics.hip, HarmonicWork::solve of mfh_harmonic.hip) and their
 * block-Jacobi preconditioner, on host vectors of dim * nDoF doubles, M with density 1, the context's fixed variables and preconditioner choice as
 * mfh_newmark / mfh_harmonic make it (tests/test_gpu_pencil_iterates.py).
 * precond: z = Dinv r with the inverse diagonal blocks the loops build for cK K + cM M (k_pencil_dinv; the rows and columns of fixed variables
 *   replaced by the identity; cK == 0 does not read K). The harmonic loop builds its blocks with cK = 1, cM = w^2 density */
mfh_status mfh_debug_pencil_precond(mfh_ctx* ctx, double cK, double cM, const double* r, double* z);
/* newmark_pcg: the PCG on cK K + cM M for the right-hand side b (its fixed rows are zeroed, the threshold is rtol^2 b . b) from the start vector x0
 *   (NULL: zero; zero on the fixed variables). cK == 0 runs the block-Jacobi of cM M whatever the context's preconditioner, as the solve for the
 *   initial acceleration does. x = the iterate the loop ends on, ALWAYS written; history: 4 (maxit + 1) doubles, the rows {r.z, p.Ap, r.r, -} of
 *   iterations 0 .. maxit as the loop left them (r.z stays 0 in the block-Jacobi-free form until the preconditioner ran); *its = the loop's return
 *   value: the iteration that met the threshold, -1 at maxit, -2 on a breakdown. Status MFH_ERR_NOT_CONVERGED with *its < 0 */
mfh_status mfh_debug_newmark_pcg(mfh_ctx* ctx, double cK, double cM, double rtol, int32_t maxit, const double* b, const double* x0, double* x, double* history,
                                 int32_t* its);
/* harmonic_cocg: the COCG on zK K + zM M (zK, zM: {re, im}) for the load fRe + i fIm (fIm may be NULL) from x0 (either plane may be NULL: zero),
 *   without the continuations from the true residual mfh_harmonic adds. jacobiCM: the cM of the block-Jacobi blocks K + cM M, used where the context's
 *   choice is block-Jacobi. history as above (its r.r the Hermitian one); chistory: 4 (maxit + 1) doubles, {Re r^T z, Im r^T z, Re p^T Z p, Im p^T Z p}
 *   per iteration; *its and the status as above */
mfh_status mfh_debug_harmonic_cocg(mfh_ctx* ctx, const double* zK, const double* zM, double jacobiCM, double rtol, int32_t maxit, const double* fRe,
                                   const double* fIm, const double* x0Re, const double* x0Im, double* xRe, double* xIm, double* history, double* chistory,
                                   int32_t* its);
/* the pair product of mfh_modes_prestressed through the launcher its loop uses: yA (in: any vector, out: yA + s Kg x) and yB = rho M x (M with the
 * density field in force), rows of fixed variables zeroed in both if masked != 0. k_spmv_kron_pair, or, if twoPass != 0 (or where its LDS does not
 * fit), k_spmv_kron_acc on the geometric buffer followed by k_spmv_kron on the mass buffer and the density scaling */
mfh_status mfh_debug_kron_pair(mfh_ctx* ctx, double s, double rho, int32_t masked, int32_t twoPass, const double* x, double* yA, double* yB);
/* test hook: the block LOBPCG loop of mfh_modes / mfh_modes_many / mfh_buckling / mfh_modes_prestressed itself (lobpcg_run of mfh_modes.hip) with its
 * history (tests/test_gpu_lobpcg_iterates.py). pencil: 0 vibration (K, density M), 1 buckling (Kg, K), 2 prestressed (K + loadFactor Kg, density M);
 * the context's fixed variables, prestress and preconditioner choice as the entry point of that pencil takes them; freeBody != 0: the known-kernel
 * variant of the vibration pencil. *blockSize = the loop's block size, nev + max(2, (nev + 3) / 4) capped by 24 and by the dimension of the space;
 * with S0 == NULL nothing else happens. S0: the whole start block, m rows of dim * nDoF doubles, in place of the hashed and smoothed block (masked,
 * projected and orthonormalised as that one is); m != *blockSize is refused. Q (nq rows, NULL with nq == 0): a deflation set, B-orthonormal and zero
 * on the fixed variables as the caller gives it; the loop runs in its B-orthogonal complement and its residuals are those of the restricted pencil.
 * X: the whole block, m rows, as the loop left it, before the returned columns are orthonormalised once more. Per call c = 0 .. maxit of the loop's
 * convergence check: lambdaHist[c m + j], resHist[c m + j] = the Ritz value and the relative residual of column j; sets[3 c ..] = {columns of W,
 * columns of P in the basis of the iteration before, restarts so far}; the calls a stop spared hold NaN / -1. *iterations = the loop's count where
 * it stopped converged, else -1 with status MFH_ERR_NOT_CONVERGED (every output written). *precondUsed as in mfh_modes_info */
mfh_status mfh_debug_lobpcg(mfh_ctx* ctx, int32_t pencil, double density, double loadFactor, int32_t freeBody, int32_t nev, double rtol, int32_t maxit,
                            int32_t m, const double* S0, int32_t nq, const double* Q, int32_t* blockSize, double* X, double* lambdaHist, double* resHist,
                            int32_t* sets, int32_t* iterations, int32_t* precondUsed);


/* ---------------------------------------------------------------- device-pointer building blocks
 * (multi-GPU driver: local kernels here, RCCL halo exchange / all-reduce in between)           */
/* y[0:dim*nOwnedDoF] = K x ; x has dim*nColDoF entries (owned then halo). fixed-variable mask NOT applied */
mfh_status mfh_dev_spmv(mfh_ctx* ctx, const double* x_dev, double* y_dev);
/* z = M^-1 r on the owned rows (block-Jacobi of the assembled K, fixed variables decoupled)     */
mfh_status mfh_dev_precond(mfh_ctx* ctx, const double* r_dev, double* z_dev);
/* Two-level preconditioner with CALLER-supplied aggregates (row-partitioned contexts; the aggregates are global,
 * the caller reduces over ranks): begin() takes, for every local node (owned then halo), its aggregate id in
 * [0,nAgg) and relPos = (position - aggregate centre)/H (3 doubles per node, z = 0 in 2D), and writes this
 * rank's Galerkin contribution Z^T K_ownedRows Z (m x m row-major, m = nAgg * (dim==3 ? 6 : 3)) into Ac_dev.
 * The fixed-variable mask must cover halo nodes as well. After summing Ac_dev over ranks, finish() inverts it on
 * the device. restrict: rc[m] = Z_owned^T r (to be summed over ranks); apply: z = D^-1 r + Z_owned (A_c^-1 rc). */
mfh_status mfh_tl_partitioned_begin(mfh_ctx* ctx, int32_t nAgg, const int32_t* aggOfNode, const double* relPos, double* Ac_dev);
mfh_status mfh_tl_partitioned_finish(mfh_ctx* ctx, const double* Ac_dev);
mfh_status mfh_dev_tl_restrict(mfh_ctx* ctx, const double* r_dev, double* rc_dev);
mfh_status mfh_dev_tl_apply(mfh_ctx* ctx, const double* r_dev, const double* rc_dev, double* z_dev);
/* fused vector updates of the distributed PCG over the owned rows; scalars are read from DEVICE memory (they are
 * results of all-reduces): x += (num/den) p, r -= (num/den) Ap ;  p = z + (num/den) p ;  out2 = {r.z, r.r} */
mfh_status mfh_dev_pcg_update_xr(mfh_ctx* ctx, const double* num_dev, const double* den_dev, const double* p_dev, const double* Ap_dev,
                                 double* x_dev, double* r_dev);
mfh_status mfh_dev_pcg_direction(mfh_ctx* ctx, const double* num_dev, const double* den_dev, const double* z_dev, double* p_dev);
mfh_status mfh_dev_dots(mfh_ctx* ctx, const double* r_dev, const double* z_dev, double* out2_dev);
/* r[fixed] = 0 */
mfh_status mfh_dev_mask_fixed(mfh_ctx* ctx, double* r_dev);
/* copy the fixed-variable values into u (u[fixed] = value) */
mfh_status mfh_dev_set_fixed_values(mfh_ctx* ctx, double* u_dev);
mfh_status mfh_dev_sync(mfh_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MESHFEM_HIP_EXTRAS_H */
