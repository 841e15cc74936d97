// The option knobs of a context (mfh_set_option / mfh_get_option, include/meshfem_hip.h): ONE table holds, per option, its name, the mfh_ctx member
// behind it, how a value is converted or rejected, which derived state a change makes stale, and whether the forced-degree-1 view follows it. The
// setter, the getter and the inheritance of a new view all walk this table; the members themselves are declared in table order in mfh_ctx.hh.
#include "mfh_ctx.hh"
#include <cstdio>
#include <cstring>

using namespace mfh;

namespace {
using namespace mfhi;

// ---- storage: a member of mfh_ctx, or (two options) an accessor to a value that lives elsewhere
struct Slot {
    enum Kind { INT, BOOL, REAL } kind;
    int mfh_ctx::*i = nullptr;
    bool mfh_ctx::*b = nullptr;
    double mfh_ctx::*d = nullptr;
    int *(*iat)(mfh_ctx *) = nullptr;      // accessors
    bool *(*bat)(mfh_ctx *) = nullptr;
    Slot(int mfh_ctx::*p) : kind(INT), i(p) {}
    Slot(bool mfh_ctx::*p) : kind(BOOL), b(p) {}
    Slot(double mfh_ctx::*p) : kind(REAL), d(p) {}
    Slot(int *(*f)(mfh_ctx *)) : kind(INT), iat(f) {}
    Slot(bool *(*f)(mfh_ctx *)) : kind(BOOL), bat(f) {}
    int &as_int(mfh_ctx *c) const { return iat ? *iat(c) : c->*i; }
    bool &as_bool(mfh_ctx *c) const { return bat ? *bat(c) : c->*b; }
    double load(const mfh_ctx *cc) const {
        mfh_ctx *c = const_cast<mfh_ctx *>(cc);      // (read only)
        switch (kind) {
        case INT: return (double)as_int(c);
        case BOOL: return as_bool(c) ? 1.0 : 0.0;
        default: return c->*d;
        }
    }
    void store(mfh_ctx *c, double v) const {
        switch (kind) {
        case INT: as_int(c) = (int)v; break;
        case BOOL: as_bool(c) = v != 0; break;
        default: c->*d = v; break;
        }
    }
};
bool *dist_profile_at(mfh_ctx *c) { return &c->dist.profile; }
int *vec_grid_cap_at(mfh_ctx *) { return &k::g_vecGridCap; }      // process-wide

// ---- conversion of the caller's double into the stored value (lo / hi: the row's bounds)
enum Conv {
    C_BOOL,          // value != 0 (an int member then holds 0 / 1)
    C_INT,           // (int)value
    C_INT_FROM,      // max(lo, (int)value)
    C_INT_IN,        // (int)value clamped to [lo, hi]
    C_TRI,           // < 0 -> -1, non-zero -> 1, else 0
    C_REAL_OPEN,     // rejected outside the open interval (lo, hi)
    C_REAL_FROM,     // rejected below lo
    C_REAL_FLOOR,    // max(value, lo)
    C_MASK3,         // (int)value & 7
    C_STORAGE,       // -1, 0 or 1, anything else rejected
    C_POSITIVE,      // positive and finite, anything else rejected
};

// ---- effect: derived state that a change of the option makes stale
enum Effect : unsigned {
    E_MULTIGRID = 1u << 0,       // the multigrid hierarchy
    E_TWO_LEVEL = 1u << 1,       // the two-level preconditioner
    E_SYMBOLIC = 1u << 2,        // the symbolic phase and everything built on it (invalidate_symbolic)
    E_CLUSTER = 1u << 3,         // element blocks of the cluster operator, and the verdict that they do not fit this mesh
    E_CLUSTER_UNFIT = 1u << 4,   // that verdict only
    E_PAIRS = 1u << 5,           // (element, node) pair lists of the matrix-free operator
    E_SAMPLER = 1u << 6,         // cell grids of the field sampler
    E_PLACEMENT = 1u << 7,       // the placement trials run again
    E_STRETCH = 1u << 8,         // MFH_PRECOND_AUTO looks at the mesh again
};
void apply_effects(mfh_ctx *c, unsigned e) {
    if (e & E_MULTIGRID) c->mg.valid = false;
    if (e & E_TWO_LEVEL) c->tl.valid = false;
    if (e & E_SYMBOLIC) invalidate_symbolic(c);
    if (e & E_CLUSTER) invalidate_cluster(c);
    if (e & E_CLUSTER_UNFIT) c->mfClusterUnfit = false;
    if (e & E_PAIRS) c->mfValid = false;
    if (e & E_SAMPLER) sampler_drop(c);
    if (e & E_PLACEMENT) c->placementGen = -1;
    if (e & E_STRETCH) c->autoStretch = -1.0;
}

// ---- the forced-degree-1 view (mfh_ctx::p1) and its context's options
enum View {
    V_FOLLOWS,       // a new view starts from its context's value, an existing one gets every call forwarded
    V_FORWARDED,     // forwarded only: mfh_set_operator_degree sets it on a new view through mfh_set_option (scratch of the view's own)
    V_OWN,           // the view keeps its own value (it always multiplies by its assembled matrix)
};

// ---- the two options a row cannot express
void set_deterministic(mfh_ctx *c, double value) {
    const bool on = value != 0;
    if (on && !c->detPartials.p) {
        require_device(c);
        MFH_HIP(hipSetDevice(c->device));
        c->detPartials.alloc((size_t)8 + (size_t)4096 * 4);      // header + 4 096 workgroups x 4 partials (launches with global sums use at most that many
                                                                 // workgroups in this mode: the one-workgroup second stage reads 16 partials per lane and sum)
        c->detPartials.zero(c->stream);
        c->detCounter.alloc(64);
        c->detCounter.zero(c->stream);
        MFH_HIP(hipStreamSynchronize(c->stream));
    }
    if (on != c->deterministic) { c->deterministic = on; invalidate_matrix(c); destroy_multigrid(c); c->tl.valid = false; invalidate_cluster(c); }   // (the block size of the cluster operator depends on it)
}
void set_batch_rhs(mfh_ctx *c, double value) {       // the element blocks are stale only when the value changes
    if (c->batchRhs != (value != 0)) invalidate_cluster(c);
    c->batchRhs = value != 0;
}

struct Row {
    const char *name;
    Slot slot;
    Conv conv;
    double lo, hi;
    unsigned effects;
    View view = V_FOLLOWS;
    void (*custom)(mfh_ctx *, double) = nullptr;      // replaces conversion, store and effects
};

const double NA = 0;      // a bound the conversion does not read
using X = mfh_ctx;
const Row TABLE[] = {
    // ---- context, mesh
    {"keep_host_symbolic", &X::keepHostSymbolic, C_BOOL, NA, NA, 0},
    {"xcd_swizzle", &X::xcdSwizzle, C_INT_FROM, 0, NA, 0},            // 1: contiguous eighths; G > 1: runs of G items per XCD
    {"reembed", &X::alwaysReembed, C_BOOL, NA, NA, 0},
    {"deterministic", &X::deterministic, C_BOOL, NA, NA, 0, V_FORWARDED, set_deterministic},
    {"periodic_ignore_mismatch", &X::periodicIgnoreMismatch, C_BOOL, NA, NA, 0},
    {"periodic_ignore_dims", &X::periodicIgnoreDims, C_MASK3, NA, NA, 0},
    {"topology_device", &X::topologyDevice, C_BOOL, NA, NA, 0},
    {"sampler_cell_scale", &X::samplerCellScale, C_POSITIVE, NA, NA, E_SAMPLER},
    // ---- symbolic phase, assembly
    {"symbolic_device", &X::symbolicDevice, C_BOOL, NA, NA, E_SYMBOLIC},
    {"matrix_storage", &X::matrixStorage, C_STORAGE, NA, NA, 0},
    {"chunk_slots", &X::chunkSlots, C_INT, NA, NA, E_SYMBOLIC},
    {"contrib_order", &X::contribOrder, C_INT, NA, NA, E_SYMBOLIC},
    {"asm_packed_codes", &X::asmPackedCodes, C_BOOL, NA, NA, E_SYMBOLIC},
    {"asm_chunk_order", &X::asmChunkOrder, C_INT, NA, NA, 0},
    {"placement_trials", &X::placementTrials, C_INT_IN, 0, 8, E_PLACEMENT},
    // ---- matrix-free operator
    {"matrix_free", &X::matrixFree, C_TRI, NA, NA, 0, V_OWN},       // K x without reading the assembled K (k_spmv_mf)
    {"matrix_free_mode", &X::mfMode, C_INT, NA, NA, E_CLUSTER_UNFIT},
    {"mf_block_elems", &X::mfBlockElems, C_INT, NA, NA, E_CLUSTER},
    {"mf_reorder", &X::mfReorder, C_BOOL, NA, NA, E_CLUSTER},
    {"mf_xcd_group", &X::mfXcdGroup, C_INT_FROM, 0, NA, 0},
    {"mf_lane_stride", &X::mfLaneStride, C_INT_FROM, 1, NA, 0},
    {"mf_geometry_from_vertices", &X::mfGeoFromVerts, C_BOOL, NA, NA, 0},
    {"mf_chunk_rows", &X::mfChunkRows, C_INT_IN, 16, 4096, E_PAIRS},
    {"mf_chunk_pairs", &X::mfChunkPairs, C_INT_FROM, 256, NA, E_PAIRS},
    // ---- vector kernels
    {"vec_grid_cap", Slot(vec_grid_cap_at), C_INT_FROM, 256, NA, 0},
    {"dyn_grid_cap", &X::dynGridCap, C_INT_IN, 1, 2048, 0},
    {"harmonic_two_pass", &X::harmTwoPass, C_BOOL, NA, NA, 0},
    // ---- PCG
    {"check_every", &X::checkEvery, C_INT_FROM, 1, NA, 0},
    {"pcg_graph", &X::useGraph, C_BOOL, NA, NA, 0},
    {"refine", &X::refine, C_BOOL, NA, NA, 0},
    {"solve_homogeneous", &X::solveHomogeneous, C_BOOL, NA, NA, 0},
    {"pcg_variant", &X::pcgVariant, C_TRI, NA, NA, 0},
    {"dist_pcg_variant", &X::distPcgVariant, C_BOOL, NA, NA, 0},
    {"dist_profile", Slot(dist_profile_at), C_BOOL, NA, NA, 0},
    {"batch_rhs", &X::batchRhs, C_BOOL, NA, NA, 0, V_FOLLOWS, set_batch_rhs},
    {"auto_stretch_max", &X::autoStretchMax, C_REAL_FLOOR, 1, NA, E_STRETCH},
    // ---- two-level preconditioner
    {"agg_nodes", &X::aggNodes, C_INT, NA, NA, E_TWO_LEVEL},
    {"tl_rap_agg", &X::tlRapAgg, C_BOOL, NA, NA, E_TWO_LEVEL},
    {"tl_device_aggregates", &X::tlDeviceAggregates, C_BOOL, NA, NA, E_TWO_LEVEL},
    {"tl_probe", &X::tlProbe, C_BOOL, NA, NA, E_TWO_LEVEL},
    {"tl_host_inverse", &X::tlHostInverse, C_BOOL, NA, NA, E_TWO_LEVEL},
    // ---- multigrid preconditioner
    {"mg_steps_fine", &X::mgSteps0, C_INT_FROM, 1, NA, 0},
    {"mg_steps_coarse", &X::mgSteps1, C_INT_FROM, 1, NA, 0},
    {"mg_ratio_fine", &X::mgRatio0, C_REAL_OPEN, 0, 1, 0},
    {"mg_ratio_coarse", &X::mgRatio1, C_REAL_OPEN, 0, 1, 0},
    {"mg_coarse_cycles", &X::mgCoarseCycles, C_INT_FROM, 1, NA, 0},
    {"mg_eig_margin", &X::mgEigMargin, C_REAL_FROM, 1, NA, E_MULTIGRID},
    {"mg_agg_target", &X::mgAggTarget, C_INT_FROM, 0, NA, E_MULTIGRID},
    {"mg_dense_max", &X::mgDenseMax, C_INT_FROM, 8, NA, E_MULTIGRID},
    {"mg_coarse_fp32", &X::mgCoarseFp32, C_BOOL, NA, NA, E_MULTIGRID},
    {"mg_over_correction", &X::mgOverCorrection, C_REAL_OPEN, 0, 4, 0},
    {"mg_steps_agg", &X::mgStepsAgg, C_INT_FROM, 1, NA, 0},
    {"mg_ratio_agg", &X::mgRatioAgg, C_REAL_OPEN, 0, 1, 0},
    {"mg_replicate_max", &X::mgReplicateMax, C_INT_FROM, 0, NA, E_MULTIGRID},
    {"mg_anisotropic_bins", &X::mgAnisotropicBins, C_BOOL, NA, NA, E_MULTIGRID},
    {"mg_agg_nodes", &X::mgAggNodes, C_INT_FROM, 0, NA, E_MULTIGRID},
    {"mg_dinv_fp32", &X::mgDinvFp32, C_BOOL, NA, NA, 0},
    {"mg_fuse", &X::mgFuse, C_BOOL, NA, NA, 0},
    {"mg_batch", &X::mgBatch, C_BOOL, NA, NA, 0},
};

const Row &find_row(const char *key) {
    for (const Row &r : TABLE)
        if (!strcmp(r.name, key)) return r;
    throw Error(MFH_ERR_INVALID, std::string("unknown option ") + key);
}

std::string bound(double v) { char b[32]; snprintf(b, sizeof b, "%g", v); return b; }

// the value to store, or an error that names the option and what it admits
double convert(const Row &r, double v) {
    const std::string name(r.name);
    switch (r.conv) {
    case C_BOOL: return v != 0 ? 1 : 0;
    case C_INT: return (int)v;
    case C_INT_FROM: return std::max((int)r.lo, (int)v);
    case C_INT_IN: return std::max((int)r.lo, std::min((int)r.hi, (int)v));
    case C_TRI: return v < 0 ? -1 : (v != 0 ? 1 : 0);
    case C_REAL_OPEN:
        if (!(v > r.lo && v < r.hi)) throw Error(MFH_ERR_INVALID, name + " must lie in (" + bound(r.lo) + ", " + bound(r.hi) + ")");
        return v;
    case C_REAL_FROM:
        if (!(v >= r.lo)) throw Error(MFH_ERR_INVALID, name + " must be >= " + bound(r.lo));
        return v;
    case C_REAL_FLOOR: return v > r.lo ? v : r.lo;
    case C_MASK3: return (int)v & 7;
    case C_STORAGE:
        if (!(v == 0 || v == 1 || v == -1)) throw Error(MFH_ERR_INVALID, name + ": 0 = both triangles, 1 = blocks (r, c >= r) only, -1 = automatic");
        return v;
    case C_POSITIVE:
        if (!(v > 0 && std::isfinite(v))) throw Error(MFH_ERR_INVALID, name + " must be positive and finite");
        return v;
    }
    return v;
}
}   // namespace

namespace mfhi {
// a new forced-degree-1 view starts from the options of its context: what mfh_set_option would have forwarded had the view existed all along
void inherit_options(mfh_ctx *view, const mfh_ctx *parent) {
    for (const Row &r : TABLE)
        if (r.view == V_FOLLOWS) r.slot.store(view, r.slot.load(parent));
}
}   // namespace mfhi

extern "C" {

mfh_status mfh_set_option(mfh_ctx *c, const char *key, double value) {
    MFH_TRY(c)
    require(c && key, MFH_ERR_INVALID, "null argument");
    const Row &r = find_row(key);
    if (r.custom) r.custom(c, value);
    else {
        r.slot.store(c, convert(r, value));
        apply_effects(c, r.effects);
    }
    refresh_storage_rule(c);   // matrix_storage, matrix_free, tl_probe, tl_rap_agg decide the storage of K
    if (c->p1 && r.view != V_OWN) {              // the forced-degree-1 view follows its context's options
        const mfh_status st = mfh_set_option(c->p1, key, value);
        if (st != MFH_OK) throw Error(st, c->p1->err);
    }
    MFH_CATCH(c)
}

// the context's own value (the view is not followed); bool options read 0 / 1
mfh_status mfh_get_option(const mfh_ctx *c, const char *key, double *value) {
    if (!c || !key || !value) return MFH_ERR_INVALID;
    try {
        *value = find_row(key).slot.load(c);
    } catch (const Error &e) {
        const_cast<mfh_ctx *>(c)->err = e.what();      // the one read-only entry point that reports a text: the unknown name, as the setter does
        return e.code;
    } catch (...) { return MFH_ERR_INVALID; }
    return MFH_OK;
}

} // extern "C"
