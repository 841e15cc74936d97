// C++ drop-in test of include/MeshFEMHip/DifferentialOperators.hh: the operators of a quadratic Simulator at their own degree and at
// forced degree 1, compared with triplet files the CPU oracle wrote (TripletMatrix::dumpBinary format).
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), directory with the expected files.
#include <MeshFEMHip/DifferentialOperators.hh>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

static bool readTriplets(const std::string &path, TripletMatrix &T) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint64_t n = 0;
    bool ok = fread(&n, sizeof(n), 1, f) == 1;
    std::vector<uint64_t> i(n), j(n);
    std::vector<Real> v(n);
    ok = ok && fread(i.data(), 8, n, f) == n && fread(j.data(), 8, n, f) == n && fread(v.data(), 8, n, f) == n;
    fclose(f);
    T.nz.resize(n);
    for (uint64_t k = 0; k < n; ++k) T.nz[k] = Triplet{(size_t)i[k], (size_t)j[k], v[k]};
    return ok;
}

// entry for entry: same (i, j) in the same order, values to tol * max |ref|
static bool same(const char *what, const TripletMatrix &A, const TripletMatrix &R, Real tol) {
    Real mx = 0, err = 0;
    for (auto &t : R.nz) mx = std::max(mx, std::fabs(t.v));
    bool pattern = A.nz.size() == R.nz.size();
    for (size_t k = 0; pattern && k < A.nz.size(); ++k) {
        pattern = A.nz[k].i == R.nz[k].i && A.nz[k].j == R.nz[k].j;
        err = std::max(err, std::fabs(A.nz[k].v - R.nz[k].v));
    }
    printf("%-28s nnz %zu (expected %zu) pattern %s max err %.3e (max |ref| %.3e)\n", what, A.nz.size(), R.nz.size(), pattern ? "identical" : "DIFFERENT", err, mx);
    return pattern && err <= tol * mx;
}

int main(int argc, char **argv) {
    const int device = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<std::array<Real, 3>> V;
    std::vector<std::array<int32_t, 4>> T;
    std::string dir = argc > 3 ? argv[3] : ".";
    if (argc > 2) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
        int64_t nv = 0, ne = 0;
        bool ok = fread(&nv, 8, 1, f) == 1 && fread(&ne, 8, 1, f) == 1;
        V.resize((size_t)nv); T.resize((size_t)ne);
        ok = ok && fread(V.data(), sizeof(V[0]), (size_t)nv, f) == (size_t)nv && fread(T.data(), sizeof(T[0]), (size_t)ne, f) == (size_t)ne;
        fclose(f);
        if (!ok) { printf("truncated mesh file\n"); return 2; }
    } else {                                       // one tetrahedron: enough to reach the device (or fail to)
        V = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        T = {{0, 1, 2, 3}};
    }
    try {
        LinearElasticity::Simulator<3, 2> sim(T, V, device);
        const size_t nVert = V.size();
        TripletMatrix Mv1 = MassMatrix::construct_vector_valued<1>(sim), M1 = MassMatrix::construct<1>(sim), L1 = Laplacian::construct<1>(sim);
        TripletMatrix Ml1 = MassMatrix::construct_vector_valued<1>(sim, true), L2 = Laplacian::construct(sim), Lraw = Laplacian::construct<1>(sim.ctx());
        if (Mv1.m != 3 * nVert || M1.m != nVert || L1.m != nVert || Ml1.nz.size() != 3 * nVert || L2.m != sim.numNodes() || Lraw.nz.size() != L1.nz.size()) {
            printf("FAILED: sizes\n");
            return 2;
        }
        if (argc > 3) {
            TripletMatrix R;
            const Real tol = 1e-13;
            bool ok = true;
            ok = readTriplets(dir + "/mass_vector_p1.bin", R) && same("construct_vector_valued<1>", Mv1, R, tol) && ok;
            ok = readTriplets(dir + "/mass_p1.bin", R) && same("MassMatrix::construct<1>", M1, R, tol) && ok;
            ok = readTriplets(dir + "/laplacian_p1.bin", R) && same("Laplacian::construct<1>", L1, R, tol) && ok;
            ok = readTriplets(dir + "/mass_vector_p1_lumped.bin", R) && same("vector_valued<1> lumped", Ml1, R, 1e-14) && ok;
            if (!ok) { printf("FAILED: operators differ from the oracle\n"); return 2; }
        }
        // the Simulator is handed back with elasticity selected and the full degree in force
        int64_t rows = 0;
        check(sim.ctx(), mfh_assemble(sim.ctx(), MFH_ASSEMBLE_GATHER));
        check(sim.ctx(), mfh_matrix_info(sim.ctx(), &rows, nullptr, nullptr));
        if ((size_t)rows != sim.numNodes()) { printf("FAILED: full-degree pattern not restored\n"); return 2; }
        printf("differential operators ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
