// C++ drop-in test of include/MeshFEMHip/Eigensolver.hh on a quadratic tet Simulator clamped on its face x = min: writes the eigenvalues that
// vibrationalModes returns; tests/test_cpp_modes.py compares them with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nev, density, output file (f64 lambda[nev], then
// f64 modes[nev][nDoF][3]).
#include <MeshFEMHip/Eigensolver.hh>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

int main(int argc, char **argv) {
    const int device = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<std::array<Real, 3>> V = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // one tetrahedron: enough to reach the device (or fail to)
    std::vector<std::array<int32_t, 4>> T = {{0, 1, 2, 3}};
    if (argc > 2) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
        int64_t nv = 0, ne = 0;
        bool ok = fread(&nv, 8, 1, f) == 1 && fread(&ne, 8, 1, f) == 1;
        V.resize((size_t)nv); T.resize((size_t)ne);
        ok = ok && fread(V.data(), sizeof(V[0]), (size_t)nv, f) == (size_t)nv && fread(T.data(), sizeof(T[0]), (size_t)ne, f) == (size_t)ne;
        fclose(f);
        if (!ok) { printf("truncated mesh file\n"); return 2; }
    }
    const int nev = argc > 3 ? atoi(argv[3]) : 2;
    const Real density = argc > 4 ? atof(argv[4]) : 1.0;
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        // clamp: every boundary node on the face x = min of the bounding box (relative box coordinates)
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        mfh_modes_info info{};
        const auto r = vibrationalModes(sim, nev, density, false, ModesOptions(), &info);
        if (r.first.size() != (size_t)nev || r.second.size() != (size_t)nev || r.second[0].size() != sim.numDoFs() || !info.converged) {
            printf("FAILED: sizes / convergence\n");
            return 2;
        }
        if (argc > 5) {
            FILE *f = fopen(argv[5], "wb");
            if (!f) { printf("cannot write %s\n", argv[5]); return 2; }
            fwrite(r.first.data(), sizeof(Real), r.first.size(), f);
            for (const auto &m : r.second) fwrite(&m[0][0], sizeof(Real), 3 * m.size(), f);
            fclose(f);
        }
        printf("lambda[0] %.17g after %d iterations, block %d\n", r.first[0], (int)info.iterations, (int)info.blockSize);
        printf("modes ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
