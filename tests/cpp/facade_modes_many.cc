// C++ drop-in test of the mfh_modes_many overload of include/MeshFEMHip/Eigensolver.hh on a quadratic tet Simulator clamped on its face x = min:
// nev modes in batches of `batch`, then nMore further ones in the complement of the first (the continuation through `locked`);
// tests/test_cpp_modes_many.py compares with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nev, batch, nMore, density, output file
// (f64 lambda[nev + nMore], then f64 modes[nev + nMore][nDoF][3]).
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
    const int nev = argc > 3 ? atoi(argv[3]) : 2, batch = argc > 4 ? atoi(argv[4]) : 0, nMore = argc > 5 ? atoi(argv[5]) : 0;
    const Real density = argc > 6 ? atof(argv[6]) : 1.0;
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        ManyModesOptions opt;
        opt.batch = batch;
        mfh_modes_many_info info{};
        auto r = vibrationalModes(sim, nev, density, false, opt, {}, &info);
        if (r.first.size() != (size_t)nev || r.second.size() != (size_t)nev || r.second[0].size() != sim.numDoFs() || !info.converged || info.nFound != nev) {
            printf("FAILED: sizes / convergence\n");
            return 2;
        }
        printf("lambda[0] %.17g after %d iterations in %d batches\n", r.first[0], (int)info.iterations, (int)info.batches);
        if (nMore > 0) {
            mfh_modes_many_info more{};
            const auto r2 = vibrationalModes(sim, nMore, density, false, opt, r.second, &more);
            if (r2.first.size() != (size_t)nMore || !more.converged) { printf("FAILED: continuation\n"); return 2; }
            r.first.insert(r.first.end(), r2.first.begin(), r2.first.end());
            r.second.insert(r.second.end(), r2.second.begin(), r2.second.end());
        }
        if (argc > 7) {
            FILE *f = fopen(argv[7], "wb");
            if (!f) { printf("cannot write %s\n", argv[7]); return 2; }
            fwrite(r.first.data(), sizeof(Real), r.first.size(), f);
            for (const auto &m : r.second) fwrite(&m[0][0], sizeof(Real), 3 * m.size(), f);
            fclose(f);
        }
        printf("modes ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
