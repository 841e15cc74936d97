// C++ drop-in test of prestressedModes / applyTangentStiffness (include/MeshFEMHip/Buckling.hh) on a linear tet Simulator clamped on its face
// z = min under unit axial compression sigma_zz = -1. Writes the eigenvalues at two load factors (the second started from the shapes of the
// first) and (K + s Kg) x; tests/test_cpp_prestressed_modes.py compares them with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nev, s1, s2, output file (f64 lambda(s1)[nev],
// lambda(s2)[nev], then ((K + s1 Kg) x)[nDoF][3] for x = the node positions).
#include <MeshFEMHip/Buckling.hh>
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
    const Real s1 = argc > 4 ? atof(argv[4]) : 0.0, s2 = argc > 5 ? atof(argv[5]) : 0.0;
    try {
        using Sim = LinearElasticity::Simulator<3, 1>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1e-9}, {0, 0, 0}, true);
        std::vector<Real> sigma(T.size() * 6, 0.0);
        for (size_t e = 0; e < T.size(); ++e) sigma[6 * e + 2] = -1.0;           // zz
        setPrestress(sim, sigma);
        ModesOptions opt;
        opt.maxit = 3000;
        mfh_modes_info info1{}, info2{};
        const auto r1 = prestressedModes(sim, nev, s1, 1.0, opt, &info1);
        const auto r2 = prestressedModes(sim, nev, s2, 1.0, opt, &info2, r1.second);
        if (r1.first.size() != (size_t)nev || r2.second.size() != (size_t)nev || r2.second[0].size() != sim.numDoFs() || !info1.converged || !info2.converged) {
            printf("FAILED: sizes / convergence\n");
            return 2;
        }
        Sim::VField x(sim.numDoFs());
        int64_t nElem, nNode;
        check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), &nElem, &nNode, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<Real> pos((size_t)nNode * 3);
        check(sim.ctx(), mfh_mesh_get_node_positions(sim.ctx(), pos.data()));
        for (size_t i = 0; i < x.size(); ++i) x[i] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const auto Tx = applyTangentStiffness(sim, s1, x);
        bool refused = false;
        try { prestressedModes(sim, nev, s1, 1.0, opt, nullptr, std::vector<Sim::VField>(1, x)); } catch (const std::runtime_error &) { refused = true; }
        if (!refused && nev != 1) { printf("FAILED: a start block of the wrong size\n"); return 2; }
        setPrestress(sim, std::vector<Real>());
        refused = false;
        try { applyTangentStiffness(sim, s1, x); } catch (const std::runtime_error &) { refused = true; }
        if (!refused) { printf("FAILED: (K + s Kg) x without a prestress field\n"); return 2; }
        if (argc > 6) {
            FILE *f = fopen(argv[6], "wb");
            if (!f) { printf("cannot write %s\n", argv[6]); return 2; }
            fwrite(r1.first.data(), sizeof(Real), r1.first.size(), f);
            fwrite(r2.first.data(), sizeof(Real), r2.first.size(), f);
            fwrite(&Tx[0][0], sizeof(Real), 3 * Tx.size(), f);
            fclose(f);
        }
        printf("lambda[0] %.17g -> %.17g, iterations %d -> %d\n", r1.first[0], r2.first[0], info1.iterations, info2.iterations);
        printf("prestressed modes ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
