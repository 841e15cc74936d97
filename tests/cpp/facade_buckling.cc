// C++ drop-in test of include/MeshFEMHip/Buckling.hh on a linear tet Simulator clamped on its face z = min under unit axial compression
// sigma_zz = -1. Writes the load factors and Kg x; tests/test_cpp_buckling.py compares them with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nev, output file (f64 factors[nev], then
// (Kg x)[nDoF][3] for x = the node positions).
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
    try {
        using Sim = LinearElasticity::Simulator<3, 1>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1e-9}, {0, 0, 0}, true);
        std::vector<Real> sigma(T.size() * 6, 0.0);
        for (size_t e = 0; e < T.size(); ++e) sigma[6 * e + 2] = -1.0;           // zz
        setPrestress(sim, sigma);
        BucklingOptions opt;
        opt.maxit = 3000;
        mfh_buckling_info info{};
        const auto r = bucklingModes(sim, nev, opt, &info);
        if (r.first.size() != (size_t)nev || r.second.size() != (size_t)nev || r.second[0].size() != sim.numDoFs() || !info.converged || info.nBuckling != nev) {
            printf("FAILED: sizes / convergence\n");
            return 2;
        }
        Sim::VField x(sim.numDoFs());
        int64_t nElem, nNode;
        check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), &nElem, &nNode, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<Real> pos((size_t)nNode * 3);
        check(sim.ctx(), mfh_mesh_get_node_positions(sim.ctx(), pos.data()));
        for (size_t i = 0; i < x.size(); ++i) x[i] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const auto Gx = applyGeometricStiffness(sim, x);
        setPrestress(sim, std::vector<Real>());
        bool refused = false;
        try { applyGeometricStiffness(sim, x); } catch (const std::runtime_error &) { refused = true; }
        if (!refused) { printf("FAILED: Kg x without a prestress field\n"); return 2; }
        if (argc > 4) {
            FILE *f = fopen(argv[4], "wb");
            if (!f) { printf("cannot write %s\n", argv[4]); return 2; }
            fwrite(r.first.data(), sizeof(Real), r.first.size(), f);
            fwrite(&Gx[0][0], sizeof(Real), 3 * Gx.size(), f);
            fclose(f);
        }
        printf("factor[0] %.17g\n", r.first[0]);
        printf("buckling ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
